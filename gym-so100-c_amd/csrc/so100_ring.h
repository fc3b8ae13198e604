// so100_ring.h - what the two replay buffers (so100_her.hip, so100_replay.hip) share on the device: the keyed 64-bit draw
// of a sample call and the ring arithmetic.  include/so100.h states the formulas.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace so100 {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the 64-bit draw of (seed, sample call, batch element, field): so100_views_sample's key with the call in the
// episode's place
__device__ __forceinline__ uint64_t her_draw(uint64_t seed, uint64_t call, uint64_t i, uint32_t field) {
  const uint64_t k = splitmix64(seed ^ (i * 0x100000001B3ull) ^ ((uint64_t)field * 0xD1B54A32D192ED03ull));
  return splitmix64(k + call);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (a + b) mod T and (a - b) mod T for a in [0, T), b in [0, T]
__device__ __forceinline__ int add_mod(int a, int b, int T) {
  const int s = a - (T - b);                             // (not a + b - T: a + b can pass 2^31)
  return s >= 0 ? s : s + T;
}
__device__ __forceinline__ int sub_mod(int a, int b, int T) {
  const int s = a - b;
  return s >= 0 ? s : s + T;
}

// the one-workgroup inclusive scan of so100_her.hip over count[0..n), each clamped into [0, cap]: prefix[e] for e < n,
// prefix[n] = the total
hipError_t launch_count_scan(int n, int cap, const int32_t* count, int32_t* prefix, hipStream_t s);

}  // namespace so100
