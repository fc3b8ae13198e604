// so100_dr.hip - the physical part of domain randomisation and each env's actuator record, drawn on the device (C-ABI
// so100_dr_sample).  One thread per env.  Every draw is so100_views.hip's counter-based hash of (seed,
// global env id, episode, field number), so a record does not depend on the sharding, on the masks or on launch order,
// and per-episode resampling needs no host round trip: the launch after a step rewrites the dr_params rows of the envs
// that just finished, which the unchanged step kernel reads at the start of its next call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"

namespace so100 {

struct DrSampleArgs {
  so100_dr_ranges r;
  const uint32_t* episode;              // [n] or null = 0
  const uint8_t* mask_a;                // [n] or null
  const uint8_t* mask_b;                // [n] or null; both null = every env
  float* dr_params;                     // [n,4] or null: columns 0 and 1 are written
  float* act_params;                    // [n,4] or null
  int n, env_offset;
};

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the top 24 bits of so100_views.hip's hash: uniform() there is this * 2^-24
__device__ __forceinline__ uint32_t hash24(uint64_t seed, uint64_t id, uint32_t episode, uint32_t field) {
  const uint64_t k = splitmix64(seed ^ (id * 0x100000001B3ull) ^ ((uint64_t)field * 0xD1B54A32D192ED03ull));
  return (uint32_t)(splitmix64(k + episode) >> 40);
}

// a value from [lo, hi]; lo for a range of zero width
__device__ __forceinline__ float draw(const float* r, uint32_t h24) {
  const float u = (float)h24 * (1.f / 16777216.f);
  return fminf(fmaxf(r[0] + (r[1] - r[0]) * u, r[0]), r[1]);
}

}  // namespace

__global__ void __launch_bounds__(256) so100_dr_sample_kernel(DrSampleArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  if (a.mask_a || a.mask_b) {
    const bool on = (a.mask_a && a.mask_a[i]) || (a.mask_b && a.mask_b[i]);
    if (!on) return;
  }
  const uint64_t seed = a.r.seed, id = (uint64_t)(a.env_offset + i);
  const uint32_t ep = a.episode ? a.episode[i] : 0u;
  if (a.dr_params) {
    // columns 0 and 1: the sigma and the spare column behind them stay what they are
    a.dr_params[(size_t)i * 4 + 0] = draw(a.r.mass, hash24(seed, id, ep, 1));
    a.dr_params[(size_t)i * 4 + 1] = draw(a.r.friction, hash24(seed, id, ep, 2));
  }
  if (a.act_params) {
    const uint64_t span = (uint64_t)(a.r.delay[1] - a.r.delay[0] + 1);
    const int d = a.r.delay[0] + (int)(((uint64_t)hash24(seed, id, ep, 4) * span) >> 24);
    float* p = a.act_params + (size_t)i * 4;          // (plain float stores: no alignment is asked of the caller)
    p[0] = (float)d;
    p[1] = draw(a.r.smoothing, hash24(seed, id, ep, 5));
    p[2] = draw(a.r.rate, hash24(seed, id, ep, 6));
    p[3] = 0.f;
  }
}

hipError_t launch_dr_sample(const so100_dr_ranges& r, const uint32_t* episode, const uint8_t* mask_a,
                            const uint8_t* mask_b, float* dr_params, float* act_params, int n, int env_offset,
                            hipStream_t s) {
  const DrSampleArgs a{r, episode, mask_a, mask_b, dr_params, act_params, n, env_offset};
  hipLaunchKernelGGL(so100_dr_sample_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
