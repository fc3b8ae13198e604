// so100_her.hip - a hindsight replay buffer for the GoalEnv on the device (C-ABI so100_her_push, so100_her_discard,
// so100_her_scan, so100_her_sample; include/so100.h states the rules, DESIGN.md §3.11 the reasons).  New launches beside
// the untouched step kernel: a push reads what the step wrote and appends one transition per env to that env's ring, a
// sample draws uniformly among the transitions of closed episodes and relabels a share of the rows with a goal the same
// episode achieved later.  No atomics, no wait inside a launch, plain vector stores; every result is a function of the
// inputs alone.
//
// Layout.  The ring is slot-major, [T][n][...]: the rows one push writes (one per env, each env at its own cursor) are
// contiguous wherever neighbouring envs' cursors agree, which is every env until episodes of different lengths pull them
// apart, and within one slot's n rows after that.
//
// Push and discard.  16 lanes per env (a row of 15 floats and one lane for the scalars), 16 envs per 256-thread
// workgroup: lane c copies column c of obs and next_obs, lanes 0..2 the goal, lanes < action_dim the command, lane 15
// writes reward, terminated, offset, length and the metadata.  The 16 lanes of an env sit in one wave and compute the
// same decisions from the same metadata loads (one request per env: the lanes' addresses are equal), which all precede
// lane 15's stores in program order.
//
// Scan.  One workgroup of kScanThreads = 1024 threads (16 waves) walks the counts in tiles of kScanTile = 4096: a thread
// takes 4 consecutive counts, a wave scans its 64 sums by __shfl_up, the 16 wave totals go through LDS, and the running
// carry is the same number in every thread.  65,536 envs are 16 passes.  One workgroup, so the order of the additions is
// fixed (they are integers: the result would be exact in any order).
//
// Sample.  16 lanes per batch element, as in the push: every lane of the group makes the same two draws and the same
// binary search over the prefix sums (equal addresses: one request per group), then copies its column.  The reads are
// random rows of the ring (60 contiguous bytes each), the writes contiguous rows of the batch.  Every index that came out
// of memory is clamped before it is used as an address: corrupted metadata gives a wrong sample, never a fault.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"
#include "so100_device.h"
#include "so100_goal.h"
#include "so100_ring.h"

namespace so100 {

constexpr int kHerThreads = 256;
constexpr int kHerLanes = 16;                            // lanes per env (push) / per batch element (sample)
constexpr int kHerRows = kHerThreads / kHerLanes;        // envs / batch elements per workgroup
constexpr int kHerObs = SO100_NOBS;
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;                            // consecutive counts per thread and pass
constexpr int kScanTile = kScanThreads * kScanItems;
static_assert(kHerObs < kHerLanes, "a row's columns and one scalar lane fit the lanes of an env");
static_assert(SO100_HER_MAX_ACTION <= kHerLanes, "one lane per command component");
static_assert(64 % kHerLanes == 0, "the lanes of an env share a wave");

int her_scan_group() { return kScanThreads; }
int her_scan_tile() { return kScanTile; }

namespace {

struct HerMeta {
  int lo, count, open;
};

// the metadata of env e, clamped: lo in [0, T), count in [0, T], open in [0, T - count]
__device__ __forceinline__ HerMeta her_meta(const int32_t* meta, int n, int T, int e) {
  HerMeta m;
  m.lo = clampi(meta[e], 0, T - 1);
  m.count = clampi(meta[(size_t)n + e], 0, T);
  m.open = clampi(meta[2 * (size_t)n + e], 0, T - m.count);
  return m;
}

}  // namespace

__global__ __launch_bounds__(kHerThreads) void so100_her_push_kernel(so100_her h, so100_her_step s) {
  const int c = (int)threadIdx.x & (kHerLanes - 1);
  const long long el = (long long)blockIdx.x * kHerRows + ((int)threadIdx.x >> 4);
  if (el >= h.n) return;
  const int e = (int)el, n = h.n, T = h.T, A = h.action_dim;
  HerMeta m = her_meta(h.meta, n, T, e);
  // 1. a full ring: the oldest closed episode goes whole
  if (m.count + m.open == T) {
    if (m.count > 0) {
      const int L = clampi(h.length[(size_t)m.lo * n + e], 1, m.count);
      m.lo = add_mod(m.lo, L, T);
      m.count -= L;
    } else {
      m.open = 0;
    }
  }
  // 2. the transition at the cursor
  const int cur = add_mod(add_mod(m.lo, m.count, T), m.open, T);
  const size_t row = (size_t)cur * n + e;                // < T n < 2^31
  const bool fin = s.terminated[e] != 0 || s.truncated[e] != 0;
  const bool erase = (s.diverged != nullptr && s.diverged[e] != 0) || (s.discard != nullptr && s.discard[e] != 0);
  if (c < kHerObs) {
    const float before = s.prev_obs[(size_t)e * kHerObs + c];
    const float now = s.obs[(size_t)e * kHerObs + c];
    const float next = fin ? s.final_obs[(size_t)e * kHerObs + c] : now;
    h.obs[row * kHerObs + c] = before;
    h.next_obs[row * kHerObs + c] = next;
    h.stage_obs[(size_t)e * kHerObs + c] = now;          // 4. the next transition's "before" row
  }
  if (c < 3) {
    const float g = s.prev_goal[(size_t)e * 3 + c];
    const float g_now = s.goal[(size_t)e * 3 + c];
    h.goal[row * 3 + c] = g;
    h.stage_goal[(size_t)e * 3 + c] = g_now;
  }
  if (c < A) h.action[row * A + c] = s.action[(size_t)e * A + c];
  if (c != kHerLanes - 1) return;
  h.reward[row] = s.reward[e];
  h.terminated[row] = s.terminated[e] != 0 ? 1 : 0;
  h.offset[row] = m.open;
  m.open += 1;
  // 3. erase, close or go on
  if (erase) {
    m.open = 0;
  } else if (fin) {
    const int first = sub_mod(cur, m.open - 1, T);
    h.length[(size_t)first * n + e] = m.open;
    m.count += m.open;
    m.open = 0;
  }
  h.meta[e] = m.lo;
  h.meta[(size_t)n + e] = m.count;
  h.meta[2 * (size_t)n + e] = m.open;
}

__global__ __launch_bounds__(kHerThreads) void so100_her_discard_kernel(so100_her h, const uint8_t* __restrict__ mask,
                                                                        const float* __restrict__ obs,
                                                                        const float* __restrict__ goal) {
  const int c = (int)threadIdx.x & (kHerLanes - 1);
  const long long el = (long long)blockIdx.x * kHerRows + ((int)threadIdx.x >> 4);
  if (el >= h.n) return;
  const int e = (int)el;
  if (mask != nullptr && mask[e] == 0) return;
  if (obs != nullptr && c < kHerObs) h.stage_obs[(size_t)e * kHerObs + c] = obs[(size_t)e * kHerObs + c];
  if (goal != nullptr && c < 3) h.stage_goal[(size_t)e * 3 + c] = goal[(size_t)e * 3 + c];
  if (c == kHerLanes - 1) h.meta[2 * (size_t)h.n + e] = 0;
}

__global__ __launch_bounds__(kScanThreads) void so100_her_scan_kernel(int n, int T, const int32_t* __restrict__ count,
                                                                      int32_t* __restrict__ prefix) {
  __shared__ int wave_sum[2][kScanThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;                                         // the sum of every tile before this one: < T n < 2^31
  int buf = 0;
  for (long long t0 = 0; t0 < n; t0 += kScanTile, buf ^= 1) {
    const long long i0 = t0 + (long long)tid * kScanItems;
    int v[kScanItems];
#pragma unroll
    for (int k = 0; k < kScanItems; k++) v[k] = i0 + k < n ? clampi(count[i0 + k], 0, T) : 0;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) mine += v[k];
    int incl = mine;                                     // inclusive scan of the wave's 64 sums
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sum[buf][wave] = incl;
    __syncthreads();                                     // (the buffers alternate: one barrier per tile)
    int before = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; w++) {
      const int ws = wave_sum[buf][w];
      before += w < wave ? ws : 0;
      tile += ws;
    }
    int run = carry + before + incl - mine;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
      run += v[k];
      if (i0 + k < n) prefix[i0 + k] = run;
    }
    carry += tile;
  }
  if (tid == 0) prefix[n] = carry;
}

__global__ __launch_bounds__(kHerThreads) void so100_her_sample_kernel(so100_her h, so100_her_out o, int batch, int nrel,
                                                                       uint64_t call, const DevModel* __restrict__ model) {
  const int c = (int)threadIdx.x & (kHerLanes - 1);
  const long long il = (long long)blockIdx.x * kHerRows + ((int)threadIdx.x >> 4);
  if (il >= batch) return;
  const size_t i = (size_t)il;
  const int n = h.n, T = h.T, A = h.action_dim;
  const bool scalar = c == kHerLanes - 1;
  const long long cap = (long long)T * n;
  long long total = h.prefix[n];
  total = total < 0 ? 0 : (total > cap ? cap : total);
  if (total == 0) {                                      // an empty buffer: zeros, nothing of the ring is read
    if (c < kHerObs) {
      o.observation[i * kHerObs + c] = 0.f;
      o.next_observation[i * kHerObs + c] = 0.f;
    }
    if (c < 3) {
      o.achieved_goal[i * 3 + c] = 0.f;
      o.desired_goal[i * 3 + c] = 0.f;
      o.next_achieved_goal[i * 3 + c] = 0.f;
      o.next_desired_goal[i * 3 + c] = 0.f;
    }
    if (c < A) o.actions[i * A + c] = 0.f;
    if (scalar) {
      o.rewards[i] = 0.f;
      o.dones[i] = 0.f;
      o.env[i] = 0;
      o.slot[i] = -1;
      o.goal_slot[i] = -1;
    }
    return;
  }
  // the transition: r uniform in [0, total), its env by binary search (the first e with prefix[e] > r)
  const long long r = (long long)__umul64hi(her_draw(h.seed, call, i, 0u), (uint64_t)total);
  int lo = 0, hi = n - 1;
  for (int it = 0; it < 32 && lo < hi; it++) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if ((long long)h.prefix[mid] > r) hi = mid; else lo = mid + 1;
  }
  const int e = lo;
  const long long base = e > 0 ? (long long)h.prefix[e - 1] : 0;
  const long long kq = r - base;
  const int k = (int)(kq < 0 ? 0 : (kq > T - 1 ? T - 1 : kq));
  const int vlo = clampi(h.meta[e], 0, T - 1);
  const int slot = add_mod(vlo, k, T);
  const size_t row = (size_t)slot * n + e;
  int gslot = -1;
  size_t grow = row;
  const bool relabel = il < nrel;
  if (relabel) {
    const int off = clampi(h.offset[row], 0, T - 1);
    const int first = sub_mod(slot, off, T);
    const int len = clampi(h.length[(size_t)first * n + e], off + 1, T);
    int j;
    if (h.strategy == SO100_HER_FINAL) {
      j = len - 1;
    } else {
      const uint64_t d = her_draw(h.seed, call, i, 1u);
      j = h.strategy == SO100_HER_FUTURE ? off + (int)__umul64hi(d, (uint64_t)(len - off)) : (int)__umul64hi(d, (uint64_t)len);
    }
    gslot = add_mod(first, clampi(j, 0, T - 1), T);
    grow = (size_t)gslot * n + e;
  }
  if (c < kHerObs) {
    o.observation[i * kHerObs + c] = h.obs[row * kHerObs + c];
    o.next_observation[i * kHerObs + c] = h.next_obs[row * kHerObs + c];
  }
  if (c < 3) {
    const float g = relabel ? h.next_obs[grow * kHerObs + c] : h.goal[row * 3 + c];
    o.achieved_goal[i * 3 + c] = h.obs[row * kHerObs + c];
    o.next_achieved_goal[i * 3 + c] = h.next_obs[row * kHerObs + c];
    o.desired_goal[i * 3 + c] = g;
    o.next_desired_goal[i * 3 + c] = g;
  }
  if (c < A) o.actions[i * A + c] = h.action[row * A + c];
  if (!scalar) return;
  float rew = h.reward[row];
  if (relabel) {
    const float* a = h.next_obs + row * kHerObs;
    const float* g = h.next_obs + grow * kHerObs;
    rew = goal_reward_f32(a[0], a[1], a[2], g[0], g[1], g[2], (float)model->goal_threshold);
  }
  o.rewards[i] = rew;
  o.dones[i] = h.terminated[row] != 0 ? 1.f : 0.f;
  o.env[i] = e;
  o.slot[i] = slot;
  o.goal_slot[i] = gslot;
}

hipError_t launch_her_push(const so100_her& h, const so100_her_step& st, hipStream_t s) {
  hipLaunchKernelGGL(so100_her_push_kernel, dim3((unsigned)((h.n + kHerRows - 1) / kHerRows)), dim3(kHerThreads), 0, s, h,
                     st);
  return hipGetLastError();
}

hipError_t launch_her_discard(const so100_her& h, const uint8_t* mask, const float* obs, const float* goal, hipStream_t s) {
  hipLaunchKernelGGL(so100_her_discard_kernel, dim3((unsigned)((h.n + kHerRows - 1) / kHerRows)), dim3(kHerThreads), 0, s,
                     h, mask, obs, goal);
  return hipGetLastError();
}

hipError_t launch_her_scan(const so100_her& h, hipStream_t s) {
  hipLaunchKernelGGL(so100_her_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, h.n, h.T, h.meta + h.n, h.prefix);
  return hipGetLastError();
}

hipError_t launch_count_scan(int n, int cap, const int32_t* count, int32_t* prefix, hipStream_t s) {
  hipLaunchKernelGGL(so100_her_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, n, cap, count, prefix);
  return hipGetLastError();
}

hipError_t launch_her_sample(const DevModel* m, const so100_her& h, const so100_her_out& o, int batch, int nrel,
                             uint64_t call, hipStream_t s) {
  hipLaunchKernelGGL(so100_her_sample_kernel, dim3((unsigned)(((long long)batch + kHerRows - 1) / kHerRows)),
                     dim3(kHerThreads), 0, s, h, o, batch, nrel, call, m);
  return hipGetLastError();
}

}  // namespace so100
