// so100_act.hip - the actuation-latency model (C-ABI so100_actuate): a prologue that turns the commanded
// action into the applied one so100_step takes - a per-env delay of whole control steps out of a ring of the last eight
// commands, first-order smoothing and a slew limit.  The step kernels are untouched: this launch only writes their
// action input, as so100_ee_action does.
//
// One thread per (env, component): once an env's three parameters are read the work is elementwise, and with the ring
// slot-major ([8][n][6]) every access of a wave is one contiguous run of floats.  A workgroup is 32 whole envs (192
// threads), so every reader of an env's `head` sits in the workgroup of the one thread that writes it: a barrier between
// the read and the write orders them.  No LDS, no scratch, float32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"
#include "so100_device.h"

namespace so100 {

constexpr int kActEnvs = 32;                  // envs per workgroup
constexpr int kActThreads = kActEnvs * 6;     // 3 waves
constexpr uint32_t kActMask = SO100_ACT_HIST - 1;
static_assert((SO100_ACT_HIST & (SO100_ACT_HIST - 1)) == 0 && SO100_ACT_MAX_DELAY < SO100_ACT_HIST,
              "the ring index is a mask, and a delayed read never meets the slot just written");

struct ActArgs {
  int n;
  const float* qpos;              // [n,13]
  const float* command;           // [n,6]
  const uint8_t* reinit;          // [n] or null
  const float* act_params;        // [n,4]: delay, alpha, rate, -
  float* hist;                    // [8][n][6]
  int32_t* head;                  // [n]
  float* action;                  // [n,6] in/out: the applied action y
};

__global__ __launch_bounds__(kActThreads) void so100_actuate_kernel(const DevModel* __restrict__ m, ActArgs a) {
  const int e = blockIdx.x * kActEnvs + (int)threadIdx.x / 6, c = (int)threadIdx.x % 6;
  const bool live = e < a.n;
  uint32_t head = 0;
  if (live) head = (uint32_t)a.head[e];
  __syncthreads();                // every read of head[e] is before its write below (no thread leaves above this)
  if (!live) return;
  const size_t el = (size_t)e * 6 + c, ring = (size_t)a.n * 6;
  const float u = fminf(fmaxf(a.command[el], -1.f), 1.f);
  const float* p = a.act_params + (size_t)e * 4;
  const uint32_t d = (uint32_t)fminf(fmaxf(p[0], 0.f), (float)SO100_ACT_MAX_DELAY);   // (a NaN reads as 0)
  const float alpha = p[1], r = p[2];
  const bool re = a.reinit != nullptr && a.reinit[e] != 0;
  float y, hold = 0.f;
  if (re) {
    const float lo = m->action_lo[c], hi = m->action_hi[c];
    hold = fminf(fmaxf(2.f * (a.qpos[(size_t)e * 13 + c] - lo) / (hi - lo) - 1.f, -1.f), 1.f);
#pragma unroll
    for (int s = 0; s < SO100_ACT_HIST; s++) a.hist[s * ring + el] = hold;
    y = hold;
    head = 0;
  } else {
    y = a.action[el];
  }
  a.hist[(head & kActMask) * ring + el] = u;
  // head < d reads a slot not written since the re-initialisation: it holds `hold`
  const float v = d == 0 ? u : (re ? hold : a.hist[((head - d) & kActMask) * ring + el]);
  if (c == 0) a.head[e] = (int32_t)(head + 1);
  const float w = alpha == 1.f ? v : y + alpha * (v - y);
  const float dy = w - y;
  y = fabsf(dy) <= r ? w : y + copysignf(r, dy);
  a.action[el] = y;
}

hipError_t launch_actuate(const DevModel* m, int n, const float* qpos, const float* command, const uint8_t* reinit,
                          const float* act_params, float* hist, int32_t* head, float* action, hipStream_t s) {
  const ActArgs a{n, qpos, command, reinit, act_params, hist, head, action};
  hipLaunchKernelGGL(so100_actuate_kernel, dim3((a.n + kActEnvs - 1) / kActEnvs), dim3(kActThreads), 0, s, m, a);
  return hipGetLastError();
}

}  // namespace so100
