// probe: the actuation prologue with one env per lane (the six components in a loop, the same slot-major ring) against
// the library's thread-per-(env, component) kernel (csrc/so100_act.hip, included as it is): the same inputs, a bitwise
// comparison of every output, and HIP-event times of single launches of either at 8,192 and 65,536 envs (DESIGN.md §3.9
// "Kernel").  Stand-alone:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -I include -I gym-so100-c_amd/csrc
//         tools/dev/act_map_probe.hip -o act_map_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "so100_act.hip"

using namespace so100;

static const float k_lo[] = {-1.92f, -3.32f, -0.174f, -1.66f, -2.79f, -0.174f};
static const float k_hi[] = {1.92f, 0.174f, 3.14f, 1.66f, 2.79f, 1.75f};

// one env per lane: the formulas of so100_actuate_kernel, component by component
__global__ __launch_bounds__(64) void act_lane_kernel(const DevModel* __restrict__ m, ActArgs a) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= a.n) return;
  const size_t ring = (size_t)a.n * 6;
  const float* p = a.act_params + (size_t)e * 4;
  const uint32_t d = (uint32_t)fminf(fmaxf(p[0], 0.f), (float)SO100_ACT_MAX_DELAY);
  const float alpha = p[1], r = p[2];
  const bool re = a.reinit != nullptr && a.reinit[e] != 0;
  const uint32_t head = re ? 0u : (uint32_t)a.head[e];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    const size_t el = (size_t)e * 6 + c;
    const float u = fminf(fmaxf(a.command[el], -1.f), 1.f);
    float y, hold = 0.f;
    if (re) {
      const float lo = m->action_lo[c], hi = m->action_hi[c];
      hold = fminf(fmaxf(2.f * (a.qpos[(size_t)e * 13 + c] - lo) / (hi - lo) - 1.f, -1.f), 1.f);
#pragma unroll
      for (int s = 0; s < SO100_ACT_HIST; s++) a.hist[s * ring + el] = hold;
      y = hold;
    } else {
      y = a.action[el];
    }
    a.hist[(head & kActMask) * ring + el] = u;
    const float v = d == 0 ? u : (re ? hold : a.hist[((head - d) & kActMask) * ring + el]);
    const float w = alpha == 1.f ? v : y + alpha * (v - y);
    const float dy = w - y;
    a.action[el] = fabsf(dy) <= r ? w : y + copysignf(r, dy);
  }
  a.head[e] = (int32_t)(head + 1);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  DevModel h;
  memset(&h, 0, sizeof(h));
  memcpy(h.action_lo, k_lo, sizeof(k_lo)); memcpy(h.action_hi, k_hi, sizeof(k_hi));
  DevModel* d;
  CK(hipMalloc(&d, sizeof(h)));
  CK(hipMemcpy(d, &h, sizeof(h), hipMemcpyHostToDevice));
  const int sizes[2] = {8192, 65536};
  for (int n : sizes) {
    std::vector<float> qpos((size_t)n * 13, 0.f), cmd((size_t)n * 6), par((size_t)n * 4), hist0((size_t)n * 48), y0((size_t)n * 6);
    std::vector<int32_t> head0(n);
    std::vector<uint8_t> re(n);
    uint32_t s = 12345u;
    auto u = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.f / 16777216.f); };
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < 6; j++) {
        qpos[(size_t)i * 13 + j] = k_lo[j] + (k_hi[j] - k_lo[j]) * u();
        cmd[(size_t)i * 6 + j] = 2.4f * (u() - 0.5f);
        y0[(size_t)i * 6 + j] = 2.f * (u() - 0.5f);
      }
      par[(size_t)i * 4 + 0] = (float)(int)(8.f * u());
      par[(size_t)i * 4 + 1] = i % 4 == 0 ? 1.f : 0.3f + 0.7f * u();
      par[(size_t)i * 4 + 2] = i % 4 == 0 ? 2.f : 0.05f + 1.95f * u();
      par[(size_t)i * 4 + 3] = 0.f;
      head0[i] = (int)(40.f * u());
      re[i] = u() < 0.125f;
    }
    for (size_t t = 0; t < hist0.size(); t++) hist0[t] = 2.f * (u() - 0.5f);
    float *dq, *dc, *dp, *dh[2], *dy[2];
    int32_t* dhead[2];
    uint8_t* dre;
    CK(hipMalloc(&dq, qpos.size() * 4)); CK(hipMalloc(&dc, cmd.size() * 4)); CK(hipMalloc(&dp, par.size() * 4));
    CK(hipMalloc(&dre, n));
    CK(hipMemcpy(dq, qpos.data(), qpos.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dc, cmd.data(), cmd.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dp, par.data(), par.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dre, re.data(), n, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++) {
      CK(hipMalloc(&dh[k], hist0.size() * 4)); CK(hipMalloc(&dy[k], y0.size() * 4)); CK(hipMalloc(&dhead[k], (size_t)n * 4));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> ms[2], oh[2], oy[2];
    std::vector<int32_t> ohead[2];
    for (int k = 0; k < 2; k++) {                                   // 0: thread per element (the library's), 1: env per lane
      const ActArgs a{n, dq, dc, dre, dp, dh[k], dhead[k], dy[k]};
      for (int rep = 0; rep < 13; rep++) {                          // 3 warm-up launches, 10 timed; each from the same state
        CK(hipMemcpy(dh[k], hist0.data(), hist0.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dy[k], y0.data(), y0.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dhead[k], head0.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        CK(hipEventRecord(e0, 0));
        if (k == 0) hipLaunchKernelGGL(so100_actuate_kernel, dim3((n + kActEnvs - 1) / kActEnvs), dim3(kActThreads), 0, 0, d, a);
        else hipLaunchKernelGGL(act_lane_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, d, a);
        CK(hipGetLastError());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 3) ms[k].push_back(t * 1e3f);
      }
      oh[k].resize(hist0.size()); oy[k].resize(y0.size()); ohead[k].resize(n);
      CK(hipMemcpy(oh[k].data(), dh[k], hist0.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(oy[k].data(), dy[k], y0.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(ohead[k].data(), dhead[k], (size_t)n * 4, hipMemcpyDeviceToHost));
      std::sort(ms[k].begin(), ms[k].end());
    }
    const bool same = memcmp(oh[0].data(), oh[1].data(), hist0.size() * 4) == 0 &&
                      memcmp(oy[0].data(), oy[1].data(), y0.size() * 4) == 0 &&
                      memcmp(ohead[0].data(), ohead[1].data(), (size_t)n * 4) == 0;
    printf("%6d envs: thread per element median %.1f us (min %.1f, max %.1f); one env per lane median %.1f us (min %.1f, max %.1f); "
           "ring, head and applied action equal bit for bit: %s\n", n, 0.5f * (ms[0][4] + ms[0][5]), ms[0][0], ms[0][9],
           0.5f * (ms[1][4] + ms[1][5]), ms[1][0], ms[1][9], same ? "yes" : "NO");
    CK(hipFree(dq)); CK(hipFree(dc)); CK(hipFree(dp)); CK(hipFree(dre));
    for (int k = 0; k < 2; k++) { CK(hipFree(dh[k])); CK(hipFree(dy[k])); CK(hipFree(dhead[k])); }
  }
  return 0;
}
