// probe: the end-effector prologue in the step's lane mapping (16 lanes per env, fk_par in LDS) against the library's
// one-env-per-lane kernel (csrc/so100_ee.hip, included as it is): the same inputs, the largest difference of q_cmd, and
// HIP-event times of single launches of either at 8,192 and 65,536 envs (DESIGN.md §3.8 "Kernel").  Stand-alone:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-slp-vectorize -I include -I gym-so100-c_amd/csrc
//         tools/dev/ee_rows_probe.hip -o ee_rows_probe
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "so100_ee.hip"

using namespace so100;

static const float k_base_pos[] = {-0.469, 0.5, 0};
static const float k_base_quat[] = {0.707105483, 0, 0, 0.70710808};
static const float k_body_pos[] = {0, -0.0452, 0.0165, 0, 0.1025, 0.0306, 0, 0.11257, 0.028, 0, 0.0052, 0.1349, 0, -0.0601, 0, -0.0202, -0.0244, 0};
static const float k_body_quat[] = {0.707105281, 0.707108281, 0, 0, 0.707109018, 0.707104544, 0, 0, 0.707109018, -0.707104544, 0, 0, 0.707109018, -0.707104544, 0, 0, 0.707109018, 0, 0.707104544, 0, 1.34924e-11, -3.67321e-06, 1, -3.67321e-06};
static const float k_jnt_axis[] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
static const float k_site_ee[] = {0, -0.06, 0};
static const float k_lo[] = {-1.92f, -3.32f, -0.174f, -1.66f, -2.79f, -0.174f};
static const float k_hi[] = {1.92f, 0.174f, 3.14f, 1.66f, 2.79f, 1.75f};

// 4 envs per 64-lane workgroup, as the step: lane j < 5 of a row owns joint j, lanes k < 3 the target's component k
__global__ __launch_bounds__(kThreads) void ee_rows_kernel(const DevModel* __restrict__ m, EeArgs a) {
  __shared__ EnvShared shs[kEnvsPerBlock];
  const int row = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  const int i = blockIdx.x * kEnvsPerBlock + row;
  const bool act = i < a.n;
  EnvShared& sh = shs[row];
  const so100_ee_ctrl& c = a.ctrl;
  float q = 0.f, av = 0.f, qc = 0.f;
  if (act && lane < 5) {
    q = a.qpos[(size_t)i * 13 + lane];
    av = clampf(a.action[(size_t)i * 5 + lane], -1.f, 1.f);
    const bool re = a.reinit != nullptr && a.reinit[i] != 0;
    qc = re ? q : a.q_cmd[(size_t)i * 5 + lane];
  }
  if (lane < 13) sh.qpos[lane] = lane < 5 ? qc : (lane == 9 ? 1.f : 0.f);
  float cj = qc, p = 0.f;
  const float lam2 = c.damping * c.damping;
  for (int it = 0; it < c.iters; it++) {
    __syncthreads();
    fk_par(m, sh, lane, true);
    __syncthreads();
    if (it == 0 && lane < 3) p = clampf(sh.site_ee[lane] + c.pos_scale * av, c.ws_lo[lane], c.ws_hi[lane]);
    if (lane < 3) sh.vec[lane] = p - sh.site_ee[lane];
    float col[3] = {0.f, 0.f, 0.f};
    if (lane < kEeSolve) {
      const float r[3] = {sh.site_ee[0] - sh.anchor[lane][0], sh.site_ee[1] - sh.anchor[lane][1],
                          sh.site_ee[2] - sh.anchor[lane][2]};
      cross3(col, sh.axis[lane], r);
    }
    const float A00 = rowsum16(col[0] * col[0]) + lam2, A10 = rowsum16(col[1] * col[0]);
    const float A11 = rowsum16(col[1] * col[1]) + lam2, A20 = rowsum16(col[2] * col[0]);
    const float A21 = rowsum16(col[2] * col[1]), A22 = rowsum16(col[2] * col[2]) + lam2;
    __syncthreads();
    const float e[3] = {sh.vec[0], sh.vec[1], sh.vec[2]};
    const float l00 = sqrtf(A00), i00 = 1.0f / l00;
    const float l10 = A10 * i00, l20 = A20 * i00;
    const float l11 = sqrtf(A11 - l10 * l10), i11 = 1.0f / l11;
    const float l21 = (A21 - l20 * l10) * i11;
    const float l22 = sqrtf(A22 - l20 * l20 - l21 * l21), i22 = 1.0f / l22;
    const float y0 = e[0] * i00, y1 = (e[1] - l10 * y0) * i11, y2 = (e[2] - l20 * y0 - l21 * y1) * i22;
    const float x2 = y2 * i22, x1 = (y1 - l21 * x2) * i11, x0 = (y0 - l10 * x1 - l20 * x2) * i00;
    const float dq = col[0] * x0 + col[1] * x1 + col[2] * x2;      // 0 in lanes >= kEeSolve
    if (lane < kEeSolve) sh.vec[4 + lane] = fabsf(dq);
    __syncthreads();
    const float mx = fmaxf(fmaxf(sh.vec[4], sh.vec[5]), fmaxf(sh.vec[6], sh.vec[7]));
    const float s = c.dq_max / fmaxf(mx, c.dq_max);
    if (lane < kEeSolve) {
      cj = clampf(cj + s * dq, m->jnt_lo[lane], m->jnt_hi[lane]);
      sh.qpos[lane] = cj;
    }
  }
  if (lane < kEeSolve) qc = q + clampf(cj - q, -c.lead_max, c.lead_max);
  if (lane == 3) sh.vec[12] = av;                                   // droll for lane 4
  if (lane == 4) sh.vec[13] = av;                                   // grip for lane 5
  __syncthreads();
  if (lane == 4) qc = clampf(qc + c.rot_scale * sh.vec[12], m->jnt_lo[4], m->jnt_hi[4]);
  if (!act) return;
  if (lane < 5) {
    a.q_cmd[(size_t)i * 5 + lane] = qc;
    const float lo = m->action_lo[lane], hi = m->action_hi[lane];
    a.joint_action[(size_t)i * 6 + lane] = clampf(2.f * (qc - lo) / (hi - lo) - 1.f, -1.f, 1.f);
  }
  if (lane == 5) a.joint_action[(size_t)i * 6 + 5] = sh.vec[13];
  if (lane < 3 && a.ee_target) a.ee_target[(size_t)i * 3 + lane] = p;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
  DevModel h;
  memset(&h, 0, sizeof(h));
  memcpy(h.base_pos, k_base_pos, sizeof(h.base_pos)); memcpy(h.base_quat, k_base_quat, sizeof(h.base_quat));
  memcpy(h.body_pos, k_body_pos, sizeof(h.body_pos)); memcpy(h.body_quat, k_body_quat, sizeof(h.body_quat));
  memcpy(h.jnt_axis, k_jnt_axis, sizeof(h.jnt_axis)); memcpy(h.site_ee, k_site_ee, sizeof(h.site_ee));
  memcpy(h.jnt_lo, k_lo, sizeof(k_lo)); memcpy(h.jnt_hi, k_hi, sizeof(k_hi));
  memcpy(h.action_lo, k_lo, sizeof(k_lo)); memcpy(h.action_hi, k_hi, sizeof(k_hi));
  DevModel* d;
  CK(hipMalloc(&d, sizeof(h)));
  CK(hipMemcpy(d, &h, sizeof(h), hipMemcpyHostToDevice));
  so100_ee_ctrl ctrl = {sizeof(so100_ee_ctrl), 2, 0.01f, 0.17453292f, 0.02f, 0.2f, 0.5f, {-0.6096f, 0.219f, 0.f}, {0.6096f, 0.981f, 0.6f}};
  const int sizes[2] = {8192, 65536};
  for (int n : sizes) {
    std::vector<float> qpos((size_t)n * 13, 0.f), act((size_t)n * 5), qcmd((size_t)n * 5);
    uint32_t s = 12345u;
    auto u = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.f / 16777216.f); };
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < 5; j++) {
        const float mid = j == 1 ? -0.96f : (j == 2 ? 1.16f : 0.f);
        qpos[(size_t)i * 13 + j] = mid + 0.6f * (u() - 0.5f);
        qcmd[(size_t)i * 5 + j] = qpos[(size_t)i * 13 + j] + 0.2f * (u() - 0.5f);
        act[(size_t)i * 5 + j] = 2.4f * (u() - 0.5f);
      }
      qpos[(size_t)i * 13 + 9] = 1.f;
    }
    float *dq, *da, *dc[2], *dj[2], *dt[2];
    CK(hipMalloc(&dq, qpos.size() * 4)); CK(hipMalloc(&da, act.size() * 4));
    CK(hipMemcpy(dq, qpos.data(), qpos.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(da, act.data(), act.size() * 4, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++) {
      CK(hipMalloc(&dc[k], qcmd.size() * 4)); CK(hipMalloc(&dj[k], (size_t)n * 6 * 4)); CK(hipMalloc(&dt[k], (size_t)n * 3 * 4));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> out[2], ms[2];
    for (int k = 0; k < 2; k++) {                                   // 0: one env per lane (the library's), 1: rows
      const EeArgs a{ctrl, n, dq, da, nullptr, dc[k], dj[k], dt[k]};
      for (int rep = 0; rep < 13; rep++) {                          // 3 warm-up launches, 10 timed; each from the same q_cmd
        CK(hipMemcpy(dc[k], qcmd.data(), qcmd.size() * 4, hipMemcpyHostToDevice));
        CK(hipEventRecord(e0, 0));
        if (k == 0) hipLaunchKernelGGL(so100_ee_action_kernel, dim3((n + kEeThreads - 1) / kEeThreads), dim3(kEeThreads), 0, 0, d, a);
        else hipLaunchKernelGGL(ee_rows_kernel, dim3((n + kEnvsPerBlock - 1) / kEnvsPerBlock), dim3(kThreads), 0, 0, d, a);
        CK(hipGetLastError());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 3) ms[k].push_back(t * 1e3f);
      }
      out[k].resize(qcmd.size());
      CK(hipMemcpy(out[k].data(), dc[k], qcmd.size() * 4, hipMemcpyDeviceToHost));
      std::sort(ms[k].begin(), ms[k].end());
    }
    float worst = 0.f, moved = 0.f;
    for (size_t t = 0; t < qcmd.size(); t++) {
      worst = fmaxf(worst, fabsf(out[0][t] - out[1][t]));
      moved = fmaxf(moved, fabsf(out[0][t] - qcmd[t]));
    }
    printf("%6d envs: one env per lane median %.1f us (min %.1f, max %.1f); 16 lanes per env median %.1f us (min %.1f, max %.1f); "
           "max |q_cmd difference| %.3e (largest move %.3f rad)\n", n, 0.5f * (ms[0][4] + ms[0][5]), ms[0][0], ms[0][9],
           0.5f * (ms[1][4] + ms[1][5]), ms[1][0], ms[1][9], worst, moved);
    CK(hipFree(dq)); CK(hipFree(da));
    for (int k = 0; k < 2; k++) { CK(hipFree(dc[k])); CK(hipFree(dj[k])); CK(hipFree(dt[k])); }
  }
  return 0;
}
