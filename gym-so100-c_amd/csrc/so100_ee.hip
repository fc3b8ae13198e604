// so100_ee.hip - the Cartesian end-effector action mode (C-ABI so100_ee_action, so100_ee_jacobian): a
// prologue that turns an end-effector delta (dx, dy, dz, droll, grip) into the six normalised joint actions so100_step
// takes.  The step kernels are untouched: this launch only writes their action input.
//
// One env per lane, the chain's forward kinematics in registers: the arm's five joints before ee_site are a serial chain
// of quaternion products, so a 16-lane row per env (the step's mapping) would leave 11 lanes idle in it, and EnvShared
// (3,200 B per env) rules out fk_stage's LDS staging at 64 envs per wave.  ee_fk restates fk_stage's formulas (the
// oracle's kinematics()) for bodies 0..4 and keeps what the Jacobian needs: the joint anchors, the joint axes, ee_site.
// No LDS, no scratch, float32 throughout; the 3x3 damped least-squares system is solved by Cholesky in closed form.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"
#include "so100_kin.h"

namespace so100 {

constexpr int kEeJoints = 5;      // the joints in front of ee_site (the jaw, joint 5, is behind it)
constexpr int kEeSolve = 4;       // the joints the position solve moves (wrist roll turns about an axis through ee_site)
constexpr int kEeThreads = 64;    // one wave per workgroup: the envs spread over the CUs at every batch size

struct EeArgs {
  so100_ee_ctrl ctrl;
  int n;
  const float* qpos;              // [n,13]
  const float* action;            // [n,5]
  const uint8_t* reinit;          // [n] or null
  float* q_cmd;                   // [n,5] in/out
  float* joint_action;            // [n,6]
  float* ee_target;               // [n,3] or null
};

namespace {

struct EeFrames {
  float anchor[kEeJoints][3];
  float axis[kEeJoints][3];
  float ee[3];
};

// Forward kinematics of bodies 0..4 of the chain at joint angles q[0..4] (fk_stage's formulas, per lane in registers)
DEV void ee_fk(const DevModel* __restrict__ m, const float* q, EeFrames& f) {
  float pos[3] = {m->base_pos[0], m->base_pos[1], m->base_pos[2]};
  float quat[4] = {m->base_quat[0], m->base_quat[1], m->base_quat[2], m->base_quat[3]};
  float R[9];
  quat2mat(R, quat);
#pragma unroll
  for (int a = 0; a < kEeJoints; a++) {
    float t[3];
    mulmv3(t, R, m->body_pos[a]);
    pos[0] += t[0]; pos[1] += t[1]; pos[2] += t[2];
    quat_mul(quat, quat, m->body_quat[a]);
    float R2[9];
    quat2mat(R2, quat);
    mulmv3(f.axis[a], R2, m->jnt_axis[a]);
#pragma unroll
    for (int k = 0; k < 3; k++) f.anchor[a][k] = pos[k];
    float sn, cs;
    sincosf(0.5f * q[a], &sn, &cs);
    const float qj[4] = {cs, m->jnt_axis[a][0] * sn, m->jnt_axis[a][1] * sn, m->jnt_axis[a][2] * sn};
    quat_mul(quat, quat, qj);
    quat_normalize(quat);
    quat2mat(R, quat);
  }
  float t[3];
  mulmv3(t, R, m->site_ee);
#pragma unroll
  for (int k = 0; k < 3; k++) f.ee[k] = pos[k] + t[k];
}

// column j of the positional Jacobian of ee_site: axis_j x (ee - anchor_j)
DEV void ee_jcol(const EeFrames& f, int j, float* col) {
  const float r[3] = {f.ee[0] - f.anchor[j][0], f.ee[1] - f.anchor[j][1], f.ee[2] - f.anchor[j][2]};
  cross3(col, f.axis[j], r);
}

// dq = J' (J J' + lam2 I)^-1 e for the 3 x kEeSolve Jacobian J (J[j]: column j): A = J J' + lam2 I >= lam2 I is
// symmetric positive definite, so its Cholesky factor exists and no pivot is needed
DEV void ee_dls(const float (*J)[3], const float* e, float lam2, float* dq) {
  float A00 = lam2, A10 = 0.f, A11 = lam2, A20 = 0.f, A21 = 0.f, A22 = lam2;
#pragma unroll
  for (int j = 0; j < kEeSolve; j++) {
    A00 += J[j][0] * J[j][0]; A10 += J[j][1] * J[j][0]; A11 += J[j][1] * J[j][1];
    A20 += J[j][2] * J[j][0]; A21 += J[j][2] * J[j][1]; A22 += J[j][2] * J[j][2];
  }
  const float l00 = sqrtf(A00), i00 = 1.0f / l00;
  const float l10 = A10 * i00, l20 = A20 * i00;
  const float l11 = sqrtf(A11 - l10 * l10), i11 = 1.0f / l11;
  const float l21 = (A21 - l20 * l10) * i11;
  const float l22 = sqrtf(A22 - l20 * l20 - l21 * l21), i22 = 1.0f / l22;
  const float y0 = e[0] * i00;
  const float y1 = (e[1] - l10 * y0) * i11;
  const float y2 = (e[2] - l20 * y0 - l21 * y1) * i22;
  const float x2 = y2 * i22;
  const float x1 = (y1 - l21 * x2) * i11;
  const float x0 = (y0 - l10 * x1 - l20 * x2) * i00;
#pragma unroll
  for (int j = 0; j < kEeSolve; j++) dq[j] = J[j][0] * x0 + J[j][1] * x1 + J[j][2] * x2;
}

DEV float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

}  // namespace

__global__ __launch_bounds__(kEeThreads) void so100_ee_action_kernel(const DevModel* __restrict__ m, EeArgs a) {
  const int i = blockIdx.x * kEeThreads + threadIdx.x;
  if (i >= a.n) return;
  const so100_ee_ctrl& c = a.ctrl;
  float q[kEeJoints], act[5], qc[kEeJoints];
#pragma unroll
  for (int k = 0; k < kEeJoints; k++) q[k] = a.qpos[(size_t)i * 13 + k];
#pragma unroll
  for (int k = 0; k < 5; k++) act[k] = clampf(a.action[(size_t)i * 5 + k], -1.f, 1.f);
  const bool re = a.reinit != nullptr && a.reinit[i] != 0;
#pragma unroll
  for (int k = 0; k < kEeJoints; k++) qc[k] = re ? q[k] : a.q_cmd[(size_t)i * 5 + k];

  // the target p from ee(q_cmd) (the first pass's frames), then `iters` damped least-squares steps of joints 0..3
  float cj[kEeJoints], p[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < kEeJoints; k++) cj[k] = qc[k];
  const float lam2 = c.damping * c.damping;
  for (int it = 0; it < c.iters; it++) {
    EeFrames f;
    ee_fk(m, cj, f);
    if (it == 0) {
#pragma unroll
      for (int k = 0; k < 3; k++) p[k] = clampf(f.ee[k] + c.pos_scale * act[k], c.ws_lo[k], c.ws_hi[k]);
    }
    const float e[3] = {p[0] - f.ee[0], p[1] - f.ee[1], p[2] - f.ee[2]};
    float J[kEeSolve][3], dq[kEeSolve];
#pragma unroll
    for (int j = 0; j < kEeSolve; j++) ee_jcol(f, j, J[j]);
    ee_dls(J, e, lam2, dq);
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < kEeSolve; j++) mx = fmaxf(mx, fabsf(dq[j]));
    const float s = c.dq_max / fmaxf(mx, c.dq_max);       // 1 up to dq_max, dq_max / max|dq| beyond: continuous
#pragma unroll
    for (int j = 0; j < kEeSolve; j++) cj[j] = clampf(cj[j] + s * dq[j], m->jnt_lo[j], m->jnt_hi[j]);
  }
  // anti-windup: the command leads the measured pose by at most lead_max
#pragma unroll
  for (int j = 0; j < kEeSolve; j++) qc[j] = q[j] + clampf(cj[j] - q[j], -c.lead_max, c.lead_max);
  qc[4] = clampf(qc[4] + c.rot_scale * act[3], m->jnt_lo[4], m->jnt_hi[4]);
#pragma unroll
  for (int k = 0; k < kEeJoints; k++) {
    a.q_cmd[(size_t)i * 5 + k] = qc[k];
    const float lo = m->action_lo[k], hi = m->action_hi[k];
    a.joint_action[(size_t)i * 6 + k] = clampf(2.f * (qc[k] - lo) / (hi - lo) - 1.f, -1.f, 1.f);
  }
  a.joint_action[(size_t)i * 6 + 5] = act[4];
  if (a.ee_target) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.ee_target[(size_t)i * 3 + k] = p[k];
  }
}

// ee_site and its positional Jacobian over joints 0..4 at qpos (the parity tests' op, as so100_unnormalize is)
__global__ __launch_bounds__(kEeThreads) void so100_ee_jacobian_kernel(const DevModel* __restrict__ m, int n,
                                                                       const float* qpos, float* ee, float* jac) {
  const int i = blockIdx.x * kEeThreads + threadIdx.x;
  if (i >= n) return;
  float q[kEeJoints];
#pragma unroll
  for (int k = 0; k < kEeJoints; k++) q[k] = qpos[(size_t)i * 13 + k];
  EeFrames f;
  ee_fk(m, q, f);
#pragma unroll
  for (int k = 0; k < 3; k++) ee[(size_t)i * 3 + k] = f.ee[k];
#pragma unroll
  for (int j = 0; j < kEeJoints; j++) {
    float col[3];
    ee_jcol(f, j, col);
#pragma unroll
    for (int r = 0; r < 3; r++) jac[(size_t)i * 15 + 5 * r + j] = col[r];
  }
}

hipError_t launch_ee_action(const DevModel* m, const so100_ee_ctrl& ctrl, int n, const float* qpos, const float* action,
                            const uint8_t* reinit, float* q_cmd, float* joint_action, float* ee_target, hipStream_t s) {
  const EeArgs a{ctrl, n, qpos, action, reinit, q_cmd, joint_action, ee_target};
  hipLaunchKernelGGL(so100_ee_action_kernel, dim3((a.n + kEeThreads - 1) / kEeThreads), dim3(kEeThreads), 0, s, m, a);
  return hipGetLastError();
}

hipError_t launch_ee_jacobian(const DevModel* m, int n, const float* qpos, float* ee, float* jac, hipStream_t s) {
  hipLaunchKernelGGL(so100_ee_jacobian_kernel, dim3((n + kEeThreads - 1) / kEeThreads), dim3(kEeThreads), 0, s, m, n,
                     qpos, ee, jac);
  return hipGetLastError();
}

}  // namespace so100
