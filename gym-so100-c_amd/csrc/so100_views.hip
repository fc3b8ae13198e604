// so100_views.hip - per-env view records for so100_render_views, drawn on the device (C-ABI so100_views_sample): the
// visual part of domain randomisation (camera jitter, light strengths and directions, material colours).  One thread per
// env.  Every draw is a pure function of (seed, global env id, episode, field number): the counter-based splitmix64 hash
// of the physical randomisation (gym_so100/vec_env.py _hash_uniform) with the episode mixed in, so a record does not
// depend on the sharding, on the mask or on launch order, and per-episode resampling needs no host round trip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"

namespace so100 {

struct ViewSampleArgs {
  so100_view_dr dr;
  so100_camera cam;                     // the base camera
  uint32_t base_rgb[SO100_NMATERIAL];
  const uint32_t* episode;              // [n] or null = 0
  const uint8_t* mask;                  // [n] or null: the records to fill
  so100_view* views;                    // [n]
  int n, env_offset;
};

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// U[0,1) on a 2^-24 grid (exact in float32)
__device__ __forceinline__ float uniform(uint64_t seed, uint64_t id, uint32_t episode, uint32_t field) {
  const uint64_t k = splitmix64(seed ^ (id * 0x100000001B3ull) ^ ((uint64_t)field * 0xD1B54A32D192ED03ull));
  return (float)(splitmix64(k + episode) >> 40) * (1.f / 16777216.f);
}

// a scale from [lo, hi]; lo for a range of zero width
__device__ __forceinline__ float scale(const float* r, float u) {
  return fminf(fmaxf(r[0] + (r[1] - r[0]) * u, r[0]), r[1]);
}

// Rodrigues: R = I + (sin t / t) K + (2 sin^2(t/2) / t^2) K^2, K = skew(v), t = |v|, K^2 = v v^T - t^2 I
__device__ __forceinline__ void rodrigues(float* R, const float* v) {
  const float t2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  const float t = sqrtf(t2);
  float A = 1.f, B = 0.5f;
  if (t > 1e-12f) {
    const float h = sinf(0.5f * t);
    A = sinf(t) / t;
    B = 2.f * h * h / t2;
  }
  R[0] = 1.f + B * (v[0] * v[0] - t2); R[1] = B * v[0] * v[1] - A * v[2];   R[2] = B * v[0] * v[2] + A * v[1];
  R[3] = B * v[1] * v[0] + A * v[2];   R[4] = 1.f + B * (v[1] * v[1] - t2); R[5] = B * v[1] * v[2] - A * v[0];
  R[6] = B * v[2] * v[0] - A * v[1];   R[7] = B * v[2] * v[1] + A * v[0];   R[8] = 1.f + B * (v[2] * v[2] - t2);
}

}  // namespace

__global__ void __launch_bounds__(256) so100_views_kernel(ViewSampleArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n || (a.mask && !a.mask[i])) return;
  const uint64_t seed = a.dr.seed, id = (uint64_t)(a.env_offset + i);
  const uint32_t ep = a.episode ? a.episode[i] : 0u;
  auto u = [&](uint32_t field) { return uniform(seed, id, ep, field); };
  auto sym = [&](uint32_t field, float hw) { return (2.f * u(field) - 1.f) * hw; };
  so100_view o;
  // camera: a zero half-width copies the base value (no -0 + 0 either)
  for (int k = 0; k < 3; k++) o.pos[k] = a.dr.cam_pos != 0.f ? a.cam.pos[k] + sym(16 + k, a.dr.cam_pos) : a.cam.pos[k];
  if (a.dr.cam_rot != 0.f) {
    const float v[3] = {sym(19, a.dr.cam_rot), sym(20, a.dr.cam_rot), sym(21, a.dr.cam_rot)};
    float R[9];
    rodrigues(R, v);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++)
        o.mat[3 * r + c] = a.cam.mat[3 * r] * R[c] + a.cam.mat[3 * r + 1] * R[3 + c] + a.cam.mat[3 * r + 2] * R[6 + c];
  } else {
    for (int k = 0; k < 9; k++) o.mat[k] = a.cam.mat[k];
  }
  o.fovy = a.cam.fovy * scale(a.dr.fovy, u(22));
  o.head_ambient = a.cam.head_ambient * scale(a.dr.ambient, u(23));
  o.head_diffuse = a.cam.head_diffuse * scale(a.dr.headlight, u(24));
  // lights
  float L[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  if (a.dr.light_rot != 0.f) {
    const float v[3] = {sym(29, a.dr.light_rot), sym(30, a.dr.light_rot), sym(31, a.dr.light_rot)};
    rodrigues(L, v);
  }
  for (int l = 0; l < SO100_MAX_LIGHTS; l++) {
    const float* d = a.cam.light_dir[l];
    o.light_diffuse[l] = a.cam.light_diffuse[l] * scale(a.dr.light[l], u(25 + l));
    for (int r = 0; r < 3; r++)
      o.light_dir[l][r] = a.dr.light_rot != 0.f ? L[3 * r] * d[0] + L[3 * r + 1] * d[1] + L[3 * r + 2] * d[2] : d[r];
  }
  // colours
  for (int m = 0; m < SO100_NMATERIAL; m++) {
    uint32_t q = 0;
    for (int k = 0; k < 3; k++) {
      const float base = (float)((a.base_rgb[m] >> (8 * k)) & 0xFFu) * (1.f / 255.f);
      const float val = fminf(fmaxf(base * scale(a.dr.color[m], u(32 + 3 * m + k)), 0.f), 1.f);
      q |= (uint32_t)(val * 255.f + 0.5f) << (8 * k);
    }
    o.rgb[m] = q;
  }
  for (int k = 0; k < 4; k++) o.reserved[k] = 0u;
  a.views[i] = o;
}

hipError_t launch_views_sample(const so100_view_dr& dr, const so100_camera& cam, const uint32_t* base_rgb,
                               const uint32_t* episode, const uint8_t* mask, so100_view* views, int n, int env_offset,
                               hipStream_t s) {
  ViewSampleArgs a{dr, cam, {}, episode, mask, views, n, env_offset};
  for (int m = 0; m < SO100_NMATERIAL; m++) a.base_rgb[m] = base_rgb[m];
  hipLaunchKernelGGL(so100_views_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
