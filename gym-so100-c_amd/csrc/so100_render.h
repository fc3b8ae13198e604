// so100_render.h - the render kernel's body, shared by its seven launches: so100_render.hip (the hwc image alone),
// so100_render_sinks.hip (so100_render_to's further sinks), so100_render_views.hip (so100_render_views: camera,
// lights and colours per env), so100_render_aux.hip (so100_render_aux: the depth and label sinks, with or without
// views), so100_render_cams.hip (so100_render_cams: the aux launch over a grid of (env, camera), with cameras that
// ride on a body), so100_render_shadow.hip (so100_render_shadow: the cams launch with one light occluded per pixel
// by a shadow map the block builds in LDS) and so100_render_msaa.hip (so100_render_msaa: the cams launch's colour sinks
// with S coverage samples per pixel, resolved in LDS).  One translation unit per kernel: with two instantiations in one unit the hwc-only kernel was scheduled
// differently and measured slower.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "so100_device.h"
#include "so100.h"
#include "so100_common.h"
#include "so100_kin.h"

namespace so100 {

constexpr int kRenderThreads = 256;
constexpr int kTilePx = 4096;           // depth-buffer pixels per band (32 KB of LDS)
constexpr int kBigPx = 64;              // triangles with a larger band bbox go to phase B
constexpr int kBigCap = 256;
constexpr int kBigCapMsaa = 1024;       // so100_render_msaa's list of phase-B triangles: kBigCap wide ones, the rest
constexpr int kWideKeys = 1024;         // a phase-B triangle of so100_render_msaa with fewer keys is drawn by one wave
constexpr int kWave = 64;

struct RenderArgs {
  const DevModel* m;
  const float4* tri;                    // [ntri][3] body-frame vertices (w unused)
  const int* tri_body;                  // [ntri] body (0 world, 1 Base, 2..7 links, 8 cube)
  const uint32_t* tri_rgb;              // [ntri] RGB8 base colour
  int ntri;
  const float* qpos;                    // [n][13]
  const uint8_t* mask;                  // [n] or null: envs to draw
  so100_camera cam;
  int n, width, height;
  uint8_t* out;                         // [n][height][width][3] (hwc sink; may be null in RenderSinkArgs)
};
// the launch with further sinks (so100_render_to).  The hwc-only launch keeps RenderArgs as its kernel argument: its
// instantiation is the kernel of before the sinks.
struct RenderSinkArgs : RenderArgs {
  uint8_t* chw;                         // [n][3][height][width] or null
  float* flat;                          // [n][flat_pitch] or null: floats [0, 3HW) = the hwc bytes / 255
  long long flat_pitch;
};
// the launch with a view record per env (so100_render_views): pos, mat, fovy, the headlight terms, the light directions
// and diffuses and the five base colours come from views[env]; a.cam keeps the launch-uniform track, znear and nlight
struct RenderViewArgs : RenderSinkArgs {
  const so100_view* views;              // [n]
  const uint8_t* material;              // [ntri] material id < SO100_NMATERIAL: the base colour is views[env].rgb[id]
};
// the launch with the depth and label sinks (so100_render_aux).  Its key carries a label under the colour:
// depth bits << 32 | RGB8 << 8 | label, so colour still orders equal depths as in the other three kernels and the label
// orders what is left.  views may be null (uniform per launch): the LDS record is then filled from a.cam and the base
// colour is tri_rgb[t]
struct RenderAuxArgs : RenderViewArgs {
  const uint8_t* label;                 // [ntri] label < 255, or null (every triangle 0; no seg sink then)
  float* depth;                         // [n][height][width] or null: 1 / izp of the winning key; background 0.0f
  uint8_t* seg;                         // [n][height][width] or null: the winning key's label; background 255
};
// the launch over (env, camera) (so100_render_cams): block (env, c) is the aux kernel's block drawing env from cams[c]
// and views[c * n + env] into slot env * ncam + c of every sink; frame_body[c] > 0 puts cams[c] (and its records) in
// that body's frame.  a.cam is not read
struct RenderCamsArgs : RenderAuxArgs {
  int ncam;
  so100_camera cams[SO100_MAX_CAMS];
  int frame_body[SO100_MAX_CAMS];       // 0 world, 1..8 the body the camera is mounted on
};
// the launch with cast shadows (so100_render_shadow): the cams launch whose blocks first rasterise the caster triangles
// into an orthographic depth map along light `light`, kept in LDS through all bands, and carry beside the key a second
// one whose colour is shaded with that light's diffuse taken as 0: a pixel the map occludes takes the second key's
// colour (DESIGN.md 3.7 "Shadows")
struct RenderShadowArgs : RenderCamsArgs {
  const uint8_t* caster;                // [ntri] non-zero: the triangle is drawn into the shadow map
  int light;                            // the casting light, < nlight of every camera; -1: nothing casts
  int map_size;                         // S: the map is S x S texels, S <= kShadowMapMax
  float center[3];                      // the map covers the disc of `radius` about `center` across the light
  float radius;
  float bias;                           // metres: occluded iff map depth < the point's depth - bias
  uint8_t* shadow;                      // [n][ncam][height][width] or null: 1 occluded, 0 lit, background 0
};
// the multisampled launch (so100_render_msaa): the cams launch whose pixels hold `samples` keys, one per sample point
// (x + 0.5 + ox[s], y + 0.5 + oy[s]); a triangle is set up and shaded once and its flat colour goes to every sample it
// covers.  After a band's two raster phases the samples' colours are averaged per channel, round half up (an empty
// sample is the background's 0), and the colour sinks read that byte.  depth and seg are not written (they are
// pixel-centre quantities: so100_render_cams')  (DESIGN.md 3.7 "Anti-aliasing")
struct RenderMsaaArgs : RenderCamsArgs {
  int samples;                          // S: 1, 2 or 4, with width * S <= kTilePx
  float ox[SO100_MSAA_MAX], oy[SO100_MSAA_MAX];   // the sample offsets from the pixel centre, each inside (-0.5, 0.5)
};
constexpr int kShadowMapMax = SO100_SHADOW_MAP_MAX;        // 16 KB of LDS
constexpr uint32_t kShadowEmpty = 0xFFFFFFFFu;
// float32 -> uint32 that orders as the floats do (for atomicMin), and back
DEV uint32_t shadow_encode(float d) {
  const uint32_t u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEV float shadow_decode(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }
// the light's frame and the map's placement, in LDS
struct ShadowFrame {
  float d[3], u[3], v[3];               // the light's direction and the map's two axes
};
constexpr int kViewWords = (int)(sizeof(so100_view) / sizeof(uint32_t));
static_assert(sizeof(so100_view) == 160 && kViewWords == 40, "so100_view: 40 dwords");
// the env's record in LDS, filled one dword per thread
union ViewLds {
  so100_view v;
  uint32_t w[kViewWords];
};

// byte / 255 as numpy divides it (np.float32(b) / np.float32(255), the reference's env.py:267-270): the quotients are
// rounded by the compiler's IEEE constant evaluation, never by a reciprocal multiply on the device
struct ByteUnit {
  float v[256];
  constexpr ByteUnit() : v() {
    for (int b = 0; b < 256; b++) v[b] = (float)b / 255.0f;
  }
};

// c: where pos, the headlight terms and the lights come from: the launch's so100_camera or the env's so100_view
template <class Cam>
DEV uint32_t shade(const Cam& c, int nlight, const float* cm, const float* p0, const float* p1, const float* p2,
                   uint32_t rgb) {
  float e1[3], e2[3], nrm[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { e1[k] = p1[k] - p0[k]; e2[k] = p2[k] - p0[k]; }
  cross3(nrm, e1, e2);
  const float nl = sqrtf(dot3(nrm, nrm));
  const float inv = nl > 0.f ? 1.f / nl : 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) nrm[k] *= inv;
  // two-sided: the normal facing the camera
  float v[3] = {c.pos[0] - p0[0], c.pos[1] - p0[1], c.pos[2] - p0[2]};
  if (dot3(nrm, v) < 0.f) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
  // headlight: along the view direction (camera -z), so its diffuse term is n . z_cam
  const float zc[3] = {cm[2], cm[5], cm[8]};
  float lum = c.head_ambient + c.head_diffuse * fmaxf(0.f, dot3(nrm, zc));
  for (int l = 0; l < nlight; l++) lum += c.light_diffuse[l] * fmaxf(0.f, -dot3(nrm, c.light_dir[l]));
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float base = (float)((rgb >> (8 * k)) & 0xFFu) * (1.f / 255.f);
    const float val = fminf(fmaxf(base * lum, 0.f), 1.f);
    out |= (uint32_t)(val * 255.f + 0.5f) << (8 * k);
  }
  return out;
}

// the camera-like record the body reads: a.cam, or with views the env's record in LDS
template <class Args>
DEV decltype(auto) view_source(const Args& a, const ViewLds& vl) {
  if constexpr (std::is_same<Args, RenderViewArgs>::value || std::is_same<Args, RenderAuxArgs>::value ||
                std::is_same<Args, RenderCamsArgs>::value || std::is_same<Args, RenderShadowArgs>::value ||
                std::is_same<Args, RenderMsaaArgs>::value)
    return (vl.v);
  else return (a.cam);
}
// the launch's camera: the block's own of RenderCamsArgs / RenderShadowArgs / RenderMsaaArgs, a.cam in the other four
template <class Args>
DEV const so100_camera& launch_cam(const Args& a) {
  if constexpr (std::is_same<Args, RenderCamsArgs>::value || std::is_same<Args, RenderShadowArgs>::value ||
                std::is_same<Args, RenderMsaaArgs>::value)
    return a.cams[blockIdx.y];
  else return a.cam;
}

// Args = RenderArgs: the hwc image alone (so100_render and every hwc-only so100_render_to);
// Args = RenderSinkArgs: every non-null sink of a.out / a.chw / a.flat is written from the same band;
// Args = RenderViewArgs: the same sinks, drawn from views[env] (not referenced, vl costs the other two no LDS);
// Args = RenderAuxArgs: those sinks and a.depth / a.seg, from views[env] or (a.views null) from a.cam through vl;
// Args = RenderCamsArgs: the aux kernel's block per (env, camera): grid (n, ncam), see the struct;
// Args = RenderShadowArgs: the cams kernel with the shadow map, the second key and the shadow sink, see the struct;
// Args = RenderMsaaArgs: the cams kernel with S keys per pixel and the resolve, see the struct.
template <class Args>
__global__ void __launch_bounds__(kRenderThreads) so100_render_kernel(Args a) {
  constexpr bool kSinks = sizeof(Args) != sizeof(RenderArgs);
  constexpr bool kView = std::is_same<Args, RenderViewArgs>::value;
  constexpr bool kShadow = std::is_same<Args, RenderShadowArgs>::value;
  constexpr bool kMsaa = std::is_same<Args, RenderMsaaArgs>::value;
  constexpr bool kCams = std::is_same<Args, RenderCamsArgs>::value || kShadow || kMsaa;
  constexpr bool kAux = std::is_same<Args, RenderAuxArgs>::value || kCams;
  constexpr int kColShift = kAux ? 8 : 0;                  // the colour's place in the key's lower half
  __shared__ ViewLds vl;
  __shared__ EnvShared sh;
  __shared__ float frm[SO100_NBODY][12];           // body rotation (9) + position (3)
  __shared__ unsigned long long zb[kTilePx];
  // the shadow kernel alone (not referenced, these cost the other five no LDS): the key with the dark colour, after the
  // shadow test the pixel's 0 / 1; the record with the casting light's diffuse 0; the map and its frame.  The bands are
  // the other kernels' bands: a triangle's depth is then computed by the same phase (A or B) as in so100_render_cams
  __shared__ unsigned long long zd[kShadow ? kTilePx : 1];
  __shared__ ViewLds vd;
  __shared__ uint32_t smap[kShadow ? kShadowMapMax * kShadowMapMax : 1];
  __shared__ ShadowFrame sf;
  // the multisampled kernel lists more: with S keys per pixel the same box passes kBigPx S times sooner, and a large
  // triangle past a list's end is left to one thread (4 KB, inside the 40 KB that keep four workgroups per CU)
  constexpr int kCap = kMsaa ? kBigCapMsaa : kBigCap;
  __shared__ int big[kCap];
  __shared__ int nbig;
  __shared__ int nmid;                             // the multisampled kernel alone: its second list's length
  __shared__ float cmat[9];                        // camera frame (columns x, y, z) for this env
  const DevModel* __restrict__ m = a.m;
  const int tid = threadIdx.x, env = blockIdx.x;
  if (env >= a.n || (a.mask && !a.mask[env])) return;     // uniform per block
  const int W = a.width, H = a.height;
  const so100_camera& lc = launch_cam(a);
  // the block's slot in every sink and its view record, evaluated where they are used: env in the other four kernels
  auto slot = [&]() -> size_t { if constexpr (kCams) return (size_t)env * a.ncam + blockIdx.y; else return (size_t)env; };
  auto vrec = [&]() -> size_t { if constexpr (kCams) return (size_t)blockIdx.y * a.n + env; else return (size_t)env; };

  // ---- forward kinematics of this env (the stage kernel's fk_stage on thread 0)
  if (tid < SO100_NQ) sh.qpos[tid] = a.qpos[(size_t)env * SO100_NQ + tid];
  if constexpr (kView) {
    if (tid < kViewWords) vl.w[tid] = reinterpret_cast<const uint32_t*>(a.views + vrec())[tid];
  }
  if constexpr (kAux) {
    if (a.views) {                                         // uniform per launch
      if (tid < kViewWords) vl.w[tid] = reinterpret_cast<const uint32_t*>(a.views + vrec())[tid];
    } else if (tid == 0) {
      // the base camera as a record (what an identity record holds, bit for bit); rgb is not read without views
      so100_view& v = vl.v;
      for (int k = 0; k < 3; k++) v.pos[k] = lc.pos[k];
      for (int k = 0; k < 9; k++) v.mat[k] = lc.mat[k];
      v.fovy = lc.fovy;
      v.head_ambient = lc.head_ambient;
      v.head_diffuse = lc.head_diffuse;
      for (int l = 0; l < SO100_MAX_LIGHTS; l++) {
        v.light_diffuse[l] = lc.light_diffuse[l];
        for (int k = 0; k < 3; k++) v.light_dir[l][k] = lc.light_dir[l][k];
      }
    }
  }
  const auto& cv = view_source(a, vl);                     // read after the barrier below
  __syncthreads();
  joint_sincos(sh, tid);
  __syncthreads();
  if (tid == 0) {
    fk_stage(m, sh);
    float bq[4] = {m->base_quat[0], m->base_quat[1], m->base_quat[2], m->base_quat[3]}, bm[9];
    quat2mat(bm, bq);
    for (int b = 0; b < SO100_NBODY; b++) {
      float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, P[3] = {0, 0, 0};
      if (b == 1) {
        for (int k = 0; k < 9; k++) R[k] = bm[k];
        for (int k = 0; k < 3; k++) P[k] = m->base_pos[k];
      } else if (b >= 2 && b <= 7) {
        for (int k = 0; k < 9; k++) R[k] = sh.ser.xm[b - 2][k];
        for (int k = 0; k < 3; k++) P[k] = sh.ser.xp[b - 2][k];
      } else if (b == SO100_CUBE_BODY) {
        for (int k = 0; k < 9; k++) R[k] = sh.cube_mat[k];
        for (int k = 0; k < 3; k++) P[k] = sh.cube_pos[k];
      }
      for (int k = 0; k < 9; k++) frm[b][k] = R[k];
      for (int k = 0; k < 3; k++) frm[b][9 + k] = P[k];
    }
    if constexpr (kCams) {
      // a camera on a body: pos (and mat) are in the body's frame.  The record's pos becomes the world position here,
      // before the barrier after which the other threads read it; a world camera (0) is not transformed at all
      const int fb = a.frame_body[blockIdx.y];
      if (fb > 0) {
        const float* F = frm[fb];
        const float p[3] = {vl.v.pos[0], vl.v.pos[1], vl.v.pos[2]};
        for (int k = 0; k < 3; k++) vl.v.pos[k] = F[3 * k] * p[0] + F[3 * k + 1] * p[1] + F[3 * k + 2] * p[2] + F[9 + k];
        if (!lc.track) {                                   // a rigid mount: cmat = R_b . mat
          float mm[9];
          for (int k = 0; k < 9; k++) mm[k] = vl.v.mat[k];
          for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
              vl.v.mat[3 * i + j] = F[3 * i] * mm[j] + F[3 * i + 1] * mm[3 + j] + F[3 * i + 2] * mm[6 + j];
        }
      }
    }
    if (lc.track) {
      // mode="targetbody" on the ee body (scene_so100.xml:30 front_close -> vx300s_left/camera_focus, whose
      // origin is ee_site): MuJoCo's mj_camlight frame z = pos - target, x = (0,0,1) x z, y = z x x
      float z[3] = {cv.pos[0] - sh.site_ee[0], cv.pos[1] - sh.site_ee[1], cv.pos[2] - sh.site_ee[2]};
      float x[3], y[3];
      const float up[3] = {0.f, 0.f, 1.f};
      float n = sqrtf(dot3(z, z));
      if (n < 1e-15f) { z[0] = 1.f; z[1] = z[2] = 0.f; } else { z[0] /= n; z[1] /= n; z[2] /= n; }
      cross3(x, up, z);
      n = sqrtf(dot3(x, x));
      if (n < 1e-15f) { x[0] = 1.f; x[1] = x[2] = 0.f; } else { x[0] /= n; x[1] /= n; x[2] /= n; }
      cross3(y, z, x);
      for (int k = 0; k < 3; k++) { cmat[3 * k] = x[k]; cmat[3 * k + 1] = y[k]; cmat[3 * k + 2] = z[k]; }
    } else {
      for (int k = 0; k < 9; k++) cmat[k] = cv.mat[k];
    }
    if constexpr (kShadow) {
      // the dark record: this block's record (a mounted camera's pos already the world's) without the casting light
      for (int k = 0; k < kViewWords; k++) vd.w[k] = vl.w[k];
      if (a.light >= 0) {
        vd.v.light_diffuse[a.light] = 0.f;
        // the light's frame: d the direction, u = normalize(z x d) (x if d is vertical), v = d x u
        const float* ld = vl.v.light_dir[a.light];
        const float n = sqrtf(dot3(ld, ld));
        for (int k = 0; k < 3; k++) sf.d[k] = ld[k] / n;
        float u[3] = {-sf.d[1], sf.d[0], 0.f};             // z x d
        const float un = sqrtf(dot3(u, u));
        if (un < 1e-6f) { u[0] = 1.f; u[1] = u[2] = 0.f; } else { u[0] /= un; u[1] /= un; u[2] /= un; }
        for (int k = 0; k < 3; k++) sf.u[k] = u[k];
        cross3(sf.v, sf.d, u);
      }
    }
  }
  if constexpr (kShadow) {
    for (int i = tid; i < a.map_size * a.map_size; i += kRenderThreads) smap[i] = kShadowEmpty;
  }
  __syncthreads();
  if constexpr (kShadow) {
    // ---- the shadow map: every caster triangle, one per thread, with the camera rasteriser's rules on the map's S x S
    // texels (centres at +0.5, inclusive edges, the area reject); depth along d, linear in the edge weights
    // (no FMA contraction in the map's and the test's arithmetic: a product rounded differently moves a texel's or a
    // pixel's verdict, and the float32 restatement the mask is held to rounds every product)
    if (a.light >= 0) {
#pragma clang fp contract(off)
      auto dotp = [](const float* p, const float* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
      const int S = a.map_size;
      const float sc = 0.5f / a.radius;
      for (int t = tid; t < a.ntri; t += kRenderThreads) {
        if (!a.caster[t]) continue;
        const float* R = frm[a.tri_body[t]];
        float sx[3], sy[3], dz[3];
#pragma unroll
        for (int v = 0; v < 3; v++) {
          const float4 q = a.tri[3 * t + v];
          const float w[3] = {R[0] * q.x + R[1] * q.y + R[2] * q.z + R[9] - a.center[0],
                              R[3] * q.x + R[4] * q.y + R[5] * q.z + R[10] - a.center[1],
                              R[6] * q.x + R[7] * q.y + R[8] * q.z + R[11] - a.center[2]};
          sx[v] = (dotp(w, sf.u) * sc + 0.5f) * (float)S;
          sy[v] = (dotp(w, sf.v) * sc + 0.5f) * (float)S;
          dz[v] = dotp(w, sf.d);
        }
        const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
        if (!(fabsf(area) > 1e-12f)) continue;
        const int bx0 = max(0, (int)floorf(fminf(sx[0], fminf(sx[1], sx[2])) - 0.5f));
        const int bx1 = min(S - 1, (int)ceilf(fmaxf(sx[0], fmaxf(sx[1], sx[2])) - 0.5f));
        const int by0 = max(0, (int)floorf(fminf(sy[0], fminf(sy[1], sy[2])) - 0.5f));
        const int by1 = min(S - 1, (int)ceilf(fmaxf(sy[0], fmaxf(sy[1], sy[2])) - 0.5f));
        const float sg = area > 0.f ? 1.f : -1.f, inv = 1.f / area;
        for (int y = by0; y <= by1; y++)
          for (int x = bx0; x <= bx1; x++) {
            const float px = (float)x + 0.5f, py = (float)y + 0.5f;
            const float w0 = (sx[2] - sx[1]) * (py - sy[1]) - (sy[2] - sy[1]) * (px - sx[1]);
            const float w1 = (sx[0] - sx[2]) * (py - sy[2]) - (sy[0] - sy[2]) * (px - sx[2]);
            const float w2 = (sx[1] - sx[0]) * (py - sy[0]) - (sy[1] - sy[0]) * (px - sx[0]);
            if (w0 * sg < 0.f || w1 * sg < 0.f || w2 * sg < 0.f) continue;
            const float dep = (w0 * dz[0] + w1 * dz[1] + w2 * dz[2]) * inv;
            if (dep == dep) atomicMin(&smap[y * S + x], shadow_encode(dep));      // bx, by are inside the map
          }
      }
    }
    __syncthreads();
  }

  const float th = tanf(0.5f * cv.fovy * 0.017453292519943295f);
  const float aspect = (float)W / (float)H;
  int band = kTilePx / W > 0 ? kTilePx / W : 1;              // rows per band
  // the multisampled kernel alone: a pixel holds S keys, so a band is kTilePx / (W S) rows (>= 1: the entry point
  // refuses W S > kTilePx); the extremes of the sample offsets, which widen a triangle's box of pixels
  float oxlo = 0.f, oxhi = 0.f, oylo = 0.f, oyhi = 0.f;
  if constexpr (kMsaa) {
    band = max(1, kTilePx / (W * a.samples));
    oxlo = oxhi = a.ox[0];
    oylo = oyhi = a.oy[0];
    for (int s = 1; s < a.samples; s++) {
      oxlo = fminf(oxlo, a.ox[s]); oxhi = fmaxf(oxhi, a.ox[s]);
      oylo = fminf(oylo, a.oy[s]); oyhi = fmaxf(oyhi, a.oy[s]);
    }
  }
  uint8_t* img = a.out + slot() * H * W * 3;              // used where a.out is not null

  for (int y0 = 0; y0 < H; y0 += band) {
    const int y1 = min(H, y0 + band);
    const int npx = (y1 - y0) * W;
    // the multisampled kernel's keys: sample-major, plane s = zb[s * npx, (s + 1) * npx) (S npx <= kTilePx)
    int nkey = npx;
    if constexpr (kMsaa) nkey = npx * a.samples;
    for (int i = tid; i < nkey; i += kRenderThreads) zb[i] = ~0ull;
    if constexpr (kShadow) {
      for (int i = tid; i < npx; i += kRenderThreads) zd[i] = ~0ull;
    }
    if (tid == 0) nbig = 0;
    if constexpr (kMsaa) {
      if (tid == 0) nmid = 0;
    }
    __syncthreads();

    // the shadow kernel alone: the lower half of the second key of the triangle this thread has set up, its colour
    // without the casting light (setup leaves it here for raster)
    uint32_t cold = 0;
    // the multisampled kernel alone: the samples raster visits, [slo, shi): all of them in phase A, one in phase B
    int slo = 0, shi = 1;
    if constexpr (kMsaa) shi = a.samples;
    // screen-space triangle: pixel x to the right, y down; depth along the camera's -z
    auto setup = [&](int t, float* sx, float* sy, float* iz, uint32_t& col, int& bx0, int& bx1, int& by0,
                     int& by1) -> bool {
      const int b = a.tri_body[t];
      float pw[3][3];
      bool ok = true;
#pragma unroll
      for (int v = 0; v < 3; v++) {
        const float4 q = a.tri[3 * t + v];
        const float* R = frm[b];
        float w[3];
        w[0] = R[0] * q.x + R[1] * q.y + R[2] * q.z + R[9];
        w[1] = R[3] * q.x + R[4] * q.y + R[5] * q.z + R[10];
        w[2] = R[6] * q.x + R[7] * q.y + R[8] * q.z + R[11];
        const float d[3] = {w[0] - cv.pos[0], w[1] - cv.pos[1], w[2] - cv.pos[2]};
        const float cx = cmat[0] * d[0] + cmat[3] * d[1] + cmat[6] * d[2];
        const float cy = cmat[1] * d[0] + cmat[4] * d[1] + cmat[7] * d[2];
        const float cz = cmat[2] * d[0] + cmat[5] * d[1] + cmat[8] * d[2];
        const float depth = -cz;
        ok = ok && depth > lc.znear;
        const float id = 1.f / depth;
        sx[v] = (cx * id / (th * aspect) * 0.5f + 0.5f) * (float)W;
        sy[v] = (0.5f - cy * id / th * 0.5f) * (float)H;
        iz[v] = id;
#pragma unroll
        for (int k = 0; k < 3; k++) pw[v][k] = w[k];
      }
      if (!ok) return false;
      const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
      if (!(fabsf(area) > 1e-12f)) return false;
      if constexpr (kMsaa) {
        // every pixel one of whose samples the triangle can cover
        bx0 = max(0, (int)floorf(fminf(sx[0], fminf(sx[1], sx[2])) - 0.5f - oxhi));
        bx1 = min(W - 1, (int)ceilf(fmaxf(sx[0], fmaxf(sx[1], sx[2])) - 0.5f - oxlo));
        by0 = max(y0, (int)floorf(fminf(sy[0], fminf(sy[1], sy[2])) - 0.5f - oyhi));
        by1 = min(y1 - 1, (int)ceilf(fmaxf(sy[0], fmaxf(sy[1], sy[2])) - 0.5f - oylo));
      } else {
        bx0 = max(0, (int)floorf(fminf(sx[0], fminf(sx[1], sx[2])) - 0.5f));
        bx1 = min(W - 1, (int)ceilf(fmaxf(sx[0], fmaxf(sx[1], sx[2])) - 0.5f));
        by0 = max(y0, (int)floorf(fminf(sy[0], fminf(sy[1], sy[2])) - 0.5f));
        by1 = min(y1 - 1, (int)ceilf(fmaxf(sy[0], fmaxf(sy[1], sy[2])) - 0.5f));
      }
      if (bx0 > bx1 || by0 > by1) return false;
      uint32_t base;
      if constexpr (kView) base = cv.rgb[a.material[t]];
      else if constexpr (kAux) base = a.views ? cv.rgb[a.material[t]] : a.tri_rgb[t];
      else base = a.tri_rgb[t];
      col = shade(cv, lc.nlight, cmat, pw[0], pw[1], pw[2], base);
      if constexpr (kAux) col = (col << 8) | (a.label ? (uint32_t)a.label[t] : 0u);   // the key's lower half
      if constexpr (kShadow)
        cold = (shade(vd.v, lc.nlight, cmat, pw[0], pw[1], pw[2], base) << 8) | (col & 0xFFu);
      return true;
    };
    // one pixel of a set-up triangle: edge functions at the pixel centre, perspective-correct depth
    auto raster = [&](const float* sx, const float* sy, const float* iz, uint32_t col, int x, int y) {
      if constexpr (kMsaa) {
        // the same rules at each sample point of [slo, shi), each with its own key in its plane of zb
        for (int s = slo; s < shi; s++) {
          const float px = (float)x + 0.5f + a.ox[s], py = (float)y + 0.5f + a.oy[s];
          const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
          const float w0 = (sx[2] - sx[1]) * (py - sy[1]) - (sy[2] - sy[1]) * (px - sx[1]);
          const float w1 = (sx[0] - sx[2]) * (py - sy[2]) - (sy[0] - sy[2]) * (px - sx[2]);
          const float w2 = (sx[1] - sx[0]) * (py - sy[0]) - (sy[1] - sy[0]) * (px - sx[0]);
          const float sg = area > 0.f ? 1.f : -1.f;
          if (w0 * sg < 0.f || w1 * sg < 0.f || w2 * sg < 0.f) continue;
          const float inv = 1.f / area;
          const float izp = (w0 * iz[0] + w1 * iz[1] + w2 * iz[2]) * inv;
          if (!(izp > 0.f)) continue;
          const float depth = 1.f / izp;
          const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | col;
          atomicMin(&zb[s * npx + (y - y0) * W + x], key);
        }
        return;
      }
      const float px = (float)x + 0.5f, py = (float)y + 0.5f;
      const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
      const float w0 = (sx[2] - sx[1]) * (py - sy[1]) - (sy[2] - sy[1]) * (px - sx[1]);
      const float w1 = (sx[0] - sx[2]) * (py - sy[2]) - (sy[0] - sy[2]) * (px - sx[2]);
      const float w2 = (sx[1] - sx[0]) * (py - sy[0]) - (sy[1] - sy[0]) * (px - sx[0]);
      const float sg = area > 0.f ? 1.f : -1.f;
      if (w0 * sg < 0.f || w1 * sg < 0.f || w2 * sg < 0.f) return;
      const float inv = 1.f / area;
      const float izp = (w0 * iz[0] + w1 * iz[1] + w2 * iz[2]) * inv;
      if (!(izp > 0.f)) return;
      const float depth = 1.f / izp;
      const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | col;
      atomicMin(&zb[(y - y0) * W + x], key);
      if constexpr (kShadow)
        atomicMin(&zd[(y - y0) * W + x], ((unsigned long long)__float_as_uint(depth) << 32) | cold);
    };

    // A band is drawn in rounds of phase A and phase B; one round unless a list fills.  A listed triangle is always
    // drawn by phase B: a thread whose triangle a full list refuses ends its phase A there and takes it up again in
    // the next round (tnext), after phase B has emptied the lists.  Which triangles the atomics refuse therefore
    // changes no key: the two phases' arithmetic is contracted differently, and a refused triangle drawn by its own
    // thread would carry phase A's depth bits into the image (DESIGN.md 3.7 "Synthetic meshes")
    int tnext = tid;
    for (;;) {
    // ---- phase A: one triangle per thread; large ones are listed for phase B
    int t = tnext;
    for (; t < a.ntri; t += kRenderThreads) {
      float sx[3], sy[3], iz[3];
      uint32_t col;
      int bx0, bx1, by0, by1;
      if (!setup(t, sx, sy, iz, col, bx0, bx1, by0, by1)) continue;
      int boxpx = (bx1 - bx0 + 1) * (by1 - by0 + 1);
      if constexpr (kMsaa) boxpx *= a.samples;              // the keys the triangle can touch
      if constexpr (kMsaa) {
        // two lists in big[]: triangles of >= kWideKeys keys from the front (all threads each), the others from the
        // back (a wave each)
        if (boxpx >= kWideKeys) {
          const int k = atomicAdd(&nbig, 1);
          if (k < kBigCap) { big[k] = t; continue; }
          break;
        } else if (boxpx > kBigPx) {
          const int k = atomicAdd(&nmid, 1);
          if (k < kCap - kBigCap) { big[kCap - 1 - k] = t; continue; }
          break;
        }
      } else if (boxpx > kBigPx) {
        const int k = atomicAdd(&nbig, 1);
        if (k < kCap) { big[k] = t; continue; }
        break;
      }
      for (int y = by0; y <= by1; y++)
        for (int x = bx0; x <= bx1; x++) raster(sx, sy, iz, col, x, y);
    }
    tnext = t;
    __syncthreads();
    // the lists' lengths of this round, read by every thread before thread 0 may reset them (uniform)
    const int nlisted = nbig;
    int nmlisted = 0;
    if constexpr (kMsaa) nmlisted = nmid;
    // ---- phase B: each large triangle with all threads over its bbox
    int nb = min(nlisted, kCap);
    if constexpr (kMsaa) nb = min(nlisted, kBigCap);        // the wide list
    for (int k = 0; k < nb; k++) {
      float sx[3], sy[3], iz[3];
      uint32_t col;
      int bx0, bx1, by0, by1;
      if (!setup(big[k], sx, sy, iz, col, bx0, bx1, by0, by1)) continue;   // uniform: same triangle
      const int bw = bx1 - bx0 + 1, cnt = bw * (by1 - by0 + 1);
      if constexpr (kMsaa) {
        // all threads over (sample, box pixel), the pixel fastest: a wave's atomics go to consecutive keys of one plane
        for (int i = tid; i < cnt * a.samples; i += kRenderThreads) {
          const int s = i / cnt, j = i - s * cnt;
          slo = s; shi = s + 1;
          raster(sx, sy, iz, col, bx0 + j % bw, by0 + j / bw);
        }
        continue;
      }
      for (int i = tid; i < cnt; i += kRenderThreads) raster(sx, sy, iz, col, bx0 + i % bw, by0 + i / bw);
    }
    if constexpr (kMsaa) {
      // the other list: a triangle per wave, its lanes over (sample, box pixel).  These are a few wavefuls of keys each,
      // and setting one up in every thread of the block costs more than drawing it
      const int nm = min(nmlisted, kCap - kBigCap);
      for (int k = tid / kWave; k < nm; k += kRenderThreads / kWave) {
        float sx[3], sy[3], iz[3];
        uint32_t col;
        int bx0, bx1, by0, by1;
        if (!setup(big[kCap - 1 - k], sx, sy, iz, col, bx0, bx1, by0, by1)) continue;   // uniform per wave
        const int bw = bx1 - bx0 + 1, cnt = bw * (by1 - by0 + 1);
        for (int i = tid % kWave; i < cnt * a.samples; i += kWave) {
          const int s = i / cnt, j = i - s * cnt;
          slo = s; shi = s + 1;
          raster(sx, sy, iz, col, bx0 + j % bw, by0 + j / bw);
        }
      }
    }
    __syncthreads();
    // another round when a list refused triangles (uniform: every thread read the same lengths)
    bool more = nlisted > kCap;
    if constexpr (kMsaa) more = nlisted > kBigCap || nmlisted > kCap - kBigCap;
    if (!more) break;
    if (tid == 0) nbig = 0;
    if constexpr (kMsaa) {
      if (tid == 0) nmid = 0;
    }
    __syncthreads();
    }
    if constexpr (kMsaa) {
      // ---- the resolve: per pixel and channel (sum of the S samples' bytes + S / 2) / S, an empty sample 0.  The result
      // goes to plane 0 as a key with the colour in its place and the upper half 0 (never the empty key), which the
      // sinks below read as they read any band.  Thread i touches keys i, npx + i, ... alone: no barrier in between
      const int sh = a.samples >> 1;                           // log2 S of 1, 2, 4
      for (int i = tid; i < npx; i += kRenderThreads) {
        uint32_t r = 0, g = 0, b = 0;
        for (int s = 0; s < a.samples; s++) {
          const unsigned long long key = zb[s * npx + i];
          const uint32_t c = key == ~0ull ? 0u : (uint32_t)key >> kColShift;
          r += c & 0xFFu; g += (c >> 8) & 0xFFu; b += (c >> 16) & 0xFFu;
        }
        const uint32_t h = (uint32_t)a.samples >> 1;
        r = (r + h) >> sh; g = (g + h) >> sh; b = (b + h) >> sh;
        zb[i] = (unsigned long long)((r | (g << 8) | (b << 16)) << kColShift);
      }
      __syncthreads();
    }
    if constexpr (kShadow) {
#pragma clang fp contract(off)
      auto dotp = [](const float* p, const float* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
      // ---- the shadow test, once per pixel with a winning key: the point the pixel's centre sees at the key's depth,
      // looked up in the map without filtering.  An occluded pixel takes the dark key's colour (depth and label stay
      // the key's own); zd then holds the pixel's 0 / 1 for the shadow sink
      const int S = a.map_size;
      const float sc = 0.5f / a.radius;
      for (int i = tid; i < npx; i += kRenderThreads) {
        const unsigned long long key = zb[i];
        bool dark = false;
        if (a.light >= 0 && key != ~0ull) {
          const int y = y0 + i / W, x = i - (i / W) * W;
          const float depth = __uint_as_float((uint32_t)(key >> 32));
          const float xn = (((float)x + 0.5f) / (float)W - 0.5f) * 2.f * th * aspect;
          const float yn = (0.5f - ((float)y + 0.5f) / (float)H) * 2.f * th;
          float p[3];
#pragma unroll
          for (int k = 0; k < 3; k++)
            p[k] = cv.pos[k] + depth * (cmat[3 * k] * xn + cmat[3 * k + 1] * yn - cmat[3 * k + 2]) - a.center[k];
          const float fa = floorf((dotp(p, sf.u) * sc + 0.5f) * (float)S);
          const float fb = floorf((dotp(p, sf.v) * sc + 0.5f) * (float)S);
          if (fa >= 0.f && fa < (float)S && fb >= 0.f && fb < (float)S) {       // false for NaN
            const uint32_t e = smap[(int)fb * S + (int)fa];
            dark = e != kShadowEmpty && shadow_decode(e) < dotp(p, sf.d) - a.bias;
          }
        }
        if (dark) zb[i] = (key & ~0xFFFFFF00ull) | (zd[i] & 0xFFFFFF00ull);
        zd[i] = dark ? 1ull : 0ull;
      }
      __syncthreads();
    }
    // ---- band -> image (background: black)
    if constexpr (!kSinks) {
      for (int i = tid; i < npx; i += kRenderThreads) {
        const unsigned long long key = zb[i];
        const uint32_t col = key == ~0ull ? 0u : (uint32_t)(key & 0xFFFFFFu);
        uint8_t* px = img + ((size_t)y0 * W + i) * 3;
        px[0] = (uint8_t)(col & 0xFFu);
        px[1] = (uint8_t)((col >> 8) & 0xFFu);
        px[2] = (uint8_t)((col >> 16) & 0xFFu);
      }
    } else {
      // channel c of band pixel i (background: 0)
      auto chan = [&](int i, int c) -> uint32_t {
        const unsigned long long key = zb[i];
        return key == ~0ull ? 0u : ((uint32_t)key >> (8 * c + kColShift)) & 0xFFu;
      };
      if (a.out) {                                            // uniform per launch
        for (int i = tid; i < npx; i += kRenderThreads) {
          uint8_t* px = img + ((size_t)y0 * W + i) * 3;
          px[0] = (uint8_t)chan(i, 0);
          px[1] = (uint8_t)chan(i, 1);
          px[2] = (uint8_t)chan(i, 2);
        }
      }
      if (a.chw) {
        // a band is whole rows: within plane c it is the span [p, p + npx).  Bytes up to the first 4-byte aligned
        // address and after the last whole dword go out one by one, the rest as dwords of four pixels' channel bytes;
        // nothing outside the span is touched (its neighbours are other planes, other envs or the caller's memory)
#pragma unroll 1
        for (int c = 0; c < 3; c++) {
          uint8_t* p = a.chw + ((slot() * 3 + c) * H + y0) * W;
          const int head = min(npx, (int)((4u - (uint32_t)((uintptr_t)p & 3u)) & 3u));
          const int nquad = (npx - head) >> 2;
          const int tail = head + 4 * nquad;
          uint32_t* q = (uint32_t*)(p + head);                // 4-byte aligned (unused when nquad == 0)
          for (int k = tid; k < nquad; k += kRenderThreads) {
            const int i = head + 4 * k;
            q[k] = chan(i, c) | (chan(i + 1, c) << 8) | (chan(i + 2, c) << 16) | (chan(i + 3, c) << 24);
          }
          if (tid < head) p[tid] = (uint8_t)chan(tid, c);     // head < 4
          if (tid < npx - tail) p[tail + tid] = (uint8_t)chan(tail + tid, c);   // npx - tail < 4
        }
      }
      if (a.flat) {
        // float j of the band = byte j of its hwc form: consecutive threads store consecutive floats
        static constexpr ByteUnit kByteUnit{};
        float* f = a.flat + (size_t)env * (size_t)a.flat_pitch + (size_t)y0 * W * 3;
        if constexpr (kCams) f += (size_t)blockIdx.y * 3 * H * W;      // camera c's floats within the env's row
        for (int j = tid; j < 3 * npx; j += kRenderThreads) {
          const int i = j / 3;
          f[j] = kByteUnit.v[chan(i, j - 3 * i)];
        }
      }
      if constexpr (kAux) {
        if (a.depth) {
          // the float32 the depth test compared: the key's upper half as it is (the empty key gives 0.0f)
          float* d = a.depth + (slot() * H + y0) * W;
          for (int i = tid; i < npx; i += kRenderThreads) {
            const unsigned long long key = zb[i];
            d[i] = key == ~0ull ? 0.f : __uint_as_float((uint32_t)(key >> 32));
          }
        }
        if (a.seg) {
          // the key's low byte (the empty key's is 255, the background label); the chw plane's head / dword / tail
          // scheme on the band's span [p, p + npx): nothing outside it is touched
          uint8_t* p = a.seg + (slot() * H + y0) * W;
          const int head = min(npx, (int)((4u - (uint32_t)((uintptr_t)p & 3u)) & 3u));
          const int nquad = (npx - head) >> 2;
          const int tail = head + 4 * nquad;
          uint32_t* q = (uint32_t*)(p + head);                // 4-byte aligned (unused when nquad == 0)
          auto lab = [&](int i) -> uint32_t { return (uint32_t)zb[i] & 0xFFu; };
          for (int k = tid; k < nquad; k += kRenderThreads) {
            const int i = head + 4 * k;
            q[k] = lab(i) | (lab(i + 1) << 8) | (lab(i + 2) << 16) | (lab(i + 3) << 24);
          }
          if (tid < head) p[tid] = (uint8_t)lab(tid);         // head < 4
          if (tid < npx - tail) p[tail + tid] = (uint8_t)lab(tail + tid);   // npx - tail < 4
        }
      }
      if constexpr (kShadow) {
        if (a.shadow) {
          // the pixel's 0 / 1 left in zd, with the seg plane's head / dword / tail scheme on the band's span
          uint8_t* p = a.shadow + (slot() * H + y0) * W;
          const int head = min(npx, (int)((4u - (uint32_t)((uintptr_t)p & 3u)) & 3u));
          const int nquad = (npx - head) >> 2;
          const int tail = head + 4 * nquad;
          uint32_t* q = (uint32_t*)(p + head);                // 4-byte aligned (unused when nquad == 0)
          auto bit = [&](int i) -> uint32_t { return (uint32_t)zd[i]; };
          for (int k = tid; k < nquad; k += kRenderThreads) {
            const int i = head + 4 * k;
            q[k] = bit(i) | (bit(i + 1) << 8) | (bit(i + 2) << 16) | (bit(i + 3) << 24);
          }
          if (tid < head) p[tid] = (uint8_t)bit(tid);         // head < 4
          if (tid < npx - tail) p[tail + tid] = (uint8_t)bit(tail + tid);   // npx - tail < 4
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace so100
