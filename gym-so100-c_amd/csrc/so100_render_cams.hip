// so100_render_cams.hip - the render launch over (env, camera) (C-ABI so100_render_cams): the kernel of
// so100_render_aux.hip (same body, so100_render.h: bands, phases A and B, the mask, the five sinks, views or not) on a
// grid of dim3(n, ncam).  Block (env, c) draws env from cams[c] and views[c * n + env] into slot env * ncam + c of every
// sink; a camera with frame_body[c] > 0 rides on that body: thread 0 takes its position (and, without tracking, its
// frame) from the body's frame to the world after the kinematics.  Each block repeats its env's forward kinematics
// (DESIGN.md 3.7 "Cameras").  A translation unit of its own: the other four kernels stay the code they were.
#include "so100_render.h"

namespace so100 {

static_assert(sizeof(RenderCamsArgs) <= 4096, "kernel arguments: 4 KB");

hipError_t launch_render_cams(const DevModel* m, const float4* tri, const int* body, const uint32_t* rgb,
                              const uint8_t* material, const uint8_t* label, int ntri, const float* qpos,
                              const uint8_t* mask, const so100_cams& cams, const so100_view* views, int n, int width,
                              int height, const so100_image_out& o, const so100_aux_out& x, hipStream_t s) {
  RenderCamsArgs a{};
  a.m = m; a.tri = tri; a.tri_body = body; a.tri_rgb = rgb; a.ntri = ntri;
  a.qpos = qpos; a.mask = mask; a.n = n; a.width = width; a.height = height;
  a.out = o.hwc; a.chw = o.chw; a.flat = o.flat; a.flat_pitch = (long long)o.flat_pitch;
  a.views = views; a.material = material;
  a.label = label; a.depth = x.depth; a.seg = x.label;
  a.ncam = cams.ncam;
  for (int c = 0; c < cams.ncam; c++) { a.cams[c] = cams.cam[c]; a.frame_body[c] = cams.frame_body[c]; }
  hipLaunchKernelGGL(so100_render_kernel<RenderCamsArgs>, dim3(a.n, a.ncam), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
