// so100_render_views.hip - the render launch with a view record per env (C-ABI so100_render_views): the kernel of
// so100_render.hip (same body, so100_render.h: bands, phases A and B, 64-bit depth keys, the three sinks, the mask) whose
// camera pose, field of view, headlight terms, light directions and diffuses and base colours come from views[env],
// loaded into LDS once per workgroup by threads 0-39.  A translation unit of its own: the other two kernels stay the
// code they were.
#include "so100_render.h"

namespace so100 {

hipError_t launch_render_views(const DevModel* m, const float4* tri, const int* body, const uint8_t* material, int ntri,
                               const float* qpos, const uint8_t* mask, const so100_camera& cam, const so100_view* views,
                               int n, int width, int height, const so100_image_out& o, hipStream_t s) {
  RenderViewArgs a{};
  a.m = m; a.tri = tri; a.tri_body = body; a.tri_rgb = nullptr; a.ntri = ntri;
  a.qpos = qpos; a.mask = mask; a.cam = cam; a.n = n; a.width = width; a.height = height;
  a.out = o.hwc; a.chw = o.chw; a.flat = o.flat; a.flat_pitch = (long long)o.flat_pitch;
  a.views = views; a.material = material;
  hipLaunchKernelGGL(so100_render_kernel<RenderViewArgs>, dim3(a.n), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
