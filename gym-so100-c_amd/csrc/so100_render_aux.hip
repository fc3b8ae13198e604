// so100_render_aux.hip - the render launch with the depth and label sinks (C-ABI so100_render_aux): the kernel of
// so100_render.hip (same body, so100_render.h: bands, phases A and B, the mask, the three colour sinks) whose 64-bit
// key is depth bits << 32 | RGB8 << 8 | label, so the band -> image phase can also write the float32 depth the depth
// test compared and the winning triangle's label.  With views it draws each env from views[env] as so100_render_views
// does; without, the LDS record is filled from the launch's camera and the colours are the mesh's.  A translation unit
// of its own: the other three kernels stay the code they were.
#include "so100_render.h"

namespace so100 {

hipError_t launch_render_aux(const DevModel* m, const float4* tri, const int* body, const uint32_t* rgb,
                             const uint8_t* material, const uint8_t* label, int ntri, const float* qpos,
                             const uint8_t* mask, const so100_camera& cam, const so100_view* views, int n, int width,
                             int height, const so100_image_out& o, const so100_aux_out& x, hipStream_t s) {
  RenderAuxArgs a{};
  a.m = m; a.tri = tri; a.tri_body = body; a.tri_rgb = rgb; a.ntri = ntri;
  a.qpos = qpos; a.mask = mask; a.cam = cam; a.n = n; a.width = width; a.height = height;
  a.out = o.hwc; a.chw = o.chw; a.flat = o.flat; a.flat_pitch = (long long)o.flat_pitch;
  a.views = views; a.material = material;
  a.label = label; a.depth = x.depth; a.seg = x.label;
  hipLaunchKernelGGL(so100_render_kernel<RenderAuxArgs>, dim3(a.n), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
