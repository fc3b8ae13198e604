// so100_render_msaa.hip - the multisampled render launch (C-ABI so100_render_msaa): the kernel of
// so100_render_cams.hip (same body, so100_render.h, on the grid dim3(n, ncam), with views, body-mounted cameras and the
// mask) whose pixels hold S = 1, 2 or 4 keys, one per sample point.  A triangle is set up and shaded once; coverage, depth
// and the key's atomicMin are evaluated at every sample.  After a band's two raster phases the samples' colours are
// averaged in LDS, round half up, and the three colour sinks read the resolved byte: only W x H bytes leave the chip
// (DESIGN.md 3.7 "Anti-aliasing").  It has no depth or label sink.  A translation unit of its own: the other six kernels
// stay the code they were.
#include "so100_render.h"

namespace so100 {

static_assert(sizeof(RenderMsaaArgs) <= 4096, "kernel arguments: 4 KB");

hipError_t launch_render_msaa(const DevModel* m, const float4* tri, const int* body, const uint32_t* rgb,
                              const uint8_t* material, int ntri, const float* qpos, const uint8_t* mask,
                              const so100_cams& cams, const so100_view* views, int n, int width, int height,
                              const so100_image_out& o, const so100_msaa& ms, hipStream_t s) {
  RenderMsaaArgs a{};
  a.m = m; a.tri = tri; a.tri_body = body; a.tri_rgb = rgb; a.ntri = ntri;
  a.qpos = qpos; a.mask = mask; a.n = n; a.width = width; a.height = height;
  a.out = o.hwc; a.chw = o.chw; a.flat = o.flat; a.flat_pitch = (long long)o.flat_pitch;
  a.views = views; a.material = material;
  a.label = nullptr; a.depth = nullptr; a.seg = nullptr;
  a.ncam = cams.ncam;
  for (int c = 0; c < cams.ncam; c++) { a.cams[c] = cams.cam[c]; a.frame_body[c] = cams.frame_body[c]; }
  a.samples = ms.samples;
  for (int k = 0; k < ms.samples; k++) { a.ox[k] = ms.offset[k][0]; a.oy[k] = ms.offset[k][1]; }
  hipLaunchKernelGGL(so100_render_kernel<RenderMsaaArgs>, dim3(a.n, a.ncam), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
