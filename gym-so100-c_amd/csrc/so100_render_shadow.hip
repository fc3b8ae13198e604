// so100_render_shadow.hip - the render launch with cast shadows (C-ABI so100_render_shadow): the kernel of
// so100_render_cams.hip (same body, so100_render.h, on the grid dim3(n, ncam)) whose blocks first draw the caster
// triangles into an orthographic depth map along one light, S x S texels in LDS, and keep beside each pixel's key a
// second one shaded without that light.  After a band's two raster phases every pixel with a winning key is looked up
// in the map once; an occluded pixel takes the second key's colour, so the colour sinks are
// where(shadow, dark, full) of two so100_render_cams images bit for bit, and depth and labels are that launch's
// (DESIGN.md 3.7 "Shadows").  A translation unit of its own: the other five kernels stay the code they were.
#include "so100_render.h"

namespace so100 {

static_assert(sizeof(RenderShadowArgs) <= 4096, "kernel arguments: 4 KB");

hipError_t launch_render_shadow(const DevModel* m, const float4* tri, const int* body, const uint32_t* rgb,
                                const uint8_t* material, const uint8_t* label, const uint8_t* caster, int ntri,
                                const float* qpos, const uint8_t* mask, const so100_cams& cams, const so100_view* views,
                                int n, int width, int height, const so100_image_out& o, const so100_aux_out& x,
                                const so100_shadow& sh, hipStream_t s) {
  RenderShadowArgs a{};
  a.m = m; a.tri = tri; a.tri_body = body; a.tri_rgb = rgb; a.ntri = ntri;
  a.qpos = qpos; a.mask = mask; a.n = n; a.width = width; a.height = height;
  a.out = o.hwc; a.chw = o.chw; a.flat = o.flat; a.flat_pitch = (long long)o.flat_pitch;
  a.views = views; a.material = material;
  a.label = label; a.depth = x.depth; a.seg = x.label;
  a.ncam = cams.ncam;
  for (int c = 0; c < cams.ncam; c++) { a.cams[c] = cams.cam[c]; a.frame_body[c] = cams.frame_body[c]; }
  a.caster = caster; a.light = sh.light; a.map_size = sh.map_size;
  for (int k = 0; k < 3; k++) a.center[k] = sh.center[k];
  a.radius = sh.radius; a.bias = sh.bias; a.shadow = sh.shadow_out;
  hipLaunchKernelGGL(so100_render_kernel<RenderShadowArgs>, dim3(a.n, a.ncam), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
