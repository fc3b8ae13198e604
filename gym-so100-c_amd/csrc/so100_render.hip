// so100_render.hip — batched camera images: the reference's default observation
// (obs_type="so100_pixels_agent_pos", gym_so100/__init__.py:4-32), the `top` camera rendered by
// dm_control's physics.render (gym_so100/env.py:84-94,130-136; scene_so100.xml:30), SURVEY §8 f.3.
//
// MuJoCo renders with OpenGL; this is a rasteriser of our own on the same scene description: the
// visible geoms (tools/compile_render.py: the arm's visual meshes, decimated, the table, bin and cube
// boxes, with their colours), the camera pose and field of view, the headlight and the scene's
// directional lights (Lambert diffuse + ambient, two-sided, flat per triangle; no specular; this launch has
// no shadows or anti-aliasing: so100_render_shadow.hip and so100_render_msaa.hip).  It reproduces what is where in the image, not MuJoCo's pixel values: parity with
// MuJoCo's renderer is unpinned.
//
// Layout: one 256-thread workgroup per env.
//   * thread 0 runs the stage kernel's forward kinematics (so100_kin.h) into LDS, 9 body frames;
//   * the image is drawn in bands of up to kTilePx pixels; per band, an LDS depth buffer of 64-bit keys
//     (depth bits << 32 | RGB8) takes ds_min_u64 atomics, so the nearest surface wins and equal depths
//     resolve to the smaller colour: the image does not depend on thread order;
//   * phase A: thread t projects triangles t, t+256, ... and rasterises the small ones itself; triangles
//     covering more than kBigPx pixels of the band go to an LDS list and phase B rasterises each with all
//     256 threads (the table's two faces cover the whole image: one thread would serialise the block);
//   * the band -> image phase writes the band from LDS to every sink the caller gave (so100_render_to): the
//     [H][W][3] bytes, the channel-first [3][H][W] bytes SB3's image policies take, and the flattened float32
//     bytes / 255 of the reference's GoalEnv observation (env.py:267-270).  One rasterisation, several layouts.
#include "so100_render.h"

namespace so100 {

hipError_t launch_render_sinks(const RenderSinkArgs& a, hipStream_t s);      // so100_render_sinks.hip

hipError_t launch_render(const DevModel* m, const float4* tri, const int* body, const uint32_t* rgb, int ntri,
                         const float* qpos, const uint8_t* mask, const so100_camera& cam, int n, int width, int height,
                         const so100_image_out& o, hipStream_t s) {
  RenderArgs a{m, tri, body, rgb, ntri, qpos, mask, cam, n, width, height, o.hwc};
  if (o.chw || o.flat) return launch_render_sinks(RenderSinkArgs{a, o.chw, o.flat, (long long)o.flat_pitch}, s);
  hipLaunchKernelGGL(so100_render_kernel<RenderArgs>, dim3(n), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
