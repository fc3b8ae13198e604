// so100_render_sinks.hip - the render launch with further sinks (C-ABI so100_render_to): the kernel of so100_render.hip
// (same body, so100_render.h) whose band -> image phase also writes the channel-first image and the flattened float32
// image / 255.  A translation unit of its own: the hwc-only kernel of so100_render.hip stays the code it was.
#include "so100_render.h"

namespace so100 {

hipError_t launch_render_sinks(const RenderSinkArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(so100_render_kernel<RenderSinkArgs>, dim3(a.n), dim3(kRenderThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace so100
