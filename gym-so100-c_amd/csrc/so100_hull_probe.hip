// so100_hull_probe.hip - the hull support of the convex collider on its own (C-ABI so100_hull_support_probe): the
// step kernels' hull_support (so100_convex.h), through the direction cells' block table or by the whole-hull scan, for
// a list of directions.  A test probe: tests/test_gpu_hull_support.py holds the two paths to the same vertex, bit for
// bit, and both to the first maximal vertex of the fp32 FMA scores.
#include "so100_convex.h"

namespace so100 {

constexpr int kProbeDirs = 16;   // directions per workgroup: its 4 rows take 4 each, one after the other

__global__ void __launch_bounds__(kThreads) so100_hull_support_probe_kernel(const DevModel* __restrict__ m, int k,
                                                                            const float* __restrict__ dirs, int n,
                                                                            int cells, float4* __restrict__ out) {
  const int lane = (int)threadIdx.x & (kLanes - 1), grp = (int)threadIdx.x / kLanes;
  const int s0 = m->hull_start[k], cnt = m->hull_count[k];
  for (int j = 0; j < kProbeDirs / kEnvsPerBlock; j++) {
    const int i = (int)blockIdx.x * kProbeDirs + grp * (kProbeDirs / kEnvsPerBlock) + j;
    const int ii = min(i, n - 1);      // (a row past the end repeats the last direction: the whole row stays active)
    const float n0 = dirs[3 * ii], n1 = dirs[3 * ii + 1], n2 = dirs[3 * ii + 2];
    const float4 v = cells == 1   ? hull_support(m, kSupBlock, k, s0, cnt, n0, n1, n2, lane)
                     : cells == 2 ? hull_support(m, kSupCells, k, s0, cnt, n0, n1, n2, lane)
                                  : hull_support(m, kSupScan, k, s0, cnt, n0, n1, n2, lane);
    if (i < n && lane == 0) out[i] = v;
  }
}

hipError_t launch_hull_support_probe(const DevModel* m, int hull, const float* dirs, int n, int cells, float* out,
                                     hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(so100_hull_support_probe_kernel, dim3((n + kProbeDirs - 1) / kProbeDirs), dim3(kThreads), 0, s, m,
                     hull, dirs, n, cells, reinterpret_cast<float4*>(out));
  return hipGetLastError();
}

}  // namespace so100
