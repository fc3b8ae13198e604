// so100_norm.hip - running observation / reward normalisation on the device (C-ABI so100_norm_update, so100_norm_apply,
// so100_norm_return): SB3 VecNormalize's running mean / variance in float64, kept and used without a
// host synchronisation.  New launches beside the untouched step kernel: they read what the step wrote (obs, reward, the
// done flags) and write tensors of their own.
//
// Moments.  A workgroup is 256 threads = 32 column slots x 8 row slots (column = thread & 31, so lanes l and l + 32 of
// a wave hold the same column and a row's columns are one contiguous run of floats).  It reduces a contiguous range of
// rows to per-column (b, sum (x - c), sum (x - c)^2) in float64, c the current running mean (so the squares do not
// cancel): the two halves of a wave by one __shfl_xor, the four waves through LDS in wave order, and writes the three
// numbers to its slot of the workspace.  Below the cap a workgroup takes kNormRows = 128 rows (16 loads per thread in
// flight); the grid is capped at kNormMaxGroups = 256 workgroups, one per CU of the chip: more workgroups add no
// parallelism, and the merge reads every partial, so its serial length grows with the grid.  Past 32,768 rows each
// workgroup's range grows instead (its row loop runs longer).
//
// Merge.  One workgroup, launched after the moments on the same stream (the launch boundary orders partials -> merge
// -> normalise; nothing waits inside a launch, there is no atomic on the statistics).  Thread (column, slot) adds the
// partials of an eighth of the workgroups in index order, the eight slot sums are added in slot order, and the column's
// thread applies the update formula.  The association is a function of the row count alone, so the statistics are bit
// for bit the same from run to run.  b = 0 leaves the statistics untouched.
//
// Apply.  One thread per element: y = clip((x - mean) / sqrt(var + eps)) in float64, rounded once to float32; with a row
// mask only the masked rows are written (the final observation).  The inverse flag computes x = y sqrt(var + eps) + mean.
//
// Return.  ret <- ret gamma + reward and its moments in one launch (one thread per env, a full wave reduction), the
// shared merge, then reward_norm and the zeroing of ret at done in a third.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"

namespace so100 {

constexpr int kNormThreads = 256;
constexpr int kNormCols = SO100_NORM_MAX_DIM;           // column slots
constexpr int kNormSlots = kNormThreads / kNormCols;    // row slots
constexpr int kNormRows = 128;                          // rows per workgroup below the cap
constexpr int kNormMaxGroups = 256;                     // the grid cap
constexpr int kNormPart = 3 * kNormCols;                // doubles per workgroup in the workspace: b, s1, s2 [32] each
static_assert(kNormCols == 32 && kNormSlots == 8, "column = thread & 31: the two halves of a wave hold the same columns");

int norm_groups(int n) {
  const int g = (n + kNormRows - 1) / kNormRows;
  return g < 1 ? 1 : (g > kNormMaxGroups ? kNormMaxGroups : g);
}
int norm_rows_per_group() { return kNormRows; }
int norm_max_groups() { return kNormMaxGroups; }

// the sources of one call, flattened (no runtime-indexed array in the kernel arguments: selects only)
struct NormArgs {
  const float* x0; const float* x1; const float* x2;
  float* y0; float* y1; float* y2;
  int stride0, stride1, stride2;
  int off0, off1, off2;          // column offset in the source row, less the source's first column slot
  int ystride0, ystride1, ystride2;
  int end0, end1;                // column slots [0, end0) are source 0, [end0, end1) source 1, [end1, D) source 2
  int D;
  int n;
  int rows;                      // rows per workgroup
  const uint8_t* mask;           // [n] or null
  double epsilon;
  float clip;
  int inverse;
};

// (b, s1, s2) of this thread -> the workgroup's sums per column slot, W lanes apart: W = 32 the observation layout,
// W = 1 one column over all lanes.  Written by threads [0, W) to part[0..2][column].
template <int W>
__device__ __forceinline__ void norm_block_reduce(double b, double s1, double s2, double* __restrict__ part) {
  __shared__ double red[kNormThreads / 64][W][3];
#pragma unroll
  for (int off = 32; off >= W; off >>= 1) {
    b += __shfl_xor(b, off);
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane < W) {
    red[wave][lane][0] = b;
    red[wave][lane][1] = s1;
    red[wave][lane][2] = s2;
  }
  __syncthreads();
  if ((int)threadIdx.x < W) {
    double tb = red[0][threadIdx.x][0], t1 = red[0][threadIdx.x][1], t2 = red[0][threadIdx.x][2];
#pragma unroll
    for (int w = 1; w < kNormThreads / 64; w++) {
      tb += red[w][threadIdx.x][0];
      t1 += red[w][threadIdx.x][1];
      t2 += red[w][threadIdx.x][2];
    }
    part[threadIdx.x] = tb;
    part[kNormCols + threadIdx.x] = t1;
    part[2 * kNormCols + threadIdx.x] = t2;
  }
}

__global__ __launch_bounds__(kNormThreads) void so100_norm_moments_kernel(NormArgs a, const double* __restrict__ stats,
                                                                          double* __restrict__ work) {
  const int c = (int)threadIdx.x & (kNormCols - 1), slot = (int)threadIdx.x >> 5;
  const bool live = c < a.D;
  const float* x = c < a.end0 ? a.x0 : (c < a.end1 ? a.x1 : a.x2);
  const int stride = c < a.end0 ? a.stride0 : (c < a.end1 ? a.stride1 : a.stride2);
  const int col = c + (c < a.end0 ? a.off0 : (c < a.end1 ? a.off1 : a.off2));
  const double shift = live ? stats[c] : 0.0;
  const long long r0 = (long long)blockIdx.x * a.rows;
  const long long r1 = r0 + a.rows < a.n ? r0 + a.rows : a.n;
  double b = 0.0, s1 = 0.0, s2 = 0.0;
  if (live) {
#pragma unroll 4
    for (long long r = r0 + slot; r < r1; r += kNormSlots) {
      if (a.mask != nullptr && a.mask[r] == 0) continue;
      const double v = (double)x[(size_t)r * stride + col] - shift;
      b += 1.0;
      s1 += v;
      s2 += v * v;
    }
  }
  norm_block_reduce<kNormCols>(b, s1, s2, work + (size_t)blockIdx.x * kNormPart);
}

// ret <- ret gamma + reward per env, and the moments of the new ret (column 0)
__global__ __launch_bounds__(kNormThreads) void so100_norm_ret_moments_kernel(int n, int rows, double gamma,
                                                                              const float* __restrict__ reward,
                                                                              double* __restrict__ ret,
                                                                              const double* __restrict__ stats,
                                                                              double* __restrict__ work) {
  const double shift = stats[0];
  const long long r0 = (long long)blockIdx.x * rows;
  const long long r1 = r0 + rows < n ? r0 + rows : n;
  double b = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long r = r0 + (int)threadIdx.x; r < r1; r += kNormThreads) {
#pragma clang fp contract(off)                 // ret gamma rounded, then the sum: the float64 formula as written
    const double g = ret[r] * gamma + (double)reward[r];
    ret[r] = g;
    const double v = g - shift;
    b += 1.0;
    s1 += v;
    s2 += v * v;
  }
  norm_block_reduce<1>(b, s1, s2, work + (size_t)blockIdx.x * kNormPart);
}

// The update formula of include/so100.h for one column (st[0] mean, st[32] var, st[64] count) from b > 0 rows' sums
// of (x - mean) and (x - mean)^2.  Every product is rounded on its own (no fused multiply-add): one row gives
// s2 / b - d d = 0 exactly, and the update is the formula operation for operation.
__device__ __forceinline__ void norm_update_column(double b, double s1, double s2, double* __restrict__ st) {
#pragma clang fp contract(off)
  const double mean = st[0], var = st[kNormCols], count = st[2 * kNormCols];
  const double d = s1 / b;                     // batch mean - running mean (the shift was the running mean)
  double bv = s2 / b - d * d;                  // population variance of the batch
  bv = bv < 0.0 ? 0.0 : bv;
  const double tot = count + b;
  st[0] = mean + d * b / tot;
  st[kNormCols] = (var * count + bv * b + d * d * count * b / tot) / tot;
  st[2 * kNormCols] = tot;
}

// the partials of `groups` workgroups -> the running statistics of columns [0, D): stats[0][c] mean, [1][c] var,
// [2][c] count
__global__ __launch_bounds__(kNormThreads) void so100_norm_merge_kernel(int D, int groups, const double* __restrict__ work,
                                                                        double* __restrict__ stats) {
  __shared__ double red[kNormSlots][kNormCols][3];
  const int c = (int)threadIdx.x & (kNormCols - 1), slot = (int)threadIdx.x >> 5;
  const int per = (groups + kNormSlots - 1) / kNormSlots;
  const int g0 = slot * per, g1 = g0 + per < groups ? g0 + per : groups;
  double b = 0.0, s1 = 0.0, s2 = 0.0;
  if (c < D) {
#pragma unroll 4
    for (int g = g0; g < g1; g++) {
      const double* p = work + (size_t)g * kNormPart + c;
      b += p[0];
      s1 += p[kNormCols];
      s2 += p[2 * kNormCols];
    }
  }
  red[slot][c][0] = b;
  red[slot][c][1] = s1;
  red[slot][c][2] = s2;
  __syncthreads();
  if ((int)threadIdx.x >= D) return;
  b = red[0][c][0], s1 = red[0][c][1], s2 = red[0][c][2];
#pragma unroll
  for (int s = 1; s < kNormSlots; s++) {
    b += red[s][c][0];
    s1 += red[s][c][1];
    s2 += red[s][c][2];
  }
  if (b == 0.0) return;                        // an empty batch: the statistics stay what they are, bit for bit
  norm_update_column(b, s1, s2, stats + c);
}

__global__ __launch_bounds__(kNormThreads) void so100_norm_apply_kernel(NormArgs a, const double* __restrict__ stats) {
  const long long idx = (long long)blockIdx.x * kNormThreads + (int)threadIdx.x;
  if (idx >= (long long)a.n * a.D) return;
  const long long r = idx / a.D;
  const int c = (int)(idx - r * a.D);
  if (a.mask != nullptr && a.mask[r] == 0) return;
  const float* x = c < a.end0 ? a.x0 : (c < a.end1 ? a.x1 : a.x2);
  float* y = c < a.end0 ? a.y0 : (c < a.end1 ? a.y1 : a.y2);
  const int stride = c < a.end0 ? a.stride0 : (c < a.end1 ? a.stride1 : a.stride2);
  const int ystride = c < a.end0 ? a.ystride0 : (c < a.end1 ? a.ystride1 : a.ystride2);
  const int off = c < a.end0 ? a.off0 : (c < a.end1 ? a.off1 : a.off2);
  const int first = c < a.end0 ? 0 : (c < a.end1 ? a.end0 : a.end1);
  const double mean = stats[c], sd = sqrt(stats[kNormCols + c] + a.epsilon);
  const double v = (double)x[(size_t)r * stride + c + off];
  float out;
  if (a.inverse) {
    out = (float)(v * sd + mean);
  } else {
    out = (float)((v - mean) / sd);
    out = fminf(fmaxf(out, -a.clip), a.clip);
  }
  y[(size_t)r * ystride + (c - first)] = out;
}

// reward_norm = clip(reward / sqrt(var + eps)) where asked for, and ret <- 0 for the envs that finished
__global__ __launch_bounds__(kNormThreads) void so100_norm_ret_finish_kernel(int n, double epsilon, float clip,
                                                                             const float* __restrict__ reward,
                                                                             const uint8_t* __restrict__ terminated,
                                                                             const uint8_t* __restrict__ truncated,
                                                                             const double* __restrict__ stats,
                                                                             double* __restrict__ ret,
                                                                             float* __restrict__ reward_norm) {
  const long long i = (long long)blockIdx.x * kNormThreads + (int)threadIdx.x;
  if (i >= n) return;
  if (reward_norm != nullptr) {
    const float y = (float)((double)reward[i] / sqrt(stats[kNormCols] + epsilon));
    reward_norm[i] = fminf(fmaxf(y, -clip), clip);
  }
  const bool done = (terminated != nullptr && terminated[i] != 0) || (truncated != nullptr && truncated[i] != 0);
  if (done) ret[i] = 0.0;
}

static NormArgs norm_args(const so100_norm& nm, int n, const uint8_t* mask) {
  NormArgs a{};
  const so100_norm_src* s = nm.src;
  const int d0 = s[0].dim, d1 = nm.nsrc > 1 ? s[1].dim : 0, d2 = nm.nsrc > 2 ? s[2].dim : 0;
  a.x0 = s[0].x; a.y0 = s[0].y; a.stride0 = s[0].stride; a.ystride0 = s[0].y_stride; a.off0 = s[0].offset;
  a.end0 = d0;
  a.end1 = d0 + d1;
  a.D = d0 + d1 + d2;
  if (nm.nsrc > 1) { a.x1 = s[1].x; a.y1 = s[1].y; a.stride1 = s[1].stride; a.ystride1 = s[1].y_stride; a.off1 = s[1].offset - a.end0; }
  if (nm.nsrc > 2) { a.x2 = s[2].x; a.y2 = s[2].y; a.stride2 = s[2].stride; a.ystride2 = s[2].y_stride; a.off2 = s[2].offset - a.end1; }
  a.n = n;
  const int g = norm_groups(n);
  a.rows = (n + g - 1) / g < kNormRows ? kNormRows : (n + g - 1) / g;
  a.mask = mask;
  a.epsilon = nm.epsilon;
  a.clip = (float)nm.clip;
  a.inverse = (nm.flags & SO100_NORM_INVERSE) != 0;
  return a;
}

hipError_t launch_norm_update(const so100_norm& nm, int n, const uint8_t* mask, double* stats, double* work, hipStream_t s) {
  const NormArgs a = norm_args(nm, n, mask);
  const int g = norm_groups(n);
  hipLaunchKernelGGL(so100_norm_moments_kernel, dim3(g), dim3(kNormThreads), 0, s, a, stats, work);
  hipLaunchKernelGGL(so100_norm_merge_kernel, dim3(1), dim3(kNormThreads), 0, s, a.D, g, work, stats);
  return hipGetLastError();
}

hipError_t launch_norm_apply(const so100_norm& nm, int n, const uint8_t* mask, const double* stats, hipStream_t s) {
  const NormArgs a = norm_args(nm, n, mask);
  const long long total = (long long)n * a.D;
  hipLaunchKernelGGL(so100_norm_apply_kernel, dim3((unsigned)((total + kNormThreads - 1) / kNormThreads)),
                     dim3(kNormThreads), 0, s, a, stats);
  return hipGetLastError();
}

hipError_t launch_norm_return(const so100_norm_ret& r, int n, const float* reward, const uint8_t* terminated,
                              const uint8_t* truncated, double* ret, double* stats, double* work, float* reward_norm,
                              hipStream_t s) {
  if (r.flags & SO100_NORM_RET_UPDATE) {
    const int g = norm_groups(n);
    const int rows = (n + g - 1) / g < kNormRows ? kNormRows : (n + g - 1) / g;
    hipLaunchKernelGGL(so100_norm_ret_moments_kernel, dim3(g), dim3(kNormThreads), 0, s, n, rows, r.gamma, reward, ret,
                       stats, work);
    hipLaunchKernelGGL(so100_norm_merge_kernel, dim3(1), dim3(kNormThreads), 0, s, 1, g, work, stats);
  }
  hipLaunchKernelGGL(so100_norm_ret_finish_kernel, dim3((n + kNormThreads - 1) / kNormThreads), dim3(kNormThreads), 0, s,
                     n, r.epsilon, (float)r.clip, reward, terminated, truncated, stats,
                     ret, (r.flags & SO100_NORM_RET_NORMALIZE) ? reward_norm : nullptr);
  return hipGetLastError();
}

}  // namespace so100
