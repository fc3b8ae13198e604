// so100_replay.hip - a uniform replay buffer for the arm tasks on the device, for state and pixel observations (C-ABI
// so100_replay_push, so100_replay_stage, so100_replay_scan, so100_replay_sample; include/so100.h states the rules,
// DESIGN.md §3.12 the reasons).  New launches beside the untouched step kernel: a push copies what the step and the
// rasteriser left (15 floats, the command, the scalars and, with P > 0, the P bytes of the env's images) into the env's
// ring, a sample draws uniformly among the valid transitions and, with pad > 0, shifts the two images of each row by
// independent random offsets (DrQ's replicate-pad and crop) while it gathers them.  No atomics, no wait for another
// workgroup, plain vector stores; every result is a function of the inputs alone.  No LDS.
//
// Addressing.  Rows of P bytes start at (slot n + e) P and i P: byte offsets are 64-bit, and neither P nor a row start is
// a multiple of 4 in general.  Every access wider than a byte is naturally aligned: stores go to the 4-aligned words of
// the destination row (its 0..3 head bytes and 0..3 tail bytes singly), and the 4 source bytes of such a word come from
// the one or two aligned words that hold them, joined by v_alignbyte_b32.  An aligned word that holds one byte of an
// array lies in that byte's page, so the join never touches an unmapped page.  Where the rows and P are all multiples of
// 16 (every real image size) the copy moves 16 bytes per lane instead.
//
// Push and stage.  One workgroup per env (256 threads with images, 64 without): thread c < 15 copies column c of the
// observation, threads 16.. the command, thread 32 the scalars, and all of them the image rows.  An env that did not
// finish reads its `pixels` row once and stores it twice (next_img at the cursor, obs_img at the new cursor) when the two
// destinations agree mod 4 (always when P is a multiple of 4); a finished env copies final_pixels and pixels once each.
// The metadata: every thread reads cursor and count first, a workgroup barrier follows the copies, thread 0 then writes
// them; no other workgroup of the launch touches this env.
//
// Sample.  One launch of two kinds of workgroups.  The first ceil(B / 16) take the float rows, 16 lanes per batch element
// as in so100_her.hip.  The others take the images in pieces of one output image, `span` chunks of kChunk bytes each,
// spread over a grid of at most kMaxPieceGroups workgroups.  Every workgroup repeats the draw and the search of its row:
// a chain of dependent loads that hit L2, which is what a piece costs before its first byte moves.  So each wave searches
// the prefix sums 64 ways at a time (3 rounds for 8,192 envs, not 13), and the launcher grows `span` with the batch (one
// chunk per piece up to kSpanPieces pieces, then more).  A thread builds 4-aligned output words, 4 per chunk: with
// pad == 0 by the aligned join above, with pad > 0 from 4 byte loads at the clamped source coordinates, found by two
// divisions per word and increments between its bytes.  The stores are contiguous 256-byte runs per wave; the loads are
// rows of the ring, each source byte fetched from HBM once and again only from L1 / L2.
//
// N-step returns (so100_replay_push_nstep, so100_replay_stage_nstep, so100_replay_sample_nstep).  The
// same three kernel bodies, instantiated a second time with the `ends` bytes: push and stage mark where an episode ends,
// the sample reads the window's n_step `ends` bytes and rewards in one round (one slot per lane), finds its length by a
// ballot and sums the rewards in a fixed order by shuffles.  The plain entry points launch the instantiations without.
//
// Prioritised replay (so100_replay_push_per, so100_replay_per_scan, so100_replay_sample_per, so100_replay_per_update;
// DESIGN.md §3.14).  The push and sample bodies instantiated once more per combination with the uint32 fixed-point
// priorities; the plain and n-step entry points launch the instantiations without, as before.  The sums are uint64, so a
// scan in any order gives the same bits: per-env sums by the whole device, then one workgroup's scan over the envs (the
// only LDS of this file, and still no wait for another workgroup).  The update holds the library's only atomics, an
// integer maximum per applied row and one per wave: commutative, so the result is still a function of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "so100.h"
#include "so100_ring.h"

namespace so100 {

constexpr int kRepThreads = 256;
constexpr int kRepStateThreads = 64;                     // push / stage without images
constexpr int kRepLanes = 16;                            // lanes per batch element (the sample's float rows)
constexpr int kRepRows = kRepThreads / kRepLanes;
constexpr int kRepObs = SO100_NOBS;
constexpr int kChunk = 4096;                             // output bytes of one image piece
constexpr int kChunkWords = kChunk / 4;
constexpr unsigned kMaxPieceGroups = 1u << 20;
constexpr long long kSpanPieces = 8192;                  // pieces of one chunk beyond which a piece takes more chunks
static_assert(kRepObs < kRepLanes, "a row's columns and one scalar lane fit the lanes of a batch element");
static_assert(SO100_REPLAY_MAX_ACTION <= kRepLanes, "one lane per command component");
static_assert(16 + SO100_REPLAY_MAX_ACTION <= 32 && 32 < kRepStateThreads, "the push's thread roles fit one wave");
static_assert(kChunkWords % kRepThreads == 0, "a piece is a whole number of words per thread");

namespace {

// the 4 bytes at s (any alignment) from the aligned words that hold them
__device__ __forceinline__ uint32_t load4(const uint8_t* s) {
  const uintptr_t a = (uintptr_t)s;
  const uint32_t* w = (const uint32_t*)(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t w0 = w[0];
  const uint32_t w1 = sh != 0 ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(w1, w0, sh);
}

// dst[0..P) (and dst2[0..P) where TWO; dst2 = dst mod 4) <- src[0..P), by the nt threads of a workgroup
template <bool TWO>
__device__ __forceinline__ void copy_row(uint8_t* dst, uint8_t* dst2, const uint8_t* src, int P, int tid, int nt) {
  const uintptr_t all = (uintptr_t)dst | (uintptr_t)src | (TWO ? (uintptr_t)dst2 : 0) | (uintptr_t)(uint32_t)P;
  if ((all & 15) == 0) {
    const uint4* s16 = (const uint4*)src;
    uint4* d16 = (uint4*)dst;
    uint4* e16 = (uint4*)dst2;
    const int nq = P >> 4;
    for (int q = tid; q < nq; q += nt) {
      const uint4 v = s16[q];
      d16[q] = v;
      if (TWO) e16[q] = v;
    }
    return;
  }
  const int align = (int)((0 - (uintptr_t)dst) & 3);
  const int head = align < P ? align : P;
  const int nw = (P - head) >> 2;
  const int tail0 = head + 4 * nw;
  if (tid < head) {
    const uint8_t v = src[tid];
    dst[tid] = v;
    if (TWO) dst2[tid] = v;
  }
  if (tail0 + tid < P) {                                 // (at most 3 bytes)
    const uint8_t v = src[tail0 + tid];
    dst[tail0 + tid] = v;
    if (TWO) dst2[tail0 + tid] = v;
  }
  uint32_t* dw = (uint32_t*)(dst + head);
  uint32_t* ew = (uint32_t*)(dst2 + head);
  for (int w = tid; w < nw; w += nt) {
    const uint32_t v = load4(src + head + 4 * (size_t)w);
    dw[w] = v;
    if (TWO) ew[w] = v;
  }
}

struct RepPick {
  int e, slot;
  int k, cnt;                                            // the slot's index among the env's valid transitions, their count
  bool any;
};

// the first env e of [0, n) with prefix[e] > r (n - 1 when there is none), by bisection: any set of lanes.  (V, R): the
// counts' (int32_t, long long) or the priority sums' (uint64_t, uint64_t)
template <class V, class R>
__device__ __forceinline__ int find_env_bisect(const V* prefix, int n, R r) {
  int lo = 0, hi = n - 1;
  for (int it = 0; it < 32 && lo < hi; it++) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if ((R)prefix[mid] > r) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the same env found by a whole wave (all 64 lanes active, r equal in all): each round the lanes probe 64 evenly spaced
// candidates and a ballot narrows the range 64-fold, so 8,192 envs take 3 dependent loads where bisection takes 13
template <class V, class R>
__device__ __forceinline__ int find_env_wave(const V* prefix, int n, R r) {
  const int lane = (int)threadIdx.x & 63;
  int lo = 0, cnt = n;                                   // the candidates are [lo, lo + cnt)
  for (int it = 0; it < 6 && cnt > 1; it++) {
    const int step = (cnt + 63) >> 6;
    const int last = lo + cnt - 1;
    const long long want = (long long)lo + (long long)(lane + 1) * step - 1;
    const int probe = want < last ? (int)want : last;    // nondecreasing in the lane, within [lo, last]
    const bool below = (R)prefix[probe] <= r;
    const int f = __popcll(__ballot(below));             // the lanes whose probe is still <= r: the first f
    if (f == 64) return last;                            // (no env of the range exceeds r)
    const long long nlo = (long long)lo + (long long)f * step;       // one past lane f - 1's probe
    if (nlo > last) return last;                         // (only a prefix array that does not ascend gets here)
    const long long nhi = (long long)lo + (long long)(f + 1) * step - 1;
    const int hi = nhi < last ? (int)nhi : last;
    lo = f == 0 ? lo : (int)nlo;
    cnt = hi - lo + 1;
  }
  return lo;
}

// the transition of batch element i: r uniform in [0, total), its env the first e with prefix[e] > r.  WAVE: called by
// whole waves with one i per wave
template <bool WAVE>
__device__ __forceinline__ RepPick replay_pick(const so100_replay& h, uint64_t call, size_t i) {
  RepPick p = {0, -1, 0, 0, false};
  const int n = h.n, T = h.T;
  const long long cap = (long long)(T - 1) * n;
  long long total = h.prefix[n];
  total = total < 0 ? 0 : (total > cap ? cap : total);
  if (total == 0) return p;
  const long long r = (long long)__umul64hi(her_draw(h.seed, call, i, 0u), (uint64_t)total);
  const int e = WAVE ? find_env_wave(h.prefix, n, r) : find_env_bisect(h.prefix, n, r);
  const long long base = e > 0 ? (long long)h.prefix[e - 1] : 0;
  const long long kq = r - base;
  const int k = (int)(kq < 0 ? 0 : (kq > T - 2 ? T - 2 : kq));
  const int cur = clampi(h.meta[e], 0, T - 1);
  const int cnt = clampi(h.meta[(size_t)n + e], 0, T - 1);
  p.e = e;
  p.slot = add_mod(sub_mod(cur, cnt, T), k, T);
  p.k = k;
  p.cnt = cnt;
  p.any = true;
  return p;
}

// the prioritised pick of batch element i (so100_replay_sample_per, rules 1-4): r uniform in [0, total) of the priority
// sums, the env by the same searches on 64-bit values, then the first of the env's valid slots, oldest first, whose
// running sum exceeds rr.  The slots' addresses follow from the metadata alone, so the L lanes of the caller (WAVE: a
// whole wave, one i per wave; else the 16 lanes [base, base + 16) of a batch element, all active, same i) split the cnt
// slots into L runs of `per` consecutive ones and load them side by side, `per` independent loads per lane: one more
// round trip on the chain, not cnt.  A shuffle prefix over the runs' sums and a ballot find the run; with per > 1 every
// lane then walks that run again (the same addresses in all lanes, just loaded: L1 hits) without a branch on what it
// reads.  q: the pick's priority, total: the sum the draw was scaled by.
template <bool WAVE>
__device__ __forceinline__ RepPick replay_pick_per(const so100_replay& h, const so100_replay_per& pr, uint64_t call,
                                                   size_t i, uint32_t& q, uint64_t& total) {
  constexpr int L = WAVE ? 64 : kRepLanes;
  RepPick p = {0, -1, 0, 0, false};
  q = 0u;
  const int n = h.n, T = h.T;
  total = pr.sum[n];
  if (total == 0) return p;
  const uint64_t r = __umul64hi(her_draw(h.seed, call, i, 0u), total);
  const int e = WAVE ? find_env_wave<uint64_t, uint64_t>(pr.sum, n, r) : find_env_bisect<uint64_t, uint64_t>(pr.sum, n, r);
  const uint64_t before_env = e > 0 ? pr.sum[e - 1] : 0ull;
  const uint64_t rr = r >= before_env ? r - before_env : 0ull;
  const int cur = clampi(h.meta[e], 0, T - 1);
  const int cnt = clampi(h.meta[(size_t)n + e], 0, T - 1);
  const int start = sub_mod(cur, cnt, T);
  const int lane = (int)threadIdx.x & (L - 1), base = WAVE ? 0 : ((int)threadIdx.x & 48);
  const int per = (cnt + L - 1) / L;                     // slots per lane: 1 up to L valid slots
  uint64_t mine = 0;
  for (int t = 0; t < per; t++) {
    const int k = lane * per + t;                        // < L per < cnt + L <= T + 63
    if (k < cnt) mine += pr.prio[(size_t)add_mod(start, k, T) * n + e];
  }
  uint64_t incl = mine;                                  // inclusive scan of the L runs' sums
#pragma unroll
  for (int off = 1; off < L; off <<= 1) {
    const uint64_t up = __shfl_up(incl, off, L);
    if (lane >= off) incl += up;
  }
  const unsigned long long hit = (__ballot(incl > rr) >> base) & (WAVE ? ~0ull : 0xFFFFull);
  int k = cnt > 0 ? cnt - 1 : 0;                         // corrupted sums leave no run: the last valid slot
  bool found = false;
  if (hit != 0) {
    const int f = __ffsll(hit) - 1;                      // the first run whose inclusive sum exceeds rr
    uint64_t run = __shfl(incl, f, L) - __shfl(mine, f, L);
    for (int t = 0; t < per; t++) {
      const int kk = f * per + t;
      const uint32_t v = kk < cnt ? pr.prio[(size_t)add_mod(start, kk, T) * n + e] : 0u;
      run += v;
      if (!found && run > rr && kk < cnt) {
        found = true;
        k = kk;
        q = v;
      }
    }
  }
  p.e = e;
  p.slot = add_mod(start, k, T);
  p.k = k;
  p.cnt = cnt;
  p.any = true;
  if (!found && cnt > 0) q = pr.prio[(size_t)p.slot * n + e];
  return p;
}

// (dx, dy) of the 64-bit draw h for S = 2 pad + 1 offsets
__device__ __forceinline__ void replay_shift(uint64_t h, int S, int& dx, int& dy) {
  dx = (int)(((h & 0xFFFFFFFFull) * (uint64_t)S) >> 32);
  dy = (int)(((h >> 32) * (uint64_t)S) >> 32);
}

// the coordinates of one output byte, stepped through the image in memory order
struct RepCoord {
  int q, y, x, c;                                        // q = p H: the first row of the byte's plane
  __device__ __forceinline__ void set(int k, int H, int W, int chan) {
    const int rowbytes = W * chan;
    const int row = k / rowbytes, cb = k - row * rowbytes;
    const int p = row / H;
    q = p * H;
    y = row - q;
    x = cb / chan;
    c = cb - x * chan;
  }
  __device__ __forceinline__ void next(int H, int W, int chan) {
    if (++c == chan) {
      c = 0;
      if (++x == W) {
        x = 0;
        if (++y == H) {
          y = 0;
          q += H;
        }
      }
    }
  }
  // the source byte's offset under the shift (ox, oy) = (dx - pad, dy - pad)
  __device__ __forceinline__ int source(int ox, int oy, int H, int W, int chan) const {
    const int sy = clampi(y + oy, 0, H - 1), sx = clampi(x + ox, 0, W - 1);
    return ((q + sy) * W + sx) * chan + c;               // < P < 2^31
  }
};

// the length m of the n-step window that starts at the pick p (so100_replay_sample_nstep, rule 2), by the lanes
// [base, base + 16) of a wave, all of them active and with the same p: lane base + j looks at the window's slot j (its
// `ends` byte, `closes`, and whether it is the env's newest transition), a ballot finds the first that stops the window.
// n_step <= 16, and lane base + n_step - 1 always stops it, so 1 <= m <= n_step
__device__ __forceinline__ int window_length(bool closes, int j, const RepPick& p, int n_step, int base) {
  const bool stop = j < n_step && (j + 1 == n_step || closes || p.k + j + 1 >= p.cnt);
  const unsigned long long b = __ballot(stop) >> base;
  return __ffs((unsigned)(b & 0xFFFFull));               // (0 only if n_step < 1, which the launcher refuses)
}

// acc + g r in float32 with the product rounded before the sum (so100_replay_sample_nstep, rule 3).  Written out under
// the pragma: to the compiler __fmul_rn and __fadd_rn are a plain * and +, which it contracts into one fused multiply-add
__device__ __forceinline__ float mul_then_add(float acc, float g, float r) {
#pragma clang fp contract(off)
  const float p = g * r;
  return acc + p;
}

// NSTEP: with the `ends` bytes (rules 6 and 7 of so100_replay_push_nstep); ends is NULL otherwise.  PER: with the
// priorities (rules 8 and 9 of so100_replay_push_per); prio and max_prio are not read otherwise
template <bool NSTEP, bool PER>
__device__ __forceinline__ void replay_push_body(const so100_replay& h, const so100_replay_step& s, uint8_t* ends,
                                                 uint32_t* prio, const uint32_t* max_prio) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int e = (int)blockIdx.x, n = h.n, T = h.T, A = h.action_dim, P = h.P;
  const int c = clampi(h.meta[e], 0, T - 1);
  const int k = clampi(h.meta[(size_t)n + e], 0, T - 1);
  const bool done = s.terminated[e] != 0 || s.truncated[e] != 0;
  const bool drop = s.diverged != nullptr && s.diverged[e] != 0;
  const int c2 = drop ? c : (c + 1 == T ? 0 : c + 1);
  const int k2 = drop ? k : (k + 1 < T - 1 ? k + 1 : T - 1);
  const size_t row = (size_t)c * n + e, row2 = (size_t)c2 * n + e;     // < T n < 2^31
  if (tid < kRepObs) {
    const float now = s.obs[(size_t)e * kRepObs + tid];
    const float next = done ? s.final_obs[(size_t)e * kRepObs + tid] : now;
    h.next_obs[row * kRepObs + tid] = next;              // 1.
    h.obs[row2 * kRepObs + tid] = now;                   // 4.
  }
  if (tid >= 16 && tid < 16 + A) h.action[row * A + (tid - 16)] = s.action[(size_t)e * A + (tid - 16)];
  if (tid == 32) {
    h.reward[row] = s.reward[e];
    h.terminated[row] = s.terminated[e] != 0 ? 1 : 0;
    if (NSTEP) {
      ends[row] = done ? 1 : 0;                          // 6.
      if (drop && k > 0) ends[(size_t)sub_mod(c, 1, T) * n + e] = 1;   // 7.
    }
    if (PER) {
      if (drop) {
        prio[row] = 0u;                                  // 9.
      } else {
        const uint32_t top = max_prio[0];
        prio[row] = top > 0u ? top : 1u;                 // 8.
        prio[row2] = 0u;                                 // (T >= 2: row2 != row)
      }
    }
  }
  if (P > 0) {
    const uint8_t* now = s.pixels + (size_t)e * P;
    uint8_t* nxt = h.next_img + row * P;
    uint8_t* stage = h.obs_img + row2 * P;
    if (!done && (((uintptr_t)nxt ^ (uintptr_t)stage) & 3) == 0) {
      copy_row<true>(nxt, stage, now, P, tid, nt);
    } else {
      copy_row<false>(nxt, nullptr, done ? s.final_pixels + (size_t)e * P : now, P, tid, nt);
      copy_row<false>(stage, nullptr, now, P, tid, nt);
    }
  }
  __syncthreads();                                       // every read of meta[e] is above, in every thread
  if (tid == 0) {
    h.meta[e] = c2;
    h.meta[(size_t)n + e] = k2;
  }
}

}  // namespace

__global__ __launch_bounds__(kRepThreads) void so100_replay_push_kernel(so100_replay h, so100_replay_step s) {
  replay_push_body<false, false>(h, s, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_push_nstep_kernel(so100_replay h, so100_replay_step s,
                                                                               uint8_t* ends) {
  replay_push_body<true, false>(h, s, ends, nullptr, nullptr);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_push_per_kernel(so100_replay h, so100_replay_step s,
                                                                             uint32_t* prio, const uint32_t* max_prio) {
  replay_push_body<false, true>(h, s, nullptr, prio, max_prio);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_push_nstep_per_kernel(so100_replay h, so100_replay_step s,
                                                                                   uint8_t* ends, uint32_t* prio,
                                                                                   const uint32_t* max_prio) {
  replay_push_body<true, true>(h, s, ends, prio, max_prio);
}

namespace {

template <bool NSTEP>
__device__ __forceinline__ void replay_stage_body(const so100_replay& h, const uint8_t* __restrict__ mask,
                                                  const float* __restrict__ obs, const uint8_t* __restrict__ pixels,
                                                  uint8_t* ends) {
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int e = (int)blockIdx.x, n = h.n, T = h.T, P = h.P;
  if (mask != nullptr && mask[e] == 0) return;
  const int c = clampi(h.meta[e], 0, T - 1);
  const size_t row = (size_t)c * n + e;
  if (tid < kRepObs) h.obs[row * kRepObs + tid] = obs[(size_t)e * kRepObs + tid];
  if (NSTEP && tid == 32 && clampi(h.meta[(size_t)n + e], 0, T - 1) > 0) ends[(size_t)sub_mod(c, 1, T) * n + e] = 1;
  if (P > 0) copy_row<false>(h.obs_img + row * P, nullptr, pixels + (size_t)e * P, P, tid, nt);
}

}  // namespace

__global__ __launch_bounds__(kRepThreads) void so100_replay_stage_kernel(so100_replay h, const uint8_t* __restrict__ mask,
                                                                         const float* __restrict__ obs,
                                                                         const uint8_t* __restrict__ pixels) {
  replay_stage_body<false>(h, mask, obs, pixels, nullptr);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_stage_nstep_kernel(so100_replay h,
                                                                                const uint8_t* __restrict__ mask,
                                                                                const float* __restrict__ obs,
                                                                                const uint8_t* __restrict__ pixels,
                                                                                uint8_t* ends) {
  replay_stage_body<true>(h, mask, obs, pixels, ends);
}

namespace {

// NSTEP: with the n-step window (so100_replay_sample_nstep); ns and no are not read otherwise.  The window adds one round
// of loads to the chain that a workgroup pays before its first byte moves, whatever n_step is: the addresses of the
// window's `ends` and reward entries follow from the pick, so the lanes read them side by side.
// PER: with the prioritised pick (so100_replay_sample_per); pr and po are not read otherwise.  Every workgroup, the
// image pieces' included, repeats the pick as it repeats the plain one: the float and the image workgroups of a row find
// the same slot because they run the same function on the same arrays.
template <bool NSTEP, bool PER>
__device__ __forceinline__ void replay_sample_body(const so100_replay& h, const so100_replay_out& o,
                                                   const so100_replay_nstep& ns, const so100_replay_nstep_out& no,
                                                   const so100_replay_per& pr, const so100_replay_per_out& po,
                                                   int batch, uint64_t call, unsigned row_groups, int chunks, int span) {
  const int n = h.n, A = h.action_dim, P = h.P, pad = h.pad;
  if (blockIdx.x < row_groups) {
    // ---- the float rows, 16 lanes per batch element
    const int c = (int)threadIdx.x & (kRepLanes - 1);
    const long long il = (long long)blockIdx.x * kRepRows + ((int)threadIdx.x >> 4);
    if (il >= batch) return;
    const size_t i = (size_t)il;
    const bool scalar = c == kRepLanes - 1;
    uint32_t q = 0u;
    uint64_t mass = 0ull;
    const RepPick p = PER ? replay_pick_per<false>(h, pr, call, i, q, mass) : replay_pick<false>(h, call, i);
    if (!p.any) {                                        // an empty buffer: zeros, nothing of the ring is read
      if (c < kRepObs) {
        o.obs[i * kRepObs + c] = 0.f;
        o.next_obs[i * kRepObs + c] = 0.f;
      }
      if (c < A) o.actions[i * A + c] = 0.f;
      if (c < 4) o.shift[i * 4 + c] = 0;
      if (scalar) {
        o.rewards[i] = 0.f;
        o.dones[i] = 0.f;
        o.env[i] = 0;
        o.slot[i] = -1;
        if (NSTEP) {
          no.discounts[i] = 0.f;
          no.nsteps[i] = 0;
          no.last_slot[i] = -1;
        }
        if (PER) {
          po.probs[i] = 0.f;
          po.weights[i] = 0.f;
        }
      }
      return;
    }
    const size_t row = (size_t)p.slot * n + p.e;
    size_t last = row;                                   // the row of the window's last transition
    float ret = 0.f, disc = 0.f;
    int m = 1, last_slot = p.slot;
    if (NSTEP) {
      // lane j of the element's 16: ends and reward of the window's slot j, in one round
      const int T = h.T;
      const bool mine = c < ns.n_step;
      const size_t wrow = (size_t)add_mod(p.slot, mine ? c : 0, T) * n + p.e;
      const bool closes = mine && ns.ends[wrow] != 0;
      const float rw = mine ? h.reward[wrow] : 0.f;
      m = clampi(window_length(closes, c, p, ns.n_step, (int)threadIdx.x & 48), 1, ns.n_step);
      // every lane sums in the header's order: each product rounded, then each sum
      ret = __shfl(rw, 0, kRepLanes);
      disc = ns.gamma;
      for (int j = 1; j < ns.n_step; j++) {
        const float rj = __shfl(rw, j, kRepLanes);
        if (j < m) {
          ret = mul_then_add(ret, disc, rj);
          disc = disc * ns.gamma;
        }
      }
      last_slot = add_mod(p.slot, m - 1, T);
      last = (size_t)last_slot * n + p.e;
    }
    if (c < kRepObs) {
      o.obs[i * kRepObs + c] = h.obs[row * kRepObs + c];
      o.next_obs[i * kRepObs + c] = h.next_obs[last * kRepObs + c];
    }
    if (c < A) o.actions[i * A + c] = h.action[row * A + c];
    if (c < 4) {
      int d[4] = {pad, pad, pad, pad};
      if (pad > 0) {
        replay_shift(her_draw(h.seed, call, i, 2u), 2 * pad + 1, d[0], d[1]);
        replay_shift(her_draw(h.seed, call, i, 3u), 2 * pad + 1, d[2], d[3]);
      }
      o.shift[i * 4 + c] = c == 0 ? d[0] : (c == 1 ? d[1] : (c == 2 ? d[2] : d[3]));
    }
    if (!scalar) return;
    o.rewards[i] = NSTEP ? ret : h.reward[row];
    o.dones[i] = h.terminated[last] != 0 ? 1.f : 0.f;
    o.env[i] = p.e;
    o.slot[i] = p.slot;
    if (NSTEP) {
      no.discounts[i] = disc;
      no.nsteps[i] = m;
      no.last_slot[i] = last_slot;
    }
    if (PER) {
      // rule 6: the division in float64, one rounding to float32; the weight from the count of valid transitions
      const float prob = (float)((double)q / (double)mass);
      const int valid = h.prefix[n];
      po.probs[i] = prob;
      po.weights[i] = q != 0u ? powf((float)(valid < 0 ? 0 : valid) * prob, -pr.beta) : 0.f;
    }
    return;
  }
  // ---- the images: a piece is `span` chunks of kChunk bytes of one output image
  const int tid = (int)threadIdx.x;
  const int H = h.H, W = h.W, chan = h.chan;
  const int groups = (chunks + span - 1) / span;
  const long long per_row = 2ll * groups, pieces = (long long)batch * per_row;
  const long long stride = (long long)gridDim.x - row_groups;
  for (long long piece = (long long)blockIdx.x - row_groups; piece < pieces; piece += stride) {
    const size_t i = (size_t)(piece / per_row);
    const int rem = (int)(piece - (long long)i * per_row);
    const int which = rem >= groups ? 1 : 0, grp = rem - which * groups;
    const int ch0 = grp * span, ch1 = ch0 + span < chunks ? ch0 + span : chunks;
    uint8_t* dst = (which ? o.next_pixels : o.pixels) + i * (size_t)P;
    const int align = (int)((0 - (uintptr_t)dst) & 3);
    const int head = align < P ? align : P;
    const int nw = (P - head) >> 2;
    const int tail0 = head + 4 * nw;
    const bool ends = grp == 0;                          // this piece also takes the row's head and tail bytes
    uint32_t* dw = (uint32_t*)(dst + head);
    uint32_t q = 0u;
    uint64_t mass = 0ull;
    const RepPick p = PER ? replay_pick_per<true>(h, pr, call, i, q, mass) : replay_pick<true>(h, call, i);
    if (!p.any) {
      if (ends && tid < head) dst[tid] = 0;
      if (ends && tail0 + tid < P) dst[tail0 + tid] = 0;
      for (int ch = ch0; ch < ch1; ch++) {
#pragma unroll
        for (int u = 0; u < kChunkWords / kRepThreads; u++) {
          const int w = ch * kChunkWords + u * kRepThreads + tid;
          if (w < nw) dw[w] = 0u;
        }
      }
      continue;
    }
    int slot = p.slot;
    if (NSTEP && which) {                                // the next image is the window's last: lane j of each wave
      const int lane = tid & 63, T = h.T;                // reads the `ends` byte of the window's slot j
      const bool mine = lane < ns.n_step;
      const bool closes = mine && ns.ends[(size_t)add_mod(p.slot, mine ? lane : 0, T) * n + p.e] != 0;
      const int m = clampi(window_length(closes, lane, p, ns.n_step, 0), 1, ns.n_step);
      slot = add_mod(p.slot, m - 1, T);
    }
    const uint8_t* src = (which ? h.next_img : h.obs_img) + ((size_t)slot * n + p.e) * (size_t)P;
    if (pad == 0) {
      if (ends && tid < head) dst[tid] = src[tid];
      if (ends && tail0 + tid < P) dst[tail0 + tid] = src[tail0 + tid];
      for (int ch = ch0; ch < ch1; ch++) {
#pragma unroll
        for (int u = 0; u < kChunkWords / kRepThreads; u++) {
          const int w = ch * kChunkWords + u * kRepThreads + tid;
          if (w < nw) dw[w] = load4(src + head + 4 * (size_t)w);
        }
      }
      continue;
    }
    int dx, dy;
    replay_shift(her_draw(h.seed, call, i, which ? 3u : 2u), 2 * pad + 1, dx, dy);
    const int ox = dx - pad, oy = dy - pad;
    RepCoord at;
    if (ends && tid < head) {
      at.set(tid, H, W, chan);
      dst[tid] = src[at.source(ox, oy, H, W, chan)];
    }
    if (ends && tail0 + tid < P) {
      at.set(tail0 + tid, H, W, chan);
      dst[tail0 + tid] = src[at.source(ox, oy, H, W, chan)];
    }
    for (int ch = ch0; ch < ch1; ch++) {
#pragma unroll
      for (int u = 0; u < kChunkWords / kRepThreads; u++) {
        const int w = ch * kChunkWords + u * kRepThreads + tid;
        if (w < nw) {
          at.set(head + 4 * w, H, W, chan);
          uint32_t v = 0;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            v |= (uint32_t)src[at.source(ox, oy, H, W, chan)] << (8 * j);
            at.next(H, W, chan);
          }
          dw[w] = v;
        }
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kRepThreads) void so100_replay_sample_kernel(so100_replay h, so100_replay_out o, int batch,
                                                                          uint64_t call, unsigned row_groups, int chunks,
                                                                          int span) {
  replay_sample_body<false, false>(h, o, so100_replay_nstep{}, so100_replay_nstep_out{}, so100_replay_per{},
                                   so100_replay_per_out{}, batch, call, row_groups, chunks, span);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_sample_nstep_kernel(so100_replay h, so100_replay_out o,
                                                                                so100_replay_nstep ns,
                                                                                so100_replay_nstep_out no, int batch,
                                                                                uint64_t call, unsigned row_groups,
                                                                                int chunks, int span) {
  replay_sample_body<true, false>(h, o, ns, no, so100_replay_per{}, so100_replay_per_out{}, batch, call, row_groups,
                                  chunks, span);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_sample_per_kernel(so100_replay h, so100_replay_out o,
                                                                              so100_replay_per pr, so100_replay_per_out po,
                                                                              int batch, uint64_t call,
                                                                              unsigned row_groups, int chunks, int span) {
  replay_sample_body<false, true>(h, o, so100_replay_nstep{}, so100_replay_nstep_out{}, pr, po, batch, call, row_groups,
                                  chunks, span);
}

__global__ __launch_bounds__(kRepThreads) void so100_replay_sample_nstep_per_kernel(
    so100_replay h, so100_replay_out o, so100_replay_nstep ns, so100_replay_nstep_out no, so100_replay_per pr,
    so100_replay_per_out po, int batch, uint64_t call, unsigned row_groups, int chunks, int span) {
  replay_sample_body<true, true>(h, o, ns, no, pr, po, batch, call, row_groups, chunks, span);
}

// the priorities of each env summed over its T slots (so100_replay_per_scan, first launch): 64 envs by kSumParts parts of
// the slots per workgroup, so that a wave's loads are 256 contiguous bytes of one slot's row; the parts meet in LDS
constexpr int kSumParts = kRepThreads / 64;
__global__ __launch_bounds__(kRepThreads) void so100_replay_per_sum_kernel(int n, int T, const uint32_t* __restrict__ prio,
                                                                           uint64_t* __restrict__ sum) {
  __shared__ uint64_t part_sum[kSumParts][64];
  const int lane = (int)threadIdx.x & 63, part = (int)threadIdx.x >> 6;
  const long long el = (long long)blockIdx.x * 64 + lane;
  uint64_t acc = 0;
  if (el < n) {
#pragma unroll 4
    for (int s = part; s < T; s += kSumParts) acc += prio[(size_t)s * n + (size_t)el];
  }
  part_sum[part][lane] = acc;
  __syncthreads();
  if (part == 0 && el < n) {
    uint64_t all = 0;
#pragma unroll
    for (int k = 0; k < kSumParts; k++) all += part_sum[k][lane];
    sum[el] = all;
  }
}

// sum[0..n) <- its inclusive scan, sum[n] <- the total (so100_replay_per_scan, second launch): so100_her.hip's
// one-workgroup scan on uint64 values, in place (a thread reads its items of a tile before any thread writes that tile's)
constexpr int kPerScanThreads = 1024;
constexpr int kPerScanItems = 4;
constexpr int kPerScanTile = kPerScanThreads * kPerScanItems;
__global__ __launch_bounds__(kPerScanThreads) void so100_replay_per_scan_kernel(int n, uint64_t* sum) {
  __shared__ uint64_t wave_sum[2][kPerScanThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t carry = 0;                                    // the sum of every tile before this one: < 2^63
  int buf = 0;
  for (long long t0 = 0; t0 < n; t0 += kPerScanTile, buf ^= 1) {
    const long long i0 = t0 + (long long)tid * kPerScanItems;
    uint64_t v[kPerScanItems];
#pragma unroll
    for (int k = 0; k < kPerScanItems; k++) v[k] = i0 + k < n ? sum[i0 + k] : 0ull;
    uint64_t mine = 0;
#pragma unroll
    for (int k = 0; k < kPerScanItems; k++) mine += v[k];
    uint64_t incl = mine;                                // inclusive scan of the wave's 64 sums
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint64_t up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sum[buf][wave] = incl;
    __syncthreads();                                     // (the buffers alternate: one barrier per tile)
    uint64_t before = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < kPerScanThreads / 64; w++) {
      const uint64_t ws = wave_sum[buf][w];
      before += w < wave ? ws : 0ull;
      tile += ws;
    }
    uint64_t run = carry + before + incl - mine;
#pragma unroll
    for (int k = 0; k < kPerScanItems; k++) {
      run += v[k];
      if (i0 + k < n) sum[i0 + k] = run;
    }
    carry += tile;
  }
  if (tid == 0) sum[n] = carry;
}

// the fixed-point priority of |td| (so100_replay_per_update, rule 1)
__device__ __forceinline__ uint32_t per_priority(float td, float alpha, float eps) {
  const float x = fmaxf(fabsf(td), 0.f);                 // (fmaxf drops a NaN)
  const float v = rintf(powf(x + eps, alpha) * (float)SO100_REPLAY_PRIO_ONE);
  if (!(v >= 1.f)) return 1u;
  return v >= 4294967296.f ? 0xFFFFFFFFu : (uint32_t)v;
}

// so100_replay_per_update's two launches: phase 0 stores 0 from every applied row, phase 1 raises the slot to the row's
// q by an integer atomic maximum, so a slot named more than once ends at the greatest q whatever the order; the wave's
// greatest q goes to max_prio[0] by one more.  No thread leaves before the wave's shuffles
__global__ __launch_bounds__(kRepThreads) void so100_replay_per_update_kernel(so100_replay h, so100_replay_per pr,
                                                                              int batch,
                                                                              const int32_t* __restrict__ env_idx,
                                                                              const int32_t* __restrict__ slot_idx,
                                                                              const float* __restrict__ td_abs,
                                                                              int phase) {
  const long long j = (long long)blockIdx.x * kRepThreads + (int)threadIdx.x;
  const int n = h.n, T = h.T;
  bool applied = false;
  size_t row = 0;
  uint32_t q = 0u;
  if (j < batch) {
    const int e = env_idx[j], s = slot_idx[j];
    if (e >= 0 && e < n && s >= 0 && s < T) {
      const int cur = clampi(h.meta[e], 0, T - 1);
      const int cnt = clampi(h.meta[(size_t)n + e], 0, T - 1);
      applied = sub_mod(s, sub_mod(cur, cnt, T), T) < cnt;           // s is among the env's valid slots
      row = (size_t)s * n + e;
    }
  }
  if (phase == 0) {
    if (applied) pr.prio[row] = 0u;
    return;
  }
  if (applied) {
    q = per_priority(td_abs[j], pr.alpha, pr.eps);
    atomicMax(&pr.prio[row], q);
  }
  uint32_t top = q;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)top, off);
    top = other > top ? other : top;
  }
  if (((int)threadIdx.x & 63) == 0 && top > 0u) atomicMax(&pr.max_prio[0], top);
}

hipError_t launch_replay_push(const so100_replay& h, const so100_replay_step& st, hipStream_t s) {
  hipLaunchKernelGGL(so100_replay_push_kernel, dim3((unsigned)h.n), dim3(h.P > 0 ? kRepThreads : kRepStateThreads), 0, s,
                     h, st);
  return hipGetLastError();
}

hipError_t launch_replay_stage(const so100_replay& h, const uint8_t* mask, const float* obs, const uint8_t* pixels,
                               hipStream_t s) {
  hipLaunchKernelGGL(so100_replay_stage_kernel, dim3((unsigned)h.n), dim3(h.P > 0 ? kRepThreads : kRepStateThreads), 0,
                     s, h, mask, obs, pixels);
  return hipGetLastError();
}

hipError_t launch_replay_scan(const so100_replay& h, hipStream_t s) {
  return launch_count_scan(h.n, h.T - 1, h.meta + h.n, h.prefix, s);
}

// ns, no: NULL for the plain sample; pr, po: NULL for the uniform pick
static hipError_t launch_sample(const so100_replay& h, const so100_replay_out& o, const so100_replay_nstep* ns,
                                const so100_replay_nstep_out* no, const so100_replay_per* pr,
                                const so100_replay_per_out* po, int batch, uint64_t call, hipStream_t s) {
  const unsigned row_groups = (unsigned)(((long long)batch + kRepRows - 1) / kRepRows);
  const int chunks = (h.P + kChunk - 1) / kChunk;        // 0 without images
  // a workgroup finds its row's transition once (the draw, a search of the prefix sums, the metadata: dependent loads),
  // so a large batch gives it `span` chunks of the image for that price, a small one keeps the pieces small and many
  const long long small = 2ll * chunks * batch;
  long long span = (small + kSpanPieces - 1) / kSpanPieces;
  span = span < 1 ? 1 : (span > chunks ? chunks : span);
  const long long pieces = chunks > 0 ? 2ll * ((chunks + span - 1) / span) * batch : 0;
  const unsigned piece_groups = (unsigned)(pieces < (long long)kMaxPieceGroups ? pieces : (long long)kMaxPieceGroups);
  if (pr != nullptr && ns != nullptr)
    hipLaunchKernelGGL(so100_replay_sample_nstep_per_kernel, dim3(row_groups + piece_groups), dim3(kRepThreads), 0, s, h,
                       o, *ns, *no, *pr, *po, batch, call, row_groups, chunks, (int)span);
  else if (pr != nullptr)
    hipLaunchKernelGGL(so100_replay_sample_per_kernel, dim3(row_groups + piece_groups), dim3(kRepThreads), 0, s, h, o,
                       *pr, *po, batch, call, row_groups, chunks, (int)span);
  else if (ns != nullptr)
    hipLaunchKernelGGL(so100_replay_sample_nstep_kernel, dim3(row_groups + piece_groups), dim3(kRepThreads), 0, s, h, o,
                       *ns, *no, batch, call, row_groups, chunks, (int)span);
  else
    hipLaunchKernelGGL(so100_replay_sample_kernel, dim3(row_groups + piece_groups), dim3(kRepThreads), 0, s, h, o, batch,
                       call, row_groups, chunks, (int)span);
  return hipGetLastError();
}

hipError_t launch_replay_sample(const so100_replay& h, const so100_replay_out& o, int batch, uint64_t call,
                                hipStream_t s) {
  return launch_sample(h, o, nullptr, nullptr, nullptr, nullptr, batch, call, s);
}

hipError_t launch_replay_sample_nstep(const so100_replay& h, const so100_replay_out& o, const so100_replay_nstep& ns,
                                      const so100_replay_nstep_out& no, int batch, uint64_t call, hipStream_t s) {
  return launch_sample(h, o, &ns, &no, nullptr, nullptr, batch, call, s);
}

hipError_t launch_replay_push_nstep(const so100_replay& h, const so100_replay_nstep& ns, const so100_replay_step& st,
                                    hipStream_t s) {
  hipLaunchKernelGGL(so100_replay_push_nstep_kernel, dim3((unsigned)h.n), dim3(h.P > 0 ? kRepThreads : kRepStateThreads),
                     0, s, h, st, ns.ends);
  return hipGetLastError();
}

hipError_t launch_replay_stage_nstep(const so100_replay& h, const so100_replay_nstep& ns, const uint8_t* mask,
                                     const float* obs, const uint8_t* pixels, hipStream_t s) {
  hipLaunchKernelGGL(so100_replay_stage_nstep_kernel, dim3((unsigned)h.n),
                     dim3(h.P > 0 ? kRepThreads : kRepStateThreads), 0, s, h, mask, obs, pixels, ns.ends);
  return hipGetLastError();
}

// ns: NULL without the `ends` bytes
hipError_t launch_replay_push_per(const so100_replay& h, const so100_replay_per& pr, const so100_replay_nstep* ns,
                                  const so100_replay_step& st, hipStream_t s) {
  const dim3 block(h.P > 0 ? kRepThreads : kRepStateThreads);
  if (ns != nullptr)
    hipLaunchKernelGGL(so100_replay_push_nstep_per_kernel, dim3((unsigned)h.n), block, 0, s, h, st, ns->ends, pr.prio,
                       pr.max_prio);
  else
    hipLaunchKernelGGL(so100_replay_push_per_kernel, dim3((unsigned)h.n), block, 0, s, h, st, pr.prio, pr.max_prio);
  return hipGetLastError();
}

hipError_t launch_replay_per_scan(const so100_replay& h, const so100_replay_per& pr, hipStream_t s) {
  if (h.n > 0) {
    hipLaunchKernelGGL(so100_replay_per_sum_kernel, dim3((unsigned)((h.n + 63) / 64)), dim3(kRepThreads), 0, s, h.n, h.T,
                       pr.prio, pr.sum);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(so100_replay_per_scan_kernel, dim3(1), dim3(kPerScanThreads), 0, s, h.n, pr.sum);
  return hipGetLastError();
}

// ns, no: NULL without the n-step window
hipError_t launch_replay_sample_per(const so100_replay& h, const so100_replay_out& o, const so100_replay_per& pr,
                                    const so100_replay_per_out& po, const so100_replay_nstep* ns,
                                    const so100_replay_nstep_out* no, int batch, uint64_t call, hipStream_t s) {
  return launch_sample(h, o, ns, no, &pr, &po, batch, call, s);
}

hipError_t launch_replay_per_update(const so100_replay& h, const so100_replay_per& pr, int batch, const int32_t* env_idx,
                                    const int32_t* slot_idx, const float* td_abs, hipStream_t s) {
  const unsigned groups = (unsigned)(((long long)batch + kRepThreads - 1) / kRepThreads);
  for (int phase = 0; phase < 2; phase++) {
    hipLaunchKernelGGL(so100_replay_per_update_kernel, dim3(groups), dim3(kRepThreads), 0, s, h, pr, batch, env_idx,
                       slot_idx, td_abs, phase);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace so100
