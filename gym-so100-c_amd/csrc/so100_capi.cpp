// so100_capi.cpp — extern "C" boundary of libso100_hip.so (declared in include/so100.h).
//
// so100_create converts the double-precision host model (so100_model) into the fp32 device model
// (DevModel) with the model-constant parts of MuJoCo's constraint setup precomputed on the host
// (frictionloss R at pos 0, solref -> K/B, pair invweight sums), uploads it once, and returns an
// opaque handle.  Every other call only validates arguments and enqueues a kernel on the caller's
// stream: no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <exception>
#include <new>
#include <vector>
#include "so100.h"
#include "so100_device.h"

namespace so100 {
hipError_t launch_step(const DevModel*, int, int, int, int, int, Workspace&, const so100_buffers&, int, int, int, int,
                       uint64_t, int, hipStream_t, hipEvent_t*);
int fused_build(int n, int waves, bool debug);
bool fused_order_active(int n);
bool fused_pack_auto(int n);
hipError_t launch_contact_count(const Workspace&, int, uint64_t*, hipStream_t);
hipError_t launch_contact_counts(const Workspace&, int, int32_t*, hipStream_t);
hipError_t launch_render(const DevModel*, const float4*, const int*, const uint32_t*, int, const float*,
                         const uint8_t*, const so100_camera&, int, int, int, const so100_image_out&, hipStream_t);
hipError_t launch_render_views(const DevModel*, const float4*, const int*, const uint8_t*, int, const float*,
                               const uint8_t*, const so100_camera&, const so100_view*, int, int, int,
                               const so100_image_out&, hipStream_t);
hipError_t launch_render_aux(const DevModel*, const float4*, const int*, const uint32_t*, const uint8_t*, const uint8_t*,
                             int, const float*, const uint8_t*, const so100_camera&, const so100_view*, int, int, int,
                             const so100_image_out&, const so100_aux_out&, hipStream_t);
hipError_t launch_render_cams(const DevModel*, const float4*, const int*, const uint32_t*, const uint8_t*, const uint8_t*,
                              int, const float*, const uint8_t*, const so100_cams&, const so100_view*, int, int, int,
                              const so100_image_out&, const so100_aux_out&, hipStream_t);
hipError_t launch_render_shadow(const DevModel*, const float4*, const int*, const uint32_t*, const uint8_t*,
                                const uint8_t*, const uint8_t*, int, const float*, const uint8_t*, const so100_cams&,
                                const so100_view*, int, int, int, const so100_image_out&, const so100_aux_out&,
                                const so100_shadow&, hipStream_t);
hipError_t launch_render_msaa(const DevModel*, const float4*, const int*, const uint32_t*, const uint8_t*, int,
                              const float*, const uint8_t*, const so100_cams&, const so100_view*, int, int, int,
                              const so100_image_out&, const so100_msaa&, hipStream_t);
hipError_t launch_views_sample(const so100_view_dr&, const so100_camera&, const uint32_t*, const uint32_t*,
                               const uint8_t*, so100_view*, int, int, hipStream_t);
hipError_t alloc_workspace(int, Workspace*);
hipError_t alloc_fused_workspace(int, Workspace*);
hipError_t free_workspace(Workspace*);
hipError_t launch_reset(const DevModel*, const so100_buffers&, int, int, uint64_t, int, const uint8_t*, const uint32_t*,
                        hipStream_t);
hipError_t launch_reward(const DevModel*, int, int, const float*, const float*, const uint32_t*, float*, hipStream_t);
hipError_t launch_spawn(const DevModel*, int, const uint32_t*, double*, hipStream_t);
hipError_t launch_unnormalize(const DevModel*, int, const float*, float*, hipStream_t);
hipError_t launch_goal_reward(const DevModel*, int, const float*, const float*, float*, hipStream_t);
hipError_t launch_ee_action(const DevModel*, const so100_ee_ctrl&, int, const float*, const float*, const uint8_t*,
                            float*, float*, float*, hipStream_t);
hipError_t launch_ee_jacobian(const DevModel*, int, const float*, float*, float*, hipStream_t);
hipError_t launch_hull_support_probe(const DevModel*, int, const float*, int, int, float*, hipStream_t);
hipError_t launch_dr_sample(const so100_dr_ranges&, const uint32_t*, const uint8_t*, const uint8_t*, float*, float*, int,
                            int, hipStream_t);
hipError_t launch_actuate(const DevModel*, int, const float*, const float*, const uint8_t*, const float*, float*,
                          int32_t*, float*, hipStream_t);
int norm_groups(int n);
int norm_rows_per_group();
int norm_max_groups();
hipError_t launch_norm_update(const so100_norm&, int, const uint8_t*, double*, double*, hipStream_t);
hipError_t launch_norm_apply(const so100_norm&, int, const uint8_t*, const double*, hipStream_t);
hipError_t launch_norm_return(const so100_norm_ret&, int, const float*, const uint8_t*, const uint8_t*, double*, double*,
                              double*, float*, hipStream_t);
int her_scan_group();
int her_scan_tile();
hipError_t launch_her_push(const so100_her&, const so100_her_step&, hipStream_t);
hipError_t launch_her_discard(const so100_her&, const uint8_t*, const float*, const float*, hipStream_t);
hipError_t launch_her_scan(const so100_her&, hipStream_t);
hipError_t launch_her_sample(const DevModel*, const so100_her&, const so100_her_out&, int, int, uint64_t, hipStream_t);
hipError_t launch_replay_push(const so100_replay&, const so100_replay_step&, hipStream_t);
hipError_t launch_replay_stage(const so100_replay&, const uint8_t*, const float*, const uint8_t*, hipStream_t);
hipError_t launch_replay_scan(const so100_replay&, hipStream_t);
hipError_t launch_replay_sample(const so100_replay&, const so100_replay_out&, int, uint64_t, hipStream_t);
hipError_t launch_replay_push_nstep(const so100_replay&, const so100_replay_nstep&, const so100_replay_step&, hipStream_t);
hipError_t launch_replay_stage_nstep(const so100_replay&, const so100_replay_nstep&, const uint8_t*, const float*,
                                     const uint8_t*, hipStream_t);
hipError_t launch_replay_sample_nstep(const so100_replay&, const so100_replay_out&, const so100_replay_nstep&,
                                      const so100_replay_nstep_out&, int, uint64_t, hipStream_t);
hipError_t launch_replay_push_per(const so100_replay&, const so100_replay_per&, const so100_replay_nstep*,
                                  const so100_replay_step&, hipStream_t);
hipError_t launch_replay_per_scan(const so100_replay&, const so100_replay_per&, hipStream_t);
hipError_t launch_replay_sample_per(const so100_replay&, const so100_replay_out&, const so100_replay_per&,
                                    const so100_replay_per_out&, const so100_replay_nstep*,
                                    const so100_replay_nstep_out*, int, uint64_t, hipStream_t);
hipError_t launch_replay_per_update(const so100_replay&, const so100_replay_per&, int, const int32_t*, const int32_t*,
                                    const float*, hipStream_t);
}  // namespace so100

using so100::DevModel;
using so100::Workspace;

// A contiguous env range with its own substep workspace and stream.  With more than one chunk the
// chunks' launch sequences run concurrently (forked from / joined to the caller's stream), so one
// chunk's stage kernel fills the SIMD slots left idle by another chunk's solver tail.
struct Chunk {
  int start = 0, count = 0;
  Workspace ws{};               // substep hand-off record between the stage and solver kernels
  hipStream_t s = nullptr;      // nullptr: the caller's stream (single chunk)
  hipEvent_t done = nullptr;
};

struct StepGraph {
  hipGraphExec_t exec = nullptr;
  hipEvent_t done = nullptr;    // recorded after each replay (eviction waits for it)
  so100_buffers buf{};
  int flags = 0;
  uint32_t par = 0;             // substep-counter parity at the captured step's start
  uint64_t last_use = 0;
};
constexpr size_t kMaxStepGraphs = 32;

struct so100_env {
  int device;
  int n;
  DevModel* d_model;
  int nsubstep;
  int solver;                   // SO100_SOLVER_* of the model
  int fused;                    // step mode: 1 fused, 0 split, -1 auto (fused up to fused_max envs; Newton only)
  int fused_max;                // auto mode: the largest env count that runs fused
  Workspace fws{};              // fused launches: record header (contact counts) of all n envs, wave order
  bool last_fused = false;      // the mode of the last step (so100_contact_count reads its record)
  std::vector<Chunk> chunks;
  hipEvent_t fork = nullptr;
  int task;
  int max_steps;
  uint64_t base_seed;
  int env_offset;
  // camera render mesh (so100_render_mesh)
  float4* r_tri = nullptr;
  int* r_body = nullptr;
  uint32_t* r_rgb = nullptr;
  int r_ntri = 0;
  uint8_t* r_mat = nullptr;     // per-triangle material ids of that mesh (so100_render_materials), or none yet
  uint8_t* r_label = nullptr;   // per-triangle labels of that mesh (so100_render_labels), or none yet
  uint8_t* r_caster = nullptr;  // per-triangle shadow-caster bytes of that mesh (so100_render_casters), or none yet
  // profiling (so100_profile_enable): events[step][prof_per] (2 nsubstep + 2 split, 2 fused)
  std::vector<hipEvent_t> prof_ev;
  int prof_cap = 0, prof_used = 0, prof_per = 0;
  // step graphs: the 21 launches per chunk, the chunk fork and join, captured once per (buffers, flags,
  // substep parity) and replayed with one hipGraphLaunch when SO100_GRAPH=1.  A small LRU cache serves
  // callers that rotate a few action buffers (bench.py's pool of 16).  Off by default: the step is not
  // launch-bound (measured equal rates at 8,192 / 16,384 / 65,536 envs).
  bool use_graph = false;
  hipStream_t cap_s = nullptr;
  std::vector<StepGraph> graphs;
  uint64_t graph_clock = 0;
  float4* d_cand = nullptr;     // the hulls' support-cell candidates (DevModel::hull_cand)
  int fused_waves = 0;          // the fused product build: 2 | 3 waves per SIMD, 0 auto (so100_set_fused_build)
  int pack = -1;                // the fused step's env packing: -1 auto, 0 off, 1 on (so100_set_env_packing)
  int ee = 0;                   // the model's ee flag (the weld variant: so100_ee_action refuses it)
};

// An instantiated step graph can still be running when it is evicted: wait for its last replay first.
static void graph_destroy(StepGraph& g) {
  if (g.done) { (void)hipEventSynchronize(g.done); (void)hipEventDestroy(g.done); }
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  g.exec = nullptr;
  g.done = nullptr;
}

static void graph_free(so100_env* env) {
  for (StepGraph& g : env->graphs) graph_destroy(g);
  env->graphs.clear();
}

// The fused kernel implements the Newton solver only: PGS always takes the split launches.  Auto mode runs
// fused up to fused_max envs per GPU (SO100_FUSED_MAX; default: every size): round 3 measured the fused step
// faster at every shard size of the benchmark, 65,536 envs included (22.0 M vs 21.4 M env steps/s, +20 % at
// 32,768, +41 % at 16,384).
constexpr int kFusedAutoMax = 1 << 30;
static bool step_is_fused(const so100_env* env) {
  if (env->solver != SO100_SOLVER_NEWTON) return false;
  return env->fused < 0 ? env->n <= env->fused_max : env->fused != 0;
}

// Whether the fused step packs envs of like solver cost into the same wave (so100_order_kernel).  Auto: fused_pack_auto
// (off at every size: no measured gain).
static int env_packing(const so100_env* env) {
  if (env->pack >= 0) return env->pack;
  return so100::fused_pack_auto(env->n) ? 1 : 0;
}

static hipError_t free_chunks(so100_env* env) {
  hipError_t e = hipSuccess;
  for (Chunk& c : env->chunks) {
    hipError_t e2 = so100::free_workspace(&c.ws);
    if (e == hipSuccess) e = e2;
    if (c.done) (void)hipEventDestroy(c.done);
    if (c.s) (void)hipStreamDestroy(c.s);
  }
  env->chunks.clear();
  if (env->fork) (void)hipEventDestroy(env->fork);
  env->fork = nullptr;
  return e;
}

// Chunk count: SO100_CHUNKS overrides; otherwise as many chunks as the process has hardware queues
// (GPU_MAX_HW_QUEUES, HIP's default 4; chunk 0 shares the caller's), at least 1,024 envs each.  More
// streams than queues serialise on shared queues (measured: 5-8 chunks run 1.6x slower than 4).
static int default_chunks(int n) {
  if (const char* v = getenv("SO100_CHUNKS")) {
    const int k = atoi(v);
    if (k >= 1 && k <= 16) return k;
  }
  int q = 4;
  if (const char* v = getenv("GPU_MAX_HW_QUEUES")) {
    const int k = atoi(v);
    if (k >= 1) q = k;
  }
  if (q > 4) q = 4;
  const int k = n / 1024;
  return k < 1 ? 1 : (k > q ? q : k);
}

static hipError_t make_chunks(so100_env* env, int nchunk) {
  const int n = env->n;
  const int unit = 64;                                   // whole stage blocks and solver groups
  const int units = (n + unit - 1) / unit;
  if (nchunk > units) nchunk = units;
  hipError_t e = hipSuccess;
  if (nchunk > 1) e = hipEventCreateWithFlags(&env->fork, hipEventDisableTiming);
  int start = 0;
  for (int k = 0; k < nchunk && e == hipSuccess; k++) {
    Chunk c;
    c.start = start;
    const int end = k == nchunk - 1 ? n : (int)((long)units * (k + 1) / nchunk) * unit;
    c.count = end - start;
    start = end;
    e = so100::alloc_workspace(c.count, &c.ws);
    // chunk 0 runs on the caller's stream: K chunks take K - 1 extra hardware queues
    if (e == hipSuccess && k > 0) e = hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking);
    if (e == hipSuccess && k > 0) e = hipEventCreateWithFlags(&c.done, hipEventDisableTiming);
    env->chunks.push_back(c);
  }
  return e;
}

// per-env buffer pointers of the env range starting at `s`
static so100_buffers offset_buffers(const so100_buffers& b, int s) {
  so100_buffers o = b;
  const size_t k = (size_t)s;
  auto off = [k](auto* p, int dim) { return p ? p + k * dim : p; };
  o.qpos = off(b.qpos, SO100_NQ);
  o.qvel = off(b.qvel, SO100_NV);
  o.qacc_warmstart = off(b.qacc_warmstart, SO100_NV);
  o.elapsed = off(b.elapsed, 1);
  o.episode = off(b.episode, 1);
  o.action = off(b.action, SO100_NU);
  o.obs = off(b.obs, SO100_NOBS);
  o.reward = off(b.reward, 1);
  o.terminated = off(b.terminated, 1);
  o.truncated = off(b.truncated, 1);
  o.success = off(b.success, 1);
  o.final_obs = off(b.final_obs, SO100_NOBS);
  o.diverged = off(b.diverged, 1);
  o.contact_bits = off(b.contact_bits, 1);
  o.achieved_goal = off(b.achieved_goal, 3);
  o.desired_goal = off(b.desired_goal, 3);
  o.total_steps = off(b.total_steps, 1);
  o.dr_params = off(b.dr_params, 4);
  o.debug = off(b.debug, SO100_DBG_STRIDE);
  o.mocap = off(b.mocap, 7);
  o.reward64 = off(b.reward64, 1);
  o.ncon_dropped = off(b.ncon_dropped, 1);
  o.ep_return = off(b.ep_return, 1);
  o.ep_final = off(b.ep_final, 2);
  o.ep_accum = off(b.ep_accum, 4);
  return o;
}

static void profile_free(so100_env* env) {
  for (hipEvent_t e : env->prof_ev) (void)hipEventDestroy(e);
  env->prof_ev.clear();
  env->prof_cap = env->prof_used = 0;
}

// the last error of this thread: a fixed buffer, so reporting an error never allocates (or throws)
static thread_local char g_err[512];

static int fail(const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return -1;
}
static int fail_hip(const char* where, hipError_t e) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return -2;
}

namespace {
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

void quat2mat(const double* q, double* m) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = 1 - 2 * (y * y + z * z); m[1] = 2 * (x * y - w * z);     m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z);     m[4] = 1 - 2 * (x * x + z * z); m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y);     m[7] = 2 * (y * z + w * x);     m[8] = 1 - 2 * (x * x + y * y);
}
void normq(const double* q, double* o) {
  double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) o[k] = q[k] / n;
}
double clampimp(double v) { return v < 0.0001 ? 0.0001 : (v > 0.9999 ? 0.9999 : v); }
// MuJoCo getimpedance at pos == margin (x = 0) -> dmin (or the flat value)
double imp_at_zero(const double* solimp) {
  double dmin = clampimp(solimp[0]), dmax = clampimp(solimp[1]);
  if (dmin == dmax || solimp[2] <= 1e-15) return 0.5 * (dmin + dmax);
  return dmin;
}
void solref_kb(const double* solref, const double* solimp, double h, double* K, double* B) {
  double dmax = clampimp(solimp[1]);
  double tc = solref[0], dr = solref[1];
  if (tc > 0) {
    if (tc < 2 * h) tc = 2 * h;
    double den = dmax * dmax * tc * tc * dr * dr;
    *K = 1 / (den > 1e-15 ? den : 1e-15);
    double db = dmax * tc;
    *B = 2 / (db > 1e-15 ? db : 1e-15);
  } else {
    *K = -tc / (dmax * dmax);
    *B = -dr / dmax;
  }
}

int build_device_model(const so100_model* s, DevModel* d) {
  memset(d, 0, sizeof(*d));
  // structural assumptions of the specialised kernel
  for (int b = 2; b <= 7; b++)
    if (s->body_parent[b] != b - 1) return fail("model: arm bodies 2..7 must form a chain rooted at Base (1)");
  if (s->body_parent[1] != 0 || s->body_parent[SO100_CUBE_BODY] != 0) return fail("model: Base/cube must hang off world");
  for (int j = 0; j < SO100_NHINGE; j++)
    if (s->jnt_body[j] != j + 2) return fail("model: hinge j must sit on body j+2");
  for (int k = 0; k < 3; k++)
    if (fabs(s->body_ipos[SO100_CUBE_BODY][k]) > 1e-12) return fail("model: cube COM must be at the body origin");
  if (fabs(s->body_iquat[SO100_CUBE_BODY][0] - 1) > 1e-12) return fail("model: cube inertia must be body-aligned");
  if (s->site_ee_body != 6 || s->site_cube_body != SO100_CUBE_BODY) return fail("model: unexpected site bodies");
  for (int p = 0; p < SO100_NPAIR_BOX; p++)
    if (s->pair_condim[p] != 4) return fail("model: box-box pairs must have condim 4");
  if (s->geom_body[0] != 0 || fabs(s->geom_pos[0][2] + s->geom_size[0][2] - s->table_top) > 1e-9 ||
      fabs(s->geom_pos[0][0] - s->geom_size[0][0] - s->table_lo[0]) > 1e-6 ||
      fabs(s->geom_pos[0][0] + s->geom_size[0][0] - s->table_hi[0]) > 1e-6 ||
      fabs(s->geom_pos[0][1] - s->geom_size[0][1] - s->table_lo[1]) > 1e-6 ||
      fabs(s->geom_pos[0][1] + s->geom_size[0][1] - s->table_hi[1]) > 1e-6 || fabs(s->geom_quat[0][0] - 1) > 1e-12)
    return fail("model: geom 0 must be the table box, its top face table_top over table_lo..table_hi");
  for (int p = SO100_NPAIR_BOX; p < SO100_PAIR_MPR0; p++) {
    const int k = p - SO100_NPAIR_BOX;
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: hull pairs must have condim 3 or 4");
    if (s->pair_body1[p] != 0 || s->pair_body2[p] != s->hull_body[k]) return fail("model: hull pair k must be (table, hull k)");
    // the table is geom 0, a box (its mesh is an exact box) whose top face is table_top: the convex collider takes
    // it as obj1 (mpr_obj_setup's static box), the top-face rule as its top face and bottom
    if (s->pair_geom1[p] != 0 || s->pair_geom2[p] != -1 - k) return fail("model: hull pair k must be (geom 0 = the table, hull k)");
    if (s->pair_margin[p] != 0) return fail("model: table-hull pairs take no margin");
    if (s->hull_body[k] < 2 || s->hull_body[k] > 7) return fail("model: hulls must sit on arm bodies 2..7");
    if (s->hull_start[k] < 0 || s->hull_count[k] < 1 || s->hull_start[k] + s->hull_count[k] > SO100_HULL_NVERT)
      return fail("model: hull vertex range out of bounds");
  }
  // (box, hull) pairs of the MPR collider: box j = cube (geom 9) then the bin boxes (geoms 10..14), hull k
  for (int p = SO100_PAIR_MPR0; p < SO100_PAIR_SELF0; p++) {
    const int q = p - SO100_PAIR_MPR0, j = q / SO100_NHULL, k = q % SO100_NHULL;
    const int g = SO100_CUBE_GEOM + j;
    if (s->pair_geom1[p] != g || s->pair_geom2[p] != -1 - k) return fail("model: MPR pair p must be (box j, hull k)");
    if (s->pair_body1[p] != s->geom_body[g] || s->pair_body2[p] != s->hull_body[k]) return fail("model: MPR pair bodies");
    if (j > 0 && s->geom_body[g] != 0) return fail("model: bin boxes must be static");
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: MPR pairs must have condim 3 or 4");
    if (s->pair_margin[p] != 0) return fail("model: MPR pairs take no margin");
  }
  // the static Base hull: (cube, Base hull) then (Base hull, link hull k), all through MPR
  if (s->hull_body[SO100_HULL_BASE] != 1) return fail("model: hull 9 must be the Base's");
  if (s->hull_start[SO100_HULL_BASE] < 0 || s->hull_count[SO100_HULL_BASE] < 1 ||
      s->hull_start[SO100_HULL_BASE] + s->hull_count[SO100_HULL_BASE] > SO100_HULL_NVERT)
    return fail("model: Base hull vertex range out of bounds");
  if (s->body_parent[1] != 0) return fail("model: the Base must hang off the world");
  for (int p = SO100_PAIR_BASE0; p < SO100_PAIR_PADLINK0; p++) {
    const int g1 = s->pair_geom1[p], k2 = -1 - s->pair_geom2[p];
    if (p == SO100_PAIR_BASE0) {
      if (g1 != SO100_CUBE_GEOM || k2 != SO100_HULL_BASE) return fail("model: pair 98 must be (cube, Base hull)");
    } else if (g1 != -1 - SO100_HULL_BASE || k2 < 0 || k2 >= SO100_NHULL) {
      return fail("model: Base pairs must be (Base hull, link hull k)");
    }
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: Base pairs must have condim 3 or 4");
    if (s->pair_margin[p] != 0) return fail("model: MPR pairs take no margin");
  }
  // hull-hull self-collision pairs: two hulls on different arm links
  for (int p = SO100_PAIR_SELF0; p < SO100_PAIR_BASE0; p++) {
    const int k1 = -1 - s->pair_geom1[p], k2 = -1 - s->pair_geom2[p];
    if (k1 < 0 || k1 >= SO100_NHULL || k2 < 0 || k2 >= SO100_NHULL) return fail("model: self pair must be two hulls");
    if (s->pair_body1[p] != s->hull_body[k1] || s->pair_body2[p] != s->hull_body[k2] || k1 == k2)
      return fail("model: self pair bodies");
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: self pairs must have condim 3 or 4");
    if (s->pair_margin[p] != 0) return fail("model: MPR pairs take no margin");
  }
  // (finger pad, link hull) pairs through MPR: a pad box on a jaw against the Base or a link hull on bodies
  // 2..5 (the MPR kernel takes the pad's pose from its jaw's frame)
  for (int p = SO100_PAIR_PADLINK0; p < SO100_PAIR_MOCAPHULL0; p++) {
    const int g1 = s->pair_geom1[p], k2 = -1 - s->pair_geom2[p];
    if (g1 < 1 || g1 > SO100_NPAD || (s->geom_body[g1] != 6 && s->geom_body[g1] != 7))
      return fail("model: pad-link pair p must have a finger pad as geom1");
    if (k2 < 0 || k2 >= SO100_NHULL_ALL || s->hull_body[k2] > 5) return fail("model: pad-link pair p must have a link hull as geom2");
    if (s->pair_body1[p] != s->geom_body[g1] || s->pair_body2[p] != s->hull_body[k2]) return fail("model: pad-link pair bodies");
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: pad-link pairs must have condim 3 or 4");
    if (s->pair_margin[p] != 0) return fail("model: MPR pairs take no margin");
  }
  // the EE variant's mocap marker box (geom SO100_MOCAP_GEOM on the mocap body, centred on it: the kernels take its
  // pose as the mocap pose) against link hull k, through the convex collider
  if (s->geom_body[SO100_MOCAP_GEOM] != SO100_MOCAP_BODY) return fail("model: the marker box must sit on the mocap body");
  for (int k = 0; k < 3; k++)
    if (s->geom_pos[SO100_MOCAP_GEOM][k] != 0 || s->geom_quat[SO100_MOCAP_GEOM][1 + k] != 0)
      return fail("model: the marker box must be centred on the mocap body");
  for (int p = SO100_PAIR_MOCAPHULL0; p < SO100_PAIR_PAD0; p++) {
    const int k = p - SO100_PAIR_MOCAPHULL0;
    if (s->pair_geom1[p] != SO100_MOCAP_GEOM || s->pair_geom2[p] != -1 - k) return fail("model: pair p must be (marker, hull k)");
    if (s->pair_body1[p] != SO100_MOCAP_BODY || s->pair_body2[p] != s->hull_body[k]) return fail("model: marker-hull pair bodies");
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: marker pairs must have condim 3 or 4");
    if (s->pair_margin[p] != 0) return fail("model: MPR pairs take no margin");
  }
  // (cube | pad i, marker box) box-box pairs
  for (int p = SO100_PAIR_MOCAPBOX0; p < SO100_NPAIR; p++) {
    const int i = p - SO100_PAIR_MOCAPBOX0;
    if (s->pair_geom1[p] != (i == 0 ? SO100_CUBE_GEOM : i) || s->pair_geom2[p] != SO100_MOCAP_GEOM)
      return fail("model: pair p must be (cube | pad i, marker)");
    if (s->pair_body1[p] != s->geom_body[s->pair_geom1[p]] || s->pair_body2[p] != SO100_MOCAP_BODY)
      return fail("model: marker box pair bodies");
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: marker pairs must have condim 3 or 4");
  }
  // pad pairs: (finger pad i, table) at SO100_PAIR_PAD0 + i, (pad i, bin box j) at SO100_PAIR_PADBIN0 + 5 i + j
  for (int p = SO100_PAIR_PAD0; p < SO100_PAIR_MOCAPBOX0; p++) {
    const bool tbl = p < SO100_PAIR_PADBIN0;
    const int q = p - SO100_PAIR_PADBIN0;
    const int i = tbl ? p - SO100_PAIR_PAD0 : q / SO100_NBINBOX, j = tbl ? 0 : 1 + q % SO100_NBINBOX;
    const int g1 = s->pair_geom1[p], g2 = s->pair_geom2[p];
    if (g1 != 1 + i || g2 != (j == 0 ? 0 : SO100_CUBE_GEOM + j)) return fail("model: pad pair p must be (pad i, table | bin box j)");
    if (s->geom_body[g1] != 6 && s->geom_body[g1] != 7) return fail("model: pads must sit on the jaws");
    if (s->geom_body[g2] != 0) return fail("model: table and bin boxes must be static");
    if (s->pair_body1[p] != s->geom_body[g1] || s->pair_body2[p] != 0) return fail("model: pad pair bodies");
    if (s->pair_condim[p] != 3 && s->pair_condim[p] != 4) return fail("model: pad pairs must have condim 3 or 4");
  }
  for (int g = 0; g < SO100_NGEOM; g++) {
    int b = s->geom_body[g];
    if (!(b == 0 || b == 6 || b == 7 || b == SO100_CUBE_BODY || (g == SO100_MOCAP_GEOM && b == SO100_MOCAP_BODY)))
      return fail("model: geoms must be static, on the jaws, the cube or (the marker) the mocap body");
  }

  {
    double bq[4], bm[9];
    normq(s->body_quat[1], bq);
    quat2mat(bq, bm);
    for (int k = 0; k < 9; k++) d->base_xmat[k] = (float)bm[k];
    for (int k = 0; k < 3; k++) d->base_xpos[k] = (float)s->body_pos[1][k];
  }
  d->timestep = (float)s->timestep;
  d->nsubstep = s->nsubstep;
  d->iterations = s->iterations;
  if (s->solver != SO100_SOLVER_PGS && s->solver != SO100_SOLVER_NEWTON) return fail("model: unknown solver");
  d->solver = s->solver;
  if (s->convex != SO100_CONVEX_MPR && s->convex != SO100_CONVEX_EPA) return fail("model: unknown convex collider");
  d->convex = s->convex;
  d->tolerance = (float)s->tolerance;
  d->impratio = (float)s->impratio;
  for (int k = 0; k < 3; k++) d->gravity[k] = (float)s->gravity[k];
  d->pgs_scale = (float)(1.0 / (s->meaninertia * SO100_NV));
  double bq[4];
  normq(s->body_quat[1], bq);
  for (int k = 0; k < 3; k++) d->base_pos[k] = (float)s->body_pos[1][k];
  for (int k = 0; k < 4; k++) d->base_quat[k] = (float)bq[k];
  for (int a = 0; a < 6; a++) {
    int b = a + 2;
    double q[4], im[9];
    normq(s->body_quat[b], q);
    for (int k = 0; k < 3; k++) d->body_pos[a][k] = (float)s->body_pos[b][k];
    for (int k = 0; k < 4; k++) d->body_quat[a][k] = (float)q[k];
    for (int k = 0; k < 3; k++) d->body_ipos[a][k] = (float)s->body_ipos[b][k];
    normq(s->body_iquat[b], q);
    quat2mat(q, im);
    for (int k = 0; k < 9; k++) d->body_imat[a][k] = (float)im[k];
    d->body_mass[a] = (float)s->body_mass[b];
    for (int k = 0; k < 3; k++) d->body_inertia[a][k] = (float)s->body_inertia[b][k];
    for (int k = 0; k < 3; k++) d->jnt_axis[a][k] = (float)s->jnt_axis[a][k];
    d->jnt_lo[a] = (float)s->jnt_range[a][0];
    d->jnt_hi[a] = (float)s->jnt_range[a][1];
    d->armature[a] = (float)s->dof_armature[a];
  }
  d->cube_mass = (float)s->body_mass[SO100_CUBE_BODY];
  for (int k = 0; k < 3; k++) d->cube_inertia[k] = (float)s->body_inertia[SO100_CUBE_BODY][k];
  // frictionloss rows: pos = 0 -> imp = dmin; R = (1-imp)/imp * dof_invweight0
  double K, B;
  const double fimp = imp_at_zero(s->dof_solimp);
  for (int k = 0; k < SO100_NV; k++) {
    d->fr_floss[k] = (float)s->dof_frictionloss[k];
    double R = (1 - fimp) / fimp * s->dof_invweight0[k];
    d->fr_R[k] = (float)(R > 1e-15 ? R : 1e-15);
    if (!(s->dof_frictionloss[k] > 0)) return fail("model: the kernel expects frictionloss on every dof");
  }
  solref_kb(s->dof_solref, s->dof_solimp, s->timestep, &K, &B);
  d->fr_B = (float)B;
  solref_kb(s->jnt_solref, s->jnt_solimp, s->timestep, &K, &B);
  d->lim_K = (float)K;
  d->lim_B = (float)B;
  for (int k = 0; k < 5; k++) d->lim_solimp[k] = (float)s->jnt_solimp[k];
  // the kernels' impedance (so100_dynamics.h getimpedance) takes solimp power 1 or 2 (MuJoCo's power, clamped at 1)
  auto power_ok = [](const double* si) { const double pw = si[4] < 1 ? 1 : si[4]; return pw == 1 || pw == 2; };
  if (!power_ok(s->jnt_solimp) || !power_ok(s->dof_solimp) || !power_ok(s->weld_solimp))
    return fail("model: solimp power must be 1 or 2");
  for (int p = 0; p < SO100_NPAIR; p++)
    if (!power_ok(s->pair_solimp[p])) return fail("model: solimp power must be 1 or 2");
  for (int j = 0; j < 6; j++) d->lim_invw[j] = (float)s->dof_invweight0[j];
  for (int i = 0; i < SO100_NU; i++) {
    d->act_kp[i] = (float)s->act_kp[i];
    d->act_kv[i] = (float)s->act_kv[i];
    d->act_flo[i] = (float)s->act_forcerange[i][0];
    d->act_fhi[i] = (float)s->act_forcerange[i][1];
    d->act_clo[i] = (float)s->act_ctrlrange[i][0];
    d->act_chi[i] = (float)s->act_ctrlrange[i][1];
  }
  for (int g = 0; g < SO100_NGEOM; g++) {
    double q[4], gm[9];
    normq(s->geom_quat[g], q);
    quat2mat(q, gm);
    d->geom_body[g] = s->geom_body[g];
    for (int k = 0; k < 3; k++) d->geom_pos[g][k] = (float)s->geom_pos[g][k];
    for (int k = 0; k < 9; k++) d->geom_mat[g][k] = (float)gm[k];
    for (int k = 0; k < 3; k++) d->geom_size[g][k] = (float)s->geom_size[g][k];
    d->geom_rbound[g] = (float)sqrt(s->geom_size[g][0] * s->geom_size[g][0] + s->geom_size[g][1] * s->geom_size[g][1] +
                                    s->geom_size[g][2] * s->geom_size[g][2]);
  }
  for (int k = 0; k < 3; k++) { d->bin_lo[k] = 1e30f; d->bin_hi[k] = -1e30f; }
  for (int g = SO100_CUBE_GEOM + 1; g < SO100_CUBE_GEOM + 1 + SO100_NBINBOX; g++) {
    double q[4], gm[9];
    normq(s->geom_quat[g], q);
    quat2mat(q, gm);
    for (int k = 0; k < 3; k++) {
      const double r = fabs(gm[3 * k]) * s->geom_size[g][0] + fabs(gm[3 * k + 1]) * s->geom_size[g][1] +
                       fabs(gm[3 * k + 2]) * s->geom_size[g][2];
      d->bin_lo[k] = fminf(d->bin_lo[k], (float)(s->geom_pos[g][k] - r));
      d->bin_hi[k] = fmaxf(d->bin_hi[k], (float)(s->geom_pos[g][k] + r));
    }
  }
  for (int p = 0; p < SO100_NPAIR; p++) {
    // geoms: 0 <= g < SO100_NGEOM, or a hull -1 - k with 0 <= k < SO100_NHULL_ALL
    for (int g : {s->pair_geom1[p], s->pair_geom2[p]})
      if (g >= SO100_NGEOM || (g < 0 && -1 - g >= SO100_NHULL_ALL)) return fail("model: pair geom out of range");
    d->pair_g1[p] = s->pair_geom1[p];
    d->pair_g2[p] = s->pair_geom2[p];
    solref_kb(s->pair_solref[p], s->pair_solimp[p], s->timestep, &K, &B);
    d->pair_K[p] = (float)K;
    d->pair_B[p] = (float)B;
    for (int k = 0; k < 5; k++) d->pair_solimp[p][k] = (float)s->pair_solimp[p][k];
    d->pair_mu0[p] = (float)s->pair_friction[p][0];
    d->pair_mu1[p] = (float)s->pair_friction[p][1];
    d->pair_margin[p] = (float)s->pair_margin[p];
    const int b1 = s->pair_body1[p], b2 = s->pair_body2[p];
    // bodies 0..SO100_NBODY-1, or the mocap body (no dofs, welded to the world for the dynamics: invweight0 = 0)
    if (b1 < 0 || b1 > SO100_NBODY || b2 < 0 || b2 > SO100_NBODY) return fail("model: pair body out of range");
    static_assert(SO100_MOCAP_BODY == SO100_NBODY, "the mocap body follows the body arrays");
    // the kernels' box pairs take a geom's body from the pair (geom_pose_b)
    if ((s->pair_geom1[p] >= 0 && s->geom_body[s->pair_geom1[p]] != b1) ||
        (s->pair_geom2[p] >= 0 && s->geom_body[s->pair_geom2[p]] != b2))
      return fail("model: pair bodies must be their geoms' bodies");
    d->pair_b1[p] = b1;
    d->pair_b2[p] = b2;
    d->pair_cond4[p] = s->pair_condim[p] == 4;
    d->pair_arm[p] = (b1 >= 2 && b1 <= 7) || (b2 >= 2 && b2 <= 7);
    d->pair_cube[p] = b1 == SO100_CUBE_BODY || b2 == SO100_CUBE_BODY;
    auto invw = [&](int b, int k) { return b == SO100_MOCAP_BODY ? 0.0 : s->body_invweight0[b][k]; };
    d->pair_tran[p] = (float)(invw(b1, 0) + invw(b2, 0));
    d->pair_rot[p] = (float)(invw(b1, 1) + invw(b2, 1));
  }
  for (int k = 0; k < SO100_NHULL_ALL; k++) {
    // the convex collider's support ids hold a vertex index in 10 bits (so100_convex.h sup_from_id)
    if (s->hull_start[k] < 0 || s->hull_count[k] < 1 || s->hull_count[k] > 1024 ||
        s->hull_start[k] + s->hull_count[k] > SO100_HULL_NVERT)
      return fail("model: hull vertex range out of bounds (at most 1024 vertices per hull)");
    d->hull_body[k] = s->hull_body[k];
    d->hull_start[k] = s->hull_start[k];
    d->hull_count[k] = s->hull_count[k];
    d->hull_center[k] = {(float)s->hull_center[k][0], (float)s->hull_center[k][1], (float)s->hull_center[k][2], 0.f};
    d->hull_half[k] = {(float)s->hull_half[k][0], (float)s->hull_half[k][1], (float)s->hull_half[k][2],
                       (float)sqrt(s->hull_half[k][0] * s->hull_half[k][0] + s->hull_half[k][1] * s->hull_half[k][1] +
                                   s->hull_half[k][2] * s->hull_half[k][2])};
    d->hull_centroid[k] = {(float)s->hull_centroid[k][0], (float)s->hull_centroid[k][1], (float)s->hull_centroid[k][2], 0.f};
  }
  for (int v = 0; v < SO100_HULL_NVERT; v++)
    d->hull_vert[v] = {(float)s->hull_vert[v][0], (float)s->hull_vert[v][1], (float)s->hull_vert[v][2], 0.f};
  d->table_top = (float)s->table_top;
  d->table_bottom = (float)(s->table_top - 2 * s->geom_size[0][2]);
  for (int k = 0; k < 2; k++) {
    d->table_lo[k] = (float)s->table_lo[k];
    d->table_hi[k] = (float)s->table_hi[k];
  }
  for (int k = 0; k < 3; k++) {
    d->site_cube[k] = (float)s->site_cube_pos[k];
    d->site_ee[k] = (float)s->site_ee_pos[k];
    d->bin_center_f[k] = (float)s->bin_center[k];
    d->bin_center[k] = s->bin_center[k];
    d->spawn_lo[k] = s->spawn_lo[k];
    d->spawn_hi[k] = s->spawn_hi[k];
    d->goal_bin_lo[k] = (float)s->goal_bin_lo[k];
    d->goal_bin_hi[k] = (float)s->goal_bin_hi[k];
  }
  d->bin_hw = s->bin_hw;
  d->bin_h = s->bin_h;
  d->cube_half = s->cube_half;
  d->goal_threshold = s->goal_threshold;
  d->max_reward = s->max_reward;
  for (int i = 0; i < 6; i++) {
    d->start_qpos[i] = (float)s->start_qpos[i];
    d->action_lo[i] = (float)s->action_lo[i];
    d->action_hi[i] = (float)s->action_hi[i];
    d->action_span[i] = (float)(s->action_hi[i] - s->action_lo[i]);
  }
  // EE / mocap weld
  if (s->ee != 0 && s->ee != 1) return fail("model: ee must be 0 or 1");
  d->ee = s->ee;
  {
    double q[4], R[9];
    normq(s->weld_quat2, q);
    quat2mat(q, R);
    for (int k = 0; k < 9; k++) d->weld_mat2[k] = (float)R[k];
    for (int k = 0; k < 3; k++) d->weld_pos2[k] = (float)s->weld_pos2[k];
    for (int k = 0; k < 5; k++) d->weld_solimp[k] = (float)s->weld_solimp[k];
    solref_kb(s->weld_solref, s->weld_solimp, s->timestep, &K, &B);
    d->weld_K = (float)K;
    d->weld_B = (float)B;
    d->weld_ts = (float)s->weld_torquescale;
    for (int k = 0; k < 2; k++) d->weld_invw[k] = (float)s->weld_invweight0[k];
    for (int k = 0; k < 3; k++) d->mocap0[k] = (float)s->mocap_pos0[k];
    normq(s->mocap_quat0, q);
    for (int k = 0; k < 4; k++) d->mocap0[3 + k] = (float)q[k];
    if (s->ee && !(s->weld_invweight0[0] > 0 && s->weld_invweight0[1] > 0 && s->weld_solimp[2] > 0))
      return fail("model: weld parameters");
  }
  return 0;
}
}  // namespace

// Every exported entry point runs its implementation inside try / catch: host-side allocations (std::vector, new)
// can throw std::bad_alloc, and no C++ exception may cross the C-ABI (include/so100.h).  The error becomes status
// -3 (NULL for so100_create) with the message in so100_last_error().
static int caught(const char* where) {
  try {
    throw;
  } catch (const std::bad_alloc&) {
    snprintf(g_err, sizeof(g_err), "%s: out of host memory", where);
  } catch (const std::exception& e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, e.what());
  } catch (...) {
    snprintf(g_err, sizeof(g_err), "%s: unknown C++ exception", where);
  }
  return -3;
}


static int so100_abi_version_impl(void) { return SO100_ABI_VERSION; }
static const char* so100_last_error_impl(void) { return g_err; }

// ---- support-direction cells of the hulls (so100_hull_cells, include/so100.h).  For each cube-map cell
// (face f: axis f / 2, sign f % 2; cell (cu, cv) of u = n_a / |n_axis|, v = n_b / |n_axis|, a < b the other
// axes) the candidates are the vertices not beaten over the whole cell by one vertex of a sample support set
// S by >= kCellMargin: (v_j - v_i) . d is affine in (u, v), so its minimum over the (widened) cell is at a
// corner.  A vertex that is the support for some direction of the cell, or within kCellMargin of it, is never
// left out, so fp32 scans of the list and of the hull agree (the fp32 winner is within rounding, << the
// margin, of the exact maximum).  Deterministic: a function of the model only.
static constexpr double kCellWiden = 1e-3, kCellMargin = 1e-6;
static void hull_cells_build(const so100_model* s, std::vector<uint32_t>& cells, std::vector<float>& cand) {
  constexpr int G = SO100_HULL_CELLG;
  cells.assign((size_t)SO100_NHULL_ALL * SO100_HULL_NCELL, 0u);
  cand.clear();
  std::vector<double> V, P;
  std::vector<int> S;
  for (int k = 0; k < SO100_NHULL_ALL; k++) {
    const int n = s->hull_count[k], s0 = s->hull_start[k];
    V.resize(3 * (size_t)n);
    for (int i = 0; i < n; i++)
      for (int t = 0; t < 3; t++) V[3 * i + t] = (double)(float)s->hull_vert[s0 + i][t];   // the device's values
    P.resize(4 * (size_t)n);
    for (int f = 0; f < 6; f++) {
      const int ax = f / 2, a = ax == 0 ? 1 : 0, b = ax == 2 ? 1 : 2;
      const double sg = (f & 1) ? -1.0 : 1.0;
      for (int cu = 0; cu < G; cu++)
        for (int cv = 0; cv < G; cv++) {
          const double u0 = -1.0 + 2.0 * cu / G - kCellWiden, u1 = -1.0 + 2.0 * (cu + 1) / G + kCellWiden;
          const double v0 = -1.0 + 2.0 * cv / G - kCellWiden, v1 = -1.0 + 2.0 * (cv + 1) / G + kCellWiden;
          auto score = [&](int i, double u, double v) { return sg * V[3 * i + ax] + u * V[3 * i + a] + v * V[3 * i + b]; };
          // sample supports (first maximal vertex) on a 7 x 7 grid of the widened cell
          S.clear();
          for (int su = 0; su < 7; su++)
            for (int sv = 0; sv < 7; sv++) {
              const double u = u0 + (u1 - u0) * su / 6.0, v = v0 + (v1 - v0) * sv / 6.0;
              int bi = 0;
              double bs = score(0, u, v);
              for (int i = 1; i < n; i++) {
                const double sc = score(i, u, v);
                if (sc > bs) { bs = sc; bi = i; }
              }
              if (std::find(S.begin(), S.end(), bi) == S.end()) S.push_back(bi);
            }
          const double cu4[4] = {u0, u0, u1, u1}, cv4[4] = {v0, v1, v0, v1};
          for (int i = 0; i < n; i++)
            for (int c = 0; c < 4; c++) P[4 * i + c] = score(i, cu4[c], cv4[c]);
          const size_t start = cand.size() / 4;
          int cnt = 0;
          for (int i = 0; i < n; i++) {
            bool beaten = false;
            for (int j : S) {
              if (j == i) continue;
              double mn = P[4 * j] - P[4 * i];
              for (int c = 1; c < 4; c++) mn = std::min(mn, P[4 * j + c] - P[4 * i + c]);
              if (mn >= kCellMargin) { beaten = true; break; }
            }
            if (beaten) continue;
            float w;
            std::memcpy(&w, &i, sizeof(w));
            cand.insert(cand.end(), {(float)V[3 * i], (float)V[3 * i + 1], (float)V[3 * i + 2], w});
            cnt++;
          }
          uint32_t& e = cells[(size_t)k * SO100_HULL_NCELL + (size_t)(f * G + cu) * G + cv];
          if (cnt > 255 || start > 0xFFFFFFu) {
            cand.resize(start * 4);          // too many for the 8-bit count: the kernel scans the whole hull
            e = 0u;
          } else {
            e = (uint32_t)start << 8 | (uint32_t)cnt;
          }
        }
    }
  }
}

static int so100_hull_cells_impl(const so100_model* model, uint32_t* cells, float* cand, int cap) {
  if (!model) return fail("so100_hull_cells: model is NULL");
  for (int k = 0; k < SO100_NHULL_ALL; k++)
    if (model->hull_start[k] < 0 || model->hull_count[k] < 1 || model->hull_start[k] + model->hull_count[k] > SO100_HULL_NVERT)
      return fail("so100_hull_cells: hull vertex range");
  std::vector<uint32_t> c;
  std::vector<float> v;
  hull_cells_build(model, c, v);
  const int nc = (int)(v.size() / 4);
  if (cells) std::memcpy(cells, c.data(), c.size() * sizeof(uint32_t));
  if (cand) {
    if (cap < nc) return fail("so100_hull_cells: cap too small");
    std::memcpy(cand, v.data(), v.size() * sizeof(float));
  }
  return nc;
}

// The block table of the cells (so100_hull_blocks; on the device behind the model, so100_device.h kHullBlkOff): cell c's
// list as kCellBlk entries at c * kCellBlk, a list of 1..kCellBlk candidates padded with its last one, any other cell
// (no list, or a longer one) kCellBlk entries of zero coordinates and the index kCellBlkNone.
static void hull_blocks_build(const std::vector<uint32_t>& cells, const std::vector<float>& cand, std::vector<float>& blk) {
  float none;
  const uint32_t nb = so100::kCellBlkNone;
  std::memcpy(&none, &nb, sizeof(none));
  blk.assign(4 * cells.size() * so100::kCellBlk, 0.f);
  for (size_t c = 0; c < cells.size(); c++) {
    const uint32_t cnt = cells[c] & 255u, start = cells[c] >> 8;
    for (int i = 0; i < so100::kCellBlk; i++) {
      float* dst = &blk[4 * (c * so100::kCellBlk + i)];
      if (cnt >= 1u && cnt <= (uint32_t)so100::kCellBlk)
        std::memcpy(dst, &cand[4 * (size_t)(start + std::min<uint32_t>((uint32_t)i, cnt - 1u))], 4 * sizeof(float));
      else
        dst[3] = none;
    }
  }
}

static int so100_hull_blocks_impl(const so100_model* model, float* blk, int cap) {
  if (!model) return fail("so100_hull_blocks: model is NULL");
  for (int k = 0; k < SO100_NHULL_ALL; k++)
    if (model->hull_start[k] < 0 || model->hull_count[k] < 1 || model->hull_start[k] + model->hull_count[k] > SO100_HULL_NVERT)
      return fail("so100_hull_blocks: hull vertex range");
  std::vector<uint32_t> c;
  std::vector<float> v, b;
  hull_cells_build(model, c, v);
  hull_blocks_build(c, v, b);
  const int nb = (int)(b.size() / 4);
  if (blk) {
    if (cap < nb) return fail("so100_hull_blocks: cap too small");
    std::memcpy(blk, b.data(), b.size() * sizeof(float));
  }
  return nb;
}

static int so100_struct_sizes_impl(int* model_bytes, int* buffers_bytes) {
  if (model_bytes) *model_bytes = (int)sizeof(so100_model);
  if (buffers_bytes) *buffers_bytes = (int)sizeof(so100_buffers);
  return 0;
}

static so100_env* so100_create_impl(const so100_model* model, int n_envs, int device) {
  if (!model) { fail("so100_create: model is NULL"); return nullptr; }
  if (n_envs <= 0) { fail("so100_create: n_envs must be > 0"); return nullptr; }
  // the model check first: host-only, so a malformed model fails the same way with or without a device
  DevModel h;
  if (build_device_model(model, &h) != 0) return nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) { fail_hip("so100_create: no HIP device", e == hipSuccess ? hipErrorNoDevice : e); return nullptr; }
  if (device < 0 || device >= ndev) { fail("so100_create: device index out of range"); return nullptr; }
  DeviceGuard g(device);
  // the hulls' support cells: the table in the model, the candidates in their own buffer
  std::vector<uint32_t> hc;
  std::vector<float> hv;
  hull_cells_build(model, hc, hv);
  std::memcpy(h.hull_cells, hc.data(), sizeof(h.hull_cells));
  // the candidate lists in their own buffer (the list path of the cells whose list is longer than a block)
  if (hv.empty()) hv.assign(4, 0.f);
  float4* dcand = nullptr;
  e = hipMalloc(&dcand, hv.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(dcand, hv.data(), hv.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (dcand) (void)hipFree(dcand); fail_hip("so100_create: hull cells", e); return nullptr; }
  h.hull_cand = reinterpret_cast<const so100::float4_t*>(dcand);
  // the model and, behind it in the same allocation, the cells' block table (kHullBlkOff: the kernel's block address
  // is the model pointer plus a constant); the env owns the one allocation (d_model)
  std::vector<float> blk;
  hull_blocks_build(hc, hv, blk);
  if (blk.size() * sizeof(float) != so100::kHullBlkTotal) { (void)hipFree(dcand); fail("so100_create: block table size"); return nullptr; }
  DevModel* dm = nullptr;
  e = hipMalloc(&dm, so100::kHullBlkOff + so100::kHullBlkTotal);
  if (e != hipSuccess) { (void)hipFree(dcand); fail_hip("so100_create: hipMalloc", e); return nullptr; }
  h.hull_blk = reinterpret_cast<const so100::float4_t*>(reinterpret_cast<const char*>(dm) + so100::kHullBlkOff);
  e = hipMemcpy(dm, &h, sizeof(DevModel), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(reinterpret_cast<char*>(dm) + so100::kHullBlkOff, blk.data(), so100::kHullBlkTotal, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(dm); (void)hipFree(dcand); fail_hip("so100_create: hipMemcpy", e); return nullptr; }
  so100_env* env = new so100_env{device, n_envs, dm, h.nsubstep, h.solver, -1, kFusedAutoMax, {}, false, {}, nullptr, SO100_TASK_CUBE_TO_BIN, 700, 0, 0, {}, 0, 0};
  env->d_cand = dcand;
  env->ee = h.ee;
  if (const char* v = getenv("SO100_GRAPH")) env->use_graph = atoi(v) != 0;
  if (const char* v = getenv("SO100_FUSED")) env->fused = atoi(v) < 0 ? -1 : atoi(v) != 0;   // A/B: 0 split, 1 fused
  if (const char* v = getenv("SO100_FUSED_MAX")) env->fused_max = atoi(v);
  if (const char* v = getenv("SO100_PACK")) env->pack = atoi(v) < 0 ? -1 : atoi(v) != 0;   // A/B: 0 off, 1 on
  if (const char* v = getenv("SO100_FUSED_WAVES")) {
    const int w = atoi(v);
    env->fused_waves = (w == 2 || w == 3) ? w : 0;
  }
  // the split path's per-chunk workspaces (solver records) are allocated when the split path is first used
  // (here for PGS or a split default; else by so100_set_step_mode): each holds every env's whole contact list
  if (!step_is_fused(env)) e = make_chunks(env, default_chunks(n_envs));
  if (e == hipSuccess && env->solver == SO100_SOLVER_NEWTON) {
    // the fused launches: the record header (only its contact counts are written), the wave order, and the
    // contact record of the contacts beyond the kMaxCon held on chip
    e = so100::alloc_fused_workspace(n_envs, &env->fws);
  }
  if (e != hipSuccess) {
    (void)free_chunks(env);
    (void)hipFree(dm);
    (void)hipFree(dcand);
    delete env;
    fail_hip("so100_create: workspace", e);
    return nullptr;
  }
  return env;
}

static int so100_destroy_impl(so100_env* env) {
  if (!env) return 0;
  DeviceGuard g(env->device);
  profile_free(env);
  graph_free(env);
  if (env->cap_s) (void)hipStreamDestroy(env->cap_s);
  if (env->r_tri) (void)hipFree(env->r_tri);
  if (env->r_body) (void)hipFree(env->r_body);
  if (env->r_rgb) (void)hipFree(env->r_rgb);
  if (env->r_mat) (void)hipFree(env->r_mat);
  if (env->r_label) (void)hipFree(env->r_label);
  if (env->r_caster) (void)hipFree(env->r_caster);
  hipError_t e = hipFree(env->d_model);
  if (env->d_cand) (void)hipFree(env->d_cand);
  hipError_t e2 = free_chunks(env);
  if (e == hipSuccess) e = e2;
  if (e == hipSuccess) e = so100::free_workspace(&env->fws);
  else (void)so100::free_workspace(&env->fws);
  delete env;
  return e == hipSuccess ? 0 : fail_hip("so100_destroy", e);
}

static int so100_num_envs_impl(const so100_env* env) { return env ? env->n : -1; }

static int so100_configure_impl(so100_env* env, int task, int max_episode_steps, uint64_t base_seed, int env_offset) {
  if (!env) return fail("so100_configure: env is NULL");
  if (task < SO100_TASK_CUBE_TO_BIN || task > SO100_TASK_GOAL) return fail("so100_configure: unknown task");
  env->task = task;
  env->max_steps = max_episode_steps;
  env->base_seed = base_seed;
  if (env_offset < 0) return fail("so100_configure: env_offset < 0");
  env->env_offset = env_offset;
  graph_free(env);                           // kernel arguments changed
  return 0;
}

static int check_state(const so100_buffers* b) {
  if (!b) return fail("buffers is NULL");
  if (!b->qpos || !b->qvel || !b->qacc_warmstart) return fail("qpos/qvel/qacc_warmstart are required");
  return 0;
}

static int so100_reset_impl(so100_env* env, const so100_buffers* b, const uint8_t* mask, const uint32_t* seeds, void* stream) {
  if (!env) return fail("so100_reset: env is NULL");
  if (check_state(b)) return -1;
  if (env->task == SO100_TASK_GOAL && !b->desired_goal) return fail("so100_reset: GoalEnv needs desired_goal");
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_reset(env->d_model, *b, env->n, env->task, env->base_seed, env->env_offset, mask, seeds,
                                     (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_reset", e);
}

// The launches of one env step on stream s: chunk 0 on s, chunks 1.. on their own streams forked from s
// and joined back to it.  The profiling events (if any) ride on chunk 0.
static hipError_t enqueue_step(so100_env* env, const so100_buffers* b, int flags, hipStream_t s, hipEvent_t* ev) {
  env->last_fused = step_is_fused(env);
  if (env->last_fused) {
    // one launch over all n envs (every wave runs its whole env step: no chunks needed to fill the gaps)
    return so100::launch_step(env->d_model, env->nsubstep, env->solver, 1, env->fused_waves, env_packing(env), env->fws, *b, env->n, env->task, flags,
                              env->max_steps, env->base_seed, env->env_offset, s, ev);
  }
  if (env->chunks.empty()) return hipErrorNotReady;      // (so100_set_step_mode allocates them)
  if (env->chunks.size() == 1) {
    Chunk& c = env->chunks[0];
    return so100::launch_step(env->d_model, env->nsubstep, env->solver, 0, 0, 0, c.ws, *b, c.count, env->task, flags, env->max_steps,
                              env->base_seed, env->env_offset, s, ev);
  }
  hipError_t e = hipEventRecord(env->fork, s);
  for (size_t k = 1; k < env->chunks.size() && e == hipSuccess; k++) {
    Chunk& c = env->chunks[k];
    e = hipStreamWaitEvent(c.s, env->fork, 0);
    if (e == hipSuccess)
      e = so100::launch_step(env->d_model, env->nsubstep, env->solver, 0, 0, 0, c.ws, offset_buffers(*b, c.start), c.count, env->task, flags,
                             env->max_steps, env->base_seed, env->env_offset + c.start, c.s, nullptr);
    if (e == hipSuccess) e = hipEventRecord(c.done, c.s);
  }
  Chunk& c0 = env->chunks[0];
  if (e == hipSuccess)
    e = so100::launch_step(env->d_model, env->nsubstep, env->solver, 0, 0, 0, c0.ws, *b, c0.count, env->task, flags, env->max_steps,
                           env->base_seed, env->env_offset, s, ev);
  for (size_t k = 1; k < env->chunks.size() && e == hipSuccess; k++) e = hipStreamWaitEvent(s, env->chunks[k].done, 0);
  return e;
}

// Capture the step for (b, flags) on the private capture stream and instantiate it into g.
// the split path's substep-counter parity (its PGS heavy-group lists alternate by it); the fused step has none
static uint32_t step_parity(const so100_env* env) {
  return (step_is_fused(env) || env->chunks.empty()) ? 0u : env->chunks[0].ws.sub_count & 1u;
}

static hipError_t build_step_graph(so100_env* env, const so100_buffers* b, int flags, StepGraph& g) {
  const uint32_t par = step_parity(env);
  hipError_t e = hipSuccess;
  if (!env->cap_s) e = hipStreamCreateWithFlags(&env->cap_s, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&g.done, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  e = hipStreamBeginCapture(env->cap_s, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return e;
  hipError_t el = enqueue_step(env, b, flags, env->cap_s, nullptr);
  hipGraph_t graph = nullptr;
  e = hipStreamEndCapture(env->cap_s, &graph);
  if (el != hipSuccess) e = el;
  if (e == hipSuccess) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (e != hipSuccess) { g.exec = nullptr; return e; }
  g.buf = *b;
  g.flags = flags;
  g.par = par;
  return hipSuccess;
}

// Replay the step graph for (b, flags) on s, capturing it first if it is not cached.
static hipError_t graph_step(so100_env* env, const so100_buffers* b, int flags, hipStream_t s) {
  const uint32_t par = step_parity(env);
  StepGraph* hit = nullptr;
  for (StepGraph& g : env->graphs)
    if (g.flags == flags && g.par == par && memcmp(&g.buf, b, sizeof(so100_buffers)) == 0) { hit = &g; break; }
  hipError_t e = hipSuccess;
  if (hit) {
    // the capture advanced the host substep counters as an eager step would; a replay does it here
    for (Chunk& c : env->chunks) c.ws.sub_count += (uint32_t)env->nsubstep;
  } else {
    if (env->graphs.size() >= kMaxStepGraphs) {
      size_t lru = 0;
      for (size_t i = 1; i < env->graphs.size(); i++)
        if (env->graphs[i].last_use < env->graphs[lru].last_use) lru = i;
      graph_destroy(env->graphs[lru]);
      env->graphs.erase(env->graphs.begin() + (long)lru);
    }
    StepGraph g;
    e = build_step_graph(env, b, flags, g);
    if (e != hipSuccess) { graph_destroy(g); return e; }
    env->graphs.push_back(g);
    hit = &env->graphs.back();
  }
  hit->last_use = ++env->graph_clock;
  e = hipGraphLaunch(hit->exec, s);
  if (e == hipSuccess) e = hipEventRecord(hit->done, s);
  return e;
}

static int so100_step_impl(so100_env* env, const so100_buffers* b, int flags, void* stream) {
  if (!env) return fail("so100_step: env is NULL");
  if (check_state(b)) return -1;
  if (!b->action) return fail("so100_step: action is NULL");
  if (env->task == SO100_TASK_GOAL && !b->desired_goal) return fail("so100_step: GoalEnv needs desired_goal");
  if ((flags & SO100_FLAG_DR) && !b->dr_params) return fail("so100_step: FLAG_DR needs dr_params");
  if ((flags & SO100_FLAG_AUTORESET) && !b->episode) return fail("so100_step: FLAG_AUTORESET needs episode");
  DeviceGuard g(env->device);
  hipEvent_t* ev = nullptr;
  if (env->prof_used < env->prof_cap) ev = env->prof_ev.data() + (size_t)(env->prof_used++) * env->prof_per;
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if (env->use_graph && !ev) {
    e = graph_step(env, b, flags, s);
  } else {
    e = enqueue_step(env, b, flags, s, ev);
  }
  return e == hipSuccess ? 0 : fail_hip("so100_step", e);
}

static int so100_profile_enable_impl(so100_env* env, int max_steps) {
  if (!env) return fail("so100_profile_enable: env is NULL");
  if (max_steps < 0) return fail("so100_profile_enable: max_steps < 0");
  DeviceGuard g(env->device);
  profile_free(env);
  env->prof_per = step_is_fused(env) ? 2 : 2 * env->nsubstep + 2;
  const size_t count = (size_t)max_steps * env->prof_per;
  env->prof_ev.resize(count);
  for (size_t i = 0; i < count; i++) {
    hipError_t e = hipEventCreate(&env->prof_ev[i]);
    if (e != hipSuccess) { env->prof_ev.resize(i); profile_free(env); return fail_hip("so100_profile_enable", e); }
  }
  env->prof_cap = max_steps;
  return 0;
}

static int so100_profile_read_impl(so100_env* env, double* solver_ms, int* solver_launches, double* stage_ms, int* stage_launches) {
  if (!env || !solver_ms || !solver_launches || !stage_ms || !stage_launches) return fail("so100_profile_read: bad arguments");
  DeviceGuard g(env->device);
  *solver_ms = *stage_ms = 0.0;
  *solver_launches = *stage_launches = 0;
  const int per = env->prof_per;
  if (env->prof_used > 0) {
    hipError_t e = hipEventSynchronize(env->prof_ev[(size_t)env->prof_used * per - 1]);
    if (e != hipSuccess) return fail_hip("so100_profile_read", e);
  }
  for (int st = 0; st < env->prof_used; st++) {
    const hipEvent_t* ev = env->prof_ev.data() + (size_t)st * per;
    if (per == 2) {                        // fused: the one launch contains the solves
      float ms = 0.f;
      hipError_t e = hipEventElapsedTime(&ms, ev[0], ev[1]);
      if (e != hipSuccess) return fail_hip("so100_profile_read", e);
      *solver_ms += ms;
      (*solver_launches)++;
      continue;
    }
    for (int k = 0; k + 1 < per; k++) {   // launch order: stage, solver, stage, solver, ..., final stage
      float ms = 0.f;
      hipError_t e = hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
      if (e != hipSuccess) return fail_hip("so100_profile_read", e);
      if (k & 1) { *solver_ms += ms; (*solver_launches)++; }
      else { *stage_ms += ms; (*stage_launches)++; }
    }
  }
  return 0;
}

static int so100_set_step_mode_impl(so100_env* env, int fused) {
  if (!env) return fail("so100_set_step_mode: env is NULL");
  if (fused < -1 || fused > 1) return fail("so100_set_step_mode: mode must be -1 (auto), 0 (split) or 1 (fused)");
  if (env->prof_cap > 0) return fail("so100_set_step_mode: disable profiling first");
  DeviceGuard g(env->device);
  graph_free(env);                     // captured graphs hold the other mode's launches
  const int prev = env->fused;
  env->fused = fused;
  if (!step_is_fused(env) && env->chunks.empty()) {
    // first use of the split path: its chunk workspaces (one synchronising allocation, here, never in a step)
    hipError_t e = make_chunks(env, default_chunks(env->n));
    if (e != hipSuccess) {
      (void)free_chunks(env);
      env->fused = prev;
      return fail_hip("so100_set_step_mode: split workspace", e);
    }
  }
  return 0;
}

static int so100_step_mode_impl(const so100_env* env) {
  if (!env) return fail("so100_step_mode: env is NULL");
  return step_is_fused(env) ? 1 : 0;
}

static int so100_set_fused_build_impl(so100_env* env, int waves) {
  if (!env) return fail("so100_set_fused_build: env is NULL");
  if (waves != 0 && waves != 2 && waves != 3) return fail("so100_set_fused_build: waves must be 0 (auto), 2 or 3");
  if (env->prof_cap > 0) return fail("so100_set_fused_build: disable profiling first");
  DeviceGuard g(env->device);
  graph_free(env);                     // captured graphs hold the other build's launch
  env->fused_waves = waves;
  return 0;
}

static int so100_fused_build_impl(const so100_env* env, int debug) {
  if (!env) return fail("so100_fused_build: env is NULL");
  DeviceGuard g(env->device);
  return so100::fused_build(env->n, env->fused_waves, debug != 0);
}

static int so100_set_env_packing_impl(so100_env* env, int mode) {
  if (!env) return fail("so100_set_env_packing: env is NULL");
  if (mode < -1 || mode > 1) return fail("so100_set_env_packing: mode must be -1 (auto), 0 (off) or 1 (on)");
  if (env->prof_cap > 0) return fail("so100_set_env_packing: disable profiling first");
  DeviceGuard g(env->device);
  graph_free(env);                     // captured graphs hold the other mode's order launch
  env->pack = mode;
  return 0;
}

static int so100_env_order_impl(so100_env* env, int32_t* out, int cap) {
  if (!env || !out || cap < 0) return fail("so100_env_order: bad arguments");
  if (!env->fws.eorder) return fail("so100_env_order: no fused workspace");
  DeviceGuard g(env->device);
  const int rows = (env->n + 3) / 4 * 4, k = cap < rows ? cap : rows;
  if (!so100::fused_order_active(env->n)) {   // the launch takes the natural envs
    for (int i = 0; i < k; i++) out[i] = i;
    return 0;
  }
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && k > 0) e = hipMemcpy(out, env->fws.eorder, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : fail_hip("so100_env_order", e);
}

static int so100_wave_cost_impl(so100_env* env, uint32_t* out, int cap) {
  if (!env || !out || cap < 0) return fail("so100_wave_cost: bad arguments");
  if (!env->fws.gcost) return fail("so100_wave_cost: no fused workspace");
  DeviceGuard g(env->device);
  const int ng = (env->n + 3) / 4, k = cap < ng ? cap : ng;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && k > 0) e = hipMemcpy(out, env->fws.gcost, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : fail_hip("so100_wave_cost", e);
}

static int so100_chunk_info_impl(const so100_env* env, int* nchunks, int* profiled_envs) {
  if (!env) return fail("so100_chunk_info: env is NULL");
  if (nchunks) *nchunks = (int)env->chunks.size();
  if (step_is_fused(env)) {     // one launch over all envs
    if (nchunks) *nchunks = 1;
    if (profiled_envs) *profiled_envs = env->n;
    return 0;
  }
  if (nchunks && env->chunks.empty()) *nchunks = default_chunks(env->n);
  if (profiled_envs) *profiled_envs = env->chunks.empty() ? 0 : env->chunks[0].count;
  return 0;
}

static int so100_contact_count_impl(so100_env* env, uint64_t* accum, void* stream) {
  if (!env || !accum) return fail("so100_contact_count: bad arguments");
  DeviceGuard g(env->device);
  hipError_t e = hipSuccess;
  if (env->last_fused) {
    if (env->fws.hdr) e = so100::launch_contact_count(env->fws, env->n, accum, (hipStream_t)stream);
  } else {
    for (const Chunk& c : env->chunks)
      if (e == hipSuccess) e = so100::launch_contact_count(c.ws, c.count, accum, (hipStream_t)stream);
  }
  return e == hipSuccess ? 0 : fail_hip("so100_contact_count", e);
}

static int so100_contact_counts_impl(so100_env* env, int32_t* out, void* stream) {
  if (!env || !out) return fail("so100_contact_counts: bad arguments");
  DeviceGuard g(env->device);
  hipError_t e = hipSuccess;
  if (env->last_fused) {
    if (env->fws.hdr) e = so100::launch_contact_counts(env->fws, env->n, out, (hipStream_t)stream);
  } else {
    for (const Chunk& c : env->chunks)
      if (e == hipSuccess) e = so100::launch_contact_counts(c.ws, c.count, out + c.start, (hipStream_t)stream);
  }
  return e == hipSuccess ? 0 : fail_hip("so100_contact_counts", e);
}

static int so100_pool_stats_impl(so100_env* env, uint64_t* out, int reset) {
  if (!env || !out) return fail("so100_pool_stats: bad arguments");
  DeviceGuard g(env->device);
  unsigned long long st[2] = {0, 0};
  hipError_t e = hipSuccess;
  if (env->fws.pool_stat) {
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(st, env->fws.pool_stat, sizeof(st), hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) e = hipMemset(env->fws.pool_stat, 0, sizeof(st));
  }
  if (e != hipSuccess) return fail_hip("so100_pool_stats", e);
  out[0] = st[0];
  out[1] = st[1];
  out[2] = (uint64_t)env->fws.pool_recs;
  return 0;
}

static int so100_env_cost_impl(so100_env* env, uint32_t* out, int cap) {
  if (!env || !out || cap < 0) return fail("so100_env_cost: bad arguments");
  if (!env->fws.ecost) return fail("so100_env_cost: no fused workspace");
  DeviceGuard g(env->device);
  const int k = cap < env->n ? cap : env->n;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && k > 0) e = hipMemcpy(out, env->fws.ecost, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : fail_hip("so100_env_cost", e);
}

static int so100_goal_reward_impl(so100_env* env, int n, const float* a, const float* d, float* out, void* stream) {
  if (!env || !a || !d || !out || n < 0) return fail("so100_goal_reward: bad arguments");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_goal_reward(env->d_model, n, a, d, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_goal_reward", e);
}

static int so100_eval_reward_impl(so100_env* env, int task, int n, const float* cube, const float* ee, const uint32_t* bits,
                      float* out, void* stream) {
  if (!env || !cube || !ee || !bits || !out || n < 0) return fail("so100_eval_reward: bad arguments");
  if (task < SO100_TASK_CUBE_TO_BIN || task > SO100_TASK_GOAL) return fail("so100_eval_reward: unknown task");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_reward(env->d_model, task, n, cube, ee, bits, out, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_eval_reward", e);
}

static int so100_spawn_pose_impl(so100_env* env, int n, const uint32_t* seeds, double* pose, void* stream) {
  if (!env || !seeds || !pose || n < 0) return fail("so100_spawn_pose: bad arguments");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_spawn(env->d_model, n, seeds, pose, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_spawn_pose", e);
}

static int so100_unnormalize_impl(so100_env* env, int n, const float* action, float* ctrl, void* stream) {
  if (!env || !action || !ctrl || n < 0) return fail("so100_unnormalize: bad arguments");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_unnormalize(env->d_model, n, action, ctrl, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_unnormalize", e);
}


static int so100_render_mesh_impl(so100_env* env, const float* tri, const int* body, const float* rgb, int ntri) {
  if (!env || !tri || !body || !rgb || ntri <= 0) return fail("so100_render_mesh: bad arguments");
  std::vector<float4> t((size_t)ntri * 3);
  std::vector<uint32_t> c((size_t)ntri);
  for (int i = 0; i < ntri; i++) {
    if (body[i] < 0 || body[i] >= SO100_NBODY) return fail("so100_render_mesh: body out of range");
    for (int v = 0; v < 3; v++) {
      const float* p = tri + (size_t)9 * i + 3 * v;
      t[(size_t)3 * i + v] = make_float4(p[0], p[1], p[2], 0.f);
    }
    uint32_t col = 0;
    for (int k = 0; k < 3; k++) {
      const float x = rgb[(size_t)3 * i + k] < 0.f ? 0.f : (rgb[(size_t)3 * i + k] > 1.f ? 1.f : rgb[(size_t)3 * i + k]);
      col |= (uint32_t)(x * 255.f + 0.5f) << (8 * k);
    }
    c[i] = col;
  }
  DeviceGuard g(env->device);
  if (env->r_tri) (void)hipFree(env->r_tri);
  if (env->r_body) (void)hipFree(env->r_body);
  if (env->r_rgb) (void)hipFree(env->r_rgb);
  if (env->r_mat) (void)hipFree(env->r_mat);
  if (env->r_label) (void)hipFree(env->r_label);
  if (env->r_caster) (void)hipFree(env->r_caster);
  env->r_tri = nullptr; env->r_body = nullptr; env->r_rgb = nullptr; env->r_mat = nullptr; env->r_label = nullptr;
  env->r_caster = nullptr;
  env->r_ntri = 0;
  hipError_t e = hipMalloc(&env->r_tri, t.size() * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc(&env->r_body, (size_t)ntri * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&env->r_rgb, (size_t)ntri * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(env->r_tri, t.data(), t.size() * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(env->r_body, body, (size_t)ntri * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(env->r_rgb, c.data(), (size_t)ntri * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail_hip("so100_render_mesh", e);
  env->r_ntri = ntri;
  return 0;
}

// the one render launch behind so100_render (hwc alone), so100_render_to, with a record per env (views != nullptr)
// so100_render_views and, with the depth / label sinks (aux != nullptr, views or not), so100_render_aux; `who` names the
// entry point in errors
static int render_launch(const char* who, so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                         int width, int height, const so100_image_out& o, void* stream,
                         const so100_view* views = nullptr, const so100_aux_out* aux = nullptr) {
  char msg[160];
  auto bad = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return fail(msg);
  };
  if (!env || !qpos || !cam) return bad("bad arguments");
  // (so100_render_aux has looked for a sink across both structs before it comes here)
  if (!aux && !o.hwc && !o.chw && !o.flat) return bad("no sink (hwc, chw and flat are all NULL)");
  if (env->r_ntri <= 0) return bad("no render mesh (so100_render_mesh)");
  if (width <= 0 || height <= 0 || width > 4096 || (long)width * height > (1L << 22))
    return bad("bad image size (width <= 4096, width*height <= 2^22)");
  if (o.flat && o.flat_pitch < (int64_t)3 * width * height) return bad("flat_pitch < 3*H*W");
  if (cam->nlight < 0 || cam->nlight > SO100_MAX_LIGHTS || !(cam->fovy > 0.f && cam->fovy < 180.f))
    return bad("bad camera");
  if (views && !env->r_mat) return bad("no materials (so100_render_materials)");
  if (aux && aux->label && !env->r_label) return bad("no labels (so100_render_labels)");
  DeviceGuard g(env->device);
  if (aux) {
    hipError_t e = so100::launch_render_aux(env->d_model, env->r_tri, env->r_body, env->r_rgb, env->r_mat, env->r_label,
                                            env->r_ntri, qpos, mask, *cam, views, env->n, width, height, o, *aux,
                                            (hipStream_t)stream);
    return e == hipSuccess ? 0 : fail_hip(who, e);
  }
  hipError_t e = views ? so100::launch_render_views(env->d_model, env->r_tri, env->r_body, env->r_mat, env->r_ntri, qpos,
                                                    mask, *cam, views, env->n, width, height, o, (hipStream_t)stream)
                       : so100::launch_render(env->d_model, env->r_tri, env->r_body, env->r_rgb, env->r_ntri, qpos, mask,
                                              *cam, env->n, width, height, o, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(who, e);
}

static int so100_render_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam, int width,
                 int height, uint8_t* out, void* stream) {
  if (!out) return fail("so100_render: bad arguments");
  so100_image_out o{(uint32_t)sizeof(so100_image_out), out, nullptr, nullptr, 0};
  return render_launch("so100_render", env, qpos, mask, cam, width, height, o, stream);
}

static int so100_render_to_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                                int width, int height, const so100_image_out* out, void* stream) {
  // the struct's size first: nothing else of *out is read before it is known to be this library's layout
  if (!out) return fail("so100_render_to: NULL out");
  if (out->size != sizeof(so100_image_out)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "so100_render_to: so100_image_out.size %u, expected %zu", out->size,
             sizeof(so100_image_out));
    return fail(msg);
  }
  if (!env) return fail("so100_render_to: NULL env");
  return render_launch("so100_render_to", env, qpos, mask, cam, width, height, *out, stream);
}

// the size check of a caller-filled struct: nothing else of it is read before it is known to be this library's layout
static int size_mismatch(const char* who, const char* what, uint32_t got, size_t want) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s.size %u, expected %zu", who, what, got, want);
  return fail(msg);
}

static int so100_render_materials_impl(so100_env* env, const uint8_t* material, int ntri) {
  if (!env || !material) return fail("so100_render_materials: bad arguments");
  if (env->r_ntri <= 0) return fail("so100_render_materials: no render mesh (so100_render_mesh)");
  if (ntri != env->r_ntri) {
    char msg[160];
    snprintf(msg, sizeof(msg), "so100_render_materials: ntri %d, the mesh has %d", ntri, env->r_ntri);
    return fail(msg);
  }
  for (int i = 0; i < ntri; i++)
    if (material[i] >= SO100_NMATERIAL) return fail("so100_render_materials: material id out of range");
  DeviceGuard g(env->device);
  hipError_t e = hipSuccess;
  if (!env->r_mat) e = hipMalloc(&env->r_mat, (size_t)ntri);
  if (e == hipSuccess) e = hipMemcpy(env->r_mat, material, (size_t)ntri, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (env->r_mat) (void)hipFree(env->r_mat);
    env->r_mat = nullptr;
    return fail_hip("so100_render_materials", e);
  }
  return 0;
}

static int so100_render_views_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                                   const so100_view* views, int width, int height, const so100_image_out* out,
                                   void* stream) {
  if (!out) return fail("so100_render_views: NULL out");
  if (out->size != sizeof(so100_image_out))
    return size_mismatch("so100_render_views", "so100_image_out", out->size, sizeof(so100_image_out));
  if (!env) return fail("so100_render_views: NULL env");
  if (!views) return fail("so100_render_views: NULL views");
  return render_launch("so100_render_views", env, qpos, mask, cam, width, height, *out, stream, views);
}

static int so100_render_labels_impl(so100_env* env, const uint8_t* label, int ntri) {
  if (!env || !label) return fail("so100_render_labels: bad arguments");
  if (env->r_ntri <= 0) return fail("so100_render_labels: no render mesh (so100_render_mesh)");
  if (ntri != env->r_ntri) {
    char msg[160];
    snprintf(msg, sizeof(msg), "so100_render_labels: ntri %d, the mesh has %d", ntri, env->r_ntri);
    return fail(msg);
  }
  for (int i = 0; i < ntri; i++)
    if (label[i] == 255) return fail("so100_render_labels: label 255 is the background's");
  DeviceGuard g(env->device);
  hipError_t e = hipSuccess;
  if (!env->r_label) e = hipMalloc(&env->r_label, (size_t)ntri);
  if (e == hipSuccess) e = hipMemcpy(env->r_label, label, (size_t)ntri, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (env->r_label) (void)hipFree(env->r_label);
    env->r_label = nullptr;
    return fail_hip("so100_render_labels", e);
  }
  return 0;
}

static int so100_render_aux_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                                 const so100_view* views, int width, int height, const so100_image_out* out,
                                 const so100_aux_out* aux, void* stream) {
  // the structs' sizes first: nothing else of them is read before they are known to be this library's layout
  if (out && out->size != sizeof(so100_image_out))
    return size_mismatch("so100_render_aux", "so100_image_out", out->size, sizeof(so100_image_out));
  if (aux && aux->size != sizeof(so100_aux_out))
    return size_mismatch("so100_render_aux", "so100_aux_out", aux->size, sizeof(so100_aux_out));
  if (!(out && (out->hwc || out->chw || out->flat)) && !(aux && (aux->depth || aux->label)))
    return fail("so100_render_aux: no sink (hwc, chw, flat, depth and label are all NULL)");
  if (!env) return fail("so100_render_aux: NULL env");
  const so100_image_out none{(uint32_t)sizeof(so100_image_out), nullptr, nullptr, nullptr, 0};
  const so100_aux_out no_aux{(uint32_t)sizeof(so100_aux_out), nullptr, nullptr};
  return render_launch("so100_render_aux", env, qpos, mask, cam, width, height, out ? *out : none, stream, views,
                       aux ? aux : &no_aux);
}

// the launch over (env, camera): so100_render_aux's checks, per camera where they are the camera's.  With sh it is
// so100_render_shadow (`who` names the call in the messages): the same checks, then the shadow struct's.  With ms it is
// so100_render_msaa (aux NULL): the same checks with the sample struct's among those the arguments alone decide
static int cams_launch(const char* who, so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                       const so100_view* views, int width, int height, const so100_image_out* out,
                       const so100_aux_out* aux, const so100_shadow* sh, void* stream, const so100_msaa* ms = nullptr) {
  // the structs' sizes first: nothing else of them is read before they are known to be this library's layout
  if (ms && ms->size != sizeof(so100_msaa)) return size_mismatch(who, "so100_msaa", ms->size, sizeof(so100_msaa));
  if (cams && cams->size != sizeof(so100_cams)) return size_mismatch(who, "so100_cams", cams->size, sizeof(so100_cams));
  if (out && out->size != sizeof(so100_image_out))
    return size_mismatch(who, "so100_image_out", out->size, sizeof(so100_image_out));
  if (aux && aux->size != sizeof(so100_aux_out))
    return size_mismatch(who, "so100_aux_out", aux->size, sizeof(so100_aux_out));
  if (sh && sh->size != sizeof(so100_shadow))
    return size_mismatch(who, "so100_shadow", sh->size, sizeof(so100_shadow));
  char msg[200];
  auto bad = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return fail(msg);
  };
  if (!cams) return bad("NULL cams");
  if (cams->ncam < 1 || cams->ncam > SO100_MAX_CAMS) {
    snprintf(msg, sizeof(msg), "%s: ncam %d, expected 1..%d", who, cams->ncam, SO100_MAX_CAMS);
    return fail(msg);
  }
  for (int c = 0; c < cams->ncam; c++)
    if (cams->frame_body[c] < 0 || cams->frame_body[c] >= SO100_NBODY) {
      snprintf(msg, sizeof(msg), "%s: frame_body[%d] %d, expected 0 (world) or 1..%d", who, c, cams->frame_body[c],
               SO100_NBODY - 1);
      return fail(msg);
    }
  // what the arguments alone decide comes before the env is looked at
  const int K = cams->ncam;
  if (width <= 0 || height <= 0 || width > 4096 || (long)width * height * K > (1L << 22))
    return bad("bad image size (width <= 4096, width*height*ncam <= 2^22)");
  if (out && out->flat && out->flat_pitch < (int64_t)3 * width * height * K) return bad("flat_pitch < ncam*3*H*W");
  if (ms) {
    if (ms->samples != 1 && ms->samples != 2 && ms->samples != 4) {
      snprintf(msg, sizeof(msg), "%s: samples %d, expected 1, 2 or 4", who, ms->samples);
      return fail(msg);
    }
    for (int k = 0; k < ms->samples; k++)
      for (int j = 0; j < 2; j++)
        if (!(std::isfinite(ms->offset[k][j]) && std::fabs(ms->offset[k][j]) < 0.5f)) {
          snprintf(msg, sizeof(msg), "%s: offset[%d][%d] must be finite and inside (-0.5, 0.5)", who, k, j);
          return fail(msg);
        }
    if (width * ms->samples > 4096) {
      snprintf(msg, sizeof(msg), "%s: width %d * samples %d > 4096 (a band is at least one row of samples)", who,
               width, ms->samples);
      return fail(msg);
    }
    if (!out) return bad("NULL out");
    if (!(out->hwc || out->chw || out->flat)) return bad("no colour sink (hwc, chw and flat are all NULL)");
  }
  if (!(out && (out->hwc || out->chw || out->flat)) && !(aux && (aux->depth || aux->label)) &&
      !(sh && sh->shadow_out))
    return bad(sh ? "no sink (hwc, chw, flat, depth, label and shadow_out are all NULL)"
                  : "no sink (hwc, chw, flat, depth and label are all NULL)");
  if (!env) return bad("NULL env");
  if (!qpos) return bad("bad arguments");
  if (env->r_ntri <= 0) return bad("no render mesh (so100_render_mesh)");
  for (int c = 0; c < K; c++) {
    const so100_camera& cam = cams->cam[c];
    if (cam.nlight < 0 || cam.nlight > SO100_MAX_LIGHTS || !(cam.fovy > 0.f && cam.fovy < 180.f)) {
      snprintf(msg, sizeof(msg), "%s: bad camera %d", who, c);
      return fail(msg);
    }
  }
  if (views && !env->r_mat) return bad("no materials (so100_render_materials)");
  if (aux && aux->label && !env->r_label) return bad("no labels (so100_render_labels)");
  const so100_image_out none{(uint32_t)sizeof(so100_image_out), nullptr, nullptr, nullptr, 0};
  const so100_aux_out no_aux{(uint32_t)sizeof(so100_aux_out), nullptr, nullptr};
  if (sh) {
    for (int c = 0; c < K; c++)
      if (sh->light < -1 || sh->light >= cams->cam[c].nlight) {
        snprintf(msg, sizeof(msg), "%s: light %d, expected -1 (none) or 0..%d (camera %d's lights)", who, sh->light,
                 cams->cam[c].nlight - 1, c);
        return fail(msg);
      }
    if (sh->map_size < 8 || sh->map_size > SO100_SHADOW_MAP_MAX || sh->map_size % 8 != 0) {
      snprintf(msg, sizeof(msg), "%s: map_size %d, expected a multiple of 8 in 8..%d (the map lives in LDS)", who,
               sh->map_size, SO100_SHADOW_MAP_MAX);
      return fail(msg);
    }
    if (!(std::isfinite(sh->radius) && sh->radius > 0.f)) return bad("radius must be finite and > 0");
    if (!(std::isfinite(sh->bias) && sh->bias >= 0.f)) return bad("bias must be finite and >= 0");
    if (!(std::isfinite(sh->center[0]) && std::isfinite(sh->center[1]) && std::isfinite(sh->center[2])))
      return bad("center must be finite");
    if (!env->r_caster) return bad("no casters (so100_render_casters)");
    DeviceGuard g(env->device);
    hipError_t e = so100::launch_render_shadow(env->d_model, env->r_tri, env->r_body, env->r_rgb, env->r_mat,
                                               env->r_label, env->r_caster, env->r_ntri, qpos, mask, *cams, views,
                                               env->n, width, height, out ? *out : none, aux ? *aux : no_aux, *sh,
                                               (hipStream_t)stream);
    return e == hipSuccess ? 0 : fail_hip(who, e);
  }
  if (ms) {
    DeviceGuard g(env->device);
    hipError_t e = so100::launch_render_msaa(env->d_model, env->r_tri, env->r_body, env->r_rgb, env->r_mat, env->r_ntri,
                                             qpos, mask, *cams, views, env->n, width, height, *out, *ms,
                                             (hipStream_t)stream);
    return e == hipSuccess ? 0 : fail_hip(who, e);
  }
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_render_cams(env->d_model, env->r_tri, env->r_body, env->r_rgb, env->r_mat, env->r_label,
                                           env->r_ntri, qpos, mask, *cams, views, env->n, width, height,
                                           out ? *out : none, aux ? *aux : no_aux, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(who, e);
}

static int so100_render_cams_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                                  const so100_view* views, int width, int height, const so100_image_out* out,
                                  const so100_aux_out* aux, void* stream) {
  return cams_launch("so100_render_cams", env, qpos, mask, cams, views, width, height, out, aux, nullptr, stream);
}

static int so100_render_casters_impl(so100_env* env, const uint8_t* caster, int ntri) {
  if (!env || !caster) return fail("so100_render_casters: bad arguments");
  if (env->r_ntri <= 0) return fail("so100_render_casters: no render mesh (so100_render_mesh)");
  if (ntri != env->r_ntri) {
    char msg[160];
    snprintf(msg, sizeof(msg), "so100_render_casters: ntri %d, the mesh has %d", ntri, env->r_ntri);
    return fail(msg);
  }
  DeviceGuard g(env->device);
  hipError_t e = hipSuccess;
  if (!env->r_caster) e = hipMalloc(&env->r_caster, (size_t)ntri);
  if (e == hipSuccess) e = hipMemcpy(env->r_caster, caster, (size_t)ntri, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (env->r_caster) (void)hipFree(env->r_caster);
    env->r_caster = nullptr;
    return fail_hip("so100_render_casters", e);
  }
  return 0;
}

static int so100_render_shadow_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                                    const so100_view* views, int width, int height, const so100_image_out* out,
                                    const so100_aux_out* aux, const so100_shadow* shadow, void* stream) {
  if (!shadow) return fail("so100_render_shadow: NULL shadow");
  return cams_launch("so100_render_shadow", env, qpos, mask, cams, views, width, height, out, aux, shadow, stream);
}

static int so100_render_msaa_impl(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                                  const so100_view* views, int width, int height, const so100_image_out* out,
                                  const so100_msaa* msaa, void* stream) {
  if (!msaa) return fail("so100_render_msaa: NULL msaa");
  return cams_launch("so100_render_msaa", env, qpos, mask, cams, views, width, height, out, nullptr, nullptr, stream,
                     msaa);
}

static int so100_views_sample_impl(so100_env* env, const so100_view_dr* dr, const so100_camera* cam,
                                   const uint32_t* base_rgb, const uint32_t* episode, const uint8_t* mask,
                                   so100_view* views, void* stream) {
  if (!dr) return fail("so100_views_sample: NULL dr");
  if (dr->size != sizeof(so100_view_dr))
    return size_mismatch("so100_views_sample", "so100_view_dr", dr->size, sizeof(so100_view_dr));
  if (!env) return fail("so100_views_sample: NULL env");
  if (!cam || !base_rgb || !views) return fail("so100_views_sample: NULL cam, base_rgb or views");
  auto pair_ok = [](const float* r) { return r[0] >= 0.f && r[1] >= r[0]; };     // false for NaN
  bool ok = dr->cam_pos >= 0.f && dr->cam_rot >= 0.f && dr->light_rot >= 0.f && pair_ok(dr->fovy) &&
            pair_ok(dr->ambient) && pair_ok(dr->headlight);
  for (int l = 0; l < SO100_MAX_LIGHTS; l++) ok = ok && pair_ok(dr->light[l]);
  for (int m = 0; m < SO100_NMATERIAL; m++) ok = ok && pair_ok(dr->color[m]);
  if (!ok) return fail("so100_views_sample: bad range (half-widths >= 0, 0 <= lo <= hi)");
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_views_sample(*dr, *cam, base_rgb, episode, mask, views, env->n, env->env_offset,
                                            (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_views_sample", e);
}


static int so100_ee_action_impl(so100_env* env, const so100_ee_ctrl* ctrl, const float* qpos, const float* action,
                                const uint8_t* reinit, float* q_cmd, float* joint_action, float* ee_target,
                                void* stream) {
  if (!ctrl) return fail("so100_ee_action: NULL ctrl");
  if (ctrl->size != sizeof(so100_ee_ctrl))
    return size_mismatch("so100_ee_action", "so100_ee_ctrl", ctrl->size, sizeof(so100_ee_ctrl));
  if (ctrl->iters < 1 || ctrl->iters > 8) return fail("so100_ee_action: iters outside 1..8");
  auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
  if (!positive(ctrl->pos_scale)) return fail("so100_ee_action: pos_scale must be finite and > 0");
  if (!(std::isfinite(ctrl->rot_scale) && ctrl->rot_scale >= 0.f))
    return fail("so100_ee_action: rot_scale must be finite and >= 0");
  if (!positive(ctrl->damping)) return fail("so100_ee_action: damping must be finite and > 0");
  if (!positive(ctrl->dq_max)) return fail("so100_ee_action: dq_max must be finite and > 0");
  if (!positive(ctrl->lead_max)) return fail("so100_ee_action: lead_max must be finite and > 0");
  for (int k = 0; k < 3; k++)
    if (!(std::isfinite(ctrl->ws_lo[k]) && std::isfinite(ctrl->ws_hi[k]) && ctrl->ws_lo[k] <= ctrl->ws_hi[k]))
      return fail("so100_ee_action: workspace box must be finite with ws_lo <= ws_hi");
  if (!env) return fail("so100_ee_action: NULL env");
  if (!qpos || !action || !q_cmd || !joint_action) return fail("so100_ee_action: NULL qpos, action, q_cmd or joint_action");
  if (env->ee) return fail("so100_ee_action: the model has ee = 1 (the weld variant takes a mocap pose, not an action mode)");
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_ee_action(env->d_model, *ctrl, env->n, qpos, action, reinit, q_cmd, joint_action,
                                         ee_target, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_ee_action", e);
}

static int so100_ee_jacobian_impl(so100_env* env, int n, const float* qpos, float* ee, float* jac, void* stream) {
  if (!env || !qpos || !ee || !jac || n < 0) return fail("so100_ee_jacobian: bad arguments");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_ee_jacobian(env->d_model, n, qpos, ee, jac, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_ee_jacobian", e);
}

static int so100_dr_sample_impl(so100_env* env, const so100_dr_ranges* r, const uint32_t* episode, const uint8_t* mask_a,
                                const uint8_t* mask_b, float* dr_params, float* act_params, void* stream) {
  if (!r) return fail("so100_dr_sample: NULL ranges");
  if (r->size != sizeof(so100_dr_ranges))
    return size_mismatch("so100_dr_sample", "so100_dr_ranges", r->size, sizeof(so100_dr_ranges));
  if (!env) return fail("so100_dr_sample: NULL env");
  if (!dr_params && !act_params) return fail("so100_dr_sample: NULL dr_params and act_params (nothing to draw)");
  auto positive = [](const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && p[0] > 0.f && p[0] <= p[1]; };
  if (!positive(r->mass)) return fail("so100_dr_sample: mass range must be finite with 0 < lo <= hi");
  if (!positive(r->friction)) return fail("so100_dr_sample: friction range must be finite with 0 < lo <= hi");
  if (r->delay[0] < 0 || r->delay[1] > SO100_ACT_MAX_DELAY || r->delay[0] > r->delay[1])
    return fail("so100_dr_sample: delay range must lie in 0..7 with lo <= hi");
  if (!(r->smoothing[0] > 0.f && r->smoothing[1] <= 1.f && r->smoothing[0] <= r->smoothing[1]))     // false for NaN
    return fail("so100_dr_sample: smoothing range must lie in (0, 1] with lo <= hi");
  if (!positive(r->rate)) return fail("so100_dr_sample: rate range must be finite with 0 < lo <= hi");
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_dr_sample(*r, episode, mask_a, mask_b, dr_params, act_params, env->n, env->env_offset,
                                         (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_dr_sample", e);
}

static int so100_actuate_impl(so100_env* env, const float* qpos, const float* command, const uint8_t* reinit,
                              const float* act_params, float* hist, int32_t* head, float* action, void* stream) {
  if (!env) return fail("so100_actuate: NULL env");
  if (!qpos || !command || !act_params || !hist || !head || !action)
    return fail("so100_actuate: NULL qpos, command, act_params, hist, head or action");
  if (env->ee) return fail("so100_actuate: the model has ee = 1 (the weld variant takes a mocap pose, not an action)");
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_actuate(env->d_model, env->n, qpos, command, reinit, act_params, hist, head, action,
                                       (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_actuate", e);
}

// the checks so100_norm_update and so100_norm_apply share (include/so100.h): the record first, then the env and pointers
static int norm_check(const char* fn, so100_env* env, const so100_norm* nm, int n, const void* stats, bool apply) {
  char msg[160];
  auto bad = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return fail(msg);
  };
  if (!nm) return bad("NULL norm");
  if (nm->size != sizeof(so100_norm)) return size_mismatch(fn, "so100_norm", nm->size, sizeof(so100_norm));
  if (nm->nsrc < 1 || nm->nsrc > SO100_NORM_MAX_SRC) return bad("nsrc outside 1..3");
  long long total = 0;
  for (int k = 0; k < nm->nsrc; k++) {
    const so100_norm_src& s = nm->src[k];
    if (s.dim < 1 || s.dim > SO100_NORM_MAX_DIM) return bad("dim outside 1..32");
    if (s.offset < 0) return bad("offset < 0");
    if ((long long)s.stride < (long long)s.offset + s.dim) return bad("stride smaller than offset + dim");
    if (apply && s.y_stride < s.dim) return bad("y_stride smaller than dim");
    total += s.dim;
  }
  if (total > SO100_NORM_MAX_DIM) return bad("total dim outside 1..32");
  if (!(std::isfinite(nm->epsilon) && nm->epsilon > 0.0)) return bad("epsilon must be finite and > 0");
  if (!(std::isfinite(nm->clip) && nm->clip > 0.0)) return bad("clip must be finite and > 0");
  if (nm->flags & ~SO100_NORM_INVERSE) return bad("unknown flags");
  if (n < 0) return bad("n < 0");
  if (!env) return bad("NULL env");
  for (int k = 0; k < nm->nsrc; k++) {
    if (!nm->src[k].x) return bad("NULL source");
    if (apply && !nm->src[k].y) return bad("NULL output");
  }
  if (!stats) return bad("NULL stats");
  return 0;
}

static int so100_norm_update_impl(so100_env* env, const so100_norm* nm, int n, const uint8_t* mask, double* stats,
                                  void* work, void* stream) {
  if (int rc = norm_check("so100_norm_update", env, nm, n, stats, false)) return rc;
  if (!work) return fail("so100_norm_update: NULL work");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_norm_update(*nm, n, mask, stats, (double*)work, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_norm_update", e);
}

static int so100_norm_apply_impl(so100_env* env, const so100_norm* nm, int n, const uint8_t* mask, const double* stats,
                                 void* stream) {
  if (int rc = norm_check("so100_norm_apply", env, nm, n, stats, true)) return rc;
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_norm_apply(*nm, n, mask, stats, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_norm_apply", e);
}

// the checks every so100_her_* call shares (include/so100.h): the record's numbers first, then (her_check_ptrs, after the
// call's own records) the env and the arrays
static int her_fail(const char* fn, const char* what) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", fn, what);
  return fail(msg);
}
static int her_check(const char* fn, const so100_her* h, bool sample) {
  if (!h) return her_fail(fn, "NULL her");
  if (h->size != sizeof(so100_her)) return size_mismatch(fn, "so100_her", h->size, sizeof(so100_her));
  if (h->T < 1) return her_fail(fn, "T < 1");
  if (h->n < 0) return her_fail(fn, "n < 0");
  if ((long long)h->T * h->n >= (1ll << 31)) return her_fail(fn, "T * n >= 2^31");
  if (h->action_dim < 1 || h->action_dim > SO100_HER_MAX_ACTION) return her_fail(fn, "action_dim outside 1..16");
  if (sample) {
    if (h->strategy != SO100_HER_FUTURE && h->strategy != SO100_HER_FINAL && h->strategy != SO100_HER_EPISODE)
      return her_fail(fn, "unknown strategy");
    if (h->n_sampled_goal < 0) return her_fail(fn, "n_sampled_goal < 0");
  }
  return 0;
}
static int her_check_ptrs(const char* fn, const so100_env* env, const so100_her* h) {
  if (!env) return her_fail(fn, "NULL env");
  if (!h->obs || !h->next_obs || !h->goal || !h->action || !h->reward || !h->terminated || !h->offset || !h->length ||
      !h->meta || !h->stage_obs || !h->stage_goal || !h->prefix)
    return her_fail(fn, "NULL array in so100_her");
  return 0;
}

static int so100_her_push_impl(so100_env* env, const so100_her* h, const so100_her_step* st, void* stream) {
  const char* fn = "so100_her_push";
  if (int rc = her_check(fn, h, false)) return rc;
  if (!st) return her_fail(fn, "NULL step");
  if (st->size != sizeof(so100_her_step)) return size_mismatch(fn, "so100_her_step", st->size, sizeof(so100_her_step));
  if (int rc = her_check_ptrs(fn, env, h)) return rc;
  if (!st->prev_obs || !st->prev_goal || !st->obs || !st->final_obs || !st->goal || !st->action || !st->reward ||
      !st->terminated || !st->truncated)
    return her_fail(fn, "NULL pointer in so100_her_step");
  if (h->n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_her_push(*h, *st, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_her_discard_impl(so100_env* env, const so100_her* h, const uint8_t* mask, const float* obs,
                                  const float* goal, void* stream) {
  const char* fn = "so100_her_discard";
  if (int rc = her_check(fn, h, false)) return rc;
  if (int rc = her_check_ptrs(fn, env, h)) return rc;
  if (h->n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_her_discard(*h, mask, obs, goal, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_her_scan_impl(so100_env* env, const so100_her* h, void* stream) {
  const char* fn = "so100_her_scan";
  if (int rc = her_check(fn, h, false)) return rc;
  if (int rc = her_check_ptrs(fn, env, h)) return rc;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_her_scan(*h, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_her_sample_impl(so100_env* env, const so100_her* h, int batch, uint64_t call, const so100_her_out* o,
                                 void* stream) {
  const char* fn = "so100_her_sample";
  if (int rc = her_check(fn, h, true)) return rc;
  if (batch < 0) return her_fail(fn, "batch < 0");
  if (!o) return her_fail(fn, "NULL out");
  if (o->size != sizeof(so100_her_out)) return size_mismatch(fn, "so100_her_out", o->size, sizeof(so100_her_out));
  if (int rc = her_check_ptrs(fn, env, h)) return rc;
  if (!o->observation || !o->achieved_goal || !o->desired_goal || !o->next_observation || !o->next_achieved_goal ||
      !o->next_desired_goal || !o->actions || !o->rewards || !o->dones || !o->env || !o->slot || !o->goal_slot)
    return her_fail(fn, "NULL pointer in so100_her_out");
  if (batch == 0) return 0;
  // the relabelled rows: int(her_ratio * batch), her_ratio = 1 - 1 / (n_sampled_goal + 1), in float64 as SB3 computes it
  const double ratio = 1.0 - 1.0 / ((double)h->n_sampled_goal + 1.0);
  int nrel = (int)(ratio * (double)batch);
  nrel = nrel < 0 ? 0 : (nrel > batch ? batch : nrel);
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_her_sample(env->d_model, *h, *o, batch, nrel, call, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

// the checks every so100_replay_* call shares (include/so100.h): the record's numbers first, then (replay_check_ptrs,
// after the call's own records) the env and the arrays
static int replay_check(const char* fn, const so100_replay* h) {
  if (!h) return her_fail(fn, "NULL replay");
  if (h->size != sizeof(so100_replay)) return size_mismatch(fn, "so100_replay", h->size, sizeof(so100_replay));
  if (h->T < 2) return her_fail(fn, "T < 2");
  if (h->n < 0) return her_fail(fn, "n < 0");
  if ((long long)h->T * h->n >= (1ll << 31)) return her_fail(fn, "T * n >= 2^31");
  if (h->action_dim < 1 || h->action_dim > SO100_REPLAY_MAX_ACTION) return her_fail(fn, "action_dim outside 1..16");
  bool shape_ok;
  if (h->P == 0) {
    shape_ok = h->planes == 0 && h->H == 0 && h->W == 0 && h->chan == 0;
  } else {
    shape_ok = h->P > 0 && h->planes >= 1 && h->H >= 1 && h->W >= 1 && h->chan >= 1;
    // (each factor <= P < 2^31: the product is formed stepwise in 64 bits and cut off as soon as it passes P)
    long long prod = 1;
    const int32_t f[4] = {h->planes, h->H, h->W, h->chan};
    for (int k = 0; shape_ok && k < 4; k++) {
      prod *= f[k];
      if (prod > h->P) shape_ok = false;
    }
    if (shape_ok && prod != h->P) shape_ok = false;
  }
  if (!shape_ok) return her_fail(fn, "planes, H, W, chan and P do not agree");
  if (h->pad < 0 || h->pad > SO100_REPLAY_MAX_PAD) return her_fail(fn, "pad outside 0..64");
  if (h->pad != 0 && h->P == 0) return her_fail(fn, "pad without images");
  return 0;
}
static int replay_check_ptrs(const char* fn, const so100_env* env, const so100_replay* h) {
  if (!env) return her_fail(fn, "NULL env");
  if (!h->obs || !h->next_obs || !h->action || !h->reward || !h->terminated || !h->meta || !h->prefix)
    return her_fail(fn, "NULL array in so100_replay");
  if (h->P == 0 && (h->obs_img || h->next_img)) return her_fail(fn, "image arrays in so100_replay with P == 0");
  if (h->P > 0 && (!h->obs_img || !h->next_img)) return her_fail(fn, "NULL image array in so100_replay with P > 0");
  return 0;
}

// the n-step record's numbers (include/so100.h: after the call's own records, before the env) and its array (after
// so100_replay's)
static int replay_check_nstep(const char* fn, const so100_replay* h, const so100_replay_nstep* ns) {
  if (!ns) return her_fail(fn, "NULL nstep");
  if (ns->size != sizeof(so100_replay_nstep))
    return size_mismatch(fn, "so100_replay_nstep", ns->size, sizeof(so100_replay_nstep));
  const int most = h->T - 1 < SO100_REPLAY_MAX_NSTEP ? h->T - 1 : SO100_REPLAY_MAX_NSTEP;
  if (ns->n_step < 1 || ns->n_step > most) return her_fail(fn, "n_step outside 1..min(16, T - 1)");
  if (!(ns->gamma >= 0.f && ns->gamma <= 1.f)) return her_fail(fn, "gamma outside [0, 1]");      // false for NaN
  return 0;
}
static int replay_check_ends(const char* fn, const so100_replay_nstep* ns) {
  return ns->ends ? 0 : her_fail(fn, "NULL ends in so100_replay_nstep");
}

// nstep: the _nstep entry point (ns is then checked), else ns is not looked at
static int so100_replay_push_impl(so100_env* env, const so100_replay* h, const so100_replay_nstep* ns, bool nstep,
                                  const so100_replay_step* st, void* stream) {
  const char* fn = nstep ? "so100_replay_push_nstep" : "so100_replay_push";
  if (int rc = replay_check(fn, h)) return rc;
  if (!st) return her_fail(fn, "NULL step");
  if (st->size != sizeof(so100_replay_step))
    return size_mismatch(fn, "so100_replay_step", st->size, sizeof(so100_replay_step));
  if (nstep)
    if (int rc = replay_check_nstep(fn, h, ns)) return rc;
  if (int rc = replay_check_ptrs(fn, env, h)) return rc;
  if (nstep)
    if (int rc = replay_check_ends(fn, ns)) return rc;
  if (!st->obs || !st->final_obs || !st->action || !st->reward || !st->terminated || !st->truncated)
    return her_fail(fn, "NULL pointer in so100_replay_step");
  if (h->P == 0 && (st->pixels || st->final_pixels)) return her_fail(fn, "image pointers in so100_replay_step with P == 0");
  if (h->P > 0 && (!st->pixels || !st->final_pixels))
    return her_fail(fn, "NULL image pointer in so100_replay_step with P > 0");
  if (h->n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = nstep ? so100::launch_replay_push_nstep(*h, *ns, *st, (hipStream_t)stream)
                       : so100::launch_replay_push(*h, *st, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_replay_stage_impl(so100_env* env, const so100_replay* h, const so100_replay_nstep* ns, bool nstep,
                                   const uint8_t* mask, const float* obs, const uint8_t* pixels, void* stream) {
  const char* fn = nstep ? "so100_replay_stage_nstep" : "so100_replay_stage";
  if (int rc = replay_check(fn, h)) return rc;
  if (nstep)
    if (int rc = replay_check_nstep(fn, h, ns)) return rc;
  if (int rc = replay_check_ptrs(fn, env, h)) return rc;
  if (nstep)
    if (int rc = replay_check_ends(fn, ns)) return rc;
  if (!obs) return her_fail(fn, "NULL obs");
  if (h->P == 0 && pixels) return her_fail(fn, "pixels with P == 0");
  if (h->P > 0 && !pixels) return her_fail(fn, "NULL pixels with P > 0");
  if (h->n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = nstep ? so100::launch_replay_stage_nstep(*h, *ns, mask, obs, pixels, (hipStream_t)stream)
                       : so100::launch_replay_stage(*h, mask, obs, pixels, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_replay_scan_impl(so100_env* env, const so100_replay* h, void* stream) {
  const char* fn = "so100_replay_scan";
  if (int rc = replay_check(fn, h)) return rc;
  if (int rc = replay_check_ptrs(fn, env, h)) return rc;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_replay_scan(*h, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_replay_sample_impl(so100_env* env, const so100_replay* h, const so100_replay_nstep* ns, bool nstep,
                                    int batch, uint64_t call, const so100_replay_out* o,
                                    const so100_replay_nstep_out* no, void* stream) {
  const char* fn = nstep ? "so100_replay_sample_nstep" : "so100_replay_sample";
  if (int rc = replay_check(fn, h)) return rc;
  if (batch < 0) return her_fail(fn, "batch < 0");
  if (!o) return her_fail(fn, "NULL out");
  if (o->size != sizeof(so100_replay_out)) return size_mismatch(fn, "so100_replay_out", o->size, sizeof(so100_replay_out));
  if (nstep) {
    if (int rc = replay_check_nstep(fn, h, ns)) return rc;
    if (!no) return her_fail(fn, "NULL nout");
    if (no->size != sizeof(so100_replay_nstep_out))
      return size_mismatch(fn, "so100_replay_nstep_out", no->size, sizeof(so100_replay_nstep_out));
  }
  if (int rc = replay_check_ptrs(fn, env, h)) return rc;
  if (nstep)
    if (int rc = replay_check_ends(fn, ns)) return rc;
  if (!o->obs || !o->next_obs || !o->actions || !o->rewards || !o->dones || !o->env || !o->slot || !o->shift)
    return her_fail(fn, "NULL pointer in so100_replay_out");
  if (h->P == 0 && (o->pixels || o->next_pixels)) return her_fail(fn, "image pointers in so100_replay_out with P == 0");
  if (h->P > 0 && (!o->pixels || !o->next_pixels))
    return her_fail(fn, "NULL image pointer in so100_replay_out with P > 0");
  if (nstep && (!no->discounts || !no->nsteps || !no->last_slot))
    return her_fail(fn, "NULL pointer in so100_replay_nstep_out");
  if (batch == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = nstep ? so100::launch_replay_sample_nstep(*h, *o, *ns, *no, batch, call, (hipStream_t)stream)
                       : so100::launch_replay_sample(*h, *o, batch, call, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

// the prioritised calls (include/so100.h, the numbered refusals above so100_replay_push_per).  replay_check_per: 2-5;
// replay_check_per_ptrs: the arrays of 9 up to max_prio
static int replay_check_per(const char* fn, const so100_replay* h, const so100_replay_per* pr,
                            const so100_replay_nstep* ns) {
  if (!pr) return her_fail(fn, "NULL per");
  if (pr->size != sizeof(so100_replay_per)) return size_mismatch(fn, "so100_replay_per", pr->size, sizeof(so100_replay_per));
  if (!(pr->alpha >= 0.f && pr->alpha <= 1.f)) return her_fail(fn, "alpha outside [0, 1]");      // false for NaN
  if (!(pr->beta >= 0.f && pr->beta <= 1.f)) return her_fail(fn, "beta outside [0, 1]");
  if (!(pr->eps > 0.f && std::isfinite(pr->eps))) return her_fail(fn, "eps not finite or <= 0");
  if (ns)
    if (int rc = replay_check_nstep(fn, h, ns)) return rc;
  return 0;
}
static int replay_check_per_ptrs(const char* fn, const so100_env* env, const so100_replay* h, const so100_replay_per* pr,
                                 const so100_replay_nstep* ns) {
  if (int rc = replay_check_ptrs(fn, env, h)) return rc;
  if (ns)
    if (int rc = replay_check_ends(fn, ns)) return rc;
  if (!pr->prio || !pr->sum || !pr->max_prio) return her_fail(fn, "NULL array in so100_replay_per");
  return 0;
}

static int so100_replay_push_per_impl(so100_env* env, const so100_replay* h, const so100_replay_per* pr,
                                      const so100_replay_nstep* ns, const so100_replay_step* st, void* stream) {
  const char* fn = "so100_replay_push_per";
  if (int rc = replay_check(fn, h)) return rc;
  if (int rc = replay_check_per(fn, h, pr, ns)) return rc;
  if (!st) return her_fail(fn, "NULL step");
  if (st->size != sizeof(so100_replay_step))
    return size_mismatch(fn, "so100_replay_step", st->size, sizeof(so100_replay_step));
  if (int rc = replay_check_per_ptrs(fn, env, h, pr, ns)) return rc;
  if (!st->obs || !st->final_obs || !st->action || !st->reward || !st->terminated || !st->truncated)
    return her_fail(fn, "NULL pointer in so100_replay_step");
  if (h->P == 0 && (st->pixels || st->final_pixels)) return her_fail(fn, "image pointers in so100_replay_step with P == 0");
  if (h->P > 0 && (!st->pixels || !st->final_pixels))
    return her_fail(fn, "NULL image pointer in so100_replay_step with P > 0");
  if (h->n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_replay_push_per(*h, *pr, ns, *st, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_replay_per_scan_impl(so100_env* env, const so100_replay* h, const so100_replay_per* pr, void* stream) {
  const char* fn = "so100_replay_per_scan";
  if (int rc = replay_check(fn, h)) return rc;
  if (int rc = replay_check_per(fn, h, pr, nullptr)) return rc;
  if (int rc = replay_check_per_ptrs(fn, env, h, pr, nullptr)) return rc;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_replay_per_scan(*h, *pr, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_replay_sample_per_impl(so100_env* env, const so100_replay* h, const so100_replay_per* pr,
                                        const so100_replay_nstep* ns, int batch, uint64_t call,
                                        const so100_replay_out* o, const so100_replay_nstep_out* no,
                                        const so100_replay_per_out* po, void* stream) {
  const char* fn = "so100_replay_sample_per";
  if (int rc = replay_check(fn, h)) return rc;
  if (int rc = replay_check_per(fn, h, pr, ns)) return rc;
  if (no && !ns) return her_fail(fn, "nout without nstep");
  if (ns && !no) return her_fail(fn, "NULL nout with nstep");
  if (no && no->size != sizeof(so100_replay_nstep_out))
    return size_mismatch(fn, "so100_replay_nstep_out", no->size, sizeof(so100_replay_nstep_out));
  if (!po) return her_fail(fn, "NULL pout");
  if (po->size != sizeof(so100_replay_per_out))
    return size_mismatch(fn, "so100_replay_per_out", po->size, sizeof(so100_replay_per_out));
  if (!o) return her_fail(fn, "NULL out");
  if (o->size != sizeof(so100_replay_out)) return size_mismatch(fn, "so100_replay_out", o->size, sizeof(so100_replay_out));
  if (batch < 0) return her_fail(fn, "batch < 0");
  if (int rc = replay_check_per_ptrs(fn, env, h, pr, ns)) return rc;
  if (!o->obs || !o->next_obs || !o->actions || !o->rewards || !o->dones || !o->env || !o->slot || !o->shift)
    return her_fail(fn, "NULL pointer in so100_replay_out");
  if (h->P == 0 && (o->pixels || o->next_pixels)) return her_fail(fn, "image pointers in so100_replay_out with P == 0");
  if (h->P > 0 && (!o->pixels || !o->next_pixels))
    return her_fail(fn, "NULL image pointer in so100_replay_out with P > 0");
  if (ns && (!no->discounts || !no->nsteps || !no->last_slot))
    return her_fail(fn, "NULL pointer in so100_replay_nstep_out");
  if (!po->probs || !po->weights) return her_fail(fn, "NULL pointer in so100_replay_per_out");
  if (batch == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_replay_sample_per(*h, *o, *pr, *po, ns, no, batch, call, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_replay_per_update_impl(so100_env* env, const so100_replay* h, const so100_replay_per* pr, int batch,
                                        const int32_t* env_idx, const int32_t* slot_idx, const float* td_abs,
                                        void* stream) {
  const char* fn = "so100_replay_per_update";
  if (int rc = replay_check(fn, h)) return rc;
  if (int rc = replay_check_per(fn, h, pr, nullptr)) return rc;
  if (batch < 0) return her_fail(fn, "batch < 0");
  if (int rc = replay_check_per_ptrs(fn, env, h, pr, nullptr)) return rc;
  if (!env_idx || !slot_idx || !td_abs) return her_fail(fn, "NULL env_idx, slot_idx or td_abs");
  if (batch == 0 || h->n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_replay_per_update(*h, *pr, batch, env_idx, slot_idx, td_abs, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip(fn, e);
}

static int so100_norm_return_impl(so100_env* env, const so100_norm_ret* a, int n, const float* reward,
                                  const uint8_t* terminated, const uint8_t* truncated, double* ret, double* stats,
                                  void* work, float* reward_norm, void* stream) {
  if (!a) return fail("so100_norm_return: NULL args");
  if (a->size != sizeof(so100_norm_ret))
    return size_mismatch("so100_norm_return", "so100_norm_ret", a->size, sizeof(so100_norm_ret));
  if (!(a->gamma > 0.0 && a->gamma <= 1.0)) return fail("so100_norm_return: gamma outside (0, 1]");      // false for NaN
  if (!(std::isfinite(a->epsilon) && a->epsilon > 0.0)) return fail("so100_norm_return: epsilon must be finite and > 0");
  if (!(std::isfinite(a->clip) && a->clip > 0.0)) return fail("so100_norm_return: clip must be finite and > 0");
  if (a->flags & ~(SO100_NORM_RET_UPDATE | SO100_NORM_RET_NORMALIZE)) return fail("so100_norm_return: unknown flags");
  if (n < 0) return fail("so100_norm_return: n < 0");
  if (!env) return fail("so100_norm_return: NULL env");
  if (!reward || !ret || !stats) return fail("so100_norm_return: NULL reward, ret or stats");
  if ((a->flags & SO100_NORM_RET_UPDATE) && !work) return fail("so100_norm_return: NULL work");
  if ((a->flags & SO100_NORM_RET_NORMALIZE) && !reward_norm) return fail("so100_norm_return: NULL reward_norm");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_norm_return(*a, n, reward, terminated, truncated, ret, stats, (double*)work, reward_norm,
                                           (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail_hip("so100_norm_return", e);
}

// the step kernels' hull support for n directions of one hull (device buffers; the null stream, waited for)
static int so100_hull_support_probe_impl(so100_env* env, int hull, const float* dirs, int n, int use_cells, float* out) {
  if (!env || !dirs || !out || n < 0) return fail("so100_hull_support_probe: bad arguments");
  if (hull < 0 || hull >= SO100_NHULL_ALL) return fail("so100_hull_support_probe: hull index out of range");
  if (use_cells < 0 || use_cells > 2) return fail("so100_hull_support_probe: use_cells must be 0, 1 or 2");
  if (n == 0) return 0;
  DeviceGuard g(env->device);
  hipError_t e = so100::launch_hull_support_probe(env->d_model, hull, dirs, n, use_cells, out, nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return e == hipSuccess ? 0 : fail_hip("so100_hull_support_probe", e);
}


extern "C" {
int so100_hull_blocks(const so100_model* model, float* blk, int cap) {
  try {
    return so100_hull_blocks_impl(model, blk, cap);
  } catch (...) {
    return caught("so100_hull_blocks");
  }
}

int so100_hull_support_probe(so100_env* env, int hull, const float* dirs, int n, int use_cells, float* out) {
  try {
    return so100_hull_support_probe_impl(env, hull, dirs, n, use_cells, out);
  } catch (...) {
    return caught("so100_hull_support_probe");
  }
}


int so100_dr_ranges_bytes(void) { return (int)sizeof(so100_dr_ranges); }

int so100_dr_sample(so100_env* env, const so100_dr_ranges* ranges, const uint32_t* episode, const uint8_t* mask_a,
                    const uint8_t* mask_b, float* dr_params, float* act_params, void* stream) {
  try {
    return so100_dr_sample_impl(env, ranges, episode, mask_a, mask_b, dr_params, act_params, stream);
  } catch (...) {
    return caught("so100_dr_sample");
  }
}

int so100_actuate(so100_env* env, const float* qpos, const float* command, const uint8_t* reinit,
                  const float* act_params, float* hist, int32_t* head, float* action, void* stream) {
  try {
    return so100_actuate_impl(env, qpos, command, reinit, act_params, hist, head, action, stream);
  } catch (...) {
    return caught("so100_actuate");
  }
}

int so100_her_bytes(void) { return (int)sizeof(so100_her); }
int so100_her_step_bytes(void) { return (int)sizeof(so100_her_step); }
int so100_her_out_bytes(void) { return (int)sizeof(so100_her_out); }

int so100_her_limits(int* scan_group, int* scan_tile) {
  if (!scan_group || !scan_tile) return fail("so100_her_limits: NULL argument");
  *scan_group = so100::her_scan_group();
  *scan_tile = so100::her_scan_tile();
  return 0;
}

int64_t so100_her_storage_bytes(int n, int T, int action_dim) {
  if (n < 0 || T < 1 || (long long)T * n >= (1ll << 31) || action_dim < 1 || action_dim > SO100_HER_MAX_ACTION) {
    fail("so100_her_storage_bytes: n < 0, T < 1, T * n >= 2^31 or action_dim outside 1..16");
    return -1;
  }
  const int64_t slots = (int64_t)T * n;
  return slots * (4 * (SO100_NOBS + SO100_NOBS + 3 + action_dim + 1 + 2) + 1) + 4 * (3 * (int64_t)n + 18 * (int64_t)n + n + 1);
}

int so100_her_push(so100_env* env, const so100_her* her, const so100_her_step* step, void* stream) {
  try {
    return so100_her_push_impl(env, her, step, stream);
  } catch (...) {
    return caught("so100_her_push");
  }
}

int so100_her_discard(so100_env* env, const so100_her* her, const uint8_t* mask, const float* obs, const float* goal,
                      void* stream) {
  try {
    return so100_her_discard_impl(env, her, mask, obs, goal, stream);
  } catch (...) {
    return caught("so100_her_discard");
  }
}

int so100_her_scan(so100_env* env, const so100_her* her, void* stream) {
  try {
    return so100_her_scan_impl(env, her, stream);
  } catch (...) {
    return caught("so100_her_scan");
  }
}

int so100_her_sample(so100_env* env, const so100_her* her, int batch, uint64_t call, const so100_her_out* out,
                     void* stream) {
  try {
    return so100_her_sample_impl(env, her, batch, call, out, stream);
  } catch (...) {
    return caught("so100_her_sample");
  }
}

int so100_replay_bytes(void) { return (int)sizeof(so100_replay); }
int so100_replay_step_bytes(void) { return (int)sizeof(so100_replay_step); }
int so100_replay_out_bytes(void) { return (int)sizeof(so100_replay_out); }

int64_t so100_replay_storage_bytes(int n, int T, int action_dim, int P) {
  if (n < 0 || T < 2 || (long long)T * n >= (1ll << 31) || action_dim < 1 || action_dim > SO100_REPLAY_MAX_ACTION ||
      P < 0) {
    fail("so100_replay_storage_bytes: n < 0, T < 2, T * n >= 2^31, action_dim outside 1..16 or P < 0");
    return -1;
  }
  const int64_t slots = (int64_t)T * n;
  return slots * (4 * (SO100_NOBS + SO100_NOBS + action_dim + 1) + 1 + 2 * (int64_t)P) + 4 * (2 * (int64_t)n + n + 1);
}

int so100_replay_push(so100_env* env, const so100_replay* replay, const so100_replay_step* step, void* stream) {
  try {
    return so100_replay_push_impl(env, replay, nullptr, false, step, stream);
  } catch (...) {
    return caught("so100_replay_push");
  }
}

int so100_replay_stage(so100_env* env, const so100_replay* replay, const uint8_t* mask, const float* obs,
                       const uint8_t* pixels, void* stream) {
  try {
    return so100_replay_stage_impl(env, replay, nullptr, false, mask, obs, pixels, stream);
  } catch (...) {
    return caught("so100_replay_stage");
  }
}

int so100_replay_scan(so100_env* env, const so100_replay* replay, void* stream) {
  try {
    return so100_replay_scan_impl(env, replay, stream);
  } catch (...) {
    return caught("so100_replay_scan");
  }
}

int so100_replay_sample(so100_env* env, const so100_replay* replay, int batch, uint64_t call, const so100_replay_out* out,
                        void* stream) {
  try {
    return so100_replay_sample_impl(env, replay, nullptr, false, batch, call, out, nullptr, stream);
  } catch (...) {
    return caught("so100_replay_sample");
  }
}

int so100_replay_nstep_bytes(void) { return (int)sizeof(so100_replay_nstep); }
int so100_replay_nstep_out_bytes(void) { return (int)sizeof(so100_replay_nstep_out); }

int64_t so100_replay_nstep_storage_bytes(int n, int T) {
  if (n < 0 || T < 2 || (long long)T * n >= (1ll << 31)) {
    fail("so100_replay_nstep_storage_bytes: n < 0, T < 2 or T * n >= 2^31");
    return -1;
  }
  return (int64_t)T * n;
}

int so100_replay_push_nstep(so100_env* env, const so100_replay* replay, const so100_replay_nstep* nstep,
                            const so100_replay_step* step, void* stream) {
  try {
    return so100_replay_push_impl(env, replay, nstep, true, step, stream);
  } catch (...) {
    return caught("so100_replay_push_nstep");
  }
}

int so100_replay_stage_nstep(so100_env* env, const so100_replay* replay, const so100_replay_nstep* nstep,
                             const uint8_t* mask, const float* obs, const uint8_t* pixels, void* stream) {
  try {
    return so100_replay_stage_impl(env, replay, nstep, true, mask, obs, pixels, stream);
  } catch (...) {
    return caught("so100_replay_stage_nstep");
  }
}

int so100_replay_per_bytes(void) { return (int)sizeof(so100_replay_per); }
int so100_replay_per_out_bytes(void) { return (int)sizeof(so100_replay_per_out); }

int64_t so100_replay_per_storage_bytes(int n, int T) {
  if (n < 0 || T < 2 || (long long)T * n >= (1ll << 31)) {
    fail("so100_replay_per_storage_bytes: n < 0, T < 2 or T * n >= 2^31");
    return -1;
  }
  return 4ll * T * n + 8ll * ((long long)n + 1) + 8;
}

int so100_replay_push_per(so100_env* env, const so100_replay* replay, const so100_replay_per* per,
                          const so100_replay_nstep* nstep, const so100_replay_step* step, void* stream) {
  try {
    return so100_replay_push_per_impl(env, replay, per, nstep, step, stream);
  } catch (...) {
    return caught("so100_replay_push_per");
  }
}

int so100_replay_per_scan(so100_env* env, const so100_replay* replay, const so100_replay_per* per, void* stream) {
  try {
    return so100_replay_per_scan_impl(env, replay, per, stream);
  } catch (...) {
    return caught("so100_replay_per_scan");
  }
}

int so100_replay_sample_per(so100_env* env, const so100_replay* replay, const so100_replay_per* per,
                            const so100_replay_nstep* nstep, int batch, uint64_t call, const so100_replay_out* out,
                            const so100_replay_nstep_out* nout, const so100_replay_per_out* pout, void* stream) {
  try {
    return so100_replay_sample_per_impl(env, replay, per, nstep, batch, call, out, nout, pout, stream);
  } catch (...) {
    return caught("so100_replay_sample_per");
  }
}

int so100_replay_per_update(so100_env* env, const so100_replay* replay, const so100_replay_per* per, int batch,
                            const int32_t* env_idx, const int32_t* slot_idx, const float* td_abs, void* stream) {
  try {
    return so100_replay_per_update_impl(env, replay, per, batch, env_idx, slot_idx, td_abs, stream);
  } catch (...) {
    return caught("so100_replay_per_update");
  }
}

int so100_replay_sample_nstep(so100_env* env, const so100_replay* replay, const so100_replay_nstep* nstep, int batch,
                              uint64_t call, const so100_replay_out* out, const so100_replay_nstep_out* nout,
                              void* stream) {
  try {
    return so100_replay_sample_impl(env, replay, nstep, true, batch, call, out, nout, stream);
  } catch (...) {
    return caught("so100_replay_sample_nstep");
  }
}

int so100_norm_bytes(void) { return (int)sizeof(so100_norm); }
int so100_norm_ret_bytes(void) { return (int)sizeof(so100_norm_ret); }

int so100_norm_limits(int* rows_per_group, int* max_groups) {
  if (!rows_per_group || !max_groups) return fail("so100_norm_limits: NULL argument");
  *rows_per_group = so100::norm_rows_per_group();
  *max_groups = so100::norm_max_groups();
  return 0;
}

int so100_norm_work_bytes(int n) {
  if (n < 0) {
    fail("so100_norm_work_bytes: n < 0");
    return -1;
  }
  return so100::norm_groups(n) * 3 * SO100_NORM_MAX_DIM * (int)sizeof(double);
}

int so100_norm_update(so100_env* env, const so100_norm* norm, int n, const uint8_t* mask, double* stats, void* work,
                      void* stream) {
  try {
    return so100_norm_update_impl(env, norm, n, mask, stats, work, stream);
  } catch (...) {
    return caught("so100_norm_update");
  }
}

int so100_norm_apply(so100_env* env, const so100_norm* norm, int n, const uint8_t* mask, const double* stats,
                     void* stream) {
  try {
    return so100_norm_apply_impl(env, norm, n, mask, stats, stream);
  } catch (...) {
    return caught("so100_norm_apply");
  }
}

int so100_norm_return(so100_env* env, const so100_norm_ret* args, int n, const float* reward, const uint8_t* terminated,
                      const uint8_t* truncated, double* ret, double* stats, void* work, float* reward_norm,
                      void* stream) {
  try {
    return so100_norm_return_impl(env, args, n, reward, terminated, truncated, ret, stats, work, reward_norm, stream);
  } catch (...) {
    return caught("so100_norm_return");
  }
}

int so100_ee_ctrl_bytes(void) { return (int)sizeof(so100_ee_ctrl); }

int so100_ee_action(so100_env* env, const so100_ee_ctrl* ctrl, const float* qpos, const float* action,
                    const uint8_t* reinit, float* q_cmd, float* joint_action, float* ee_target, void* stream) {
  try {
    return so100_ee_action_impl(env, ctrl, qpos, action, reinit, q_cmd, joint_action, ee_target, stream);
  } catch (...) {
    return caught("so100_ee_action");
  }
}

int so100_ee_jacobian(so100_env* env, int n, const float* qpos, float* ee, float* jac, void* stream) {
  try {
    return so100_ee_jacobian_impl(env, n, qpos, ee, jac, stream);
  } catch (...) {
    return caught("so100_ee_jacobian");
  }
}

int so100_view_bytes(void) { return (int)sizeof(so100_view); }

int so100_render_materials(so100_env* env, const uint8_t* material, int ntri) {
  try {
    return so100_render_materials_impl(env, material, ntri);
  } catch (...) {
    return caught("so100_render_materials");
  }
}

int so100_render_views(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                       const so100_view* views, int width, int height, const so100_image_out* out, void* stream) {
  try {
    return so100_render_views_impl(env, qpos, mask, cam, views, width, height, out, stream);
  } catch (...) {
    return caught("so100_render_views");
  }
}

int so100_aux_out_bytes(void) { return (int)sizeof(so100_aux_out); }

int so100_render_labels(so100_env* env, const uint8_t* label, int ntri) {
  try {
    return so100_render_labels_impl(env, label, ntri);
  } catch (...) {
    return caught("so100_render_labels");
  }
}

int so100_render_aux(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                     const so100_view* views, int width, int height, const so100_image_out* out,
                     const so100_aux_out* aux, void* stream) {
  try {
    return so100_render_aux_impl(env, qpos, mask, cam, views, width, height, out, aux, stream);
  } catch (...) {
    return caught("so100_render_aux");
  }
}

int so100_cams_bytes(void) { return (int)sizeof(so100_cams); }

int so100_render_cams(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                      const so100_view* views, int width, int height, const so100_image_out* out,
                      const so100_aux_out* aux, void* stream) {
  try {
    return so100_render_cams_impl(env, qpos, mask, cams, views, width, height, out, aux, stream);
  } catch (...) {
    return caught("so100_render_cams");
  }
}

int so100_shadow_bytes(void) { return (int)sizeof(so100_shadow); }

int so100_render_casters(so100_env* env, const uint8_t* caster, int ntri) {
  try {
    return so100_render_casters_impl(env, caster, ntri);
  } catch (...) {
    return caught("so100_render_casters");
  }
}

int so100_render_shadow(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                        const so100_view* views, int width, int height, const so100_image_out* out,
                        const so100_aux_out* aux, const so100_shadow* shadow, void* stream) {
  try {
    return so100_render_shadow_impl(env, qpos, mask, cams, views, width, height, out, aux, shadow, stream);
  } catch (...) {
    return caught("so100_render_shadow");
  }
}

int so100_msaa_bytes(void) { return (int)sizeof(so100_msaa); }

int so100_render_msaa(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                      const so100_view* views, int width, int height, const so100_image_out* out,
                      const so100_msaa* msaa, void* stream) {
  try {
    return so100_render_msaa_impl(env, qpos, mask, cams, views, width, height, out, msaa, stream);
  } catch (...) {
    return caught("so100_render_msaa");
  }
}

int so100_views_sample(so100_env* env, const so100_view_dr* dr, const so100_camera* cam, const uint32_t* base_rgb,
                       const uint32_t* episode, const uint8_t* mask, so100_view* views, void* stream) {
  try {
    return so100_views_sample_impl(env, dr, cam, base_rgb, episode, mask, views, stream);
  } catch (...) {
    return caught("so100_views_sample");
  }
}

int so100_abi_version(void) {
  try {
    return so100_abi_version_impl();
  } catch (...) {
    return caught("so100_abi_version");
  }
}

const char* so100_last_error(void) { return so100_last_error_impl(); }

#ifndef SO100_SRC_HASH
#define SO100_SRC_HASH "unknown"
#endif
// the Makefile's content hash of the sources this library was built from (ABI 16)
const char* so100_source_hash(void) { return SO100_SRC_HASH; }

int so100_hull_cells(const so100_model* model, uint32_t* cells, float* cand, int cap) {
  try {
    return so100_hull_cells_impl(model, cells, cand, cap);
  } catch (...) {
    return caught("so100_hull_cells");
  }
}

int so100_struct_sizes(int* model_bytes, int* buffers_bytes) {
  try {
    return so100_struct_sizes_impl(model_bytes, buffers_bytes);
  } catch (...) {
    return caught("so100_struct_sizes");
  }
}

so100_env* so100_create(const so100_model* model, int n_envs, int device) {
  try {
    return so100_create_impl(model, n_envs, device);
  } catch (...) {
    caught("so100_create");
    return nullptr;
  }
}

int so100_destroy(so100_env* env) {
  try {
    return so100_destroy_impl(env);
  } catch (...) {
    return caught("so100_destroy");
  }
}

int so100_num_envs(const so100_env* env) {
  try {
    return so100_num_envs_impl(env);
  } catch (...) {
    return caught("so100_num_envs");
  }
}

int so100_configure(so100_env* env, int task, int max_episode_steps, uint64_t base_seed, int env_offset) {
  try {
    return so100_configure_impl(env, task, max_episode_steps, base_seed, env_offset);
  } catch (...) {
    return caught("so100_configure");
  }
}

int so100_reset(so100_env* env, const so100_buffers* b, const uint8_t* mask, const uint32_t* seeds, void* stream) {
  try {
    return so100_reset_impl(env, b, mask, seeds, stream);
  } catch (...) {
    return caught("so100_reset");
  }
}

int so100_step(so100_env* env, const so100_buffers* b, int flags, void* stream) {
  try {
    return so100_step_impl(env, b, flags, stream);
  } catch (...) {
    return caught("so100_step");
  }
}

int so100_profile_enable(so100_env* env, int max_steps) {
  try {
    return so100_profile_enable_impl(env, max_steps);
  } catch (...) {
    return caught("so100_profile_enable");
  }
}

int so100_profile_read(so100_env* env, double* solver_ms, int* solver_launches, double* stage_ms, int* stage_launches) {
  try {
    return so100_profile_read_impl(env, solver_ms, solver_launches, stage_ms, stage_launches);
  } catch (...) {
    return caught("so100_profile_read");
  }
}

int so100_set_step_mode(so100_env* env, int fused) {
  try {
    return so100_set_step_mode_impl(env, fused);
  } catch (...) {
    return caught("so100_set_step_mode");
  }
}

int so100_step_mode(const so100_env* env) {
  try {
    return so100_step_mode_impl(env);
  } catch (...) {
    return caught("so100_step_mode");
  }
}

int so100_set_fused_build(so100_env* env, int waves) {
  try {
    return so100_set_fused_build_impl(env, waves);
  } catch (...) {
    return caught("so100_set_fused_build");
  }
}

int so100_fused_build(const so100_env* env, int debug) {
  try {
    return so100_fused_build_impl(env, debug);
  } catch (...) {
    return caught("so100_fused_build");
  }
}

int so100_set_env_packing(so100_env* env, int mode) {
  try {
    return so100_set_env_packing_impl(env, mode);
  } catch (...) {
    return caught("so100_set_env_packing");
  }
}

int so100_env_packing(const so100_env* env) {
  try {
    if (!env) return fail("so100_env_packing: env is NULL");
    DeviceGuard g(env->device);
    return env_packing(env);
  } catch (...) {
    return caught("so100_env_packing");
  }
}

int so100_env_order(so100_env* env, int32_t* out, int cap) {
  try {
    return so100_env_order_impl(env, out, cap);
  } catch (...) {
    return caught("so100_env_order");
  }
}

int so100_wave_cost(so100_env* env, uint32_t* out, int cap) {
  try {
    return so100_wave_cost_impl(env, out, cap);
  } catch (...) {
    return caught("so100_wave_cost");
  }
}

int so100_chunk_info(const so100_env* env, int* nchunks, int* profiled_envs) {
  try {
    return so100_chunk_info_impl(env, nchunks, profiled_envs);
  } catch (...) {
    return caught("so100_chunk_info");
  }
}

int so100_contact_count(so100_env* env, uint64_t* accum, void* stream) {
  try {
    return so100_contact_count_impl(env, accum, stream);
  } catch (...) {
    return caught("so100_contact_count");
  }
}

int so100_pool_stats(so100_env* env, uint64_t* out, int reset) {
  try {
    return so100_pool_stats_impl(env, out, reset);
  } catch (...) {
    return caught("so100_pool_stats");
  }
}

int so100_env_cost(so100_env* env, uint32_t* out, int cap) {
  try {
    return so100_env_cost_impl(env, out, cap);
  } catch (...) {
    return caught("so100_env_cost");
  }
}

int so100_contact_counts(so100_env* env, int32_t* out, void* stream) {
  try {
    return so100_contact_counts_impl(env, out, stream);
  } catch (...) {
    return caught("so100_contact_counts");
  }
}

int so100_goal_reward(so100_env* env, int n, const float* a, const float* d, float* out, void* stream) {
  try {
    return so100_goal_reward_impl(env, n, a, d, out, stream);
  } catch (...) {
    return caught("so100_goal_reward");
  }
}

int so100_eval_reward(so100_env* env, int task, int n, const float* cube, const float* ee, const uint32_t* bits,
                      float* out, void* stream) {
  try {
    return so100_eval_reward_impl(env, task, n, cube, ee, bits, out, stream);
  } catch (...) {
    return caught("so100_eval_reward");
  }
}

int so100_spawn_pose(so100_env* env, int n, const uint32_t* seeds, double* pose, void* stream) {
  try {
    return so100_spawn_pose_impl(env, n, seeds, pose, stream);
  } catch (...) {
    return caught("so100_spawn_pose");
  }
}

int so100_unnormalize(so100_env* env, int n, const float* action, float* ctrl, void* stream) {
  try {
    return so100_unnormalize_impl(env, n, action, ctrl, stream);
  } catch (...) {
    return caught("so100_unnormalize");
  }
}

int so100_render_mesh(so100_env* env, const float* tri, const int* body, const float* rgb, int ntri) {
  try {
    return so100_render_mesh_impl(env, tri, body, rgb, ntri);
  } catch (...) {
    return caught("so100_render_mesh");
  }
}

int so100_render(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam, int width,
                 int height, uint8_t* out, void* stream) {
  try {
    return so100_render_impl(env, qpos, mask, cam, width, height, out, stream);
  } catch (...) {
    return caught("so100_render");
  }
}

int so100_render_to(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam, int width,
                    int height, const so100_image_out* out, void* stream) {
  try {
    return so100_render_to_impl(env, qpos, mask, cam, width, height, out, stream);
  } catch (...) {
    return caught("so100_render_to");
  }
}

}  // extern "C"
