/* so100.h — C-ABI of the MI355X-native batched SO-ARM100 simulator (libso100_hip.so).
 *
 * This boundary replaces, for N envs at once, what the reference reaches through dm_control:
 *   gym_so100/env.py:98-127   mujoco.Physics.from_xml_path + control.Environment   -> so100_create
 *   gym_so100/env.py:148-170  SO100Env.reset (BOX_POSE, reset_context, mj_forward)  -> so100_reset
 *   gym_so100/env.py:172-182  SO100Env.step -> control.Environment.step:
 *        single_arm.py:33-38  before_step (unnormalize, fp32 ctrl)
 *        env.py:174           Physics.step(10)  (mj_step2; mj_step x9; mj_step1)
 *        single_arm.py:322-380/149-215/246-285 get_reward,  :82-114 get_observation
 *        env.py:130-146,175   obs packing, terminated = reward == 4                 -> so100_step
 *   gym_so100/env.py:341-353  SO100GoalEnv.compute_reward (batched)                 -> so100_goal_reward
 *
 * Conventions: plain pointers and sizes only; every array is DEVICE memory allocated by the caller
 * (PyTorch-ROCm tensors in the Python layer); row-major [n_envs, dim].  Calls enqueue on `stream`
 * (a hipStream_t, NULL = default stream) and never synchronise the host.  Status: 0 = ok, < 0 = error
 * (message in so100_last_error()): -1 bad arguments / model, -2 a HIP error, -3 a C++ exception caught at the
 * boundary (e.g. host memory exhausted).  No C++ exceptions cross this boundary.
 */
#ifndef SO100_H
#define SO100_H
#include <stdint.h>
#include "so100_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SO100_ABI_VERSION 25  /* (added without a new version, no existing entry point or struct changes: so100_hull_blocks / so100_hull_support_probe, the support cells' self-describing block table behind the device model and the step kernels' hull support on its own; a caller finds them by symbol);  25: so100_ee_ctrl / so100_ee_action / so100_ee_jacobian / so100_ee_ctrl_bytes (Cartesian end-effector action mode: a batched damped least-squares prologue in front of so100_step);  24: so100_msaa / so100_render_msaa / so100_msaa_bytes (multisample anti-aliasing, resolved in LDS inside the render launch);  23: so100_shadow / so100_render_shadow / so100_render_casters / so100_shadow_bytes (cast shadows from one light, a shadow map per block);  22: so100_cams / so100_render_cams / so100_cams_bytes (several cameras in one render launch, cameras mounted on a body);  21: so100_render_aux / so100_aux_out / so100_render_labels / so100_aux_out_bytes (depth and segmentation images from the render launch);  20: so100_view / so100_render_views / so100_render_materials / so100_views_sample / so100_view_bytes (camera, lights and colours per env);  19: so100_render_to / so100_image_out (one render launch, several sinks: hwc, chw, flat float32);  18: env packing of the fused step (so100_set_env_packing, so100_env_packing, so100_env_order, so100_env_cost, so100_wave_cost);  17: so100_pool_stats (the fused step's contact-record pool, sized never to run out);  16: so100_source_hash;  15: the EE variant's mocap marker box collides (SO100_NGEOM 16, SO100_NPAIR 209, SO100_NCON_MAX 643, debug stride 3,922);  14: no per-env contact cap (SO100_NCON_MAX: every pair at its collider's maximum), debug stride 3,436 (SO100_DBG_OVF), ncon_dropped always 0, status -3 for a caught C++ exception;  13: so100_buffers.ep_return / ep_final / ep_accum (device-side episode statistics);  12: so100_model.convex (GJK/EPA mesh collider, MuJoCo 3.3.3 default), box-box up to 8 contacts, cube-table one convex contact;  11: so100_buffers.ncon_dropped, debug stride 160 (contact friction forces), so100_set_fused_build;  10: so100_hull_cells (MPR support lookup);  9: pad/link-hull pairs (SO100_NPAIR 191);  8: fused step kernel, so100_set_step_mode;  7: reward64 buffer;  6: Base hull + pad pairs (SO100_NPAIR 155, SO100_NHULL_ALL 10); 5: EE/mocap weld, render API */

/* tasks (gym_so100/__init__.py:4-32 ids; single_arm.py task classes) */
#define SO100_TASK_CUBE_TO_BIN 0          /* gym_so100/SO100CubeToBin-v0, TimeLimit 700 */
#define SO100_TASK_TOUCH_CUBE 1           /* gym_so100/SO100TouchCube-v0, TimeLimit 300 */
#define SO100_TASK_TOUCH_CUBE_SPARSE 2    /* gym_so100/SO100TouchCubeSparse-v0, TimeLimit 300 */
#define SO100_TASK_GOAL 3                 /* SO100GoalEnv (env.py:188-409), own 300-step limit */

/* step flags */
#define SO100_FLAG_AUTORESET 1            /* reset done envs in-kernel, final obs -> final_obs */
#define SO100_FLAG_DR 2                   /* per-env domain randomisation (dr_params)          */

typedef struct so100_buffers {
  /* per-env state, updated in place */
  float*    qpos;            /* [N,13]  hinges(6) cube pos(3) cube quat wxyz(4) */
  float*    qvel;            /* [N,12]  hinges(6) cube linear(3, world) angular(3, body) */
  float*    qacc_warmstart;  /* [N,12] */
  int32_t*  elapsed;         /* [N]     steps in the current episode (TimeLimit counter) */
  uint32_t* episode;         /* [N]     episodes started (drives in-kernel reset seeds) */
  /* inputs */
  const float* action;       /* [N,6]   in [-1,1] (action_space Box) */
  /* outputs (any may be NULL) */
  float*    obs;             /* [N,15]  box(3) bin(3) ee(3) qpos[:6] */
  float*    reward;          /* [N] */
  uint8_t*  terminated;      /* [N] */
  uint8_t*  truncated;       /* [N] */
  uint8_t*  success;         /* [N]     info["is_success"] */
  float*    final_obs;       /* [N,15]  obs of the finished episode when auto-reset fired */
  uint8_t*  diverged;        /* [N]     non-finite / exploding state detected (env reset) */
  uint32_t* contact_bits;    /* [N]     bit p: contact pair p active after the step */
  /* GoalEnv (task SO100_TASK_GOAL) */
  float*    achieved_goal;   /* [N,3] */
  float*    desired_goal;    /* [N,3] */
  int32_t*  total_steps;     /* [N]     curriculum counter (env.py:324) */
  /* domain randomisation (flag SO100_FLAG_DR): [N,4] = cube mass scale, friction scale,
   * action-noise sigma, reserved */
  const float* dr_params;
  /* diagnostics: [N, SO100_DBG_STRIDE] floats or NULL */
  float*    debug;
  /* EE / mocap variant (model.ee = 1): [N,7] mocap body pose, position(3) + quaternion wxyz(4), the
   * target the weld equality pulls ee_site to (teleop_ee.py:52-98 drives data.mocap_pos/quat); NULL =
   * the model's default pose */
  const float* mocap;
  /* [N] the reward in float64, as the reference returns it (task_reward computes in double; `reward`
   * holds its float32 rounding, exact for the CubeToBin / sparse / GoalEnv ladders, rounded for the dense
   * TouchCube shaping); NULL = not written */
  double*   reward64;
  /* [N] contacts left out of the env's contact list, summed over the step's substeps (the oracle's ncon_dropped).
   * Since ABI 14 the list holds every contact (SO100_NCON_MAX, as MuJoCo keeps every contact), so this is always
   * written as 0: kept as a checked invariant.  NULL = not written */
  uint32_t* ncon_dropped;
  /* Device-side episode statistics (what gymnasium's RecordEpisodeStatistics / SB3's VecMonitor keep on the
   * host, reference scripts/train_sac.py:290; SURVEY §5 Metrics), written by the step epilogue; the host reads
   * them only on demand.  ep_final and ep_accum are written only when ep_return is given.  NULL = not kept.
   *   ep_return [N]   return of the running episode: the sum of its float64 rewards so far; set to 0 when the
   *                   episode ends (terminated or truncated, with or without auto-reset) and by so100_reset;
   *                   without auto-reset, an env stepped on past its TimeLimit without a reset is counted once;
   *   ep_final  [N,2] return and length (steps) of the env's last finished episode, written at its end;
   *   ep_accum  [N,4] over the env's finished episodes: count, successes (ended with is_success), sum of
   *                   returns, sum of lengths; never cleared by the library (the caller zeroes it). */
  double*   ep_return;
  double*   ep_final;
  double*   ep_accum;
} so100_buffers;

/* Debug record per env (floats), written by the last substep of a step when `debug` is not NULL:
 *   [0] ncon  [1] solver iterations  [2] last improvement  [3] nefc  [4..15] qacc (the last solve)
 *   [16..31] contact dist  [32..47] contact normal force (efc_force row 0 of contact c)   (contacts c < 16)
 *   [48..63] contact pair id (-1 unused)  [64..75] qacc_smooth  [76..87] dof frictionloss forces
 *   [88..95] profiling stamps (diagnostic builds)
 *   [96..143] contact c's friction forces (efc_force rows 1..3 of contact c) at 96 + 3 c   (contacts c < 16)
 *   [144..159] reserved
 *   [SO100_DBG_OVF + 6 (c - 16) ...] contacts c >= 16 of the list: dist, pair id, normal force, 3 friction forces */
#define SO100_DBG_OVF 160
#define SO100_DBG_STRIDE (SO100_DBG_OVF + 6 * (SO100_NCON_MAX - SO100_MAXCON))   /* 3,922 */

typedef struct so100_env so100_env;   /* opaque: device model copy + launch config */

int         so100_abi_version(void);
const char* so100_last_error(void);
/* (ABI 16) the content hash (sha256, 16 hex digits) of the sources the library was built from: ties a committed
 * measurement (profiles/r05_pmc_step_*.json) to the kernels it measured (bench.py reports traffic only on a match) */
const char* so100_source_hash(void);
/* sizeof(so100_model), sizeof(so100_buffers) as compiled — lets bindings verify their mirrors. */
int         so100_struct_sizes(int* model_bytes, int* buffers_bytes);

/* Upload the model (converted to fp32) to `device`.  n_envs > 0.  Returns NULL on error. */
so100_env*  so100_create(const so100_model* model, int n_envs, int device);
int         so100_destroy(so100_env* env);
int         so100_num_envs(const so100_env* env);

/* Task selection: task id, TimeLimit (max_episode_steps; <= 0 = none), base seed for in-kernel resets,
 * global index of this shard's env 0 (multi-GPU sharding: in-kernel seeds use the global env id). */
int so100_configure(so100_env* env, int task, int max_episode_steps, uint64_t base_seed, int env_offset);

/* Reset the envs whose mask byte is non-zero (mask NULL = all).  seeds: [N] uint32 per-env seeds for
 * the reference's RandomState(seed) cube spawn (utils.py:18-29), or NULL -> in-kernel seed from
 * (base_seed, env, episode).  Writes obs (and GoalEnv goals). */
int so100_reset(so100_env* env, const so100_buffers* b, const uint8_t* mask, const uint32_t* seeds,
                void* stream);

/* One env step for all N envs (10 physics substeps + final position stage + reward/obs epilogue).
 * The N envs are split into up to 4 contiguous chunks (so100_chunk_info) whose launch sequences run
 * concurrently on internal streams forked from and joined back to `stream`: from the caller's side
 * the step is one ordered operation on `stream`. */
int so100_step(so100_env* env, const so100_buffers* b, int flags, void* stream);

/* Kernel timing for the benchmark's roofline (not needed for stepping).  so100_profile_enable(env,
 * max_steps) allocates HIP events for up to max_steps subsequent so100_step calls (0 frees them and
 * stops recording); while enabled each step records an event on its stream before its first launch
 * and after every launch (stage / solver kernels) of the first chunk.  so100_profile_read synchronises
 * on the last event and returns the summed device time of the solver and of the stage launches since
 * enabling. */
int so100_profile_enable(so100_env* env, int max_steps);
int so100_profile_read(so100_env* env, double* solver_ms, int* solver_launches, double* stage_ms,
                       int* stage_launches);

/* Step mode (Newton solver): 1 = the whole env step as ONE fused kernel launch over all N envs, the
 * substep's constraint rows handed from the assembly to the solve in registers; 0 = the split path, per
 * substep a stage kernel and a solver kernel exchanging an HBM record (2 nsubstep + 1 launches per env
 * chunk); -1 = auto (default): fused at every N (SO100_FUSED_MAX=n: split above n).  Both give
 * the same results bit for bit.  The PGS solver always runs split.  so100_step_mode returns the mode in
 * effect (0/1).  In fused mode so100_profile_read reports the fused launches as the solver launches
 * (stage: 0) and so100_chunk_info reports 1 chunk of N envs. */
int so100_set_step_mode(so100_env* env, int fused);
int so100_step_mode(const so100_env* env);

/* Register budget of the fused kernel's product build (the build launched when `debug` is NULL): 2 = 2 waves
 * per SIMD (186 VGPRs, no scratch), 3 = 3 waves per SIMD (168 VGPRs), 0 = auto (default: the 2-wave build
 * when the grid fits the chip at 2 waves per SIMD, <= 8 x CUs workgroups; the 3-wave build above).  The
 * SO100_FUSED_WAVES environment variable sets the initial value.  Register allocation only: every build
 * gives the same results bit for bit (tests/test_gpu_parity.py test_product_builds_bitwise).
 * so100_fused_build returns the build the next fused step of the env launches (1 = the debug build). */
int so100_set_fused_build(so100_env* env, int waves);
int so100_fused_build(const so100_env* env, int debug);

/* Support-direction cells of the convex hulls (host only; no device needed).  The MPR collider's hull
 * support (the first vertex maximising n . v, MuJoCo's mesh support by exhaustive scan) reads a candidate
 * list instead of the whole hull: the direction's cube-map face (largest |n_k|) and its G x G cell on that
 * face select the vertices that can be the support for some direction of the cell (a vertex beaten by one
 * other vertex by >= 1e-6 over the whole cell, its bounds widened by 1e-3, is left out), so the scan of the
 * list returns the same vertex as the scan of the hull.
 *   cells[SO100_NHULL_ALL * SO100_HULL_NCELL]: hull k, face f (2 axis + (n_axis < 0)), cell (cu, cv) at
 *     k * NCELL + (f * G + cu) * G + cv: start << 8 | count (count 0: scan the whole hull);
 *   cand[cap][4]: x, y, z (the hull vertex as float) and the vertex index within the hull (as float bits).
 * Returns the number of candidates (cand may be NULL to query it), -1 on error. */
/* (SO100_HULL_CELLG, SO100_HULL_NCELL: so100_model.h) */
int so100_hull_cells(const so100_model* model, uint32_t* cells, float* cand, int cap);

/* The cells' block table, exactly as so100_create uploads it behind the device model (host only; added under ABI 25): the fused
 * step's 2-wave build reads one block per support and nothing else (its 3-wave builds read the cell's entry first).  SO100_HULL_BLK = 16 entries (x, y, z, vertex
 * index as float bits) per cell, cell c at blk[16 c .. 16 c + 15]: a cell whose list has 1..16 candidates holds the
 * list, padded with its last candidate; a cell with no list or a longer one holds 16 entries of zero coordinates and
 * the index SO100_HULL_BLK_NONE, and the kernel goes on to the cell's entry (so100_hull_cells).
 *   blk[cap][4]; returns the number of entries (SO100_NHULL_ALL * SO100_HULL_NCELL * 16; blk may be NULL to query
 * it), -1 on error. */
#define SO100_HULL_BLK 16
#define SO100_HULL_BLK_NONE 0x7fffffff
int so100_hull_blocks(const so100_model* model, float* blk, int cap);

/* The step kernels' hull support on its own (a test probe; added under ABI 25): for each of the n directions dirs[n][3] (DEVICE
 * float32) the first vertex of hull `hull` (0 .. SO100_NHULL_ALL - 1) maximising dir . v: use_cells 1 through the cells'
 * block table alone (the fused step's 2-wave build: one load per support), 2 through the cell's entry and then its
 * block (the fused step's 3-wave builds), 0 by the whole-hull scan (the split step): out[n][4] (DEVICE) takes the
 * vertex (x, y, z) and its index within the hull (as float bits).  One workgroup per 16 directions on the null
 * stream; returns after the kernel has finished.  0, or -1 on error. */
int so100_hull_support_probe(so100_env* env, int hull, const float* dirs, int n, int use_cells, float* out);

/* Number of env chunks and the env count of chunk 0 (the launches so100_profile_read times). */
int so100_chunk_info(const so100_env* env, int* nchunks, int* profiled_envs);

/* Adds the contact count of the last solver launch, summed over the N envs, to *accum (DEVICE
 * uint64).  Enqueued on `stream`, no synchronisation. */
int so100_contact_count(so100_env* env, uint64_t* accum, void* stream);
/* Writes each env's contact count of the last solver launch (the last substep's list) to out (DEVICE int32 [N]).
 * Enqueued on `stream`, no synchronisation.  (ABI 14) */
int so100_contact_counts(so100_env* env, int32_t* out, void* stream);
/* (ABI 17) The fused step's contact-record pool: out[0] = pool entries taken (wave-substeps whose
 * env lists passed the 16 held on chip), out[1] = entry requests that found none free (0 by construction: each XCD's
 * pool holds as many entries as the XCD can hold fused waves resident), out[2] = entries per XCD; the first two summed
 * over the steps since so100_create or the last reset != 0 call.  Synchronises the device (a benchmark / test hook). */
int so100_pool_stats(so100_env* env, uint64_t* out, int reset);
/* (ABI 18) Env packing of the fused step: a wave steps 4 envs in lockstep and waits for the slowest
 * of them in every solver loop, so before each launch the envs of every block of 64 consecutive envs are ranked by
 * their last step's solver cost and cut into the waves' quartets.  A schedule only: every result is bit for bit the
 * same with it on or off.  mode: -1 auto (default; off at every size: it measured no gain at 65,536 envs and slower
 * below), 0 off, 1 on; the SO100_PACK environment variable sets the initial value.
 * so100_env_packing returns what the next fused step uses (0 | 1). */
int so100_set_env_packing(so100_env* env, int mode);
int so100_env_packing(const so100_env* env);
/* The order the last fused launch used, to out (HOST int32 [min(cap, 4 * ceil(N / 4))]): out[4 * slot + row] = the env
 * that row `row` of launch slot `slot` stepped; ids >= N are idle rows.  Synchronises the device (a test hook). */
int so100_env_order(so100_env* env, int32_t* out, int cap);
/* Each env's solver cost in the last packed fused step (recorded only while packing is on), summed over its substeps,
 * to out (HOST uint32 [min(cap, N)]): Newton loop passes << 24 (saturating at 255) | contacts << 12 | convex
 * narrowphase items (saturating at 4095 each): the packing key.  so100_wave_cost: the shader cycles of each wave of
 * the last fused step (HOST uint32 [min(cap, ceil(N / 4))]), indexed by launch slot with packing on and by natural
 * group (env / 4) with it off.  Both synchronise the device (profiling hooks). */
int so100_env_cost(so100_env* env, uint32_t* out, int cap);
int so100_wave_cost(so100_env* env, uint32_t* out, int cap);

/* ---- camera images: the reference's default observation, obs_type
 * "so100_pixels_agent_pos" (gym_so100/__init__.py:4-32) = the `top` camera rendered by dm_control
 * (gym_so100/env.py:84-94,130-136; scene_so100.xml:30).  A rasteriser of its own (not MuJoCo's OpenGL
 * output): flat Lambert shading of the visible geoms under the scene's lights.  DESIGN.md §3.7. */
#define SO100_MAX_LIGHTS 4
typedef struct so100_camera {
  float pos[3];                     /* camera position (world) */
  float mat[9];                     /* row-major rotation; columns = camera x (right), y (up), z (backward) */
  int   track;                      /* 1: mode="targetbody" on the ee body, frame recomputed per env (mat unused) */
  float fovy;                       /* vertical field of view, degrees */
  float znear;                      /* triangles with a vertex nearer than this are not drawn */
  float head_ambient, head_diffuse; /* headlight (scene_so100.xml:9) */
  int   nlight;                     /* directional lights (scene_so100.xml:13-18) */
  float light_dir[SO100_MAX_LIGHTS][3];
  float light_diffuse[SO100_MAX_LIGHTS];
} so100_camera;
/* Upload the scene's triangles (host arrays): tri [ntri][3][3] vertices in their body's frame, body
 * [ntri] (0 world, 1 Base, 2..7 arm links, 8 cube), rgb [ntri][3] base colour in [0, 1]. */
int so100_render_mesh(so100_env* env, const float* tri, const int* body, const float* rgb, int ntri);
/* Render the N envs at qpos (device [N][13]) from `cam` into out (device [N][height][width][3] uint8);
 * mask (device [N] uint8, NULL = all) limits the envs drawn, the others' images are left as they were.
 * Enqueued on stream; width <= 4096 and width * height <= 1 << 22. */
int so100_render(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam, int width,
                 int height, uint8_t* out, void* stream);
/* (ABI 19) The same launch with several sinks: the image is rasterised once and the band -> image phase writes every
 * non-NULL sink.  A masked-out env is untouched in every sink; background is 0 / 0.0f.  No alignment is asked of any
 * pointer: a sink may be a slice of a larger allocation. */
typedef struct so100_image_out {
  uint32_t size;        /* sizeof(so100_image_out): the callee rejects a mismatch */
  uint8_t* hwc;         /* [n][H][W][3] or NULL (what so100_render writes) */
  uint8_t* chw;         /* [n][3][H][W] or NULL */
  float*   flat;        /* [n][flat_pitch] or NULL: floats [0, 3HW) of env i = its HWC bytes / 255, each quotient the
                           true float32 division (numpy's np.float32(b) / np.float32(255), the reference's env.py:267-270) */
  int64_t  flat_pitch;  /* floats per env, >= 3*H*W; floats beyond 3HW are never written */
} so100_image_out;
/* Nonzero (text in so100_last_error) for a NULL env, a wrong `size`, no sink at all or flat_pitch < 3HW, and for what
 * so100_render rejects.  so100_render is the hwc-only case of this call. */
int so100_render_to(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam, int width,
                    int height, const so100_image_out* out, void* stream);

/* ---- (ABI 20) visual domain randomisation: camera, lights and colours per env.  The physical
 * randomisation (SO100_FLAG_DR) leaves every image drawn from one camera under one set of lights; here env i is drawn
 * from its own record views[i]. */
#define SO100_NMATERIAL 5   /* 0 table, 1 bin, 2 arm light parts, 3 arm dark parts, 4 cube */
typedef struct so100_view {          /* one per env, DEVICE memory, 40 dwords = 160 B */
  float pos[3]; float mat[9]; float fovy;                    /* as so100_camera's */
  float head_ambient, head_diffuse;
  float light_diffuse[SO100_MAX_LIGHTS]; float light_dir[SO100_MAX_LIGHTS][3];
  uint32_t rgb[SO100_NMATERIAL];     /* packed RGB8 base colour per material (R in bits 0-7, G 8-15, B 16-23) */
  uint32_t reserved[4];
} so100_view;
int so100_view_bytes(void);          /* sizeof(so100_view) as compiled: lets bindings verify their mirror */
/* Upload each triangle's material id (host [ntri], every id < SO100_NMATERIAL) for the mesh of the last
 * so100_render_mesh call, which drops the ids of the mesh before it.  Nonzero for an ntri other than the mesh's or an id
 * out of range. */
int so100_render_materials(so100_env* env, const uint8_t* material, int ntri);
/* so100_render_to with env i drawn from views[i] (device [N]): its pos, mat, fovy, headlight terms, light directions
 * and diffuses, and as a triangle's base colour views[i].rgb[material].  cam supplies only the launch-uniform track,
 * znear and nlight; with track = 1 the frame is the targetbody rule from the env's own pos (mat unused).  Nonzero
 * (text in so100_last_error) for NULL views, no uploaded materials, and for what so100_render_to rejects. */
int so100_render_views(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                       const so100_view* views, int width, int height, const so100_image_out* out, void* stream);
/* The ranges the records are drawn from.  Half-widths are symmetric about the base value, [lo, hi] pairs scale it;
 * a range of zero width (half-width 0, lo = hi = 1) gives the base value bit for bit. */
typedef struct so100_view_dr {
  uint32_t size;                         /* sizeof(so100_view_dr): the callee rejects a mismatch */
  uint32_t reserved0;
  uint64_t seed;
  float cam_pos;                         /* camera position half-width per axis, metres */
  float cam_rot;                         /* half-width per component of a rotation vector about the camera's own axes,
                                            radians: mat' = mat . Rodrigues(v) */
  float fovy[2];                         /* scale of fovy */
  float ambient[2], headlight[2];        /* scale of head_ambient, head_diffuse */
  float light[SO100_MAX_LIGHTS][2];      /* scale of each directional light's diffuse (independent draws) */
  float light_rot;                       /* half-width per component of one rotation vector (world axes) that turns
                                            every light direction, radians */
  float color[SO100_NMATERIAL][2];       /* per-channel scale of each material's base colour (three draws) */
  float reserved1;
} so100_view_dr;
/* Fill views[i] (device [N]) of the envs whose mask byte is non-zero (device [N], NULL = all) on the device: every
 * draw is a pure function of (dr->seed, global env id = env_offset + i, episode[i], field number), so the records
 * depend neither on the sharding nor on the mask nor on launch order.  U[0,1) = the top 24 bits of
 * splitmix64(splitmix64(seed ^ id * 0x100000001B3 ^ field * 0xD1B54A32D192ED03) + episode) / 2^24 (the hash of the
 * physical randomisation's fields 1 and 2 with the episode mixed in); fields: 16-18 camera position x y z, 19-21
 * camera rotation vector, 22 fovy, 23 ambient, 24 headlight, 25 + l light l, 29-31 light rotation vector,
 * 32 + 3 material + channel colour.  Colour channel = floor(clip(base * s, 0, 1) * 255 + 0.5), base = base_rgb byte /
 * 255.  cam: the base camera (host); base_rgb: host [SO100_NMATERIAL] packed RGB8; episode: device uint32 [N] or NULL
 * = 0.  Enqueued on stream. */
int so100_views_sample(so100_env* env, const so100_view_dr* dr, const so100_camera* cam, const uint32_t* base_rgb,
                       const uint32_t* episode, const uint8_t* mask, so100_view* views, void* stream);

/* ---- (ABI 21) depth and segmentation images (dm_control's physics.render(depth=True / segmentation=True)), written by
 * the render launch itself: the kernel's per-pixel key is depth bits << 32 | RGB8 << 8 | label, so the nearest surface
 * wins, equal depths take the smaller packed RGB (the colour images are so100_render_to's / so100_render_views' bit
 * for bit) and equal colours the smaller label.  DESIGN.md §3.7. */
/* labels: host [ntri] bytes, each < 255, for the mesh of the last so100_render_mesh call (a new mesh drops them) */
int so100_render_labels(so100_env* env, const uint8_t* label, int ntri);
typedef struct so100_aux_out {
  uint32_t size;     /* sizeof(so100_aux_out): the callee rejects a mismatch */
  float*   depth;    /* [n][H][W] or NULL; background 0.0f */
  uint8_t* label;    /* [n][H][W] or NULL; background 255 */
} so100_aux_out;
int so100_aux_out_bytes(void);
/* so100_render_to / so100_render_views (views may be NULL) with the further sinks of aux; out may be NULL.  depth is
 * the float32 the depth test compared: the distance along the camera's viewing axis in metres (not the ray length).
 * label is the winning triangle's uploaded byte.  No alignment is asked of label; depth must be 4-byte aligned, as a
 * float pointer is.  A masked-out env is untouched in every sink.  Nonzero (text in so100_last_error) for a NULL env, a
 * wrong `size` in either struct, no sink at all across both, a label sink without uploaded labels, views without
 * uploaded materials, and for what so100_render_to rejects. */
int so100_render_aux(so100_env* env, const float* qpos, const uint8_t* mask, const so100_camera* cam,
                     const so100_view* views, int width, int height, const so100_image_out* out,
                     const so100_aux_out* aux, void* stream);

/* ---- (ABI 22) several cameras in one launch, world-fixed or mounted on a body (the reference's observation is `top`,
 * `angle` and `front_close`, tasks/single_arm.py:88-102, and its arm carries `left_wrist` on Fixed_Jaw,
 * so_arm100.xml:126).  The launch's grid is (env, camera): block (env, c) is so100_render_aux's block drawing env from
 * cam[c] and views[c * N + env] into slot env * ncam + c of every sink.  DESIGN.md §3.7. */
#define SO100_MAX_CAMS 4
typedef struct so100_cams {
  uint32_t size;                          /* sizeof(so100_cams): the callee rejects a mismatch */
  int32_t  ncam;                          /* 1..SO100_MAX_CAMS */
  so100_camera cam[SO100_MAX_CAMS];       /* track, znear and nlight are per camera */
  int32_t  frame_body[SO100_MAX_CAMS];    /* 0: cam[c].pos / mat are in the world, used as they are; 1..8: in that body's
                                             frame (1 Base, 2..7 arm links, 8 cube): pos_w = R_b pos + p_b per env, then
                                             track = 1: the targetbody rule from pos_w; track = 0: R_b mat (a rigid mount).
                                             A view record's pos and mat are in the same frame as its camera's. */
} so100_cams;
int so100_cams_bytes(void);
/* Sinks (K = ncam; with K = 1 so100_render_aux's): hwc [N][K][H][W][3], chw [N][K][3][H][W], depth and label
 * [N][K][H][W], flat [N][flat_pitch] with camera c in floats [c*3HW, (c+1)*3HW) and flat_pitch >= K*3HW.  views is
 * camera-major, [K][N] (each camera's records a contiguous [N] array so100_views_sample fills), or NULL.  qpos and mask
 * are per env: an env is drawn in all its cameras or in none, and nothing outside a drawn slot's span is written.
 * Enqueued on stream, never synchronises.  Nonzero (text in so100_last_error), before any device work, for a wrong
 * `size` in any of the three structs (checked first), NULL cams, ncam outside 1..SO100_MAX_CAMS, a frame_body outside
 * 0..8, flat_pitch < ncam*3HW, width*height*ncam > 1 << 22, and for what so100_render_aux rejects. */
int so100_render_cams(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                      const so100_view* views, int width, int height, const so100_image_out* out,
                      const so100_aux_out* aux, void* stream);

/* ---- (ABI 23) cast shadows (scene_so100.xml:13-16: of the three directional lights the middle one, dir="-1 1 -1",
 * keeps MuJoCo's castshadow default).  so100_render_cams with one light occluded per pixel: each block rasterises the
 * caster triangles into an orthographic map_size x map_size depth map along the light, then a pixel whose surface point
 * lies more than `bias` behind the map's depth takes the colour it has with that light's diffuse taken as 0.  With `full`
 * the image of so100_render_cams and `dark` its image from the same records with light_diffuse[light] = 0, the colour
 * sinks hold where(shadow, dark, full) bit for bit; depth and label are so100_render_cams'.  DESIGN.md §3.7. */
#define SO100_SHADOW_MAP_MAX 64        /* map_size <= this: the map lives in LDS */
typedef struct so100_shadow {
  uint32_t size;        /* sizeof(so100_shadow): the callee rejects a mismatch */
  int32_t  light;       /* the casting light, 0..nlight-1 of every camera; -1: nothing casts (the image is so100_render_cams') */
  int32_t  map_size;    /* S, a multiple of 8 in 8..SO100_SHADOW_MAP_MAX */
  float    center[3];   /* the map is the square of half-side `radius` about `center`, seen along the light: */
  float    radius;      /*   u = normalize(z x d) (x if |z x d| < 1e-6), v = d x u, texel = floor((((P-center).u|v) / radius * 0.5 + 0.5) * S) */
  float    bias;        /* metres, >= 0: occluded iff map depth < (P-center).d - bias */
  uint8_t* shadow_out;  /* [N][K][H][W] or NULL: 1 occluded, 0 lit, background 0; no alignment asked */
} so100_shadow;
int so100_shadow_bytes(void);
/* casters: host [ntri] bytes, non-zero = the triangle is drawn into the map, for the mesh of the last so100_render_mesh
 * call (a new mesh drops them) */
int so100_render_casters(so100_env* env, const uint8_t* caster, int ntri);
/* so100_render_cams' arguments and refusals, plus (each before any device work, text in so100_last_error): NULL shadow
 * or a wrong `size`, light outside -1..nlight-1 of any camera, a map_size that is no multiple of 8 in
 * 8..SO100_SHADOW_MAP_MAX, radius not finite or <= 0, bias negative or not finite, a non-finite center, casters not
 * uploaded.  shadow_out alone counts as a sink.  A point outside the map is lit. */
int so100_render_shadow(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                        const so100_view* views, int width, int height, const so100_image_out* out,
                        const so100_aux_out* aux, const so100_shadow* shadow, void* stream);

/* ---- (ABI 24) multisample anti-aliasing (scene_so100.xml:8, <quality offsamples="4"/>: the reference renders into a
 * 4x multisampled buffer).  so100_render_cams' colour sinks with `samples` coverage samples per pixel: sample s of pixel
 * (x, y) is the point (x + 0.5 + offset[s][0], y + 0.5 + offset[s][1]); coverage, depth and the depth test are the
 * rasteriser's rules at that point, a triangle is shaded once and its flat colour goes to every sample it covers, and a
 * pixel's byte is (sum of its samples' bytes + samples / 2) / samples per channel (round half up; an empty sample is the
 * background's 0).  The resolve runs in LDS inside the launch: W x H bytes leave the chip.  With samples = 1 and offset 0
 * the image is so100_render_cams'.  DESIGN.md §3.7. */
#define SO100_MSAA_MAX 4
typedef struct so100_msaa {
  uint32_t size;                       /* sizeof(so100_msaa): the callee rejects a mismatch */
  int32_t  samples;                    /* 1, 2 or 4 */
  float    offset[SO100_MSAA_MAX][2];  /* (x, y) of the first `samples` from the pixel centre, each inside (-0.5, 0.5) */
} so100_msaa;
int so100_msaa_bytes(void);
/* so100_render_cams' arguments without aux (depth and labels are pixel-centre quantities: draw them with
 * so100_render_cams, out NULL), and its refusals, plus (each before any device work, text in so100_last_error): NULL msaa
 * or a wrong `size` (checked first), samples other than 1, 2 or 4, one of the first `samples` offsets not finite or with
 * |o| >= 0.5, width * samples > 4096, NULL out or no colour sink in it.  Enqueued on stream, never synchronises. */
int so100_render_msaa(so100_env* env, const float* qpos, const uint8_t* mask, const so100_cams* cams,
                      const so100_view* views /* [ncam][N] or NULL */, int width, int height,
                      const so100_image_out* out, const so100_msaa* msaa, void* stream);

/* ---- (ABI 25) Cartesian end-effector action mode on the joint model: a prologue that turns an
 * end-effector delta a = (dx, dy, dz, droll, grip) in [-1,1]^5 (clipped first) into the six normalised joint actions
 * so100_step takes; the step itself is untouched.  The reference drives its EE scene the same way, mocap_pos moved by
 * +-0.01 m per key (scripts/teleop_ee.py:53-64).  State: q_cmd [N,5], the last commanded targets of the five arm joints
 * (radians): the target moves from where the last command put it, not from the sagging measured pose.  Per env, with
 * q = qpos[0:6], ee(.) = ee_site with the five arm joints at the argument, [lo_j, hi_j] joint j's range:
 *   1. reinit[i] != 0: q_cmd <- q[0:5];
 *   2. p = clip(ee(q_cmd) + pos_scale a[0:3], ws_lo, ws_hi);
 *   3. c = q_cmd[0:4]; `iters` times: e = p - ee(c); J[:,j] = axis_j x (ee - anchor_j), j = 0..3 (wrist roll and jaw do
 *      not move ee_site); dq = J' (J J' + damping^2 I)^-1 e; dq *= dq_max / max(max|dq|, dq_max); c <- clip(c + dq, lo, hi);
 *   4. q_cmd[0:4] <- q[0:4] + clip(c - q[0:4], -lead_max, lead_max)   (anti-windup against a blocked or unreachable target);
 *   5. q_cmd[4] <- clip(q_cmd[4] + rot_scale a[3], lo_4, hi_4);
 *   6. joint_action[j] = clip(2 (q_cmd[j] - lo_j) / (hi_j - lo_j) - 1, -1, 1), j < 5; joint_action[5] = a[4] (the
 *      gripper stays the joint mode's absolute command); ee_target[i] = p.
 * float32 throughout; every step is continuous in its inputs. */
typedef struct so100_ee_ctrl {
  uint32_t size;        /* sizeof(so100_ee_ctrl): the callee rejects a mismatch */
  int32_t  iters;       /* 1..8 damped least-squares steps per call */
  float pos_scale;      /* metres per unit of a[0:3], > 0 */
  float rot_scale;      /* radians of wrist roll per unit of a[3], >= 0 */
  float damping;        /* > 0 */
  float dq_max;         /* radians, > 0: the largest joint move of one least-squares step */
  float lead_max;       /* radians, > 0: the most q_cmd may lead the measured pose */
  float ws_lo[3], ws_hi[3];   /* the box the target is kept in, ws_lo <= ws_hi */
} so100_ee_ctrl;
int so100_ee_ctrl_bytes(void);
/* One launch on `stream`, no allocation, no synchronisation.  Nonzero (text in so100_last_error), before any device
 * work: NULL ctrl, a wrong `size` (checked first), iters outside 1..8, a pos_scale, rot_scale, damping, dq_max or
 * lead_max that is not finite or not positive (rot_scale may be 0), a non-finite or inverted workspace box, a NULL env,
 * qpos, action, q_cmd or joint_action, a model with ee = 1 (the weld variant has its mocap input). */
int so100_ee_action(so100_env* env, const so100_ee_ctrl* ctrl, const float* qpos /* [N,13] */,
                    const float* action /* [N,5] */, const uint8_t* reinit /* [N] or NULL */,
                    float* q_cmd /* [N,5] in/out */, float* joint_action /* [N,6] */,
                    float* ee_target /* [N,3] or NULL */, void* stream);
/* The kinematics of the above as a standalone op (for parity tests): qpos[n,13] -> ee[n,3] = ee_site,
 * jac[n,3,5] = its positional Jacobian over joints 0..4 (the roll column is written: it is 0 up to rounding). */
int so100_ee_jacobian(so100_env* env, int n, const float* qpos, float* ee, float* jac, void* stream);

/* ---- (additions to ABI 25) per-episode physical randomisation and an actuation-latency model: two
 * launches beside the untouched step.  so100_dr_sample rewrites the dr_params rows so100_step reads (and draws each
 * env's actuator record); so100_actuate turns the commanded action into the applied one the step then takes. */
#define SO100_ACT_MAX_DELAY 7          /* control steps; the command ring holds SO100_ACT_HIST = 8 */
#define SO100_ACT_HIST 8
typedef struct so100_dr_ranges {
  uint32_t size;          /* sizeof(so100_dr_ranges): the callee rejects a mismatch */
  uint32_t reserved0;
  uint64_t seed;
  float   mass[2];        /* [lo, hi] of the cube mass scale, finite, > 0 */
  float   friction[2];    /* [lo, hi] of the contact friction scale, finite, > 0 */
  int32_t delay[2];       /* [lo, hi] of the actuation delay in control steps, 0..SO100_ACT_MAX_DELAY */
  float   smoothing[2];   /* [lo, hi] of the first-order smoothing factor alpha, in (0, 1]; 1 = none */
  float   rate[2];        /* [lo, hi] of the slew limit per control step in normalised action units, finite, > 0; >= 2 = none */
} so100_dr_ranges;
int so100_dr_ranges_bytes(void);
/* Draw, on the device, dr_params[i][0:2] = (mass, friction) and / or act_params[i] = (delay, alpha, rate, 0) of the envs
 * whose byte in mask_a or mask_b is non-zero (device [N] each; both NULL = all).  Every draw is so100_views_sample's
 * U[0,1) of (seed, global env id = env_offset + i, episode[i], field): fields 1 mass, 2 friction, 4 delay, 5 smoothing,
 * 6 rate.  Real values: clip(lo + (hi - lo) u, lo, hi) in float32; the delay, with h the 64-bit hash behind u (u = (h >>
 * 40) / 2^24): lo + (((h >> 40) * (hi - lo + 1)) >> 24), stored as a float.  dr_params[i][2:4] (the action-noise sigma
 * and the spare column) and the rows outside the masks are not written.  episode: device uint32 [N] or NULL = 0.  One
 * launch on `stream`, no allocation, no synchronisation.  Nonzero (text in so100_last_error), before any device work and
 * with nothing written: NULL ranges, a wrong `size` (checked first), a NULL env, both outputs NULL, a mass, friction or
 * rate range that is not finite, not positive or inverted, a delay range outside 0..SO100_ACT_MAX_DELAY or inverted, a
 * smoothing range outside (0, 1] or inverted. */
int so100_dr_sample(so100_env* env, const so100_dr_ranges* ranges, const uint32_t* episode /* [N] or NULL */,
                    const uint8_t* mask_a /* [N] or NULL */, const uint8_t* mask_b /* [N] or NULL */,
                    float* dr_params /* [N,4] or NULL */, float* act_params /* [N,4] or NULL */, void* stream);
/* The actuator model, one launch before so100_step.  State per env: hist [SO100_ACT_HIST][N][6] (slot-major: the ring of
 * the last 8 clipped commands), head [N] (calls since the last re-initialisation) and action [N,6] itself, the applied
 * action y of the last call, which is the step's action input.  Per env i and component c, with u = clip(command, -1, 1),
 * (d, alpha, r) = act_params[i][0:3] and [lo_c, hi_c] the model's action range:
 *   1. reinit[i] != 0: hold_c = clip(2 (qpos_c - lo_c) / (hi_c - lo_c) - 1, -1, 1) (the command that holds the measured
 *      pose, so100_ee_action's step 6); every ring slot <- hold, y <- hold, head <- 0;
 *   2. hist[head mod 8] <- u; v = hist[(head - d) mod 8]; head <- head + 1   (while head < d the slot read holds `hold`);
 *   3. w = v if alpha == 1, else y + alpha (v - y);
 *   4. y <- w if |w - y| <= r, else y + copysign(r, w - y);
 *   5. action[i][c] <- y.
 * With d = 0, alpha = 1 and r >= 2 the applied action is clip(command) bit for bit.  float32.  Nonzero (text in
 * so100_last_error) before any device work, every output untouched: a NULL env, qpos, command, act_params, hist, head or
 * action, a model with ee = 1 (its input is the mocap pose). */
int so100_actuate(so100_env* env, const float* qpos /* [N,13] */, const float* command /* [N,6] */,
                  const uint8_t* reinit /* [N] or NULL */, const float* act_params /* [N,4] */,
                  float* hist /* [8][N][6] in/out */, int32_t* head /* [N] in/out */, float* action /* [N,6] in/out */,
                  void* stream);

/* ---- (additions to ABI 25) running observation / reward normalisation on the device: SB3
 * VecNormalize's running statistics in float64, as launches beside the untouched step.  Statistics of one normaliser:
 * device double [3][SO100_NORM_MAX_DIM], row 0 the mean, row 1 the variance, row 2 the count of each column (they start
 * at 0, 1 and 1e-4; the caller writes them).  A call names up to SO100_NORM_MAX_SRC sources, each rows of float32 at
 * (x, row stride in floats, first column, dim); their columns, in order, are the statistics' columns 0 .. D-1,
 * D = sum of dim <= SO100_NORM_MAX_DIM.
 *   update, with the b rows whose mask byte is non-zero (mask NULL = all n; b = 0 changes nothing, bit for bit):
 *     bm = batch mean, bv = population variance of the batch, delta = bm - mean, tot = count + b;
 *     mean <- mean + delta b / tot;  var <- (var count + bv b + delta^2 count b / tot) / tot;  count <- tot.
 *   The moments are float64 sums of (x - mean) and (x - mean)^2 per workgroup, a workgroup taking a contiguous range of
 *   max(rows_per_group, ceil(n / max_groups)) rows (so100_norm_limits); the workgroups' partials are combined in
 *   index order by a second launch, so the result is bit for bit reproducible.  No atomics on the statistics.
 *   apply: y = clip((x - mean) / sqrt(var + epsilon), -clip, clip), computed in float64 and rounded once to float32, to
 *     (y, y_stride) columns 0 .. dim-1 of each source; with a mask only the masked rows are written.  With
 *     SO100_NORM_INVERSE in flags: y = x sqrt(var + epsilon) + mean (no clip).
 * Workspace: so100_norm_work_bytes(n) = groups(n) * 3 * SO100_NORM_MAX_DIM * 8 bytes of device memory, groups(n) =
 * min(max_groups, max(1, ceil(n / rows_per_group))); its contents carry nothing between calls. */
#define SO100_NORM_MAX_DIM 32
#define SO100_NORM_MAX_SRC 3
#define SO100_NORM_INVERSE 1u
typedef struct so100_norm_src {
  const float* x;       /* device rows of float32 */
  float*  y;            /* so100_norm_apply's output rows (may be x's own memory); so100_norm_update ignores it */
  int32_t stride;       /* floats between rows of x, >= offset + dim */
  int32_t offset;       /* first column read, >= 0 */
  int32_t dim;          /* columns, >= 1 */
  int32_t y_stride;     /* floats between rows of y, >= dim (apply only) */
} so100_norm_src;
typedef struct so100_norm {
  uint32_t size;        /* sizeof(so100_norm): the callee rejects a mismatch */
  int32_t  nsrc;        /* 1..SO100_NORM_MAX_SRC */
  double   epsilon;     /* finite, > 0 */
  double   clip;        /* finite, > 0 */
  uint32_t flags;       /* SO100_NORM_INVERSE or 0 */
  uint32_t reserved0;
  so100_norm_src src[SO100_NORM_MAX_SRC];
} so100_norm;
int so100_norm_bytes(void);
/* The moments kernel's constants: rows a workgroup takes below the grid cap, and the cap. */
int so100_norm_limits(int* rows_per_group, int* max_groups);
/* Bytes of workspace for n rows (the formula above); -1 for n < 0. */
int so100_norm_work_bytes(int n);
/* Both: launches on `stream` (update two, apply one), no allocation, no synchronisation; n = 0 launches nothing.
 * Nonzero (text in so100_last_error) before any device work and with nothing written: NULL norm, a wrong `size`
 * (checked first), nsrc outside 1..SO100_NORM_MAX_SRC, a dim outside 1..SO100_NORM_MAX_DIM, an offset < 0, a stride <
 * offset + dim, a y_stride < dim (apply), a total dim > SO100_NORM_MAX_DIM, an epsilon or clip that is not finite or not
 * positive, flags other than SO100_NORM_INVERSE, n < 0, a NULL env, a NULL source pointer x, a NULL y (apply), NULL
 * stats, NULL work (update). */
int so100_norm_update(so100_env* env, const so100_norm* norm, int n, const uint8_t* mask /* [n] or NULL */,
                      double* stats /* [3][32] in/out */, void* work, void* stream);
int so100_norm_apply(so100_env* env, const so100_norm* norm, int n, const uint8_t* mask /* [n] or NULL */,
                     const double* stats /* [3][32] */, void* stream);
/* The return path of reward normalisation, per env i, ret float64 [n], stats the one-column statistics of ret:
 *   SO100_NORM_RET_UPDATE:    ret[i] <- ret[i] gamma + reward[i], then the update above with the n values of ret;
 *   SO100_NORM_RET_NORMALIZE: reward_norm[i] = clip(reward[i] / sqrt(var + epsilon), -clip, clip)   (the updated var);
 *   always:                   ret[i] <- 0 where terminated[i] or truncated[i] is non-zero (either may be NULL).
 * Three launches (one without UPDATE) on `stream`, no allocation, no synchronisation.  Nonzero as above: NULL args, a
 * wrong `size` (checked first), gamma outside (0, 1], a bad epsilon or clip, unknown flags, n < 0, a NULL env, reward,
 * ret or stats, NULL work with UPDATE, NULL reward_norm with NORMALIZE. */
#define SO100_NORM_RET_UPDATE 1u
#define SO100_NORM_RET_NORMALIZE 2u
typedef struct so100_norm_ret {
  uint32_t size;        /* sizeof(so100_norm_ret): the callee rejects a mismatch */
  uint32_t flags;
  double   gamma;       /* in (0, 1] */
  double   epsilon;     /* finite, > 0 */
  double   clip;        /* finite, > 0 */
} so100_norm_ret;
int so100_norm_ret_bytes(void);
int so100_norm_return(so100_env* env, const so100_norm_ret* args, int n, const float* reward /* [n] */,
                      const uint8_t* terminated /* [n] or NULL */, const uint8_t* truncated /* [n] or NULL */,
                      double* ret /* [n] in/out */, double* stats /* [3][32] in/out */, void* work,
                      float* reward_norm /* [n] or NULL */, void* stream);

/* ---- (additions to ABI 25) a hindsight replay buffer for the GoalEnv on the device: SB3's
 * HerReplayBuffer (scripts/train_sac_her.py:236-251 trains with n_sampled_goal = 4, "future") as launches beside the
 * untouched step.  The caller owns every array; so100_her names them.
 *
 * Storage.  A ring of T slots for each of n envs, slot-major ([T][n][...]: the envs of one slot are contiguous, so a push
 * writes contiguous rows).  Slot s of env e holds one transition: obs (the raw observation before the step), next_obs
 * (the true next observation: the final_obs row where the env finished, else the new obs row), goal (the desired goal in
 * force during the step), action (the command given to step), reward, terminated, offset (the transition's index within
 * its episode) and, at an episode's first slot once the episode has closed, length (the episode's transitions).  The
 * achieved goal and the next achieved goal are columns 0..2 of obs and next_obs.  An episode's first slot is
 * (s - offset) mod T, so its length is one load away from any of its slots.
 * Metadata, int32 meta[3][n]: valid_lo[e], count[e], open_len[e].  The count[e] transitions of closed, intact episodes
 * occupy the slots valid_lo, valid_lo + 1, .. (mod T) in episode order; the open episode's open_len[e] transitions follow
 * them; the write cursor is (valid_lo + count + open_len) mod T.  count + open_len <= T.  All zero at the start.
 *
 * so100_her_push, env e (one launch):
 *   1. count + open_len == T (the ring is full): with count > 0 the oldest closed episode goes whole, L = length[valid_lo]:
 *      valid_lo <- (valid_lo + L) mod T, count <- count - L; with count == 0 (an open episode of T transitions: a caller
 *      with T >= its episode cap never gets here) the open episode goes, open_len <- 0.
 *   2. the transition is written at the cursor with offset = open_len (obs and goal from prev_obs / prev_goal);
 *      open_len <- open_len + 1.
 *   3. diverged[e] or discard[e] non-zero: the open episode, this transition included, is erased: open_len <- 0 (the
 *      cursor moves back over it: no hole).  Else terminated[e] | truncated[e]: the episode closes: length[first slot]
 *      <- open_len, count <- count + open_len, open_len <- 0.
 *   4. stage_obs[e] <- obs[e], stage_goal[e] <- goal[e]: the next transition's "before" values.  stage_obs / stage_goal
 *      may be prev_obs / prev_goal themselves (each element is read before it is written, by the same thread).
 * so100_her_discard: open_len <- 0 for the envs whose mask byte is non-zero (mask NULL = all), and, where obs / goal are
 *   given, stage_obs / stage_goal <- their rows for the same envs (after a reset).
 * so100_her_scan (one launch, one workgroup): prefix[e] = count[0] + .. + count[e] for e < n, prefix[n] = the total.
 * so100_her_sample, batch element i (one launch; it reads prefix, so a scan must follow the last push), with
 *   draw(field) = splitmix64(splitmix64(seed ^ (i * 0x100000001B3) ^ (field * 0xD1B54A32D192ED03)) + call), all in
 *   uint64 arithmetic mod 2^64, splitmix64 the finaliser of so100_views_sample (x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30)
 *   * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31), and `call` the caller's count of sample
 *   calls:
 *   total = prefix[n]; total == 0: every output row i is 0, env[i] = 0, slot[i] = goal_slot[i] = -1, nothing of the ring
 *     is read.  Else
 *   r = floor(draw(0) * total / 2^64); e = the first env with prefix[e] > r; slot = (valid_lo[e] + r - prefix[e-1]) mod T
 *     (prefix[-1] = 0): every valid transition is equally likely;
 *   o = offset[slot], first = (slot - o) mod T, len = length[first];
 *   i < floor((1 - 1 / (n_sampled_goal + 1)) * batch) (in float64): the row is relabelled, with the transition
 *     j = o + floor(draw(1) * (len - o) / 2^64) (SO100_HER_FUTURE: the transition's own next achieved goal included),
 *     j = len - 1 (SO100_HER_FINAL) or j = floor(draw(1) * len / 2^64) (SO100_HER_EPISODE) of the same episode:
 *     goal_slot = (first + j) mod T, desired_goal = next_obs[goal_slot][0:3], reward = so100_goal_reward(next_obs[slot]
 *     [0:3], desired_goal) (the same device function); the other rows keep their stored goal and reward, goal_slot = -1;
 *   gathered: observation, achieved_goal (= observation[0:3]), desired_goal, next_observation, next_achieved_goal,
 *     next_desired_goal (= desired_goal), actions, rewards, dones (the stored terminated as 0 / 1: SB3's dones *
 *     (1 - timeouts)), env, slot, goal_slot.
 * Every index read from meta, offset, length or prefix is clamped into its range before it addresses memory. */
#define SO100_HER_FUTURE 0
#define SO100_HER_FINAL 1
#define SO100_HER_EPISODE 2
#define SO100_HER_MAX_ACTION 16
typedef struct so100_her {
  uint32_t size;            /* sizeof(so100_her): the callee rejects a mismatch */
  int32_t  n;               /* envs, >= 0 */
  int32_t  T;               /* slots per env, >= 1, T * n < 2^31 */
  int32_t  action_dim;      /* floats per command, 1..SO100_HER_MAX_ACTION */
  int32_t  strategy;        /* SO100_HER_FUTURE | _FINAL | _EPISODE (sample) */
  int32_t  n_sampled_goal;  /* >= 0 (sample) */
  uint64_t seed;            /* (sample) */
  float*   obs;             /* [T][n][15] */
  float*   next_obs;        /* [T][n][15] */
  float*   goal;            /* [T][n][3] */
  float*   action;          /* [T][n][action_dim] */
  float*   reward;          /* [T][n] */
  uint8_t* terminated;      /* [T][n] */
  int32_t* offset;          /* [T][n] */
  int32_t* length;          /* [T][n] */
  int32_t* meta;            /* [3][n]: valid_lo, count, open_len */
  float*   stage_obs;       /* [n][15] */
  float*   stage_goal;      /* [n][3] */
  int32_t* prefix;          /* [n + 1] */
} so100_her;
int so100_her_bytes(void);
/* The inputs of one push: device rows of the n envs, as the step left them. */
typedef struct so100_her_step {
  uint32_t size;              /* sizeof(so100_her_step) */
  uint32_t reserved0;
  const float*   prev_obs;    /* [n][15]: the observation before the step (the staged rows) */
  const float*   prev_goal;   /* [n][3]: the desired goal in force during the step */
  const float*   obs;         /* [n][15] */
  const float*   final_obs;   /* [n][15]: read where terminated | truncated */
  const float*   goal;        /* [n][3]: the desired goal after the step (a finished env's new one) */
  const float*   action;      /* [n][action_dim] */
  const float*   reward;      /* [n] */
  const uint8_t* terminated;  /* [n] */
  const uint8_t* truncated;   /* [n] */
  const uint8_t* diverged;    /* [n] or NULL */
  const uint8_t* discard;     /* [n] or NULL */
} so100_her_step;
int so100_her_step_bytes(void);
/* The outputs of one sample call: device arrays of `batch` rows, every one required. */
typedef struct so100_her_out {
  uint32_t size;              /* sizeof(so100_her_out) */
  uint32_t reserved0;
  float* observation;         /* [B][15] */
  float* achieved_goal;       /* [B][3] */
  float* desired_goal;        /* [B][3] */
  float* next_observation;    /* [B][15] */
  float* next_achieved_goal;  /* [B][3] */
  float* next_desired_goal;   /* [B][3] */
  float* actions;             /* [B][action_dim] */
  float* rewards;             /* [B] */
  float* dones;               /* [B] */
  int32_t* env;               /* [B] */
  int32_t* slot;              /* [B] */
  int32_t* goal_slot;         /* [B] */
} so100_her_out;
int so100_her_out_bytes(void);
/* The scan's workgroup size W and the elements one pass of the workgroup takes (a multiple of W). */
int so100_her_limits(int* scan_group, int* scan_tile);
/* Bytes of all the arrays of so100_her together: T n (4 (15 + 15 + 3 + action_dim + 1 + 2) + 1) + 4 (3 n + 18 n + n + 1);
 * -1 (text in so100_last_error) for n < 0, T < 1, T * n >= 2^31 or an action_dim outside 1..SO100_HER_MAX_ACTION. */
int64_t so100_her_storage_bytes(int n, int T, int action_dim);
/* All four: launches on `stream` (one each), no allocation, no synchronisation, no atomics; push and discard launch nothing
 * for n = 0, sample nothing for batch = 0.  Nonzero (text in so100_last_error) before any device work and with nothing written, in this order:
 * NULL her, a wrong `size`, T < 1, n < 0, T * n >= 2^31, an action_dim outside 1..SO100_HER_MAX_ACTION, (sample) an
 * unknown strategy, n_sampled_goal < 0, batch < 0, NULL out or a wrong `size` of it, (push) NULL step or a wrong `size` of
 * it; then a NULL env, a NULL array of so100_her, a NULL required pointer of step or out. */
int so100_her_push(so100_env* env, const so100_her* her, const so100_her_step* step, void* stream);
int so100_her_discard(so100_env* env, const so100_her* her, const uint8_t* mask /* [n] or NULL */,
                      const float* obs /* [n][15] or NULL */, const float* goal /* [n][3] or NULL */, void* stream);
int so100_her_scan(so100_env* env, const so100_her* her, void* stream);
int so100_her_sample(so100_env* env, const so100_her* her, int batch, uint64_t call, const so100_her_out* out,
                     void* stream);

/* ---- (additions to ABI 25) a uniform replay buffer for the arm tasks on the device, for state and pixel observations,
 * with the random-shift image augmentation in the sample launch: SB3's DictReplayBuffer
 * (scripts/train_sac.py trains SAC("MultiInputPolicy", buffer_size=50_000, batch_size=256) on {"pixels", "agent_pos"}) as
 * launches beside the untouched step.  The caller owns every array; so100_replay names them.
 *
 * Storage.  A ring of T >= 2 slots for each of n envs, slot-major ([T][n][...]).  Slot s of env e holds one transition:
 * obs (the raw 15-float observation before the step), next_obs (the true next observation: the final_obs row where the
 * env finished, else the new obs row), action (the command given to step), reward, terminated and, with P > 0, obs_img
 * and next_img, P = planes * H * W * chan bytes each: `planes` images of [H][W][chan] bytes.  (planes, chan) = (K, 3) for
 * the env's HWC images of K cameras and (3 K, 1) for channels_first, so that one rule covers [H,W,3], [3,H,W], [K,H,W,3]
 * and [K,3,H,W].  P == 0: no images, obs_img and next_img (and the image pointers of step and out) are NULL.  Both frames
 * of a transition are stored, as DictReplayBuffer stores them.
 * Metadata, int32 meta[2][n]: cursor[e], count[e], all zero at the start.  The slot at the cursor holds the staged
 * "before" half (obs, obs_img) of the next transition, so the ring holds at most T - 1 complete ones: the count[e] valid
 * transitions of env e are the slots cursor - count, .., cursor - 1 (mod T), oldest first.
 *
 * so100_replay_push, env e (one launch), c = cursor[e], k = count[e], done = terminated[e] | truncated[e]:
 *   1. next_obs[c] <- done ? final_obs[e] : obs[e]; next_img[c] <- done ? final_pixels[e] : pixels[e] (the final_pixels
 *      row of an env that is not done is never read).
 *   2. action[c] <- action[e], reward[c] <- reward[e], terminated[c] <- terminated[e] != 0.
 *   3. diverged[e] non-zero (diverged may be NULL): c' = c, k' = k: the transition is dropped, its slot is used again.
 *      Else c' = (c + 1) mod T, k' = min(k + 1, T - 1).
 *   4. obs[c'] <- obs[e], obs_img[c'] <- pixels[e]: the next transition's "before" rows (of a finished env: the new
 *      episode's first).
 *   5. cursor[e] <- c', count[e] <- k'.
 *   One workgroup owns an env whole: every thread of it reads meta[e] before a workgroup barrier, thread 0 writes it after
 *   that barrier, and no other workgroup of the launch touches meta[e] or the env's rows.
 * so100_replay_stage: obs[cursor[e]] <- obs[e], obs_img[cursor[e]] <- pixels[e] for the envs whose mask byte is non-zero
 *   (mask NULL = all); no count and no cursor changes (after a reset).
 * so100_replay_scan (one launch, one workgroup; so100_her_scan's device code): prefix[e] = count[0] + .. + count[e] for
 *   e < n, prefix[n] = the total.
 * so100_replay_sample, batch element i (one launch; it reads prefix, so a scan must follow the last push), with
 *   draw(field) the draw of so100_her_sample above from (seed, call, i, field):
 *   total = prefix[n]; total == 0: every output row i is 0 (shift included), env[i] = 0, slot[i] = -1, nothing of the ring
 *     is read.  Else
 *   r = floor(draw(0) * total / 2^64); e = the first env with prefix[e] > r;
 *   slot = (cursor[e] - count[e] + r - prefix[e-1]) mod T (prefix[-1] = 0): every valid transition is equally likely;
 *   gathered: obs, next_obs, actions, rewards, dones (the stored terminated as 0 / 1), env, slot;
 *   pad == 0: pixels <- obs_img[slot][e], next_pixels <- next_img[slot][e], byte for byte; shift[i] = (pad, pad, pad,
 *     pad) = 0: (pad, pad) is the shift that moves nothing.
 *   pad > 0, S = 2 pad + 1 (DrQ's random shift: replicate-pad by `pad`, crop at a random offset): the observation image
 *     takes h = draw(2), the next image h = draw(3) (independent), dx = ((h & 0xFFFFFFFF) * S) >> 32,
 *     dy = ((h >> 32) * S) >> 32, every plane of one image the same shift:
 *     out[p][y][x][ch] = in[p][clamp(y + dy - pad, 0, H - 1)][clamp(x + dx - pad, 0, W - 1)][ch];
 *     shift[i] = (dx, dy, dx', dy') (the next image's primed).
 * Every index read from meta or prefix is clamped into its range before it addresses memory.  Byte offsets into the image
 * arrays are 64-bit (T n P passes 2^32 at real sizes); no alignment of P or of any pointer is required. */
#define SO100_REPLAY_MAX_ACTION 16
#define SO100_REPLAY_MAX_PAD 64
typedef struct so100_replay {
  uint32_t size;            /* sizeof(so100_replay): the callee rejects a mismatch */
  int32_t  n;               /* envs, >= 0 */
  int32_t  T;               /* slots per env, >= 2, T * n < 2^31 */
  int32_t  action_dim;      /* floats per command, 1..SO100_REPLAY_MAX_ACTION */
  int32_t  planes, H, W, chan;  /* all 0 with P == 0, else all >= 1 and planes * H * W * chan == P < 2^31 */
  int32_t  P;               /* bytes per image row, >= 0 */
  int32_t  pad;             /* 0..SO100_REPLAY_MAX_PAD (sample; P == 0: 0) */
  uint64_t seed;            /* (sample) */
  float*   obs;             /* [T][n][15] */
  float*   next_obs;        /* [T][n][15] */
  float*   action;          /* [T][n][action_dim] */
  float*   reward;          /* [T][n] */
  uint8_t* terminated;      /* [T][n] */
  uint8_t* obs_img;         /* [T][n][P], NULL with P == 0 */
  uint8_t* next_img;        /* [T][n][P], NULL with P == 0 */
  int32_t* meta;            /* [2][n]: cursor, count */
  int32_t* prefix;          /* [n + 1] */
} so100_replay;
int so100_replay_bytes(void);
/* The inputs of one push: device rows of the n envs, as the step left them. */
typedef struct so100_replay_step {
  uint32_t size;                /* sizeof(so100_replay_step) */
  uint32_t reserved0;
  const float*   obs;           /* [n][15] */
  const float*   final_obs;     /* [n][15]: read where terminated | truncated */
  const float*   action;        /* [n][action_dim] */
  const float*   reward;        /* [n] */
  const uint8_t* terminated;    /* [n] */
  const uint8_t* truncated;     /* [n] */
  const uint8_t* diverged;      /* [n] or NULL */
  const uint8_t* pixels;        /* [n][P], NULL with P == 0 */
  const uint8_t* final_pixels;  /* [n][P]: read where terminated | truncated; NULL with P == 0 */
} so100_replay_step;
int so100_replay_step_bytes(void);
/* The outputs of one sample call: device arrays of `batch` rows. */
typedef struct so100_replay_out {
  uint32_t size;              /* sizeof(so100_replay_out) */
  uint32_t reserved0;
  float*   obs;               /* [B][15] */
  float*   next_obs;          /* [B][15] */
  float*   actions;           /* [B][action_dim] */
  float*   rewards;           /* [B] */
  float*   dones;             /* [B] */
  uint8_t* pixels;            /* [B][P], NULL with P == 0 */
  uint8_t* next_pixels;       /* [B][P], NULL with P == 0 */
  int32_t* env;               /* [B] */
  int32_t* slot;              /* [B] */
  int32_t* shift;             /* [B][4] */
} so100_replay_out;
int so100_replay_out_bytes(void);
/* Bytes of all the arrays of so100_replay together: T n (4 (15 + 15 + action_dim + 1) + 1 + 2 P) + 4 (2 n + n + 1), in
 * 64-bit arithmetic; -1 (text in so100_last_error) for n < 0, T < 2, T * n >= 2^31, an action_dim outside
 * 1..SO100_REPLAY_MAX_ACTION or P < 0. */
int64_t so100_replay_storage_bytes(int n, int T, int action_dim, int P);
/* All four: launches on `stream` (one each), no allocation, no synchronisation, no atomics; push and stage launch nothing
 * for n = 0, sample nothing for batch = 0.  Nonzero (text in so100_last_error) before any device work and with nothing
 * written, in this order: NULL replay, a wrong `size`, T < 2, n < 0, T * n >= 2^31, an action_dim outside
 * 1..SO100_REPLAY_MAX_ACTION, inconsistent planes / H / W / chan / P (P < 0; P == 0 with one of the four non-zero; P > 0
 * with one of them < 1 or their product not P), a pad outside 0..SO100_REPLAY_MAX_PAD or non-zero with P == 0, (sample)
 * batch < 0, NULL out or a wrong `size` of it, (push) NULL step or a wrong `size` of it; then a NULL env, a NULL required
 * array of so100_replay, image arrays of so100_replay present with P == 0 or absent with P > 0, a NULL required pointer of
 * step or out, image pointers of step or out present with P == 0 or absent with P > 0, (stage) the same for obs and
 * pixels. */
int so100_replay_push(so100_env* env, const so100_replay* replay, const so100_replay_step* step, void* stream);
int so100_replay_stage(so100_env* env, const so100_replay* replay, const uint8_t* mask /* [n] or NULL */,
                       const float* obs /* [n][15] */, const uint8_t* pixels /* [n][P], NULL with P == 0 */, void* stream);
int so100_replay_scan(so100_env* env, const so100_replay* replay, void* stream);
int so100_replay_sample(so100_env* env, const so100_replay* replay, int batch, uint64_t call, const so100_replay_out* out,
                        void* stream);

/* ---- (additions to ABI 25) n-step returns in the uniform replay buffer: the multi-step target of
 * DrQ-v2 (n = 3) and of SB3's off-policy `n_steps=`, gathered and summed by the sample launch.  Only the push and the
 * stage see where an episode ends (a truncation, a reset(mask) in mid-episode and a dropped step leave no trace in
 * so100_replay), so they record it: one more caller-owned array, `ends`, uint8 [T][n], slot-major, zero at the start,
 * named by so100_replay_nstep beside so100_replay.  ends[s][e] != 0: the transition in slot s of env e is the last one
 * that an n-step window may include from its episode.  Extra storage: T n bytes (so100_replay_nstep_storage_bytes).
 * Below n stays the number of envs; n_step, gamma and ends are the fields of so100_replay_nstep.
 *
 * so100_replay_push_nstep (one launch: so100_replay_push's kernel compiled with the extra pointer): rules 1-5 of
 *   so100_replay_push, and in the same workgroup, with c = cursor[e] and k = count[e] as read before the push:
 *   6. ends[c] <- (terminated[e] | truncated[e]) != 0, as 0 / 1.
 *   7. diverged[e] non-zero and k > 0: ends[(c - 1) mod T] <- 1: the episode was cut, its last stored transition closes
 *      it; the slot c is used again by the next episode.
 * so100_replay_stage_nstep (one launch): what so100_replay_stage does, and for every staged env with count[e] > 0:
 *   ends[(cursor[e] - 1) mod T] <- 1: a reset in mid-episode cuts the episode there (after a finished episode the byte
 *   is 1 already).
 * so100_replay_sample_nstep, batch element i (one launch: so100_replay_sample's kernel with the window compiled in; it
 *   reads prefix, so a scan must follow the last push):
 *   1. The pick is so100_replay_sample's: (e, slot s) from draw(0); kidx = r - prefix[e-1] is the index of s among env
 *      e's valid transitions, oldest = 0.  So for the same (seed, call, i) the outputs obs, actions, env, slot, shift
 *      and pixels are bit-equal to so100_replay_sample's, for every n_step.
 *   2. m = the smallest j in 1..n_step with j == n_step, or ends[(s + j - 1) mod T][e] != 0, or kidx + j == count[e]
 *      (the window has reached the newest stored transition; it never waits for a later push).
 *   3. In float32, each product rounded, then each sum (no fused multiply-add): R = reward[s][e], g = gamma; for
 *      j = 1..m-1: R = R + g * reward[(s + j) mod T][e], then g = g * gamma.  rewards[i] = R, discounts[i] = g (gamma
 *      for m = 1: the factor of the bootstrap value), nsteps[i] = m, last_slot[i] = (s + m - 1) mod T.
 *   4. next_obs, dones (the stored terminated) and next_pixels come from last_slot; ends is a superset of the terminated
 *      flags, so a terminal transition always closes its window.  The next image takes the shift of draw(3), as in
 *      so100_replay_sample.
 *   5. total == 0: the rows of so100_replay_sample's empty buffer, and nsteps[i] = 0, discounts[i] = 0,
 *      last_slot[i] = -1.
 *   6. n_step == 1 gives so100_replay_sample's outputs bit for bit (and discounts = gamma, nsteps = 1, last_slot = slot).
 *   Every index read from meta or prefix is clamped into its range before it addresses memory, and every window slot is
 *   taken mod T; the bytes of ends only stop a window.
 * The window costs one more round of loads, not n_step: lane j of a batch element's 16 lanes (of a wave, in the image
 * workgroups) reads ends and reward of slot s + j, whose addresses follow from s alone; a ballot gives m.  Hence
 * SO100_REPLAY_MAX_NSTEP = 16. */
#define SO100_REPLAY_MAX_NSTEP 16
typedef struct so100_replay_nstep {
  uint32_t size;            /* sizeof(so100_replay_nstep) */
  int32_t  n_step;          /* 1..min(SO100_REPLAY_MAX_NSTEP, T - 1) */
  float    gamma;           /* finite, in [0, 1] */
  uint32_t reserved0;
  uint8_t* ends;            /* [T][n] */
} so100_replay_nstep;
int so100_replay_nstep_bytes(void);
/* The additional outputs of one so100_replay_sample_nstep call: device arrays of `batch` rows. */
typedef struct so100_replay_nstep_out {
  uint32_t size;            /* sizeof(so100_replay_nstep_out) */
  uint32_t reserved0;
  float*   discounts;       /* [B]: gamma^m */
  int32_t* nsteps;          /* [B]: m */
  int32_t* last_slot;       /* [B] */
} so100_replay_nstep_out;
int so100_replay_nstep_out_bytes(void);
/* Bytes of `ends`: T n, in 64-bit arithmetic; -1 (text in so100_last_error) for n < 0, T < 2 or T * n >= 2^31.
 * so100_replay_storage_bytes does not count them. */
int64_t so100_replay_nstep_storage_bytes(int n, int T);
/* All three: as their namesakes above (one launch on `stream`, no allocation, no synchronisation, no atomics; nothing
 * launched for n = 0 or batch = 0), with the same refusals in the same order under their own names.  The refusals of
 * the n-step records sit in that order as follows.  After the numbers of so100_replay and the call's own records (batch,
 * out, step and their sizes) and before the NULL env: NULL nstep, a wrong `size` of it, an n_step outside
 * 1..min(SO100_REPLAY_MAX_NSTEP, T - 1), a gamma that is not finite or outside [0, 1] (all three calls check both
 * numbers), (sample) NULL nout or a wrong `size` of it.  After the arrays of so100_replay and before the pointers of step
 * or out: NULL ends.  Last: a NULL pointer of nout. */
int so100_replay_push_nstep(so100_env* env, const so100_replay* replay, const so100_replay_nstep* nstep,
                            const so100_replay_step* step, void* stream);
int so100_replay_stage_nstep(so100_env* env, const so100_replay* replay, const so100_replay_nstep* nstep,
                             const uint8_t* mask /* [n] or NULL */, const float* obs /* [n][15] */,
                             const uint8_t* pixels /* [n][P], NULL with P == 0 */, void* stream);
int so100_replay_sample_nstep(so100_env* env, const so100_replay* replay, const so100_replay_nstep* nstep, int batch,
                              uint64_t call, const so100_replay_out* out, const so100_replay_nstep_out* nout,
                              void* stream);

/* ---- (additions to ABI 25) prioritised replay in the uniform replay buffer: proportional
 * prioritisation (Schaul et al.), for the plain and the n-step buffer alike.  Only the pick changes: a transition is
 * drawn with probability q / total, q its priority.  Three more caller-owned arrays, named by so100_replay_per beside
 * so100_replay (and so100_replay_nstep); so100_replay, so100_replay_nstep, so100_replay_out and the entry points above
 * keep their meaning.
 *
 * Priorities are integers: uint32 fixed point, SO100_REPLAY_PRIO_ONE = 65536 is the priority 1.0.  A valid transition's
 * lies in 1 .. 2^32 - 1, every slot that holds none has 0.  Sums are uint64 (T n < 2^31 slots of < 2^32 stay below
 * 2^63): exact and associative, so a scan in any order gives the same bits.
 *   prio      uint32 [T][n], slot-major, zero at the start.  After every launch below: prio[s][e] > 0 exactly when slot s
 *             of env e is one of the env's count[e] valid transitions.
 *   sum       uint64 [n + 1]: sum[e] = the priorities of the envs 0..e, sum[n] = the total (so100_replay_per_scan).
 *   max_prio  uint32 [2], word 0 used, SO100_REPLAY_PRIO_ONE at the start: the greatest priority ever applied.
 *
 * so100_replay_push_per (one launch: so100_replay_push's kernel, or so100_replay_push_nstep's when nstep is given,
 *   compiled once more with the priorities): rules 1-5 (and 6, 7) of the push, and in the same workgroup, by the thread
 *   that writes the scalars, with c, c' the cursor before and after:
 *   8. a stored step: prio[c] <- max(max_prio[0], 1) (a new transition is drawn at least once soon), then prio[c'] <- 0:
 *      c' is now the staged slot; in a full ring it held the oldest transition, which thereby leaves the sum.
 *   9. a dropped step (diverged[e] non-zero): prio[c] <- 0.
 *   so100_replay_stage / so100_replay_stage_nstep move neither cursor nor count: they serve this buffer as they are.
 * so100_replay_per_scan (two launches: the per-env sums read T n words with the whole device, the scan over the envs
 *   is one workgroup's, and nothing in this file waits for another workgroup): sum as defined above, recomputed from
 *   prio every time.  so100_replay_scan stays the scan of the counts, which the weights need.
 * so100_replay_sample_per, batch element i (one launch: so100_replay_sample's kernel, or so100_replay_sample_nstep's,
 *   with this pick compiled in; it reads sum and prefix, so both scans must follow the last push or update):
 *   1. total = sum[n]; total == 0: the rows of so100_replay_sample's empty buffer (and of so100_replay_sample_nstep's),
 *      probs[i] = 0, weights[i] = 0.  Else
 *   2. r = floor(draw(0) * total / 2^64): the draw field of the plain pick, exactly uniform on [0, total).
 *   3. e = the first env with sum[e] > r (n - 1 if corrupted sums leave none).
 *   4. rr = r - sum[e-1] (sum[-1] = 0); the valid slots oldest first, k = 0 .. count[e] - 1 from (cursor[e] - count[e])
 *      mod T: the pick is the first k whose running sum of priorities exceeds rr; if corrupted sums leave none, the last
 *      valid slot (count[e] == 0, which only corrupted arrays reach: k = 0, the slot at the cursor).  q = its priority.
 *   5. Everything downstream (the gathered rows, the shifts, the n-step window from (slot, k, count[e])) is the plain
 *      sample's from that pick.  With all valid priorities equal the pick is the plain pick bit for bit:
 *      floor(floor(h c M / 2^64) / c) = floor(h M / 2^64).
 *   6. probs[i] = (float)((double)q / (double)total), both conversions and the division correctly rounded;
 *      weights[i] = powf((float)prefix[n] * probs[i], -beta) (prefix[n] the count of valid transitions), un-normalised
 *      (0 where q == 0).  The caller divides by the batch maximum.
 * so100_replay_per_update (two launches of one kernel), row j of `batch`, e = env_idx[j], s = slot_idx[j]:
 *   1. x = fmaxf(fabsf(td_abs[j]), 0) (a NaN counts as 0); q = rintf(powf(x + eps, alpha) * 65536) clamped into
 *      1 .. 2^32 - 1 (inf saturates), in float32.
 *   2. The row is ignored when e is outside 0..n-1, s outside 0..T-1 (the -1 of an empty-buffer row included), or s is
 *      not among env e's valid slots now: a transition evicted since the sample is skipped; a slot overwritten since
 *      takes the value.
 *   3. Sampling is with replacement, so a batch names the same slot more than once: the slot gets the greatest q
 *      written to it in the call.  The first launch stores 0 from every applied row, the second does an integer
 *      atomic maximum from every applied row.
 *   4. max_prio[0] <- max(max_prio[0], q) over the applied rows: one atomic per wave after a wave reduction.
 *   The integer maximum is commutative and associative: the result is a function of the inputs alone.  These are the
 *   library's only atomics; there are no float atomics.
 * Every index read from memory is clamped into its range before it addresses anything. */
#define SO100_REPLAY_PRIO_ONE 65536u
typedef struct so100_replay_per {
  uint32_t  size;           /* sizeof(so100_replay_per) */
  float     alpha;          /* (update) finite, in [0, 1] */
  float     beta;           /* (sample) finite, in [0, 1] */
  float     eps;            /* (update) finite, > 0 */
  uint32_t  reserved[2];
  uint32_t* prio;           /* [T][n] */
  uint64_t* sum;            /* [n + 1] */
  uint32_t* max_prio;       /* [2] */
} so100_replay_per;
int so100_replay_per_bytes(void);
/* The additional outputs of one so100_replay_sample_per call: device arrays of `batch` rows. */
typedef struct so100_replay_per_out {
  uint32_t size;            /* sizeof(so100_replay_per_out) */
  uint32_t reserved0;
  float*   probs;           /* [B]: q / total */
  float*   weights;         /* [B]: (count * probs)^-beta, un-normalised */
} so100_replay_per_out;
int so100_replay_per_out_bytes(void);
/* Bytes of prio, sum and max_prio together: 4 T n + 8 (n + 1) + 8, in 64-bit arithmetic; -1 (text in so100_last_error)
 * for n < 0, T < 2 or T * n >= 2^31.  so100_replay_storage_bytes does not count them. */
int64_t so100_replay_per_storage_bytes(int n, int T);
/* All four: launches on `stream`, no allocation, no synchronisation; nothing launched for n = 0 (push, update) or
 * batch = 0 (sample, update).  Nonzero (text in so100_last_error) before any device work and with nothing written, in
 * this order:
 *   1. the numbers of so100_replay, as so100_replay_push refuses them (NULL replay .. pad);
 *   2. NULL per, a wrong `size` of it;
 *   3. an alpha or a beta that is not finite or outside [0, 1];
 *   4. an eps that is not finite or <= 0;
 *   5. (nstep given) a wrong `size` of it, its n_step, its gamma, as so100_replay_push_nstep refuses them;
 *   6. (sample) nout without nstep, nstep without nout, a wrong `size` of nout;
 *   7. (sample) NULL pout, a wrong `size` of it;
 *   8. (push) NULL step or a wrong `size`; (sample) NULL out or a wrong `size`; (sample, update) batch < 0;
 *   9. a NULL env, the arrays of so100_replay as so100_replay_push refuses them, (nstep given) NULL ends, then NULL
 *      prio, sum or max_prio, then the pointers of step, out, nout and pout as their own calls refuse them, (update)
 *      NULL env_idx, slot_idx or td_abs. */
int so100_replay_push_per(so100_env* env, const so100_replay* replay, const so100_replay_per* per,
                          const so100_replay_nstep* nstep /* or NULL */, const so100_replay_step* step, void* stream);
int so100_replay_per_scan(so100_env* env, const so100_replay* replay, const so100_replay_per* per, void* stream);
int so100_replay_sample_per(so100_env* env, const so100_replay* replay, const so100_replay_per* per,
                            const so100_replay_nstep* nstep /* or NULL */, int batch, uint64_t call,
                            const so100_replay_out* out, const so100_replay_nstep_out* nout /* NULL without nstep */,
                            const so100_replay_per_out* pout, void* stream);
int so100_replay_per_update(so100_env* env, const so100_replay* replay, const so100_replay_per* per, int batch,
                            const int32_t* env_idx /* [B] */, const int32_t* slot_idx /* [B] */,
                            const float* td_abs /* [B] */, void* stream);

/* Batched sparse GoalEnv reward (env.py:341-353): out[i] = ||a_i - d_i|| < threshold ? 0 : -1. */
int so100_goal_reward(so100_env* env, int n, const float* achieved, const float* desired, float* out,
                      void* stream);

/* Task reward epilogue as a standalone op (for parity against the reference's golden vectors):
 * cube_site[n,3] fp32, ee_site[n,3] fp32, pair_bits[n] -> reward[n] fp32, using the same device
 * function as the step kernel. */
int so100_eval_reward(so100_env* env, int task, int n, const float* cube_site, const float* ee_site,
                      const uint32_t* pair_bits, float* reward, void* stream);

/* Reference spawn op: seeds[n] -> pose[n,7] (fp64) via device MT19937 (utils.py:18-29). */
int so100_spawn_pose(so100_env* env, int n, const uint32_t* seeds, double* pose, void* stream);

/* Action prologue as a standalone op: action[n,6] -> ctrl[n,6] (constants.py:78-86, fp32 write-back). */
int so100_unnormalize(so100_env* env, int n, const float* action, float* ctrl, void* stream);

#ifdef __cplusplus
}
#endif
#endif
