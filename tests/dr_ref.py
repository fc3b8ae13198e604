"""Host restatements of the build-defined parts of the step kernel (TEST INFRASTRUCTURE, numpy only): the
per-env model of a domain-randomised env, the counter-based hashes of the in-kernel resets and the action
noise (csrc/so100_task.h splitmix64 / episode_seed / hash_uniform / hash_normal), the action-noise key
(csrc/so100_step.hip set_controls) and the GoalEnv goal sampler (final_stage and so100_reset_kernel).

Integers are np.uint64 with wrapping arithmetic, reals float64: the device's fp32 values are reproduced where
the kernel holds an fp32 value (hash_uniform's 24 bits are exact in both), and evaluated in float64 where it
computes (log, sqrt, cos, lo + (hi - lo) * u), so a comparison carries the device's rounding alone.
"""
import numpy as np

from gym_so100.model import NPAIR, SO100Model

CUBE_BODY = 8
_U = np.uint64


def _u64(x):
    """x (python int of any sign/size, or an integer array) as np.uint64 modulo 2^64"""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return _U(int(x) & 0xFFFFFFFFFFFFFFFF)


def scaled_model(model, mscale, fscale):
    """The model of a domain-randomised env: a copy of `model` with the cube's body_mass and body_inertia times
    mscale and pair_friction (all three coefficients) times fscale on every pair that holds the cube.

    Everything else stays, body_invweight0 included: the device scales the cube's mass, inertia and friction where
    the dynamics and the constraint rows read them and keeps the contact rows' regularisation (pair_tran / pair_rot,
    from body_invweight0) of the unscaled model.  This is what MuJoCo computes when body_mass / geom_friction are
    edited in place without a call of mj_setConst."""
    m = SO100Model.from_buffer_copy(model)
    ms, fs = float(mscale), float(fscale)
    m.body_mass[CUBE_BODY] *= ms
    for k in range(3):
        m.body_inertia[CUBE_BODY][k] *= ms
    for p in range(NPAIR):
        if m.pair_body1[p] == CUBE_BODY or m.pair_body2[p] == CUBE_BODY:
            for k in range(3):
                m.pair_friction[p][k] *= fs
    return m


def splitmix64(x):
    x = _u64(x)
    with np.errstate(over="ignore"):
        x = x + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def episode_seed(base, env, episode):
    """the RandomState seed (uint32) of global env `env`'s episode `episode` (so100_task.h episode_seed)"""
    inner = splitmix64((_u64(env) << _U(32)) | _u64(episode))
    return splitmix64(_u64(base) ^ inner) & _U(0xFFFFFFFF)


def hash_uniform(key):
    """U[0, 1) on the 2^-24 grid: exact in fp32 and in float64"""
    return (splitmix64(key) >> _U(40)).astype(np.float64) / 16777216.0


def hash_normal(key):
    """Box-Muller on two hash_uniform draws; u1 is floored at fp32(1e-7) as the kernel does (hash_uniform can
    return 0), so |hash_normal| <= sqrt(-2 ln 1e-7) = 5.68"""
    key = _u64(key)
    u1 = np.maximum(hash_uniform(key), np.float64(np.float32(1e-7)))
    u2 = hash_uniform(key ^ _U(0xA5A5A5A5A5A5A5A5))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def action_noise_key(base_seed, global_env, episode, elapsed, lane):
    """The key set_controls hashes: env in bits 40.., episode in bits 20..39, elapsed * 8 + lane below.  Keys alias
    once elapsed reaches 2^17 or episode 2^20 (a property of the layout, far past any episode length here)."""
    k = (_u64(base_seed) ^ (_u64(global_env) << _U(40)) ^ (_u64(episode) << _U(20)) ^
         _u64(np.asarray(elapsed) * 8 + np.asarray(lane)))
    return splitmix64(k)


def action_noise(base_seed, global_env, episode, elapsed, lane):
    """The unit normal the kernel adds (times sigma) to action component `lane` of global env `global_env` at step
    `elapsed` (before the step's increment) of episode `episode`."""
    return hash_normal(action_noise_key(base_seed, global_env, episode, elapsed, lane))


def goal_box(spawn_xy, total_steps, model):
    """(lo, hi) [3] of the box a goal is drawn from, the kernel's fp32 values as float64: below 5000 total steps
    +-0.03 around the spawn's xy and z in [0.01, 0.05] (the lifted-goal curriculum), from 5000 on the bin box
    (model.goal_bin_lo / hi)."""
    f32 = np.float32
    if int(total_steps) < 5000:
        c = np.asarray(spawn_xy, np.float64).astype(f32)
        lo = np.array([c[0] - f32(0.03), c[1] - f32(0.03), f32(0.01)], f32)
        hi = np.array([c[0] + f32(0.03), c[1] + f32(0.03), f32(0.05)], f32)
    else:
        lo = np.array(model.goal_bin_lo[:], np.float64).astype(f32)
        hi = np.array(model.goal_bin_hi[:], np.float64).astype(f32)
    return lo.astype(np.float64), hi.astype(np.float64)


def goal_sample(base_seed, global_env, episode, spawn_xy, total_steps, model):
    """GoalEnv's desired goal [3] of global env `global_env`'s episode `episode`: the float64 value of
    lo + (hi - lo) * u with lo, hi (goal_box) and u as the kernel's fp32 values.  total_steps is the env's step count
    when the goal is sampled: after the terminal step's increment for an auto-reset."""
    with np.errstate(over="ignore"):
        key = _u64(base_seed) * _U(31) + (_u64(global_env) << _U(24)) + _u64(episode) * _U(3) + np.arange(3, dtype=np.uint64)
    u = hash_uniform(splitmix64(key))
    lo, hi = goal_box(spawn_xy, total_steps, model)
    return lo + (hi - lo) * u


# ------------------------------------------------------------------ state recipes of the DR parity classes
# (shared by tests/test_gpu_dr.py, which steps them on the GPU, and tests/test_dr_ref_cpu.py, which measures on the
# oracle alone how far a wrong DR model moves the result)
CORNERS = ((0.8, 1.2), (1.2, 0.8))     # (mass scale, friction scale): the corners of the DR ranges that differ most


def sliding_cube_state(oracle64, model, seed):
    """(qpos, qvel, qacc_warmstart) of a sliding, tumbling cube: the RandomState(seed) spawn settled on the table by
    the fp64 oracle (30 zero-action env steps on `model`), then 0.3 m/s tangential velocity in a random direction and
    an angular velocity of N(0, 3 rad/s) per axis."""
    d = oracle64.new_data()
    oracle64.reset(model, d, oracle64.spawn_pose(seed))
    zero = np.zeros(6, np.float32)
    for _ in range(30):
        oracle64.env_step(model, d, 0, zero)
    q, v, w, _ = oracle64.get_state(d)
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, 2 * np.pi)
    v = v.copy()
    v[6:9] = [0.3 * np.cos(th), 0.3 * np.sin(th), 0.0]
    v[9:12] = rng.normal(0, 3.0, 3)
    return q, v, w


def bin_corner_states(model, n, rng):
    """(qpos, qvel) [n, 13] / [n, 12] float64 of the cube pressed into a bin corner (the floor and two walls, up to 12
    contacts): tests/test_gpu_parity.py test_heavy_contact_parity's recipe, the arm at its start pose."""
    qpos = np.zeros((n, 13))
    qpos[:, :6] = np.array(model.start_qpos[:], np.float64).astype(np.float32)
    pen = rng.uniform(2e-4, 1e-3, (n, 3))
    # bin inner faces (assets: bin_wall3 x = -0.14 - 0.005, bin_wall y = 0.76 - 0.005, floor top z = 0.001)
    qpos[:, 6] = -0.145 - 0.02 + pen[:, 0]
    qpos[:, 7] = 0.755 - 0.02 + pen[:, 1]
    qpos[:, 8] = 0.001 + 0.02 - pen[:, 2]
    ang = rng.uniform(-0.01, 0.01, n)
    qpos[:, 9:13] = np.stack([np.cos(ang / 2), np.zeros(n), np.zeros(n), np.sin(ang / 2)], 1)
    qvel = np.zeros((n, 12))
    qvel[:, 6:9] = rng.normal(0, 0.02, (n, 3))
    return qpos.astype(np.float32).astype(np.float64), qvel.astype(np.float32).astype(np.float64)


def rel_dist(a, o):
    """max |a - o| / (1 + |o|): the parity tests' relative distance of a qvel / qacc vector from the oracle's"""
    return (np.abs(np.asarray(a) - np.asarray(o)) / (1 + np.abs(np.asarray(o)))).max()


def force_dist(f, fo, floor=1e-3):
    """per-contact relative force distance ||f - fo|| / max(||fo||, floor) (floor in N: the cube weighs 0.49 N)"""
    return np.linalg.norm(f - fo, axis=1) / np.maximum(np.linalg.norm(fo, axis=1), floor)


def oracle_step(oracle, model, state, action, task=0, mocap=None):
    """One env step of `oracle` on `model` from state (qpos, qvel, warmstart): (qpos, qvel, last_solve record)."""
    d = oracle.new_data()
    oracle.set_state(d, state[0], state[1], state[2])
    if mocap is not None:
        for k in range(3):
            d.mocap_pos[k] = float(mocap[k])
        for k in range(4):
            d.mocap_quat[k] = float(mocap[3 + k])
    oracle.env_step(model, d, task, np.asarray(action, np.float32))
    q, v = oracle.get_state(d)[:2]
    return q, v, oracle.last_solve(d)
