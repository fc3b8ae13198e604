"""Batched SO-ARM100 envs on one MI355X: torch-ROCm tensors in, torch-ROCm tensors out.

``SO100VecEnv`` is the batched form of the reference's ``SO100Env`` (gym_so100/env.py:26-185) and
``SO100GoalEnv`` (env.py:188-409): N independent envs stepped by one HIP launch per env step
(csrc/so100_step.hip).  Semantics kept from the reference:

* actions [N,6] in [-1,1], un-normalised per joint with float32 write-back (single_arm.py:33-38);
* 10 physics substeps per env step (control_timestep 0.02 / timestep 0.002, env.py:120-127);
* reward ladders of the three tasks (single_arm.py), ``terminated = is_success = reward == 4``
  (env.py:175), TimeLimit truncation at 700 / 300 steps (gym_so100/__init__.py:7,17,27);
* so100_state observation = [box, bin, ee, qpos[:6]] float32 (env.py:137-145);
* so100_pixels_agent_pos observation = {"pixels": top camera uint8 [N,H,W,3], "agent_pos": qpos[:6]}
  (env.py:130-136), rendered on the device by render.CameraRenderer (csrc/so100_render.hip);
* GoalEnv: sparse reward 0/-1 at 0.01 m, terminated = success, own 300-step truncation, lifted-goal
  curriculum for the first 5000 steps (env.py:322-353, 372-406);
* reset(seed=s) reproduces ``RandomState(s)`` cube spawns bit-for-bit (utils.py:18-29).

Auto-reset follows the SB3/gymnasium-vector convention: when an env finishes, ``obs`` already holds
the first observation of the next episode and ``info["final_observation"]`` the last one of the
finished episode (mask in ``info["_final_observation"]``).

With pixel observations an env that finishes is stepped, its terminal image drawn into
``final_pixels``, then reset by the masked reset kernel (the same spawn and episode counter as the
in-kernel auto-reset) and drawn again: ``info["final_observation"]`` is then {"pixels", "agent_pos"}.

Output tensors are persistent device buffers overwritten by the next ``step``/``reset``; clone them if
you keep them across calls.
"""
import ctypes

import numpy as np

from . import _native
from .model import NOBS, NQ, NV, build_model
from .constants import GOAL_MAX_EPISODE_STEPS
from .normalize import Normalizer, merge_normalize_states, normalize_options  # noqa: F401  (re-exported)
from .replay import HerReplay, UniformReplay, replay_options, uniform_replay_options

_MAX_STEPS = {"so100_cube_to_bin": 700, "so100_touch_cube": 300, "so100_touch_cube_sparse": 300,
              "so100_goal": GOAL_MAX_EPISODE_STEPS}


def _torch():
    import torch
    return torch


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _hash_uniform(seed, ids, field):
    """U[0,1) per global env id from a counter-based hash (splitmix64), independent of sharding."""
    with np.errstate(over="ignore"):
        key = _splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ (ids * np.uint64(0x100000001B3)) ^
                          np.uint64(field * 0xD1B54A32D192ED03 & 0xFFFFFFFFFFFFFFFF))
    return (key >> np.uint64(40)).astype(np.float64) / float(1 << 24)


# so100_ee_ctrl's defaults (include/so100.h): pos_scale and rot_scale are the key steps of the reference's
# scripts/teleop_ee.py:53-64 (0.01 m, 10 degrees)
EE_CONTROL_DEFAULTS = {"iters": 2, "pos_scale": 0.01, "rot_scale": 0.17453292, "damping": 0.02, "dq_max": 0.2,
                       "lead_max": 0.5}
ACTION_MODES = ("joint", "ee_delta")


def ee_control_options(control, model=None):
    """The checked control record of action_mode="ee_delta" as a dict (no device use): EE_CONTROL_DEFAULTS overridden
    by `control`; with `model` the workspace box defaults to the table's x / y extent and z in [0, 0.6].  Raises
    ValueError for what so100_ee_action refuses."""
    c = dict(EE_CONTROL_DEFAULTS)
    control = {} if control is None else control
    if not isinstance(control, dict):
        raise ValueError("ee_control: None or a dict")
    unknown = set(control) - set(c) - {"ws_lo", "ws_hi"}
    if unknown:
        raise ValueError(f"ee_control: unknown keys {sorted(unknown)}; known: {sorted(c) + ['ws_lo', 'ws_hi']}")
    c.update(control)
    if isinstance(c["iters"], bool) or not isinstance(c["iters"], (int, np.integer)) or not 1 <= c["iters"] <= 8:
        raise ValueError(f"ee_control: iters {c['iters']!r} outside 1..8")
    for k in ("pos_scale", "rot_scale", "damping", "dq_max", "lead_max"):
        try:
            v = float(c[k])
        except (TypeError, ValueError):
            raise ValueError(f"ee_control: {k} {c[k]!r} is not a number") from None
        if not np.isfinite(v) or v < 0 or (v == 0 and k != "rot_scale"):
            raise ValueError(f"ee_control: {k} {v!r} must be finite and {'>= 0' if k == 'rot_scale' else '> 0'}")
        c[k] = v
    if model is not None:
        c.setdefault("ws_lo", (float(model.table_lo[0]), float(model.table_lo[1]), 0.0))
        c.setdefault("ws_hi", (float(model.table_hi[0]), float(model.table_hi[1]), 0.6))
    for k in ("ws_lo", "ws_hi"):
        if k in c:
            try:
                v = tuple(float(x) for x in c[k])
            except (TypeError, ValueError):
                raise ValueError(f"ee_control: {k} {c[k]!r} is not three numbers") from None
            if len(v) != 3 or not all(np.isfinite(v)):
                raise ValueError(f"ee_control: {k} {c[k]!r} is not three finite numbers")
            c[k] = v
    if "ws_lo" in c and "ws_hi" in c and any(lo > hi for lo, hi in zip(c["ws_lo"], c["ws_hi"])):
        raise ValueError(f"ee_control: workspace box inverted: ws_lo {c['ws_lo']} > ws_hi {c['ws_hi']}")
    return c


# the actuation model's ranges with the model off (include/so100.h so100_dr_ranges): no delay, alpha = 1, no slew limit
ACTUATION_OFF = {"delay": (0, 0), "smoothing": (1.0, 1.0), "rate": (2.0, 2.0)}
ACT_MAX_DELAY = 7                  # SO100_ACT_MAX_DELAY


def _real_range(what, value, upper=None):
    """(lo, hi) floats of a range argument; ValueError for what so100_dr_sample refuses"""
    try:
        lo, hi = (float(x) for x in value)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {value!r} is not a (lo, hi) pair of numbers") from None
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo <= 0 or lo > hi or (upper is not None and hi > upper):
        raise ValueError(f"{what}: {value!r} must be finite with 0 < lo <= hi" + ("" if upper is None else f" <= {upper}"))
    return lo, hi


def actuation_options(actuation):
    """The checked ranges of domain_randomization["actuation"] as a dict (no device use): ACTUATION_OFF overridden by
    `actuation`.  Raises ValueError for unknown keys and for what so100_dr_sample refuses."""
    if not isinstance(actuation, dict):
        raise ValueError("actuation: a dict(delay=(lo, hi), smoothing=(lo, hi), rate=(lo, hi))")
    unknown = set(actuation) - set(ACTUATION_OFF)
    if unknown:
        raise ValueError(f"actuation: unknown keys {sorted(unknown)}; known: {sorted(ACTUATION_OFF)}")
    a = dict(ACTUATION_OFF)
    a.update(actuation)
    try:
        lo, hi = a["delay"]
    except (TypeError, ValueError):
        raise ValueError(f"actuation: delay {a['delay']!r} is not a (lo, hi) pair") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"actuation: delay {a['delay']!r} must be whole control steps")
    if lo < 0 or hi > ACT_MAX_DELAY or lo > hi:
        raise ValueError(f"actuation: delay {a['delay']!r} must lie in 0..{ACT_MAX_DELAY} with lo <= hi")
    return {"delay": (int(lo), int(hi)), "smoothing": _real_range("actuation: smoothing", a["smoothing"], upper=1.0),
            "rate": _real_range("actuation: rate", a["rate"])}


def physical_dr_options(dr, variant="joint"):
    """The argument checks of a domain_randomization dict's per_episode / actuation keys (no device use): ValueError for
    what so100_dr_sample would refuse and for an actuation model on variant="ee".  The other keys are checked as they
    always were."""
    if not dr:
        return
    if dr.get("actuation") is not None:
        if variant == "ee":
            raise ValueError("domain_randomization['actuation'] models the joint command's latency; variant='ee' takes "
                             "its mocap pose (set_mocap)")
        actuation_options(dr["actuation"])
    if dr.get("per_episode"):
        _real_range("domain_randomization: mass", dr.get("mass", (0.8, 1.2)))
        _real_range("domain_randomization: friction", dr.get("friction", (0.8, 1.2)))


class NormalizeOffError(AttributeError, ValueError):
    """The normalisation attributes of an env built without normalize=...: a ValueError for callers, an AttributeError
    so that ``hasattr(env, "obs_rms")`` is False."""


class SO100VecEnv:
    """N parallel SO-ARM100 envs on one GPU.

    Args:
        num_envs: number of envs on this device.
        task: "so100_cube_to_bin" | "so100_touch_cube" | "so100_touch_cube_sparse" | "so100_goal".
        obs_type: "so100_state" (15 floats) or "so100_pixels_agent_pos" (the reference's registered
            default: top-camera image + joint positions; GoalEnv: the flattened form of env.py:267-270).
        observation_width, observation_height: image size for pixel observations (env.py:34-35).
        variant: "joint" (so100_transfer_cube.xml, the registered envs) or "ee" (so100_transfer_cube_ee.xml:
            a weld equality pulls ee_site to each env's mocap pose ``self.mocap`` [N,7], set with
            ``set_mocap``; teleop_ee.py drives the same inputs).
        device: torch device string ("cuda:0").
        seed: base seed for in-kernel (auto-)reset spawns.
        max_episode_steps: TimeLimit; default per task as registered by the reference.
        autoreset: reset finished envs inside the step kernel.
        domain_randomization: None or dict(mass=(lo,hi), friction=(lo,hi), action_noise=sigma):
            per-env cube mass / friction scales (fixed per env) + Gaussian action noise.  With pixel observations
            the dict may carry ``visual=dict(...)``: camera jitter, light and colour randomisation per env
            (``set_domain_randomization``); ValueError with any other obs_type.  Two more keys, both off by default:
            ``per_episode=True`` draws mass and friction on the device (csrc/so100_dr.hip) from each env's episode
            counter, again whenever an env is reset, by ``reset`` or by auto-reset, with no host synchronisation;
            ``actuation=dict(delay=(lo,hi), smoothing=(lo,hi), rate=(lo,hi))`` puts an actuator model between the
            command and the step (csrc/so100_act.hip, include/so100.h so100_actuate): per env a delay of whole control
            steps (0..7), a first-order smoothing factor and a slew limit per control step, drawn per env (per episode
            with ``per_episode``) into ``act_params`` [N,4]; ``actions`` then holds the applied action, and an
            ``action_mode="ee_delta"`` command passes EE prologue -> actuator -> step.  ValueError with variant="ee".
        env_offset: global index of this shard's first env (multi-GPU sharding); in-kernel seeds use
            the global env id so trajectories do not depend on the number of GPUs.
        iterations: solver iterations per substep, PGS sweeps or Newton steps (default: the model's 100,
            MuJoCo's default).
        solver: "newton" (default: MuJoCo's default solver, which the reference's model runs; the
            unique minimiser of the constraint problem) or "pgs" (north_star's projected Gauss-Seidel).
        debug: allocate the [N, 160] diagnostics buffer (contacts, forces, solver iterations; layout:
            include/so100.h SO100_DBG_STRIDE).  While it is passed (``debug_enabled``, default True) the
            fused step launches its debug build; set ``debug_enabled = False`` to run the product build.
        reward64: also keep the reward in float64 (``self.reward64``), as the reference returns it; the
            float32 ``reward`` rounds the dense TouchCube shaping (the other ladders are exact in float32).
        convex: the collider of the mesh pairs (the cube, bin boxes and finger pads against the link hulls, the
            links against each other and the Base): "epa" (default: GJK + EPA, MuJoCo 3.3.3's default native
            convex collider: the minimum penetration) or "mpr" (libccd's MPR, MuJoCo's mjDSBL_NATIVECCD path).
        episode_stats: keep device-side episode statistics (RecordEpisodeStatistics): the running float64
            return ``ep_return`` [N], the last finished episode's (return, length) ``ep_final`` [N,2] and the
            per-env totals ``ep_accum`` [N,4] (episodes, successes, sum of returns, sum of lengths), written
            by the step kernel's epilogue; ``info["episode"]`` then carries r / l of the envs that finished
            (mask ``info["_episode"]``), and ``episode_statistics()`` reduces the totals on demand.
        nsubstep: physics substeps per env step (default: the reference's 10, control_timestep / timestep);
            1 makes an env step one mj_step + the final mj_step1 (the parity tests' per-substep checks).
        channels_first: pixel observations only: ``pixels``, ``final_pixels`` and
            ``info["final_observation"]["pixels"]`` are [N,3,H,W], the layout SB3's image policies take, written
            by the render kernel itself (no transpose pass).  ValueError with task="so100_goal", whose flattened
            observation is the reference's HWC order.
        flat_pixels: pixel observations only: keep ``pixels_flat``, a persistent float32 [N, 3HW+6] tensor:
            every full render fills its image part (the [H,W,3] bytes / 255 as numpy divides them, env.py:267-270)
            in the launch that fills ``pixels``, and reset / step copy agent_pos into its last six columns.  The
            GoalEnv then returns it as ``"observation"`` (the same tensor every call, overwritten by the next step);
            without the flag that observation is built by torch on every call.
        depth, segmentation: pixel observations only: the observation dict gains ``"depth"`` (float32 [N,H,W], metres
            along the camera's viewing axis, background 0) and / or ``"segmentation"`` (uint8 [N,H,W], the classes of
            render.segment_labels, background render.SEG_BACKGROUND), what dm_control's physics.render(depth=True /
            segmentation=True) returns, drawn by the launch that draws ``pixels``.  With auto-reset ``final_depth`` /
            ``final_segmentation`` ride in ``info["final_observation"]`` beside ``final_pixels``.  The GoalEnv's
            flattened ``"observation"`` stays as it is; the two tensors are further keys of its dict.  ValueError with
            any other obs_type.
        cameras: None (default: the ``top`` camera, every call what it is without the argument) or a tuple of 1..4 names
            of render.CAMERAS / render.MOUNTED_CAMERAS, e.g. ("top", "left_wrist"): pixel observations only (ValueError
            otherwise).  ``pixels`` is then the one [N,K,H,W,3] tensor (channels_first: [N,K,3,H,W]) of K cameras drawn
            by one launch (render.MultiCameraRenderer), ``camera_names`` names its K axis, ``depth`` / ``segmentation``
            and the three ``final_*`` tensors gain the K axis, ``pixels_flat`` is [N, K*3HW+6] (camera c's image / 255
            in floats [c*3HW, (c+1)*3HW), agent_pos last) and domain_randomization["visual"] draws a view per camera.
        shadows: pixel observations only (ValueError otherwise): True or a dict (render.SHADOW_KEYS) makes the scene's
            shadow-casting light cast hard shadows in ``pixels``, ``final_pixels`` and ``pixels_flat``, drawn by the
            one render launch (render.CameraRenderer(shadows=...)); with visual randomisation ``light_rot_deg`` moves
            them per env.  Physics, depth and segmentation are untouched.  The default False changes no call.
        antialias: pixel observations only (ValueError otherwise): True (4 samples), 2, 4 or a dict
            (render.AA_KEYS): ``pixels``, ``final_pixels``, ``pixels_flat`` and masked renders are drawn with that many
            coverage samples per pixel, resolved inside the render launch (render.CameraRenderer(antialias=...)).
            ``depth`` / ``segmentation`` stay what they are without it, drawn by a second launch.  Not together with
            shadows.  The default False changes no call.
        action_mode: "joint" (default: six normalised joint targets, every call what it is without the argument) or
            "ee_delta": a Cartesian action a = (dx, dy, dz, droll, grip) in [-1,1]^5 on the joint model: each step a HIP
            prologue (csrc/so100_ee.hip, include/so100.h so100_ee_action) moves an end-effector target by
            pos_scale * a[0:3] metres, solves the four positioning joints for it by damped least squares, turns the wrist
            by rot_scale * a[3] and writes the six joint actions into ``actions``, which the unchanged step then takes;
            a[4] is the gripper's joint-mode command.  ``action_dim`` is 5, ``step`` / ``set_action_buffer`` take [N,5],
            ``ee_joint_target`` [N,5] is the commanded joint targets (radians) the next delta starts from,
            ``ee_target`` [N,3] the last position target and ``reinit`` [N] uint8 marks the envs whose command is
            seeded from their measured pose at the next step (set by ``reset`` and, with auto-reset, for the envs that
            finished).  ValueError with variant="ee", which has its mocap input (``set_mocap``).
        ee_control: None or a dict overriding EE_CONTROL_DEFAULTS (iters, pos_scale, rot_scale, damping, dq_max,
            lead_max, ws_lo, ws_hi; the workspace box defaults to the table's x / y extent and z in [0, 0.6]); unknown
            keys and out-of-range values raise ValueError before any device use.  action_mode="ee_delta" only.
        normalize: None (default: every call what it is without the argument), True or a dict overriding
            normalize.NORMALIZE_DEFAULTS (obs, reward, clip_obs, clip_reward, gamma, epsilon, training): SB3
            VecNormalize's running normalisation, on the device (csrc/so100_norm.hip, include/so100.h
            so100_norm_update).  True is the reference scripts' setting: observations on, rewards off,
            clip 10.  Running float64 mean / variance / count per column, updated after every ``step`` / ``reset`` with
            the observations returned (while ``training``), with no host synchronisation.  ``step`` / ``reset`` then
            return the normalised observation (state env: ``obs_norm`` [N,15]; GoalEnv: ``observation``,
            ``achieved_goal`` and ``desired_goal``, one set of statistics each; pixel observations: ``agent_pos`` only,
            images are never touched) and, with ``reward=True``, ``reward_norm`` = clip(reward / sqrt(var of the
            discounted return)); ``info["final_observation"]`` is normalised with the same statistics and never enters
            them.  The raw tensors (``obs``, ``reward``, ``final_obs``, ``achieved_goal``, ``desired_goal``) stay what
            they are.  ``training`` (settable), ``obs_rms``, ``ret_rms``, ``normalize_obs``, ``unnormalize_obs``,
            ``normalize_state`` and ``set_normalize_state`` below.  ValueError for unknown keys and bad values, and for
            the GoalEnv's flattened pixel observation (thousands of columns: not normalised).
        replay: None (default: every call what it is without the argument, ``replay`` is None) or a dict overriding
            replay.REPLAY_DEFAULTS (buffer_size, n_sampled_goal, goal_selection_strategy, seed): SB3
            HerReplayBuffer's storage and hindsight relabelling, on the device (csrc/so100_her.hip, include/so100.h
            so100_her_push).  ``buffer_size // num_envs`` slots per env; every ``step`` stores one
            transition per env (the raw observation, the true next observation, the goal, the command as passed in, the
            reward, ``terminated``) with no host synchronisation, ``reset`` drops the open episodes of the envs it
            resets, a diverged episode is erased, and ``replay.sample(batch_size)`` draws from the finished episodes.
            ``step_async_raw`` stores nothing.  ValueError for unknown keys and bad values, and unless
            task="so100_goal", obs_type="so100_state", autoreset=True and buffer_size // num_envs >= max_episode_steps.
        uniform_replay: None (default: every call what it is without the argument, ``uniform_replay`` is None) or a
            dict overriding replay.UNIFORM_REPLAY_DEFAULTS (buffer_size, augment, seed): SB3 DictReplayBuffer's storage
            for the arm tasks, on the device (csrc/so100_replay.hip, include/so100.h so100_replay_push; DESIGN.md
            §3.12), for both observation types.  ``buffer_size // num_envs`` slots per env, one of which holds the
            staged observation; every ``step`` stores one transition per env (the raw 15-float observation and the true
            next one, with pixel observations both images as ``pixels`` holds them, the command as passed in, the reward,
            ``terminated``) with no host synchronisation, ``reset`` stages the fresh observations, a diverged step is
            dropped, and ``uniform_replay.sample(batch_size)`` draws uniformly.  ``augment`` (None / False, True = pad 4,
            an int pad, dict(pad=)): DrQ's random shift of the two sampled images, in the sample launch.  Depth and
            segmentation images are not stored.  ``step_async_raw`` stores nothing.  ValueError for unknown keys and bad
            values, for task="so100_goal" (``replay=`` is its buffer), autoreset=False, buffer_size // num_envs < 2 and
            ``augment`` without pixel observations.  ``n_step`` (1..16, at most the slots per env - 1) with ``gamma``
            (default 0.99) turns on n-step returns: push and reset then also record where episodes
            end (a done, a ``reset(mask)`` in mid-episode, a dropped step), and ``sample`` sums the discounted rewards
            over a window that stays within one episode and gains the keys ``discounts``, ``n_steps`` and
            ``last_slot``.  Without the key nothing changes.  ``prioritized`` (None / False, True = alpha 0.6, beta
            0.4, eps 1e-6, or dict(alpha=, beta=, eps=)) turns on proportional prioritised replay: a
            new transition takes the greatest priority so far, ``sample`` draws in proportion to the priorities and
            gains ``probs`` and ``weights``, and ``uniform_replay.update_priorities(env, slot, td_abs)`` sets them from
            |TD error|.  It composes with ``n_step``; without the key nothing changes.
    """

    def __init__(self, num_envs, task="so100_cube_to_bin", obs_type="so100_state", device="cuda:0", seed=0,
                 max_episode_steps=None, autoreset=True, domain_randomization=None, env_offset=0,
                 iterations=None, debug=False, solver="newton", observation_width=640, observation_height=480,
                 variant="joint", reward64=False, nsubstep=None, convex="epa", episode_stats=False, channels_first=False,
                 flat_pixels=False, depth=False, segmentation=False, cameras=None, shadows=False,
                 antialias=False, action_mode="joint", ee_control=None, normalize=None, replay=None,
                 uniform_replay=None):
        torch = _torch()
        norm_options = normalize_options(normalize)      # its ValueErrors before any device work
        replay_opts = replay_options(replay, num_envs, task, obs_type, autoreset,
                                     _MAX_STEPS.get(task) if max_episode_steps is None else max_episode_steps)
        uniform_opts = uniform_replay_options(uniform_replay, num_envs, task, obs_type, autoreset)
        if norm_options is not None and norm_options["obs"] and task == "so100_goal" \
                and obs_type == "so100_pixels_agent_pos":
            raise ValueError("normalize: the GoalEnv's flattened pixel observation ([N, 3HW+6]) is not normalised; use "
                             "normalize=dict(obs=False, ...) or the state observation")
        if action_mode not in ACTION_MODES:
            raise ValueError(f"action_mode {action_mode!r}: one of {ACTION_MODES}")
        if action_mode == "ee_delta":
            if variant == "ee":
                raise ValueError("action_mode='ee_delta' is an action mode of the joint model; variant='ee' takes its "
                                 "mocap pose (set_mocap)")
            ee_control_options(ee_control)               # its ValueErrors before any device work
        elif ee_control is not None:
            raise ValueError("ee_control needs action_mode='ee_delta'")
        if obs_type not in ("so100_state", "so100_pixels_agent_pos"):
            raise NotImplementedError(f"obs_type={obs_type!r}: 'so100_state' or 'so100_pixels_agent_pos'")
        if task not in _native.TASKS:
            raise NotImplementedError(task)    # env.py:117-118
        if channels_first and task == "so100_goal":
            raise ValueError("channels_first: the GoalEnv's flattened pixel observation is HWC (env.py:267-270)")
        if (channels_first or flat_pixels) and obs_type != "so100_pixels_agent_pos":
            raise ValueError("channels_first / flat_pixels need obs_type='so100_pixels_agent_pos'")
        if (depth or segmentation) and obs_type != "so100_pixels_agent_pos":
            raise ValueError("depth / segmentation need obs_type='so100_pixels_agent_pos'")
        if shadows:
            from .render import load_scene, shadow_options
            if obs_type != "so100_pixels_agent_pos":
                raise ValueError("shadows need obs_type='so100_pixels_agent_pos'")
            shadow_options(load_scene(), shadows)      # its ValueErrors before any device work
        if antialias:
            from .render import antialias_options
            if obs_type != "so100_pixels_agent_pos":
                raise ValueError("antialias needs obs_type='so100_pixels_agent_pos'")
            if shadows:
                raise ValueError("antialias with shadows: the two key arrays times the samples do not fit the band "
                                 "in LDS")
            aa = antialias_options(antialias)            # its ValueErrors before any device work
            if aa is not None and int(observation_width) * aa.samples > 4096:
                raise ValueError(f"antialias: width {int(observation_width)} * samples {aa.samples} > 4096")
        if cameras is not None:
            from .render import check_camera_names
            if obs_type != "so100_pixels_agent_pos":
                raise ValueError("cameras need obs_type='so100_pixels_agent_pos'")
            cameras = check_camera_names(cameras)
            if not all(isinstance(c, str) for c in cameras):
                raise ValueError("cameras: a tuple of camera names")
        physical_dr_options(domain_randomization, variant)       # its ValueErrors before any device work
        if domain_randomization and domain_randomization.get("visual") is not None:
            if obs_type != "so100_pixels_agent_pos":
                raise ValueError("domain_randomization['visual'] needs obs_type='so100_pixels_agent_pos'")
            self._check_visual(domain_randomization["visual"])
        self.lib = _native.load()
        self.num_envs = int(num_envs)
        self.task = task
        self.obs_type = obs_type
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SO100VecEnv runs on a HIP device (torch 'cuda' device on ROCm)")
        self.autoreset = bool(autoreset)
        self.max_episode_steps = _MAX_STEPS[task] if max_episode_steps is None else int(max_episode_steps)
        self.base_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.env_offset = int(env_offset)
        self.solver = solver
        self.variant = variant
        self.model = build_model(iterations=iterations, solver=solver, variant=variant, nsubstep=nsubstep, convex=convex)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._handle = self.lib.so100_create(ctypes.byref(self.model), self.num_envs, dev_index)
        if not self._handle:
            raise RuntimeError("so100_create failed: " + self.lib.so100_last_error().decode())
        _native.check(self.lib.so100_configure(self._handle, _native.TASKS[task], self.max_episode_steps,
                                               ctypes.c_uint64(self.base_seed), self.env_offset), "so100_configure")
        n, d = self.num_envs, self.device
        f32, i32 = torch.float32, torch.int32
        self.qpos = torch.zeros(n, NQ, dtype=f32, device=d)
        self.qvel = torch.zeros(n, NV, dtype=f32, device=d)
        self.qacc_warmstart = torch.zeros(n, NV, dtype=f32, device=d)
        self.elapsed = torch.zeros(n, dtype=i32, device=d)
        self.episode = torch.zeros(n, dtype=i32, device=d)
        self.actions = torch.zeros(n, 6, dtype=f32, device=d)
        self.action_mode = action_mode
        self.action_dim = 6
        self.ee_actions = self.ee_joint_target = self.ee_target = self.reinit = None
        self.ee_control = self._ee_ctrl = None
        self.act_params = self.act_hist = self.act_head = self.act_command = None
        self._act = False               # the actuation model is on (set_domain_randomization(actuation=...))
        self._dr_ranges = None          # the record so100_dr_sample draws from, while something is drawn on the device
        self._dr_per_episode = False
        if action_mode == "ee_delta":
            self.action_dim = 5
            self.ee_control = ee_control_options(ee_control, self.model)
            self._ee_ctrl = _native.SO100EeCtrl(**self.ee_control)
            self.ee_actions = torch.zeros(n, 5, dtype=f32, device=d)        # the delta actions step() copies into
            self.ee_joint_target = torch.zeros(n, 5, dtype=f32, device=d)   # q_cmd
            self.ee_target = torch.zeros(n, 3, dtype=f32, device=d)
            self.reinit = torch.ones(n, dtype=torch.uint8, device=d)        # every command starts from its env's pose
            self._reinit_bool = self.reinit.view(torch.bool)
            self._reinit_pending = True                                      # host side: some byte of reinit may be set
        self._routed = self._ee_ctrl is not None       # a prologue writes ``actions``: the step never reads an action buffer
        self._pre = self._routed                       # a step is more than the so100_step launch
        self._norm = None                              # the running normaliser (normalize=...), built below
        self.obs_norm = self.reward_norm = self.final_obs_norm = None
        self.achieved_goal_norm = self.desired_goal_norm = self.agent_pos_norm = None
        self.obs = torch.zeros(n, NOBS, dtype=f32, device=d)
        self.reward = torch.zeros(n, dtype=f32, device=d)
        self.terminated = torch.zeros(n, dtype=torch.bool, device=d)
        self.truncated = torch.zeros(n, dtype=torch.bool, device=d)
        self.success = torch.zeros(n, dtype=torch.bool, device=d)
        self.diverged = torch.zeros(n, dtype=torch.bool, device=d)
        self.final_obs = torch.zeros(n, NOBS, dtype=f32, device=d)
        self.contact_bits = torch.zeros(n, dtype=i32, device=d)
        # contacts the 16-per-env cap left out in the last step (MuJoCo has no cap: 0 is the bar)
        self.ncon_dropped = torch.zeros(n, dtype=i32, device=d)
        self.is_goal = task == "so100_goal"
        self.achieved_goal = torch.zeros(n, 3, dtype=f32, device=d) if self.is_goal else None
        self.desired_goal = torch.zeros(n, 3, dtype=f32, device=d) if self.is_goal else None
        self.total_steps = torch.zeros(n, dtype=i32, device=d) if self.is_goal else None
        self.debug = torch.zeros(n, _native.SO100_DBG_STRIDE, dtype=f32, device=d) if debug else None
        self.reward64 = torch.zeros(n, dtype=torch.float64, device=d) if reward64 else None
        f64 = torch.float64
        self.ep_return = torch.zeros(n, dtype=f64, device=d) if episode_stats else None
        self.ep_final = torch.zeros(n, 2, dtype=f64, device=d) if episode_stats else None
        self.ep_accum = torch.zeros(n, 4, dtype=f64, device=d) if episode_stats else None
        self.mocap = None
        if variant == "ee":          # mj_resetData's mocap pose: the mocap body's (so_arm100_ee.xml:155)
            m0 = list(self.model.mocap_pos0) + list(self.model.mocap_quat0)
            self.mocap = torch.tensor(m0, dtype=f32, device=d).repeat(n, 1).contiguous()
        self.dr_params = None
        self._visual = None
        self._flags = _native.SO100_FLAG_AUTORESET if self.autoreset else 0
        if domain_randomization:
            self.set_domain_randomization(**domain_randomization)
        self._buf = _native.SO100Buffers()
        self._fill_buffers()
        self._seeds = torch.zeros(n, dtype=i32, device=d)
        self._mask = torch.zeros(n, dtype=torch.uint8, device=d)
        self.pixels = self.final_pixels = self.renderer = self.pixels_flat = None
        self.depth = self.segmentation = self.final_depth = self.final_segmentation = None
        self.channels_first = bool(channels_first)
        self.camera_names = None
        if obs_type == "so100_pixels_agent_pos":
            from .render import CameraRenderer, MultiCameraRenderer, SEG_BACKGROUND
            if cameras is None:
                self.renderer = CameraRenderer(self, observation_width, observation_height,
                                               channels_first=self.channels_first, depth=depth,
                                               segmentation=segmentation, shadows=shadows, antialias=antialias)
            else:
                self.renderer = MultiCameraRenderer(self, observation_width, observation_height, cameras=cameras,
                                                    channels_first=self.channels_first, depth=depth,
                                                    segmentation=segmentation, shadows=shadows,
                                                    antialias=antialias)
                self.camera_names = self.renderer.camera_names
            if self._visual is not None:
                self._sample_views()
            self.pixels = self.renderer.pixels
            self.final_pixels = torch.zeros_like(self.pixels) if self.autoreset else None
            self.depth, self.segmentation = self.renderer.depth, self.renderer.segmentation
            if self.autoreset:
                self.final_depth = None if self.depth is None else torch.zeros_like(self.depth)
                self.final_segmentation = None if self.segmentation is None else \
                    torch.full_like(self.segmentation, SEG_BACKGROUND)
            if flat_pixels:
                self._npix = 3 * self.renderer.width * self.renderer.height * (1 if cameras is None else len(cameras))
                self.pixels_flat = torch.zeros(n, self._npix + 6, dtype=f32, device=d)
        if norm_options is not None:
            if self.renderer is not None:
                keys = [("agent_pos", self.obs, 9, 6)]
            elif self.is_goal:
                keys = [("observation", self.obs, 0, NOBS), ("achieved_goal", self.achieved_goal, 0, 3),
                        ("desired_goal", self.desired_goal, 0, 3)]
            else:
                keys = [("obs", self.obs, 0, NOBS)]
            self._norm = Normalizer(self, norm_options, keys, final_src=self.final_obs if self.autoreset else None)
            out = self._norm.out
            self.obs_norm = out.get("obs", out.get("observation"))
            self.agent_pos_norm = out.get("agent_pos")
            self.achieved_goal_norm, self.desired_goal_norm = out.get("achieved_goal"), out.get("desired_goal")
            self.final_obs_norm = self._norm.final_out      # [N,15], or the final agent_pos [N,6] with pixels
            self.reward_norm = self._norm.reward_norm
            self._pre = True
        self.replay = None if replay_opts is None else HerReplay(self, replay_opts)
        self.uniform_replay = None if uniform_opts is None else UniformReplay(self, uniform_opts)

    # ------------------------------------------------------------------ plumbing
    def _fill_buffers(self):
        P = _native.ptr
        b = self._buf
        for name in ("qpos", "qvel", "qacc_warmstart", "elapsed", "episode", "obs", "reward", "terminated",
                     "truncated", "success", "final_obs", "diverged", "contact_bits", "achieved_goal",
                     "desired_goal", "total_steps", "dr_params", "debug", "mocap", "reward64", "ncon_dropped",
                     "ep_return", "ep_final", "ep_accum"):
            setattr(b, name, P(getattr(self, name)))
        if not getattr(self, "_debug_enabled", True):
            b.debug = None
        # (ee_delta, actuation: the step always reads the joint actions the prologue writes; an action buffer feeds the
        # prologue)
        b.action = P(self.actions) if getattr(self, "_action_ref", None) is None or self._routed \
            else P(self._action_ref)

    def set_mocap(self, pos, quat=None, mask=None):
        """EE variant: the mocap target pose of every env (pos [N,3], quat [N,4] wxyz; the data.mocap_pos /
        data.mocap_quat that teleop_ee.py:52-98 edits), or of the envs in mask."""
        torch = _torch()
        if self.mocap is None:
            raise ValueError("set_mocap needs variant='ee'")
        p = torch.as_tensor(pos, dtype=torch.float32, device=self.device).reshape(-1, 3)
        q = None if quat is None else torch.as_tensor(quat, dtype=torch.float32, device=self.device).reshape(-1, 4)
        if mask is None:
            self.mocap[:, :3] = p
            if q is not None:
                self.mocap[:, 3:] = q
        else:
            m = torch.as_tensor(mask, device=self.device).bool()
            self.mocap[m, :3] = p if p.shape[0] != self.num_envs else p[m]
            if q is not None:
                self.mocap[m, 3:] = q if q.shape[0] != self.num_envs else q[m]

    def _stream(self):
        return _native.stream_ptr(_torch(), self.device)

    @staticmethod
    def _check_visual(visual):
        """The argument checks of a visual-randomisation dict (no device use); returns (ranges, per_episode, seed)."""
        from .render import view_ranges
        v = dict(visual)
        per_episode, seed = bool(v.pop("per_episode", False)), v.pop("seed", None)
        view_ranges(v, 0)
        return v, per_episode, seed

    def _sample_views(self, mask=None):
        """Draw the view records (of the envs in mask): from the device episode counter with per_episode, else with
        episode 0."""
        ranges, per_episode, seed = self._visual
        self.renderer.sample_views(ranges, seed, episode=self.episode if per_episode else None, mask=mask)

    def set_domain_randomization(self, mass=(0.8, 1.2), friction=(0.8, 1.2), action_noise=0.05, seed=None, visual=None,
                                 per_episode=False, actuation=None):
        """Per-env cube mass scale, contact friction scale (fixed per env) and action-noise sigma.

        The scales are a counter-based hash of (seed, global env id), so an env draws the same parameters
        whatever the sharding (configs[4]: 32,768 envs over 4 GPUs).

        visual (pixel observations only; None = every env drawn from the one camera): a dict of the ranges each env's
        view is drawn from, by the same hash (fields from 16 up) on the device: camera_pos (half-width, metres),
        camera_rot_deg (half-width of a rotation vector's components about the camera's axes), fovy, ambient,
        headlight, lights ((lo, hi) scales; lights: one pair or one per light), light_rot_deg (one rotation of every
        light direction), colors (one (lo, hi) per-channel scale or a dict by render.MATERIALS name), per_episode
        (default False: drawn once; True: an env's view is drawn again from its episode counter whenever it is reset,
        the terminal image in final_pixels still showing the finished episode's view) and seed (default: the env's
        base seed).  It touches images only; the physical part above applies as without it.

        per_episode (default False: ``dr_params`` is the host draw above and is never rewritten): True draws mass and
        friction on the device instead (so100_dr_sample: the visual part's hash of (seed, global env id, episode, field),
        fields 1 and 2), from each env's episode counter: now, after every ``reset`` for the reset envs and, with
        auto-reset, after every step for the envs that finished, on the caller's stream with no host synchronisation.
        ``dr_params`` keeps its address.

        actuation (default None: the command is the applied action): a dict of up to three ranges, delay=(lo, hi) whole
        control steps in 0..7, smoothing=(lo, hi) in (0, 1], rate=(lo, hi) > 0 in normalised action units per control
        step; a missing key is off (ACTUATION_OFF).  Each env draws (delay, alpha, rate) into ``act_params`` [N,4] (fields
        4, 5, 6; once, or per episode with per_episode), and every step so100_actuate turns the clipped command into the
        applied action in ``actions``: the command of `delay` steps earlier, smoothed by y + alpha (v - y), moved by at
        most `rate`.  After a reset the actuator holds the measured pose until the first delayed command arrives
        (``reinit``).  The step's action noise is added after it.  ValueError with variant="ee" and for out-of-range
        values."""
        torch = _torch()
        physical_dr_options({"mass": mass, "friction": friction, "per_episode": per_episode, "actuation": actuation},
                            self.variant)
        if visual is not None:
            if self.obs_type != "so100_pixels_agent_pos":
                raise ValueError("domain_randomization['visual'] needs obs_type='so100_pixels_agent_pos'")
            ranges, view_per_episode, vseed = self._check_visual(visual)
            self._visual = (ranges, view_per_episode, self.base_seed if vseed is None else int(vseed))
        else:
            self._visual = None
        if getattr(self, "renderer", None) is not None:      # (the constructor samples once its renderer exists)
            if self._visual is None:
                self.renderer.views = None
            else:
                self._sample_views()
        s = self.base_seed if seed is None else int(seed)
        ids = np.arange(self.env_offset, self.env_offset + self.num_envs, dtype=np.uint64)
        p = torch.zeros(self.num_envs, 4, dtype=torch.float32)
        p[:, 0] = torch.from_numpy(mass[0] + (mass[1] - mass[0]) * _hash_uniform(s, ids, 1))
        p[:, 1] = torch.from_numpy(friction[0] + (friction[1] - friction[0]) * _hash_uniform(s, ids, 2))
        p[:, 2] = float(action_noise)
        self._dr_per_episode = bool(per_episode)
        self._act = actuation is not None
        self._dr_ranges = None
        if self._dr_per_episode:
            p[:, :2] = 0.0                          # drawn on the device below
        self.dr_params = p.to(self.device)
        if self._dr_per_episode or self._act:
            act = actuation_options(actuation) if self._act else ACTUATION_OFF
            self._dr_ranges = _native.SO100DrRanges(seed=s, mass=mass if self._dr_per_episode else (1.0, 1.0),
                                                    friction=friction if self._dr_per_episode else (1.0, 1.0), **act)
        n, d = self.num_envs, self.device
        if self._act:
            if self.act_params is None:
                self.act_params = torch.zeros(n, 4, dtype=torch.float32, device=d)
                self.act_hist = torch.zeros(_native.SO100_ACT_HIST, n, 6, dtype=torch.float32, device=d)
                self.act_head = torch.zeros(n, dtype=torch.int32, device=d)
                self.act_command = torch.zeros(n, 6, dtype=torch.float32, device=d)   # the command step() copies into
            if self.reinit is None:                  # (ee_delta has it already: the two prologues share it)
                self.reinit = torch.ones(n, dtype=torch.uint8, device=d)
                self._reinit_bool = self.reinit.view(torch.bool)
            self.reinit.fill_(1)                     # every actuator starts from its env's pose
            self._reinit_pending = True
        self._routed = self._ee_ctrl is not None or self._act
        self._pre = self._routed or self._dr_per_episode or getattr(self, "_norm", None) is not None
        if self._dr_ranges is not None:
            self._dr_sample(None, None, act_only=not self._dr_per_episode)
        self._flags |= _native.SO100_FLAG_DR
        if hasattr(self, "_buf"):
            self._fill_buffers()

    def _dr_sample(self, mask_a, mask_b, act_only=False, keep_act=False):
        """so100_dr_sample on the current stream: the dr_params rows (unless act_only) and, with the actuation model
        (unless keep_act), the act_params rows of the envs in either byte mask (None, None: every env), per_episode: from
        the episode counter"""
        P = _native.ptr
        _native.check(self.lib.so100_dr_sample(self._handle, ctypes.byref(self._dr_ranges),
                                               P(self.episode) if self._dr_per_episode else None, P(mask_a), P(mask_b),
                                               None if act_only else P(self.dr_params),
                                               P(self.act_params) if self._act and not keep_act else None,
                                               self._stream()),
                      "so100_dr_sample")

    # ------------------------------------------------------------------ API
    def reset(self, seed=None, mask=None):
        """Reset all envs (or those with mask[i] true).

        seed: None -> in-kernel seeds from (base seed, global env id, episode);
              int s -> env i uses RandomState(s + i) exactly like SB3's VecEnv.seed(s);
              sequence/array/tensor of N ints -> per-env RandomState seeds.
        """
        torch = _torch()
        seeds_p = None
        if seed is not None:
            if isinstance(seed, (int, np.integer)):
                s = (int(seed) + np.arange(self.num_envs, dtype=np.int64)) & 0xFFFFFFFF
            else:
                s = np.asarray(seed.cpu() if hasattr(seed, "cpu") else seed, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
                if s.shape[0] != self.num_envs:
                    raise ValueError("need one seed per env")
            self._seeds.copy_(torch.from_numpy(s.astype(np.uint32).view(np.int32)))
            seeds_p = _native.ptr(self._seeds)
        mask_p = None
        if mask is not None:
            m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
            self._mask.copy_(m.to(self.device).to(torch.uint8))
            mask_p = _native.ptr(self._mask)
        _native.check(self.lib.so100_reset(self._handle, ctypes.byref(self._buf), mask_p, seeds_p, self._stream()),
                      "so100_reset")
        if self._dr_per_episode:                         # the reset envs' new episodes: their physical parameters
            self._dr_sample(None if mask is None else self._mask, None)
        if self._routed:                                 # the reset envs' commands start again from their fresh pose
            if mask is None:
                self.reinit.fill_(1)
            else:
                self.reinit.bitwise_or_(self._mask.ne(0).to(torch.uint8))
            self._reinit_pending = True
        if self.renderer is not None:
            if self._visual is not None and self._visual[1]:
                self._sample_views(None if mask is None else self._mask)
            self._render_all()
        if self._norm is not None:                       # the reset envs' observations enter the statistics
            self._norm.after_reset(None if mask is None else self._mask)
        if self.replay is not None:                      # the reset envs' open episodes go, their fresh rows are staged
            self.replay.after_reset(None if mask is None else self._mask)
        if self.uniform_replay is not None:              # the reset envs' fresh rows and images are staged
            self.uniform_replay.after_reset(None if mask is None else self._mask)
        info = {"is_success": torch.zeros_like(self.success)}
        return self._observation(), info

    def step(self, actions):
        """actions: [N,6] (action_mode="ee_delta": [N,5]) (torch tensor on any device, or numpy) in [-1, 1]."""
        torch = _torch()
        if getattr(self, "_action_ref", None) is not None:
            self._action_ref = None
            self._buf.action = _native.ptr(self.actions)
        k = self.action_dim
        dst = self.ee_actions if self._ee_ctrl is not None else (self.act_command if self._act else self.actions)
        if isinstance(actions, torch.Tensor):
            if actions.shape != (self.num_envs, k):
                raise ValueError(f"actions must be [{self.num_envs}, {k}], got {tuple(actions.shape)}")
            if actions.device == self.device and actions.dtype == torch.float32 and actions.is_contiguous():
                if actions.data_ptr() != dst.data_ptr():
                    dst.copy_(actions)
            else:
                dst.copy_(actions.to(self.device, torch.float32))
        else:
            a = np.asarray(actions, dtype=np.float32)
            if a.shape != (self.num_envs, k):
                raise ValueError(f"actions must be [{self.num_envs}, {k}], got {a.shape}")
            dst.copy_(torch.from_numpy(a))
        if self._routed:
            self._prologue()
        if self.renderer is None:
            _native.check(self.lib.so100_step(self._handle, ctypes.byref(self._buf), self._flags, self._stream()),
                          "so100_step")
            done = self.terminated | self.truncated
            if self._dr_per_episode and self.autoreset:  # the step has bumped the finished envs' episode counters
                self._dr_sample(self.terminated, self.truncated)
        else:
            done = self._step_pixels()
        if self._routed:
            self._epilogue()
        if self._norm is not None:
            self._norm.after_step()
        if self.replay is not None:                      # one transition per env, with the command as it came in
            self.replay.after_step(dst)
        if self.uniform_replay is not None:
            self.uniform_replay.after_step(dst)
        info = {"is_success": self.success, "diverged": self.diverged, "contact_bits": self.contact_bits,
                "ncon_dropped": self.ncon_dropped}
        if self.autoreset:
            # (normalize: the rows of the envs that finished, normalised with the statistics as the step left them)
            final = self.final_obs if self.final_obs_norm is None else self.final_obs_norm
            info["final_observation"] = final if self.renderer is None else self._with_aux(
                {"pixels": self.final_pixels,
                 "agent_pos": self.final_obs[:, 9:15] if self.final_obs_norm is None else final},
                self.final_depth, self.final_segmentation)
            info["_final_observation"] = done
        if self.is_goal:
            info["TimeLimit.truncated"] = self.truncated
        if self.ep_final is not None:                  # RecordEpisodeStatistics' info["episode"] / "_episode"
            info["episode"] = {"r": self.ep_final[:, 0], "l": self.ep_final[:, 1]}
            info["_episode"] = done
        reward = self.reward if self.reward_norm is None else self.reward_norm
        return self._observation(), reward, self.terminated, self.truncated, info

    def set_action_buffer(self, actions):
        """Point the kernel's action input at a resident [N,6] float32 device tensor (zero copy).
        The tensor must stay alive until the next call; ``step()`` copies into ``self.actions``.
        action_mode="ee_delta": a [N,5] tensor, read by the prologue that fills ``self.actions``; with the actuation
        model the tensor is the command the actuator reads."""
        torch = _torch()
        k = self.action_dim
        if actions.shape != (self.num_envs, k) or actions.dtype != torch.float32 or not actions.is_contiguous() \
                or actions.device != self.device:
            raise ValueError(f"action buffer must be a contiguous float32 [N,{k}] tensor on the env's device")
        self._action_ref = actions
        if not self._routed:
            self._buf.action = _native.ptr(actions)

    def _prologue(self):
        """ee_delta and / or the actuation model, on the current stream: the delta actions (``ee_actions`` or the action
        buffer) -> joint command -> ``actions``; the joint command is ``act_command`` (or the action buffer) when the
        actuator follows, else ``actions`` itself"""
        ref = getattr(self, "_action_ref", None)
        P = _native.ptr
        if self._ee_ctrl is not None:
            src = self.ee_actions if ref is None else ref
            _native.check(self.lib.so100_ee_action(self._handle, ctypes.byref(self._ee_ctrl), P(self.qpos), P(src),
                                                   P(self.reinit), P(self.ee_joint_target),
                                                   P(self.act_command if self._act else self.actions),
                                                   P(self.ee_target), self._stream()), "so100_ee_action")
            ref = None
        if self._act:
            src = self.act_command if ref is None else ref
            _native.check(self.lib.so100_actuate(self._handle, P(self.qpos), P(src), P(self.reinit), P(self.act_params),
                                                 P(self.act_hist), P(self.act_head), P(self.actions), self._stream()),
                          "so100_actuate")

    def _epilogue(self):
        """ee_delta / actuation: after the step, mark the envs whose command starts from their pose at the next step:
        with auto-reset the envs that just finished (their qpos is a new episode's), else none"""
        if self.autoreset:
            _torch().logical_or(self.terminated, self.truncated, out=self._reinit_bool)
        elif self._reinit_pending:
            self.reinit.zero_()
            self._reinit_pending = False

    def _step_pixels(self):
        """Pixel observations: step without the in-kernel reset, draw the terminal images of finished envs,
        reset them with the masked reset kernel (same seeds/episode counters as the in-kernel reset), then
        draw every env.  All on the current stream, no host synchronisation."""
        s = self._stream()
        flags = self._flags & ~_native.SO100_FLAG_AUTORESET
        _native.check(self.lib.so100_step(self._handle, ctypes.byref(self._buf), flags, s), "so100_step")
        done = self.terminated | self.truncated
        if self.autoreset:
            self.final_obs.copy_(self.obs)
            self._mask.copy_(done)
            self.renderer.render(out=self.final_pixels, mask=self._mask, depth=self.final_depth,
                                 segmentation=self.final_segmentation)
            _native.check(self.lib.so100_reset(self._handle, ctypes.byref(self._buf), _native.ptr(self._mask), None,
                                               s), "so100_reset")
            if self._visual is not None and self._visual[1]:
                self._sample_views(self._mask)         # the new episodes' views: final_pixels is already drawn
            if self._dr_per_episode:
                self._dr_sample(self._mask, None)      # and their physical parameters
        self._render_all()
        return done

    def _render_all(self):
        """Draw every env into ``pixels``; with flat_pixels the same launch fills the image part of ``pixels_flat``,
        and agent_pos goes into its last six columns."""
        self.renderer.render(flat=self.pixels_flat)
        if self.pixels_flat is not None:
            self.pixels_flat[:, self._npix:].copy_(self.obs[:, 9:15])

    @staticmethod
    def _with_aux(obs, depth, segmentation):
        """obs with the "depth" / "segmentation" keys of the options that are on"""
        if depth is not None:
            obs["depth"] = depth
        if segmentation is not None:
            obs["segmentation"] = segmentation
        return obs

    def episode_statistics(self, clear=False):
        """Totals of the episodes finished since construction (or the last ``clear``), reduced over the envs
        on the device and read once: episodes, successes, success_rate, mean_return, mean_length."""
        if self.ep_accum is None:
            raise ValueError("episode statistics need episode_stats=True")
        t = self.ep_accum.sum(dim=0).cpu().tolist()
        if clear:
            self.ep_accum.zero_()
        n = t[0]
        return {"episodes": int(n), "successes": int(t[1]), "success_rate": t[1] / n if n else float("nan"),
                "mean_return": t[2] / n if n else float("nan"), "mean_length": t[3] / n if n else float("nan")}

    def step_async_raw(self):
        """Launch one env step on the current stream using the actions already in ``self.actions``
        (no argument handling, no output views) — the benchmark's hot loop.  action_mode="ee_delta": the delta
        actions already in ``self.ee_actions`` (or the action buffer), through the prologue; with the actuation model
        the command already in ``self.act_command`` (or the action buffer)."""
        if self._pre:
            if self._routed:
                self._prologue()
            self.lib.so100_step(self._handle, ctypes.byref(self._buf), self._flags, self._stream())
            if self._dr_per_episode and self.autoreset:
                self._dr_sample(self.terminated, self.truncated)
            if self._routed:
                self._epilogue()
            if self._norm is not None:
                self._norm.after_step()
            return
        self.lib.so100_step(self._handle, ctypes.byref(self._buf), self._flags, self._stream())

    def _observation(self):
        if self.renderer is not None:
            agent_pos = self.obs[:, 9:15]                       # qpos[:6] float32 (single_arm.py:45-50)
            if self.is_goal:                                     # _flatten_observation (env.py:267-270)
                if self.pixels_flat is not None:
                    return self._with_aux({"observation": self.pixels_flat, "achieved_goal": self.achieved_goal,
                                           "desired_goal": self.desired_goal}, self.depth, self.segmentation)
                flat = self.pixels.reshape(self.num_envs, -1).to(_torch().float32).div_(255.0)
                return self._with_aux({"observation": _torch().cat([flat, agent_pos], dim=1),
                                       "achieved_goal": self.achieved_goal, "desired_goal": self.desired_goal},
                                      self.depth, self.segmentation)
            if self.agent_pos_norm is not None:
                agent_pos = self.agent_pos_norm
            return self._with_aux({"pixels": self.pixels, "agent_pos": agent_pos}, self.depth, self.segmentation)
        if self.obs_norm is not None:
            if self.is_goal:
                return {"observation": self.obs_norm, "achieved_goal": self.achieved_goal_norm,
                        "desired_goal": self.desired_goal_norm}
            return self.obs_norm
        if self.is_goal:
            return {"observation": self.obs, "achieved_goal": self.achieved_goal, "desired_goal": self.desired_goal}
        return self.obs

    # ------------------------------------------------------------------ running normalisation (normalize=...)
    # The properties and methods below go through _normalizer(): on an env built without normalize=... they raise
    # NormalizeOffError from inside the property (so `env.training` raises rather than answering False, and
    # hasattr(env, "obs_rms") is False, which the SB3 adapter's get_attr / set_attr rely on).
    def _normalizer(self):
        if self._norm is None:
            raise NormalizeOffError("this env was built without normalize=...")
        return self._norm

    @property
    def training(self):
        """normalize: while True every ``step`` / ``reset`` updates the statistics; False freezes them (an eval env)"""
        return self._normalizer().training

    @training.setter
    def training(self, on):
        self._normalizer().training = bool(on)

    @property
    def obs_rms(self):
        """normalize: key -> object with .mean / .var (float64 numpy) and .count, copied from the device on access (a
        synchronisation).  Keys: "obs" (state env), "observation" / "achieved_goal" / "desired_goal" (GoalEnv),
        "agent_pos" (pixel observations).  Assignable: ``eval_env.obs_rms = train_env.obs_rms``."""
        return self._normalizer().obs_rms()

    @obs_rms.setter
    def obs_rms(self, rms):
        self._normalizer().set_obs_rms(rms)

    @property
    def ret_rms(self):
        """normalize: the discounted return's .mean / .var / .count, copied from the device on access"""
        return self._normalizer().ret_rms()

    @ret_rms.setter
    def ret_rms(self, rms):
        self._normalizer().set_ret_rms(rms)

    def normalize_obs(self, obs):
        """normalize: clip((obs - mean) / sqrt(var + epsilon)) with the current statistics, on the device (no update):
        a float32 device tensor [..., dim] of the env's first key, or a dict by key (other keys pass through)"""
        return self._normalizer().transform(obs)

    def unnormalize_obs(self, obs):
        """normalize: obs * sqrt(var + epsilon) + mean, the inverse of ``normalize_obs`` where it did not clip"""
        return self._normalizer().transform(obs, inverse=True)

    def normalize_state(self):
        """normalize: the statistics as a plain dict of float64 numpy arrays ("<key>.mean" / ".var" / ".count", "ret.*")
        plus the options, as ``np.savez(path, **state)`` stores it bit for bit"""
        return self._normalizer().state()

    def set_normalize_state(self, state):
        """normalize: take the statistics of ``normalize_state()`` (another env's, a checkpoint's ``np.load``, or
        ``merge_normalize_states`` of several shards'); the options stay this env's"""
        self._normalizer().set_state(state)

    def compute_reward(self, achieved_goal, desired_goal, info=None):
        """Batched sparse GoalEnv reward on the device (env.py:341-353)."""
        torch = _torch()
        a = torch.as_tensor(achieved_goal, dtype=torch.float32, device=self.device).reshape(-1, 3).contiguous()
        d = torch.as_tensor(desired_goal, dtype=torch.float32, device=self.device).reshape(-1, 3).contiguous()
        out = torch.empty(a.shape[0], dtype=torch.float32, device=self.device)
        _native.check(self.lib.so100_goal_reward(self._handle, a.shape[0], _native.ptr(a), _native.ptr(d),
                                                 _native.ptr(out), self._stream()), "so100_goal_reward")
        return out

    # state access (checkpoint / teacher-forced parity tests)
    def get_state(self):
        st = {"qpos": self.qpos.clone(), "qvel": self.qvel.clone(), "qacc_warmstart": self.qacc_warmstart.clone(),
              "elapsed": self.elapsed.clone(), "episode": self.episode.clone()}
        if self._ee_ctrl is not None:
            st["ee_joint_target"] = self.ee_joint_target.clone()
        if self._act:
            st["actuation"] = {"hist": self.act_hist.clone(), "head": self.act_head.clone(),
                               "params": self.act_params.clone(), "applied": self.actions.clone()}
        if self._norm is not None and self._norm.ret is not None:
            st["ret"] = self._norm.ret.clone()
        return st

    def set_state(self, qpos, qvel, qacc_warmstart=None, elapsed=None, episode=None, ee_joint_target=None,
                  actuation=None, ret=None):
        """action_mode="ee_delta": ee_joint_target [N,5] restores the commanded joint targets (from ``get_state``);
        without it every command starts again from the new qpos.  ValueError in joint mode.  With the actuation model,
        actuation (``get_state()["actuation"]``: the command ring, head, act_params and the applied action) restores the
        actuators; without it every actuator starts again from the new qpos with the parameters it has.  ValueError
        without the model.  When both prologues run and only one state is given, both start again from the new qpos
        (they share ``reinit``).  With per_episode the physical parameters are drawn again from the episode counters
        given."""
        torch = _torch()
        if ee_joint_target is not None and self._ee_ctrl is None:
            raise ValueError("ee_joint_target needs action_mode='ee_delta'")
        if actuation is not None and not self._act:
            raise ValueError("actuation state needs domain_randomization['actuation']")
        if ret is not None:                          # normalize: the discounted returns (``get_state()["ret"]``)
            if self._norm is None or self._norm.ret is None:
                raise ValueError("ret needs normalize=... with a discount gamma")
            self._norm.ret.copy_(torch.as_tensor(ret, dtype=torch.float64))
        if self._routed:
            if ee_joint_target is not None:
                self.ee_joint_target.copy_(torch.as_tensor(ee_joint_target, dtype=torch.float32))
            if actuation is not None:
                self.act_hist.copy_(torch.as_tensor(actuation["hist"], dtype=torch.float32))
                self.act_head.copy_(torch.as_tensor(actuation["head"], dtype=torch.int32))
                self.act_params.copy_(torch.as_tensor(actuation["params"], dtype=torch.float32))
                self.actions.copy_(torch.as_tensor(actuation["applied"], dtype=torch.float32))
            if (self._ee_ctrl is not None and ee_joint_target is None) or (self._act and actuation is None):
                self.reinit.fill_(1)
            else:
                self.reinit.zero_()
            self._reinit_pending = True
        self.qpos.copy_(torch.as_tensor(qpos, dtype=torch.float32))
        self.qvel.copy_(torch.as_tensor(qvel, dtype=torch.float32))
        if qacc_warmstart is not None:
            self.qacc_warmstart.copy_(torch.as_tensor(qacc_warmstart, dtype=torch.float32))
        if elapsed is not None:
            self.elapsed.copy_(torch.as_tensor(elapsed, dtype=torch.int32))
        if episode is not None:
            self.episode.copy_(torch.as_tensor(episode, dtype=torch.int32))
            if self._dr_per_episode:                 # (the actuator records restored above stay what they are)
                self._dr_sample(None, None, keep_act=actuation is not None)

    # standalone ops exposed for parity tests
    def eval_reward(self, task, cube_site, ee_site, pair_bits):
        torch = _torch()
        c = torch.as_tensor(cube_site, dtype=torch.float32, device=self.device).contiguous()
        e = torch.as_tensor(ee_site, dtype=torch.float32, device=self.device).contiguous()
        b = torch.as_tensor(np.asarray(pair_bits, dtype=np.uint32).view(np.int32), device=self.device).contiguous()
        out = torch.empty(c.shape[0], dtype=torch.float32, device=self.device)
        _native.check(self.lib.so100_eval_reward(self._handle, _native.TASKS[task], c.shape[0], _native.ptr(c),
                                                 _native.ptr(e), _native.ptr(b), _native.ptr(out), self._stream()),
                      "so100_eval_reward")
        return out

    def spawn_pose(self, seeds):
        torch = _torch()
        s = np.asarray(seeds, dtype=np.int64) & 0xFFFFFFFF
        st = torch.as_tensor(s.astype(np.uint32).view(np.int32), device=self.device).contiguous()
        out = torch.empty(len(s), 7, dtype=torch.float64, device=self.device)
        _native.check(self.lib.so100_spawn_pose(self._handle, len(s), _native.ptr(st), _native.ptr(out),
                                                self._stream()), "so100_spawn_pose")
        return out

    def unnormalize(self, actions):
        torch = _torch()
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device).reshape(-1, 6).contiguous()
        out = torch.empty_like(a)
        _native.check(self.lib.so100_unnormalize(self._handle, a.shape[0], _native.ptr(a), _native.ptr(out),
                                                 self._stream()), "so100_unnormalize")
        return out

    # ---------------------------------------------------------------- benchmark instrumentation
    def profile_enable(self, max_steps):
        """Record HIP events around every stage/solver launch of the next max_steps steps (0 = off)."""
        _native.check(self.lib.so100_profile_enable(self._handle, int(max_steps)), "so100_profile_enable")

    def profile_read(self):
        """(solver_ms, solver_launches, stage_ms, stage_launches) summed since profile_enable; synchronises."""
        sm, sn, tm, tn = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0), ctypes.c_int(0)
        _native.check(self.lib.so100_profile_read(self._handle, ctypes.byref(sm), ctypes.byref(sn),
                                                  ctypes.byref(tm), ctypes.byref(tn)), "so100_profile_read")
        return sm.value, sn.value, tm.value, tn.value

    @property
    def fused(self):
        """True when a step is one fused kernel launch (Newton solver); False: the split stage/solver
        launches (always for PGS).  Set True / False to force a mode, None for auto (the default: fused at
        every size, SO100_FUSED_MAX=n splits above n envs; include/so100.h so100_set_step_mode)."""
        return bool(self.lib.so100_step_mode(self._handle))

    @fused.setter
    def fused(self, on):
        mode = -1 if on is None else (1 if on else 0)
        _native.check(self.lib.so100_set_step_mode(self._handle, mode), "so100_set_step_mode")

    @property
    def debug_enabled(self):
        """Whether steps write the debug buffer (and so launch the fused kernel's debug build)."""
        return self.debug is not None and getattr(self, "_debug_enabled", True)

    @debug_enabled.setter
    def debug_enabled(self, on):
        self._debug_enabled = bool(on)
        self._fill_buffers()

    @property
    def fused_build(self):
        """The fused kernel build the next fused step launches: 1 = debug build, 2 / 3 = the product build for
        2 / 3 waves per SIMD.  Set 2, 3 or 0 (auto, the default) to choose the product build
        (include/so100.h so100_set_fused_build); every build gives the same results bit for bit."""
        return int(self.lib.so100_fused_build(self._handle, 1 if self.debug_enabled else 0))

    @fused_build.setter
    def fused_build(self, waves):
        _native.check(self.lib.so100_set_fused_build(self._handle, int(waves or 0)), "so100_set_fused_build")

    @property
    def env_packing(self):
        """Whether the next fused step packs envs of like solver cost into the same wave: a schedule
        only, every result is bit for bit the same with it on or off.  Set True / False, or None for auto (the default:
        off at every size, where it measured no gain; include/so100.h so100_set_env_packing)."""
        return bool(self.lib.so100_env_packing(self._handle))

    @env_packing.setter
    def env_packing(self, mode):
        _native.check(self.lib.so100_set_env_packing(self._handle, -1 if mode is None else int(bool(mode))),
                      "so100_set_env_packing")

    def env_order(self):
        """The order the last fused launch used (int32 [4 * ceil(N / 4)]): entry 4 * slot + row is the env that row
        `row` of launch slot `slot` stepped; ids >= N are idle rows.  Synchronises the device."""
        out = np.zeros((self.num_envs + 3) // 4 * 4, dtype=np.int32)
        _native.check(self.lib.so100_env_order(self._handle, out.ctypes.data_as(ctypes.c_void_p), out.size), "so100_env_order")
        return out

    def env_cost(self):
        """Each env's solver cost in the last packed fused step, summed over its substeps (the packing key), as three int
        arrays: Newton loop passes (saturating at 255), contacts, convex narrowphase items (at 4095).  Synchronises
        the device."""
        out = np.zeros(self.num_envs, dtype=np.uint32)
        _native.check(self.lib.so100_env_cost(self._handle, out.ctypes.data_as(ctypes.c_void_p), out.size), "so100_env_cost")
        return (out >> 24).astype(np.int64), ((out >> 12) & 4095).astype(np.int64), (out & 4095).astype(np.int64)

    def wave_cost(self):
        """Shader cycles of each wave of the last fused step (uint32 [ceil(N / 4)]): by launch slot with packing on, by
        natural group (env // 4) with it off.  Synchronises the device."""
        out = np.zeros((self.num_envs + 3) // 4, dtype=np.uint32)
        _native.check(self.lib.so100_wave_cost(self._handle, out.ctypes.data_as(ctypes.c_void_p), out.size), "so100_wave_cost")
        return out

    def chunk_info(self):
        """(chunks, envs of chunk 0): the env split of a step; profile_read times chunk 0's launches."""
        k, n0 = ctypes.c_int(0), ctypes.c_int(0)
        _native.check(self.lib.so100_chunk_info(self._handle, ctypes.byref(k), ctypes.byref(n0)), "so100_chunk_info")
        return k.value, n0.value

    def pool_stats(self, reset=False):
        """The fused step's contact-record pool, summed over the steps since construction or the last
        reset: {"taken": entries taken (wave-substeps whose env lists passed the 16 held on chip), "none_free": entry
        requests that found none free (0 by construction: each XCD's pool holds an entry per wave it can hold
        resident), "entries_per_xcd": the pool's size}.  Synchronises the device."""
        out = (ctypes.c_uint64 * 3)()
        _native.check(self.lib.so100_pool_stats(self._handle, out, int(bool(reset))), "so100_pool_stats")
        return {"taken": int(out[0]), "none_free": int(out[1]), "entries_per_xcd": int(out[2])}

    def contact_count(self, accum):
        """accum (int64 device tensor, 1 element) += contacts in the last solver launch, summed over envs."""
        _native.check(self.lib.so100_contact_count(self._handle, _native.ptr(accum), self._stream()),
                      "so100_contact_count")

    def contact_counts(self):
        """int32 device tensor [N]: each env's contact count in the last solver launch (the last substep's list;
        up to SO100_NCON_MAX, the first 16 held on chip).  Zeros before the first solver launch (zero-initialised:
        the native call writes nothing until a launch has recorded counts)."""
        torch = _torch()
        out = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        _native.check(self.lib.so100_contact_counts(self._handle, _native.ptr(out), self._stream()),
                      "so100_contact_counts")
        return out

    def close(self):
        if getattr(self, "_handle", None):
            self.lib.so100_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
