"""A hindsight replay buffer for the GoalEnv on the device: SB3 ``HerReplayBuffer``'s semantics, the
transitions kept where the step produces them, pushed, scanned and sampled by the launches of csrc/so100_her.hip with no
host synchronisation.  ``SO100VecEnv(replay=...)`` owns one ``HerReplay`` (``env.replay``); this module also holds the
option checks, which touch no device.

Beside it the uniform replay buffer of the arm tasks: SB3 ``DictReplayBuffer``'s storage for state and
pixel observations, with DrQ's random-shift augmentation in the sample launch (csrc/so100_replay.hip).
``SO100VecEnv(uniform_replay=...)`` owns one ``UniformReplay`` (``env.uniform_replay``).  With the option ``n_step`` it
also keeps the ``ends`` bytes and samples n-step returns; with the option ``prioritized`` it keeps a
priority per transition, samples in proportion to it and takes ``update_priorities``."""
import ctypes
import math

import numpy as np

from . import _native
from .model import NOBS

# the reference's HerReplayBuffer(n_sampled_goal=4, goal_selection_strategy="future") (scripts/train_sac_her.py:236-251)
REPLAY_DEFAULTS = dict(buffer_size=None, n_sampled_goal=4, goal_selection_strategy="future", seed=None)


def _int(what, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"replay: {what} {v!r} must be an integer")
    return int(v)


def replay_options(replay, num_envs=None, task="so100_goal", obs_type="so100_state", autoreset=True,
                   max_episode_steps=None):
    """The checked options of ``SO100VecEnv(replay=...)`` as a dict (no device use): None -> None (off), a dict -> the
    defaults overridden by it, with ``T = buffer_size // num_envs`` (the slots per env) added when ``num_envs`` is
    given.  Raises ValueError for unknown keys and bad values, and, given the env's arguments, unless the task is the
    GoalEnv with its state observation and auto-reset and ``T >= max_episode_steps`` (an open episode can then never
    overwrite itself)."""
    if replay is None:
        return None
    if not isinstance(replay, dict):
        raise ValueError("replay: None or a dict(" + ", ".join(f"{k}=" for k in REPLAY_DEFAULTS) + ")")
    unknown = set(replay) - set(REPLAY_DEFAULTS)
    if unknown:
        raise ValueError(f"replay: unknown keys {sorted(unknown)}; known: {sorted(REPLAY_DEFAULTS)}")
    o = dict(REPLAY_DEFAULTS)
    o.update(replay)
    if o["buffer_size"] is None:
        raise ValueError("replay: buffer_size (transitions over all envs) is required")
    o["buffer_size"] = _int("buffer_size", o["buffer_size"])
    if o["buffer_size"] < 1:
        raise ValueError(f"replay: buffer_size {o['buffer_size']} must be >= 1")
    o["n_sampled_goal"] = _int("n_sampled_goal", o["n_sampled_goal"])
    if o["n_sampled_goal"] < 0:
        raise ValueError(f"replay: n_sampled_goal {o['n_sampled_goal']} must be >= 0")
    if o["goal_selection_strategy"] not in _native.HER_STRATEGIES:
        raise ValueError(f"replay: goal_selection_strategy {o['goal_selection_strategy']!r}: one of "
                         f"{sorted(_native.HER_STRATEGIES)}")
    if o["seed"] is not None:
        o["seed"] = _int("seed", o["seed"])
    if num_envs is not None:
        if task != "so100_goal":
            raise ValueError(f"replay: hindsight relabelling needs task='so100_goal', not {task!r}")
        if obs_type != "so100_state":
            raise ValueError("replay: the buffer stores the 15-float state observation (obs_type='so100_state')")
        if not autoreset:
            raise ValueError("replay: needs autoreset=True (the step then hands over the finished episode's last "
                             "observation and the next episode's first)")
        T = o["buffer_size"] // int(num_envs)
        if T < 1 or (max_episode_steps is not None and T < int(max_episode_steps)):
            raise ValueError(f"replay: buffer_size {o['buffer_size']} // num_envs {num_envs} = {T} slots per env; an "
                             f"episode takes up to {max_episode_steps}")
        if T * int(num_envs) >= 1 << 31:
            raise ValueError(f"replay: {T} slots x {num_envs} envs >= 2^31")
        o["T"] = T
    return o


class HerReplay:
    """The buffer of one env (``env.replay``).  ``env.step`` pushes, ``env.reset`` stages and discards; ``sample``
    returns device tensors.  Every launch goes to the current stream; only ``size()`` and ``sample(check=True)`` wait for
    the device."""

    def __init__(self, env, options):
        import torch
        self.env, self.lib, self.o = env, env.lib, dict(options)
        n, T, A, d = env.num_envs, int(options["T"]), env.action_dim, env.device
        self.n, self.T, self.action_dim = n, T, A
        self.capacity = T * n
        self.n_sampled_goal = self.o["n_sampled_goal"]
        self.goal_selection_strategy = self.o["goal_selection_strategy"]
        self.her_ratio = 1.0 - 1.0 / (self.n_sampled_goal + 1)
        self.seed = env.base_seed if self.o["seed"] is None else self.o["seed"] & 0xFFFFFFFFFFFFFFFF
        f32, i32 = torch.float32, torch.int32
        z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=d)  # noqa: E731
        self.store = {"obs": z(T, n, NOBS), "next_obs": z(T, n, NOBS), "goal": z(T, n, 3), "action": z(T, n, A),
                      "reward": z(T, n), "terminated": z(T, n, dtype=torch.uint8), "offset": z(T, n, dtype=i32),
                      "length": z(T, n, dtype=i32), "meta": z(3, n, dtype=i32), "stage_obs": z(n, NOBS),
                      "stage_goal": z(n, 3), "prefix": z(n + 1, dtype=i32)}
        held = sum(t.numel() * t.element_size() for t in self.store.values())
        if held != self.lib.so100_her_storage_bytes(n, T, A):
            raise RuntimeError(f"replay: the arrays hold {held} bytes, so100_her_storage_bytes "
                               f"{self.lib.so100_her_storage_bytes(n, T, A)}")
        self.valid_lo, self.count, self.open_len = self.store["meta"]
        self._total = self.store["prefix"][n:]
        self._her = _native.SO100Her(n=n, T=T, action_dim=A, strategy=_native.HER_STRATEGIES[self.goal_selection_strategy],
                                     n_sampled_goal=self.n_sampled_goal, seed=self.seed,
                                     **{k: _native.ptr(t) for k, t in self.store.items()})
        self._mask = torch.zeros(n, dtype=torch.uint8, device=d)
        self._dirty = False         # a push or discard since the last scan (host side: nothing waits for the device)
        self.calls = 0              # sample calls so far: the draws' counter

    # ------------------------------------------------------------------ the env's hooks
    def after_reset(self, mask):
        """the reset envs (mask: the env's uint8 mask or None = all): their open episodes go, their fresh observation
        and goal are staged"""
        env = self.env
        _native.check(self.lib.so100_her_discard(env._handle, ctypes.byref(self._her), _native.ptr(mask),
                                                 _native.ptr(env.obs), _native.ptr(env.desired_goal), env._stream()),
                      "so100_her_discard")
        self._dirty = True

    def after_step(self, command):
        """one transition per env from what the step left (command: the [N, action_dim] tensor ``step`` was given)"""
        env, P = self.env, _native.ptr
        st = self.store
        step = _native.SO100HerStep(prev_obs=P(st["stage_obs"]), prev_goal=P(st["stage_goal"]), obs=P(env.obs),
                                    final_obs=P(env.final_obs), goal=P(env.desired_goal), action=P(command),
                                    reward=P(env.reward), terminated=P(env.terminated), truncated=P(env.truncated),
                                    diverged=P(env.diverged))
        _native.check(self.lib.so100_her_push(env._handle, ctypes.byref(self._her), ctypes.byref(step), env._stream()),
                      "so100_her_push")
        self._dirty = True

    # ------------------------------------------------------------------ the user's side
    def discard(self, mask=None):
        """Drop the open episodes of the envs with mask[i] true (None: all); closed episodes stay."""
        import torch
        mask_p = None
        if mask is not None:
            m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
            self._mask.copy_(m.to(self.env.device).to(torch.uint8))
            mask_p = _native.ptr(self._mask)
        _native.check(self.lib.so100_her_discard(self.env._handle, ctypes.byref(self._her), mask_p, None, None,
                                                 self.env._stream()), "so100_her_discard")
        self._dirty = True

    def _scan(self):
        if self._dirty:
            _native.check(self.lib.so100_her_scan(self.env._handle, ctypes.byref(self._her), self.env._stream()),
                          "so100_her_scan")
            self._dirty = False

    @property
    def valid_count(self):
        """the transitions a sample draws from (those of closed episodes), a device int32 tensor of one element"""
        self._scan()
        return self._total

    def size(self):
        """``valid_count`` on the host (waits for the device)"""
        return int(self.valid_count.item())

    def sample(self, batch_size, normalize=False, check=False):
        """A batch of ``batch_size`` transitions as a dict of device tensors: observation, achieved_goal, desired_goal,
        the three ``next_*``, actions, rewards, dones (terminated only), env, slot, goal_slot.  The first
        ``int(her_ratio * batch_size)`` rows carry a goal their episode achieved and the reward of it.
        normalize: the six observation tensors through ``env.normalize_obs`` (ValueError without a normaliser); rewards
        are never normalised.  check: read ``valid_count`` and raise ValueError when it is 0 (an empty buffer otherwise
        gives rows of zeros with slot -1)."""
        import torch
        B = _int("batch_size", batch_size)
        if B < 0:
            raise ValueError(f"replay: batch_size {B} must be >= 0")
        env = self.env
        if normalize and env._norm is None:
            raise ValueError("replay: sample(normalize=True) needs an env built with normalize=...")
        if check and self.size() == 0:
            raise ValueError("replay: no finished episode in the buffer yet")
        self._scan()
        d, f32, i32 = env.device, torch.float32, torch.int32
        e = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device=d)  # noqa: E731
        out = {"observation": e(B, NOBS), "achieved_goal": e(B, 3), "desired_goal": e(B, 3),
               "next_observation": e(B, NOBS), "next_achieved_goal": e(B, 3), "next_desired_goal": e(B, 3),
               "actions": e(B, self.action_dim), "rewards": e(B), "dones": e(B), "env": e(B, dtype=i32),
               "slot": e(B, dtype=i32), "goal_slot": e(B, dtype=i32)}
        rec = _native.SO100HerOut(**{k: _native.ptr(t) for k, t in out.items()})
        if B:                        # (an empty tensor has no address to hand over)
            _native.check(self.lib.so100_her_sample(env._handle, ctypes.byref(self._her), B,
                                                    ctypes.c_uint64(self.calls), ctypes.byref(rec), env._stream()),
                          "so100_her_sample")
        self.calls += 1
        if normalize:
            keys = ("observation", "achieved_goal", "desired_goal")
            out.update(env.normalize_obs({k: out[k] for k in keys}))
            nxt = env.normalize_obs({k: out["next_" + k] for k in keys})
            out.update({"next_" + k: v for k, v in nxt.items()})
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the reference's SAC("MultiInputPolicy", buffer_size=50_000, batch_size=256) on {"pixels", "agent_pos"}
# (scripts/train_sac.py): a plain DictReplayBuffer
UNIFORM_REPLAY_DEFAULTS = dict(buffer_size=None, augment=None, seed=None)
_FLT_MIN = 1.1754943508222875e-38
AUGMENT_DEFAULT_PAD = 4          # DrQ's random shift: pad by 4, crop at a random offset
# the n-step options, in a table of their own: n_step None = a buffer exactly as without them (no ``ends``, the plain
# launches); an int (1 included) = the ``_nstep`` launches and the extra sample keys.  gamma: SB3's default
UNIFORM_REPLAY_NSTEP_DEFAULTS = dict(n_step=None, gamma=0.99)
# prioritised replay, in tables of their own: prioritized None / False = a buffer exactly as without the key; True = the
# exponents below (Schaul et al.'s proportional variant); a dict with exactly those three keys = its own
UNIFORM_REPLAY_PER_DEFAULTS = dict(prioritized=None)
PER_DEFAULTS = dict(alpha=0.6, beta=0.4, eps=1e-6)


def _unit(what, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"uniform_replay: {what} {v!r} must be a number")
    v = float(v)
    if not (math.isfinite(v) and 0.0 <= v <= 1.0):
        raise ValueError(f"uniform_replay: {what} {v} must be finite and in [0, 1]")
    return v


def per_options(prioritized):
    """The checked value of ``prioritized``: None / False -> None (off), True -> ``PER_DEFAULTS``, a dict with exactly
    the keys alpha, beta (finite, in [0, 1]) and eps (finite, > 0) -> a copy with floats; ValueError otherwise."""
    if prioritized is None or prioritized is False:
        return None
    if prioritized is True:
        return dict(PER_DEFAULTS)
    if not isinstance(prioritized, dict) or set(prioritized) != set(PER_DEFAULTS):
        raise ValueError(f"uniform_replay: prioritized {prioritized!r}: None, a bool or a dict with exactly the keys "
                         f"{sorted(PER_DEFAULTS)}")
    eps = prioritized["eps"]
    if isinstance(eps, (bool, np.bool_)) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise ValueError(f"uniform_replay: eps {eps!r} must be a number")
    eps = float(np.float32(eps))                         # (as the device reads it: an eps that rounds to 0 is refused)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"uniform_replay: eps {prioritized['eps']} must be finite and > 0 in float32")
    return dict(alpha=_unit("alpha", prioritized["alpha"]), beta=_unit("beta", prioritized["beta"]),
                eps=float(prioritized["eps"]))


def nstep_window(n_step, gamma, T=None):
    """The checked (n_step, gamma) of an n-step window: n_step an int in 1..16 (and <= T - 1 when T is given), gamma a
    finite float in [0, 1]; ValueError otherwise."""
    if isinstance(n_step, (bool, np.bool_)) or not isinstance(n_step, (int, np.integer)):
        raise ValueError(f"uniform_replay: n_step {n_step!r} must be an integer")
    n_step = int(n_step)
    if not 1 <= n_step <= _native.SO100_REPLAY_MAX_NSTEP:
        raise ValueError(f"uniform_replay: n_step {n_step} outside 1..{_native.SO100_REPLAY_MAX_NSTEP}")
    if T is not None and n_step > T - 1:
        raise ValueError(f"uniform_replay: n_step {n_step} exceeds the {T - 1} transitions that {T} slots per env hold")
    if isinstance(gamma, (bool, np.bool_)) or not isinstance(gamma, (int, float, np.integer, np.floating)):
        raise ValueError(f"uniform_replay: gamma {gamma!r} must be a number")
    gamma = float(gamma)
    if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
        raise ValueError(f"uniform_replay: gamma {gamma} must be finite and in [0, 1]")
    return n_step, gamma


def augment_pad(augment):
    """The pad of an ``augment`` value: None / False -> 0 (off), True -> 4, an int -> itself, dict(pad=) -> its pad;
    ValueError for anything else and for a pad outside 0..64."""
    if augment is None or augment is False:
        return 0
    if augment is True:
        return AUGMENT_DEFAULT_PAD
    if isinstance(augment, dict):
        if set(augment) != {"pad"}:
            raise ValueError(f"uniform_replay: augment dict takes exactly the key 'pad', got {sorted(augment)}")
        augment = augment["pad"]
    if isinstance(augment, (bool, np.bool_)) or not isinstance(augment, (int, np.integer)):
        raise ValueError(f"uniform_replay: augment {augment!r}: None, a bool, an int pad or dict(pad=)")
    pad = int(augment)
    if not 0 <= pad <= _native.SO100_REPLAY_MAX_PAD:
        raise ValueError(f"uniform_replay: augment pad {pad} outside 0..{_native.SO100_REPLAY_MAX_PAD}")
    return pad


def uniform_replay_options(uniform_replay, num_envs=None, task="so100_cube_to_bin", obs_type="so100_state",
                           autoreset=True):
    """The checked options of ``SO100VecEnv(uniform_replay=...)`` as a dict (no device use): None -> None (off), a dict
    -> the defaults overridden by it, with ``pad`` (the augmentation's) and, when ``num_envs`` is given, ``T =
    buffer_size // num_envs`` (the slots per env) added.  Raises ValueError for unknown keys and bad values, and, given
    the env's arguments, for the GoalEnv (``replay=`` is its buffer), without auto-reset, for fewer than 2 slots per env
    and for an augmentation without pixel observations.  The keys ``n_step`` (1..16, at most T - 1) and ``gamma`` (finite,
    in [0, 1], default 0.99; a ValueError without ``n_step``) turn the n-step returns on: the result's ``n_step`` is None
    without them.  The key ``prioritized`` (``per_options``) turns prioritised replay on: the result's ``prioritized`` is
    None or the checked dict(alpha=, beta=, eps=)."""
    if uniform_replay is None:
        return None
    if not isinstance(uniform_replay, dict):
        raise ValueError("uniform_replay: None or a dict(" + ", ".join(f"{k}=" for k in UNIFORM_REPLAY_DEFAULTS) + ")")
    known = {**UNIFORM_REPLAY_DEFAULTS, **UNIFORM_REPLAY_NSTEP_DEFAULTS, **UNIFORM_REPLAY_PER_DEFAULTS}
    unknown = set(uniform_replay) - set(known)
    if unknown:
        raise ValueError(f"uniform_replay: unknown keys {sorted(unknown)}; known: {sorted(known)}")
    o = dict(UNIFORM_REPLAY_DEFAULTS)
    o["n_step"] = None
    o.update(UNIFORM_REPLAY_PER_DEFAULTS)
    o.update(uniform_replay)
    o["prioritized"] = per_options(o["prioritized"])
    if o["n_step"] is None:
        if "gamma" in o:
            raise ValueError("uniform_replay: gamma is the n-step window's; it needs n_step=")
    else:
        o["n_step"], o["gamma"] = nstep_window(o["n_step"], o.get("gamma", UNIFORM_REPLAY_NSTEP_DEFAULTS["gamma"]))
    if o["buffer_size"] is None:
        raise ValueError("uniform_replay: buffer_size (slots over all envs) is required")
    if isinstance(o["buffer_size"], (bool, np.bool_)) or not isinstance(o["buffer_size"], (int, np.integer)):
        raise ValueError(f"uniform_replay: buffer_size {o['buffer_size']!r} must be an integer")
    o["buffer_size"] = int(o["buffer_size"])
    if o["buffer_size"] < 1:
        raise ValueError(f"uniform_replay: buffer_size {o['buffer_size']} must be >= 1")
    o["pad"] = augment_pad(o["augment"])
    if o["seed"] is not None:
        if isinstance(o["seed"], (bool, np.bool_)) or not isinstance(o["seed"], (int, np.integer)):
            raise ValueError(f"uniform_replay: seed {o['seed']!r} must be an integer")
        o["seed"] = int(o["seed"])
    if num_envs is not None:
        if task == "so100_goal":
            raise ValueError("uniform_replay: the arm tasks' buffer; task='so100_goal' has the hindsight buffer, replay=")
        if not autoreset:
            raise ValueError("uniform_replay: needs autoreset=True (the step then hands over the finished episode's "
                             "last observation and the next episode's first)")
        T = o["buffer_size"] // int(num_envs)
        if T < 2:
            raise ValueError(f"uniform_replay: buffer_size {o['buffer_size']} // num_envs {num_envs} = {T} slots per "
                             "env; a ring needs 2 (one holds the staged observation)")
        if T * int(num_envs) >= 1 << 31:
            raise ValueError(f"uniform_replay: {T} slots x {num_envs} envs >= 2^31")
        if o["pad"] > 0 and obs_type != "so100_pixels_agent_pos":
            raise ValueError("uniform_replay: augment shifts images; it needs obs_type='so100_pixels_agent_pos'")
        if o["n_step"] is not None:
            nstep_window(o["n_step"], o["gamma"], T)
        o["T"] = T
    return o


def image_layout(shape, channels_first):
    """(planes, H, W, chan) of an env's image tensor shape [N, ...] (include/so100.h so100_replay): [H,W,3] -> (1,H,W,3),
    [3,H,W] -> (3,H,W,1), [K,H,W,3] -> (K,H,W,3), [K,3,H,W] -> (3K,H,W,1)"""
    dims = tuple(int(x) for x in shape[1:])
    if channels_first:
        return int(np.prod(dims[:-2])), dims[-2], dims[-1], 1
    return int(np.prod(dims[:-3])), dims[-3], dims[-2], dims[-1]


class UniformReplay:
    """The uniform buffer of one env (``env.uniform_replay``).  ``env.step`` pushes, ``env.reset`` stages; ``sample``
    returns device tensors.  Every launch goes to the current stream; only ``size()`` and ``sample(check=True)`` wait for
    the device."""

    def __init__(self, env, options):
        import torch
        self.env, self.lib, self.o = env, env.lib, dict(options)
        n, T, A, d = env.num_envs, int(options["T"]), env.action_dim, env.device
        self.n, self.T, self.action_dim = n, T, A
        self.capacity = (T - 1) * n                     # the slot at each env's cursor holds half a transition
        self.pad = int(self.o["pad"])
        self.seed = env.base_seed if self.o["seed"] is None else self.o["seed"] & 0xFFFFFFFFFFFFFFFF
        self.image_shape = None if env.pixels is None else tuple(env.pixels.shape[1:])
        layout = (0, 0, 0, 0) if env.pixels is None else image_layout(env.pixels.shape, env.channels_first)
        self.layout = layout
        self.P = P = int(np.prod(layout)) if env.pixels is not None else 0
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=d)  # noqa: E731
        self.store = {"obs": z(T, n, NOBS), "next_obs": z(T, n, NOBS), "action": z(T, n, A), "reward": z(T, n),
                      "terminated": z(T, n, dtype=u8), "meta": z(2, n, dtype=i32), "prefix": z(n + 1, dtype=i32)}
        if P:
            self.store["obs_img"] = z(T, n, P, dtype=u8)
            self.store["next_img"] = z(T, n, P, dtype=u8)
        held = sum(t.numel() * t.element_size() for t in self.store.values())
        want = self.lib.so100_replay_storage_bytes(n, T, A, P)
        if held != want:
            raise RuntimeError(f"uniform_replay: the arrays hold {held} bytes, so100_replay_storage_bytes {want}")
        self.n_step, self.gamma = self.o.get("n_step"), self.o.get("gamma")
        self._nstep = None          # the n-step record: None = the plain launches, no `ends`
        if self.n_step is not None:
            self.ends = z(T, n, dtype=u8)
            if self.ends.numel() != self.lib.so100_replay_nstep_storage_bytes(n, T):
                raise RuntimeError(f"uniform_replay: ends holds {self.ends.numel()} bytes, "
                                   f"so100_replay_nstep_storage_bytes {self.lib.so100_replay_nstep_storage_bytes(n, T)}")
            self._nstep = _native.SO100ReplayNstep(n_step=self.n_step, gamma=self.gamma, ends=_native.ptr(self.ends))
        self.prioritized = self.o.get("prioritized")
        self._per = None            # the priorities' record: None = the uniform pick, none of the three arrays
        if self.prioritized is not None:
            # (not in `store`: so100_replay_storage_bytes counts that)
            self.prio = z(T, n, dtype=torch.int32)       # uint32 fixed point on the device; read it through prio_u32()
            self.prio_sum = z(n + 1, dtype=torch.int64)  # uint64 on the device, < 2^63
            self.max_prio = torch.tensor([_native.SO100_REPLAY_PRIO_ONE, 0], dtype=i32, device=d)
            held = sum(t.numel() * t.element_size() for t in (self.prio, self.prio_sum, self.max_prio))
            want = self.lib.so100_replay_per_storage_bytes(n, T)
            if held != want:
                raise RuntimeError(f"uniform_replay: the priorities hold {held} bytes, so100_replay_per_storage_bytes "
                                   f"{want}")
            self.alpha, self.beta, self.eps = (self.prioritized[k] for k in ("alpha", "beta", "eps"))
            self._per = self._per_record(self.beta)
            self._per_dirty = False  # a push or an update since the last priority scan (host side)
        self.cursor, self.count = self.store["meta"]
        self._total = self.store["prefix"][n:]
        self._rec = _native.SO100Replay(n=n, T=T, action_dim=A, planes=layout[0], H=layout[1], W=layout[2],
                                        chan=layout[3], P=P, pad=0, seed=self.seed,
                                        **{k: _native.ptr(t) for k, t in self.store.items()})
        self._dirty = False         # a push since the last scan (host side: nothing waits for the device)
        self.calls = 0              # sample calls so far: the draws' counter

    def _per_record(self, beta):
        return _native.SO100ReplayPer(alpha=self.alpha, beta=beta, eps=self.eps, prio=_native.ptr(self.prio),
                                      sum=_native.ptr(self.prio_sum), max_prio=_native.ptr(self.max_prio))

    def prio_u32(self):
        """the priorities as their unsigned values, an int64 [T, n] device tensor (a copy)"""
        return self.prio.to(self.prio_sum.dtype) & 0xFFFFFFFF

    # ------------------------------------------------------------------ the env's hooks
    def after_reset(self, mask):
        """the reset envs (mask: the env's uint8 mask or None = all): their fresh observation and image are staged at
        their cursors (a stage moves no cursor, so the priorities stay)"""
        env = self.env
        if self._nstep is not None:
            _native.check(self.lib.so100_replay_stage_nstep(env._handle, ctypes.byref(self._rec),
                                                            ctypes.byref(self._nstep), _native.ptr(mask),
                                                            _native.ptr(env.obs), _native.ptr(env.pixels),
                                                            env._stream()), "so100_replay_stage_nstep")
            return
        _native.check(self.lib.so100_replay_stage(env._handle, ctypes.byref(self._rec), _native.ptr(mask),
                                                  _native.ptr(env.obs), _native.ptr(env.pixels), env._stream()),
                      "so100_replay_stage")

    def after_step(self, command):
        """one transition per env from what the step left (command: the [N, action_dim] tensor ``step`` copied into)"""
        env, P = self.env, _native.ptr
        step = _native.SO100ReplayStep(obs=P(env.obs), final_obs=P(env.final_obs), action=P(command),
                                       reward=P(env.reward), terminated=P(env.terminated), truncated=P(env.truncated),
                                       diverged=P(env.diverged), pixels=P(env.pixels), final_pixels=P(env.final_pixels))
        if self._per is not None:
            _native.check(self.lib.so100_replay_push_per(env._handle, ctypes.byref(self._rec), ctypes.byref(self._per),
                                                         None if self._nstep is None else ctypes.byref(self._nstep),
                                                         ctypes.byref(step), env._stream()), "so100_replay_push_per")
            self._per_dirty = True
        elif self._nstep is not None:
            _native.check(self.lib.so100_replay_push_nstep(env._handle, ctypes.byref(self._rec),
                                                           ctypes.byref(self._nstep), ctypes.byref(step),
                                                           env._stream()), "so100_replay_push_nstep")
        else:
            _native.check(self.lib.so100_replay_push(env._handle, ctypes.byref(self._rec), ctypes.byref(step),
                                                     env._stream()), "so100_replay_push")
        self._dirty = True

    # ------------------------------------------------------------------ the user's side
    def _scan(self):
        if self._dirty:
            _native.check(self.lib.so100_replay_scan(self.env._handle, ctypes.byref(self._rec), self.env._stream()),
                          "so100_replay_scan")
            self._dirty = False
        if self._per is not None and self._per_dirty:
            _native.check(self.lib.so100_replay_per_scan(self.env._handle, ctypes.byref(self._rec),
                                                         ctypes.byref(self._per), self.env._stream()),
                          "so100_replay_per_scan")
            self._per_dirty = False

    @property
    def valid_count(self):
        """the transitions a sample draws from, a device int32 tensor of one element"""
        self._scan()
        return self._total

    def size(self):
        """``valid_count`` on the host (waits for the device)"""
        return int(self.valid_count.item())

    def update_priorities(self, env, slot, td_abs):
        """The priorities of the transitions (env[j], slot[j]) from |TD error| td_abs[j]: device tensors of one length
        (int32, int32, float32; other dtypes are converted), usually a batch's ``env`` and ``slot``.  q = (|td| +
        eps)^alpha in fixed point; a slot named more than once takes the greatest; rows whose transition has left the
        ring since (and the slot -1 of an empty-buffer row) are skipped, a slot overwritten since takes the value.
        Nothing waits for the device.  ValueError on a buffer built without ``prioritized``."""
        import torch
        if self._per is None:
            raise ValueError("uniform_replay: update_priorities needs a buffer built with prioritized=")
        d = self.env.device
        cols = [torch.as_tensor(t, device=d).reshape(-1).to(dt).contiguous()
                for t, dt in ((env, torch.int32), (slot, torch.int32), (td_abs, torch.float32))]
        B = cols[0].numel()
        if cols[1].numel() != B or cols[2].numel() != B:
            raise ValueError(f"uniform_replay: update_priorities takes three tensors of one length, got "
                             f"{[c.numel() for c in cols]}")
        if B:
            _native.check(self.lib.so100_replay_per_update(self.env._handle, ctypes.byref(self._rec),
                                                           ctypes.byref(self._per), B, *[_native.ptr(c) for c in cols],
                                                           self.env._stream()), "so100_replay_per_update")
            self._per_dirty = True

    def sample(self, batch_size, augment=None, normalize=False, check=False, n_step=None, gamma=None, beta=None):
        """A batch of ``batch_size`` transitions as a dict of device tensors.  Pixel env: ``pixels`` / ``next_pixels``
        ([B, *env.pixels.shape[1:]] uint8), ``agent_pos`` / ``next_agent_pos`` (columns 9:15 of the state rows) and
        ``state`` / ``next_state`` (the 15-float rows); state env: ``obs`` / ``next_obs``.  Both: ``actions``,
        ``rewards``, ``dones`` (terminated only), ``env``, ``slot``, ``shift`` ([B, 4]: dx, dy of the image and of the
        next image; the pad where nothing is shifted).
        augment: None -> the buffer's option; False -> the stored images; True, an int or dict(pad=) as in the options.
        normalize: ``agent_pos`` (or ``obs``) and its ``next_`` twin through ``env.normalize_obs`` (ValueError without a
        normaliser); images and rewards are never touched.  check: read ``valid_count`` and raise ValueError when it is
        0 (an empty buffer otherwise gives rows of zeros with slot -1).
        A buffer built with ``n_step`` also returns ``discounts`` (gamma^m, the factor of the bootstrap value),
        ``n_steps`` (m, the transitions of the row's window) and ``last_slot``; ``rewards`` is then the discounted sum
        over the window, and ``dones`` and the ``next_`` entries are those of its last transition.  n_step, gamma:
        another window for this call (the ``ends`` bytes are stored regardless); ValueError on a buffer built without
        ``n_step``.
        A buffer built with ``prioritized`` draws each row with probability ``probs`` (its priority over the sum) and
        also returns ``weights``, the importance weights (count * probs)^-beta divided by the batch's greatest.  beta:
        another exponent for this call (annealing); ValueError on a buffer built without ``prioritized``."""
        import torch
        B = _int("batch_size", batch_size)
        if B < 0:
            raise ValueError(f"uniform_replay: batch_size {B} must be >= 0")
        env = self.env
        if self._nstep is None:
            if n_step is not None or gamma is not None:
                raise ValueError("uniform_replay: sample(n_step=, gamma=) needs a buffer built with n_step=")
        else:
            window = nstep_window(self.n_step if n_step is None else n_step, self.gamma if gamma is None else gamma,
                                  self.T)
        if self._per is None:
            if beta is not None:
                raise ValueError("uniform_replay: sample(beta=) needs a buffer built with prioritized=")
        else:
            beta = self.beta if beta is None else _unit("beta", beta)
        pad = self.pad if augment is None else augment_pad(augment)
        if pad > 0 and not self.P:
            raise ValueError("uniform_replay: augment shifts images; it needs obs_type='so100_pixels_agent_pos'")
        if normalize and env._norm is None:
            raise ValueError("uniform_replay: sample(normalize=True) needs an env built with normalize=...")
        if check and self.size() == 0:
            raise ValueError("uniform_replay: no transition in the buffer yet")
        self._scan()
        d, f32, i32 = env.device, torch.float32, torch.int32
        e = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device=d)  # noqa: E731
        raw = {"obs": e(B, NOBS), "next_obs": e(B, NOBS), "actions": e(B, self.action_dim), "rewards": e(B),
               "dones": e(B), "env": e(B, dtype=i32), "slot": e(B, dtype=i32), "shift": e(B, 4, dtype=i32)}
        if self.P:
            raw["pixels"] = e(B, *self.image_shape, dtype=torch.uint8)
            raw["next_pixels"] = e(B, *self.image_shape, dtype=torch.uint8)
        rec = _native.SO100ReplayOut(**{k: _native.ptr(t) for k, t in raw.items()})
        if self._per is not None:
            more = {"discounts": e(B), "nsteps": e(B, dtype=i32), "last_slot": e(B, dtype=i32)} \
                if self._nstep is not None else {}
            pout = {"probs": e(B), "weights": e(B)}
            if B:
                self._rec.pad = pad
                ns = nrec = None
                if self._nstep is not None:
                    ns = ctypes.byref(_native.SO100ReplayNstep(n_step=window[0], gamma=window[1],
                                                               ends=_native.ptr(self.ends)))
                    nrec = ctypes.byref(_native.SO100ReplayNstepOut(**{k: _native.ptr(t) for k, t in more.items()}))
                prec = _native.SO100ReplayPerOut(**{k: _native.ptr(t) for k, t in pout.items()})
                per = self._per_record(beta)
                _native.check(self.lib.so100_replay_sample_per(env._handle, ctypes.byref(self._rec), ctypes.byref(per),
                                                               ns, B, ctypes.c_uint64(self.calls), ctypes.byref(rec),
                                                               nrec, ctypes.byref(prec), env._stream()),
                              "so100_replay_sample_per")
            if more:
                raw["discounts"], raw["n_steps"], raw["last_slot"] = more["discounts"], more["nsteps"], more["last_slot"]
            # the common batch-max normalisation: two ops, no synchronisation (an empty buffer's zeros stay zeros)
            raw["probs"] = pout["probs"]
            raw["weights"] = pout["weights"] / pout["weights"].max().clamp_min(_FLT_MIN) if B else pout["weights"]
        elif self._nstep is not None:
            more = {"discounts": e(B), "nsteps": e(B, dtype=i32), "last_slot": e(B, dtype=i32)}
            if B:
                self._rec.pad = pad
                ns = _native.SO100ReplayNstep(n_step=window[0], gamma=window[1], ends=_native.ptr(self.ends))
                nrec = _native.SO100ReplayNstepOut(**{k: _native.ptr(t) for k, t in more.items()})
                _native.check(self.lib.so100_replay_sample_nstep(env._handle, ctypes.byref(self._rec), ctypes.byref(ns),
                                                                 B, ctypes.c_uint64(self.calls), ctypes.byref(rec),
                                                                 ctypes.byref(nrec), env._stream()),
                              "so100_replay_sample_nstep")
            raw["discounts"], raw["n_steps"], raw["last_slot"] = more["discounts"], more["nsteps"], more["last_slot"]
        elif B:                      # (an empty tensor has no address to hand over)
            self._rec.pad = pad
            _native.check(self.lib.so100_replay_sample(env._handle, ctypes.byref(self._rec), B,
                                                       ctypes.c_uint64(self.calls), ctypes.byref(rec), env._stream()),
                          "so100_replay_sample")
        self.calls += 1
        if not self.P:
            out = raw
            if normalize:
                out["obs"], out["next_obs"] = env.normalize_obs(out["obs"]), env.normalize_obs(out["next_obs"])
            return out
        out = {k: v for k, v in raw.items() if k not in ("obs", "next_obs")}
        out["state"], out["next_state"] = raw["obs"], raw["next_obs"]
        out["agent_pos"], out["next_agent_pos"] = raw["obs"][:, 9:15], raw["next_obs"][:, 9:15]
        if normalize:
            out["agent_pos"] = env.normalize_obs({"agent_pos": out["agent_pos"]})["agent_pos"]
            out["next_agent_pos"] = env.normalize_obs({"agent_pos": out["next_agent_pos"]})["agent_pos"]
        return out
