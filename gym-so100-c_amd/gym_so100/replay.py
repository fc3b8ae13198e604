"""A hindsight replay buffer for the GoalEnv on the device: SB3 ``HerReplayBuffer``'s semantics, the
transitions kept where the step produces them, pushed, scanned and sampled by the launches of csrc/so100_her.hip with no
host synchronisation.  ``SO100VecEnv(replay=...)`` owns one ``HerReplay`` (``env.replay``); this module also holds the
option checks, which touch no device."""
import ctypes

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
