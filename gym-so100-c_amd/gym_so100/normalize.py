"""Running observation / reward normalisation on the device: SB3 ``VecNormalize``'s semantics, the
statistics in float64 on the GPU, updated and applied by the launches of csrc/so100_norm.hip with no host
synchronisation.  ``SO100VecEnv(normalize=...)`` owns one ``Normalizer``; this module also holds the option checks and
the host-side merge of shards' statistics, neither of which touches a device."""
import ctypes

import numpy as np

from . import _native

NORMALIZE_DEFAULTS = dict(obs=True, reward=False, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                          training=True)
COUNT0 = 1e-4            # the count the statistics start with (mean 0, variance 1), SB3's RunningMeanStd(epsilon=1e-4)


def normalize_options(normalize):
    """The checked options of ``SO100VecEnv(normalize=...)`` as a dict (no device use): None / False -> None (off),
    True -> NORMALIZE_DEFAULTS (the reference scripts' VecNormalize(norm_obs=True, norm_reward=False, clip_obs=10)), a
    dict -> the defaults overridden by it.  ``gamma=None`` keeps no discounted return (then ``reward`` must be off).
    Raises ValueError for unknown keys and for what the entry points refuse."""
    if normalize is None or normalize is False:
        return None
    if normalize is True:
        return dict(NORMALIZE_DEFAULTS)
    if not isinstance(normalize, dict):
        raise ValueError("normalize: None, True or a dict(" + ", ".join(f"{k}=" for k in NORMALIZE_DEFAULTS) + ")")
    unknown = set(normalize) - set(NORMALIZE_DEFAULTS)
    if unknown:
        raise ValueError(f"normalize: unknown keys {sorted(unknown)}; known: {sorted(NORMALIZE_DEFAULTS)}")
    o = dict(NORMALIZE_DEFAULTS)
    o.update(normalize)
    for k in ("obs", "reward", "training"):
        if not isinstance(o[k], (bool, np.bool_)):
            raise ValueError(f"normalize: {k} {o[k]!r} must be True or False")
        o[k] = bool(o[k])
    for k in ("clip_obs", "clip_reward", "epsilon"):
        try:
            v = float(o[k])
        except (TypeError, ValueError):
            raise ValueError(f"normalize: {k} {o[k]!r} is not a number") from None
        if isinstance(o[k], bool) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"normalize: {k} {o[k]!r} must be finite and > 0")
        o[k] = v
    if o["gamma"] is not None:
        try:
            g = float(o["gamma"])
        except (TypeError, ValueError):
            raise ValueError(f"normalize: gamma {o['gamma']!r} is not a number") from None
        if isinstance(o["gamma"], bool) or not (0.0 < g <= 1.0):
            raise ValueError(f"normalize: gamma {o['gamma']!r} must lie in (0, 1]")
        o["gamma"] = g
    elif o["reward"]:
        raise ValueError("normalize: reward=True needs a discount gamma (the return's variance scales the reward)")
    return o


class RunningStats:
    """mean / var / count of one normalised key as float64 numpy (a copy: what ``obs_rms[key]`` / ``ret_rms`` return)."""

    def __init__(self, mean, var, count):
        self.mean = np.array(mean, dtype=np.float64)
        self.var = np.array(var, dtype=np.float64)
        self.count = float(count)

    def __repr__(self):
        return f"RunningStats(mean={self.mean!r}, var={self.var!r}, count={self.count!r})"


def _combine(mean, var, count, bm, bv, b):
    """the update formula (include/so100.h) with a batch of mean bm, population variance bv and b rows"""
    if b == 0:
        return mean, var, count
    delta = bm - mean
    tot = count + b
    return mean + delta * b / tot, (var * count + bv * b + delta * delta * count * b / tot) / tot, tot


def _without_prior(mean, var, count):
    """(batch mean, batch variance, rows) of the data in statistics that started from (0, 1, COUNT0): the update formula
    solved for its batch"""
    b = count - COUNT0
    if abs(b - round(b)) < 1e-6:
        b = float(round(b))                 # whole rows
    if b <= 0:
        return np.zeros_like(mean), np.zeros_like(var), 0.0
    bm = mean * count / b
    bv = (var * count - COUNT0 - bm * bm * COUNT0 * b / count) / b
    return bm, np.maximum(bv, 0.0), b


def merge_normalize_states(states):
    """Combine shards' ``normalize_state()`` dicts into one, on the host, by the update formula: the result is the
    statistics one env over all the shards' rows would hold (each shard's starting count of 1e-4 is taken out before its
    data is added, so the start is counted once).  The options are the first shard's.  No collective: each rank saves
    or sends its state, one rank merges."""
    states = list(states)
    if not states:
        raise ValueError("merge_normalize_states: no states")
    keys = sorted(k[:-5] for k in states[0] if k.endswith(".mean"))
    for s in states[1:]:
        if sorted(k[:-5] for k in s if k.endswith(".mean")) != keys:
            raise ValueError("merge_normalize_states: the states normalise different keys")
    out = {k: np.array(v) for k, v in states[0].items()}
    for key in keys:
        first = states[0]
        mean = np.array(first[key + ".mean"], dtype=np.float64)
        var = np.array(first[key + ".var"], dtype=np.float64)
        count = float(first[key + ".count"])
        for s in states[1:]:
            bm, bv, b = _without_prior(np.asarray(s[key + ".mean"], dtype=np.float64),
                                       np.asarray(s[key + ".var"], dtype=np.float64), float(s[key + ".count"]))
            mean, var, count = _combine(mean, var, count, bm, bv, b)
        out[key + ".mean"], out[key + ".var"], out[key + ".count"] = mean, var, np.float64(count)
    return out


class _ObsRms(dict):
    """key -> RunningStats, read from the device when ``env.obs_rms`` was evaluated"""


class Normalizer:
    """The device state and launches of one env's normalisation.  ``keys``: (name, source tensor, column offset, dim)
    per normalised key, in the order of the statistics' columns; each key's normalised rows go to ``out[name]``
    ([N, dim] float32), the final observation's (the first key only, auto-reset) to ``final_out``."""

    def __init__(self, env, options, keys, final_src=None):
        import torch
        self.env = env
        self.lib = env.lib
        self.o = dict(options)
        self.training = self.o.pop("training")
        n, d = env.num_envs, env.device
        self.n = n
        self.keys = [(name, src, int(off), int(dim)) for name, src, off, dim in keys]
        self.D = sum(k[3] for k in self.keys)
        if self.D > _native.SO100_NORM_MAX_DIM or len(self.keys) > _native.SO100_NORM_MAX_SRC:
            raise ValueError("normalize: more columns or keys than one call carries")
        self.cols = {}
        c = 0
        for name, _, _, dim in self.keys:
            self.cols[name] = (c, c + dim)
            c += dim
        f64 = torch.float64
        self.stats = self._fresh(torch, d)
        self.ret_stats = self._fresh(torch, d)
        self.work = torch.zeros(self.lib.so100_norm_work_bytes(n) // 8, dtype=f64, device=d)
        self.out = {name: torch.zeros(n, dim, dtype=torch.float32, device=d) for name, _, _, dim in self.keys} \
            if self.o["obs"] else {}
        self.final_src = final_src
        self.final_out = None
        if self.o["obs"] and final_src is not None:
            self.final_out = torch.zeros(n, self.keys[0][3], dtype=torch.float32, device=d)
        self.track_ret = self.o["gamma"] is not None
        self.ret = torch.zeros(n, dtype=f64, device=d) if self.track_ret else None
        self.reward_norm = torch.zeros(n, dtype=torch.float32, device=d) if self.o["reward"] else None
        self._done = torch.zeros(n, dtype=torch.uint8, device=d)
        self._done_bool = self._done.view(torch.bool)
        P = _native.ptr
        self._norm = _native.SO100Norm(
            [(src.data_ptr(), src.shape[1], off, dim, self.out[name].data_ptr() if self.out else None, dim)
             for name, src, off, dim in self.keys], epsilon=self.o["epsilon"], clip=self.o["clip_obs"])
        self._final = None
        if self.final_out is not None:
            name, _, off, dim = self.keys[0]
            self._final = _native.SO100Norm([(final_src.data_ptr(), final_src.shape[1], off, dim,
                                              self.final_out.data_ptr(), dim)], epsilon=self.o["epsilon"],
                                            clip=self.o["clip_obs"])
        self._ret_args = {}
        if self.track_ret:
            for training in (False, True):
                flags = (_native.SO100_NORM_RET_UPDATE if training else 0) | \
                    (_native.SO100_NORM_RET_NORMALIZE if self.o["reward"] else 0)
                self._ret_args[training] = _native.SO100NormRet(flags=flags, gamma=self.o["gamma"],
                                                                epsilon=self.o["epsilon"], clip=self.o["clip_reward"])
        self._p = dict(stats=P(self.stats), ret_stats=P(self.ret_stats), work=P(self.work), done=P(self._done),
                       ret=P(self.ret), reward_norm=P(self.reward_norm))

    @staticmethod
    def _fresh(torch, device):
        s = torch.zeros(3, _native.SO100_NORM_MAX_DIM, dtype=torch.float64, device=device)
        s[1].fill_(1.0)
        s[2].fill_(COUNT0)
        return s

    # ------------------------------------------------------------------ the launches of a step / a reset
    def after_step(self):
        """steps 2-6 of a step (the order of DESIGN.md §3.10), on the current stream"""
        env, lib, p = self.env, self.lib, self._p
        s = env._stream()
        if self.o["obs"]:
            if self.training:
                _native.check(lib.so100_norm_update(env._handle, ctypes.byref(self._norm), self.n, None, p["stats"],
                                                    p["work"], s), "so100_norm_update")
            _native.check(lib.so100_norm_apply(env._handle, ctypes.byref(self._norm), self.n, None, p["stats"], s),
                          "so100_norm_apply")
            if self._final is not None:
                import torch
                torch.logical_or(env.terminated, env.truncated, out=self._done_bool)
                _native.check(lib.so100_norm_apply(env._handle, ctypes.byref(self._final), self.n, p["done"],
                                                   p["stats"], s), "so100_norm_apply")
        if self.track_ret:
            _native.check(lib.so100_norm_return(env._handle, ctypes.byref(self._ret_args[bool(self.training)]), self.n,
                                                _native.ptr(env.reward), _native.ptr(env.terminated),
                                                _native.ptr(env.truncated), p["ret"], p["ret_stats"], p["work"],
                                                p["reward_norm"], s), "so100_norm_return")

    def after_reset(self, mask):
        """ret <- 0 for the reset envs, one update with their observations (mask: the env's uint8 mask or None), then
        normalise every row"""
        env, lib, p = self.env, self.lib, self._p
        if self.track_ret:
            if mask is None:
                self.ret.zero_()
            else:
                self.ret.masked_fill_(mask.ne(0), 0.0)
        if self.o["obs"]:
            s = env._stream()
            if self.training:
                _native.check(lib.so100_norm_update(env._handle, ctypes.byref(self._norm), self.n, _native.ptr(mask),
                                                    p["stats"], p["work"], s), "so100_norm_update")
            _native.check(lib.so100_norm_apply(env._handle, ctypes.byref(self._norm), self.n, None, p["stats"], s),
                          "so100_norm_apply")

    # ------------------------------------------------------------------ normalise / unnormalise given tensors
    def transform(self, x, inverse=False):
        """x: a dict by key, or one tensor for the first key (device tensors, [M, dim]); returns new tensors"""
        if isinstance(x, dict):
            return {k: (self._transform_one(k, v, inverse) if k in self.cols else v) for k, v in x.items()}
        return self._transform_one(self.keys[0][0], x, inverse)

    def _transform_one(self, key, x, inverse):
        import torch
        c0, c1 = self.cols[key]
        dim = c1 - c0
        x = torch.as_tensor(x, dtype=torch.float32, device=self.env.device)
        shape = x.shape
        if shape[-1] != dim:
            raise ValueError(f"{key}: last dimension {shape[-1]}, expected {dim}")
        x = x.reshape(-1, dim).contiguous()
        y = torch.empty_like(x)
        if x.shape[0]:
            # this key's columns of the statistics: the rows of `stats` offset by its first column
            stats = ctypes.c_void_p(self.stats.data_ptr() + 8 * c0)
            nm = _native.SO100Norm([(x.data_ptr(), dim, 0, dim, y.data_ptr(), dim)], epsilon=self.o["epsilon"],
                                   clip=self.o["clip_obs"], flags=_native.SO100_NORM_INVERSE if inverse else 0)
            _native.check(self.lib.so100_norm_apply(self.env._handle, ctypes.byref(nm), x.shape[0], None, stats,
                                                    self.env._stream()), "so100_norm_apply")
        return y.reshape(shape)

    # ------------------------------------------------------------------ statistics on the host
    def obs_rms(self):
        s = self.stats.cpu().numpy()
        return _ObsRms((name, RunningStats(s[0, c0:c1], s[1, c0:c1], s[2, c0])) for name, (c0, c1) in self.cols.items())

    def ret_rms(self):
        s = self.ret_stats.cpu().numpy()
        return RunningStats(s[0, 0], s[1, 0], s[2, 0])

    def set_obs_rms(self, rms):
        import torch
        s = self.stats.cpu().numpy().copy()
        if not hasattr(rms, "items"):                # one object with mean / var / count (ours, or SB3's RunningMeanStd)
            if not all(hasattr(rms, a) for a in ("mean", "var", "count")):
                raise ValueError("obs_rms: a mapping key -> statistics, or one object with .mean, .var and .count")
            rms = {self.keys[0][0]: rms}
        for name, r in rms.items():
            if name not in self.cols:
                raise ValueError(f"obs_rms: unknown key {name!r}; this env normalises {sorted(self.cols)}")
            c0, c1 = self.cols[name]
            mean, var = np.asarray(r.mean, dtype=np.float64).reshape(-1), np.asarray(r.var, dtype=np.float64).reshape(-1)
            if mean.shape != (c1 - c0,) or var.shape != (c1 - c0,):
                raise ValueError(f"obs_rms[{name!r}]: mean / var of {c1 - c0} columns expected")
            s[0, c0:c1], s[1, c0:c1], s[2, c0:c1] = mean, var, float(r.count)
        self.stats.copy_(torch.from_numpy(s))

    def set_ret_rms(self, r):
        import torch
        s = self.ret_stats.cpu().numpy().copy()
        s[0, 0], s[1, 0] = np.asarray(r.mean).reshape(-1)[0], np.asarray(r.var).reshape(-1)[0]
        s[2, 0] = float(r.count)
        self.ret_stats.copy_(torch.from_numpy(s))

    def state(self):
        out = {}
        for name, r in self.obs_rms().items():
            out[name + ".mean"], out[name + ".var"], out[name + ".count"] = r.mean, r.var, np.float64(r.count)
        r = self.ret_rms()
        out["ret.mean"], out["ret.var"], out["ret.count"] = r.mean, r.var, np.float64(r.count)
        out["norm_obs"], out["norm_reward"] = np.bool_(self.o["obs"]), np.bool_(self.o["reward"])
        out["clip_obs"], out["clip_reward"] = np.float64(self.o["clip_obs"]), np.float64(self.o["clip_reward"])
        out["gamma"] = np.float64(np.nan if self.o["gamma"] is None else self.o["gamma"])
        out["epsilon"] = np.float64(self.o["epsilon"])
        return out

    def set_state(self, state):
        names = sorted(k[:-5] for k in state.keys() if k.endswith(".mean") and k != "ret.mean")
        if names != sorted(self.cols):
            raise ValueError(f"set_normalize_state: the state normalises {names}, this env {sorted(self.cols)}")
        self.set_obs_rms({k: RunningStats(state[k + ".mean"], state[k + ".var"], float(state[k + ".count"]))
                          for k in names})
        if "ret.mean" in state.keys():
            self.set_ret_rms(RunningStats(state["ret.mean"], state["ret.var"], float(state["ret.count"])))
