"""Float64 numpy restatement of the running normaliser (include/so100.h so100_norm_update / so100_norm_apply /
so100_norm_return), written from the formulas, not from the kernels: SB3 VecNormalize's semantics.
Used by tests/test_norm_cpu.py and tests/test_gpu_norm.py."""
import numpy as np

COUNT0 = 1e-4
MAX_DIM = 32


class RunningMeanStd:
    """mean, var, count per column; starts at 0, 1, 1e-4"""

    def __init__(self, dim):
        self.mean = np.zeros(dim, dtype=np.float64)
        self.var = np.ones(dim, dtype=np.float64)
        self.count = COUNT0
        self.updates = 0              # T of the tests' bars

    def copy(self):
        r = RunningMeanStd(self.mean.shape[0])
        r.mean, r.var, r.count, r.updates = self.mean.copy(), self.var.copy(), self.count, self.updates
        return r

    def update(self, x, mask=None):
        """x: [rows, dim]; mask: [rows] or None.  An empty batch leaves everything untouched."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.mean.shape[0])
        if mask is not None:
            x = x[np.asarray(mask).astype(bool)]
        b = x.shape[0]
        if b == 0:
            return
        bm = x.mean(axis=0)
        bv = ((x - bm) ** 2).mean(axis=0)            # population variance
        self.update_from_moments(bm, bv, b)

    def update_from_moments(self, bm, bv, b):
        delta = bm - self.mean
        tot = self.count + b
        self.mean = self.mean + delta * b / tot
        self.var = (self.var * self.count + bv * b + delta ** 2 * self.count * b / tot) / tot
        self.count = tot
        self.updates += 1


def normalize(x, rms, clip=10.0, epsilon=1e-8):
    """float64: clip((x - mean) / sqrt(var + epsilon), -clip, clip)"""
    return np.clip((np.asarray(x, dtype=np.float64) - rms.mean) / np.sqrt(rms.var + epsilon), -clip, clip)


def unnormalize(y, rms, epsilon=1e-8):
    return np.asarray(y, dtype=np.float64) * np.sqrt(rms.var + epsilon) + rms.mean


def spacing32(v):
    """the float32 spacing at |v| (float64 array)"""
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def apply_bar(x, rms, y_ref, epsilon=1e-8):
    """the per-element bar of the apply kernel against y_ref: rounding of mean and of the scale to float32, one subtract,
    one multiply"""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 * (spacing32(np.maximum(np.abs(x), np.abs(rms.mean))) / np.sqrt(rms.var + epsilon) + spacing32(y_ref))


def mean_bar(x_all):
    """|d mean| <= T n 2^-52 mean_i|x_i| per column: T updates of n rows each, the mean over the T n rows that entered
    the statistics (x_all: all of them), which is 2^-52 sum|x| (and the sum of the updates' own bars when their row
    counts differ): the worst-case float64 summation bound of any order, doubled for the merge arithmetic."""
    x_all = np.asarray(x_all, dtype=np.float64)
    return 2.0 ** -52 * np.abs(x_all).sum(axis=0)


def var_bar(x_all):
    """|d var| <= T n 2^-51 mean_i(x_i^2) = 2^-51 sum x^2"""
    x_all = np.asarray(x_all, dtype=np.float64)
    return 2.0 ** -51 * (x_all ** 2).sum(axis=0)


class VecNormalizeRef:
    """The env-level order over recorded raw data.  keys: {name: dim}."""

    def __init__(self, keys, n, obs=True, reward=False, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                 training=True, record=True):
        self.rms = {k: RunningMeanStd(d) for k, d in keys.items()}
        self.ret_rms = RunningMeanStd(1)
        self.ret = np.zeros(n, dtype=np.float64)
        self.norm_obs, self.norm_reward = obs, reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.training = training
        self.record = record                       # keep the rows that entered each key's statistics (the bars)
        self.seen = {k: [] for k in keys}
        self.ret_seen = []

    def _norm(self, obs):
        if not self.norm_obs:
            return {k: np.asarray(v, dtype=np.float64) for k, v in obs.items()}
        return {k: normalize(v, self.rms[k], self.clip_obs, self.epsilon) for k, v in obs.items()}

    def reset(self, obs, mask=None):
        """obs: {name: [n, dim]} raw, of every env after the reset; mask: the reset envs (None = all)"""
        if mask is None:
            self.ret[:] = 0.0
        else:
            self.ret[np.asarray(mask).astype(bool)] = 0.0
        if self.training and self.norm_obs:
            for k, v in obs.items():
                rows = np.asarray(v, dtype=np.float64) if mask is None else \
                    np.asarray(v, dtype=np.float64)[np.asarray(mask).astype(bool)]
                if rows.shape[0] and self.record:
                    self.seen[k].append(rows)
                self.rms[k].update(rows)
        return self._norm(obs)

    def step(self, obs, reward, terminated, truncated, final=None):
        """raw outputs of one step -> (normalised obs, normalised reward or the raw one, normalised final obs or None)"""
        if self.training and self.norm_obs:
            for k, v in obs.items():
                if self.record:
                    self.seen[k].append(np.asarray(v, dtype=np.float64))
                self.rms[k].update(v)
        out = self._norm(obs)
        fin = None if final is None else self._norm(final)
        reward = np.asarray(reward, dtype=np.float64)
        if self.gamma is not None:
            if self.training:
                self.ret = self.ret * self.gamma + reward
                if self.record:
                    self.ret_seen.append(self.ret.reshape(-1, 1).copy())
                self.ret_rms.update(self.ret.reshape(-1, 1))
        r = reward
        if self.norm_reward:
            r = np.clip(reward / np.sqrt(self.ret_rms.var[0] + self.epsilon), -self.clip_reward, self.clip_reward)
        if self.gamma is not None:
            self.ret[np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)] = 0.0
        return out, r, fin
