"""A plain numpy / Python-int restatement of prioritised replay in the uniform replay buffer (include/so100.h
so100_replay_push_per, so100_replay_per_scan, so100_replay_sample_per, so100_replay_per_update): the
yardstick of tests/test_replay_per_cpu.py and tests/test_gpu_replay_per.py.  It subclasses tests/replay_nstep_ref.py's
restatement, which it leaves untouched: the ring, the `ends` bytes, the window and the return are that class's own; only
the pick is replaced.  Priorities are Python integers (stored as uint32), sums are Python integers, `probs` is a float64
division cast to float32: all exact.  The two inexact places of the feature stay outside: `update` takes the priorities q
as given, and the weights are returned as their float32 base (count * probs) for the caller to raise."""
import math

import numpy as np

from her_ref import draw, mulhi
from replay_nstep_ref import ReplayNstepRef
from replay_ref import NOBS, shift_of, shifted

PRIO_ONE = 65536
PRIO_MAX = (1 << 32) - 1


def per_storage_bytes(n, T):
    """so100_replay_per_storage_bytes in Python integers"""
    return 4 * T * n + 8 * (n + 1) + 8


def priority64(td, alpha, eps):
    """(|td| + eps)^alpha * 65536 in float64, unrounded and unclamped (a NaN counts as 0): what the device's float32 q
    is compared against.  td and eps are taken as the float32 values the device reads."""
    x = float(np.float32(td))
    x = 0.0 if math.isnan(x) else abs(x)
    alpha = float(np.float32(alpha))
    if math.isinf(x):                                    # inf^0 = 1, as powf has it: alpha = 0 makes every priority 1.0
        return math.inf if alpha > 0 else float(PRIO_ONE)
    return (x + float(np.float32(eps))) ** alpha * PRIO_ONE


def clamp_priority(v):
    """rint and the clamp into 1 .. 2^32 - 1 of an unrounded priority"""
    if math.isinf(v):
        return PRIO_MAX
    return min(max(int(np.rint(v)), 1), PRIO_MAX)


class ReplayPerRef(ReplayNstepRef):
    """ReplayNstepRef with the priorities.  nstep=False: the buffer has no `ends` array to compare (the bytes are kept all
    the same, and unused)."""

    def __init__(self, n, T, action_dim, layout=None, seed=0, nstep=True):
        super().__init__(n, T, action_dim, layout, seed)
        self.prio = np.zeros((T, n), np.uint32)
        self.max_prio = PRIO_ONE
        if not nstep:
            self.ARRAYS = tuple(k for k in self.ARRAYS if k != "ends")
        self.ARRAYS += ("prio",)

    # ------------------------------------------------------------------ push (rules 8 and 9)
    def push(self, obs, final_obs, action, reward, terminated, truncated, diverged=None, pixels=None, final_pixels=None):
        before = self.meta.copy()
        super().push(obs, final_obs, action, reward, terminated, truncated, diverged, pixels, final_pixels)
        for e in range(self.n):
            c = int(before[0, e])
            if diverged is not None and bool(diverged[e]):
                self.prio[c, e] = 0
            else:
                self.prio[c, e] = max(self.max_prio, 1)
                self.prio[(c + 1) % self.T, e] = 0

    # ------------------------------------------------------------------ scan
    def sums(self):
        """[n + 1] Python ints: the inclusive sums over the envs of each env's T priorities, then the total"""
        out, run = [], 0
        for e in range(self.n):
            run += sum(int(x) for x in self.prio[:, e])
            out.append(run)
        return out + [run]

    # ------------------------------------------------------------------ pick (rules 1-4)
    def pick(self, sums, h):
        """(env, slot, k, q) of the 64-bit draw h, or None for total == 0"""
        total = sums[self.n]
        if total == 0:
            return None
        r = mulhi(h, total)
        e = 0
        while e < self.n - 1 and sums[e] <= r:
            e += 1
        rr = r - (sums[e - 1] if e else 0)
        slots = self.valid_slots(e)
        run, k = 0, len(slots) - 1                       # (no k found: the last valid slot)
        for j, s in enumerate(slots):
            run += int(self.prio[s, e])
            if run > rr:
                k = j
                break
        s = slots[k]
        return e, s, k, int(self.prio[s, e])

    def sample(self, batch, call, pad=0):
        """the batch of so100_replay_sample_per as numpy arrays (sample_nstep, inherited, builds the window on it): the
        plain sample's keys, and "probs" (float32), "q" and "total" (Python ints; total is one int), "wbase" (float32:
        count * probs, the base of the weight)"""
        T, P = self.T, self.P
        f32 = np.float32
        out = {"obs": np.zeros((batch, NOBS), f32), "next_obs": np.zeros((batch, NOBS), f32),
               "actions": np.zeros((batch, self.A), f32), "rewards": np.zeros(batch, f32), "dones": np.zeros(batch, f32),
               "env": np.zeros(batch, np.int32), "slot": np.full(batch, -1, np.int32),
               "shift": np.zeros((batch, 4), np.int32), "probs": np.zeros(batch, f32), "wbase": np.zeros(batch, f32),
               "q": [0] * batch}
        if P:
            out["pixels"] = np.zeros((batch, P), np.uint8)
            out["next_pixels"] = np.zeros((batch, P), np.uint8)
        sums = self.sums()
        total = out["total"] = sums[self.n]
        count = int(self.meta[1].astype(np.int64).sum())
        if total == 0:
            return out
        for i in range(batch):
            e, s, _, q = self.pick(sums, draw(self.seed, call, i, 0))
            out["env"][i], out["slot"][i], out["q"][i] = e, s, q
            out["probs"][i] = f32(np.float64(q) / np.float64(total))
            out["wbase"][i] = f32(f32(count) * out["probs"][i])
            out["obs"][i], out["next_obs"][i] = self.obs[s, e], self.next_obs[s, e]
            out["actions"][i], out["rewards"][i] = self.action[s, e], self.reward[s, e]
            out["dones"][i] = float(self.terminated[s, e])
            out["shift"][i] = pad
            if not P:
                continue
            if pad == 0:
                out["pixels"][i], out["next_pixels"][i] = self.obs_img[s, e], self.next_img[s, e]
                continue
            dx, dy = shift_of(draw(self.seed, call, i, 2), pad)
            dx2, dy2 = shift_of(draw(self.seed, call, i, 3), pad)
            out["shift"][i] = dx, dy, dx2, dy2
            out["pixels"][i] = shifted(self.obs_img[s, e].reshape(self.layout), dx, dy, pad).reshape(-1)
            out["next_pixels"][i] = shifted(self.next_img[s, e].reshape(self.layout), dx2, dy2, pad).reshape(-1)
        return out

    # ------------------------------------------------------------------ update (rules 2-4; q as given)
    def update(self, env_idx, slot_idx, q):
        """q[j]: the priority of row j, an int in 1 .. 2^32 - 1.  Returns the indices of the applied rows."""
        applied, best = [], {}
        for j, (e, s) in enumerate(zip(env_idx, slot_idx)):
            e, s = int(e), int(s)
            if not (0 <= e < self.n and 0 <= s < self.T) or s not in self.valid_slots(e):
                continue
            assert 1 <= int(q[j]) <= PRIO_MAX
            best[(s, e)] = max(best.get((s, e), 0), int(q[j]))
            applied.append(j)
        for (s, e), v in best.items():
            self.prio[s, e] = v
        if applied:
            self.max_prio = max(self.max_prio, max(int(q[j]) for j in applied))
        return applied

    def invariant(self):
        """prio > 0 exactly on the valid transitions"""
        for e in range(self.n):
            valid = set(self.valid_slots(e))
            for s in range(self.T):
                if (int(self.prio[s, e]) > 0) != (s in valid):
                    return False
        return True
