"""A plain numpy / Python-int restatement of the uniform replay buffer's rules (include/so100.h so100_replay_push,
so100_replay_stage, so100_replay_scan, so100_replay_sample): the yardstick of tests/test_replay_cpu.py and
tests/test_gpu_replay.py.  Every index and every byte is exact; nothing here has a tolerance.  The draws are her_ref's."""
import numpy as np

from her_ref import draw, mulhi

NOBS = 15


def shift_of(h, pad):
    """(dx, dy) in [0, 2 pad] of the 64-bit draw h"""
    S = 2 * pad + 1
    return ((int(h) & 0xFFFFFFFF) * S) >> 32, ((int(h) >> 32) * S) >> 32


def shifted(img, dx, dy, pad):
    """img [planes, H, W, chan] replicate-padded by pad and cropped at (dx, dy): out[p, y, x] = img[p, clamp(y + dy -
    pad), clamp(x + dx - pad)], every plane alike"""
    _, H, W, _ = img.shape
    ys = np.clip(np.arange(H) + dy - pad, 0, H - 1)
    xs = np.clip(np.arange(W) + dx - pad, 0, W - 1)
    return img[:, ys][:, :, xs]


def storage_bytes(n, T, A, P):
    """so100_replay_storage_bytes in Python integers"""
    return T * n * (4 * (NOBS + NOBS + A + 1) + 1 + 2 * P) + 4 * (2 * n + n + 1)


class ReplayRef:
    """The ring of T slots for n envs, slot-major, and its metadata, as the header describes them.  layout: None (no
    images) or (planes, H, W, chan)."""

    def __init__(self, n, T, action_dim, layout=None, seed=0):
        assert T >= 2
        self.n, self.T, self.A, self.layout, self.seed = n, T, action_dim, layout, seed
        self.P = int(np.prod(layout)) if layout else 0
        f32 = np.float32
        self.obs = np.zeros((T, n, NOBS), f32)
        self.next_obs = np.zeros((T, n, NOBS), f32)
        self.action = np.zeros((T, n, action_dim), f32)
        self.reward = np.zeros((T, n), f32)
        self.terminated = np.zeros((T, n), np.uint8)
        self.meta = np.zeros((2, n), np.int32)           # cursor, count
        self.ARRAYS = ("obs", "next_obs", "action", "reward", "terminated", "meta")
        if self.P:
            self.obs_img = np.zeros((T, n, self.P), np.uint8)
            self.next_img = np.zeros((T, n, self.P), np.uint8)
            self.ARRAYS += ("obs_img", "next_img")

    def push(self, obs, final_obs, action, reward, terminated, truncated, diverged=None, pixels=None, final_pixels=None):
        T = self.T
        for e in range(self.n):
            c, k = (int(x) for x in self.meta[:, e])
            done = bool(terminated[e]) or bool(truncated[e])
            self.next_obs[c, e] = final_obs[e] if done else obs[e]                       # 1.
            if self.P:
                self.next_img[c, e] = (final_pixels[e] if done else pixels[e]).reshape(-1)
            self.action[c, e] = action[e]                                                # 2.
            self.reward[c, e] = reward[e]
            self.terminated[c, e] = 1 if terminated[e] else 0
            if diverged is not None and bool(diverged[e]):                               # 3.
                c2, k2 = c, k
            else:
                c2, k2 = (c + 1) % T, min(k + 1, T - 1)
            self.obs[c2, e] = obs[e]                                                     # 4.
            if self.P:
                self.obs_img[c2, e] = pixels[e].reshape(-1)
            self.meta[:, e] = c2, k2                                                     # 5.

    def stage(self, mask, obs, pixels=None):
        for e in range(self.n):
            if mask is not None and not mask[e]:
                continue
            c = int(self.meta[0, e])
            self.obs[c, e] = obs[e]
            if self.P:
                self.obs_img[c, e] = pixels[e].reshape(-1)

    def prefix(self):
        """[n + 1]: the inclusive prefix sums of count, then the total"""
        c = np.cumsum(self.meta[1].astype(np.int64))
        return np.concatenate([c, c[-1:] if self.n else np.zeros(1, np.int64)])

    def valid_slots(self, e):
        """the slots of env e a sample may draw, oldest first"""
        c, k = int(self.meta[0, e]), int(self.meta[1, e])
        return [(c - k + j) % self.T for j in range(k)]

    def sample(self, batch, call, pad=0):
        """the batch as numpy arrays, by the header's rules"""
        T, P = self.T, self.P
        f32 = np.float32
        out = {"obs": np.zeros((batch, NOBS), f32), "next_obs": np.zeros((batch, NOBS), f32),
               "actions": np.zeros((batch, self.A), f32), "rewards": np.zeros(batch, f32), "dones": np.zeros(batch, f32),
               "env": np.zeros(batch, np.int32), "slot": np.full(batch, -1, np.int32),
               "shift": np.zeros((batch, 4), np.int32)}
        if P:
            out["pixels"] = np.zeros((batch, P), np.uint8)
            out["next_pixels"] = np.zeros((batch, P), np.uint8)
        pre = self.prefix()
        total = int(pre[self.n])
        if total == 0:
            return out
        for i in range(batch):
            r = mulhi(draw(self.seed, call, i, 0), total)
            e = 0
            while pre[e] <= r:
                e += 1
            c, k = int(self.meta[0, e]), int(self.meta[1, e])
            s = (c - k + r - (int(pre[e - 1]) if e else 0)) % T
            out["env"][i], out["slot"][i] = e, s
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
