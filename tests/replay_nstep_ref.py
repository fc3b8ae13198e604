"""A plain numpy / Python-int restatement of the uniform replay buffer's n-step rules (include/so100.h
so100_replay_push_nstep, so100_replay_stage_nstep, so100_replay_sample_nstep): the yardstick of
tests/test_replay_nstep_cpu.py and tests/test_gpu_replay_nstep.py.  It wraps tests/replay_ref.py's ReplayRef, which it
leaves untouched: the ring, the pick and the start-side outputs are that class's own.  Every index is exact, and the
reward is formed from explicit float32 products and sums in the header's order, so nothing here has a tolerance."""
import numpy as np

from replay_ref import ReplayRef, shifted

MAX_NSTEP = 16
N_REACHED, END_FLAG, NEWEST = "n_reached", "end_flag", "newest"
# who set an `ends` byte (the restatement's own bookkeeping, not a device array): tests use it for their coverage
# conditions
WHY_DONE, WHY_STAGE, WHY_DROP = 1, 2, 3


def rows(n, t, width, base=0.0):
    """[n, width] float32 rows that encode (env, push index t) and the column"""
    e = np.arange(n, dtype=np.float32)[:, None]
    return (1000 * e + t + base + np.arange(width, dtype=np.float32)[None, :] / 16).astype(np.float32)


def imgs(n, t, P, salt=0):
    """[n, P] bytes that encode (env, push index t) and the byte index"""
    e = np.arange(n)[:, None]
    return ((np.arange(P)[None, :] * 7 + 31 * e + 101 * t + salt) % 251).astype(np.uint8)


def order_rewards(n, t):
    """reward = 1 + 2^-20 j, j = t + 37 e (exact in float32): with gamma = 0.99 a reordered sum or a contracted
    multiply-add changes the last bit of an n-step return"""
    return (1.0 + (t + 37 * np.arange(n)) * 2.0 ** -20).astype(np.float32)


def step_rows(n, t, A, P, term, trunc, div):
    """the inputs of push t, as so100_replay_step names them"""
    done = (term | trunc).astype(bool)
    r = dict(obs=rows(n, t, 15), final_obs=rows(n, t, 15, base=0.5), action=rows(n, t, A, base=0.25),
             reward=order_rewards(n, t), terminated=term, truncated=trunc, diverged=div)
    if P:
        r["pixels"] = imgs(n, t, P)
        r["final_pixels"] = imgs(n, t, P, salt=13)
        r["final_pixels"][~done] = 255                   # stale rows of the envs that are not done: poison
    else:
        r["pixels"] = r["final_pixels"] = None
    return r


def scripted_events(n, T):
    """The episodes of the sample tests, 2 T + 3 pushes so that the ring wraps twice: per push (terminated, truncated,
    diverged, mask-of-a-stage-after-it or None).  By env mod 5: 0 never finishes (its windows stop at n_step or at the
    newest transition); 1 terminates once and is truncated once within the last T - 1 pushes; 2 is reset in mid-episode
    (a masked stage); 3 has one step dropped; 4 always diverges (it stays empty, and its stage finds count == 0)."""
    steps = 2 * T + 3
    idx = np.arange(n) % 5
    out = []
    for t in range(steps):
        term = (idx == 1) & (t == steps - T // 2 - 1)
        trunc = (idx == 1) & (t == steps - 2)
        div = (idx == 4) | ((idx == 3) & (t == steps - T // 2 + 1))
        trunc = trunc | div                              # the step truncates what it flags as diverged
        mask = ((idx == 2) | (idx == 4)).astype(np.uint8) if t == steps - T // 2 else None
        out.append((term.astype(np.uint8), trunc.astype(np.uint8), div.astype(np.uint8), mask))
    return out


def scripted(n, T, A, layout=None, seed=0, on_call=None):
    """a ReplayNstepRef driven through scripted_events; on_call(kind, t, args), when given, is called after each push
    ("push", the step rows) and stage ("stage", (mask, obs, pixels))"""
    ref = ReplayNstepRef(n, T, A, layout, seed=seed)
    for t, (term, trunc, div, mask) in enumerate(scripted_events(n, T)):
        r = step_rows(n, t, A, ref.P, term, trunc, div)
        ref.push(**r)
        if on_call:
            on_call("push", t, r)
        if mask is not None:
            args = (mask, rows(n, 500 + t, 15), imgs(n, 500 + t, ref.P) if ref.P else None)
            ref.stage(*args)
            if on_call:
                on_call("stage", t, args)
    return ref


def coverage(out, n_step):
    """what a batch of sample_nstep covers: (the window lengths, the stop reasons, who closed the end_flag rows)"""
    return (set(int(m) for m in out["nsteps"]), set(out["reason"]) - {None},
            set(w for w, r in zip(out["why"], out["reason"]) if r == END_FLAG))


def covers_everything(out, n_step):
    lengths, reasons, why = coverage(out, n_step)
    return (lengths == set(range(1, n_step + 1)) and reasons == {N_REACHED, END_FLAG, NEWEST}
            and why == {WHY_DONE, WHY_STAGE, WHY_DROP})


def nstep_storage_bytes(n, T):
    """so100_replay_nstep_storage_bytes in Python integers"""
    return T * n


class ReplayNstepRef(ReplayRef):
    """ReplayRef with the `ends` bytes: ends[s][e] != 0 where slot s of env e holds the last transition that an n-step
    window may include from its episode."""

    def __init__(self, n, T, action_dim, layout=None, seed=0):
        super().__init__(n, T, action_dim, layout, seed)
        self.ends = np.zeros((T, n), np.uint8)
        self.why = np.zeros((T, n), np.uint8)
        self.ARRAYS += ("ends",)

    def push(self, obs, final_obs, action, reward, terminated, truncated, diverged=None, pixels=None, final_pixels=None):
        T = self.T
        for e in range(self.n):
            c, k = (int(x) for x in self.meta[:, e])
            done = bool(terminated[e]) or bool(truncated[e])
            self.ends[c, e] = 1 if done else 0
            self.why[c, e] = WHY_DONE if done else 0
            if diverged is not None and bool(diverged[e]) and k > 0:     # the episode was cut before this step
                p = (c - 1) % T
                if not self.ends[p, e]:
                    self.why[p, e] = WHY_DROP
                self.ends[p, e] = 1
        super().push(obs, final_obs, action, reward, terminated, truncated, diverged, pixels, final_pixels)

    def stage(self, mask, obs, pixels=None):
        for e in range(self.n):
            if mask is not None and not mask[e]:
                continue
            c, k = (int(x) for x in self.meta[:, e])
            if k > 0:                                                    # a reset cuts the episode here
                p = (c - 1) % self.T
                if not self.ends[p, e]:
                    self.why[p, e] = WHY_STAGE
                self.ends[p, e] = 1
        super().stage(mask, obs, pixels)

    def window(self, e, s, n_step):
        """(m, reason) of the window that starts at the valid slot s of env e"""
        T = self.T
        c, k = int(self.meta[0, e]), int(self.meta[1, e])
        kidx = (s - (c - k)) % T
        assert 0 <= kidx < k
        for j in range(1, n_step + 1):
            if self.ends[(s + j - 1) % T, e]:
                return j, END_FLAG
            if kidx + j == k:
                return j, NEWEST
            if j == n_step:
                return j, N_REACHED
        raise AssertionError("n_step < 1")

    def nstep_return(self, e, s, m, gamma):
        """(R, discount) over the m slots from s, in float32: each product rounded, then each sum"""
        f32 = np.float32
        gamma = f32(gamma)
        R, g = f32(self.reward[s, e]), gamma
        for j in range(1, m):
            R = f32(R + f32(g * f32(self.reward[(s + j) % self.T, e])))
            g = f32(g * gamma)
        return R, g

    def sample_nstep(self, batch, call, n_step, gamma, pad=0):
        """the batch as numpy arrays, by the header's rules; beside the device outputs, "reason" (the stop reason of each
        row, None for an empty buffer) and "why" (who set the `ends` byte of an end_flag row)"""
        assert 1 <= n_step <= min(MAX_NSTEP, self.T - 1)
        out = self.sample(batch, call, pad)              # the pick and the start-side fields are the plain sample's
        out["discounts"] = np.zeros(batch, np.float32)
        out["nsteps"] = np.zeros(batch, np.int32)
        out["last_slot"] = np.full(batch, -1, np.int32)
        out["reason"], out["why"] = [None] * batch, [0] * batch
        for i in range(batch):
            e, s = int(out["env"][i]), int(out["slot"][i])
            if s < 0:
                continue
            m, reason = self.window(e, s, n_step)
            last = (s + m - 1) % self.T
            out["rewards"][i], out["discounts"][i] = self.nstep_return(e, s, m, gamma)
            out["nsteps"][i], out["last_slot"][i] = m, last
            out["reason"][i] = reason
            out["why"][i] = int(self.why[last, e]) if reason == END_FLAG else 0
            out["next_obs"][i] = self.next_obs[last, e]
            out["dones"][i] = float(self.terminated[last, e])
            if self.P:
                if pad == 0:
                    out["next_pixels"][i] = self.next_img[last, e]
                else:
                    dx2, dy2 = (int(x) for x in out["shift"][i][2:])
                    out["next_pixels"][i] = shifted(self.next_img[last, e].reshape(self.layout), dx2, dy2,
                                                    pad).reshape(-1)
        return out
