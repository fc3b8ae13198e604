"""A plain numpy / Python-int restatement of the hindsight replay buffer's rules (include/so100.h so100_her_push,
so100_her_discard, so100_her_scan, so100_her_sample): the yardstick of tests/test_her_cpu.py and tests/test_gpu_her.py.
Every index is an exact integer; nothing here has a tolerance.  The draws reuse the package's ``_splitmix64`` and the key
formula stated in the header."""
import numpy as np

from gym_so100.vec_env import _splitmix64

NOBS = 15
FUTURE, FINAL, EPISODE = 0, 1, 2
STRATEGIES = {"future": FUTURE, "final": FINAL, "episode": EPISODE}
M64 = (1 << 64) - 1


def draw(seed, call, i, field):
    """the 64-bit draw of (seed, sample call, batch element, field) as a Python int"""
    with np.errstate(over="ignore"):
        k = _splitmix64(np.uint64(seed & M64) ^ np.uint64((int(i) * 0x100000001B3) & M64) ^
                        np.uint64((int(field) * 0xD1B54A32D192ED03) & M64))
        return int(_splitmix64(k + np.uint64(call & M64)))


def mulhi(h, m):
    """floor(h m / 2^64): uniform in [0, m) for a uniform 64-bit h"""
    return (int(h) * int(m)) >> 64


def n_relabelled(n_sampled_goal, batch):
    """int(her_ratio * batch), her_ratio = 1 - 1 / (n_sampled_goal + 1), in float64 (SB3's expression)"""
    return int((1.0 - 1.0 / (n_sampled_goal + 1.0)) * float(batch))


def pick(prefix, total, h):
    """(env, index within the env's valid interval) of the draw h: r = floor(h total / 2^64), the first env whose
    inclusive prefix sum exceeds r"""
    r = mulhi(h, total)
    e = 0
    while prefix[e] <= r:
        e += 1
    return e, r - (prefix[e - 1] if e else 0)


class HerRef:
    """The ring of T slots for n envs, slot-major, and its metadata, as the header describes them."""

    def __init__(self, n, T, action_dim, strategy=FUTURE, n_sampled_goal=4, seed=0):
        self.n, self.T, self.A = n, T, action_dim
        self.strategy, self.n_sampled_goal, self.seed = strategy, n_sampled_goal, seed
        f32 = np.float32
        self.obs = np.zeros((T, n, NOBS), f32)
        self.next_obs = np.zeros((T, n, NOBS), f32)
        self.goal = np.zeros((T, n, 3), f32)
        self.action = np.zeros((T, n, action_dim), f32)
        self.reward = np.zeros((T, n), f32)
        self.terminated = np.zeros((T, n), np.uint8)
        self.offset = np.zeros((T, n), np.int32)
        self.length = np.zeros((T, n), np.int32)
        self.meta = np.zeros((3, n), np.int32)           # valid_lo, count, open_len
        self.stage_obs = np.zeros((n, NOBS), f32)
        self.stage_goal = np.zeros((n, 3), f32)

    ARRAYS = ("obs", "next_obs", "goal", "action", "reward", "terminated", "offset", "length", "meta", "stage_obs",
              "stage_goal")

    def cursor(self, e):
        lo, count, open_len = (int(x) for x in self.meta[:, e])
        return (lo + count + open_len) % self.T

    def push(self, prev_obs, prev_goal, obs, final_obs, goal, action, reward, terminated, truncated, diverged=None,
             discard=None):
        T = self.T
        for e in range(self.n):
            lo, count, open_len = (int(x) for x in self.meta[:, e])
            if count + open_len == T:                    # 1. a full ring
                if count > 0:
                    L = int(self.length[lo, e])
                    assert 1 <= L <= count
                    lo, count = (lo + L) % T, count - L
                else:
                    open_len = 0
            cur = (lo + count + open_len) % T            # 2. the transition at the cursor
            fin = bool(terminated[e]) or bool(truncated[e])
            self.obs[cur, e] = prev_obs[e]
            self.next_obs[cur, e] = final_obs[e] if fin else obs[e]
            self.goal[cur, e] = prev_goal[e]
            self.action[cur, e] = action[e]
            self.reward[cur, e] = reward[e]
            self.terminated[cur, e] = 1 if terminated[e] else 0
            self.offset[cur, e] = open_len
            open_len += 1
            erase = (diverged is not None and bool(diverged[e])) or (discard is not None and bool(discard[e]))
            if erase:                                    # 3. erase, close or go on
                open_len = 0
            elif fin:
                self.length[(cur - (open_len - 1)) % T, e] = open_len
                count += open_len
                open_len = 0
            self.meta[:, e] = lo, count, open_len
            self.stage_obs[e] = obs[e]                   # 4. the next transition's "before" values
            self.stage_goal[e] = goal[e]
        assert (self.meta[1] + self.meta[2] <= T).all()

    def push_staged(self, obs, final_obs, goal, action, reward, terminated, truncated, diverged=None, discard=None):
        """a push whose "before" rows are the staged ones (what SO100VecEnv does)"""
        self.push(self.stage_obs.copy(), self.stage_goal.copy(), obs, final_obs, goal, action, reward, terminated,
                  truncated, diverged, discard)

    def discard(self, mask=None, obs=None, goal=None):
        for e in range(self.n):
            if mask is not None and not mask[e]:
                continue
            self.meta[2, e] = 0
            if obs is not None:
                self.stage_obs[e] = obs[e]
            if goal is not None:
                self.stage_goal[e] = goal[e]

    def prefix(self):
        """[n + 1]: the inclusive prefix sums of count, then the total"""
        c = np.cumsum(self.meta[1].astype(np.int64))
        return np.concatenate([c, c[-1:] if self.n else np.zeros(1, np.int64)])

    def valid_slots(self, e):
        """the slots of env e a sample may draw, in ring order"""
        lo, count = int(self.meta[0, e]), int(self.meta[1, e])
        return [(lo + k) % self.T for k in range(count)]

    def sample_indices(self, batch, call):
        """(env, slot, goal_slot) [batch] int32 each; goal_slot -1 for the rows returned as stored; slot -1 (env 0) for
        every row of an empty buffer"""
        T = self.T
        pre = self.prefix()
        total = int(pre[self.n])
        env = np.zeros(batch, np.int32)
        slot = np.full(batch, -1, np.int32)
        gslot = np.full(batch, -1, np.int32)
        if total == 0:
            return env, slot, gslot
        nrel = n_relabelled(self.n_sampled_goal, batch)
        for i in range(batch):
            e, k = pick(pre, total, draw(self.seed, call, i, 0))
            s = (int(self.meta[0, e]) + k) % T
            env[i], slot[i] = e, s
            if i >= nrel:
                continue
            off = int(self.offset[s, e])
            first = (s - off) % T
            ln = int(self.length[first, e])
            assert off < ln <= T
            if self.strategy == FINAL:
                j = ln - 1
            elif self.strategy == FUTURE:
                j = off + mulhi(draw(self.seed, call, i, 1), ln - off)
            else:
                j = mulhi(draw(self.seed, call, i, 1), ln)
            gslot[i] = (first + j) % T
        return env, slot, gslot

    def sample(self, batch, call):
        """the batch as numpy arrays; ``rewards`` of the relabelled rows (goal_slot >= 0) is NaN: the reward function is
        the device's (so100_goal_reward), the tests evaluate it there"""
        env, slot, gslot = self.sample_indices(batch, call)
        f32 = np.float32
        out = {"env": env, "slot": slot, "goal_slot": gslot,
               "observation": np.zeros((batch, NOBS), f32), "next_observation": np.zeros((batch, NOBS), f32),
               "desired_goal": np.zeros((batch, 3), f32), "actions": np.zeros((batch, self.A), f32),
               "rewards": np.zeros(batch, f32), "dones": np.zeros(batch, f32)}
        for i in range(batch):
            if slot[i] < 0:
                continue
            s, e = slot[i], env[i]
            out["observation"][i] = self.obs[s, e]
            out["next_observation"][i] = self.next_obs[s, e]
            out["actions"][i] = self.action[s, e]
            out["dones"][i] = float(self.terminated[s, e])
            if gslot[i] >= 0:
                out["desired_goal"][i] = self.next_obs[gslot[i], e, 0:3]
                out["rewards"][i] = np.nan
            else:
                out["desired_goal"][i] = self.goal[s, e]
                out["rewards"][i] = self.reward[s, e]
        out["achieved_goal"] = out["observation"][:, 0:3].copy()
        out["next_achieved_goal"] = out["next_observation"][:, 0:3].copy()
        out["next_desired_goal"] = out["desired_goal"].copy()
        return out


class EpisodeList:
    """One env's buffer as SB3 thinks of it: a list of closed episodes (each a list of transition tags) and the open
    one, at most T transitions in all; the oldest closed episode is dropped whole when a write needs room.  The ring
    above must hold exactly these transitions: tests compare its valid interval with ``closed``."""

    def __init__(self, T):
        self.T, self.closed, self.open = T, [], []

    def push(self, tag, done, erase):
        if sum(len(ep) for ep in self.closed) + len(self.open) == self.T:
            if self.closed:
                self.closed.pop(0)
            else:
                self.open = []
        self.open.append(tag)
        if erase:
            self.open = []
        elif done:
            self.closed.append(self.open)
            self.open = []

    def discard(self):
        self.open = []

    def valid(self):
        return [tag for ep in self.closed for tag in ep]
