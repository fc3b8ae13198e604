"""The hindsight replay buffer on the GPU (csrc/so100_her.hip; include/so100.h so100_her_push / so100_her_discard /
so100_her_scan / so100_her_sample) against the integer restatement (tests/her_ref.py).  The direct tests
drive the C-ABI with synthetic rows that encode (env, push index), so every stored and gathered row is checked bit for
bit; nothing here has a tolerance.  The closed loop runs SO100VecEnv(replay=...) and feeds the restatement the tensors
recorded around each step."""
import ctypes

import numpy as np
import pytest

import her_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_ENV = {}
T8 = 8


def _handle():
    """a small GoalEnv: the handle (device, goal threshold) the direct launches are made on, and compute_reward"""
    if "bare" not in _ENV:
        from gym_so100 import SO100VecEnv
        _ENV["bare"] = SO100VecEnv(4, task="so100_goal", device="cuda:0")
    return _ENV["bare"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _same(a, b):
    """bit for bit (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Buf:
    """the device arrays of one buffer and its so100_her record"""

    def __init__(self, n, T, A, strategy=her_ref.FUTURE, n_sampled_goal=4, seed=0, ref=None):
        from gym_so100 import _native
        self.n, self.T, self.A = n, T, A
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")  # noqa: E731
        i32 = torch.int32
        self.t = {"obs": z(T, n, 15), "next_obs": z(T, n, 15), "goal": z(T, n, 3), "action": z(T, n, A),
                  "reward": z(T, n), "terminated": z(T, n, dtype=torch.uint8), "offset": z(T, n, dtype=i32),
                  "length": z(T, n, dtype=i32), "meta": z(3, n, dtype=i32), "stage_obs": z(n, 15),
                  "stage_goal": z(n, 3), "prefix": z(n + 1, dtype=i32)}
        if ref is not None:                              # start from a restatement's state
            for k in ref.ARRAYS:
                self.t[k].copy_(_dev(getattr(ref, k)))
        self.her = _native.SO100Her(n=n, T=T, action_dim=A, strategy=strategy, n_sampled_goal=n_sampled_goal, seed=seed,
                                    **{k: _native.ptr(v) for k, v in self.t.items()})
        self.env = _handle()

    def _ok(self, rc):
        assert rc == 0, self.env.lib.so100_last_error()

    def push(self, **rows):
        from gym_so100 import _native
        keep = {k: (_dev(v) if v is not None else None) for k, v in rows.items()}
        st = _native.SO100HerStep(**{k: _native.ptr(v) for k, v in keep.items()})
        self._ok(self.env.lib.so100_her_push(self.env._handle, ctypes.byref(self.her), ctypes.byref(st),
                                             self.env._stream()))
        torch.cuda.synchronize()

    def discard(self, mask=None, obs=None, goal=None):
        from gym_so100 import _native
        keep = [None if v is None else _dev(v) for v in (mask, obs, goal)]
        self._ok(self.env.lib.so100_her_discard(self.env._handle, ctypes.byref(self.her), *[_native.ptr(v) for v in keep],
                                                self.env._stream()))
        torch.cuda.synchronize()

    def scan(self):
        self._ok(self.env.lib.so100_her_scan(self.env._handle, ctypes.byref(self.her), self.env._stream()))
        torch.cuda.synchronize()
        return self.t["prefix"].cpu().numpy()

    def sample(self, B, call, fill=None):
        """one so100_her_sample (after a scan) -> the outputs as numpy"""
        from gym_so100 import _native
        f = lambda *s, dtype=torch.float32: torch.full(s, 7 if fill is None else fill, dtype=dtype,  # noqa: E731
                                                       device="cuda")
        i32 = torch.int32
        out = {"observation": f(B, 15), "achieved_goal": f(B, 3), "desired_goal": f(B, 3), "next_observation": f(B, 15),
               "next_achieved_goal": f(B, 3), "next_desired_goal": f(B, 3), "actions": f(B, self.A), "rewards": f(B),
               "dones": f(B), "env": f(B, dtype=i32), "slot": f(B, dtype=i32), "goal_slot": f(B, dtype=i32)}
        rec = _native.SO100HerOut(**{k: _native.ptr(v) for k, v in out.items()})
        self._ok(self.env.lib.so100_her_sample(self.env._handle, ctypes.byref(self.her), B, ctypes.c_uint64(call),
                                               ctypes.byref(rec), self.env._stream()))
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def assert_equals(self, ref, where):
        h = self.host()
        for k in ref.ARRAYS:
            assert _same(h[k], getattr(ref, k)), (where, k)


def _rows(n, t, width, base=0.0):
    """[n, width] float32 rows that encode (env, push index t) and the column"""
    e = np.arange(n, dtype=np.float32)[:, None]
    return (1000 * e + t + base + np.arange(width, dtype=np.float32)[None, :] / 16).astype(np.float32)


# episode lengths each env cycles through, rotated by the env's index: lengths 1 and T, a wrap, an eviction at a full
# ring, and neighbours whose cursors come apart after the first episode
_LENGTHS = [3, 1, T8, 5, 2, T8, 1, 1, 6, 4]


def _script(n, steps):
    """per push: (terminated, truncated, diverged, discard-or-None) [n] each.  Env e's episodes take _LENGTHS rotated
    by e; env 1 (mod 5)'s third episode diverges at its end, env 2 (mod 5)'s open episode is discarded at push 9."""
    left = np.array([_LENGTHS[e % len(_LENGTHS)] for e in range(n)])
    idx = np.arange(n) % len(_LENGTHS)
    ep = np.zeros(n, int)
    out = []
    for t in range(steps):
        left -= 1
        done = left == 0
        term = done & ((np.arange(n) + t) % 2 == 0)
        trunc = done & ~term
        div = done & (np.arange(n) % 5 == 1) & (ep == 2)
        trunc = trunc | div
        disc = (np.arange(n) % 5 == 2).astype(np.uint8) if t == 9 else None
        out.append((term.astype(np.uint8), trunc.astype(np.uint8), div.astype(np.uint8), disc))
        for e in np.flatnonzero(done):
            idx[e] = (idx[e] + 1) % len(_LENGTHS)
            left[e] = _LENGTHS[idx[e]]
            ep[e] += 1
    return out


def _filled(n, T, A, steps, **kw):
    """a restatement after `steps` scripted pushes whose achieved goals sit 0.004 apart along x within an episode (so
    relabelled rewards are 0 for goals up to two steps away and -1 beyond), the other columns encoding (env, push)"""
    ref = her_ref.HerRef(n, T, A, **kw)
    for t, (term, trunc, div, disc) in enumerate(_script(n, steps)):
        obs, fin = _rows(n, t, 15), _rows(n, t, 15, base=0.5)
        for rows, shift in ((obs, 0.0), (fin, 0.0)):
            rows[:, 0] = np.arange(n) + np.float32(0.004) * (t % 7) + shift
            rows[:, 1:3] = 0.25
        ref.push_staged(obs, fin, _rows(n, t, 3, base=0.25), _rows(n, t, A, base=0.125),
                        -(100 * np.arange(n, dtype=np.float32) + t), term, trunc, div, disc)
    return ref


# ---------------------------------------------------------------------- push
@pytest.mark.parametrize("n", [1, 5, 65])
def test_push_matches_the_restatement(n):
    T, A, steps = T8, 6, 44
    ref, buf = her_ref.HerRef(n, T, A), Buf(n, T, A)
    cursors = set()
    seen = dict(len1=False, lenT=False, evict=False, wrap=False, diverged=False, discard=False)
    for t, (term, trunc, div, disc) in enumerate(_script(n, steps)):
        rows = dict(prev_obs=_rows(n, t, 15, base=0.75), prev_goal=_rows(n, t, 3, base=0.375), obs=_rows(n, t, 15),
                    final_obs=_rows(n, t, 15, base=0.5), goal=_rows(n, t, 3, base=0.25),
                    action=_rows(n, t, A, base=0.125), reward=-(100 * np.arange(n, dtype=np.float32) + t),
                    terminated=term, truncated=trunc, diverged=div, discard=disc)
        before = ref.meta.copy()
        ref.push(**rows)
        buf.push(**rows)
        buf.assert_equals(ref, ("push", t))
        closed = ref.meta[1] - before[1]
        seen["len1"] |= bool((closed == 1).any())
        seen["lenT"] |= bool((ref.meta[1] == T).any())
        seen["evict"] |= bool(((before[1] + before[2] == T) & (before[1] > 0)).any())
        seen["wrap"] |= bool(((ref.meta[0] + ref.meta[1] + ref.meta[2]) > T).any())
        seen["diverged"] |= bool(div.any())
        seen["discard"] |= disc is not None and bool((disc != 0).any() and (before[2][disc != 0] > 0).any())
        cursors.add(tuple(ref.cursor(e) for e in range(min(n, 2))))
        if t == 20:                                      # a reset of every third env: discard, new rows staged
            mask = (np.arange(n) % 3 == 0).astype(np.uint8)
            o, g = _rows(n, t, 15, base=0.875), _rows(n, t, 3, base=0.875)
            ref.discard(mask, o, g)
            buf.discard(mask, o, g)
            buf.assert_equals(ref, ("discard", t))
        if t == 30:                                      # discard(None): every open episode, nothing staged
            ref.discard()
            buf.discard()
            buf.assert_equals(ref, ("discard all", t))
    want = {"len1", "lenT", "evict", "wrap"} | ({"diverged", "discard"} if n > 2 else set())
    assert all(seen[k] for k in want), seen
    if n > 1:
        assert any(a != b for a, b in cursors)           # two envs whose cursors have come apart
    assert _same(buf.scan()[:n], np.cumsum(ref.meta[1]).astype(np.int32))


def test_push_in_place_staging():
    """prev_obs / prev_goal may be the staged rows themselves (what SO100VecEnv passes)"""
    n, T, A = 5, T8, 6
    ref, buf = her_ref.HerRef(n, T, A), Buf(n, T, A)
    from gym_so100 import _native
    for t, (term, trunc, div, _) in enumerate(_script(n, 12)):
        rows = dict(obs=_rows(n, t, 15), final_obs=_rows(n, t, 15, base=0.5), goal=_rows(n, t, 3, base=0.25),
                    action=_rows(n, t, A, base=0.125), reward=-np.arange(n, dtype=np.float32) - t, terminated=term,
                    truncated=trunc, diverged=div)
        ref.push_staged(*[rows[k] for k in ("obs", "final_obs", "goal", "action", "reward", "terminated", "truncated",
                                            "diverged")])
        keep = {k: _dev(v) for k, v in rows.items()}
        st = _native.SO100HerStep(prev_obs=_native.ptr(buf.t["stage_obs"]), prev_goal=_native.ptr(buf.t["stage_goal"]),
                                  **{k: _native.ptr(v) for k, v in keep.items()})
        buf._ok(buf.env.lib.so100_her_push(buf.env._handle, ctypes.byref(buf.her), ctypes.byref(st), buf.env._stream()))
        torch.cuda.synchronize()
        buf.assert_equals(ref, ("staged push", t))


# ---------------------------------------------------------------------- scan
def _scan_sizes():
    from gym_so100 import _native
    w, tile = _native.her_limits()
    return w, [1, w - 1, w, w + 1, 4 * w + 1] + [63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]


def test_scan_is_cumsum():
    w, sizes = _scan_sizes()
    rng = np.random.default_rng(11)
    for n in sizes:
        T = 300
        buf = Buf(n, 2, 1)                               # (the scan reads the counts alone: a small ring will do)
        buf.her.T = T
        count = rng.integers(0, T + 1, n).astype(np.int32)
        if n > 70:
            count[[3, 64, n - 1]] = T                    # wave and tile edges at the cap
        buf.t["meta"][1].copy_(_dev(count))
        buf.t["prefix"].fill_(-5)
        pre = buf.scan()
        want = np.cumsum(count.astype(np.int64))
        assert want[-1] < 2 ** 31
        assert _same(pre[:n], want.astype(np.int32)), n
        assert pre[n] == want[-1], n
    # counts outside [0, T] (corrupted metadata) are taken as 0 / T
    buf = Buf(5, 4, 1)
    buf.t["meta"][1].copy_(_dev(np.array([2, -7, 9, 4, 0], np.int32)))
    assert buf.scan().tolist() == [2, 2, 6, 10, 10, 10]


# ---------------------------------------------------------------------- sample
_REF = {}


def _sample_ref():
    """one filled restatement (5 envs, T = 8, 37 pushes) shared by the sample tests; never modified.  Four envs hold
    closed episodes, the last has none (the search over the prefix sums must never land on it)"""
    if "ref" not in _REF:
        _REF["ref"] = _filled(5, T8, 6, 37)
        assert _REF["ref"].meta[1].tolist() == [6, 4, 4, 1, 0] and (_REF["ref"].meta[2] > 0).any()
    return _REF["ref"]


@pytest.mark.parametrize("n_sampled_goal", [0, 1, 4])
@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
@pytest.mark.parametrize("B", [1, 5, 256, 1000])
def test_sample_matches_the_restatement(B, strategy, n_sampled_goal):
    ref = _sample_ref()
    ref.strategy, ref.n_sampled_goal, ref.seed = her_ref.STRATEGIES[strategy], n_sampled_goal, 99
    before = {k: getattr(ref, k).copy() for k in ref.ARRAYS}
    buf = Buf(ref.n, ref.T, ref.A, strategy=ref.strategy, n_sampled_goal=n_sampled_goal, seed=99, ref=ref)
    pre = buf.scan()
    assert _same(pre.astype(np.int64), ref.prefix())
    got = buf.sample(B, call=2)
    want = ref.sample(B, call=2)
    for k in ("env", "slot", "goal_slot"):
        assert _same(got[k], want[k]), k
    e, s, g = got["env"], got["slot"], got["goal_slot"]
    rel = g >= 0
    nrel = int((1.0 - 1.0 / (n_sampled_goal + 1)) * B)
    assert rel[:nrel].all() and not rel[nrel:].any()
    # every gathered row is its storage row
    assert _same(got["observation"], ref.obs[s, e]) and _same(got["next_observation"], ref.next_obs[s, e])
    assert _same(got["achieved_goal"], ref.obs[s, e, 0:3]) and _same(got["next_achieved_goal"], ref.next_obs[s, e, 0:3])
    assert _same(got["actions"], ref.action[s, e])
    assert _same(got["dones"], ref.terminated[s, e].astype(np.float32))
    assert _same(got["next_desired_goal"], got["desired_goal"])
    # rows returned as stored keep their goal and reward
    assert _same(got["desired_goal"][~rel], ref.goal[s[~rel], e[~rel]])
    assert _same(got["rewards"][~rel], ref.reward[s[~rel], e[~rel]])
    # relabelled rows: the next achieved goal at goal_slot, and the env's own reward of it, bit for bit
    assert _same(got["desired_goal"][rel], ref.next_obs[g[rel], e[rel], 0:3])
    if rel.any():
        env = _handle()
        r = env.compute_reward(_dev(got["next_achieved_goal"][rel]), _dev(got["desired_goal"][rel])).cpu().numpy()
        assert _same(got["rewards"][rel], r)
        assert set(np.unique(r)) <= {0.0, -1.0}
        if nrel >= 100 and strategy != "final":
            assert (r == 0).any() and (r == -1).any()    # both sides of the threshold are exercised
    for k in ("observation", "next_observation", "desired_goal", "actions", "dones"):
        assert _same(got[k], want[k]), k
    # two calls differ; two buffers with the same seed agree bit for bit
    other = buf.sample(B, call=3)
    if B >= 5:
        assert not _same(other["slot"], got["slot"]) or not _same(other["env"], got["env"])
    twin = Buf(ref.n, ref.T, ref.A, strategy=ref.strategy, n_sampled_goal=n_sampled_goal, seed=99, ref=ref)
    twin.scan()
    again = twin.sample(B, call=2)
    assert all(_same(again[k], got[k]) for k in got)
    assert all(_same(before[k], getattr(ref, k)) for k in before)


def test_sample_uses_every_valid_transition():
    """4,000 draws over the shared buffer: every valid (env, slot) comes up, nothing else does"""
    ref = _sample_ref()
    buf = Buf(ref.n, ref.T, ref.A, seed=3, ref=ref)
    buf.scan()
    got = buf.sample(4000, call=0)
    valid = {(e, s) for e in range(ref.n) for s in ref.valid_slots(e)}
    assert set(zip(got["env"].tolist(), got["slot"].tolist())) == valid


def test_empty_buffer():
    for open_only in (False, True):
        buf = Buf(3, T8, 6)
        if open_only:                                    # transitions, but no finished episode
            z = np.zeros(3, np.uint8)
            buf.push(prev_obs=_rows(3, 0, 15), prev_goal=_rows(3, 0, 3), obs=_rows(3, 1, 15), final_obs=_rows(3, 1, 15),
                     goal=_rows(3, 1, 3), action=_rows(3, 0, 6), reward=np.ones(3, np.float32), terminated=z,
                     truncated=z, diverged=None, discard=None)
        assert buf.scan().tolist() == [0, 0, 0, 0]
        got = buf.sample(37, call=0)
        assert (got["slot"] == -1).all() and (got["goal_slot"] == -1).all() and (got["env"] == 0).all()
        for k in ("observation", "achieved_goal", "desired_goal", "next_observation", "next_achieved_goal",
                  "next_desired_goal", "actions", "rewards", "dones"):
            assert not got[k].any() and not np.signbit(got[k]).any(), k


# ---------------------------------------------------------------------- SO100VecEnv(replay=...)
class _Spy:
    """the library with the names of the entry points looked up on it"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _np(t):
    return t.detach().cpu().numpy().copy()


def test_closed_loop():
    from gym_so100 import SO100VecEnv
    n, T = 8, 16
    env = SO100VecEnv(n, task="so100_goal", max_episode_steps=6, seed=3, replay=dict(buffer_size=n * T, seed=17))
    rp = env.replay
    assert rp is not None and rp.capacity == n * T and rp.T == T and rp.her_ratio == 0.8
    with pytest.raises(ValueError):
        rp.sample(4, check=True)                         # nothing finished yet
    assert rp.size() == 0 and (rp.sample(4)["slot"] == -1).all()
    rp.calls = 0
    ref = her_ref.HerRef(n, T, 6, her_ref.FUTURE, 4, seed=17)
    env.reset()
    ref.discard(None, _np(env.obs), _np(env.desired_goal))
    rng = np.random.default_rng(0)
    step_of = np.full((T, n), -1)
    discarded, finished, terminated_seen = set(), 0, 0
    for t in range(52):
        if t in (4, 45):                                 # envs 2 and 5 reach their goal: it is where the cube is
            for e in (2, 5):
                env.desired_goal[e] = env.obs[e, 0:3]
                rp.store["stage_goal"][e] = env.obs[e, 0:3]      # (the goal in force is the staged one)
        if t == 40:                                      # a user reset in mid-episode
            mask = np.arange(n) % 3 == 1
            assert (ref.meta[2][mask] > 0).all()
            for e in np.flatnonzero(mask):
                k = int(ref.meta[2, e])
                discarded |= {(e, t - 1 - j) for j in range(k)}
            env.reset(mask=torch.from_numpy(mask))
            ref.discard(mask, _np(env.obs), _np(env.desired_goal))
            assert _same(_np(rp.store["meta"]), ref.meta)
        prev_obs, prev_goal = _np(env.obs), _np(env.desired_goal)
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        cur = [ref.cursor(e) for e in range(n)]
        env.step(torch.from_numpy(a).cuda())
        term, trunc = _np(env.terminated), _np(env.truncated)
        ref.push(prev_obs, prev_goal, _np(env.obs), _np(env.final_obs), _np(env.desired_goal), a, _np(env.reward),
                 term, trunc, _np(env.diverged))
        for e in range(n):
            step_of[cur[e], e] = t
        host = {k: _np(v) for k, v in rp.store.items()}
        for k in ref.ARRAYS:
            assert _same(host[k], getattr(ref, k)), (t, k)
        done = term | trunc
        finished += int(done.sum())
        terminated_seen += int(term.sum())
        for e in np.flatnonzero(done):                   # the true next observation, not the new episode's first
            assert _same(host["next_obs"][cur[e], e], _np(env.final_obs)[e])
            assert not _same(host["next_obs"][cur[e], e], _np(env.obs)[e])
    assert terminated_seen >= 2 and finished > 5 * n
    assert rp.size() == int(ref.meta[1].sum()) and int(rp.valid_count.item()) == rp.size()
    for e in range(n):                                   # nothing of a discarded episode can be drawn
        assert not {(e, int(step_of[s, e])) for s in ref.valid_slots(e)} & discarded
    for call in range(3):
        assert rp.calls == call
        got = {k: _np(v) for k, v in rp.sample(256).items()}
        want = ref.sample(256, call)
        for k in ("env", "slot", "goal_slot", "observation", "next_observation", "desired_goal", "actions", "dones",
                  "achieved_goal", "next_achieved_goal", "next_desired_goal"):
            assert _same(got[k], want[k]), (call, k)
        rel = got["goal_slot"] >= 0
        assert rel.sum() == 204 and _same(got["rewards"][~rel], want["rewards"][~rel])
        r = env.compute_reward(_dev(got["next_achieved_goal"][rel]), _dev(got["desired_goal"][rel]))
        assert _same(got["rewards"][rel], _np(r))
        assert all((e, s) not in discarded for e, s in zip(got["env"], step_of[got["slot"], got["env"]]))
    assert got["dones"].any()                            # the terminated transitions are in the buffer
    # discard(): the open episodes go, the closed ones stay
    rp.discard()
    ref.discard()
    assert _same(_np(rp.store["meta"]), ref.meta) and rp.size() == int(ref.meta[1].sum())
    env.close()


def test_sample_normalize_and_shim():
    from gym_so100 import SO100VecEnv
    from gym_so100.sb3 import SO100HerReplayBuffer, SO100SB3VecEnv
    n = 8
    env = SO100VecEnv(n, task="so100_goal", max_episode_steps=5, seed=1, normalize=True,
                      replay=dict(buffer_size=n * 10, n_sampled_goal=1, goal_selection_strategy="episode"))
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(12):
        env.step(torch.from_numpy(rng.uniform(-1, 1, (n, 6)).astype(np.float32)).cuda())
    env.training = False
    raw = env.replay.sample(64)
    env.replay.calls -= 1                                # the same draws again
    norm = env.replay.sample(64, normalize=True)
    keys = ("observation", "achieved_goal", "desired_goal")
    want = env.normalize_obs({k: raw[k] for k in keys})
    want_next = env.normalize_obs({k: raw["next_" + k] for k in keys})
    for k in keys:
        assert _same(_np(norm[k]), _np(want[k])) and _same(_np(norm["next_" + k]), _np(want_next[k]))
        assert not _same(_np(norm[k]), _np(raw[k]))
    for k in ("actions", "rewards", "dones", "env", "slot", "goal_slot"):
        assert _same(_np(norm[k]), _np(raw[k]))          # rewards are never normalised
    env.close()
    plain = SO100VecEnv(n, task="so100_goal", max_episode_steps=5, replay=dict(buffer_size=n * 10))
    with pytest.raises(ValueError):
        plain.replay.sample(4, normalize=True)
    plain.close()
    # the SB3 shim
    venv = SO100SB3VecEnv(n, task="so100_goal", max_episode_steps=4, replay=dict(buffer_size=n * 8))
    venv.reset()
    for _ in range(9):
        venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        venv.step_wait()
    rb = SO100HerReplayBuffer(env=venv)
    assert rb.add(1, 2, 3) is None and rb.size() == venv.venv.replay.size() > 0
    b = rb.sample(32)
    assert b._fields == ("observations", "actions", "next_observations", "dones", "rewards")
    assert tuple(b.rewards.shape) == (32, 1) and tuple(b.dones.shape) == (32, 1) and tuple(b.actions.shape) == (32, 6)
    for obs in (b.observations, b.next_observations):
        assert sorted(obs) == ["achieved_goal", "desired_goal", "observation"]
        assert tuple(obs["observation"].shape) == (32, 15) and tuple(obs["desired_goal"].shape) == (32, 3)
        assert obs["observation"].is_cuda
    with pytest.raises(ValueError):
        SO100HerReplayBuffer(env=_handle())
    venv.close()


def test_off_means_untouched_and_the_command_is_stored():
    from gym_so100 import SO100VecEnv
    env = _handle()
    assert env.replay is None
    spy = _Spy(env.lib)
    env.lib = spy
    try:
        env.reset()
        env.step(torch.zeros(4, 6, device="cuda"))
        env.step_async_raw()
    finally:
        env.lib = spy._lib
    assert "so100_step" in spy.names and not [x for x in spy.names if x.startswith("so100_her")]
    # with the argument: the step pushes (step_async_raw does not), and with ee_delta the stored command is the 5-wide one
    n = 4
    on = SO100VecEnv(n, task="so100_goal", max_episode_steps=4, action_mode="ee_delta", replay=dict(buffer_size=n * 4))
    assert on.replay.action_dim == 5
    spy = _Spy(on.lib)
    on.lib = on.replay.lib = spy
    on.reset()
    a = np.random.default_rng(2).uniform(-1, 1, (n, 5)).astype(np.float32)
    on.step(torch.from_numpy(a).cuda())
    assert spy.names.count("so100_her_push") == 1
    on.step_async_raw()
    assert spy.names.count("so100_her_push") == 1
    on.lib = on.replay.lib = spy._lib
    assert _same(_np(on.replay.store["action"])[0], a)
    assert (_np(on.replay.open_len) + _np(on.replay.count)).tolist() == [1] * n     # (a goal may be met at once)
    on.close()
