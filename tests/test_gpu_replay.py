"""The uniform replay buffer on the GPU (csrc/so100_replay.hip; include/so100.h so100_replay_push / so100_replay_stage /
so100_replay_scan / so100_replay_sample) against the integer restatement (tests/replay_ref.py).  The
direct tests drive the C-ABI with floats and bytes that encode (env, push index, column), so every stored and gathered
row is checked bit for bit; output buffers start filled with 7, so a byte not written shows.  Nothing here has a
tolerance.  The closed loops run SO100VecEnv(uniform_replay=...) and feed the restatement the tensors recorded around
each step."""
import ctypes

import numpy as np
import pytest

import replay_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_ENV = {}
LAYOUTS = {"none": None, "odd": (1, 3, 5, 3), "planes": (6, 12, 16, 1), "cams": (2, 12, 16, 3), "full": (1, 48, 64, 3)}


def _handle():
    """a small arm-task env: the handle (device) the direct launches are made on"""
    if "bare" not in _ENV:
        from gym_so100 import SO100VecEnv
        _ENV["bare"] = SO100VecEnv(4, task="so100_touch_cube", device="cuda:0")
    return _ENV["bare"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.detach().cpu().numpy().copy()


def _same(a, b):
    """bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Buf:
    """the device arrays of one buffer and its so100_replay record"""

    def __init__(self, n, T, A, layout=None, seed=0, ref=None):
        from gym_so100 import _native
        self.n, self.T, self.A, self.layout = n, T, A, layout
        self.P = P = int(np.prod(layout)) if layout else 0
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")  # noqa: E731
        u8 = torch.uint8
        self.t = {"obs": z(T, n, 15), "next_obs": z(T, n, 15), "action": z(T, n, A), "reward": z(T, n),
                  "terminated": z(T, n, dtype=u8), "meta": z(2, n, dtype=torch.int32),
                  "prefix": z(n + 1, dtype=torch.int32)}
        if P:
            self.t["obs_img"], self.t["next_img"] = z(T, n, P, dtype=u8), z(T, n, P, dtype=u8)
        if ref is not None:                              # start from a restatement's state
            for k in ref.ARRAYS:
                self.t[k].copy_(_dev(getattr(ref, k)))
        pl, H, W, ch = layout if layout else (0, 0, 0, 0)
        self.rec = _native.SO100Replay(n=n, T=T, action_dim=A, planes=pl, H=H, W=W, chan=ch, P=P, seed=seed,
                                       **{k: _native.ptr(v) for k, v in self.t.items()})
        self.env = _handle()
        assert self.env.lib.so100_replay_storage_bytes(n, T, A, P) == sum(v.numel() * v.element_size()
                                                                          for v in self.t.values())

    def _ok(self, rc):
        assert rc == 0, self.env.lib.so100_last_error()

    def push(self, **rows):
        from gym_so100 import _native
        keep = {k: (_dev(v) if v is not None else None) for k, v in rows.items()}
        st = _native.SO100ReplayStep(**{k: _native.ptr(v) for k, v in keep.items()})
        self._ok(self.env.lib.so100_replay_push(self.env._handle, ctypes.byref(self.rec), ctypes.byref(st),
                                                self.env._stream()))
        torch.cuda.synchronize()

    def stage(self, mask, obs, pixels=None):
        from gym_so100 import _native
        keep = [None if v is None else _dev(v) for v in (mask, obs, pixels)]
        self._ok(self.env.lib.so100_replay_stage(self.env._handle, ctypes.byref(self.rec),
                                                 *[_native.ptr(v) for v in keep], self.env._stream()))
        torch.cuda.synchronize()

    def scan(self):
        self._ok(self.env.lib.so100_replay_scan(self.env._handle, ctypes.byref(self.rec), self.env._stream()))
        torch.cuda.synchronize()
        return self.t["prefix"].cpu().numpy()

    def sample(self, B, call, pad=0, skew=0):
        """one so100_replay_sample (after a scan) -> the outputs as numpy; skew: the image outputs start that many bytes
        past an aligned address"""
        from gym_so100 import _native
        f = lambda *s, dtype=torch.float32: torch.full(s, 7, dtype=dtype, device="cuda")  # noqa: E731
        i32 = torch.int32
        out = {"obs": f(B, 15), "next_obs": f(B, 15), "actions": f(B, self.A), "rewards": f(B), "dones": f(B),
               "env": f(B, dtype=i32), "slot": f(B, dtype=i32), "shift": f(B, 4, dtype=i32)}
        guard = {}
        if self.P:
            for k in ("pixels", "next_pixels"):
                guard[k] = f(B * self.P + skew + 8, dtype=torch.uint8)
                out[k] = guard[k][skew:skew + B * self.P].view(B, self.P)
        rec = _native.SO100ReplayOut(**{k: _native.ptr(v) for k, v in out.items()})
        self.rec.pad = pad
        self._ok(self.env.lib.so100_replay_sample(self.env._handle, ctypes.byref(self.rec), B, ctypes.c_uint64(call),
                                                  ctypes.byref(rec), self.env._stream()))
        torch.cuda.synchronize()
        for k, g in guard.items():                       # nothing before or after the rows is written
            g = g.cpu().numpy()
            assert (g[:skew] == 7).all() and (g[skew + B * self.P:] == 7).all(), k
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


def _imgs(n, t, P, salt=0):
    """[n, P] bytes that encode (env, push index t) and the byte index"""
    e = np.arange(n)[:, None]
    return ((np.arange(P)[None, :] * 7 + 31 * e + 101 * t + salt) % 251).astype(np.uint8)


def _script(n, steps, null_at=()):
    """per push: (terminated, truncated, diverged-or-None) [n] each.  Env 0 (mod 5) never diverges and never finishes
    before push 4, env 1 (mod 5) always diverges, the others finish now and then and diverge rarely; the pushes in
    null_at pass no diverged array at all."""
    rng = np.random.default_rng(n * 1000 + steps)
    idx = np.arange(n)
    out = []
    for t in range(steps):
        done = rng.random(n) < 0.3
        done[idx % 5 == 0] &= t >= 4
        term = done & (rng.random(n) < 0.5)
        div = (rng.random(n) < 0.1) & (idx % 5 != 0)
        div[idx % 5 == 1] = True
        trunc = (done & ~term) | div
        if t in null_at:
            out.append((term.astype(np.uint8), (done & ~term).astype(np.uint8), None))
        else:
            out.append((term.astype(np.uint8), trunc.astype(np.uint8), div.astype(np.uint8)))
    return out


def _push_both(buf, ref, t, term, trunc, div):
    n, A, P = ref.n, ref.A, ref.P
    done = (term | trunc).astype(bool)
    rows = dict(obs=_rows(n, t, 15), final_obs=_rows(n, t, 15, base=0.5), action=_rows(n, t, A, base=0.25),
                reward=(-np.arange(n) - 0.5 * t).astype(np.float32), terminated=term, truncated=trunc, diverged=div)
    if P:
        rows["pixels"] = _imgs(n, t, P)
        rows["final_pixels"] = _imgs(n, t, P, salt=13)   # a finished env's last frame differs from its new first one
        rows["final_pixels"][~done] = 255                # stale rows of the envs that are not done: poison
    else:
        rows["pixels"] = rows["final_pixels"] = None
    if buf is not None:
        buf.push(**rows)
    ref.push(**rows)


# ---------------------------------------------------------------------- push, stage, scan
@pytest.mark.parametrize("layout", ["none", "odd", "planes"])
@pytest.mark.parametrize("n,T,A", [(1, 2, 5), (1, 3, 6), (1, 8, 5), (5, 2, 6), (5, 3, 5), (5, 8, 6), (65, 2, 5),
                                   (65, 3, 6), (65, 8, 5)])
def test_push_equals_the_restatement_after_every_call(n, T, A, layout):
    layout = LAYOUTS[layout]
    buf, ref = Buf(n, T, A, layout), replay_ref.ReplayRef(n, T, A, layout)
    finished = dropped = 0
    for t, (term, trunc, div) in enumerate(_script(n, 3 * T + 2)):
        _push_both(buf, ref, t, term, trunc, div)
        buf.assert_equals(ref, t)
        finished += int((term | trunc).sum())
        dropped += 0 if div is None else int(div.sum())
    assert n == 1 or (finished > 0 and dropped > 0)
    assert (ref.meta[1][np.arange(n) % 5 == 0] == T - 1).all()              # the env that never diverges is full
    assert (ref.meta[1][np.arange(n) % 5 == 1] == 0).all()                  # the one that always does is empty
    if ref.P:
        assert not (ref.next_img == 255).all(axis=2).any()                  # no poisoned row was stored


@pytest.mark.parametrize("layout", ["none", "odd", "planes"])
def test_stage_with_and_without_a_mask(layout):
    layout = LAYOUTS[layout]
    n, T, A = 65, 3, 6
    buf, ref = Buf(n, T, A, layout), replay_ref.ReplayRef(n, T, A, layout)
    P = ref.P
    for t, (term, trunc, div) in enumerate(_script(n, 4, null_at=(1, 2))):     # (a NULL diverged pointer: none dropped)
        _push_both(buf, ref, t, term, trunc, div)
        buf.assert_equals(ref, t)
    assert (ref.meta[1] >= 2).all()
    before = ref.meta.copy()
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    for m, t in ((mask, 50), (None, 60)):
        obs, pix = _rows(n, t, 15), (_imgs(n, t, P) if P else None)
        buf.stage(m, obs, pix)
        ref.stage(m, obs, pix)
        buf.assert_equals(ref, t)
        assert _same(ref.meta, before)                   # no cursor, no count moves
        cur = ref.meta[0]
        hit = np.ones(n, bool) if m is None else m.astype(bool)
        assert _same(buf.host()["obs"][cur[hit], np.flatnonzero(hit)], obs[hit])


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_scan_against_cumsum(n):
    T = 9
    ref = replay_ref.ReplayRef(n, T, 1)
    ref.meta[1] = np.random.default_rng(n).integers(0, T, n)
    ref.meta[1][n // 2] = T - 1
    buf = Buf(n, T, 1, ref=ref)
    pre = buf.scan()
    want = np.cumsum(ref.meta[1].astype(np.int64))
    assert _same(pre[:n].astype(np.int64), want) and int(pre[n]) == int(want[-1])
    assert _same(pre.astype(np.int64), ref.prefix())


# ---------------------------------------------------------------------- sample
_REFS = {}


def _sample_ref(name):
    """one filled restatement per layout, shared and never changed: 5 envs, T = 8, 19 scripted pushes (env 1 always
    diverges: count 0), a masked stage in the middle"""
    if name not in _REFS:
        n, T, A = 5, 8, 6
        ref = replay_ref.ReplayRef(n, T, A, LAYOUTS[name], seed=99)
        for t, (term, trunc, div) in enumerate(_script(n, 19)):
            _push_both(None, ref, t, term, trunc, div)
            if t == 9:
                ref.stage(np.array([0, 0, 1, 1, 0], np.uint8), _rows(n, 70, 15), _imgs(n, 70, ref.P) if ref.P else None)
        assert int(ref.meta[1][1]) == 0 and (ref.meta[1][[0, 2, 3, 4]] > 0).all() and ref.terminated.any()
        _REFS[name] = ref
    return _REFS[name]


@pytest.mark.parametrize("B", [1, 5, 256, 1000])
@pytest.mark.parametrize("pad", [0, 1, 4])
@pytest.mark.parametrize("layout", ["odd", "planes", "cams", "full"])
def test_sample_equals_the_restatement(layout, pad, B):
    ref = _sample_ref(layout)
    before = {k: getattr(ref, k).copy() for k in ref.ARRAYS}
    buf = Buf(ref.n, ref.T, ref.A, ref.layout, seed=99, ref=ref)
    assert _same(buf.scan().astype(np.int64), ref.prefix())
    got = buf.sample(B, call=2, pad=pad, skew=B % 4)
    want = ref.sample(B, call=2, pad=pad)
    assert sorted(got) == sorted(want)
    for k in want:
        assert _same(got[k], want[k]), k
    e, s = got["env"], got["slot"]
    assert (e != 1).all() and all(si in ref.valid_slots(ei) for ei, si in zip(e, s))
    assert _same(got["dones"], ref.terminated[s, e].astype(np.float32))
    if pad == 0:
        assert not got["shift"].any() and _same(got["pixels"], ref.obs_img[s, e])
        assert _same(got["next_pixels"], ref.next_img[s, e])
    else:
        assert got["shift"].min() >= 0 and got["shift"].max() <= 2 * pad
        if B >= 256:
            assert got["shift"].min() == 0 and got["shift"].max() == 2 * pad
            assert (got["shift"][:, :2] != got["shift"][:, 2:]).any()        # the two images shift independently
    # two calls differ; two buffers with the same seed agree bit for bit; the ring is only read
    if B >= 5:
        other = buf.sample(B, call=3, pad=pad)
        assert not _same(other["slot"], got["slot"]) or not _same(other["env"], got["env"])
    twin = Buf(ref.n, ref.T, ref.A, ref.layout, seed=99, ref=ref)
    twin.scan()
    again = twin.sample(B, call=2, pad=pad)
    assert all(_same(again[k], got[k]) for k in got)
    buf.assert_equals(ref, "after the samples")
    assert all(_same(before[k], getattr(ref, k)) for k in before)


@pytest.mark.parametrize("pad", [0, 4])
def test_sample_pieces_of_several_chunks(pad):
    """a batch large enough that a workgroup takes more than one 4,096-byte chunk of a 9,216-byte image (more than 8,192
    one-chunk pieces: B > 1,365)"""
    ref = _sample_ref("full")
    buf = Buf(ref.n, ref.T, ref.A, ref.layout, seed=99, ref=ref)
    buf.scan()
    got, want = buf.sample(1400, call=5, pad=pad, skew=3), ref.sample(1400, call=5, pad=pad)
    assert sorted(got) == sorted(want) and all(_same(got[k], want[k]) for k in want)


@pytest.mark.parametrize("n", [65, 4097])
def test_sample_finds_the_env_among_many(n):
    """the 64-way search of the prefix sums at 2 and 3 rounds, over counts with runs of empty envs"""
    T, A, layout = 3, 5, LAYOUTS["odd"]
    rng = np.random.default_rng(n)
    ref = replay_ref.ReplayRef(n, T, A, layout, seed=11)
    for k in ("obs", "next_obs", "action", "reward"):
        getattr(ref, k)[...] = rng.standard_normal(getattr(ref, k).shape).astype(np.float32)
    for k in ("obs_img", "next_img"):
        getattr(ref, k)[...] = rng.integers(0, 256, getattr(ref, k).shape, dtype=np.uint8)
    ref.terminated[...] = rng.integers(0, 2, ref.terminated.shape)
    ref.meta[0] = rng.integers(0, T, n)
    ref.meta[1] = rng.integers(0, T, n) * (rng.random(n) < 0.5)
    ref.meta[1, :3] = 0                                   # the first and the last envs hold nothing
    ref.meta[1, -3:] = 0
    ref.meta[1, n // 2] = T - 1
    buf = Buf(n, T, A, layout, seed=11, ref=ref)
    assert _same(buf.scan().astype(np.int64), ref.prefix())
    got, want = buf.sample(256, call=1, pad=1), ref.sample(256, call=1, pad=1)
    assert all(_same(got[k], want[k]) for k in want)
    assert (ref.meta[1][got["env"]] > 0).all() and len(set(got["env"].tolist())) >= 16


@pytest.mark.parametrize("B", [1, 5, 256, 1000])
def test_sample_without_images(B):
    n, T, A = 5, 8, 5
    ref = replay_ref.ReplayRef(n, T, A, None, seed=5)
    for t, (term, trunc, div) in enumerate(_script(n, 11)):
        _push_both(None, ref, t, term, trunc, div)
    buf = Buf(n, T, A, None, seed=5, ref=ref)
    buf.scan()
    got, want = buf.sample(B, call=1), ref.sample(B, call=1)
    assert sorted(got) == sorted(want) and all(_same(got[k], want[k]) for k in want)


def test_sample_uses_every_valid_transition():
    """4,000 draws over the shared buffer: every valid (env, slot) comes up, nothing else does"""
    ref = _sample_ref("odd")
    buf = Buf(ref.n, ref.T, ref.A, ref.layout, seed=3, ref=ref)
    buf.scan()
    got = buf.sample(4000, call=0, pad=1)
    valid = {(e, s) for e in range(ref.n) for s in ref.valid_slots(e)}
    assert set(zip(got["env"].tolist(), got["slot"].tolist())) == valid


@pytest.mark.parametrize("layout", ["none", "odd"])
def test_empty_buffer(layout):
    buf = Buf(3, 8, 6, LAYOUTS[layout])
    P = buf.P
    buf.stage(None, _rows(3, 0, 15), _imgs(3, 0, P) if P else None)      # staged rows, no transition
    assert buf.scan().tolist() == [0, 0, 0, 0]
    got = buf.sample(37, call=0, pad=4 if P else 0, skew=1)
    assert (got["slot"] == -1).all() and (got["env"] == 0).all() and not got["shift"].any()
    for k in ("obs", "next_obs", "actions", "rewards", "dones"):
        assert not got[k].any() and not np.signbit(got[k]).any(), k
    if P:
        assert not got["pixels"].any() and not got["next_pixels"].any()


# ---------------------------------------------------------------------- SO100VecEnv(uniform_replay=...)
BASE = dict(task="so100_touch_cube", obs_type="so100_pixels_agent_pos", observation_width=16, observation_height=12,
            max_episode_steps=6)


@pytest.mark.parametrize("variant", ["base", "channels_first_two_cameras", "state"])
def test_closed_loop(variant):
    from gym_so100 import SO100VecEnv
    n, T = 8, 5
    kw = dict(BASE)
    if variant == "channels_first_two_cameras":
        kw.update(channels_first=True, cameras=("top", "left_wrist"))
    if variant == "state":
        kw = dict(task="so100_touch_cube", obs_type="so100_state", max_episode_steps=6)
    pixels = variant != "state"
    env = SO100VecEnv(n, seed=3, uniform_replay=dict(buffer_size=40, augment=True if pixels else None), **kw)
    rp = env.uniform_replay
    layout = {"base": (1, 12, 16, 3), "channels_first_two_cameras": (6, 12, 16, 1), "state": None}[variant]
    assert rp is not None and rp.T == T and rp.capacity == n * (T - 1) and rp.pad == (4 if pixels else 0)
    assert rp.layout == (layout or (0, 0, 0, 0)) and env.replay is None
    with pytest.raises(ValueError):
        rp.sample(4, check=True)                         # nothing stored yet
    assert rp.size() == 0 and (rp.sample(4)["slot"] == -1).all()
    rp.calls = 0
    ref = replay_ref.ReplayRef(n, T, 6, layout, seed=3)
    assert rp.seed == env.base_seed == 3
    pix = lambda t: _np(t).reshape(n, -1) if pixels else None  # noqa: E731
    env.reset()
    ref.stage(None, _np(env.obs), pix(env.pixels))
    rng = np.random.default_rng(0)
    finished = 0
    for t in range(24):
        if t == 15:                                      # a user reset in mid-episode
            mask = np.arange(n) % 3 == 1
            env.reset(mask=torch.from_numpy(mask))
            ref.stage(mask, _np(env.obs), pix(env.pixels))
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        cur = ref.meta[0].copy()
        env.step(torch.from_numpy(a).cuda())
        term, trunc = _np(env.terminated), _np(env.truncated)
        ref.push(_np(env.obs), _np(env.final_obs), a, _np(env.reward), term, trunc, _np(env.diverged),
                 pix(env.pixels), pix(env.final_pixels))
        host = {k: _np(v) for k, v in rp.store.items()}
        for k in ref.ARRAYS:
            assert _same(host[k], getattr(ref, k)), (t, k)
        done = (term | trunc).astype(bool)
        finished += int(done.sum())
        for e in np.flatnonzero(done):                   # the true next observation, not the new episode's first
            assert _same(host["next_obs"][cur[e], e], _np(env.final_obs)[e])
            assert not _same(host["next_obs"][cur[e], e], _np(env.obs)[e])
    assert finished >= 3 * n
    assert rp.size() == int(ref.meta[1].sum()) == n * (T - 1) and int(rp.valid_count.item()) == rp.size()
    shape = tuple(env.pixels.shape[1:]) if pixels else None
    for call, aug in enumerate([None, False, 1] if pixels else [None, False]):
        assert rp.calls == call
        got = rp.sample(256, augment=aug)
        pad = {None: rp.pad, False: 0, 1: 1}[aug]
        want = ref.sample(256, call, pad=pad)
        common = ("actions", "rewards", "dones", "env", "slot", "shift")
        if pixels:
            assert sorted(got) == sorted(common + ("pixels", "next_pixels", "agent_pos", "next_agent_pos", "state",
                                                   "next_state"))
            assert tuple(got["pixels"].shape) == (256,) + shape == tuple(got["next_pixels"].shape)
            assert got["pixels"].dtype == torch.uint8 and got["pixels"].is_cuda
            assert _same(_np(got["pixels"]).reshape(256, -1), want["pixels"])
            assert _same(_np(got["next_pixels"]).reshape(256, -1), want["next_pixels"])
            assert _same(_np(got["state"]), want["obs"]) and _same(_np(got["next_state"]), want["next_obs"])
            assert _same(_np(got["agent_pos"]), want["obs"][:, 9:15])
            assert _same(_np(got["next_agent_pos"]), want["next_obs"][:, 9:15])
        else:
            assert sorted(got) == sorted(common + ("obs", "next_obs"))
            assert _same(_np(got["obs"]), want["obs"]) and _same(_np(got["next_obs"]), want["next_obs"])
        for k in common:
            assert _same(_np(got[k]), want[k]), (call, k)
    if not pixels:
        with pytest.raises(ValueError):
            rp.sample(4, augment=True)
    with pytest.raises(ValueError):
        rp.sample(4, normalize=True)                     # no normaliser
    # step_async_raw stores nothing
    meta = _np(rp.store["meta"])
    env.step_async_raw()
    torch.cuda.synchronize()
    assert _same(_np(rp.store["meta"]), meta)
    env.close()


def test_sb3_buffer_shapes_and_normalize():
    from gym_so100.sb3 import SO100ReplayBuffer, SO100SB3VecEnv
    n = 8
    rng = np.random.default_rng(1)
    venv = SO100SB3VecEnv(n, channels_first=True, normalize=True, uniform_replay=dict(buffer_size=n * 4, augment=2),
                          **BASE)
    venv.reset()
    for _ in range(5):
        venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        venv.step_wait()
    rb = SO100ReplayBuffer(env=venv)
    assert rb.add(1, 2, 3) is None and rb.size() == venv.venv.uniform_replay.size() == n * 3
    assert rb.buffer_size == 4 and rb.n_envs == n
    venv.venv.training = False
    b = rb.sample(32)
    assert b._fields == ("observations", "actions", "next_observations", "dones", "rewards")
    assert tuple(b.rewards.shape) == (32, 1) and tuple(b.dones.shape) == (32, 1) and tuple(b.actions.shape) == (32, 6)
    for obs in (b.observations, b.next_observations):
        assert sorted(obs) == ["agent_pos", "pixels"]
        assert tuple(obs["pixels"].shape) == (32, 3, 12, 16) and obs["pixels"].dtype == torch.uint8
        assert tuple(obs["agent_pos"].shape) == (32, 6) and obs["pixels"].is_cuda
    # the float part is the normalised one, the images are the buffer's own
    rp = venv.venv.uniform_replay
    rp.calls -= 1                                        # the same draws again
    raw = rp.sample(32)
    assert _same(_np(b.observations["pixels"]), _np(raw["pixels"]))
    want = venv.venv.normalize_obs({"agent_pos": raw["agent_pos"]})["agent_pos"]
    assert _same(_np(b.observations["agent_pos"]), _np(want)) and not _same(_np(want), _np(raw["agent_pos"]))
    with pytest.raises(ValueError):
        SO100ReplayBuffer(env=_handle())
    venv.close()
    # the state env: plain tensors
    venv = SO100SB3VecEnv(n, task="so100_touch_cube", max_episode_steps=6, uniform_replay=dict(buffer_size=n * 4))
    venv.reset()
    for _ in range(3):
        venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        venv.step_wait()
    b = SO100ReplayBuffer(env=venv).sample(16)
    assert tuple(b.observations.shape) == (16, 15) == tuple(b.next_observations.shape)
    venv.close()


def test_off_means_untouched_and_the_command_is_stored():
    from gym_so100 import SO100VecEnv

    class Spy:
        def __init__(self, lib):
            self._lib, self.names = lib, []

        def __getattr__(self, name):
            self.names.append(name)
            return getattr(self._lib, name)

    env = _handle()
    assert env.uniform_replay is None
    spy = Spy(env.lib)
    env.lib = spy
    try:
        env.reset()
        env.step(torch.zeros(4, 6, device="cuda"))
    finally:
        env.lib = spy._lib
    assert "so100_step" in spy.names and not [x for x in spy.names if x.startswith("so100_replay")]
    # with ee_delta the stored command is the 5-wide one
    n = 4
    on = SO100VecEnv(n, task="so100_touch_cube", max_episode_steps=4, action_mode="ee_delta",
                     uniform_replay=dict(buffer_size=n * 4))
    assert on.uniform_replay.action_dim == 5
    on.reset()
    a = np.random.default_rng(2).uniform(-1, 1, (n, 5)).astype(np.float32)
    on.step(torch.from_numpy(a).cuda())
    assert _same(_np(on.uniform_replay.store["action"])[0], a)
    assert _np(on.uniform_replay.count).tolist() == [1] * n
    on.close()
