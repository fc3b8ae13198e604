"""The n-step returns of the uniform replay buffer on the GPU (csrc/so100_replay.hip; include/so100.h
so100_replay_push_nstep / so100_replay_stage_nstep / so100_replay_sample_nstep) against the restatement
(tests/replay_nstep_ref.py, itself checked against a brute-force log in tests/test_replay_nstep_cpu.py).  The direct tests
drive the C-ABI with synthetic step rows as tests/test_gpu_replay.py does, whose device-buffer helper they extend; the
rewards are 1 + 2^-20 j, so with gamma = 0.99 a reordered sum or a fused multiply-add would change the last bit.  Every
comparison is bit for bit; output buffers start filled with 7, so a value not written shows."""
import collections
import ctypes

import numpy as np
import pytest

import replay_nstep_ref as R
import test_gpu_replay as G

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LAYOUTS = G.LAYOUTS
_same, _dev, _np = G._same, G._dev, G._np
SEED, CALL, GAMMA = 99, 2, 0.99
START_SIDE = ("obs", "actions", "env", "slot", "shift", "pixels")


class NBuf(G.Buf):
    """the device arrays of one buffer with its `ends` bytes, and the so100_replay_nstep record"""

    def __init__(self, n, T, A, layout=None, seed=0, ref=None, n_step=1, gamma=GAMMA):
        from gym_so100 import _native
        super().__init__(n, T, A, layout, seed)
        self.ends = torch.zeros(T, n, dtype=torch.uint8, device="cuda")
        if ref is not None:                              # start from a restatement's state
            for k in ref.ARRAYS:
                (self.ends if k == "ends" else self.t[k]).copy_(_dev(getattr(ref, k)))
        assert self.env.lib.so100_replay_nstep_storage_bytes(n, T) == self.ends.numel()
        self.ns = _native.SO100ReplayNstep(n_step=n_step, gamma=gamma, ends=_native.ptr(self.ends))

    def host(self):
        h = super().host()
        h["ends"] = self.ends.cpu().numpy()
        return h

    def push_nstep(self, **rows):
        from gym_so100 import _native
        keep = {k: (_dev(v) if v is not None else None) for k, v in rows.items()}
        st = _native.SO100ReplayStep(**{k: _native.ptr(v) for k, v in keep.items()})
        self._ok(self.env.lib.so100_replay_push_nstep(self.env._handle, ctypes.byref(self.rec), ctypes.byref(self.ns),
                                                      ctypes.byref(st), self.env._stream()))
        torch.cuda.synchronize()

    def stage_nstep(self, mask, obs, pixels=None):
        from gym_so100 import _native
        keep = [None if v is None else _dev(v) for v in (mask, obs, pixels)]
        self._ok(self.env.lib.so100_replay_stage_nstep(self.env._handle, ctypes.byref(self.rec), ctypes.byref(self.ns),
                                                       *[_native.ptr(v) for v in keep], self.env._stream()))
        torch.cuda.synchronize()

    def sample_nstep(self, B, call, n_step, gamma=GAMMA, pad=0, skew=0):
        """one so100_replay_sample_nstep (after a scan) -> every output as numpy"""
        from gym_so100 import _native
        f = lambda *s, dtype=torch.float32: torch.full(s, 7, dtype=dtype, device="cuda")  # noqa: E731
        i32 = torch.int32
        out = {"obs": f(B, 15), "next_obs": f(B, 15), "actions": f(B, self.A), "rewards": f(B), "dones": f(B),
               "env": f(B, dtype=i32), "slot": f(B, dtype=i32), "shift": f(B, 4, dtype=i32)}
        more = {"discounts": f(B), "nsteps": f(B, dtype=i32), "last_slot": f(B, dtype=i32)}
        guard = {}
        if self.P:
            for k in ("pixels", "next_pixels"):
                guard[k] = f(B * self.P + skew + 8, dtype=torch.uint8)
                out[k] = guard[k][skew:skew + B * self.P].view(B, self.P)
        rec = _native.SO100ReplayOut(**{k: _native.ptr(v) for k, v in out.items()})
        nrec = _native.SO100ReplayNstepOut(**{k: _native.ptr(v) for k, v in more.items()})
        ns = _native.SO100ReplayNstep(n_step=n_step, gamma=gamma, ends=_native.ptr(self.ends))
        self.rec.pad = pad
        self._ok(self.env.lib.so100_replay_sample_nstep(self.env._handle, ctypes.byref(self.rec), ctypes.byref(ns), B,
                                                        ctypes.c_uint64(call), ctypes.byref(rec), ctypes.byref(nrec),
                                                        self.env._stream()))
        torch.cuda.synchronize()
        for k, g in guard.items():                       # nothing before or after the rows is written
            g = g.cpu().numpy()
            assert (g[:skew] == 7).all() and (g[skew + B * self.P:] == 7).all(), k
        return {k: v.cpu().numpy() for k, v in {**out, **more}.items()}


def _assert_rows(got, want):
    """every device output against the restatement's, bit for bit (the restatement's "reason" and "why" are its own)"""
    keys = sorted(k for k in want if k not in ("reason", "why"))
    assert sorted(got) == keys
    for k in keys:
        assert _same(got[k], want[k]), k


# ---------------------------------------------------------------------- push, stage
def _events(n, T):
    """G._script's terminated / truncated / diverged pattern (env 1 mod 5 always diverges, env 0 mod 5 never) with a
    masked stage after every third push (the mask moves) and an unmasked one after push 3"""
    idx = np.arange(n)
    for t, (term, trunc, div) in enumerate(G._script(n, 3 * T + 2, null_at=(5,))):
        mask = None
        if t % 3 == 1:
            mask = ((idx + t) % 3 == 0).astype(np.uint8)
        yield t, term, trunc, div, (t % 3 == 1 or t == 3), mask


@pytest.mark.parametrize("layout", ["none", "odd", "planes"])
@pytest.mark.parametrize("n,T,A", [(1, 2, 5), (1, 3, 6), (1, 8, 5), (5, 2, 6), (5, 3, 5), (5, 8, 6), (65, 2, 5),
                                   (65, 3, 6), (65, 8, 5)])
def test_push_and_stage_equal_the_restatement_after_every_call(n, T, A, layout):
    layout = LAYOUTS[layout]
    buf, ref = NBuf(n, T, A, layout), R.ReplayNstepRef(n, T, A, layout)
    plain, pref = G.Buf(n, T, A, layout), R.ReplayRef(n, T, A, layout)
    P = ref.P
    why = set()
    stages_at = collections.Counter()
    for t, term, trunc, div, staged, mask in _events(n, T):
        r = R.step_rows(n, t, A, P, term, trunc, div)
        buf.push_nstep(**r)
        ref.push(**r)
        buf.assert_equals(ref, ("push", t))
        plain.push(**r)
        pref.push(**r)
        why |= set(ref.why.ravel().tolist())
        if staged:
            for e in range(n) if mask is None else np.flatnonzero(mask):
                stages_at["empty" if ref.meta[1, e] == 0 else "filled"] += 1
            args = (mask, R.rows(n, 500 + t, 15), R.imgs(n, 500 + t, P) if P else None)
            buf.stage_nstep(*args)
            ref.stage(*args)
            buf.assert_equals(ref, ("stage", t))
            plain.stage(*args)
            pref.stage(*args)
            why |= set(ref.why.ravel().tolist())
        # the arrays the plain launches know are what the plain launches write
        plain.assert_equals(pref, t)
        host, phost = buf.host(), plain.host()
        for k in pref.ARRAYS:
            assert _same(host[k], phost[k]), (t, k)
        assert set(np.unique(host["ends"]).tolist()) <= {0, 1}
    if n >= 5:
        assert {R.WHY_DONE, R.WHY_STAGE, R.WHY_DROP} <= why
        assert stages_at["empty"] > 0 and stages_at["filled"] > 0     # env 1 always diverges: its stage finds count 0
    assert (ref.ends >= ref.terminated).all()            # ends is a superset of the terminated flags


# ---------------------------------------------------------------------- sample
_REFS = {}


def _sample_ref(layout, T=8, n=5):
    """one scripted restatement per (layout, T), shared and never changed"""
    key = (layout, T, n)
    if key not in _REFS:
        _REFS[key] = R.scripted(n, T, 6, LAYOUTS[layout], seed=SEED)
    return _REFS[key]


# (a pad needs images: the state layout takes pad 0 only)
@pytest.mark.parametrize("B", [1, 5, 256, 1000])
@pytest.mark.parametrize("n_step", [1, 2, 3, 16])
@pytest.mark.parametrize("layout,pad", [("none", 0), ("odd", 0), ("odd", 4), ("planes", 0), ("planes", 4), ("cams", 0),
                                        ("cams", 4)])
def test_sample_equals_the_restatement(layout, pad, n_step, B):
    T = 20 if n_step == 16 else 8
    ref = _sample_ref(layout, T)
    before = {k: getattr(ref, k).copy() for k in ref.ARRAYS}
    buf = NBuf(ref.n, T, ref.A, ref.layout, seed=SEED, ref=ref)
    assert _same(buf.scan().astype(np.int64), ref.prefix())
    got = buf.sample_nstep(B, CALL, n_step, pad=pad, skew=B % 4)
    want = ref.sample_nstep(B, CALL, n_step, GAMMA, pad=pad)
    _assert_rows(got, want)
    # the coverage condition, on the restatement's reasons (tests/test_replay_nstep_cpu.py shows the same on the CPU):
    # every window length, the three stop reasons, an end_flag row closed by a done, by a stage and by a drop
    if B == 1000 or (B == 256 and n_step <= 3):
        lengths, reasons, why = R.coverage(want, n_step)
        assert lengths == set(range(1, n_step + 1))
        assert why == {R.WHY_DONE, R.WHY_STAGE, R.WHY_DROP} and R.END_FLAG in reasons
        assert n_step == 1 or reasons == {R.N_REACHED, R.END_FLAG, R.NEWEST}
    e, s, last = got["env"], got["slot"], got["last_slot"]
    assert (e % 5 != 4).all() and all(si in ref.valid_slots(ei) and li in ref.valid_slots(ei)
                                      for ei, si, li in zip(e, s, last))
    assert _same(got["dones"], ref.terminated[last, e].astype(np.float32))
    assert _same(got["next_obs"], ref.next_obs[last, e])
    buf.assert_equals(ref, "after the sample")           # the ring is only read
    assert all(_same(before[k], getattr(ref, k)) for k in before)


@pytest.mark.parametrize("n_step", [1, 2, 3, 16])
@pytest.mark.parametrize("layout,pad", [("none", 0), ("odd", 4), ("cams", 0)])
def test_the_start_side_is_the_plain_sample_and_one_step_is_all_of_it(layout, pad, n_step):
    """for every n_step the fields obs, actions, env, slot, shift and pixels are so100_replay_sample's for the same (seed,
    call, i); with n_step = 1 every shared field is"""
    T = 20 if n_step == 16 else 8
    ref = _sample_ref(layout, T)
    buf = NBuf(ref.n, T, ref.A, ref.layout, seed=SEED, ref=ref)
    buf.scan()
    B = 256
    plain = buf.sample(B, CALL, pad=pad, skew=1)         # so100_replay_sample itself
    got = buf.sample_nstep(B, CALL, n_step, pad=pad, skew=1)
    for k in START_SIDE:
        if k in plain:
            assert _same(got[k], plain[k]), k
    if n_step == 1:
        for k in plain:
            assert _same(got[k], plain[k]), k
        assert (got["nsteps"] == 1).all() and _same(got["last_slot"], got["slot"])
        assert _same(got["discounts"], np.full(B, GAMMA, np.float32))
    else:
        assert not _same(got["rewards"], plain["rewards"]) and not _same(got["next_obs"], plain["next_obs"])
        assert (got["nsteps"] > 1).any() and (got["nsteps"] <= n_step).all()
        if ref.P:
            assert not _same(got["next_pixels"], plain["next_pixels"])


def test_the_sum_keeps_its_order():
    """reward = 1 + 2^-20 j, gamma = 0.99, windows of up to 16: the returns equal the restatement's bit for bit, and they
    would not if the kernel fused the multiply into the add or summed from the far end"""
    T, n_step, B = 20, 16, 1000
    ref = _sample_ref("none", T)
    buf = NBuf(ref.n, T, ref.A, None, seed=SEED, ref=ref)
    buf.scan()
    got = buf.sample_nstep(B, 7, n_step)
    want = ref.sample_nstep(B, 7, n_step, GAMMA)
    assert _same(got["rewards"], want["rewards"]) and _same(got["discounts"], want["discounts"])
    assert _same(got["nsteps"], want["nsteps"])
    f32, g = np.float32, np.float32(GAMMA)
    fused, back = np.zeros(B, f32), np.zeros(B, f32)
    for i in range(B):
        e, s, m = int(got["env"][i]), int(got["slot"][i]), int(got["nsteps"][i])
        rw = [f32(ref.reward[(s + j) % T, e]) for j in range(m)]
        acc, gg = rw[0], g
        for r in rw[1:]:
            acc = f32(np.float64(acc) + np.float64(gg) * np.float64(r))
            gg = f32(gg * g)
        fused[i] = acc
        acc = f32(0)
        for j in reversed(range(m)):
            acc = f32(rw[j] + f32(g * acc))
        back[i] = acc
    assert not _same(fused, got["rewards"]) and not _same(back, got["rewards"])
    assert np.abs(fused - got["rewards"]).max() < 1e-5   # (they differ in the last bits only)
    # gamma = 0 and gamma = 1: the first reward alone, the plain sum
    zero, one = buf.sample_nstep(B, 7, n_step, gamma=0.0), buf.sample_nstep(B, 7, n_step, gamma=1.0)
    _assert_rows(zero, ref.sample_nstep(B, 7, n_step, 0.0))
    _assert_rows(one, ref.sample_nstep(B, 7, n_step, 1.0))
    assert (one["discounts"] == 1).all() and (zero["discounts"] == 0).all()
    assert _same(zero["rewards"], ref.reward[zero["slot"], zero["env"]])


@pytest.mark.parametrize("pad", [0, 4])
def test_sample_pieces_of_several_chunks(pad):
    """n_step = 3 with a batch large enough that an image workgroup takes more than one 4,096-byte chunk of a 9,216-byte
    image (B > 1,365): the image workgroups' own window lookup"""
    ref = _sample_ref("full")
    buf = NBuf(ref.n, ref.T, ref.A, ref.layout, seed=SEED, ref=ref)
    buf.scan()
    got, want = buf.sample_nstep(1400, 5, 3, pad=pad, skew=3), ref.sample_nstep(1400, 5, 3, GAMMA, pad=pad)
    _assert_rows(got, want)
    assert R.covers_everything(want, 3)


@pytest.mark.parametrize("n", [65, 4097])
def test_sample_finds_the_env_among_many(n):
    """the image workgroups' 64-way search of the prefix sums at 2 and 3 rounds, then their window: random rings, cursors
    and counts, `ends` bytes of any non-zero value"""
    T, A, layout, n_step = 6, 5, LAYOUTS["odd"], 3
    rng = np.random.default_rng(n)
    ref = R.ReplayNstepRef(n, T, A, layout, seed=11)
    for k in ("obs", "next_obs", "action", "reward"):
        getattr(ref, k)[...] = rng.standard_normal(getattr(ref, k).shape).astype(np.float32)
    for k in ("obs_img", "next_img"):
        getattr(ref, k)[...] = rng.integers(0, 256, getattr(ref, k).shape, dtype=np.uint8)
    ref.terminated[...] = rng.integers(0, 2, ref.terminated.shape)
    ref.ends[...] = rng.integers(0, 256, ref.ends.shape) * (rng.random(ref.ends.shape) < 0.3)
    ref.meta[0] = rng.integers(0, T, n)
    ref.meta[1] = rng.integers(0, T, n) * (rng.random(n) < 0.5)
    ref.meta[1, :3] = 0
    ref.meta[1, -3:] = 0
    ref.meta[1, n // 2] = T - 1
    buf = NBuf(n, T, A, layout, seed=11, ref=ref)
    assert _same(buf.scan().astype(np.int64), ref.prefix())
    got, want = buf.sample_nstep(256, 1, n_step, pad=1), ref.sample_nstep(256, 1, n_step, GAMMA, pad=1)
    _assert_rows(got, want)
    assert set(want["reason"]) == {R.N_REACHED, R.END_FLAG, R.NEWEST} and len(set(got["env"].tolist())) >= 16
    assert set(got["nsteps"].tolist()) == {1, 2, 3}


@pytest.mark.parametrize("layout", ["none", "odd"])
def test_empty_buffer(layout):
    buf = NBuf(3, 8, 6, LAYOUTS[layout])
    P = buf.P
    buf.stage_nstep(None, R.rows(3, 0, 15), R.imgs(3, 0, P) if P else None)    # staged rows, no transition
    assert not buf.ends.any().item()                     # count == 0: nothing to close
    assert buf.scan().tolist() == [0, 0, 0, 0]
    got = buf.sample_nstep(37, 0, 3, pad=4 if P else 0, skew=1)
    assert (got["slot"] == -1).all() and (got["env"] == 0).all() and not got["shift"].any()
    assert (got["last_slot"] == -1).all() and (got["nsteps"] == 0).all()
    for k in ("obs", "next_obs", "actions", "rewards", "dones", "discounts"):
        assert not got[k].any() and not np.signbit(got[k]).any(), k
    if P:
        assert not got["pixels"].any() and not got["next_pixels"].any()


# ---------------------------------------------------------------------- SO100VecEnv(uniform_replay=dict(n_step=...))
class Spy:
    """the library with a record of the entry points looked up"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("variant", ["pixels", "state"])
def test_closed_loop(variant):
    """8 envs, episodes of 5 steps, n_step = 3, one reset(mask) in mid-episode: after every step the buffer's arrays
    (`ends` included) are the restatement's, and a batch equals both the restatement and the returns summed from a host
    log of the trajectory"""
    from gym_so100 import SO100VecEnv
    n, T, n_step = 8, 8, 3
    pixels = variant == "pixels"
    kw = dict(task="so100_touch_cube", max_episode_steps=5)
    if pixels:
        kw.update(obs_type="so100_pixels_agent_pos", observation_width=16, observation_height=12)
    env = SO100VecEnv(n, seed=3, uniform_replay=dict(buffer_size=n * T, augment=True if pixels else None, n_step=n_step,
                                                     gamma=0.97), **kw)
    rp = env.uniform_replay
    layout = (1, 12, 16, 3) if pixels else None
    assert rp.n_step == n_step and rp.gamma == 0.97 and tuple(rp.ends.shape) == (T, n) and "ends" not in rp.store
    assert (rp.sample(4)["last_slot"] == -1).all()       # nothing stored yet
    rp.calls = 0
    ref = R.ReplayNstepRef(n, T, 6, layout, seed=3)
    pix = lambda t: _np(t).reshape(n, -1) if pixels else None  # noqa: E731
    spy = Spy(env.lib)
    env.lib = rp.lib = spy
    env.reset()
    ref.stage(None, _np(env.obs), pix(env.pixels))
    rng = np.random.default_rng(0)
    log = [collections.deque(maxlen=T - 1) for _ in range(n)]     # (episode, reward, slot)
    episode = [0] * n
    for t in range(17):
        if t == 13:                                      # a user reset in mid-episode (episodes end after 5, 10, 15)
            mask = np.arange(n) % 3 == 1
            env.reset(mask=torch.from_numpy(mask))
            ref.stage(mask, _np(env.obs), pix(env.pixels))
            for e in np.flatnonzero(mask):
                episode[e] += 1
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        cur = ref.meta[0].copy()
        env.step(torch.from_numpy(a).cuda())
        term, trunc, div = _np(env.terminated), _np(env.truncated), _np(env.diverged)
        rew = _np(env.reward)
        ref.push(_np(env.obs), _np(env.final_obs), a, rew, term, trunc, div, pix(env.pixels), pix(env.final_pixels))
        host = {k: _np(v) for k, v in rp.store.items()}
        host["ends"] = _np(rp.ends)
        for k in ref.ARRAYS:
            assert _same(host[k], getattr(ref, k)), (t, k)
        for e in range(n):
            if div[e]:
                episode[e] += 1
                continue
            log[e].append((episode[e], rew[e], int(cur[e])))
            if term[e] or trunc[e]:
                episode[e] += 1
    env.lib = rp.lib = spy._lib
    used = {x for x in spy.names if x.startswith("so100_replay")}
    assert used == {"so100_replay_push_nstep", "so100_replay_stage_nstep"}, used
    assert (ref.why == R.WHY_STAGE).any() and (ref.why == R.WHY_DONE).any()     # a stage cut and a done in the ring
    for call, (kw, ns, gamma) in enumerate([({}, n_step, 0.97), (dict(n_step=1), 1, 0.97),
                                            (dict(n_step=7, gamma=0.5), 7, 0.5)]):
        assert rp.calls == call
        got = rp.sample(256, **kw)
        want = ref.sample_nstep(256, call, ns, gamma, pad=rp.pad)
        common = ("actions", "rewards", "dones", "env", "slot", "shift", "discounts", "last_slot")
        extra = ("pixels", "next_pixels", "agent_pos", "next_agent_pos", "state", "next_state") if pixels else \
            ("obs", "next_obs")
        assert sorted(got) == sorted(common + ("n_steps",) + extra)
        for k in common:
            assert _same(_np(got[k]), want[k]), (call, k)
        assert _same(_np(got["n_steps"]), want["nsteps"])
        if pixels:
            assert _same(_np(got["next_pixels"]).reshape(256, -1), want["next_pixels"])
            assert _same(_np(got["pixels"]).reshape(256, -1), want["pixels"])
            assert _same(_np(got["next_state"]), want["next_obs"]) and _same(_np(got["state"]), want["obs"])
        else:
            assert _same(_np(got["next_obs"]), want["next_obs"]) and _same(_np(got["obs"]), want["obs"])
        # against the host log: the window lies in one episode and the return is the log's
        f32 = np.float32
        for i in range(256):
            e, s, m = int(want["env"][i]), int(want["slot"][i]), int(want["nsteps"][i])
            k0 = [tr[2] for tr in log[e]].index(s)
            win = [log[e][k0 + j] for j in range(m)]
            assert len({tr[0] for tr in win}) == 1 and win[-1][2] == int(want["last_slot"][i])
            if m < ns and k0 + m < len(log[e]):
                assert log[e][k0 + m][0] != win[0][0]    # it stopped early: the next transition is another episode's
            acc, g = f32(win[0][1]), f32(gamma)
            for tr in win[1:]:
                acc = f32(acc + f32(g * f32(tr[1])))
                g = f32(g * f32(gamma))
            assert acc.tobytes() == _np(got["rewards"])[i].tobytes() and g.tobytes() == _np(got["discounts"])[i].tobytes()
        if ns > 1:
            assert len(set(want["nsteps"].tolist())) > 1 and R.END_FLAG in want["reason"]
    with pytest.raises(ValueError):
        rp.sample(4, n_step=8)                           # more than T - 1
    env.close()


def test_off_means_untouched():
    """a buffer built without n_step: no `ends`, today's sample keys, the plain launches only, and the window arguments
    are refused"""
    from gym_so100 import SO100VecEnv
    n = 4
    env = SO100VecEnv(n, task="so100_touch_cube", max_episode_steps=4, uniform_replay=dict(buffer_size=n * 4))
    rp = env.uniform_replay
    assert rp.n_step is None and not hasattr(rp, "ends")
    assert sorted(rp.store) == ["action", "meta", "next_obs", "obs", "prefix", "reward", "terminated"]
    spy = Spy(env.lib)
    env.lib = rp.lib = spy
    try:
        env.reset()
        for _ in range(3):
            env.step(torch.zeros(n, 6, device="cuda"))
        got = rp.sample(16)
    finally:
        env.lib = rp.lib = spy._lib
    assert sorted(got) == sorted(("obs", "next_obs", "actions", "rewards", "dones", "env", "slot", "shift"))
    used = {x for x in spy.names if x.startswith("so100_replay")}
    assert used == {"so100_replay_stage", "so100_replay_push", "so100_replay_scan", "so100_replay_sample"}, used
    for kw in (dict(n_step=1), dict(gamma=0.9)):
        with pytest.raises(ValueError):
            rp.sample(4, **kw)
    env.close()


def test_sb3_buffer_n_steps_and_discounts():
    from gym_so100.sb3 import NStepReplaySamples, ReplaySamples, SO100ReplayBuffer, SO100SB3VecEnv
    n = 8
    rng = np.random.default_rng(1)
    venv = SO100SB3VecEnv(n, task="so100_touch_cube", max_episode_steps=6,
                          uniform_replay=dict(buffer_size=n * 6, n_step=3, gamma=0.95))
    venv.reset()
    for _ in range(8):
        venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        venv.step_wait()
    for kw in (dict(n_steps=2), dict(gamma=0.99), dict(n_steps=3, gamma=0.9)):
        with pytest.raises(ValueError, match="SO100ReplayBuffer"):
            SO100ReplayBuffer(env=venv, **kw)
    for kw in (dict(), dict(n_steps=3), dict(n_steps=3, gamma=0.95), dict(gamma=0.95)):
        rb = SO100ReplayBuffer(env=venv, **kw)
    b = rb.sample(32)
    assert isinstance(b, NStepReplaySamples)
    assert b._fields == ReplaySamples._fields + ("discounts",)
    assert tuple(b.discounts.shape) == (32, 1) == tuple(b.rewards.shape) == tuple(b.dones.shape)
    assert tuple(b.observations.shape) == (32, 15) and b.discounts.is_cuda
    rp = venv.venv.uniform_replay
    rp.calls -= 1                                        # the same draws again
    raw = rp.sample(32)
    assert _same(_np(b.discounts).ravel(), _np(raw["discounts"])) and _same(_np(b.rewards).ravel(), _np(raw["rewards"]))
    g = np.float32(0.95)
    assert set(_np(raw["discounts"]).tolist()) <= {float(g), float(np.float32(g * g)), float(np.float32(g * g) * g)}
    assert set(_np(raw["n_steps"]).tolist()) == {1, 2, 3}
    venv.close()
    # a buffer built without n_step ignores the two arguments, as before
    venv = SO100SB3VecEnv(n, task="so100_touch_cube", max_episode_steps=6, uniform_replay=dict(buffer_size=n * 4))
    venv.reset()
    venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
    venv.step_wait()
    b = SO100ReplayBuffer(env=venv, n_steps=5, gamma=0.5).sample(8)
    assert isinstance(b, ReplaySamples) and b._fields == ReplaySamples._fields
    venv.close()
