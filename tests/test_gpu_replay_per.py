"""Prioritised replay in the uniform replay buffer on the GPU (csrc/so100_replay.hip; include/so100.h
so100_replay_push_per / so100_replay_per_scan / so100_replay_sample_per / so100_replay_per_update) against
the restatement (tests/replay_per_ref.py, itself checked against a brute-force model in tests/test_replay_per_cpu.py).  The
direct tests drive the C-ABI as tests/test_gpu_replay.py does, whose device-buffer helper they extend.  Every comparison is
bit for bit, except at the two `pow` sites (the priority of an update, the importance weight), whose bound POW_BOUND is
explained beside it; output buffers start filled with 7, so a value not written shows."""
import collections
import ctypes

import numpy as np
import pytest

import replay_nstep_ref as N
import replay_per_ref as R
import replay_ref
import test_gpu_replay as G

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LAYOUTS = G.LAYOUTS
_same, _dev, _np = G._same, G._dev, G._np
SEED, GAMMA = 77, 0.99
ALPHA, BETA, EPS = 0.6, 0.4, 1e-6
# The two pow sites against float64.  Measured on an MI355X over the grids of test_pow_sites (4,096 |td| values log-spaced
# over 1e-6 .. 1e3 for alpha in {0.4, 0.6, 1.0}; the weights of 16,384 draws for beta in {0.4, 1.0}): the greatest relative
# error of the device's value was POW_MEASURED (the priorities at alpha = 1.0; 6.6e-8 and 7.7e-8 at 0.4 and 0.6; the weights
# 9.9e-8 and 1.05e-7 at beta 0.4 and 1.0).  The bound is 4 times that (the factor covers values the grids did not
# sample) and must stay within 16 float32 ulp, OpenCL's bound for pow.  It stays at that first run's figure: with the weight's
# base swept over the whole grid (test_pow_sites) the weights' greatest error is 1.20e-7 and 1.29e-7.
ULP = 2.0 ** -23
POW_MEASURED = 1.27e-7
POW_BOUND = 4 * POW_MEASURED
assert POW_BOUND <= 16 * ULP


class PBuf(G.Buf):
    """the device arrays of one buffer with its priorities (and, nstep=True, its `ends` bytes) and their records"""

    def __init__(self, n, T, A, layout=None, seed=0, ref=None, nstep=False, alpha=ALPHA, beta=BETA, eps=EPS):
        from gym_so100 import _native
        super().__init__(n, T, A, layout, seed)
        z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device="cuda")  # noqa: E731
        self.prio = z(T, n, dtype=torch.int32)           # uint32 on the device
        self.sum = z(n + 1, dtype=torch.int64)           # uint64 on the device
        self.max_prio = torch.tensor([R.PRIO_ONE, 0], dtype=torch.int32, device="cuda")
        self.ends = z(T, n, dtype=torch.uint8) if nstep else None
        if ref is not None:                              # start from a restatement's state
            for k in ref.ARRAYS:
                if k == "prio":
                    self.prio.copy_(_dev(ref.prio.view(np.int32)))
                elif k == "ends":
                    self.ends.copy_(_dev(ref.ends))
                else:
                    self.t[k].copy_(_dev(getattr(ref, k)))
            self.set_max_prio(ref.max_prio)
        held = sum(v.numel() * v.element_size() for v in (self.prio, self.sum, self.max_prio))
        assert self.env.lib.so100_replay_per_storage_bytes(n, T) == held == R.per_storage_bytes(n, T)
        self.per = _native.SO100ReplayPer(alpha=alpha, beta=beta, eps=eps, prio=_native.ptr(self.prio),
                                          sum=_native.ptr(self.sum), max_prio=_native.ptr(self.max_prio))
        self.ns = _native.SO100ReplayNstep(n_step=1, gamma=GAMMA, ends=_native.ptr(self.ends)) if nstep else None

    def set_max_prio(self, v):
        self.max_prio.copy_(_dev(np.array([v, 0], np.uint32).view(np.int32)))

    def host(self):
        h = super().host()
        h["prio"] = self.prio.cpu().numpy().view(np.uint32)
        if self.ends is not None:
            h["ends"] = self.ends.cpu().numpy()
        return h

    def host_max_prio(self):
        return int(self.max_prio.cpu().numpy().view(np.uint32)[0])

    def _ns(self):
        return None if self.ns is None else ctypes.byref(self.ns)

    def push_per(self, **rows):
        from gym_so100 import _native
        keep = {k: (_dev(v) if v is not None else None) for k, v in rows.items()}
        st = _native.SO100ReplayStep(**{k: _native.ptr(v) for k, v in keep.items()})
        self._ok(self.env.lib.so100_replay_push_per(self.env._handle, ctypes.byref(self.rec), ctypes.byref(self.per),
                                                    self._ns(), ctypes.byref(st), self.env._stream()))
        torch.cuda.synchronize()

    def stage_any(self, mask, obs, pixels=None):
        """the stage of the buffer's kind: the priorities need none of their own"""
        from gym_so100 import _native
        if self.ns is None:
            return self.stage(mask, obs, pixels)
        keep = [None if v is None else _dev(v) for v in (mask, obs, pixels)]
        self._ok(self.env.lib.so100_replay_stage_nstep(self.env._handle, ctypes.byref(self.rec), ctypes.byref(self.ns),
                                                       *[_native.ptr(v) for v in keep], self.env._stream()))
        torch.cuda.synchronize()

    def per_scan(self):
        """both scans -> sum as Python ints"""
        self.scan()
        self._ok(self.env.lib.so100_replay_per_scan(self.env._handle, ctypes.byref(self.rec), ctypes.byref(self.per),
                                                    self.env._stream()))
        torch.cuda.synchronize()
        return [int(x) for x in self.sum.cpu().numpy().view(np.uint64)]

    def sample_any(self, B, call, per=True, n_step=None, gamma=GAMMA, pad=0, skew=0, beta=BETA):
        """one sample call (after the scans) of the entry point that (per, n_step) name -> every output as numpy"""
        from gym_so100 import _native
        f = lambda *s, dtype=torch.float32: torch.full(s, 7, dtype=dtype, device="cuda")  # noqa: E731
        i32 = torch.int32
        out = {"obs": f(B, 15), "next_obs": f(B, 15), "actions": f(B, self.A), "rewards": f(B), "dones": f(B),
               "env": f(B, dtype=i32), "slot": f(B, dtype=i32), "shift": f(B, 4, dtype=i32)}
        more = {"discounts": f(B), "nsteps": f(B, dtype=i32), "last_slot": f(B, dtype=i32)} if n_step else {}
        pout = {"probs": f(B), "weights": f(B)} if per else {}
        guard = {}
        if self.P:
            for k in ("pixels", "next_pixels"):
                guard[k] = f(B * self.P + skew + 8, dtype=torch.uint8)
                out[k] = guard[k][skew:skew + B * self.P].view(B, self.P)
        rec = _native.SO100ReplayOut(**{k: _native.ptr(v) for k, v in out.items()})
        ns = nrec = None
        if n_step:
            ns = ctypes.byref(_native.SO100ReplayNstep(n_step=n_step, gamma=gamma, ends=_native.ptr(self.ends)))
            nrec = ctypes.byref(_native.SO100ReplayNstepOut(**{k: _native.ptr(v) for k, v in more.items()}))
        self.rec.pad = pad
        lib, h, s = self.env.lib, self.env._handle, self.env._stream()
        if per:
            p = _native.SO100ReplayPer(alpha=self.per.alpha, beta=beta, eps=self.per.eps, prio=_native.ptr(self.prio),
                                       sum=_native.ptr(self.sum), max_prio=_native.ptr(self.max_prio))
            prec = _native.SO100ReplayPerOut(**{k: _native.ptr(v) for k, v in pout.items()})
            self._ok(lib.so100_replay_sample_per(h, ctypes.byref(self.rec), ctypes.byref(p), ns, B, ctypes.c_uint64(call),
                                                 ctypes.byref(rec), nrec, ctypes.byref(prec), s))
        elif n_step:
            self._ok(lib.so100_replay_sample_nstep(h, ctypes.byref(self.rec), ns, B, ctypes.c_uint64(call),
                                                   ctypes.byref(rec), nrec, s))
        else:
            self._ok(lib.so100_replay_sample(h, ctypes.byref(self.rec), B, ctypes.c_uint64(call), ctypes.byref(rec), s))
        torch.cuda.synchronize()
        for k, g in guard.items():                       # nothing before or after the rows is written
            g = g.cpu().numpy()
            assert (g[:skew] == 7).all() and (g[skew + B * self.P:] == 7).all(), k
        return {k: v.cpu().numpy() for k, v in {**out, **more, **pout}.items()}

    def update(self, env_idx, slot_idx, td):
        keep = [_dev(np.array(env_idx, np.int32)), _dev(np.array(slot_idx, np.int32)), _dev(np.array(td, np.float32))]
        from gym_so100 import _native
        self._ok(self.env.lib.so100_replay_per_update(self.env._handle, ctypes.byref(self.rec), ctypes.byref(self.per),
                                                      len(env_idx), *[_native.ptr(v) for v in keep], self.env._stream()))
        torch.cuda.synchronize()


def device_q(td, alpha=ALPHA, eps=EPS):
    """the device's own priority of each |TD error|: a second buffer with one valid slot per row, updated by the same
    values through the same entry point"""
    td = np.asarray(td, np.float32)
    B = len(td)
    probe = PBuf(B, 2, 1, alpha=alpha, eps=eps)
    probe.t["meta"].copy_(_dev(np.stack([np.ones(B, np.int32), np.ones(B, np.int32)])))      # cursor 1, count 1
    probe.prio[0] = 5
    probe.update(np.arange(B), np.zeros(B), td)
    h = probe.host()["prio"]
    assert not h[1].any()                                # the staged slots stay 0
    return [int(x) for x in h[0]]


def _within_pow_bound(q_dev, td, alpha, eps):
    """q itself may differ by 1 + bound * q from the float64 value"""
    for q, x in zip(q_dev, td):
        want = R.priority64(x, alpha, eps)
        if np.isinf(want) or want >= R.PRIO_MAX:
            assert q == R.PRIO_MAX, (x, q)
        else:
            assert abs(q - max(want, 1.0)) <= 1 + POW_BOUND * want, (x, q, want)
    return True


ROW_KEYS = ("obs", "next_obs", "actions", "rewards", "dones", "env", "slot", "shift", "pixels", "next_pixels", "probs",
            "discounts", "nsteps", "last_slot")


def _assert_rows(got, want, beta=BETA):
    """every device output against the restatement's, bit for bit; the weights within the pow bound"""
    keys = sorted(k for k in want if k in ROW_KEYS)
    assert sorted(k for k in got if k != "weights") == keys
    for k in keys:
        assert _same(got[k], want[k]), k
    w64 = np.zeros(len(want["wbase"]))
    hit = want["wbase"] > 0
    w64[hit] = want["wbase"][hit].astype(np.float64) ** -float(np.float32(beta))
    assert (np.abs(got["weights"] - w64) <= POW_BOUND * w64).all()
    assert not got["weights"][~hit].any()


# ---------------------------------------------------------------------- push
@pytest.mark.parametrize("nstep", [False, True])
@pytest.mark.parametrize("layout", ["none", "odd"])
@pytest.mark.parametrize("n,T,A", [(1, 2, 5), (1, 3, 6), (1, 8, 5), (5, 2, 6), (5, 3, 5), (5, 8, 6), (65, 2, 5),
                                   (65, 3, 6), (65, 8, 5)])
def test_push_equals_the_restatement_after_every_call(n, T, A, layout, nstep):
    """3 T + 2 pushes (env 1 mod 5 diverges whenever a diverged array is passed, the others finish and diverge now and then) with stages in between
    and a greater max_prio from push T on: prio and every shared array equal the restatement after every call, and the
    shared arrays are what the plain (or n-step) push writes"""
    layout = LAYOUTS[layout]
    buf, ref = PBuf(n, T, A, layout, nstep=nstep), R.ReplayPerRef(n, T, A, layout, nstep=nstep)
    import test_gpu_replay_nstep as GN
    plain = GN.NBuf(n, T, A, layout) if nstep else G.Buf(n, T, A, layout)
    P = ref.P
    tops = set()
    for t, (term, trunc, div) in enumerate(G._script(n, 3 * T + 2, null_at=(5,))):
        if t == T:                                       # as an update would have left it
            ref.max_prio = 3 * R.PRIO_ONE + 7
            buf.set_max_prio(ref.max_prio)
        if t == 2 * T:
            ref.max_prio = R.PRIO_MAX
            buf.set_max_prio(ref.max_prio)
        r = N.step_rows(n, t, A, P, term, trunc, div)
        buf.push_per(**r)
        ref.push(**r)
        buf.assert_equals(ref, ("push", t))
        (plain.push_nstep if nstep else plain.push)(**r)
        if t % 3 == 1:
            mask = None if t == 1 else ((np.arange(n) + t) % 3 == 0).astype(np.uint8)
            args = (mask, N.rows(n, 500 + t, 15), N.imgs(n, 500 + t, P) if P else None)
            buf.stage_any(*args)
            ref.stage(*args)
            buf.assert_equals(ref, ("stage", t))
            (plain.stage_nstep if nstep else plain.stage)(*args)
        host, phost = buf.host(), plain.host()
        for k in phost:
            if k != "prefix":
                assert _same(host[k], phost[k]), (t, k)
        assert ref.invariant() and buf.host_max_prio() == ref.max_prio
        tops |= set(np.unique(ref.prio).tolist())
    assert {0, R.PRIO_ONE} <= tops and (T < 3 or n == 1 or {3 * R.PRIO_ONE + 7, R.PRIO_MAX} <= tops)
    idx = np.arange(n) % 5
    # full; and the env that diverges whenever it is told holds the one step of push 5, which passes no diverged array
    assert (ref.meta[1][idx == 0] == T - 1).all() and (ref.meta[1][idx == 1] <= 1).all()


# ---------------------------------------------------------------------- scan
@pytest.mark.parametrize("n,T", [(1, 2), (1, 9), (63, 3), (64, 5), (65, 6), (4095, 2), (4096, 3), (4097, 5), (8193, 2)])
def test_scan_sums_in_64_bits(n, T):
    """sum against Python integers around the edges of the sum kernel's 64 envs per workgroup and 4 slot parts and of the
    scan's 4,096-element tile; priorities 1 and 2^32 - 1 among random ones, totals past 2^32 and (n >= 4,095) 2^40"""
    rng = np.random.default_rng(n * 10 + T)
    ref = R.ReplayPerRef(n, T, 1, nstep=False)
    ref.prio[...] = rng.integers(0, 1 << 32, (T, n), dtype=np.uint64).astype(np.uint32)
    ref.prio[:, rng.random(n) < 0.2] = 0
    ref.prio[0, 0], ref.prio[T - 1, n - 1] = R.PRIO_MAX, 1
    ref.prio[1, n // 2] = R.PRIO_MAX
    buf = PBuf(n, T, 1, ref=ref)
    buf.sum.fill_(-1)
    want = ref.sums()
    assert buf.per_scan() == want
    assert want[n] > 1 << 32 and (n < 4095 or want[n] > 1 << 40)
    assert _same(buf.host()["prio"], ref.prio)           # the scan only reads them
    ref.prio[...] = 0
    zero = PBuf(n, T, 1, ref=ref)
    zero.sum.fill_(-1)
    assert zero.per_scan() == [0] * (n + 1)


# ---------------------------------------------------------------------- sample
def _random_ref(n, T, A, layout, seed):
    """a restatement with random contents, cursors and counts and the priority patterns by env mod 5 (n = 1: the
    pattern 3): 0 a full, wrapped ring of random priorities, 1 nothing valid, 2 its whole mass in one slot (count 1), 3 a slot of
    priority 1 right before one of 2^32 - 1 in a full, wrapped ring, 4 a partly filled ring.  `ends` bytes of any non-zero
    value."""
    rng = np.random.default_rng(seed)
    ref = R.ReplayPerRef(n, T, A, layout, seed=SEED)
    for k in ("obs", "next_obs", "action", "reward"):
        getattr(ref, k)[...] = rng.standard_normal(getattr(ref, k).shape).astype(np.float32)
    if ref.P:
        for k in ("obs_img", "next_img"):
            getattr(ref, k)[...] = rng.integers(0, 256, getattr(ref, k).shape, dtype=np.uint8)
    ref.terminated[...] = rng.integers(0, 2, ref.terminated.shape)
    ref.ends[...] = rng.integers(0, 256, ref.ends.shape) * (rng.random(ref.ends.shape) < 0.3)
    kind = np.arange(n) % 5 if n > 1 else np.array([3])
    ref.kind, ref.pair = kind, {}
    for e in range(n):
        c = int(rng.integers(0, T))
        k = {0: T - 1, 1: 0, 2: 1, 3: T - 1, 4: int(rng.integers(1, T))}[int(kind[e])]
        if kind[e] == 3 and T > 2:
            c = T // 2                                   # (wrapped: the oldest slot is c + 1)
        if kind[e] == 0:
            c = T // 3
        ref.meta[:, e] = c, k
        slots = ref.valid_slots(e)
        hi = {0: 1 << 31, 2: 1 << 31, 3: 1 << 28, 4: 1 << 30}.get(int(kind[e]), 2)
        for s in slots:
            ref.prio[s, e] = int(rng.integers(1, hi))
        if kind[e] == 2:
            ref.prio[slots[0], e] = 1 << 31
        if kind[e] == 3:
            j = min(64, k - 1)                           # k = 63, 64 where the ring holds them: across two lanes' runs
            if j >= 1:
                ref.prio[slots[j - 1], e] = 1
            ref.prio[slots[j], e] = R.PRIO_MAX
            ref.pair[e] = (slots[j - 1] if j >= 1 else None, slots[j])
    assert ref.invariant()
    return ref


_REFS = {}


def _shared_ref(n, T, layout):
    """one random restatement per shape, shared and never changed"""
    key = (n, T, layout)
    if key not in _REFS:
        ref = _random_ref(n, T, 6, LAYOUTS[layout], seed=n * 1000 + T)
        _REFS[key] = (ref, {k: getattr(ref, k).copy() for k in ref.ARRAYS})
    return _REFS[key][0]


def _unchanged(n, T, layout):
    ref, before = _REFS[(n, T, layout)]
    return all(_same(before[k], getattr(ref, k)) for k in before)


def _check_patterns(ref, want):
    """what a large batch must hold, on the restatement's own picks"""
    e, s = want["env"], want["slot"]
    kinds = ref.kind[e]
    if ref.n > 1:
        assert not (kinds == 1).any() and {0, 2, 3, 4} <= set(kinds.tolist())     # nothing valid: never drawn
        one = kinds == 2
        assert all(int(si) == ref.valid_slots(int(ei))[0] for ei, si in zip(e[one], s[one]))
    big = [i for i in range(len(e)) if kinds[i] == 3 and int(s[i]) == ref.pair[int(e[i])][1]]
    assert big and all(want["q"][i] == R.PRIO_MAX for i in big)                    # the slot after the priority 1
    if ref.T > 3:
        full = (kinds == 3) | (kinds == 0)
        cur = ref.meta[0][e[full]]
        assert (s[full] > cur).any() and (s[full] < cur).any()                     # both sides of a wrapped ring
    if ref.T > 66:                                       # more than 64 valid slots: picks past the first round
        k = np.array([ref.valid_slots(int(ei)).index(int(si)) for ei, si in zip(e, s)])
        assert (k >= 64).any() and (k < 16).any() and ((k >= 16) & (k < 64)).any()


CASES = [(B, T, n) for B in (1, 5, 256, 1000) for T in (3, 8, 70, 130) for n in (1, 5, 65)]


@pytest.mark.parametrize("B,T,n", CASES)
def test_sample_equals_the_restatement(B, T, n):
    """every (B, T, n); the layout, the pad and n_step go round with the case so that each value meets each T and n:
    env, slot, every gathered row and probs are bit-equal to the restatement's"""
    j = CASES.index((B, T, n))
    layout, pad = [("none", 0), ("odd", 0), ("odd", 4), ("none", 0), ("planes", 0), ("planes", 4)][(j + j // 6) % 6]
    if T > 8 and layout == "planes":
        layout = "odd"                                   # (keeps the large rings' images small)
    n_step = [None, 1, 3][(j + j // 3) % 3] if T > 3 else [None, 1, 2][j % 3]
    ref = _shared_ref(n, T, layout)
    buf = PBuf(n, T, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    assert buf.per_scan() == ref.sums()
    call = 3 + j
    got = buf.sample_any(B, call, n_step=n_step, pad=pad, skew=B % 4)
    want = ref.sample_nstep(B, call, n_step, GAMMA, pad=pad) if n_step else ref.sample(B, call, pad=pad)
    _assert_rows(got, want)
    if B >= 256:
        _check_patterns(ref, want)
    assert all(int(si) in ref.valid_slots(int(ei)) for ei, si in zip(got["env"], got["slot"]))
    buf.assert_equals(ref, "after the sample")           # the ring and the priorities are only read
    assert _unchanged(n, T, layout)


@pytest.mark.parametrize("n_step", [None, 1, 3])
@pytest.mark.parametrize("layout,pad", [("odd", 0), ("odd", 4), ("cams", 0), ("cams", 4)])
def test_sample_images_follow_the_pick(layout, pad, n_step):
    """pad 0 and 4 on two image layouts with every n_step: the image rows are the restatement's, so the image workgroups
    found the slot (and the window) that the float workgroups found"""
    n, T, B = 5, 70, 256
    ref = _shared_ref(n, T, layout)
    buf = PBuf(n, T, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    buf.per_scan()
    got = buf.sample_any(B, 9, n_step=n_step, pad=pad, skew=3)
    want = ref.sample_nstep(B, 9, n_step, GAMMA, pad=pad) if n_step else ref.sample(B, 9, pad=pad)
    _assert_rows(got, want)
    _check_patterns(ref, want)
    if pad == 0:                                         # the rows name their source themselves
        assert _same(got["pixels"], ref.obs_img[got["slot"], got["env"]])
        last = got["last_slot"] if n_step else got["slot"]
        assert _same(got["next_pixels"], ref.next_img[last, got["env"]])
    assert len({(int(a), int(b)) for a, b in zip(got["env"], got["slot"])}) > 20
    assert _unchanged(n, T, layout)


def test_sample_pieces_of_several_chunks():
    """a batch large enough that an image workgroup takes more than one 4,096-byte chunk of a 9,216-byte image"""
    ref = _shared_ref(5, 8, "full")
    buf = PBuf(5, 8, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    buf.per_scan()
    _assert_rows(buf.sample_any(1400, 5, n_step=3, pad=4, skew=1), ref.sample_nstep(1400, 5, 3, GAMMA, pad=4))


def test_sample_finds_the_env_among_many():
    """4,097 envs: three rounds of the 64-way search on the 64-bit sums, and the 16-lane groups' bisection"""
    n, T = 4097, 6
    ref = _shared_ref(n, T, "odd")
    buf = PBuf(n, T, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    sums = buf.per_scan()
    assert sums == ref.sums() and sums[n] > 1 << 40
    got, want = buf.sample_any(256, 1, n_step=3, pad=1), ref.sample_nstep(256, 1, 3, GAMMA, pad=1)
    _assert_rows(got, want)
    assert len(set(got["env"].tolist())) >= 64 and got["env"].max() > 3000 and got["env"].min() < 1000


def _scripted(n, T, layout, nstep):
    """a restatement filled by pushes alone (replay_nstep_ref's scripted episodes): every priority is PRIO_ONE"""
    ref = R.ReplayPerRef(n, T, 6, LAYOUTS[layout], seed=SEED, nstep=nstep)
    for t, (term, trunc, div, mask) in enumerate(N.scripted_events(n, T)):
        ref.push(**N.step_rows(n, t, 6, ref.P, term, trunc, div))
        if mask is not None:
            ref.stage(mask, N.rows(n, 500 + t, 15), N.imgs(n, 500 + t, ref.P) if ref.P else None)
    return ref


@pytest.mark.parametrize("prio", [R.PRIO_ONE, 1, R.PRIO_MAX])
@pytest.mark.parametrize("layout,pad,n_step", [("none", 0, None), ("none", 0, 3), ("odd", 4, None), ("cams", 0, 3),
                                               ("odd", 4, 1)])
def test_equal_priorities_are_the_plain_sample(layout, pad, n_step, prio):
    """a freshly filled buffer (everything at PRIO_ONE), and the same with every priority 1 or 2^32 - 1: every shared
    output of so100_replay_sample_per is so100_replay_sample's (so100_replay_sample_nstep's) bit for bit"""
    ref = _scripted(5, 8, layout, nstep=True)
    assert set(np.unique(ref.prio).tolist()) == {0, R.PRIO_ONE} and ref.invariant()
    ref.prio[ref.prio > 0] = prio
    buf = PBuf(5, 8, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    sums = buf.per_scan()
    count = int(ref.meta[1].sum())
    assert sums[5] == count * prio
    B = 300
    got = buf.sample_any(B, 4, n_step=n_step, pad=pad, skew=1)
    plain = buf.sample_any(B, 4, per=False, n_step=n_step, pad=pad, skew=1)
    assert set(got) == set(plain) | {"probs", "weights"}
    for k in plain:
        assert _same(got[k], plain[k]), k
    assert _same(got["probs"], np.full(B, np.float32(1 / count)))
    # (count * (float)(1 / count))^-beta: the base is 1 to within an ulp, not 1, so the float64 value is taken of it
    base = np.float64(np.float32(count) * np.float32(1 / count))
    assert np.abs(got["weights"] - base ** -float(np.float32(BETA))).max() <= POW_BOUND * base ** -float(np.float32(BETA))
    assert len({(int(a), int(b)) for a, b in zip(got["env"], got["slot"])}) == count


@pytest.mark.parametrize("layout", ["none", "odd"])
@pytest.mark.parametrize("n_step", [None, 3])
def test_empty_buffer(layout, n_step):
    buf = PBuf(3, 8, 6, LAYOUTS[layout], nstep=True)
    P = buf.P
    buf.stage_any(None, N.rows(3, 0, 15), N.imgs(3, 0, P) if P else None)      # staged rows, no transition
    assert buf.per_scan() == [0, 0, 0, 0] and not buf.prio.any().item()
    got = buf.sample_any(37, 0, n_step=n_step, pad=4 if P else 0, skew=1)
    assert (got["slot"] == -1).all() and (got["env"] == 0).all() and not got["shift"].any()
    for k in ("obs", "next_obs", "actions", "rewards", "dones", "probs", "weights"):
        assert not got[k].any() and not np.signbit(got[k]).any(), k
    if n_step:
        assert (got["last_slot"] == -1).all() and (got["nsteps"] == 0).all() and not got["discounts"].any()
    if P:
        assert not got["pixels"].any() and not got["next_pixels"].any()
    # an update with the rows of an empty buffer changes nothing
    buf.update(got["env"], got["slot"], np.ones(37))
    assert not buf.prio.any().item() and buf.host_max_prio() == R.PRIO_ONE


def test_two_calls_differ_and_twins_agree():
    ref = _shared_ref(5, 8, "odd")
    a = PBuf(5, 8, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    b = PBuf(5, 8, 6, ref.layout, seed=SEED, ref=ref, nstep=True)
    a.per_scan(), b.per_scan()
    one, two, twin = a.sample_any(256, 0, pad=4), a.sample_any(256, 1, pad=4), b.sample_any(256, 0, pad=4)
    for k in one:
        assert _same(one[k], twin[k]), k
    assert not _same(one["slot"], two["slot"]) and not _same(one["shift"], two["shift"])
    other = PBuf(5, 8, 6, ref.layout, seed=SEED + 1, ref=ref, nstep=True)
    other.per_scan()
    assert not _same(other.sample_any(256, 0, pad=4)["slot"], one["slot"])


# ---------------------------------------------------------------------- update
def _update_rows(ref, B, rng):
    """(env, slot, td, what): rows of every kind first, random valid rows after them, cut to B"""
    n, T = ref.n, ref.T
    full = [e for e in range(n) if ref.meta[1, e] == T - 1]
    part = [e for e in range(n) if 0 < ref.meta[1, e] < T - 1]
    a, b = (full[0], ref.valid_slots(full[0])[1]), (full[1], ref.valid_slots(full[1])[0])
    stale = (part[0], (int(ref.meta[0, part[0]]) + 1) % T)         # a slot outside the env's valid interval
    staged = (full[0], int(ref.meta[0, full[0]]))                  # the slot at the cursor
    rows = [(*a, 0.01, "up"), (*b, 100.0, "down"), (*a, 1.0, "up"), (*b, 1.0, "down"), (*a, 100.0, "up"),
            (*b, 0.01, "down"), (*stale, 50.0, "stale"), (*staged, 50.0, "stale"), (-1, 0, 5.0, "range"),
            (n, 0, 5.0, "range"), (0, T, 5.0, "range"), (0, -3, 5.0, "range"), (n + 5, T + 5, 5.0, "range"),
            (0, -1, 5.0, "minus one"), (-1, -1, 5.0, "minus one"),
            (full[2], ref.valid_slots(full[2])[0], float("nan"), "nan"),
            (full[2], ref.valid_slots(full[2])[1], float("inf"), "inf"),
            (full[2], ref.valid_slots(full[2])[2], -3.0, "negative")]
    valid = [(e, s) for e in range(n) for s in ref.valid_slots(e)]
    while len(rows) < B:
        e, s = valid[int(rng.integers(0, len(valid)))]
        rows.append((e, s, float(np.float32(10.0 ** rng.uniform(-6, 3))), "random"))
    rows = rows[:B]
    order = rng.permutation(B) if B > 18 else np.arange(B)         # the kinds spread over the waves
    rows = [rows[i] for i in order]
    return ([r[0] for r in rows], [r[1] for r in rows], np.array([r[2] for r in rows], np.float32),
            collections.Counter(r[3] for r in rows))


@pytest.mark.parametrize("B", [1, 5, 256, 1000])
@pytest.mark.parametrize("nstep", [False, True])
def test_update_takes_the_greatest_and_skips_what_left(B, nstep):
    """small rings (28 valid transitions), so duplicates are certain; the device's own q of every row is read from a
    second buffer with one slot per row; prio and max_prio then equal the restatement fed those q, and a twin buffer
    given the same call ends bit-equal"""
    rng = np.random.default_rng(B)
    n, T = 6, 8
    ref = R.ReplayPerRef(n, T, 2, nstep=nstep)
    ref.meta[0] = [3, 0, 7, 5, 2, 1]
    ref.meta[1] = [7, 7, 7, 3, 0, 4]
    for e in range(n):
        for s in ref.valid_slots(e):
            ref.prio[s, e] = int(rng.integers(1, 1 << 20))
    ref.max_prio = 2 * R.PRIO_ONE
    env_idx, slot_idx, td, kinds = _update_rows(ref, B, rng)
    if B >= 256:
        assert kinds["up"] == kinds["down"] == 3 and kinds["stale"] == 2 and kinds["range"] == 5
        assert kinds["minus one"] == 2 and kinds["nan"] == kinds["inf"] == kinds["negative"] == 1
        assert len(set(zip(env_idx, slot_idx))) < B - 100             # duplicates among the random rows too
    buf, twin = PBuf(n, T, 2, ref=ref, nstep=nstep), PBuf(n, T, 2, ref=ref, nstep=nstep)
    q = device_q(td)
    assert _within_pow_bound(q, td, ALPHA, EPS)
    before = ref.prio.copy()
    applied = ref.update(env_idx, slot_idx, q)
    buf.update(env_idx, slot_idx, td)
    twin.update(env_idx[::-1], slot_idx[::-1], td[::-1])             # the same rows the other way round
    assert _same(buf.host()["prio"], ref.prio) and buf.host_max_prio() == ref.max_prio
    assert _same(twin.host()["prio"], ref.prio) and twin.host_max_prio() == ref.max_prio
    buf.assert_equals(ref, "after the update")           # nothing else is written
    assert ref.invariant()
    if B >= 5:                                           # the greatest of three, whichever order they come in
        hundred = device_q([100.0])[0]
        ups = [j for j in range(B) if abs(td[j] - 100.0) < 1e-3 and j in applied]
        assert len(ups) == 2 and all(ref.prio[slot_idx[j], env_idx[j]] >= hundred for j in ups)
        if B == 5:                                       # (in the larger batches a random row may name the slot too)
            assert all(ref.prio[slot_idx[j], env_idx[j]] == hundred for j in ups)
    if B >= 256:
        assert ref.max_prio == R.PRIO_MAX and len(applied) == B - 9   # the inf row; stale, range and -1 rows skipped
        assert (ref.prio != before).sum() >= 20
    else:
        assert ref.max_prio == max(2 * R.PRIO_ONE, max(q[j] for j in applied))


def test_update_then_scan_then_sample():
    """the three launches in a row on one stream, with no synchronisation between them"""
    ref = _scripted(5, 8, "none", nstep=False)
    buf = PBuf(5, 8, 6, None, seed=SEED, ref=ref)
    valid = [(e, s) for e in range(5) for s in ref.valid_slots(e)]
    td = np.array([0.001 * 3 ** (j % 9) for j in range(len(valid))], np.float32)
    q = device_q(td)
    ref.update([v[0] for v in valid], [v[1] for v in valid], q)
    buf.update([v[0] for v in valid], [v[1] for v in valid], td)
    assert buf.per_scan() == ref.sums()
    got, want = buf.sample_any(1000, 2), ref.sample(1000, 2)
    _assert_rows(got, want)
    # the greater priorities are drawn more often: the top third of the priorities takes most of the rows
    top = sorted(q)[2 * len(q) // 3]
    assert sum(1 for x in want["q"] if x >= top) > 600


# ---------------------------------------------------------------------- the two pow sites
def _covers_the_grid(base):
    """the bases of the weights reach every eighth of a decade of 1e-4 .. 1e3 (the priorities' grid is 1e-6 .. 1e3 in
    |td|, which alpha = 0.4 .. 1.0 maps into 4e-3 .. 1e3), with at least 4,096 distinct values among them"""
    bins = np.floor(np.log10(base[(base >= 1e-4) & (base < 1e3)].astype(np.float64)) * 8).astype(int)
    return set(bins.tolist()) == set(range(-32, 24)) and len(np.unique(base)) >= 4096


def test_pow_sites(capsys):
    """the priority (|td| + eps)^alpha and the weight (count probs)^-beta against float64 on the grids; prints the
    greatest relative errors, which POW_MEASURED records"""
    td = np.logspace(-6, 3, 4096).astype(np.float32)
    worst = {}
    for alpha in (0.4, 0.6, 1.0):
        q = device_q(td, alpha=alpha)
        want = np.array([R.priority64(x, alpha, EPS) for x in td])
        # (the rounding to an integer adds up to 0.5, and below 1 the clamp answers: what is left is the pow site's)
        err = np.maximum(np.abs(np.array(q, np.float64) - want) - 0.5, 0) / want
        worst["q", alpha] = float(err[want >= 1].max())
        assert _within_pow_bound(q, td, alpha, EPS)
    # alpha = 0 is allowed and makes every priority 1.0, an infinite |td| included: powf(inf, 0) = 1
    special = [float("inf"), float("nan"), 0.0, 1e3]
    assert device_q(special, alpha=0.0) == [R.PRIO_ONE] * 4 == [R.clamp_priority(R.priority64(x, 0.0, EPS)) for x in special]
    assert device_q(special[:2], alpha=1.0) == [R.PRIO_MAX, 1]
    n, T = 64, 65
    ref = R.ReplayPerRef(n, T, 1, seed=SEED, nstep=False)
    ref.meta[0], ref.meta[1] = T - 1, T - 1
    grid = [R.clamp_priority(R.priority64(x, 0.4, EPS)) for x in td]
    ref.prio[:T - 1] = np.array(grid, np.uint32).reshape(T - 1, n)
    buf = PBuf(n, T, 1, seed=SEED, ref=ref)
    assert buf.per_scan() == ref.sums()
    want = ref.sample(16384, 0)
    assert len({(int(a), int(b)) for a, b in zip(want["env"], want["slot"])}) > 1500
    # Draws are proportional, so the slots of low priority are hardly drawn and the probs of one batch span two decades.
    # The base of the weight is (float)prefix[n] * probs, and prefix[n] is a device word like any other: written directly
    # (as prio is), 1 .. 10^7 in 15 steps, it moves those probs over the whole range of the priorities' grid and past it.
    counts = [int(round(10 ** (j / 2))) for j in range(15)]
    assert _covers_the_grid(np.concatenate([np.float32(c) * want["probs"] for c in counts]))
    for beta in (0.4, 1.0):
        worst["w", beta] = 0.0
        for c in counts:
            buf.t["prefix"][n] = c
            got = buf.sample_any(16384, 0, beta=beta)
            assert _same(got["probs"], want["probs"]) and _same(got["slot"], want["slot"])
            base = (np.float32(c) * want["probs"]).astype(np.float32)
            w64 = base.astype(np.float64) ** -float(np.float32(beta))
            worst["w", beta] = max(worst["w", beta], float((np.abs(got["weights"] - w64) / w64).max()))
        assert worst["w", beta] <= POW_BOUND
    with capsys.disabled():
        print("\npow sites, greatest relative error against float64:",
              ", ".join(f"{k[0]} {k[1]}: {v:.3e}" for k, v in worst.items()), f"(bound {POW_BOUND:.3e})")
    assert max(worst.values()) <= POW_BOUND


# ---------------------------------------------------------------------- SO100VecEnv(uniform_replay=dict(prioritized=...))
class Spy:
    """the library with a record of the entry points looked up"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("n_step", [None, 3])
@pytest.mark.parametrize("variant", ["pixels", "state"])
def test_closed_loop(variant, n_step):
    """8 envs, episodes of 5 steps, T = 8, one reset(mask) in mid-episode; every third step a batch is sampled and its
    priorities are updated from a scripted |td|.  The restatement is fed the recorded tensors (and the device's own q of
    each |td|); after every call the buffer's arrays are the restatement's and prio > 0 exactly on the valid interval of
    every env"""
    from gym_so100 import SO100VecEnv
    n, T = 8, 8
    pixels = variant == "pixels"
    kw = dict(task="so100_touch_cube", max_episode_steps=5)
    if pixels:
        kw.update(obs_type="so100_pixels_agent_pos", observation_width=16, observation_height=12)
    opts = dict(buffer_size=n * T, augment=True if pixels else None, prioritized=dict(alpha=0.7, beta=0.5, eps=1e-3))
    if n_step:
        opts.update(n_step=n_step, gamma=0.97)
    env = SO100VecEnv(n, seed=3, uniform_replay=opts, **kw)
    rp = env.uniform_replay
    layout = (1, 12, 16, 3) if pixels else None
    assert rp.prioritized == dict(alpha=0.7, beta=0.5, eps=1e-3) and tuple(rp.prio.shape) == (T, n)
    assert "prio" not in rp.store and sorted(rp.store) == sorted(
        ["action", "meta", "next_obs", "obs", "prefix", "reward", "terminated"] + (["next_img", "obs_img"] if pixels else []))
    first = rp.sample(4)
    assert (first["slot"] == -1).all() and not first["weights"].any().item() and not first["probs"].any().item()
    rp.calls = 0
    ref = R.ReplayPerRef(n, T, 6, layout, seed=3, nstep=bool(n_step))
    pix = lambda t: _np(t).reshape(n, -1) if pixels else None  # noqa: E731

    def check(where):
        host = {k: _np(v) for k, v in rp.store.items()}
        host["prio"] = _np(rp.prio).view(np.uint32)
        if n_step:
            host["ends"] = _np(rp.ends)
        for k in ref.ARRAYS:
            assert _same(host[k], getattr(ref, k)), (where, k)
        assert int(_np(rp.max_prio).view(np.uint32)[0]) == ref.max_prio and ref.invariant()
        assert _same(_np(rp.prio_u32()), ref.prio.astype(np.int64))

    spy = Spy(env.lib)
    env.lib = rp.lib = spy
    env.reset()
    ref.stage(None, _np(env.obs), pix(env.pixels))
    rng = np.random.default_rng(0)
    sampled = updated = 0
    for t in range(17):
        if t == 13:                                      # a user reset in mid-episode (episodes end after 5, 10, 15)
            mask = np.arange(n) % 3 == 1
            env.reset(mask=torch.from_numpy(mask))
            ref.stage(mask, _np(env.obs), pix(env.pixels))
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        env.step(torch.from_numpy(a).cuda())
        ref.push(_np(env.obs), _np(env.final_obs), a, _np(env.reward), _np(env.terminated), _np(env.truncated),
                 _np(env.diverged), pix(env.pixels), pix(env.final_pixels))
        check(("step", t))
        if t % 3 == 2:
            B = 64
            beta = None if t < 9 else 1.0
            got = rp.sample(B, **({} if beta is None else dict(beta=beta)))
            want = ref.sample_nstep(B, sampled, n_step, 0.97, pad=rp.pad) if n_step else \
                ref.sample(B, sampled, pad=rp.pad)
            sampled += 1
            for k in ("env", "slot", "rewards", "dones", "actions", "shift", "probs"):
                assert _same(_np(got[k]), want[k]), (t, k)
            assert _same(_np(got["state" if pixels else "obs"]), want["obs"])
            assert _same(_np(got["next_state" if pixels else "next_obs"]), want["next_obs"])
            if pixels:
                assert _same(_np(got["pixels"]).reshape(B, -1), want["pixels"])
                assert _same(_np(got["next_pixels"]).reshape(B, -1), want["next_pixels"])
            if n_step:
                assert _same(_np(got["n_steps"]), want["nsteps"]) and _same(_np(got["discounts"]), want["discounts"])
            w64 = want["wbase"].astype(np.float64) ** -(0.5 if beta is None else 1.0)
            w64 /= w64.max()
            w = _np(got["weights"])
            # (a quotient of two values within POW_BOUND each, rounded once more)
            assert w.max() == 1.0 and (np.abs(w - w64) <= (2 * POW_BOUND + ULP) * w64).all()
            # |td| scripted from the row: some slots several times with different values, a NaN and an inf
            td = (0.01 + np.abs(_np(got["rewards"])) * (1 + np.arange(B) % 3)).astype(np.float32)
            td[5], td[6] = np.nan, (np.inf if t == 14 else 2.5)
            # a stale batch: the rows of the sample after push 8 again; those of push 7 lie at the cursor now
            if t == 14:
                env_idx, slot_idx = np.concatenate([held[0], _np(got["env"])]), np.concatenate([held[1], _np(got["slot"])])
                td = np.concatenate([held[2], td])
                rp.update_priorities(torch.from_numpy(env_idx).cuda(), torch.from_numpy(slot_idx).cuda().long(),
                                     torch.from_numpy(td).cuda().double())
            else:
                env_idx, slot_idx = _np(got["env"]), _np(got["slot"])
                rp.update_priorities(got["env"], got["slot"], torch.from_numpy(td).cuda())
            if t == 8:
                held = (env_idx.copy(), slot_idx.copy(), td.copy())
            q = device_q(td, alpha=0.7, eps=1e-3)
            applied = ref.update(env_idx, slot_idx, q)
            if t == 14:
                assert len(applied) < len(td)            # rows of that batch have left the ring
            updated += 1
            check(("update", t))
    env.lib = rp.lib = spy._lib
    used = {x for x in spy.names if x.startswith("so100_replay")}
    assert used == {"so100_replay_push_per", "so100_replay_stage_nstep" if n_step else "so100_replay_stage",
                    "so100_replay_scan", "so100_replay_per_scan", "so100_replay_sample_per",
                    "so100_replay_per_update"}, used
    # a scan follows a push or an update only: 5 samples, each after a step and an update
    assert spy.names.count("so100_replay_per_scan") == 5 == sampled == updated
    assert ref.max_prio == R.PRIO_MAX and len(set(np.unique(ref.prio).tolist())) > 5
    with pytest.raises(ValueError):
        rp.sample(4, beta=1.5)
    env.close()


def test_off_means_untouched():
    """a buffer built without prioritized: none of the arrays, today's sample keys, the plain launches only, and the new
    arguments are refused"""
    from gym_so100 import SO100VecEnv
    n = 4
    env = SO100VecEnv(n, task="so100_touch_cube", max_episode_steps=4, uniform_replay=dict(buffer_size=n * 4))
    rp = env.uniform_replay
    assert rp.prioritized is None and rp._per is None and not hasattr(rp, "prio") and not hasattr(rp, "prio_sum")
    assert sorted(rp.store) == ["action", "meta", "next_obs", "obs", "prefix", "reward", "terminated"]
    ref = replay_ref.ReplayRef(n, 4, 6, seed=env.base_seed)
    spy = Spy(env.lib)
    env.lib = rp.lib = spy
    try:
        env.reset()
        ref.stage(None, _np(env.obs))
        for _ in range(3):
            a = torch.zeros(n, 6, device="cuda")
            env.step(a)
            ref.push(_np(env.obs), _np(env.final_obs), _np(a), _np(env.reward), _np(env.terminated), _np(env.truncated),
                     _np(env.diverged))
        got = rp.sample(16)
    finally:
        env.lib = rp.lib = spy._lib
    want = ref.sample(16, 0)
    assert sorted(got) == sorted(("obs", "next_obs", "actions", "rewards", "dones", "env", "slot", "shift"))
    for k in got:
        assert _same(_np(got[k]), want[k]), k
    used = {x for x in spy.names if x.startswith("so100_replay")}
    assert used == {"so100_replay_stage", "so100_replay_push", "so100_replay_scan", "so100_replay_sample"}, used
    with pytest.raises(ValueError):
        rp.sample(4, beta=0.4)
    with pytest.raises(ValueError):
        rp.update_priorities(got["env"], got["slot"], got["rewards"])
    env.close()


def test_sb3_buffer_weights_and_update():
    from gym_so100.sb3 import (NStepReplaySamples, PrioritizedNStepReplaySamples, PrioritizedReplaySamples,
                               ReplaySamples, SO100ReplayBuffer, SO100SB3VecEnv)
    n = 8
    rng = np.random.default_rng(1)
    for extra, kind, base in [(dict(), PrioritizedReplaySamples, ReplaySamples),
                              (dict(n_step=3, gamma=0.95), PrioritizedNStepReplaySamples, NStepReplaySamples)]:
        venv = SO100SB3VecEnv(n, task="so100_touch_cube", max_episode_steps=6,
                              uniform_replay=dict(buffer_size=n * 6, prioritized=True, **extra))
        venv.reset()
        for _ in range(8):
            venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
            venv.step_wait()
        rb = SO100ReplayBuffer(env=venv)
        b = rb.sample(32)
        assert isinstance(b, kind) and b._fields == base._fields + ("weights", "env_indices", "slot_indices")
        assert tuple(b.weights.shape) == (32, 1) == tuple(b.rewards.shape) and b.weights.is_cuda
        assert tuple(b.env_indices.shape) == (32,) == tuple(b.slot_indices.shape) and b.env_indices.dtype == torch.int32
        assert _same(_np(b.weights), np.ones((32, 1), np.float32))       # a fresh buffer: equal priorities
        rp = venv.venv.uniform_replay
        before = _np(rp.prio_u32())
        rb.update_priorities(b.env_indices, b.slot_indices, torch.arange(32, device="cuda") * 0.25)
        after = _np(rp.prio_u32())
        assert ((before > 0) == (after > 0)).all() and (after != before).any()
        assert int(_np(rp.max_prio).view(np.uint32)[0]) == after.max() > R.PRIO_ONE
        w = _np(rb.sample(256).weights)
        assert w.max() == 1.0 and w.min() < 1.0 and (w > 0).all()
        venv.close()
    venv = SO100SB3VecEnv(n, task="so100_touch_cube", max_episode_steps=6, uniform_replay=dict(buffer_size=n * 4))
    venv.reset()
    venv.step_async(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
    venv.step_wait()
    rb = SO100ReplayBuffer(env=venv)
    assert type(rb.sample(8)) is ReplaySamples
    with pytest.raises(ValueError):
        rb.update_priorities(torch.zeros(1), torch.zeros(1), torch.zeros(1))
    venv.close()
