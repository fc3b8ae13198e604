"""CPU checks of the n-step returns of the uniform replay buffer (include/so100.h so100_replay_push_nstep /
so100_replay_stage_nstep / so100_replay_sample_nstep): the new symbols and struct mirrors under the
unchanged ABI 25, every refusal of the three entry points (none needs a device), the option parsing, and the restatement
(tests/replay_nstep_ref.py) against a brute-force log of every transition with its episode id, before the GPU is
involved.  The last tests check that the scripted episodes of tests/test_gpu_replay_nstep.py cover what they claim."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

import replay_nstep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEP_SYMBOLS = ("so100_replay_nstep_bytes", "so100_replay_nstep_out_bytes", "so100_replay_nstep_storage_bytes",
                 "so100_replay_push_nstep", "so100_replay_stage_nstep", "so100_replay_sample_nstep")


# ---------------------------------------------------------------------- ABI
def test_symbols_and_abi():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25
    header = open(os.path.join(ROOT, "include", "so100.h")).read()
    assert re.search(r"#define SO100_ABI_VERSION 25\b", header)
    assert re.search(r"#define SO100_REPLAY_MAX_NSTEP 16\b", header)
    assert _native.SO100_REPLAY_MAX_NSTEP == R.MAX_NSTEP == 16
    for fn in NSTEP_SYMBOLS:
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn), fn
        assert re.search(r"\b%s\(" % fn, header), fn


def test_struct_mirrors_and_storage():
    from gym_so100 import _native
    lib = _native.load()
    assert lib.so100_replay_nstep_bytes() == ctypes.sizeof(_native.SO100ReplayNstep) == 16 + 8
    assert lib.so100_replay_nstep_out_bytes() == ctypes.sizeof(_native.SO100ReplayNstepOut) == 8 + 3 * 8
    assert lib.so100_replay_bytes() == ctypes.sizeof(_native.SO100Replay) == 40 + 8 + 9 * 8        # unchanged
    ns = _native.SO100ReplayNstep(n_step=3, gamma=0.5, ends=ctypes.c_void_p(0x1000))
    assert (ns.size, ns.n_step, ns.gamma, ns.ends) == (24, 3, 0.5, 0x1000)
    assert _native.SO100ReplayNstep.gamma.offset == 8 and _native.SO100ReplayNstep.ends.offset == 16
    assert [f[0] for f in _native.SO100ReplayNstepOut._fields_] == ["size", "reserved0", "discounts", "nsteps",
                                                                     "last_slot"]
    for n, T in [(1, 2), (5, 8), (65536, 300), (0, 3)]:
        assert lib.so100_replay_nstep_storage_bytes(n, T) == n * T == R.nstep_storage_bytes(n, T)
        assert R.ReplayNstepRef(min(n, 5), min(T, 8), 1).ends.nbytes == min(n, 5) * min(T, 8)
    for bad in [(-1, 4), (4, 1), (1 << 16, 1 << 15)]:
        assert lib.so100_replay_nstep_storage_bytes(*bad) == -1
        assert b"so100_replay_nstep_storage_bytes" in lib.so100_last_error()
    # so100_replay_storage_bytes does not count the new array
    assert lib.so100_replay_storage_bytes(5, 8, 6, 0) == 5 * 8 * (4 * 37 + 1) + 4 * 16


# ---------------------------------------------------------------------- refusals
def _records(T=8, **ns_kw):
    from gym_so100 import _native
    fake = ctypes.c_void_p(0x1000)
    img = lambda k: "img" in k or "pixels" in k  # noqa: E731
    rec = _native.SO100Replay(n=4, T=T, action_dim=6, **{k: fake for k in _native.REPLAY_ARRAYS if not img(k)})
    step = _native.SO100ReplayStep(**{k: fake for k in _native.REPLAY_STEP_INPUTS if not img(k)})
    out = _native.SO100ReplayOut(**{k: fake for k in _native.REPLAY_OUTPUTS if not img(k)})
    ns = _native.SO100ReplayNstep(**{**dict(n_step=3, gamma=0.99, ends=fake), **ns_kw})
    nout = _native.SO100ReplayNstepOut(**{k: fake for k in _native.REPLAY_NSTEP_OUTPUTS})
    return rec, step, out, ns, nout, fake


def _calls(lib, env, rec, step, out, ns, nout, batch=4):
    """the three entry points on these records: name -> a call that returns the status"""
    B = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    fake = ctypes.c_void_p(0x1000)
    return {"so100_replay_push_nstep": lambda: lib.so100_replay_push_nstep(env, B(rec), B(ns), B(step), None),
            "so100_replay_stage_nstep": lambda: lib.so100_replay_stage_nstep(env, B(rec), B(ns), None, fake, None, None),
            "so100_replay_sample_nstep": lambda: lib.so100_replay_sample_nstep(env, B(rec), B(ns), batch, 0, B(out),
                                                                               B(nout), None)}


def _refused(lib, call, text):
    assert call() != 0
    msg = lib.so100_last_error().decode()
    assert text in msg, msg


def test_refusals_of_the_nstep_entry_points():
    """every pointer is a fake that is never dereferenced (or the env is NULL): each refusal comes before device work"""
    from gym_so100 import _native
    lib = _native.load()
    rec, step, out, ns, nout, fake = _records()
    # n_step: 0, 17, and more than T - 1; gamma: NaN, -0.1, 1.5 (and the infinities)
    for T, n_step in [(8, 0), (8, -1), (20, 17), (8, 8), (3, 3), (2, 2)]:
        r, _, _, bad, _, _ = _records(T=T, n_step=n_step)
        for name, call in _calls(lib, fake, r, step, out, bad, nout).items():
            _refused(lib, call, name + ": n_step outside 1..min(16, T - 1)")
    for gamma in [float("nan"), -0.1, 1.5, float("inf"), float("-inf")]:
        bad = _records(gamma=gamma)[3]
        for name, call in _calls(lib, fake, rec, step, out, bad, nout).items():
            _refused(lib, call, name + ": gamma outside [0, 1]")
    # NULL records and wrong sizes
    for name, call in _calls(lib, fake, rec, step, out, None, nout).items():
        _refused(lib, call, name + ": NULL nstep")
    bad = _records()[3]
    bad.size += 8
    for name, call in _calls(lib, fake, rec, step, out, bad, nout).items():
        _refused(lib, call, "so100_replay_nstep")
        assert name in lib.so100_last_error().decode() and "size" in lib.so100_last_error().decode()
    sample = "so100_replay_sample_nstep"
    _refused(lib, _calls(lib, fake, rec, step, out, ns, None)[sample], sample + ": NULL nout")
    bad_out = _records()[4]
    bad_out.size -= 8
    _refused(lib, _calls(lib, fake, rec, step, out, ns, bad_out)[sample], "so100_replay_nstep_out")
    # NULL ends, NULL output arrays
    bad = _records(ends=None)[3]
    for name, call in _calls(lib, fake, rec, step, out, bad, nout).items():
        _refused(lib, call, name + ": NULL ends in so100_replay_nstep")
    for k in _native.REPLAY_NSTEP_OUTPUTS:
        o = _records()[4]
        setattr(o, k, None)
        _refused(lib, _calls(lib, fake, rec, step, out, ns, o)[sample], "NULL pointer in so100_replay_nstep_out")
    # the order: so100_replay's numbers and the call's own records first ...
    r = _records(T=1)[0]
    for name, call in _calls(lib, None, r, None, None, None, None).items():
        _refused(lib, call, name + ": T < 2")
    calls = _calls(lib, None, rec, None, None, None, None, batch=-1)
    _refused(lib, calls["so100_replay_push_nstep"], "NULL step")
    _refused(lib, calls[sample], "batch < 0")
    _refused(lib, _calls(lib, None, rec, step, None, None, None)[sample], "NULL out")
    # ... then the n-step record's numbers, before the env ...
    bad = _records(n_step=0, ends=None)[3]
    for name, call in _calls(lib, None, rec, step, out, bad, None).items():
        _refused(lib, call, name + ": n_step outside")
    _refused(lib, _calls(lib, None, rec, step, out, ns, None)[sample], "NULL nout")
    # ... then the env and so100_replay's arrays, then ends, then the pointers of step / out, nout's last
    bad = _records(ends=None)[3]
    for name, call in _calls(lib, None, rec, step, out, bad, nout).items():
        _refused(lib, call, name + ": NULL env")
    r = _records()[0]
    r.reward = None
    for name, call in _calls(lib, fake, r, step, out, bad, nout).items():
        _refused(lib, call, name + ": NULL array in so100_replay")
    st, o = _records()[1], _records()[2]
    st.obs, o.obs = None, None
    calls = _calls(lib, fake, rec, st, o, bad, nout)
    _refused(lib, calls["so100_replay_push_nstep"], "NULL ends")
    _refused(lib, calls[sample], "NULL ends")
    no = _records()[4]
    no.nsteps = None
    _refused(lib, _calls(lib, fake, rec, step, o, ns, no)[sample], "NULL pointer in so100_replay_out")
    # nothing to do is no error and reaches no device
    empty = _records()[0]
    empty.n = 0
    calls = _calls(lib, fake, empty, step, out, ns, nout)
    assert calls["so100_replay_push_nstep"]() == 0 and calls["so100_replay_stage_nstep"]() == 0
    assert _calls(lib, fake, rec, step, out, ns, nout, batch=0)[sample]() == 0
    # the edges that pass: gamma 0 and 1, n_step = T - 1 and 16
    for T, n_step, gamma in [(8, 7, 0.0), (17, 16, 1.0), (2, 1, 0.5)]:
        r, _, _, good, _, _ = _records(T=T, n_step=n_step, gamma=gamma)
        assert _calls(lib, fake, r, step, out, good, nout, batch=0)[sample]() == 0, lib.so100_last_error()


# ---------------------------------------------------------------------- options
def test_options():
    from gym_so100.replay import (UNIFORM_REPLAY_DEFAULTS, UNIFORM_REPLAY_NSTEP_DEFAULTS, nstep_window,
                                  uniform_replay_options)
    assert UNIFORM_REPLAY_DEFAULTS == dict(buffer_size=None, augment=None, seed=None)
    assert UNIFORM_REPLAY_NSTEP_DEFAULTS == dict(n_step=None, gamma=0.99)
    env = dict(num_envs=8, task="so100_touch_cube")
    off = uniform_replay_options(dict(buffer_size=40), **env)
    assert off["n_step"] is None and "gamma" not in off and off["T"] == 5
    on = uniform_replay_options(dict(buffer_size=40, n_step=3), **env)
    assert (on["n_step"], on["gamma"], on["T"]) == (3, 0.99, 5)
    assert uniform_replay_options(dict(buffer_size=40, n_step=np.int64(1), gamma=1), **env)["gamma"] == 1.0
    assert uniform_replay_options(dict(buffer_size=40, n_step=4, gamma=0.0), **env)["n_step"] == 4      # T - 1
    assert uniform_replay_options(dict(buffer_size=1 << 20, n_step=16))["n_step"] == 16
    for bad in [dict(gamma=0.9), dict(n_step=None, gamma=0.9), dict(n_step=0), dict(n_step=17), dict(n_step=-1),
                dict(n_step=2.0), dict(n_step=True), dict(n_step="3"), dict(n_step=3, gamma=float("nan")),
                dict(n_step=3, gamma=-0.1), dict(n_step=3, gamma=1.5), dict(n_step=3, gamma=float("inf")),
                dict(n_step=3, gamma="0.9"), dict(n_step=3, gamma=None), dict(n_step=3, gamma=True),
                dict(n_step=3, discount=0.9)]:
        with pytest.raises(ValueError, match="uniform_replay"):
            uniform_replay_options(dict(buffer_size=40, **bad))
    with pytest.raises(ValueError, match="n_step"):
        uniform_replay_options(dict(buffer_size=40, n_step=5), **env)            # 5 slots per env hold 4 transitions
    assert nstep_window(3, 0.5, T=4) == (3, 0.5)
    with pytest.raises(ValueError):
        nstep_window(3, 0.5, T=3)


def test_constructor_raises_before_any_device_work(monkeypatch):
    from gym_so100 import SO100VecEnv, _native

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "load", no_device)
    for ur in [dict(buffer_size=64, gamma=0.9), dict(buffer_size=64, n_step=17), dict(buffer_size=64, n_step=8),
               dict(buffer_size=64, n_step=3, gamma=2.0)]:
        with pytest.raises(ValueError, match="uniform_replay"):
            SO100VecEnv(8, task="so100_touch_cube", uniform_replay=ur)


class _FakeEnv:
    """what UniformReplay.__init__ reads of an env, on the CPU"""
    num_envs, action_dim, device, base_seed, pixels, channels_first = 4, 6, "cpu", 0, None, False

    def __init__(self):
        from gym_so100 import _native
        self.lib = _native.load()


def test_a_buffer_without_n_step_has_no_ends():
    torch = pytest.importorskip("torch")
    from gym_so100.replay import UniformReplay, uniform_replay_options
    off = UniformReplay(_FakeEnv(), uniform_replay_options(dict(buffer_size=32), num_envs=4, task="so100_touch_cube"))
    assert off.n_step is None and off._nstep is None and not hasattr(off, "ends")
    assert sorted(off.store) == ["action", "meta", "next_obs", "obs", "prefix", "reward", "terminated"]
    for kw in (dict(n_step=2), dict(gamma=0.5)):
        with pytest.raises(ValueError, match="n_step"):
            off.sample(4, **kw)
    on = UniformReplay(_FakeEnv(), uniform_replay_options(dict(buffer_size=32, n_step=1), num_envs=4,
                                                          task="so100_touch_cube"))
    assert on.n_step == 1 and on.gamma == 0.99 and tuple(on.ends.shape) == (8, 4) and on.ends.dtype == torch.uint8
    assert sorted(on.store) == sorted(off.store) and on._nstep.ends == on.ends.data_ptr()
    for kw in (dict(n_step=8), dict(n_step=0), dict(gamma=1.5)):
        with pytest.raises(ValueError, match="uniform_replay"):
            on.sample(4, **kw)


# ---------------------------------------------------------------------- the restatement against brute force
Tr = collections.namedtuple("Tr", "episode reward terminated slot")


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("T", [2, 3, 8])
def test_restatement_against_a_log_of_every_transition(n, T):
    """random pushes, masked stages (also right after a finished episode and at count == 0) and drops (also at a full
    ring), a few hundred calls; a plain Python log keeps every stored transition with its episode id.  For every valid
    (env, slot) and every n_step the restatement's (R, discount, m, last_slot, done) is the log's, and no window holds
    transitions of two episodes."""
    rng = np.random.default_rng(100 * n + T)
    gamma = 0.99
    ref = R.ReplayNstepRef(n, T, 2)
    log = [collections.deque(maxlen=T - 1) for _ in range(n)]
    episode = [0] * n
    seen = collections.Counter()
    checked = 0
    for t in range(300):
        if t == 0 or rng.random() < 0.25:                # a reset: of every env at the start, of some later
            mask = None if t == 0 or rng.random() < 0.2 else rng.random(n) < 0.5
            for e in range(n) if mask is None else np.flatnonzero(mask):
                k = int(ref.meta[1, e])
                seen["stage at count 0" if k == 0 else
                     ("stage after a finished episode" if ref.ends[(int(ref.meta[0, e]) - 1) % T, e] else "stage cut")] += 1
                episode[e] += 1                          # what follows is another episode
            ref.stage(mask, R.rows(n, t, 15))
        else:
            term = rng.random(n) < 0.12
            trunc = rng.random(n) < 0.08
            div = rng.random(n) < 0.12
            trunc |= div
            rew = rng.standard_normal(n).astype(np.float32)
            cur = ref.meta[0].copy()
            full = ref.meta[1] == T - 1
            use_div = rng.random() < 0.85
            ref.push(R.rows(n, t, 15), R.rows(n, t, 15, 0.5), R.rows(n, t, 2), rew, term, trunc, div if use_div else None)
            for e in range(n):
                if use_div and div[e]:
                    seen["drop"] += 1
                    seen["drop at a full ring"] += int(full[e])
                    episode[e] += 1                      # the episode was cut: what follows is another one
                    continue
                log[e].append(Tr(episode[e], rew[e], int(term[e]), int(cur[e])))
                if term[e] or trunc[e]:
                    episode[e] += 1
        # every valid transition, every window
        for e in range(n):
            slots = ref.valid_slots(e)
            assert slots == [tr.slot for tr in log[e]]
            for kidx, s in enumerate(slots):
                for n_step in range(1, min(16, T - 1) + 1):
                    win = [log[e][kidx]]
                    while len(win) < n_step and kidx + len(win) < len(log[e]) and \
                            log[e][kidx + len(win)].episode == win[0].episode:
                        win.append(log[e][kidx + len(win)])
                    Rw, g = np.float32(win[0].reward), np.float32(gamma)
                    for tr in win[1:]:
                        Rw = np.float32(Rw + np.float32(g * np.float32(tr.reward)))
                        g = np.float32(g * np.float32(gamma))
                    m, reason = ref.window(e, s, n_step)
                    got = ref.nstep_return(e, s, m, gamma)
                    last = (s + m - 1) % T
                    assert (m, last, int(ref.terminated[last, e])) == (len(win), win[-1].slot, win[-1].terminated)
                    assert got[0].tobytes() == Rw.tobytes() and got[1].tobytes() == g.tobytes()
                    assert len({tr.episode for tr in win}) == 1
                    seen[reason] += 1
                    checked += 1
    assert checked >= 200
    want = {"stage at count 0", "stage cut", "drop", R.N_REACHED if T > 2 else R.NEWEST, R.END_FLAG, R.NEWEST}
    if T > 2:
        want |= {"stage after a finished episode", "drop at a full ring"}
    assert want <= {k for k, v in seen.items() if v}, sorted(seen.items())


def test_sample_nstep_restatement_is_the_plain_sample_at_the_start_and_for_one_step():
    ref = R.scripted(5, 8, 6, (1, 3, 5, 3), seed=99)
    plain = ref.sample(300, 2, pad=4)
    for n_step in (1, 2, 3, 7):
        got = ref.sample_nstep(300, 2, n_step, 0.99, pad=4)
        for k in ("obs", "actions", "env", "slot", "shift", "pixels"):
            assert got[k].tobytes() == plain[k].tobytes(), (n_step, k)
        if n_step == 1:
            assert all(got[k].tobytes() == plain[k].tobytes() for k in plain)
            assert (got["nsteps"] == 1).all() and (got["last_slot"] == got["slot"]).all()
            assert (got["discounts"] == np.float32(0.99)).all()
        else:
            assert (got["rewards"] != plain["rewards"]).any() and (got["next_obs"] != plain["next_obs"]).any()
            assert (got["next_pixels"] != plain["next_pixels"]).any()
        assert ((got["last_slot"] - got["slot"]) % 8 == got["nsteps"] - 1).all()
    empty = R.ReplayNstepRef(3, 8, 6).sample_nstep(5, 0, 3, 0.99)
    assert (empty["nsteps"] == 0).all() and (empty["discounts"] == 0).all() and (empty["last_slot"] == -1).all()


# ---------------------------------------------------------------------- what the GPU tests' scripted episodes cover
@pytest.mark.parametrize("n_step,T,B", [(1, 8, 256), (2, 8, 256), (3, 8, 256), (1, 8, 1000), (2, 8, 1000), (3, 8, 1000),
                                        (16, 20, 1000)])
def test_the_scripted_episodes_cover_every_window(n_step, T, B):
    """the batches of tests/test_gpu_replay_nstep.py (seed 99, call 2) hold every window length 1..n_step, the three
    stop reasons and, among the end_flag rows, one closed by a done, one by a stage and one by a drop: by the
    restatement alone.  (A batch of 1 or 5 rows cannot hold 16 window lengths, and 256 draws over the 76 transitions of
    T = 20 miss one: the GPU test asserts the condition on these batches and compares the smaller ones all the same.)"""
    ref = R.scripted(5, T, 6, None, seed=99)
    out = ref.sample_nstep(B, 2, n_step, 0.99)
    lengths, reasons, why = R.coverage(out, n_step)
    assert lengths == set(range(1, n_step + 1)), lengths
    if n_step == 1:                                      # (a window of one transition stops at n_step at the latest)
        assert R.END_FLAG in reasons and why == {R.WHY_DONE, R.WHY_STAGE, R.WHY_DROP}
    else:
        assert R.covers_everything(out, n_step), (lengths, reasons, why)
    assert int(ref.meta[1][4]) == 0 and (out["env"] != 4).all()


def test_the_rewards_make_the_order_visible():
    """reward = 1 + 2^-20 j, gamma = 0.99: summing from the far end, or fusing the multiply into the add, changes bits of
    some window's return, so a kernel that did either would not match bit for bit"""
    ref = R.scripted(5, 20, 6, None, seed=99)
    f32, g = np.float32, np.float32(0.99)
    differs = collections.Counter()
    for e in range(5):
        for s in ref.valid_slots(e):
            m, _ = ref.window(e, s, 16)
            rw = [f32(ref.reward[(s + j) % 20, e]) for j in range(m)]
            want = ref.nstep_return(e, s, m, 0.99)[0]
            fused, gg = rw[0], g
            for r in rw[1:]:
                fused = f32(np.float64(fused) + np.float64(gg) * np.float64(r))      # one rounding
                gg = f32(gg * g)
            back = f32(0)
            for j in reversed(range(m)):                 # Horner from the far end
                back = f32(rw[j] + f32(g * back))
            differs["fused"] += fused.tobytes() != want.tobytes()
            differs["reordered"] += back.tobytes() != want.tobytes()
    assert differs["fused"] > 0 and differs["reordered"] > 0, differs
