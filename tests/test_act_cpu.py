"""CPU checks of the device-side physical randomisation and the actuation-latency model (include/so100.h so100_dr_sample,
so100_actuate): the struct mirror, the argument-level refusals of both entry points (each before any
device work, so they answer without a device; the refusal of a model with ee = 1 needs an env and is in
tests/test_gpu_act.py), the ValueErrors of SO100VecEnv(domain_randomization=dict(per_episode=, actuation=)), the
properties of the numpy restatement (tests/act_ref.py), the delay draw's coverage and the restatement's float32 floor,
which sets the bar of tests/test_gpu_act.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import act_ref
import ee_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- struct and arguments
def test_struct_mirror_matches_library_and_header():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25        # additions only: the version stays
    assert lib.so100_dr_ranges_bytes() == ctypes.sizeof(_native.SO100DrRanges) == 56
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    body = re.search(r"typedef struct so100_dr_ranges \{(.*?)\} so100_dr_ranges;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _native.SO100DrRanges._fields_]
    assert re.search(r"#define SO100_ACT_MAX_DELAY 7\b", src) and re.search(r"#define SO100_ACT_HIST 8\b", src)
    assert (_native.SO100_ACT_MAX_DELAY, _native.SO100_ACT_HIST) == (act_ref.MAX_DELAY, act_ref.HIST) == (7, 8)
    r = _native.SO100DrRanges()                          # the default record: everything off
    assert r.size == 56 and list(r.mass) == [1.0, 1.0] and list(r.friction) == [1.0, 1.0]
    assert {"delay": tuple(r.delay), "smoothing": tuple(r.smoothing), "rate": tuple(r.rate)} == act_ref.OFF
    for fn in ("so100_dr_ranges_bytes", "so100_dr_sample", "so100_actuate"):
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn)


def _sample(lib, ranges, env=None, outs=(1, 1)):
    """so100_dr_sample with fake non-NULL outputs: every check below returns before either is written"""
    dr, act = (ctypes.c_void_p(p) if p else None for p in outs)
    rc = lib.so100_dr_sample(env, None if ranges is None else ctypes.byref(ranges), None, None, None, dr, act, None)
    return rc, lib.so100_last_error().decode()


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (dict(mass=(0.0, 1.0)), "mass range must be finite with 0 < lo <= hi"), (dict(mass=(1.2, 0.8)), "mass range"),
    (dict(mass=(NAN, 1.0)), "mass range"), (dict(mass=(0.5, INF)), "mass range"), (dict(mass=(-1.0, 1.0)), "mass range"),
    (dict(friction=(0.0, 1.0)), "friction range must be finite with 0 < lo <= hi"),
    (dict(friction=(1.2, 0.8)), "friction range"), (dict(friction=(0.5, NAN)), "friction range"),
    (dict(delay=(-1, 2)), "delay range must lie in 0..7 with lo <= hi"), (dict(delay=(0, 8)), "delay range"),
    (dict(delay=(3, 2)), "delay range"),
    (dict(smoothing=(0.0, 1.0)), "smoothing range must lie in (0, 1] with lo <= hi"),
    (dict(smoothing=(0.5, 1.5)), "smoothing range"), (dict(smoothing=(0.9, 0.3)), "smoothing range"),
    (dict(smoothing=(NAN, 1.0)), "smoothing range"),
    (dict(rate=(0.0, 1.0)), "rate range must be finite with 0 < lo <= hi"), (dict(rate=(2.0, 1.0)), "rate range"),
    (dict(rate=(1.0, INF)), "rate range"), (dict(rate=(NAN, NAN)), "rate range"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in REFUSALS])
def test_dr_sample_range_refusals(kw, text):
    """a fake non-NULL env: the range checks answer before the env is looked into"""
    from gym_so100 import _native
    lib = _native.load()
    for outs in ((1, 1), (1, 0), (0, 1)):                # the ranges are checked whichever output is asked for
        rc, err = _sample(lib, _native.SO100DrRanges(**kw), env=ctypes.c_void_p(1), outs=outs)
        assert rc == -1 and "so100_dr_sample" in err and text in err, err


def test_dr_sample_null_and_size_refusals():
    from gym_so100 import _native
    lib = _native.load()
    rc, err = _sample(lib, None)
    assert rc == -1 and "so100_dr_sample: NULL ranges" in err
    r = _native.SO100DrRanges()
    r.size = 48
    r.delay[1] = 99                                      # the size is checked first
    rc, err = _sample(lib, r)
    assert rc == -1 and "so100_dr_ranges.size 48, expected 56" in err
    rc, err = _sample(lib, _native.SO100DrRanges())      # a good record: the NULL env is what is left to refuse
    assert rc == -1 and "so100_dr_sample: NULL env" in err
    rc, err = _sample(lib, _native.SO100DrRanges(), env=ctypes.c_void_p(1), outs=(0, 0))
    assert rc == -1 and "NULL dr_params and act_params" in err
    # the edges of the ranges are inside: what is left to refuse is the NULL env
    edge = _native.SO100DrRanges(delay=(0, 7), smoothing=(1e-3, 1.0), rate=(1e-3, 1e3), mass=(0.1, 0.1))
    assert "NULL env" in _sample(lib, edge)[1]


def test_actuate_refusals():
    from gym_so100 import _native
    lib = _native.load()
    one = ctypes.c_void_p(1)
    assert lib.so100_actuate(None, one, one, None, one, one, one, one, None) == -1
    assert "so100_actuate: NULL env" in lib.so100_last_error().decode()
    for k in range(6):                                   # qpos, command, act_params, hist, head, action (reinit may be NULL)
        args = [one] * 6
        args[k] = None
        q, c, p, h, hd, a = args
        assert lib.so100_actuate(one, q, c, None, p, h, hd, a, None) == -1
        assert "so100_actuate: NULL qpos, command, act_params, hist, head or action" in lib.so100_last_error().decode()


def test_vec_env_value_errors_need_no_device(monkeypatch):
    """every ValueError is raised before the library is loaded or a device touched"""
    from gym_so100 import SO100VecEnv, _native
    from gym_so100.sb3 import SO100SB3VecEnv

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_load)
    bad = [dict(actuation={"lag": (0, 1)}), dict(actuation=[1]), dict(actuation={"delay": (0, 8)}),
           dict(actuation={"delay": (-1, 2)}), dict(actuation={"delay": (3, 2)}), dict(actuation={"delay": (0.5, 2)}),
           dict(actuation={"delay": 3}), dict(actuation={"smoothing": (0.0, 1.0)}),
           dict(actuation={"smoothing": (0.5, 1.5)}), dict(actuation={"smoothing": (0.9, 0.3)}),
           dict(actuation={"smoothing": (NAN, 1.0)}), dict(actuation={"rate": (0.0, 1.0)}),
           dict(actuation={"rate": (2.0, 1.0)}), dict(actuation={"rate": (1.0, INF)}), dict(actuation={"rate": "x"}),
           dict(per_episode=True, mass=(0.0, 1.0)), dict(per_episode=True, mass=(1.2, 0.8)),
           dict(per_episode=True, friction=(NAN, 1.0)), dict(per_episode=True, friction=(0.5, INF))]
    for dr in bad:
        with pytest.raises(ValueError):
            SO100VecEnv(4, domain_randomization=dr)
        with pytest.raises(ValueError):
            SO100SB3VecEnv(4, domain_randomization=dr)
    with pytest.raises(ValueError, match="variant='ee'"):
        SO100VecEnv(4, variant="ee", domain_randomization=dict(actuation={}))
    # what is accepted goes on to load the library
    for dr in (dict(actuation={}), dict(per_episode=True), dict(actuation={"delay": (0, 7), "smoothing": (0.3, 1.0)})):
        with pytest.raises(AssertionError, match="the library was loaded"):
            SO100VecEnv(4, domain_randomization=dr)


def test_actuation_options_defaults():
    from gym_so100.vec_env import ACTUATION_OFF, ACT_MAX_DELAY, actuation_options
    assert ACTUATION_OFF == act_ref.OFF and ACT_MAX_DELAY == act_ref.MAX_DELAY
    assert actuation_options({}) == act_ref.OFF
    assert actuation_options({"delay": (np.int64(1), 3)}) == dict(act_ref.OFF, delay=(1, 3))


# ---------------------------------------------------------------------- the restatement's properties
def _inputs(model, oracle64, n=16, calls=24, seed=3):
    rng = np.random.default_rng(seed)
    qpos = ee_ref.rollout_states(oracle64, model, 257)[:n]
    return qpos, rng.uniform(-1.2, 1.2, size=(calls, n, 6)).astype(np.float32)


def _params(n, d=0, alpha=1.0, r=2.0):
    return np.tile(np.array([d, alpha, r, 0.0], np.float32), (n, 1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_off_is_the_identity(model, oracle64, dtype):
    """d = 0, alpha = 1, r >= 2: the applied action is clip(command) bit for bit, from the first call on"""
    qpos, cmd = _inputs(model, oracle64)
    a = act_ref.Actuator(model, len(qpos), dtype)
    for t, c in enumerate(cmd):
        y = a(qpos, c, _params(len(qpos), r=2.0 if t % 2 else 5.0), reinit=np.full(len(qpos), t in (0, 7)))
        assert y.dtype == dtype and np.array_equal(y, np.clip(c, -1, 1).astype(dtype))
        assert not a.from_hold.any()


@pytest.mark.parametrize("d", [1, 3, 7])
def test_pure_delay(model, oracle64, d):
    """a delay d returns hold for d calls and then the command of d calls earlier, bit for bit"""
    qpos, cmd = _inputs(model, oracle64)
    a = act_ref.Actuator(model, len(qpos), np.float32)
    hold = a.hold(qpos)
    assert np.abs(hold).max() <= 1 and np.abs(hold).min() < 1
    for t, c in enumerate(cmd):
        y = a(qpos, c, _params(len(qpos), d=d), reinit=np.full(len(qpos), t == 0))
        want = hold if t < d else np.clip(cmd[t - d], -1, 1)
        assert np.array_equal(y, want), t
        assert a.from_hold.all() if t < d else not a.from_hold.any()
    assert (a.head == len(cmd)).all()


def test_reinit_mid_run_restarts_the_delay(model, oracle64):
    qpos, cmd = _inputs(model, oracle64)
    n = len(qpos)
    a = act_ref.Actuator(model, n, np.float32)
    re = np.arange(n) % 2 == 0
    for t, c in enumerate(cmd[:12]):
        y = a(qpos, c, _params(n, d=2), reinit=np.ones(n) if t == 0 else (re if t == 6 else None))
    # call 11 is 5 calls after the re-initialisation at 6: every env is back on the command of two calls earlier
    assert np.array_equal(y, np.clip(cmd[9], -1, 1))
    assert (a.head[re] == 6).all() and (a.head[~re] == 12).all()


def test_rate_limit_bounds_the_step(model, oracle64):
    qpos, cmd = _inputs(model, oracle64)
    n = len(qpos)
    a = act_ref.Actuator(model, n, np.float64)
    r = np.float32(0.07)
    prev, moved = a.hold(qpos), 0
    for t, c in enumerate(cmd):
        y = a(qpos, c, _params(n, d=1, alpha=0.8, r=r), reinit=np.full(n, t == 0))
        step = np.abs(y - prev)
        assert step.max() <= float(r) * (1 + 1e-12)
        moved += int((step >= float(r) * (1 - 1e-12)).sum())
        prev = y
    assert moved > 0                                     # the limit was met, not merely never reached


def test_smoothing_converges_to_a_constant_command(model, oracle64):
    qpos, cmd = _inputs(model, oracle64)
    n = len(qpos)
    a = act_ref.Actuator(model, n, np.float64)
    target = np.clip(cmd[0], -1, 1).astype(np.float64)
    err0 = np.abs(a.hold(qpos) - target).max()
    for t in range(40):
        y = a(qpos, cmd[0], _params(n, alpha=0.5), reinit=np.full(n, t == 0))
        # y_t - target = (1 - alpha)^(t + 1) (hold - target)
        assert np.abs(y - target).max() <= err0 * 0.5 ** (t + 1) * (1 + 1e-9) + 1e-15
    assert np.abs(y - target).max() <= 1e-11


# ---------------------------------------------------------------------- the draws
@pytest.mark.parametrize("rng", [(0, 0), (0, 3), (2, 7)])
def test_delay_draws_cover_their_range(rng):
    ids = np.arange(4096)
    seen = set()
    for ep in (0, 1):
        d = act_ref.draw_delay(11, ids, np.full(4096, ep), rng)
        assert d.min() >= rng[0] and d.max() <= rng[1]
        seen |= set(d.tolist())
        if ep == 0:
            assert set(d.tolist()) == set(range(rng[0], rng[1] + 1))     # 4,096 draws take every value
    first = act_ref.draw_delay(11, ids, np.zeros(4096), (0, 7))
    assert not np.array_equal(first, act_ref.draw_delay(11, ids, np.ones(4096), (0, 7)))      # the episode matters
    assert not np.array_equal(first, act_ref.draw_delay(12, ids, np.zeros(4096), (0, 7)))     # and the seed


def test_real_draws_stay_inside_and_zero_width_is_exact():
    ids = np.arange(4096)
    for dt in (np.float32, np.float64):
        dr, act = act_ref.sample(3, ids, ids % 5, mass=(0.8, 1.2), friction=(0.5, 0.5), smoothing=(0.3, 1.0),
                                 rate=(0.05, 2.0), dtype=dt)
        assert dr.dtype == dt and act.dtype == dt
        assert dr[:, 0].min() >= dt(np.float32(0.8)) and dr[:, 0].max() <= dt(np.float32(1.2))
        assert (dr[:, 1] == dt(0.5)).all()
        assert act[:, 1].min() >= dt(np.float32(0.3)) and act[:, 1].max() <= 1 and (act[:, 3] == 0).all()
        assert (act[:, 0] == 0).all()
    # the draws are the visual part's hash with the physical fields: independent of each other
    assert abs(np.corrcoef(dr[:, 0], act[:, 1])[0, 1]) < 0.05


# ---------------------------------------------------------------------- float32 floor
def test_float32_floor(model, oracle64):
    """F = max |float32 restatement - float64 restatement| of the applied action over the GPU test's inputs (257 envs,
    20 calls); the constant act_ref.F_ACT that sets the GPU bar is no smaller than what is measured here"""
    q, cmd, re, par = act_ref.gpu_cases(ee_ref.rollout_states(oracle64, model, 257))
    a32, a64 = act_ref.Actuator(model, 257, np.float32), act_ref.Actuator(model, 257, np.float64)
    f = 0.0
    for t in range(act_ref.CALLS):
        y32, y64 = a32(q[t], cmd[t], par, re[t]), a64(q[t], cmd[t], par, re[t])
        assert y32.dtype == np.float32 and y64.dtype == np.float64
        f = max(f, np.abs(y64 - y32.astype(np.float64)).max())
    print(f"float32 floor of the applied action: {f:.3e}; recorded {act_ref.F_ACT:.3e}")
    assert f <= act_ref.F_ACT
    assert f > 0                                         # the two precisions do differ: the floor measures something
    assert set(par[:, 0].astype(int).tolist()) == set(range(8))      # every delay is among the cases
    assert ((par[:, 1] == 1) & (par[:, 2] >= 2)).sum() >= 64 and (par[:, 1] < 1).sum() >= 64
