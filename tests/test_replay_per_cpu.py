"""CPU checks of prioritised replay in the uniform replay buffer (include/so100.h so100_replay_push_per /
so100_replay_per_scan / so100_replay_sample_per / so100_replay_per_update): the new symbols and struct
mirrors under the unchanged ABI 25, the storage formula, every refusal of the four entry points with its text and the order
(none needs a device), the option parsing, and the restatement (tests/replay_per_ref.py) against a brute-force model, a
plain list of live transitions per env, before the GPU is involved."""
import collections
import ctypes
import math
import os
import re

import numpy as np
import pytest

import replay_per_ref as R
import replay_ref
from her_ref import draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_SYMBOLS = ("so100_replay_per_bytes", "so100_replay_per_out_bytes", "so100_replay_per_storage_bytes",
               "so100_replay_push_per", "so100_replay_per_scan", "so100_replay_sample_per", "so100_replay_per_update")


# ---------------------------------------------------------------------- ABI
def test_symbols_and_abi():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25
    header = open(os.path.join(ROOT, "include", "so100.h")).read()
    assert re.search(r"#define SO100_ABI_VERSION 25\b", header)
    assert re.search(r"#define SO100_REPLAY_PRIO_ONE 65536u\b", header)
    assert _native.SO100_REPLAY_PRIO_ONE == R.PRIO_ONE == 65536
    for fn in PER_SYMBOLS:
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn), fn
        assert re.search(r"\b%s\(" % fn, header), fn


def test_struct_mirrors_and_storage():
    from gym_so100 import _native
    lib = _native.load()
    assert lib.so100_replay_per_bytes() == ctypes.sizeof(_native.SO100ReplayPer) == 24 + 3 * 8
    assert lib.so100_replay_per_out_bytes() == ctypes.sizeof(_native.SO100ReplayPerOut) == 8 + 2 * 8
    assert lib.so100_replay_bytes() == ctypes.sizeof(_native.SO100Replay) == 120                   # unchanged
    assert lib.so100_replay_nstep_bytes() == 24 and lib.so100_replay_out_bytes() == 8 + 10 * 8     # unchanged
    p = _native.SO100ReplayPer(alpha=0.5, beta=0.25, eps=0.125, prio=ctypes.c_void_p(0x1000),
                               sum=ctypes.c_void_p(0x2000), max_prio=ctypes.c_void_p(0x3000))
    assert (p.size, p.alpha, p.beta, p.eps, p.prio, p.sum, p.max_prio) == (48, 0.5, 0.25, 0.125, 0x1000, 0x2000, 0x3000)
    assert [f[0] for f in _native.SO100ReplayPer._fields_] == ["size", "alpha", "beta", "eps", "reserved", "prio", "sum",
                                                               "max_prio"]
    assert _native.SO100ReplayPer.prio.offset == 24
    assert [f[0] for f in _native.SO100ReplayPerOut._fields_] == ["size", "reserved0", "probs", "weights"]
    with pytest.raises(TypeError):
        _native.SO100ReplayPer(ends=None)
    for n, T in [(1, 2), (5, 8), (8192, 32), (65536, 300), (0, 3), (1 << 16, (1 << 15) - 1)]:
        want = 4 * T * n + 8 * (n + 1) + 8
        assert lib.so100_replay_per_storage_bytes(n, T) == want == R.per_storage_bytes(n, T)
    assert lib.so100_replay_per_storage_bytes(1 << 16, (1 << 15) - 1) > 1 << 33    # (64-bit arithmetic)
    for bad in [(-1, 4), (4, 1), (1 << 16, 1 << 15)]:
        assert lib.so100_replay_per_storage_bytes(*bad) == -1
        assert b"so100_replay_per_storage_bytes" in lib.so100_last_error()
    # the other two formulas do not count the new arrays
    assert lib.so100_replay_storage_bytes(5, 8, 6, 0) == 5 * 8 * (4 * 37 + 1) + 4 * 16
    assert lib.so100_replay_nstep_storage_bytes(5, 8) == 40


# ---------------------------------------------------------------------- refusals
def _records(T=8, per_kw=None, ns_kw=None):
    from gym_so100 import _native
    fake = ctypes.c_void_p(0x1000)
    img = lambda k: "img" in k or "pixels" in k  # noqa: E731
    rec = _native.SO100Replay(n=4, T=T, action_dim=6, **{k: fake for k in _native.REPLAY_ARRAYS if not img(k)})
    step = _native.SO100ReplayStep(**{k: fake for k in _native.REPLAY_STEP_INPUTS if not img(k)})
    out = _native.SO100ReplayOut(**{k: fake for k in _native.REPLAY_OUTPUTS if not img(k)})
    ns = _native.SO100ReplayNstep(**{**dict(n_step=3, gamma=0.99, ends=fake), **(ns_kw or {})})
    nout = _native.SO100ReplayNstepOut(**{k: fake for k in _native.REPLAY_NSTEP_OUTPUTS})
    per = _native.SO100ReplayPer(**{**dict(alpha=0.6, beta=0.4, eps=1e-6, prio=fake, sum=fake, max_prio=fake),
                                    **(per_kw or {})})
    pout = _native.SO100ReplayPerOut(probs=fake, weights=fake)
    return dict(rec=rec, step=step, out=out, ns=ns, nout=nout, per=per, pout=pout)


FAKE = ctypes.c_void_p(0x1000)
PUSH, SCAN, SAMPLE, UPDATE = PER_SYMBOLS[3:]


def _calls(lib, env, r, batch=4, idx=(FAKE, FAKE, FAKE)):
    """the four entry points on the records r: name -> a call that returns the status"""
    B = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return {PUSH: lambda: lib.so100_replay_push_per(env, B(r["rec"]), B(r["per"]), B(r["ns"]), B(r["step"]), None),
            SCAN: lambda: lib.so100_replay_per_scan(env, B(r["rec"]), B(r["per"]), None),
            SAMPLE: lambda: lib.so100_replay_sample_per(env, B(r["rec"]), B(r["per"]), B(r["ns"]), batch, 0, B(r["out"]),
                                                        B(r["nout"]), B(r["pout"]), None),
            UPDATE: lambda: lib.so100_replay_per_update(env, B(r["rec"]), B(r["per"]), batch, *idx, None)}


def _refused(lib, call, text):
    assert call() != 0
    msg = lib.so100_last_error().decode()
    assert text in msg, msg


def _all_refuse(lib, env, r, text, names=PER_SYMBOLS[3:], **kw):
    for name in names:
        _refused(lib, _calls(lib, env, r, **kw)[name], name + ": " + text)


def test_refusals_of_the_per_entry_points():
    """every pointer is a fake that is never dereferenced (or the env is NULL): each refusal comes before device work"""
    from gym_so100 import _native
    lib = _native.load()
    nan, inf = float("nan"), float("inf")
    # 1. so100_replay's numbers come first, whatever else is wrong
    bad = _records(T=1, per_kw=dict(alpha=2.0))
    bad.update(step=None, out=None, pout=None)
    _all_refuse(lib, None, bad, "T < 2", batch=-1)
    bad = _records()
    bad["rec"] = None
    _all_refuse(lib, None, bad, "NULL replay")
    # 2. NULL per, its size
    bad = _records()
    bad["per"] = None
    _all_refuse(lib, None, bad, "NULL per")
    bad = _records()
    bad["per"].size += 8
    for name in PER_SYMBOLS[3:]:
        _refused(lib, _calls(lib, None, bad)[name], "so100_replay_per")
        assert name in lib.so100_last_error().decode() and "size" in lib.so100_last_error().decode()
    # 3. alpha, beta; 4. eps: checked by all four
    for v in [nan, -0.1, 1.5, inf, -inf]:
        _all_refuse(lib, None, _records(per_kw=dict(alpha=v, beta=v, eps=0.0)), "alpha outside [0, 1]")
        _all_refuse(lib, None, _records(per_kw=dict(beta=v, eps=0.0)), "beta outside [0, 1]")
    for v in [nan, 0.0, -1e-6, inf, -inf]:
        _all_refuse(lib, None, _records(per_kw=dict(eps=v), ns_kw=dict(n_step=0)), "eps not finite or <= 0")
    # 5. the n-step record where it is given (push, sample), before the call's own records
    bad = _records(ns_kw=dict(n_step=0))
    bad.update(step=None, out=None, nout=None, pout=None)
    _all_refuse(lib, None, bad, "n_step outside 1..min(16, T - 1)", names=(PUSH, SAMPLE))
    bad = _records(ns_kw=dict(gamma=1.5))
    _all_refuse(lib, None, bad, "gamma outside [0, 1]", names=(PUSH, SAMPLE))
    bad = _records()
    bad["ns"].size -= 8
    for name in (PUSH, SAMPLE):
        _refused(lib, _calls(lib, None, bad)[name], "so100_replay_nstep")
    # 6. nout and nstep go together; 7. pout; 8. the call's records and batch
    bad = _records()
    bad.update(ns=None, pout=None)
    _refused(lib, _calls(lib, None, bad)[SAMPLE], SAMPLE + ": nout without nstep")
    bad = _records()
    bad.update(nout=None, pout=None)
    _refused(lib, _calls(lib, None, bad)[SAMPLE], SAMPLE + ": NULL nout with nstep")
    bad = _records()
    bad["nout"].size += 8
    bad["pout"] = None
    _refused(lib, _calls(lib, None, bad)[SAMPLE], "so100_replay_nstep_out")
    bad = _records()
    bad.update(pout=None, out=None)
    _refused(lib, _calls(lib, None, bad, batch=-1)[SAMPLE], SAMPLE + ": NULL pout")
    bad = _records()
    bad["pout"].size += 8
    bad["out"] = None
    _refused(lib, _calls(lib, None, bad, batch=-1)[SAMPLE], "so100_replay_per_out")
    bad = _records()
    bad["out"] = None
    _refused(lib, _calls(lib, None, bad, batch=-1)[SAMPLE], SAMPLE + ": NULL out")
    bad = _records()
    bad["out"].size += 8
    _refused(lib, _calls(lib, None, bad, batch=-1)[SAMPLE], "so100_replay_out")
    bad = _records()
    bad["step"] = None
    _refused(lib, _calls(lib, None, bad)[PUSH], PUSH + ": NULL step")
    bad = _records()
    bad["step"].size += 8
    _refused(lib, _calls(lib, None, bad)[PUSH], "so100_replay_step")
    _all_refuse(lib, None, _records(), "batch < 0", names=(SAMPLE, UPDATE), batch=-1)
    # 9. the env, so100_replay's arrays, ends, the priorities' arrays, then the call's pointers
    bad = _records(ns_kw=dict(ends=None), per_kw=dict(prio=None))
    bad["rec"].reward = None
    _all_refuse(lib, None, bad, "NULL env")
    _all_refuse(lib, FAKE, bad, "NULL array in so100_replay")
    bad = _records(ns_kw=dict(ends=None), per_kw=dict(prio=None))
    _all_refuse(lib, FAKE, bad, "NULL ends in so100_replay_nstep", names=(PUSH, SAMPLE))
    for k in _native.REPLAY_PER_ARRAYS:
        bad = _records(per_kw={k: None})
        bad["step"].obs = bad["out"].obs = None
        _all_refuse(lib, FAKE, bad, "NULL array in so100_replay_per", idx=(None, None, None))
    bad = _records()
    bad["step"].obs = bad["out"].obs = None
    bad["nout"].nsteps = bad["pout"].probs = None
    _refused(lib, _calls(lib, FAKE, bad)[PUSH], PUSH + ": NULL pointer in so100_replay_step")
    _refused(lib, _calls(lib, FAKE, bad)[SAMPLE], SAMPLE + ": NULL pointer in so100_replay_out")
    bad = _records()
    bad["nout"].nsteps = bad["pout"].probs = None
    _refused(lib, _calls(lib, FAKE, bad)[SAMPLE], SAMPLE + ": NULL pointer in so100_replay_nstep_out")
    for k in _native.REPLAY_PER_OUTPUTS:
        bad = _records()
        setattr(bad["pout"], k, None)
        _refused(lib, _calls(lib, FAKE, bad)[SAMPLE], SAMPLE + ": NULL pointer in so100_replay_per_out")
    for j in range(3):
        idx = [FAKE] * 3
        idx[j] = None
        _refused(lib, _calls(lib, FAKE, _records(), idx=tuple(idx))[UPDATE], UPDATE + ": NULL env_idx, slot_idx or td_abs")
    # nothing to do is no error and reaches no device; the n-step record may be absent
    empty = _records()
    empty["rec"].n = 0
    calls = _calls(lib, FAKE, empty)
    assert calls[PUSH]() == 0 and calls[UPDATE]() == 0, lib.so100_last_error()
    calls = _calls(lib, FAKE, _records(), batch=0)
    assert calls[SAMPLE]() == 0 and calls[UPDATE]() == 0, lib.so100_last_error()
    plain = _records()
    plain.update(ns=None, nout=None)
    assert _calls(lib, FAKE, plain, batch=0)[SAMPLE]() == 0, lib.so100_last_error()
    # the edges that pass: alpha and beta 0 and 1, a tiny eps
    for a, b, eps in [(0.0, 1.0, 1e-30), (1.0, 0.0, 3e38)]:
        good = _records(per_kw=dict(alpha=a, beta=b, eps=eps))
        assert _calls(lib, FAKE, good, batch=0)[SAMPLE]() == 0, lib.so100_last_error()


# ---------------------------------------------------------------------- options
def test_options():
    from gym_so100.replay import (PER_DEFAULTS, UNIFORM_REPLAY_DEFAULTS, UNIFORM_REPLAY_NSTEP_DEFAULTS,
                                  UNIFORM_REPLAY_PER_DEFAULTS, per_options, uniform_replay_options)
    assert UNIFORM_REPLAY_PER_DEFAULTS == dict(prioritized=None)
    assert PER_DEFAULTS == dict(alpha=0.6, beta=0.4, eps=1e-6)
    assert UNIFORM_REPLAY_DEFAULTS == dict(buffer_size=None, augment=None, seed=None)
    assert UNIFORM_REPLAY_NSTEP_DEFAULTS == dict(n_step=None, gamma=0.99)
    env = dict(num_envs=8, task="so100_touch_cube")
    assert uniform_replay_options(dict(buffer_size=40), **env)["prioritized"] is None
    for off in (None, False):
        assert uniform_replay_options(dict(buffer_size=40, prioritized=off), **env)["prioritized"] is None
    on = uniform_replay_options(dict(buffer_size=40, prioritized=True), **env)
    assert on["prioritized"] == PER_DEFAULTS and on["prioritized"] is not PER_DEFAULTS and on["n_step"] is None
    own = dict(alpha=1, beta=0, eps=np.float32(0.5))
    both = uniform_replay_options(dict(buffer_size=40, prioritized=own, n_step=3), **env)
    assert both["prioritized"] == dict(alpha=1.0, beta=0.0, eps=0.5) and both["n_step"] == 3
    assert all(type(v) is float for v in both["prioritized"].values())
    assert per_options(None) is None and per_options(True) == PER_DEFAULTS
    nan, inf = float("nan"), float("inf")
    # each refusal by its own text (a tree without the key refuses all of these alike, as an unknown key)
    keys, unit, number = "exactly the keys", r"must be finite and in \[0, 1\]", "must be a number"
    for bad, text in [(1, keys), (0.6, keys), ("yes", keys), ([0.6, 0.4], keys), (dict(), keys), (dict(alpha=0.6), keys),
                      (dict(alpha=0.6, beta=0.4), keys), (dict(alpha=0.6, beta=0.4, eps=1e-6, gamma=1), keys),
                      (dict(alpha=nan, beta=0.4, eps=1e-6), "alpha nan " + unit),
                      (dict(alpha=-0.1, beta=0.4, eps=1e-6), "alpha -0.1 " + unit),
                      (dict(alpha=1.5, beta=0.4, eps=1e-6), "alpha 1.5 " + unit),
                      (dict(alpha=0.6, beta=inf, eps=1e-6), "beta inf " + unit),
                      (dict(alpha=0.6, beta=2, eps=1e-6), "beta 2.0 " + unit),
                      (dict(alpha=0.6, beta="0.4", eps=1e-6), "beta '0.4' " + number),
                      (dict(alpha=True, beta=0.4, eps=1e-6), "alpha True " + number),
                      (dict(alpha=0.6, beta=0.4, eps=None), "eps None " + number)] + \
            [(dict(alpha=0.6, beta=0.4, eps=e), "eps .* must be finite and > 0") for e in (0, -1e-6, nan, inf, 1e-60)]:
        with pytest.raises(ValueError, match="uniform_replay: (prioritized .*)?" + text):
            uniform_replay_options(dict(buffer_size=40, prioritized=bad))
    with pytest.raises(ValueError, match="unknown keys"):
        uniform_replay_options(dict(buffer_size=40, prioritised=True))


def test_constructor_raises_before_any_device_work(monkeypatch):
    from gym_so100 import SO100VecEnv, _native

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "load", no_device)
    # (by the texts of per_options: a tree without the key refuses `prioritized` itself, as an unknown key)
    for p, text in [(dict(alpha=0.6), "exactly the keys"), (dict(alpha=2, beta=0.4, eps=1e-6), r"alpha 2.0 must be finite"),
                    (0.6, "exactly the keys"), (dict(alpha=0.6, beta=0.4, eps=0), "eps 0 must be finite and > 0")]:
        with pytest.raises(ValueError, match="uniform_replay: (prioritized .*)?" + text):
            SO100VecEnv(8, task="so100_touch_cube", uniform_replay=dict(buffer_size=64, prioritized=p))


class _FakeEnv:
    """what UniformReplay.__init__ reads of an env, on the CPU"""
    num_envs, action_dim, device, base_seed, pixels, channels_first = 4, 6, "cpu", 0, None, False

    def __init__(self):
        from gym_so100 import _native
        self.lib = _native.load()


def test_a_buffer_without_prioritized_has_none_of_it():
    torch = pytest.importorskip("torch")
    from gym_so100.replay import UniformReplay, uniform_replay_options
    env = dict(num_envs=4, task="so100_touch_cube")
    off = UniformReplay(_FakeEnv(), uniform_replay_options(dict(buffer_size=32), **env))
    assert off.prioritized is None and off._per is None
    for name in ("prio", "prio_sum", "max_prio", "alpha", "beta", "eps"):
        assert not hasattr(off, name), name
    assert sorted(off.store) == ["action", "meta", "next_obs", "obs", "prefix", "reward", "terminated"]
    with pytest.raises(ValueError, match="prioritized"):
        off.sample(4, beta=0.5)
    with pytest.raises(ValueError, match="prioritized"):
        off.update_priorities(torch.zeros(1), torch.zeros(1), torch.zeros(1))
    on = UniformReplay(_FakeEnv(), uniform_replay_options(dict(buffer_size=32, prioritized=True, n_step=2), **env))
    assert sorted(on.store) == sorted(off.store) and not hasattr(off, "ends") and tuple(on.ends.shape) == (8, 4)
    assert tuple(on.prio.shape) == (8, 4) and on.prio.element_size() == 4 and not on.prio.any()
    assert tuple(on.prio_sum.shape) == (5,) and on.prio_sum.element_size() == 8
    assert on.max_prio.tolist() == [65536, 0]
    assert (on.alpha, on.beta, on.eps) == (0.6, 0.4, 1e-6)
    assert (on._per.prio, on._per.sum, on._per.max_prio) == (on.prio.data_ptr(), on.prio_sum.data_ptr(),
                                                             on.max_prio.data_ptr())
    assert abs(on._per.alpha - 0.6) < 1e-7 and abs(on._per.beta - 0.4) < 1e-7
    for beta in (1.5, -0.1, float("nan"), "0.4"):
        with pytest.raises(ValueError, match="uniform_replay"):
            on.sample(4, beta=beta)
    with pytest.raises(ValueError, match="one length"):
        on.update_priorities(torch.zeros(2), torch.zeros(3), torch.zeros(2))


# ---------------------------------------------------------------------- the restatement against brute force
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("T", [2, 3, 8])
def test_restatement_against_a_list_of_live_transitions(n, T):
    """300 random calls: pushes (with dones, drops, a missing diverged array), masked stages and priority updates whose
    rows were recorded some calls earlier (so some are stale), hold duplicates and rows out of range.  The model is a
    plain list of live transitions per env, each with the slot it went to, an id and its priority.  After every call
    prio > 0 exactly on the live transitions, the priorities and the sums are the list's, and no update lands on a
    transition that has left the ring."""
    rng = np.random.default_rng(1000 * n + T)
    ref = R.ReplayPerRef(n, T, 2)
    live = [collections.deque() for _ in range(n)]       # [slot, id, prio]
    cursor, next_id, top = [0] * n, 0, R.PRIO_ONE
    held = []                                            # (env, slot, id) recorded at earlier calls
    seen = collections.Counter()
    for t in range(300):
        kind = rng.random()
        if t == 0 or kind < 0.15:
            mask = None if t == 0 or rng.random() < 0.3 else rng.random(n) < 0.5
            ref.stage(mask, np.zeros((n, 15), np.float32))
            seen["stage"] += 1
        elif kind < 0.7:
            term, trunc, div = rng.random(n) < 0.12, rng.random(n) < 0.08, rng.random(n) < 0.15
            trunc |= div
            use_div = rng.random() < 0.85
            z = np.zeros((n, 15), np.float32)
            ref.push(z, z, np.zeros((n, 2), np.float32), np.zeros(n, np.float32), term, trunc, div if use_div else None)
            for e in range(n):
                if use_div and div[e]:
                    seen["drop"] += 1
                    continue
                live[e].append([cursor[e], next_id, top])
                next_id += 1
                cursor[e] = (cursor[e] + 1) % T
                if len(live[e]) > T - 1:
                    live[e].popleft()
                    seen["evicted"] += 1
        else:
            rows = [held[j] for j in rng.integers(0, len(held), rng.integers(1, 12))] if held else []
            rows += [(int(rng.integers(-2, n + 2)), int(rng.integers(-2, T + 2)), None) for _ in range(3)]
            rows += rows[:2] + rows[:1]                  # duplicates, some three times
            q = [int(x) for x in rng.choice([1, 2, 1000, R.PRIO_ONE, 3 * R.PRIO_ONE, 1 << 31, R.PRIO_MAX], len(rows))]
            ids_before = [{tr[0]: tr[1] for tr in live[e]} for e in range(n)]
            applied = ref.update([r[0] for r in rows], [r[1] for r in rows], q)
            best = {}
            for j, (e, s, ident) in enumerate(rows):
                tr = next((tr for tr in live[e] if tr[0] == s), None) if 0 <= e < n else None
                if tr is None:
                    assert j not in applied              # out of range, the staged slot, or evicted since
                    seen["skipped" if ident is None else "stale"] += 1
                    continue
                assert j in applied
                seen["overwritten since" if ident is not None and ident != tr[1] else "applied"] += 1
                best[(e, s)] = max(best.get((e, s), 0), q[j])
                top = max(top, q[j])
            for (e, s), v in best.items():
                next(tr for tr in live[e] if tr[0] == s)[2] = v
            assert ids_before == [{tr[0]: tr[1] for tr in live[e]} for e in range(n)]
        # record some rows for later updates
        for e in range(n):
            for tr in live[e]:
                if rng.random() < 0.2:
                    held.append((e, tr[0], tr[1]))
        held = held[-40:]
        # the state
        assert ref.invariant() and ref.max_prio == top
        run, sums = 0, ref.sums()
        for e in range(n):
            assert ref.valid_slots(e) == [tr[0] for tr in live[e]]
            assert [int(ref.prio[s, e]) for s in ref.valid_slots(e)] == [tr[2] for tr in live[e]]
            run += sum(tr[2] for tr in live[e])
            assert sums[e] == run
        assert sums[n] == run
    want = {"stage", "drop", "evicted", "applied", "skipped", "stale"} | ({"overwritten since"} if T > 2 else set())
    assert want <= {k for k, v in seen.items() if v}, sorted(seen.items())


def _filled(n, T, counts, seed=5):
    """a restatement whose env e holds counts[e] transitions at a wrapped cursor, every priority PRIO_ONE"""
    ref = R.ReplayPerRef(n, T, 2, seed=seed)
    for e, k in enumerate(counts):
        c = (e + T - 2) % T
        ref.meta[:, e] = c, k
        for j in range(k):
            ref.prio[(c - k + j) % T, e] = R.PRIO_ONE
    return ref


def test_equal_priorities_give_the_plain_pick():
    """floor(floor(h c M / 2^64) / c) = floor(h M / 2^64): 10,000 rows against tests/replay_ref.py's plain pick, for the
    fresh buffer's PRIO_ONE and for two other common values"""
    counts = [3, 0, 7, 1, 7, 0, 5]
    ref = _filled(7, 8, counts)
    plain = replay_ref.ReplayRef(7, 8, 2, seed=5)
    plain.meta[...] = ref.meta
    want = plain.sample(10000, 3)
    for c in (R.PRIO_ONE, 1, R.PRIO_MAX):
        ref.prio[ref.prio > 0] = c
        got = ref.sample(10000, 3)
        assert got["env"].tobytes() == want["env"].tobytes() and got["slot"].tobytes() == want["slot"].tobytes()
        assert (got["probs"] == np.float32(1 / 23)).all() and got["total"] == 23 * c
    assert len(set(zip(want["env"].tolist(), want["slot"].tolist()))) == 23


@pytest.mark.parametrize("seed,call", [(11, 0), (12, 7)])
def test_draw_frequencies(seed, call):
    """100,000 draws over 10 transitions spread 7 / 0 / 3 over three envs with the priorities 1, 2, .., 10 times PRIO_ONE:
    each frequency lies within 5 sigma of q / total (a condition on the restatement alone, for these seeds)"""
    ref = _filled(3, 9, [7, 0, 3], seed=seed)
    q = 0
    for e in range(3):
        for s in ref.valid_slots(e):
            q += 1
            ref.prio[s, e] = q * R.PRIO_ONE
    N, total = 100000, 55 * R.PRIO_ONE
    sums = ref.sums()
    assert sums == [28 * R.PRIO_ONE, 28 * R.PRIO_ONE, total, total]
    hits = collections.Counter()
    for i in range(N):
        e, s, k, qq = ref.pick(sums, draw(seed, call, i, 0))
        assert qq == int(ref.prio[s, e]) and ref.valid_slots(e)[k] == s
        hits[qq // R.PRIO_ONE] += 1
    assert sorted(hits) == list(range(1, 11))
    for j in range(1, 11):
        p = j / 55
        assert abs(hits[j] - N * p) <= 5 * math.sqrt(N * p * (1 - p)), (j, hits[j], N * p)


def test_probs_and_the_priority_formula():
    """probs is the float64 quotient cast once; the float64 priority and its clamp at the edges"""
    ref = _filled(2, 4, [3, 2])
    ref.prio[ref.valid_slots(0)[0], 0] = 1
    ref.prio[ref.valid_slots(1)[1], 1] = R.PRIO_MAX
    out = ref.sample(200, 0)
    total = out["total"]
    assert total == 3 * R.PRIO_ONE + 1 + R.PRIO_MAX > 1 << 32
    for i in range(200):
        assert out["probs"][i] == np.float32(out["q"][i] / total)
        assert out["wbase"][i] == np.float32(np.float32(5) * out["probs"][i])
    assert R.clamp_priority(R.priority64(float("nan"), 0.6, 1e-6)) == R.clamp_priority(R.priority64(0.0, 0.6, 1e-6)) == 16
    assert R.clamp_priority(R.priority64(float("inf"), 0.6, 1e-6)) == R.PRIO_MAX
    assert R.clamp_priority(R.priority64(-float("inf"), 1.0, 1e-6)) == R.PRIO_MAX
    assert R.clamp_priority(R.priority64(1e9, 1.0, 1e-6)) == R.PRIO_MAX
    assert R.clamp_priority(R.priority64(0.0, 1.0, 1e-6)) == 1
    assert R.clamp_priority(R.priority64(-2.0, 1.0, 1e-6)) == 2 * R.PRIO_ONE
    assert R.clamp_priority(R.priority64(123.0, 0.0, 1e-6)) == R.PRIO_ONE
    assert R.clamp_priority(R.priority64(float("inf"), 0.0, 1e-6)) == R.PRIO_ONE         # inf^0 = 1
