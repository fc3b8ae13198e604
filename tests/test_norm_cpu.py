"""CPU checks of the running normaliser (include/so100.h so100_norm_update / so100_norm_apply / so100_norm_return;
DESIGN.md §3.10): the float64 restatement (tests/norm_ref.py) against hand-worked values, its batch-splitting and
shard-merging properties, the option parsing of SO100VecEnv(normalize=...), the exported symbols under the unchanged
ABI 25, the struct mirrors, and every entry point's refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import norm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------- the restatement
def test_hand_worked_two_batches():
    """Column 0: batches (1, 2, 3) and (4, 6, 8); column 1: (10, 10, 10) and (-2, 0, 2); start (0, 1, 1e-4)."""
    r = norm_ref.RunningMeanStd(2)
    assert (r.mean == 0).all() and (r.var == 1).all() and r.count == 1e-4
    r.update([[1, 10], [2, 10], [3, 10]])
    # column 0: bm = 2, bv = ((1)^2 + 0 + 1^2) / 3 = 2/3, delta = 2, tot = 3.0001
    tot = 3.0001
    m0 = 2 * 3 / tot
    v0 = (1 * 1e-4 + (2 / 3) * 3 + 2 ** 2 * 1e-4 * 3 / tot) / tot
    # column 1: bm = 10, bv = 0, delta = 10
    m1 = 10 * 3 / tot
    v1 = (1 * 1e-4 + 0 * 3 + 10 ** 2 * 1e-4 * 3 / tot) / tot
    assert r.count == tot
    np.testing.assert_allclose(r.mean, [m0, m1], rtol=1e-15)
    np.testing.assert_allclose(r.var, [v0, v1], rtol=1e-15)
    np.testing.assert_allclose(r.mean, [1.9999333355554816, 9.999666677777407], rtol=1e-14)
    np.testing.assert_allclose(r.var, [0.6668111018523086, 0.0033664433444809865], rtol=1e-13)
    r.update([[4, -2], [6, 0], [8, 2]])
    # column 0: bm = 6, bv = (4 + 0 + 4) / 3 = 8/3; column 1: bm = 0, bv = 8/3
    tot2 = tot + 3
    d0, d1 = 6 - m0, 0 - m1
    m0b = m0 + d0 * 3 / tot2
    v0b = (v0 * tot + (8 / 3) * 3 + d0 ** 2 * tot * 3 / tot2) / tot2
    m1b = m1 + d1 * 3 / tot2
    v1b = (v1 * tot + (8 / 3) * 3 + d1 ** 2 * tot * 3 / tot2) / tot2
    assert r.count == tot2
    np.testing.assert_allclose(r.mean, [m0b, m1b], rtol=1e-15)
    np.testing.assert_allclose(r.var, [v0b, v1b], rtol=1e-15)
    # the same numbers from the pooled form over (1e-4 rows of mean 0 and variance 1) and the six rows
    np.testing.assert_allclose(r.mean, [3.999933334444426, 4.9999166680555325], rtol=1e-14)
    np.testing.assert_allclose(r.var, [5.666855547963164, 26.333327770926157], rtol=1e-14)
    y = norm_ref.normalize([[4.0, 5.0], [1e6, -1e6]], r)
    np.testing.assert_allclose(y[0], [(4 - m0b) / np.sqrt(v0b + 1e-8), (5 - m1b) / np.sqrt(v1b + 1e-8)], rtol=1e-15)
    assert (y[1] == [10.0, -10.0]).all()
    np.testing.assert_allclose(norm_ref.unnormalize(y[0], r), [4.0, 5.0], rtol=1e-15)


def _awkward(rng, n):
    """columns of awkward conditioning: mean 5 / sd 1e-3, a constant, +-10, a unit normal"""
    return np.stack([5.0 + 1e-3 * rng.standard_normal(n), np.full(n, 0.37), rng.uniform(-10, 10, n),
                     rng.standard_normal(n)], axis=1).astype(np.float32).astype(np.float64)


def test_one_batch_equals_two_halves():
    rng = np.random.default_rng(0)
    for n, cut in ((2, 1), (65, 32), (257, 1), (1000, 613)):
        x = _awkward(rng, n)
        one, two = norm_ref.RunningMeanStd(4), norm_ref.RunningMeanStd(4)
        one.update(x)
        two.update(x[:cut])
        two.update(x[cut:])
        # (1e-4 + n) against ((1e-4 + cut) + (n - cut)): the formula's own additions, one rounding apart
        assert abs(one.count - two.count) <= np.spacing(one.count)
        assert (np.abs(one.mean - two.mean) <= norm_ref.mean_bar(x)).all(), (n, one.mean - two.mean)
        assert (np.abs(one.var - two.var) <= norm_ref.var_bar(x)).all(), (n, one.var - two.var)


def test_empty_batch_and_mask():
    rng = np.random.default_rng(1)
    x = _awkward(rng, 40)
    r = norm_ref.RunningMeanStd(4)
    r.update(x)
    before = (r.mean.tobytes(), r.var.tobytes(), r.count)
    r.update(x, mask=np.zeros(40, bool))
    r.update(np.zeros((0, 4)))
    assert (r.mean.tobytes(), r.var.tobytes(), r.count) == before
    m = rng.random(40) < 0.3
    a, b = r.copy(), r.copy()
    a.update(x, mask=m)
    b.update(x[m])
    assert a.mean.tobytes() == b.mean.tobytes() and a.var.tobytes() == b.var.tobytes() and a.count == b.count


def _state(rms_by_key, ret):
    s = {}
    for k, r in list(rms_by_key.items()) + [("ret", ret)]:
        s[k + ".mean"], s[k + ".var"], s[k + ".count"] = r.mean.copy(), r.var.copy(), np.float64(r.count)
    return s


def test_merge_of_two_shards_equals_one_env_over_both():
    from gym_so100 import merge_normalize_states
    rng = np.random.default_rng(2)
    steps, na, nb = 7, 32, 33
    whole, a, b = (norm_ref.RunningMeanStd(4) for _ in range(3))
    wr, ar, br = (norm_ref.RunningMeanStd(1) for _ in range(3))
    seen, gseen = [], []
    for _ in range(steps):
        x = _awkward(rng, na + nb)
        g = rng.standard_normal((na + nb, 1))
        seen.append(x)
        gseen.append(g)
        whole.update(x), a.update(x[:na]), b.update(x[na:])
        wr.update(g), ar.update(g[:na]), br.update(g[na:])
    merged = merge_normalize_states([_state({"obs": a}, ar), _state({"obs": b}, br)])
    x_all = np.concatenate(seen)
    assert float(merged["obs.count"]) == whole.count
    assert (np.abs(merged["obs.mean"] - whole.mean) <= norm_ref.mean_bar(x_all)).all()
    assert (np.abs(merged["obs.var"] - whole.var) <= norm_ref.var_bar(x_all)).all()
    g_all = np.concatenate(gseen)
    assert (np.abs(merged["ret.mean"] - wr.mean) <= norm_ref.mean_bar(g_all)).all()
    assert (np.abs(merged["ret.var"] - wr.var) <= norm_ref.var_bar(g_all)).all()
    assert float(merged["ret.count"]) == wr.count
    # one shard alone is itself; a shard that saw nothing adds nothing
    alone = merge_normalize_states([_state({"obs": a}, ar)])
    assert alone["obs.mean"].tobytes() == a.mean.tobytes() and alone["obs.var"].tobytes() == a.var.tobytes()
    idle = merge_normalize_states([_state({"obs": a}, ar), _state({"obs": norm_ref.RunningMeanStd(4)},
                                                                  norm_ref.RunningMeanStd(1))])
    assert idle["obs.mean"].tobytes() == a.mean.tobytes() and float(idle["obs.count"]) == a.count
    with pytest.raises(ValueError):
        merge_normalize_states([])
    with pytest.raises(ValueError):
        merge_normalize_states([_state({"obs": a}, ar), _state({"agent_pos": b}, br)])


# ---------------------------------------------------------------------- options
def test_option_parsing():
    from gym_so100.normalize import NORMALIZE_DEFAULTS, normalize_options
    assert normalize_options(None) is None and normalize_options(False) is None
    assert NORMALIZE_DEFAULTS == dict(obs=True, reward=False, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                                      training=True)
    assert normalize_options(True) == NORMALIZE_DEFAULTS
    assert normalize_options({}) == NORMALIZE_DEFAULTS
    o = normalize_options(dict(reward=True, clip_obs=5, gamma=1, training=False))
    assert o["reward"] is True and o["clip_obs"] == 5.0 and o["gamma"] == 1.0 and o["training"] is False and o["obs"]
    assert normalize_options(dict(gamma=None))["gamma"] is None
    for bad in (dict(clip=3.0), dict(obs=1), dict(reward="yes"), dict(training=None), dict(clip_obs=0.0),
                dict(clip_obs=-1.0), dict(clip_obs=NAN), dict(clip_reward=INF), dict(clip_reward="x"), dict(epsilon=0.0),
                dict(epsilon=NAN), dict(epsilon=True), dict(gamma=0.0), dict(gamma=1.5), dict(gamma=NAN),
                dict(gamma=-0.1), dict(gamma="g"), dict(gamma=None, reward=True), "on", 1, [True]):
        with pytest.raises(ValueError):
            normalize_options(bad)


def test_env_refuses_bad_options_before_any_device_use():
    """SO100VecEnv checks normalize= first: these raise without a library load or a device."""
    from gym_so100 import SO100VecEnv
    from gym_so100.sb3 import SO100SB3VecEnv
    with pytest.raises(ValueError, match="unknown keys"):
        SO100VecEnv(4, normalize=dict(clip=3.0))
    with pytest.raises(ValueError, match="gamma"):
        SO100VecEnv(4, normalize=dict(gamma=2.0))
    with pytest.raises(ValueError, match="flattened pixel observation"):
        SO100VecEnv(4, task="so100_goal", obs_type="so100_pixels_agent_pos", normalize=True)
    with pytest.raises(ValueError, match="unknown keys"):
        SO100SB3VecEnv(4, normalize=dict(norm_obs=True))
    for name in ("obs_rms", "ret_rms", "training", "norm_reward", "get_original_obs", "get_original_reward",
                 "normalize_obs", "unnormalize_obs", "save", "load_stats"):
        assert hasattr(SO100SB3VecEnv, name), name
    for name in ("training", "obs_rms", "ret_rms", "normalize_obs", "unnormalize_obs", "normalize_state",
                 "set_normalize_state"):
        assert hasattr(SO100VecEnv, name), name


# ---------------------------------------------------------------------- the library
NEW_SYMBOLS = ("so100_norm_bytes", "so100_norm_ret_bytes", "so100_norm_limits", "so100_norm_work_bytes",
               "so100_norm_update", "so100_norm_apply", "so100_norm_return")


def test_symbols_structs_and_abi():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25        # additions only: the version stays
    for fn in NEW_SYMBOLS:
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn), fn
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    assert re.search(r"#define SO100_NORM_MAX_DIM 32\b", src) and re.search(r"#define SO100_NORM_MAX_SRC 3\b", src)
    assert (_native.SO100_NORM_MAX_DIM, _native.SO100_NORM_MAX_SRC) == (norm_ref.MAX_DIM, 3)
    assert lib.so100_norm_bytes() == ctypes.sizeof(_native.SO100Norm) == 32 + 3 * 32
    assert lib.so100_norm_ret_bytes() == ctypes.sizeof(_native.SO100NormRet) == 32
    for struct, mirror in (("so100_norm_src", _native.SO100NormSrc), ("so100_norm", _native.SO100Norm),
                           ("so100_norm_ret", _native.SO100NormRet)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in mirror._fields_], struct
    rows, groups = _native.norm_limits()
    assert rows >= 64 and groups >= 1
    # the workspace formula of the header
    for n in (0, 1, rows, rows + 1, rows * groups, rows * groups + 1, 10 * rows * groups):
        want = min(groups, max(1, -(-n // rows))) * 3 * 32 * 8
        assert lib.so100_norm_work_bytes(n) == want, n
    assert lib.so100_norm_work_bytes(-1) == -1 and b"n < 0" in lib.so100_last_error()


def test_norm_source_names_no_oracle_symbol():
    txt = open(os.path.join(ROOT, "gym-so100-c_amd", "csrc", "so100_norm.hip")).read()
    assert not re.search(r"oracle|so100o_", txt)
    mk = open(os.path.join(ROOT, "gym-so100-c_amd", "csrc", "Makefile")).read()
    assert "so100_norm.hip" in mk and "so100_norm.o" in mk          # built into the library and into its source hash


FAKE = 0x1000          # a non-NULL pointer no refusal below dereferences


def _norm(sources=((FAKE, 15, 0, 15, FAKE, 15),), **kw):
    from gym_so100 import _native
    return _native.SO100Norm(list(sources), **kw)


def _update(lib, nm, env=None, n=8, stats=FAKE, work=FAKE):
    rc = lib.so100_norm_update(env, None if nm is None else ctypes.byref(nm), n, None, ctypes.c_void_p(stats),
                               ctypes.c_void_p(work), None)
    return rc, lib.so100_last_error().decode()


def _apply(lib, nm, env=None, n=8, stats=FAKE):
    rc = lib.so100_norm_apply(env, None if nm is None else ctypes.byref(nm), n, None, ctypes.c_void_p(stats), None)
    return rc, lib.so100_last_error().decode()


RECORD_REFUSALS = [
    (dict(sources=()), "nsrc outside 1..3"),
    (dict(sources=((FAKE, 15, 0, 0, FAKE, 15),)), "dim outside 1..32"),
    (dict(sources=((FAKE, 40, 0, 33, FAKE, 40),)), "dim outside 1..32"),
    (dict(sources=((FAKE, 15, 0, -1, FAKE, 15),)), "dim outside 1..32"),
    (dict(sources=((FAKE, 15, 0, 15, FAKE, 15), (FAKE, 15, 0, 15, FAKE, 15), (FAKE, 3, 0, 3, FAKE, 3))),
     "total dim outside 1..32"),
    (dict(sources=((FAKE, 15, -1, 6, FAKE, 6),)), "offset < 0"),
    (dict(sources=((FAKE, 14, 9, 6, FAKE, 6),)), "stride smaller than offset + dim"),
    (dict(sources=((FAKE, 15, 0, 15, FAKE, 15), (FAKE, 2, 0, 3, FAKE, 3))), "stride smaller than offset + dim"),
    (dict(epsilon=0.0), "epsilon must be finite and > 0"), (dict(epsilon=-1e-8), "epsilon"), (dict(epsilon=NAN), "epsilon"),
    (dict(epsilon=INF), "epsilon"),
    (dict(clip=0.0), "clip must be finite and > 0"), (dict(clip=NAN), "clip"), (dict(clip=INF), "clip"),
    (dict(clip=-10.0), "clip"),
    (dict(flags=2), "unknown flags"),
]


@pytest.mark.parametrize("fn", ["update", "apply"])
def test_update_and_apply_refusals_need_no_device(fn):
    from gym_so100 import _native
    lib = _native.load()
    call = _update if fn == "update" else _apply
    name = "so100_norm_" + fn
    rc, err = call(lib, None)
    assert rc != 0 and err == f"{name}: NULL norm"
    nm = _norm()
    nm.size += 8                                       # checked first: the other fields are not looked at
    nm.nsrc = 99
    rc, err = call(lib, nm)
    assert rc != 0 and f"{name}: so100_norm.size 136, expected 128" in err
    for kw, text in RECORD_REFUSALS:
        rc, err = call(lib, _norm(**kw))
        assert rc != 0 and err.startswith(name + ": ") and text in err, (kw, err)
    if fn == "apply":
        rc, err = call(lib, _norm(sources=((FAKE, 15, 9, 6, FAKE, 5),)))
        assert rc != 0 and "y_stride smaller than dim" in err
    rc, err = call(lib, _norm(), n=-1)
    assert rc != 0 and "n < 0" in err
    rc, err = call(lib, _norm())                       # a good record: the env is looked at next
    assert rc != 0 and err == f"{name}: NULL env"


def _return(lib, args, env=None, n=8):
    p = ctypes.c_void_p(FAKE)
    rc = lib.so100_norm_return(env, None if args is None else ctypes.byref(args), n, p, None, None, p, p, p, p, None)
    return rc, lib.so100_last_error().decode()


def test_return_refusals_need_no_device():
    from gym_so100 import _native
    lib = _native.load()
    rc, err = _return(lib, None)
    assert rc != 0 and err == "so100_norm_return: NULL args"
    a = _native.SO100NormRet(flags=3)
    a.size = 24
    a.gamma = 7.0
    rc, err = _return(lib, a)
    assert rc != 0 and "so100_norm_ret.size 24, expected 32" in err
    for kw, text in ((dict(gamma=0.0), "gamma outside (0, 1]"), (dict(gamma=1.0001), "gamma"), (dict(gamma=NAN), "gamma"),
                     (dict(gamma=-0.5), "gamma"), (dict(epsilon=0.0), "epsilon must be finite and > 0"),
                     (dict(epsilon=NAN), "epsilon"), (dict(clip=0.0), "clip must be finite and > 0"),
                     (dict(clip=INF), "clip"), (dict(flags=4), "unknown flags")):
        rc, err = _return(lib, _native.SO100NormRet(**kw))
        assert rc != 0 and err.startswith("so100_norm_return: ") and text in err, (kw, err)
    rc, err = _return(lib, _native.SO100NormRet(flags=3), n=-2)
    assert rc != 0 and "n < 0" in err
    rc, err = _return(lib, _native.SO100NormRet(flags=3, gamma=1.0))
    assert rc != 0 and err == "so100_norm_return: NULL env"
    r, g = ctypes.c_int(), ctypes.c_int()
    assert lib.so100_norm_limits(None, ctypes.byref(g)) != 0 and b"NULL argument" in lib.so100_last_error()
    assert lib.so100_norm_limits(ctypes.byref(r), ctypes.byref(g)) == 0 and (r.value, g.value) == _native.norm_limits()
