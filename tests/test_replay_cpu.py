"""CPU checks of the uniform replay buffer (include/so100.h so100_replay_push / so100_replay_stage / so100_replay_scan /
so100_replay_sample): the struct mirrors and the exported symbols under the unchanged ABI 25, the
storage formula, every entry point's refusals (none needs a device), the option parsing of
SO100VecEnv(uniform_replay=...), and the restatement (tests/replay_ref.py) against a deque model of SB3's buffer and
against the uniform distribution of the shifts."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest

import her_ref
import replay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY_SYMBOLS = ("so100_replay_bytes", "so100_replay_step_bytes", "so100_replay_out_bytes",
                  "so100_replay_storage_bytes", "so100_replay_push", "so100_replay_stage", "so100_replay_scan",
                  "so100_replay_sample")


# ---------------------------------------------------------------------- ABI
def test_symbols_and_abi():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25
    header = open(os.path.join(ROOT, "include", "so100.h")).read()
    assert re.search(r"#define SO100_ABI_VERSION 25\b", header)
    for fn in REPLAY_SYMBOLS:
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn), fn
        assert re.search(r"\b%s\(" % fn, header), fn


def test_struct_mirrors():
    from gym_so100 import _native
    lib = _native.load()
    assert lib.so100_replay_bytes() == ctypes.sizeof(_native.SO100Replay) == 40 + 8 + 9 * 8
    assert lib.so100_replay_step_bytes() == ctypes.sizeof(_native.SO100ReplayStep) == 8 + 9 * 8
    assert lib.so100_replay_out_bytes() == ctypes.sizeof(_native.SO100ReplayOut) == 8 + 10 * 8
    h = _native.SO100Replay(n=3, T=7, action_dim=5, planes=2, H=12, W=16, chan=3, P=1152, pad=4, seed=-1)
    assert (h.size, h.n, h.T, h.action_dim) == (ctypes.sizeof(h), 3, 7, 5)
    assert (h.planes, h.H, h.W, h.chan, h.P, h.pad) == (2, 12, 16, 3, 1152, 4)
    assert h.seed == 0xFFFFFFFFFFFFFFFF
    assert _native.SO100Replay.seed.offset == 40 and _native.SO100Replay.obs.offset == 48
    assert _native.SO100Replay.prefix.offset == 48 + 8 * 8
    assert _native.SO100_REPLAY_MAX_ACTION == 16 and _native.SO100_REPLAY_MAX_PAD == 64


def test_storage_bytes():
    from gym_so100 import _native
    lib = _native.load()
    for n, T, A, layout in [(1, 2, 1, None), (8, 16, 6, (1, 3, 5, 3)), (65, 8, 5, (6, 12, 16, 1)), (0, 3, 6, None)]:
        r = replay_ref.ReplayRef(n, T, A, layout)
        held = sum(getattr(r, k).nbytes for k in r.ARRAYS) + 4 * (n + 1)       # and the prefix array
        assert lib.so100_replay_storage_bytes(n, T, A, r.P) == held == replay_ref.storage_bytes(n, T, A, r.P)
    # 65,536 envs x 300 slots of one 64 x 48 RGB image pair: a 32-bit product would wrap
    n, T, A, P = 65536, 300, 6, 9216
    want = n * T * (4 * (15 + 15 + A + 1) + 1 + 2 * P) + 4 * (3 * n + 1)
    assert want > 1 << 38 and lib.so100_replay_storage_bytes(n, T, A, P) == want
    for bad in [(-1, 4, 6, 0), (4, 1, 6, 0), (4, 0, 6, 0), (1 << 16, 1 << 15, 6, 0), (4, 4, 0, 0), (4, 4, 17, 0),
                (4, 4, 6, -1)]:
        assert lib.so100_replay_storage_bytes(*bad) == -1
        assert b"so100_replay_storage_bytes" in lib.so100_last_error()
    assert lib.so100_replay_storage_bytes((1 << 16) - 1, 1 << 15, 6, 0) > 0     # T n = 2^31 - 2^15


IMG = dict(planes=1, H=3, W=5, chan=3, P=45)


def _records(images=False, **kw):
    """records whose every pointer is a (never dereferenced) non-NULL address; images: with the image arrays"""
    from gym_so100 import _native
    fake = ctypes.c_void_p(0x1000)
    is_img = lambda k: "img" in k or "pixels" in k  # noqa: E731
    keep = lambda names: {k: fake for k in names if images or not is_img(k)}  # noqa: E731
    rec = _native.SO100Replay(**{**dict(n=4, T=8, action_dim=6), **(IMG if images else {}), **kw},
                              **keep(_native.REPLAY_ARRAYS))
    step = _native.SO100ReplayStep(**keep(_native.REPLAY_STEP_INPUTS))
    out = _native.SO100ReplayOut(**keep(_native.REPLAY_OUTPUTS))
    return rec, step, out, fake


def _calls(lib, env, rec, step, out, batch=4, obs=True, pixels=None):
    """the four entry points on these records: name -> status"""
    B = ctypes.byref
    fake = ctypes.c_void_p(0x1000)
    r = B(rec) if rec else None
    return {"so100_replay_push": lambda: lib.so100_replay_push(env, r, B(step) if step else None, None),
            "so100_replay_stage": lambda: lib.so100_replay_stage(env, r, None, fake if obs else None, pixels, None),
            "so100_replay_scan": lambda: lib.so100_replay_scan(env, r, None),
            "so100_replay_sample": lambda: lib.so100_replay_sample(env, r, batch, 0, B(out) if out else None, None)}


def _refused(lib, call, text):
    assert call() != 0
    msg = lib.so100_last_error().decode()
    assert text in msg, msg


def test_refusals_of_every_entry_point():
    """each argument error of the header: nonzero, its text, and (the pointers being fakes, the env NULL) no device"""
    from gym_so100 import _native
    lib = _native.load()
    rec, step, out, fake = _records()
    for name, call in _calls(lib, fake, None, step, out).items():
        _refused(lib, call, name + ": NULL replay")
    rec.size += 4
    for name, call in _calls(lib, fake, rec, step, out).items():
        _refused(lib, call, "so100_replay")
        assert name in lib.so100_last_error().decode() and "size" in lib.so100_last_error().decode()
    shape = "planes, H, W, chan and P do not agree"
    for kw, text in [(dict(T=1), "T < 2"), (dict(T=0), "T < 2"), (dict(T=-3), "T < 2"), (dict(n=-1), "n < 0"),
                     (dict(n=1 << 16, T=1 << 15), "T * n >= 2^31"), (dict(action_dim=0), "action_dim outside 1..16"),
                     (dict(action_dim=17), "action_dim outside 1..16"), (dict(P=-1), shape), (dict(P=45), shape),
                     (dict(planes=1), shape), (dict(chan=3), shape), (dict(**{**IMG, "P": 44}), shape),
                     (dict(**{**IMG, "H": 0}), shape), (dict(**{**IMG, "W": -5, "chan": -3}), shape),
                     (dict(planes=1 << 16, H=1 << 16, W=1 << 16, chan=1 << 16, P=1 << 16), shape),
                     (dict(pad=-1), "pad outside 0..64"), (dict(**IMG, pad=65), "pad outside 0..64"),
                     (dict(pad=1), "pad without images")]:
        rec = _records(**kw)[0]
        for name, call in _calls(lib, fake, rec, step, out).items():
            _refused(lib, call, name + ": " + text)
    # the order: the record's numbers come before the env and the pointers
    rec = _records(T=1)[0]
    rec.obs = None
    for name, call in _calls(lib, None, rec, None, None).items():
        _refused(lib, call, name + ": T < 2")
    # the sample's own: batch, the output record
    rec = _records()[0]
    sample = lambda h, o=out, b=4: _calls(lib, fake, h, step, o, b)["so100_replay_sample"]  # noqa: E731
    _refused(lib, sample(rec, b=-1), "batch < 0")
    _refused(lib, sample(rec, o=None), "NULL out")
    bad_out = _records()[2]
    bad_out.size -= 8
    _refused(lib, sample(rec, o=bad_out), "so100_replay_out")
    # the push's own record
    _refused(lib, _calls(lib, fake, rec, None, out)["so100_replay_push"], "NULL step")
    bad_step = _records()[1]
    bad_step.size = 0
    _refused(lib, _calls(lib, fake, rec, bad_step, out)["so100_replay_push"], "so100_replay_step")
    # NULL pointers: the env, every array of the record, every required input / output
    for name, call in _calls(lib, None, rec, step, out).items():
        _refused(lib, call, name + ": NULL env")
    for k in _native.REPLAY_ARRAYS:
        if "img" in k:
            continue
        h = _records()[0]
        setattr(h, k, None)
        for name, call in _calls(lib, fake, h, step, out).items():
            _refused(lib, call, name + ": NULL array in so100_replay")
    for k in _native.REPLAY_STEP_INPUTS:
        if k in ("diverged", "pixels", "final_pixels"):
            continue                                     # optional, or an image
        st = _records()[1]
        setattr(st, k, None)
        _refused(lib, _calls(lib, fake, rec, st, out)["so100_replay_push"], "NULL pointer in so100_replay_step")
    for k in _native.REPLAY_OUTPUTS:
        if "pixels" in k:
            continue
        o = _records()[2]
        setattr(o, k, None)
        _refused(lib, sample(rec, o=o), "NULL pointer in so100_replay_out")
    _refused(lib, _calls(lib, fake, rec, step, out, obs=False)["so100_replay_stage"], "NULL obs")
    # image pointers present with P == 0 ...
    for k in ("obs_img", "next_img"):
        h = _records()[0]
        setattr(h, k, fake)
        for name, call in _calls(lib, fake, h, step, out).items():
            _refused(lib, call, name + ": image arrays in so100_replay with P == 0")
    for k in ("pixels", "final_pixels"):
        st = _records()[1]
        setattr(st, k, fake)
        _refused(lib, _calls(lib, fake, rec, st, out)["so100_replay_push"], "image pointers in so100_replay_step")
    for k in ("pixels", "next_pixels"):
        o = _records()[2]
        setattr(o, k, fake)
        _refused(lib, sample(rec, o=o), "image pointers in so100_replay_out")
    _refused(lib, _calls(lib, fake, rec, step, out, pixels=fake)["so100_replay_stage"], "pixels with P == 0")
    # ... and absent with P > 0
    irec, istep, iout, _ = _records(images=True)
    for k in ("obs_img", "next_img"):
        h = _records(images=True)[0]
        setattr(h, k, None)
        for name, call in _calls(lib, fake, h, istep, iout, pixels=fake).items():
            _refused(lib, call, name + ": NULL image array in so100_replay")
    for k in ("pixels", "final_pixels"):
        st = _records(images=True)[1]
        setattr(st, k, None)
        _refused(lib, _calls(lib, fake, irec, st, iout)["so100_replay_push"], "NULL image pointer in so100_replay_step")
    for k in ("pixels", "next_pixels"):
        o = _records(images=True)[2]
        setattr(o, k, None)
        _refused(lib, _calls(lib, fake, irec, istep, o)["so100_replay_sample"], "NULL image pointer in so100_replay_out")
    _refused(lib, _calls(lib, fake, irec, istep, iout)["so100_replay_stage"], "NULL pixels with P > 0")
    # nothing to do is no error and reaches no device: n = 0 (push, stage), batch = 0 (sample)
    empty = _records(n=0)[0]
    assert _calls(lib, fake, empty, step, out)["so100_replay_push"]() == 0
    assert _calls(lib, fake, empty, step, out)["so100_replay_stage"]() == 0
    assert _calls(lib, fake, rec, step, out, batch=0)["so100_replay_sample"]() == 0


# ---------------------------------------------------------------------- options
def test_uniform_replay_options():
    from gym_so100.replay import UNIFORM_REPLAY_DEFAULTS, augment_pad, image_layout, uniform_replay_options
    assert UNIFORM_REPLAY_DEFAULTS == dict(buffer_size=None, augment=None, seed=None)
    assert uniform_replay_options(None) is None
    o = uniform_replay_options(dict(buffer_size=1000), num_envs=3)
    assert o["T"] == 333 and o["pad"] == 0 and o["seed"] is None
    pix = dict(num_envs=8, task="so100_touch_cube", obs_type="so100_pixels_agent_pos")
    assert uniform_replay_options(dict(buffer_size=40, augment=True, seed=7), **pix)["pad"] == 4
    assert [augment_pad(a) for a in (None, False, True, 0, 1, 64, dict(pad=3), np.int64(2))] == [0, 0, 4, 0, 1, 64, 3, 2]
    for bad in [True, 5, dict(), dict(buffer_size=None), dict(buffer_size=0), dict(buffer_size=2.5),
                dict(buffer_size=True), dict(buffer_size=10, seed=0.5), dict(buffer_size=10, size=3),
                dict(buffer_size=10, augment=-1), dict(buffer_size=10, augment=65), dict(buffer_size=10, augment=1.5),
                dict(buffer_size=10, augment="shift"), dict(buffer_size=10, augment=dict(pad=4, mode="x")),
                dict(buffer_size=10, augment=dict()), dict(buffer_size=10, augment=dict(pad=True))]:
        with pytest.raises(ValueError, match="uniform_replay"):
            uniform_replay_options(bad)
    good = dict(buffer_size=40)
    with pytest.raises(ValueError, match="replay="):
        uniform_replay_options(good, num_envs=8, task="so100_goal")
    for kw in [dict(autoreset=False), dict(num_envs=21), dict(num_envs=41)]:
        with pytest.raises(ValueError, match="uniform_replay"):
            uniform_replay_options(good, **{**dict(num_envs=8, task="so100_touch_cube"), **kw})
    with pytest.raises(ValueError, match="pixel"):
        uniform_replay_options(dict(buffer_size=40, augment=2), num_envs=8, task="so100_touch_cube")
    assert uniform_replay_options(dict(buffer_size=40, augment=0), num_envs=8, task="so100_touch_cube")["pad"] == 0
    assert image_layout((8, 12, 16, 3), False) == (1, 12, 16, 3)
    assert image_layout((8, 3, 12, 16), True) == (3, 12, 16, 1)
    assert image_layout((8, 2, 12, 16, 3), False) == (2, 12, 16, 3)
    assert image_layout((8, 2, 3, 12, 16), True) == (6, 12, 16, 1)


def test_constructor_raises_before_any_device_work(monkeypatch):
    """every ValueError of uniform_replay=... comes before the library is loaded or a device touched"""
    from gym_so100 import SO100VecEnv, _native
    from gym_so100.sb3 import SO100ReplayBuffer, SO100SB3VecEnv

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "load", no_device)
    for kw in [dict(task="so100_goal", uniform_replay=dict(buffer_size=1 << 20)),
               dict(autoreset=False, uniform_replay=dict(buffer_size=1 << 20)),
               dict(uniform_replay=dict(buffer_size=15)),                                  # 15 // 8 = 1 slot per env
               dict(uniform_replay=dict(buffer_size=1 << 20, augment=True)),               # the state observation
               dict(obs_type="so100_pixels_agent_pos", uniform_replay=dict(buffer_size=64, augment=65)),
               dict(uniform_replay=dict(buffer_size=1 << 20, bogus=1)),
               dict(uniform_replay=dict(buffer_size=1 << 20, seed="x")),
               dict(uniform_replay=True)]:
        with pytest.raises(ValueError, match="uniform_replay"):
            SO100VecEnv(8, **{**dict(task="so100_touch_cube"), **kw})
    with pytest.raises(ValueError, match="replay="):
        SO100VecEnv(8, task="so100_goal", uniform_replay=dict(buffer_size=1 << 20))
    with pytest.raises(ValueError, match="uniform_replay"):
        SO100SB3VecEnv(8, task="so100_goal", uniform_replay=dict(buffer_size=1 << 20))
    with pytest.raises(ValueError, match="uniform_replay"):
        SO100ReplayBuffer(env=None)


# ---------------------------------------------------------------------- the restatement
def _row(e, t, width):
    """a row that encodes (env, push index)"""
    return np.float32(1000 * e + t) + np.arange(width, dtype=np.float32) / 16


def _img(e, t, P, salt=0):
    """P bytes that encode (env, push index, byte index)"""
    return ((np.arange(P) * 7 + 31 * e + 101 * t + salt) % 251).astype(np.uint8)


@pytest.mark.parametrize("n,T,layout,seed", [(1, 2, None, 0), (3, 3, (1, 3, 5, 3), 1), (5, 8, None, 2),
                                             (4, 13, (2, 2, 3, 1), 3)])
def test_ring_is_one_deque_per_env(n, T, layout, seed):
    """random done / diverged / masked-reset scripts: the valid interval of every env holds exactly the transitions of a
    deque(maxlen=T - 1) that appends every push but the diverged ones, oldest first, each with the observation that was
    current before its step (the staged one after a reset) and the true next one"""
    rng = np.random.default_rng(seed)
    ref = replay_ref.ReplayRef(n, T, 2, layout)
    P = ref.P
    model = [collections.deque(maxlen=T - 1) for _ in range(n)]
    obs0 = np.stack([_row(e, -1, 15) for e in range(n)])
    pix0 = np.stack([_img(e, -1, P) for e in range(n)]) if P else None
    ref.stage(None, obs0, pix0)
    before = [(obs0[e].copy(), None if not P else pix0[e].copy()) for e in range(n)]
    for t in range(6 * T + 5):
        obs = np.stack([_row(e, t, 15) for e in range(n)])
        fin_obs = obs + 0.5
        pix = np.stack([_img(e, t, P) for e in range(n)]) if P else None
        fin_pix = np.stack([_img(e, t, P, salt=13) for e in range(n)]) if P else None
        term = rng.random(n) < 0.15
        trunc = rng.random(n) < 0.1
        div = rng.random(n) < 0.1
        trunc |= div                                     # the step truncates what it flags as diverged
        done = term | trunc
        act = np.stack([_row(e, t, 2) for e in range(n)])
        rew = -np.arange(n, dtype=np.float32) - t
        if P:
            fin_pix[~done] = 255                         # stale rows: never read
        ref.push(obs, fin_obs, act, rew, term, trunc, div if t % 2 else None, pix, fin_pix)
        for e in range(n):
            if not (t % 2 and div[e]):
                nxt = (fin_obs[e], None if not P else fin_pix[e]) if done[e] else (obs[e], None if not P else pix[e])
                model[e].append((before[e], nxt, act[e].copy(), float(rew[e]), int(term[e])))
            before[e] = (obs[e].copy(), None if not P else pix[e].copy())
        if t % 7 == 3:                                   # a user reset of some envs
            mask = rng.random(n) < 0.5
            robs = obs + 7
            rpix = None if not P else (pix ^ 0x55)
            ref.stage(mask, robs, rpix)
            for e in np.flatnonzero(mask):
                before[e] = (robs[e].copy(), None if not P else rpix[e].copy())
        assert (ref.meta[1] <= T - 1).all() and (ref.meta >= 0).all() and (ref.meta[0] < T).all()
        for e in range(n):
            slots = ref.valid_slots(e)
            assert len(slots) == len(model[e])
            for s, (b, nx, a, r, tm) in zip(slots, model[e]):
                assert (ref.obs[s, e] == b[0]).all() and (ref.next_obs[s, e] == nx[0]).all()
                assert (ref.action[s, e] == a).all() and float(ref.reward[s, e]) == r and int(ref.terminated[s, e]) == tm
                if P:
                    assert (ref.obs_img[s, e] == b[1]).all() and (ref.next_img[s, e] == nx[1]).all()
            c = int(ref.meta[0, e])                      # the staged half of the next transition
            assert (ref.obs[c, e] == before[e][0]).all() and (not P or (ref.obs_img[c, e] == before[e][1]).all())
    assert all(len(m) == T - 1 for m in model)


def test_sample_restatement_draws_only_valid_transitions():
    """7, 0 and 3 valid transitions of T = 8: every (env, slot) drawn is valid, the env with none is never drawn, a call
    repeats itself and two calls differ, an empty buffer gives zeros with slot -1"""
    ref = replay_ref.ReplayRef(3, 8, 1, (1, 3, 5, 3), seed=1234)
    z15, z1 = np.zeros((3, 15), np.float32), np.zeros((3, 1), np.float32)
    empty = ref.sample(5, 0, pad=4)
    assert (empty["slot"] == -1).all() and all((v == 0).all() for k, v in empty.items() if k != "slot")
    for t in range(9):
        pix = np.stack([_img(e, t, 45) for e in range(3)])
        div = np.array([t >= 7, True, t % 3 != 0])
        ref.push(z15 + t, z15, z1, np.full(3, t, np.float32), div & False, div & False, div, pix, pix)
    assert ref.meta[1].tolist() == [7, 0, 3]
    a, b, c = ref.sample(500, 3, pad=4), ref.sample(500, 3, pad=4), ref.sample(500, 4, pad=4)
    assert all((a[k] == b[k]).all() for k in a) and (a["slot"] != c["slot"]).any() and (a["shift"] != c["shift"]).any()
    assert set(a["env"].tolist()) == {0, 2}
    for e, s in zip(a["env"], a["slot"]):
        assert s in ref.valid_slots(e)
    assert a["shift"].min() == 0 and a["shift"].max() == 8
    plain = ref.sample(500, 3, pad=0)
    assert (plain["shift"] == 0).all() and (plain["slot"] == a["slot"]).all()
    centred = (a["shift"][:, :2] == 4).all(axis=1)       # the shift that moves nothing
    assert centred.any() and (a["pixels"][centred] == plain["pixels"][centred]).all()
    assert (a["pixels"][~centred] != plain["pixels"][~centred]).any()


def test_shift_against_numpy_pad_and_crop():
    """the clamp rule is replicate padding followed by a crop at (dx, dy)"""
    rng = np.random.default_rng(0)
    for layout, pad in [((1, 3, 5, 3), 4), ((6, 12, 16, 1), 1), ((2, 12, 16, 3), 4)]:
        img = rng.integers(0, 256, layout, dtype=np.uint8)
        _, H, W, _ = layout
        padded = np.pad(img, ((0, 0), (pad, pad), (pad, pad), (0, 0)), mode="edge")
        for dx in range(2 * pad + 1):
            for dy in range(2 * pad + 1):
                assert (replay_ref.shifted(img, dx, dy, pad) == padded[:, dy:dy + H, dx:dx + W]).all()


@pytest.mark.parametrize("seed,call,field", [(s, c, f) for s in (0, 7) for c in (0, 1) for f in (2, 3)])
def test_shifts_are_uniform(seed, call, field):
    """100,000 rows, pad 1 and 4: every (dx, dy) cell within 5 sigma of 1 / S^2, sigma = sqrt(p (1 - p) / rows)"""
    rows = 100_000
    h = [her_ref.draw(seed, call, i, field) for i in range(rows)]
    for pad in (1, 4):
        S = 2 * pad + 1
        hits = np.zeros((S, S), np.int64)
        for x in h:
            dx, dy = replay_ref.shift_of(x, pad)
            hits[dy, dx] += 1
        p = 1 / S ** 2
        sigma = np.sqrt(p * (1 - p) / rows)
        worst = np.abs(hits / rows - p).max() / sigma
        print(f"seed {seed} call {call} field {field} pad {pad}: worst cell {worst:.2f} sigma")
        assert hits.sum() == rows and worst <= 5


def test_obs_and_next_shifts_are_independent():
    """the two images of a row take different draws: at pad 4 their dy agree about 1 time in 9"""
    rows, pad = 100_000, 4
    same = sum(replay_ref.shift_of(her_ref.draw(0, 0, i, 2), pad)[1] == replay_ref.shift_of(her_ref.draw(0, 0, i, 3), pad)[1]
               for i in range(rows))
    p = 1 / 9
    assert abs(same / rows - p) <= 5 * np.sqrt(p * (1 - p) / rows), same
