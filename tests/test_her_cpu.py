"""CPU checks of the hindsight replay buffer (include/so100.h so100_her_push / so100_her_discard / so100_her_scan /
so100_her_sample): the struct mirrors and the exported symbols under the unchanged ABI 25, every entry
point's refusals (none needs a device), the option parsing of SO100VecEnv(replay=...), and the restatement
(tests/her_ref.py) against an episode-list model of SB3's buffer and against the uniform distribution."""
import ctypes
import os
import re

import numpy as np
import pytest

import her_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HER_SYMBOLS = ("so100_her_bytes", "so100_her_step_bytes", "so100_her_out_bytes", "so100_her_limits",
               "so100_her_storage_bytes", "so100_her_push", "so100_her_discard", "so100_her_scan", "so100_her_sample")


# ---------------------------------------------------------------------- ABI
def test_symbols_and_abi():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25
    header = open(os.path.join(ROOT, "include", "so100.h")).read()
    for fn in HER_SYMBOLS:
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn), fn
        assert re.search(r"\b%s\(" % fn, header), fn


def test_struct_mirrors():
    from gym_so100 import _native
    lib = _native.load()
    assert lib.so100_her_bytes() == ctypes.sizeof(_native.SO100Her) == 24 + 8 + 12 * 8
    assert lib.so100_her_step_bytes() == ctypes.sizeof(_native.SO100HerStep) == 8 + 11 * 8
    assert lib.so100_her_out_bytes() == ctypes.sizeof(_native.SO100HerOut) == 8 + 12 * 8
    h = _native.SO100Her(n=3, T=7, action_dim=5, strategy=2, n_sampled_goal=1, seed=-1)
    assert (h.size, h.n, h.T, h.action_dim, h.strategy, h.n_sampled_goal) == (ctypes.sizeof(h), 3, 7, 5, 2, 1)
    assert h.seed == 0xFFFFFFFFFFFFFFFF
    assert _native.SO100Her.seed.offset == 24 and _native.SO100Her.obs.offset == 32
    assert _native.SO100Her.prefix.offset == 32 + 11 * 8
    assert _native.HER_STRATEGIES == her_ref.STRATEGIES


def test_limits_and_storage_bytes():
    from gym_so100 import _native
    lib = _native.load()
    w, tile = _native.her_limits()
    assert w >= 64 and w % 64 == 0 and tile % w == 0
    assert lib.so100_her_limits(None, None) != 0 and b"NULL" in lib.so100_last_error()
    for n, T, A in [(1, 1, 1), (8, 16, 6), (65, 8, 5), (0, 3, 6)]:
        r = her_ref.HerRef(n, T, A)
        held = sum(getattr(r, k).nbytes for k in r.ARRAYS) + 4 * (n + 1)       # and the prefix array
        assert lib.so100_her_storage_bytes(n, T, A) == held
    for bad in [(-1, 4, 6), (4, 0, 6), (1 << 16, 1 << 15, 6), (4, 4, 0), (4, 4, 17)]:
        assert lib.so100_her_storage_bytes(*bad) == -1
        assert b"so100_her_storage_bytes" in lib.so100_last_error()
    assert lib.so100_her_storage_bytes((1 << 16) - 1, 1 << 15, 6) > 0          # T n = 2^31 - 2^15


def _records(**kw):
    """a record whose every pointer is a (never dereferenced) non-NULL address"""
    from gym_so100 import _native
    fake = ctypes.c_void_p(0x1000)
    her = _native.SO100Her(**{**dict(n=4, T=8, action_dim=6), **kw}, **{k: fake for k in _native.HER_ARRAYS})
    step = _native.SO100HerStep(**{k: fake for k in _native.HER_STEP_INPUTS})
    out = _native.SO100HerOut(**{k: fake for k in _native.HER_OUTPUTS})
    return her, step, out, fake


def _calls(lib, env, her, step, out, batch=4):
    """the four entry points on these records: name -> status"""
    B = ctypes.byref
    return {"so100_her_push": lambda: lib.so100_her_push(env, B(her) if her else None, B(step) if step else None, None),
            "so100_her_discard": lambda: lib.so100_her_discard(env, B(her) if her else None, None, None, None, None),
            "so100_her_scan": lambda: lib.so100_her_scan(env, B(her) if her else None, None),
            "so100_her_sample": lambda: lib.so100_her_sample(env, B(her) if her else None, batch, 0,
                                                             B(out) if out else None, None)}


def _refused(lib, call, text):
    assert call() != 0
    msg = lib.so100_last_error().decode()
    assert text in msg, msg


def test_refusals_of_every_entry_point():
    """each argument error of the header: nonzero, its text, and (the pointers being fakes, the env NULL) no device"""
    from gym_so100 import _native
    lib = _native.load()
    her, step, out, fake = _records()
    for name, call in _calls(lib, fake, None, step, out).items():
        _refused(lib, call, name + ": NULL her")
    her.size += 4
    for name, call in _calls(lib, fake, her, step, out).items():
        _refused(lib, call, "so100_her")
        assert name in lib.so100_last_error().decode() and "size" in lib.so100_last_error().decode()
    for kw, text in [(dict(T=0), "T < 1"), (dict(T=-3), "T < 1"), (dict(n=-1), "n < 0"),
                     (dict(n=1 << 16, T=1 << 15), "T * n >= 2^31"), (dict(action_dim=0), "action_dim"),
                     (dict(action_dim=17), "action_dim")]:
        her = _records(**kw)[0]
        for name, call in _calls(lib, fake, her, step, out).items():
            _refused(lib, call, name + ": " + text)
    # the sample's own: strategy, n_sampled_goal, batch, the output record
    her = _records()[0]
    sample = lambda h, o=out, b=4: _calls(lib, fake, h, step, o, b)["so100_her_sample"]  # noqa: E731
    _refused(lib, sample(_records(strategy=3)[0]), "unknown strategy")
    _refused(lib, sample(_records(strategy=-1)[0]), "unknown strategy")
    _refused(lib, sample(_records(n_sampled_goal=-1)[0]), "n_sampled_goal < 0")
    _refused(lib, sample(her, b=-1), "batch < 0")
    _refused(lib, sample(her, o=None), "NULL out")
    bad_out = _records()[2]
    bad_out.size -= 8
    _refused(lib, sample(her, o=bad_out), "so100_her_out")
    # the push's own record
    _refused(lib, _calls(lib, fake, her, None, out)["so100_her_push"], "NULL step")
    bad_step = _records()[1]
    bad_step.size = 0
    _refused(lib, _calls(lib, fake, her, bad_step, out)["so100_her_push"], "so100_her_step")
    # NULL pointers: the env, every array of the record, every required input / output
    for name, call in _calls(lib, None, her, step, out).items():
        _refused(lib, call, name + ": NULL env")
    for k in _native.HER_ARRAYS:
        h = _records()[0]
        setattr(h, k, None)
        for name, call in _calls(lib, fake, h, step, out).items():
            _refused(lib, call, name + ": NULL array")
    for k in _native.HER_STEP_INPUTS:
        if k in ("diverged", "discard"):
            continue                                     # optional
        st = _records()[1]
        setattr(st, k, None)
        _refused(lib, _calls(lib, fake, her, st, out)["so100_her_push"], "NULL pointer in so100_her_step")
    for k in _native.HER_OUTPUTS:
        o = _records()[2]
        setattr(o, k, None)
        _refused(lib, sample(her, o=o), "NULL pointer in so100_her_out")


# ---------------------------------------------------------------------- options
def test_replay_options():
    from gym_so100.replay import REPLAY_DEFAULTS, replay_options
    assert replay_options(None) is None
    assert REPLAY_DEFAULTS["n_sampled_goal"] == 4 and REPLAY_DEFAULTS["goal_selection_strategy"] == "future"
    o = replay_options(dict(buffer_size=1000), num_envs=3, max_episode_steps=300)
    assert o["T"] == 333 and o["n_sampled_goal"] == 4 and o["goal_selection_strategy"] == "future" and o["seed"] is None
    assert replay_options(dict(buffer_size=8, n_sampled_goal=0, goal_selection_strategy="final", seed=7))["seed"] == 7
    for bad in [True, 5, dict(), dict(buffer_size=None), dict(buffer_size=0), dict(buffer_size=2.5),
                dict(buffer_size=True), dict(buffer_size=10, n_sampled_goal=-1), dict(buffer_size=10, n_sampled_goal=1.5),
                dict(buffer_size=10, goal_selection_strategy="random"), dict(buffer_size=10, seed=0.5),
                dict(buffer_size=10, size=3)]:
        with pytest.raises(ValueError):
            replay_options(bad)
    good = dict(buffer_size=8 * 300)
    for kw in [dict(task="so100_touch_cube"), dict(obs_type="so100_pixels_agent_pos"), dict(autoreset=False),
               dict(max_episode_steps=301), dict(num_envs=9)]:
        with pytest.raises(ValueError):
            replay_options(good, **{**dict(num_envs=8, task="so100_goal", obs_type="so100_state", autoreset=True,
                                           max_episode_steps=300), **kw})


def test_constructor_raises_before_any_device_work(monkeypatch):
    """every ValueError of replay=... comes before the library is loaded or a device touched"""
    from gym_so100 import SO100VecEnv, _native
    from gym_so100.sb3 import SO100SB3VecEnv

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "load", no_device)
    for kw in [dict(task="so100_cube_to_bin", replay=dict(buffer_size=1 << 20)),
               dict(task="so100_goal", obs_type="so100_pixels_agent_pos", replay=dict(buffer_size=1 << 20)),
               dict(task="so100_goal", autoreset=False, replay=dict(buffer_size=1 << 20)),
               dict(task="so100_goal", replay=dict(buffer_size=8 * 299)),                  # T < the GoalEnv's 300
               dict(task="so100_goal", max_episode_steps=6, replay=dict(buffer_size=8 * 5)),
               dict(task="so100_goal", replay=dict(buffer_size=1 << 20, bogus=1)),
               dict(task="so100_goal", replay=dict(buffer_size=1 << 20, n_sampled_goal=-2)),
               dict(task="so100_goal", replay=dict(buffer_size=1 << 20, goal_selection_strategy="past")),
               dict(task="so100_goal", replay=True)]:
        with pytest.raises(ValueError, match="replay"):
            SO100VecEnv(8, **kw)
    with pytest.raises(ValueError, match="replay"):
        SO100SB3VecEnv(8, task="so100_touch_cube", replay=dict(buffer_size=1 << 20))


# ---------------------------------------------------------------------- the restatement
def _row(e, t, width):
    """a row that encodes (env, push index)"""
    return np.float32(1000 * e + t) + np.arange(width, dtype=np.float32) / 16


@pytest.mark.parametrize("n,T,seed", [(1, 1, 0), (3, 4, 1), (5, 8, 2), (4, 13, 3)])
def test_ring_is_the_episode_list(n, T, seed):
    """random done / diverged / discard scripts: count + open_len <= T after every call, the valid interval holds
    exactly the transitions of the closed, non-evicted, non-erased episodes in their order, offsets and lengths name
    each one's episode, and the staged rows are the last observation"""
    rng = np.random.default_rng(seed)
    ref = her_ref.HerRef(n, T, 2)
    lists = [her_ref.EpisodeList(T) for _ in range(n)]
    age = np.zeros(n, int)                               # the open episode's length, capped at T as an env caps it
    for t in range(12 * T + 7):
        obs = np.stack([_row(e, t, 15) for e in range(n)])
        fin_obs = obs + 0.5
        goal = np.stack([_row(e, t, 3) for e in range(n)]) + 0.25
        term = rng.random(n) < 0.15
        trunc = (rng.random(n) < 0.1) | (age + 1 >= T)
        div = rng.random(n) < 0.05
        trunc |= div                                     # the step truncates what it flags as diverged
        disc = rng.random(n) < 0.03 if t % 3 == 0 else None
        act = np.stack([_row(e, t, 2) for e in range(n)])
        rew = -np.arange(n, dtype=np.float32) - t
        prev_obs, prev_goal = ref.stage_obs.copy(), ref.stage_goal.copy()
        ref.push(prev_obs, prev_goal, obs, fin_obs, goal, act, rew, term, trunc, div, disc)
        for e in range(n):
            erase = bool(div[e]) or (disc is not None and bool(disc[e]))
            lists[e].push((t, float(rew[e])), bool(term[e] or trunc[e]), erase)
            age[e] = 0 if (term[e] or trunc[e] or erase) else age[e] + 1
        if t % 11 == 5:                                  # a user reset of some envs
            mask = rng.random(n) < 0.4
            ref.discard(mask, obs + 7, goal + 7)
            for e in np.flatnonzero(mask):
                lists[e].discard()
                age[e] = 0
            assert (ref.stage_obs[mask] == (obs + 7)[mask]).all() and (ref.stage_obs[~mask] == obs[~mask]).all()
        else:
            assert (ref.stage_obs == obs).all() and (ref.stage_goal == goal).all()
        assert (ref.meta[1] + ref.meta[2] <= T).all() and (ref.meta >= 0).all() and (ref.meta[0] < T).all()
        for e in range(n):
            slots = ref.valid_slots(e)
            want = lists[e].valid()
            assert [float(ref.reward[s, e]) for s in slots] == [r for _, r in want]
            assert [int(ref.action[s, e, 0]) - 1000 * e for s in slots] == [tt for tt, _ in want]
            assert int(ref.meta[2, e]) == len(lists[e].open)
            k = 0
            for ep in lists[e].closed:                   # offsets count up from each episode's first slot
                first = slots[k]
                assert int(ref.length[first, e]) == len(ep)
                for j in range(len(ep)):
                    assert int(ref.offset[slots[k + j], e]) == j and (slots[k + j] - j) % T == first
                k += len(ep)
    assert sum(int(ref.meta[1, e]) for e in range(n)) > 0


def test_transition_pick_is_uniform():
    """10 valid transitions spread unevenly over 3 envs (7, 0 and 3 of T = 8; the second env's episode is still open),
    100,000 draws: each transition's frequency within 5 sigma of 1/10, sigma = sqrt(p (1 - p) / draws)"""
    T = 8
    ref = her_ref.HerRef(3, T, 1, seed=1234)
    z15, z3 = np.zeros((3, 15), np.float32), np.zeros((3, 3), np.float32)
    for t in range(7):
        done = np.array([t == 6, False, t in (0, 2)])    # env 0: one episode of 7; env 2: 1 + 2, then 4 open
        ref.push(z15, z3, z15, z15, z3, np.zeros((3, 1), np.float32), np.zeros(3, np.float32), done, ~done & False)
    assert ref.meta[1].tolist() == [7, 0, 3] and ref.meta[2].tolist() == [0, 7, 4]
    pre = ref.prefix()
    assert pre.tolist() == [7, 7, 10, 10]
    draws, total = 100_000, int(pre[3])
    hits = {}
    for i in range(draws):
        e, k = her_ref.pick(pre, total, her_ref.draw(ref.seed, 0, i, 0))
        hits[(e, k)] = hits.get((e, k), 0) + 1
    assert sorted(hits) == [(0, k) for k in range(7)] + [(2, k) for k in range(3)]
    p = 1 / total
    sigma = np.sqrt(p * (1 - p) / draws)
    for key, c in hits.items():
        assert abs(c / draws - p) <= 5 * sigma, (key, c)


def test_relabelled_share_and_goal_choice():
    """int(her_ratio * B) rows are relabelled; future picks from [offset, len), final len - 1, episode [0, len)"""
    assert [her_ref.n_relabelled(4, b) for b in (1, 5, 256, 1000)] == [0, 4, 204, 800]
    assert [her_ref.n_relabelled(0, b) for b in (1, 5, 256)] == [0, 0, 0]
    assert [her_ref.n_relabelled(1, b) for b in (1, 5, 256)] == [0, 2, 128]
    T = 8
    for strategy in (her_ref.FUTURE, her_ref.FINAL, her_ref.EPISODE):
        ref = her_ref.HerRef(2, T, 1, strategy=strategy, n_sampled_goal=4, seed=5)
        z15, z3 = np.zeros((2, 15), np.float32), np.zeros((2, 3), np.float32)
        for t in range(11):                              # env 0: episodes of 3 (it wraps); env 1: of 5
            done = np.array([t % 3 == 2, t % 5 == 4])
            ref.push(z15, z3, z15, z15, z3, np.zeros((2, 1), np.float32), np.zeros(2, np.float32), done, done & False)
        env, slot, gslot = ref.sample_indices(500, call=3)
        assert (gslot[400:] == -1).all() and (gslot[:400] >= 0).all() and (slot >= 0).all()
        seen_later = False
        for e, s, g in zip(env[:400], slot[:400], gslot[:400]):
            off = int(ref.offset[s, e])
            first = (s - off) % T
            ln = int(ref.length[first, e])
            j = (g - first) % T
            assert s in ref.valid_slots(e) and g in ref.valid_slots(e) and 0 <= j < ln
            if strategy == her_ref.FUTURE:
                assert j >= off
                seen_later |= j > off
            elif strategy == her_ref.FINAL:
                assert j == ln - 1
            else:
                seen_later |= j < off
        assert seen_later or strategy == her_ref.FINAL
        again = ref.sample_indices(500, call=3)
        assert all((a == b).all() for a, b in zip((env, slot, gslot), again))
        other = ref.sample_indices(500, call=4)
        assert (other[1] != slot).any()
