"""The running normaliser on the GPU (csrc/so100_norm.hip; include/so100.h so100_norm_update / so100_norm_apply /
so100_norm_return) against the float64 numpy restatement (tests/norm_ref.py): the moments and the merge
at the row counts where a reduction goes wrong, determinism and masks, the apply kernel, the return path, and
SO100VecEnv(normalize=...) / SO100SB3VecEnv(normalize=...) in closed loop.

Bars (derived, norm_ref.mean_bar / var_bar / apply_bar).  Statistics: |d mean| <= T n 2^-52 mean|x| and
|d var| <= T n 2^-51 mean(x^2) per column after T updates of n rows, the worst-case float64 summation bound of any order
doubled for the merge arithmetic (a float32 accumulator misses them by about 2^29); count exact.  Normalised values:
|y - y_ref| <= 2 (spacing32(max(|x|, |mean|)) / sqrt(var + eps) + spacing32(|y_ref|)), y_ref the restatement with its own
statistics; |y| <= clip bit for bit.  ret: T 2^-52 max|ret|, and exactly 0 after a done."""
import ctypes
import os

import numpy as np
import pytest

import norm_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

_ENV = {}


def _handle():
    """a small default env: the handle (device) the direct launches are made on"""
    if "bare" not in _ENV:
        from gym_so100 import SO100VecEnv
        _ENV["bare"] = SO100VecEnv(4, task="so100_touch_cube", device="cuda:0", autoreset=False)
    return _ENV["bare"]


def _limits():
    from gym_so100 import _native
    return _native.norm_limits()


def _sizes():
    rows, groups = _limits()
    return [1, 5, 63, 64, 65, 257, rows - 1, rows, rows + 1]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _fresh_stats():
    s = np.zeros((3, 32), dtype=np.float64)
    s[1], s[2] = 1.0, norm_ref.COUNT0
    return _dev(s)


def _work(n):
    env = _handle()
    return torch.zeros(env.lib.so100_norm_work_bytes(n) // 8, dtype=torch.float64, device="cuda")


def _update(sources, n, stats, mask=None, work=None):
    """one so100_norm_update over device tensors: sources = [(tensor [n, stride], offset, dim)]"""
    from gym_so100 import _native
    env = _handle()
    nm = _native.SO100Norm([(t.data_ptr(), t.shape[1], off, dim, None, dim) for t, off, dim in sources])
    work = _work(n) if work is None else work
    rc = env.lib.so100_norm_update(env._handle, ctypes.byref(nm), n, _native.ptr(mask), _native.ptr(stats),
                                   _native.ptr(work), env._stream())
    assert rc == 0, env.lib.so100_last_error()
    torch.cuda.synchronize()
    return stats.cpu().numpy()


def _apply(sources, n, stats, mask=None, fill=None, **kw):
    """one so100_norm_apply -> the outputs [n, dim] as numpy (float32); rows outside the mask keep `fill`"""
    from gym_so100 import _native
    env = _handle()
    outs = [torch.full((n, dim), np.nan if fill is None else fill, dtype=torch.float32, device="cuda")
            for _, _, dim in sources]
    nm = _native.SO100Norm([(t.data_ptr(), t.shape[1], off, dim, o.data_ptr(), dim)
                            for (t, off, dim), o in zip(sources, outs)], **kw)
    rc = env.lib.so100_norm_apply(env._handle, ctypes.byref(nm), n, _native.ptr(mask), _native.ptr(stats), env._stream())
    assert rc == 0, env.lib.so100_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _awkward(rng, n):
    """[n, 15] float32 of awkward conditioning: column 0 mean 5 / sd 1e-3, column 1 constant, column 2 spanning +-10,
    column 3 a large offset, the rest unit normals of growing scale"""
    x = rng.standard_normal((n, 15)) * np.linspace(0.1, 3.0, 15)
    x[:, 0] = 5.0 + 1e-3 * rng.standard_normal(n)
    x[:, 1] = 0.37
    x[:, 2] = rng.uniform(-10, 10, n)
    x[:, 3] = -300.0 + rng.standard_normal(n)
    return x.astype(np.float32)


def _check_stats(dev, rms, c0, seen, what=""):
    """columns [c0, c0 + dim) of the device statistics against the restatement, within bar 1; count exact"""
    d = rms.mean.shape[0]
    x_all = np.concatenate(seen).astype(np.float64)
    em, ev = np.abs(dev[0, c0:c0 + d] - rms.mean), np.abs(dev[1, c0:c0 + d] - rms.var)
    bm, bv = norm_ref.mean_bar(x_all), norm_ref.var_bar(x_all)
    print(f"{what} n={x_all.shape[0]} T={rms.updates}: max |d mean| / bar {np.max(em / np.maximum(bm, 1e-300)):.3g}, "
          f"max |d var| / bar {np.max(ev / np.maximum(bv, 1e-300)):.3g}")
    assert (em <= bm).all(), (what, em, bm)
    assert (ev <= bv).all(), (what, ev, bv)
    assert (dev[2, c0:c0 + d] == rms.count).all(), (what, dev[2, c0:c0 + d], rms.count)


# ---------------------------------------------------------------------- moments and merge
def test_moments_and_merge_match_restatement():
    """every size: two updates of [n,15] (the second from a non-zero shift), then a dim of 1 out of the middle of the row"""
    rng = np.random.default_rng(10)
    for n in _sizes():
        x1, x2 = _awkward(rng, n), _awkward(rng, n)
        stats, rms, seen = _fresh_stats(), norm_ref.RunningMeanStd(15), []
        for x in (x1, x2):
            dev = _update([(_dev(x), 0, 15)], n, stats)
            rms.update(x)
            seen.append(x)
            _check_stats(dev, rms, 0, seen, "obs")
        assert (dev[0, 15:] == 0).all() and (dev[1, 15:] == 1).all() and (dev[2, 15:] == norm_ref.COUNT0).all()
        if n == 1:                                     # one row: the batch variance is exactly 0
            one = norm_ref.RunningMeanStd(15)
            one.update_from_moments(x1[0].astype(np.float64), np.zeros(15), 1)
            first = _update([(_dev(x1), 0, 15)], 1, _fresh_stats())
            assert np.array_equal(first[1, :15], one.var) and np.array_equal(first[0, :15], one.mean)
        stats1, rms1 = _fresh_stats(), norm_ref.RunningMeanStd(1)
        dev = _update([(_dev(x1), 3, 1)], n, stats1)
        rms1.update(x1[:, 3:4])
        _check_stats(dev, rms1, 0, [x1[:, 3:4]], "dim 1")


def test_three_sources_one_call():
    """the GoalEnv's call: strides 15, 15 and 3, the second source from column offset 9"""
    rng = np.random.default_rng(11)
    for n in (5, 65, 257):
        a, b, g = _awkward(rng, n), _awkward(rng, n), (rng.standard_normal((n, 3)) * 0.05 + 0.3).astype(np.float32)
        stats = _fresh_stats()
        ref = [norm_ref.RunningMeanStd(15), norm_ref.RunningMeanStd(6), norm_ref.RunningMeanStd(3)]
        seen = [[], [], []]
        for _ in range(2):
            dev = _update([(_dev(a), 0, 15), (_dev(b), 9, 6), (_dev(g), 0, 3)], n, stats)
            for r, s, x in zip(ref, seen, (a, b[:, 9:15], g)):
                r.update(x)
                s.append(x)
        for r, s, c0 in zip(ref, seen, (0, 15, 21)):
            _check_stats(dev, r, c0, s, f"source at column {c0}")
        ys = _apply([(_dev(a), 0, 15), (_dev(b), 9, 6), (_dev(g), 0, 3)], n, stats)
        for y, r, x in zip(ys, ref, (a, b[:, 9:15], g)):
            y_ref = norm_ref.normalize(x, r)
            assert (np.abs(y - y_ref) <= norm_ref.apply_bar(x, r, y_ref)).all()


def test_grid_cap_engages_the_long_row_loop():
    """past rows_per_group * max_groups rows every workgroup's range grows: dims 3 and 1, under 1 MB of input"""
    rows, groups = _limits()
    rng = np.random.default_rng(12)
    env = _handle()
    for n in (rows * groups, rows * groups + 1, rows * groups + rows + 7):
        assert env.lib.so100_norm_work_bytes(n) == groups * 3 * 32 * 8
        x = (rng.standard_normal((n, 3)) * [1.0, 1e-3, 4.0] + [0.0, 5.0, -2.0]).astype(np.float32)
        assert x.nbytes < 1 << 20
        stats, rms = _fresh_stats(), norm_ref.RunningMeanStd(3)
        dev = _update([(_dev(x), 0, 3)], n, stats)
        rms.update(x)
        _check_stats(dev, rms, 0, [x], "cap")
        stats1, rms1 = _fresh_stats(), norm_ref.RunningMeanStd(1)
        dev = _update([(_dev(x), 1, 1)], n, stats1)
        rms1.update(x[:, 1:2])
        _check_stats(dev, rms1, 0, [x[:, 1:2]], "cap dim 1")


# ---------------------------------------------------------------------- determinism and masks
def test_determinism_and_masks():
    rows, groups = _limits()
    rng = np.random.default_rng(13)
    for n in (65, rows + 1, 4 * rows + 3):
        x = _dev(_awkward(rng, n))
        start = _update([(x, 0, 15)], n, _fresh_stats())          # a state with a non-zero shift
        a = _update([(x, 0, 15)], n, _dev(start))
        b = _update([(x, 0, 15)], n, _dev(start), work=torch.full_like(_work(n), 1e300))   # (a dirty workspace)
        assert a.tobytes() == b.tobytes()
        m = rng.random(n) < 0.4
        m[0] = True
        dev = _update([(x, 0, 15)], n, _dev(start), mask=_dev(m.astype(np.uint8)))
        rms = norm_ref.RunningMeanStd(15)
        rms.mean, rms.var, rms.count = start[0, :15].copy(), start[1, :15].copy(), start[2, 0]
        xm = x.cpu().numpy()[m]
        rms.update(xm)
        em, ev = np.abs(dev[0, :15] - rms.mean), np.abs(dev[1, :15] - rms.var)
        assert (em <= norm_ref.mean_bar(xm)).all() and (ev <= norm_ref.var_bar(xm)).all()
        assert (dev[2, :15] == rms.count).all()
        none = _update([(x, 0, 15)], n, _dev(start), mask=torch.zeros(n, dtype=torch.uint8, device="cuda"))
        assert none.tobytes() == start.tobytes()


# ---------------------------------------------------------------------- apply
def test_apply_clip_mask_and_inverse():
    rng = np.random.default_rng(14)
    for n in (1, 65, 257):
        x = _awkward(rng, n)
        rms = norm_ref.RunningMeanStd(15)
        rms.update(_awkward(rng, 300))
        rms.update(_awkward(rng, 300))
        stats = np.zeros((3, 32))
        stats[0, :15], stats[1, :15], stats[2, :15] = rms.mean, rms.var, rms.count
        x[:, 4] *= 40.0                                    # a column that clips
        x[n // 2, 5] = 1e30
        for clip in (10.0, 2.5):
            y, = _apply([(_dev(x), 0, 15)], n, _dev(stats), clip=clip)
            y_ref = norm_ref.normalize(x, rms, clip=clip)
            bar = norm_ref.apply_bar(x, rms, y_ref)
            assert y.dtype == np.float32 and (np.abs(y - y_ref) <= bar).all()
            assert (np.abs(y) <= np.float32(clip)).all()
            raw = (x.astype(np.float64) - rms.mean) / np.sqrt(rms.var + 1e-8)
            far = np.abs(raw) > clip + norm_ref.apply_bar(x, rms, raw)
            assert far.any() and (y[far] == np.sign(raw[far]).astype(np.float32) * np.float32(clip)).all()
        # the inverse: back to x within the same bar scaled by sqrt(var + eps), where nothing clipped
        y, = _apply([(_dev(x), 0, 15)], n, _dev(stats), clip=10.0)
        back, = _apply([(_dev(y), 0, 15)], n, _dev(stats), flags=1)
        inside = np.abs(raw) < 10.0
        y_ref = norm_ref.normalize(x, rms)
        bar = norm_ref.apply_bar(x, rms, y_ref) * np.sqrt(rms.var + 1e-8)
        assert inside.sum() > 10 * n and (np.abs(back.astype(np.float64) - x)[inside] <= bar[inside]).all()
        # a row mask: only the masked rows are written
        m = rng.random(n) < 0.5
        ym, = _apply([(_dev(x), 0, 15)], n, _dev(stats), mask=_dev(m.astype(np.uint8)), fill=77.0)
        assert np.array_equal(ym[m], y[m]) and (ym[~m] == 77.0).all()


# ---------------------------------------------------------------------- the return path
def test_return_path_twelve_steps():
    from gym_so100 import _native
    env = _handle()
    rng = np.random.default_rng(15)
    for n in (1, 65, 257):
        ref = norm_ref.VecNormalizeRef({}, n, obs=False, reward=True, clip_reward=3.0, gamma=0.9)
        ret = torch.zeros(n, dtype=torch.float64, device="cuda")
        stats, work = _fresh_stats(), _work(n)
        out = torch.zeros(n, dtype=torch.float32, device="cuda")
        args = _native.SO100NormRet(flags=3, gamma=0.9, clip=3.0)
        P = _native.ptr
        for t in range(12):
            reward = (rng.standard_normal(n) * 3.0 - 1.0).astype(np.float32)
            term, trunc = rng.random(n) < 0.15, rng.random(n) < 0.1
            if t == 5:
                term[:] = trunc[:] = False
            r, tm, tr = _dev(reward), _dev(term), _dev(trunc)
            rc = env.lib.so100_norm_return(env._handle, ctypes.byref(args), n, P(r), P(tm), P(tr), P(ret), P(stats),
                                           P(work), P(out), env._stream())
            assert rc == 0, env.lib.so100_last_error()
            torch.cuda.synchronize()
            _, r_ref, _ = ref.step({}, reward, term, trunc)
            got, dstats = ret.cpu().numpy(), stats.cpu().numpy()
            done = term | trunc
            assert (got[done] == 0.0).all() and (ref.ret[done] == 0.0).all()
            assert (np.abs(got - ref.ret) <= (t + 1) * 2.0 ** -52 * max(np.abs(ref.ret).max(), 1e-300)).all()
            g_all = np.concatenate(ref.ret_seen)
            assert abs(dstats[0, 0] - ref.ret_rms.mean[0]) <= norm_ref.mean_bar(g_all)[0]
            assert abs(dstats[1, 0] - ref.ret_rms.var[0]) <= norm_ref.var_bar(g_all)[0]
            assert dstats[2, 0] == ref.ret_rms.count
            y = out.cpu().numpy()
            bar = 2 * (norm_ref.spacing32(reward) / np.sqrt(ref.ret_rms.var[0] + 1e-8) + norm_ref.spacing32(r_ref))
            assert (np.abs(y - r_ref) <= bar).all() and (np.abs(y) <= np.float32(3.0)).all()
        # frozen: no update, the reward still normalised, ret still zeroed at done
        frozen = _native.SO100NormRet(flags=2, gamma=0.9, clip=3.0)
        before, ret_before = stats.cpu().numpy().tobytes(), ret.cpu().numpy()
        rc = env.lib.so100_norm_return(env._handle, ctypes.byref(frozen), n, P(r), P(tm), None, P(ret), P(stats), None,
                                       P(out), env._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert stats.cpu().numpy().tobytes() == before
        assert np.array_equal(ret.cpu().numpy(), np.where(term, 0.0, ret_before))


def test_refusals_that_need_an_env():
    from gym_so100 import _native
    env = _handle()
    x = torch.zeros(8, 15, device="cuda")
    stats, work = _fresh_stats(), _work(8)
    P = _native.ptr
    good = [(x.data_ptr(), 15, 0, 15, x.data_ptr(), 15)]
    for nm, st, wk, text in ((_native.SO100Norm([(None, 15, 0, 15, None, 15)]), stats, work, "NULL source"),
                             (_native.SO100Norm(good), None, work, "NULL stats"),
                             (_native.SO100Norm(good), stats, None, "NULL work")):
        rc = env.lib.so100_norm_update(env._handle, ctypes.byref(nm), 8, None, P(st), P(wk), env._stream())
        assert rc != 0 and text.encode() in env.lib.so100_last_error()
    nm = _native.SO100Norm([(x.data_ptr(), 15, 0, 15, None, 15)])
    assert env.lib.so100_norm_apply(env._handle, ctypes.byref(nm), 8, None, P(stats), env._stream()) != 0
    assert b"NULL output" in env.lib.so100_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(stats.cpu().numpy(), _fresh_stats().cpu().numpy())      # nothing was written
    assert env.lib.so100_norm_update(env._handle, ctypes.byref(_native.SO100Norm(good)), 0, None, P(stats), P(work),
                                     env._stream()) == 0                         # no rows: nothing launched


# ---------------------------------------------------------------------- closed loop through SO100VecEnv
KEYS = {False: {"obs": 15}, True: {"observation": 15, "achieved_goal": 3, "desired_goal": 3}}


def _raw(env):
    if env.is_goal:
        return {"observation": env.obs.cpu().numpy(), "achieved_goal": env.achieved_goal.cpu().numpy(),
                "desired_goal": env.desired_goal.cpu().numpy()}
    return {"obs": env.obs.cpu().numpy()}


def _returned(env, obs):
    return {k: v.cpu().numpy() for k, v in obs.items()} if env.is_goal else {"obs": obs.cpu().numpy()}


def _check_obs(got, want, raw, ref, what):
    for k in want:
        bar = norm_ref.apply_bar(raw[k], ref.rms[k], want[k], ref.epsilon)
        assert got[k].dtype == np.float32 and (np.abs(got[k] - want[k]) <= bar).all(), (what, k)
        assert (np.abs(got[k]) <= np.float32(ref.clip_obs)).all()


def _check_rms(env, ref, what):
    rms = env.obs_rms
    for k, r in ref.rms.items():
        x_all = np.concatenate(ref.seen[k])
        assert (np.abs(rms[k].mean - r.mean) <= norm_ref.mean_bar(x_all)).all(), (what, k)
        assert (np.abs(rms[k].var - r.var) <= norm_ref.var_bar(x_all)).all(), (what, k)
        assert rms[k].count == r.count, (what, k)


@pytest.mark.parametrize("task,n", [("so100_touch_cube", 65), ("so100_goal", 5)])
def test_closed_loop_matches_replayed_restatement(task, n):
    from gym_so100 import SO100VecEnv
    opts = dict(obs=True, reward=True, clip_obs=4.0, clip_reward=5.0, gamma=0.95)
    kw = dict(task=task, device="cuda:0", seed=7, max_episode_steps=6, autoreset=True)
    env = SO100VecEnv(n, normalize=opts, **kw)
    twin = SO100VecEnv(n, normalize=opts, **kw)
    goal = task == "so100_goal"
    ref = norm_ref.VecNormalizeRef(KEYS[goal], n, **opts)
    obs, _ = env.reset()
    tobs, _ = twin.reset()
    raw = _raw(env)
    _check_obs(_returned(env, obs), ref.reset(raw), raw, ref, "reset")
    g = torch.Generator(device="cuda").manual_seed(5)
    dones = 0
    for t in range(20):
        a = torch.rand(n, 6, device="cuda", generator=g) * 2 - 1
        obs, rew, term, trunc, info = env.step(a)
        tobs, trew, _, _, tinfo = twin.step(a)
        raw, done = _raw(env), (term | trunc).cpu().numpy()
        dones += int(done.sum())
        assert rew.data_ptr() == env.reward_norm.data_ptr() and env.reward.data_ptr() != rew.data_ptr()
        final_raw = env.final_obs.cpu().numpy()
        want, r_want, fin = ref.step(raw, env.reward.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(),
                                     final={"observation" if goal else "obs": final_raw})
        _check_obs(_returned(env, obs), want, raw, ref, f"step {t}")
        _check_rms(env, ref, f"step {t}")
        # the final observation: normalised with the statistics as the step left them, and not part of them (the
        # statistics above match a replay that never saw it)
        fk = "observation" if goal else "obs"
        fgot = info["final_observation"].cpu().numpy()
        fbar = norm_ref.apply_bar(final_raw, ref.rms[fk], fin[fk], ref.epsilon)
        assert (np.abs(fgot - fin[fk])[done] <= fbar[done]).all()
        # the return path
        rr = env.ret_rms
        g_all = np.concatenate(ref.ret_seen)
        assert abs(rr.mean - ref.ret_rms.mean[0]) <= norm_ref.mean_bar(g_all)[0]
        assert abs(rr.var - ref.ret_rms.var[0]) <= norm_ref.var_bar(g_all)[0] and rr.count == ref.ret_rms.count
        reward = env.reward.cpu().numpy()
        rbar = 2 * (norm_ref.spacing32(reward) / np.sqrt(ref.ret_rms.var[0] + 1e-8) + norm_ref.spacing32(r_want))
        assert (np.abs(rew.cpu().numpy() - r_want) <= rbar).all()
        ret = env.get_state()["ret"].cpu().numpy()
        assert (ret[done] == 0).all() and (np.abs(ret - ref.ret) <= (t + 1) * 2.0 ** -52 * max(np.abs(ref.ret).max(), 1e-300)).all()
        # twins with the same seed stay bit-equal
        for k, v in _returned(env, obs).items():
            assert v.tobytes() == _returned(twin, tobs)[k].tobytes()
        assert rew.cpu().numpy().tobytes() == trew.cpu().numpy().tobytes()
    assert dones >= 2 * n                                # resets occurred
    a_state, b_state = env.normalize_state(), twin.normalize_state()
    assert all(a_state[k].tobytes() == b_state[k].tobytes() for k in a_state)
    # training off freezes the statistics bit for bit; the observation is still normalised
    env.training = False
    assert env.training is False
    for _ in range(3):
        obs, *_ = env.step(torch.rand(n, 6, device="cuda", generator=g) * 2 - 1)
    env.reset()
    c_state = env.normalize_state()
    assert all(a_state[k].tobytes() == c_state[k].tobytes() for k in a_state)
    ref.training = False
    raw = _raw(env)
    _check_obs(_returned(env, env._observation()), ref.reset(raw), raw, ref, "frozen")
    env.close(), twin.close()


def test_normalize_none_is_the_parents_env():
    from gym_so100 import SO100VecEnv
    kw = dict(task="so100_touch_cube", device="cuda:0", seed=7, max_episode_steps=6)
    plain, on = SO100VecEnv(5, **kw), SO100VecEnv(5, normalize=True, **kw)
    assert plain._pre is False and plain._norm is None and on._pre is True
    for name in ("obs_norm", "reward_norm", "final_obs_norm", "achieved_goal_norm", "desired_goal_norm", "agent_pos_norm"):
        assert getattr(plain, name) is None, name
    assert not hasattr(plain, "obs_rms") and "ret" not in plain.get_state()
    with pytest.raises(ValueError):
        plain.normalize_obs(plain.obs)
    o0, _ = plain.reset()
    o1, _ = on.reset()
    assert o0.data_ptr() == plain.obs.data_ptr() and o1.data_ptr() == on.obs_norm.data_ptr()
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(8):
        a = torch.rand(5, 6, device="cuda", generator=g) * 2 - 1
        o0, r0, *_ = plain.step(a)
        o1, r1, *_ = on.step(a)
        assert o0.data_ptr() == plain.obs.data_ptr() and r0.data_ptr() == plain.reward.data_ptr()
        assert r1.data_ptr() == on.reward.data_ptr()                   # reward off: the raw reward
        # the physics does not see the option: raw outputs equal bit for bit
        assert torch.equal(plain.obs, on.obs) and torch.equal(plain.reward, on.reward)
        assert torch.equal(plain.final_obs, on.final_obs) and torch.equal(plain.qpos, on.qpos)
    plain.actions.copy_(a), on.actions.copy_(a)
    plain.step_async_raw(), on.step_async_raw()                        # the raw route carries the launches too
    rms = on.obs_rms["obs"]
    assert abs(rms.count - (norm_ref.COUNT0 + 5 * 10)) < 1e-9 and torch.equal(plain.obs, on.obs)
    plain.close(), on.close()


# ---------------------------------------------------------------------- state hand-off and shards
def test_state_hand_off_and_checkpoint_round_trip(tmp_path):
    from gym_so100 import SO100VecEnv
    kw = dict(task="so100_touch_cube", device="cuda:0", seed=3, max_episode_steps=5, normalize=dict(reward=True))
    a, b = SO100VecEnv(9, **kw), SO100VecEnv(9, **kw)
    a.reset(), b.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(7):
        a.step(torch.rand(9, 6, device="cuda", generator=g) * 2 - 1)
    state = a.normalize_state()
    path = os.path.join(tmp_path, "norm.npz")
    np.savez(path, **state)
    with np.load(path) as z:
        loaded = {k: z[k] for k in z.files}
    assert set(loaded) == set(state) and all(loaded[k].tobytes() == state[k].tobytes() for k in state)
    assert all(v.dtype in (np.float64, np.bool_) for v in state.values())
    b.set_normalize_state(loaded)
    after = b.normalize_state()
    assert all(after[k].tobytes() == state[k].tobytes() for k in state)
    st = a.get_state()
    b.set_state(st["qpos"], st["qvel"], st["qacc_warmstart"], st["elapsed"], st["episode"], ret=st["ret"])
    act = torch.rand(9, 6, device="cuda", generator=g) * 2 - 1
    oa, ra, *_ = a.step(act)
    ob, rb, *_ = b.step(act)
    assert oa.cpu().numpy().tobytes() == ob.cpu().numpy().tobytes()
    assert ra.cpu().numpy().tobytes() == rb.cpu().numpy().tobytes()
    # normalize_obs / unnormalize_obs on device tensors, with the env's statistics
    x = a.obs.clone()
    y = a.normalize_obs(x)
    assert y.is_cuda and y.dtype == torch.float32 and torch.equal(y, a.obs_norm)
    rms = a.obs_rms["obs"]
    ref = norm_ref.RunningMeanStd(15)
    ref.mean, ref.var = rms.mean, rms.var
    y_ref = norm_ref.normalize(x.cpu().numpy(), ref)
    back = a.unnormalize_obs(y).cpu().numpy().astype(np.float64)
    bar = norm_ref.apply_bar(x.cpu().numpy(), ref, y_ref) * np.sqrt(ref.var + 1e-8)
    inside = np.abs(y_ref) < 10.0
    assert (np.abs(back - x.cpu().numpy())[inside] <= bar[inside]).all()
    a.close(), b.close()


def test_two_shards_merge_to_the_whole():
    from gym_so100 import SO100VecEnv, merge_normalize_states
    kw = dict(task="so100_touch_cube", device="cuda:0", seed=11, max_episode_steps=6, normalize=True)
    whole = SO100VecEnv(65, **kw)
    lo, hi = SO100VecEnv(32, env_offset=0, **kw), SO100VecEnv(33, env_offset=32, **kw)
    seen = []
    for e in (whole, lo, hi):
        e.reset()
    seen.append(whole.obs.cpu().numpy())
    g = torch.Generator(device="cuda").manual_seed(4)
    for _ in range(20):
        a = torch.rand(65, 6, device="cuda", generator=g) * 2 - 1
        whole.step(a), lo.step(a[:32]), hi.step(a[32:])
        seen.append(whole.obs.cpu().numpy())
    assert torch.equal(whole.obs, torch.cat([lo.obs, hi.obs]))         # the shards are the whole's envs
    merged = merge_normalize_states([lo.normalize_state(), hi.normalize_state()])
    want = whole.normalize_state()
    x_all = np.concatenate(seen)
    assert (np.abs(merged["obs.mean"] - want["obs.mean"]) <= norm_ref.mean_bar(x_all)).all()
    assert (np.abs(merged["obs.var"] - want["obs.var"]) <= norm_ref.var_bar(x_all)).all()
    assert float(merged["obs.count"]) == float(want["obs.count"])
    for e in (whole, lo, hi):
        e.close()


# ---------------------------------------------------------------------- the SB3 adapter
def test_sb3_adapter_normalizes(tmp_path):
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 6
    train = SO100SB3VecEnv(n, task="so100_touch_cube", seed=3, max_episode_steps=4, normalize=dict(reward=True))
    ev = SO100SB3VecEnv(n, task="so100_touch_cube", seed=3, max_episode_steps=4, normalize=True)
    assert train.norm_reward is True and ev.norm_reward is False and train.training is True
    obs = train.reset()
    assert obs.dtype == np.float32 and np.array_equal(obs, train.venv.obs_norm.cpu().numpy())
    assert np.array_equal(train.get_original_obs(), train.venv.obs.cpu().numpy())
    rng = np.random.default_rng(0)
    terminal = 0
    for _ in range(9):
        obs, rew, dones, infos = train.step(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        v = train.venv
        assert obs.dtype == np.float32 and np.array_equal(obs, v.obs_norm.cpu().numpy())
        assert rew.dtype == np.float32 and np.array_equal(rew, v.reward_norm.cpu().numpy())
        assert np.array_equal(train.get_original_obs(), v.obs.cpu().numpy())
        assert np.array_equal(train.get_original_reward(), v.reward.cpu().numpy())
        for i in np.flatnonzero(dones):
            terminal += 1
            assert np.array_equal(infos[i]["terminal_observation"], v.final_obs_norm[i].cpu().numpy())
            want = train.normalize_obs(v.final_obs[i].cpu().numpy())
            assert np.array_equal(infos[i]["terminal_observation"], want)
    assert terminal >= n
    # the scripts' line: the eval env takes the training env's statistics by assignment
    ev.reset()
    ev.obs_rms = train.obs_rms
    ev.training = False
    assert ev.training is False
    # any object with mean / var / count is taken (SB3's own RunningMeanStd); anything else is refused
    import types
    taken = train.obs_rms
    ev.obs_rms = types.SimpleNamespace(mean=taken.mean, var=taken.var, count=taken.count)
    assert np.array_equal(ev.obs_rms.mean, taken.mean) and ev.obs_rms.count == taken.count
    with pytest.raises(ValueError):
        ev.obs_rms = 3.0
    raw = train.get_original_obs()
    ya, yb = train.normalize_obs(raw), ev.normalize_obs(raw)
    assert ya.dtype == np.float32 and np.array_equal(ya, yb) and not np.array_equal(ya, raw)
    frozen = ev.venv.normalize_state()
    ev.step(np.zeros((n, 6), np.float32))
    assert all(frozen[k].tobytes() == v2.tobytes() for k, v2 in ev.venv.normalize_state().items())
    x = train.unnormalize_obs(ya)
    inside = np.abs(ya) < 10.0
    assert inside.mean() > 0.9 and np.allclose(x[inside], raw[inside], rtol=1e-5, atol=1e-5)
    # save / load_stats: bit exact
    path = os.path.join(tmp_path, "vecnormalize.npz")
    train.save(path)
    fresh = SO100SB3VecEnv(n, task="so100_touch_cube", seed=9, normalize=dict(reward=True))
    fresh.load_stats(path)
    s0, s1 = train.venv.normalize_state(), fresh.venv.normalize_state()
    assert all(s0[k].tobytes() == s1[k].tobytes() for k in s0)
    assert np.array_equal(fresh.obs_rms.mean, train.obs_rms.mean) and fresh.ret_rms.var == train.ret_rms.var
    for e in (train, ev, fresh):
        e.close()


def test_sb3_goal_env_terminal_observation_is_normalized():
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 4
    env = SO100SB3VecEnv(n, task="so100_goal", seed=2, max_episode_steps=3, normalize=True)
    obs = env.reset()
    assert set(obs) == {"observation", "achieved_goal", "desired_goal"} and set(env.obs_rms) == set(obs)
    seen = 0
    for _ in range(4):
        prev_goal = env.venv.desired_goal.clone()
        obs, rew, dones, infos = env.step(np.zeros((n, 6), np.float32))
        v = env.venv
        assert np.array_equal(obs["achieved_goal"], v.achieved_goal_norm.cpu().numpy())
        assert np.array_equal(rew, v.reward.cpu().numpy())                 # reward off
        for i in np.flatnonzero(dones):
            seen += 1
            want = v.normalize_obs({"observation": v.final_obs[i:i + 1], "achieved_goal": v.final_obs[i:i + 1, 0:3],
                                    "desired_goal": prev_goal[i:i + 1]})
            for k in want:
                assert np.array_equal(infos[i]["terminal_observation"][k], want[k][0].cpu().numpy()), k
    assert seen >= n
    env.close()


def test_sb3_pixels_only_agent_pos_changes():
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 3
    kw = dict(task="so100_touch_cube", seed=5, max_episode_steps=3, obs_type="so100_pixels_agent_pos",
              observation_width=64, observation_height=48)
    on, off = SO100SB3VecEnv(n, normalize=True, **kw), SO100SB3VecEnv(n, **kw)
    a, b = on.reset(), off.reset()
    assert set(on.obs_rms) == {"agent_pos"}
    rng = np.random.default_rng(3)
    terminal = 0
    for _ in range(5):
        assert a["pixels"].dtype == np.uint8 and a["pixels"].tobytes() == b["pixels"].tobytes()
        assert np.array_equal(a["agent_pos"], on.venv.agent_pos_norm.cpu().numpy())
        assert np.array_equal(on.get_original_obs()["agent_pos"], b["agent_pos"])
        assert not np.array_equal(a["agent_pos"], b["agent_pos"])
        act = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        a, ra, da, ia = on.step(act)
        b, rb, db, ib = off.step(act)
        assert np.array_equal(ra, rb) and np.array_equal(da, db)
        for i in np.flatnonzero(da):
            terminal += 1
            ta, tb = ia[i]["terminal_observation"], ib[i]["terminal_observation"]
            assert ta["pixels"].tobytes() == tb["pixels"].tobytes()
            assert np.array_equal(ta["agent_pos"], on.normalize_obs({"agent_pos": tb["agent_pos"]})["agent_pos"])
    assert terminal >= n
    on.close(), off.close()
