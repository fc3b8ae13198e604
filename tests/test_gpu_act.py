"""Per-episode physical randomisation and the actuation-latency model on the GPU (csrc/so100_dr.hip, csrc/so100_act.hip,
include/so100.h so100_dr_sample / so100_actuate): both kernels against the numpy restatement
(tests/act_ref.py), masking, sharding and determinism of the draw, the refusals that need an env, and
SO100VecEnv(domain_randomization=dict(per_episode=, actuation=)) / SO100SB3VecEnv in closed loop.

Bars.  Delays, `head` and the ring's command slots: exact.  Drawn real values: 4 float32 ulp at their magnitude (two
roundings and a clamp, with or without contraction).  Applied actions: bit for bit where the model claims it (alpha = 1,
r >= 2, values that descend from `hold` aside), else 4 F + 1e-6 against the float64 restatement, F the float32
restatement's own floor over these very inputs (act_ref.F_ACT, measured by tests/test_act_cpu.py).
The sizes cross a partial wave (1, 5), a workgroup of 32 envs and a wave (65) and one past a multiple of 64 (257)."""
import ctypes

import numpy as np
import pytest

import act_ref
import ee_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 65, 257]
BAR = 4 * act_ref.F_ACT + 1e-6
RANGES = dict(mass=(0.8, 1.2), friction=(0.6, 1.4), delay=(0, 7), smoothing=(0.3, 1.0), rate=(0.05, 2.0))
_ENVS, _REF = {}, {}


def _env(n, **kw):
    from gym_so100 import SO100VecEnv
    kw.setdefault("autoreset", False)
    return SO100VecEnv(n, task="so100_touch_cube", device="cuda:0", **kw)


def _bare(n, offset=0):
    """a default env, kept per (n, offset): the handle the direct launches below are made on"""
    if (n, offset) not in _ENVS:
        _ENVS[(n, offset)] = _env(n, env_offset=offset)
    return _ENVS[(n, offset)]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ulp_ok(dev, ref64, ulps=4):
    """|dev - ref| <= ulps float32 spacings at the reference's magnitude"""
    return np.abs(dev.astype(np.float64) - ref64) <= ulps * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def _sample(env, ranges, episode=None, mask_a=None, mask_b=None, dr=True, act=True, fill=7.0):
    """one so100_dr_sample launch into tensors filled with `fill` -> (rc, dr_params, act_params) as numpy"""
    from gym_so100 import _native
    P = _native.ptr
    n = env.num_envs
    d = torch.full((n, 4), fill, dtype=torch.float32, device="cuda")
    a = torch.full((n, 4), fill, dtype=torch.float32, device="cuda")
    ep = None if episode is None else _dev(np.asarray(episode, np.int32))
    ma = None if mask_a is None else _dev(np.asarray(mask_a, np.uint8))
    mb = None if mask_b is None else _dev(np.asarray(mask_b, np.uint8))
    rc = env.lib.so100_dr_sample(env._handle, ctypes.byref(ranges), P(ep), P(ma), P(mb), P(d) if dr else None,
                                 P(a) if act else None, env._stream())
    torch.cuda.synchronize()
    return rc, d.cpu().numpy(), a.cpu().numpy()


def _check_rows(dr, act, seed, ids, episode, rows=None, ranges=RANGES):
    """the drawn columns of rows `rows` against the float64 restatement: delays exact, reals within 4 ulp"""
    rdr, ract = act_ref.sample(seed, ids, episode, **ranges)
    rows = np.arange(len(ids)) if rows is None else rows
    if dr is not None:
        assert _ulp_ok(dr[rows, :2], rdr[rows]).all()
    if act is not None:
        assert np.array_equal(act[rows, 0], ract[rows, 0])
        assert _ulp_ok(act[rows, 1:3], ract[rows, 1:3]).all() and (act[rows, 3] == 0).all()


# ---------------------------------------------------------------------- so100_dr_sample
@pytest.mark.parametrize("n", SIZES)
def test_dr_sample_matches_restatement(n):
    from gym_so100 import _native
    env = _bare(n)
    r = _native.SO100DrRanges(seed=9, **RANGES)
    ep = (np.arange(n) * 7) % 5
    rc, dr, act = _sample(env, r, ep)
    assert rc == 0
    _check_rows(dr, act, 9, np.arange(n), ep)
    assert (dr[:, 2:] == 7.0).all()                      # the sigma and the spare column are left as they are
    rc, dr0, act0 = _sample(env, r, None)                # a NULL episode is episode 0
    _check_rows(dr0, act0, 9, np.arange(n), None)
    # two launches give equal bytes
    rc, dr2, act2 = _sample(env, r, ep)
    assert dr2.tobytes() == dr.tobytes() and act2.tobytes() == act.tobytes()
    # another episode or seed changes the rows
    _, dr3, act3 = _sample(env, r, ep + 1)
    _, dr4, act4 = _sample(env, _native.SO100DrRanges(seed=10, **RANGES), ep)
    for other_dr, other_act in ((dr3, act3), (dr4, act4)):
        assert (other_dr[:, :2] != dr[:, :2]).all(axis=1).all() and (other_act[:, 1:3] != act[:, 1:3]).all(axis=1).all()
    _check_rows(dr3, act3, 9, np.arange(n), ep + 1)
    _check_rows(dr4, act4, 10, np.arange(n), ep)
    # a range of zero width is its value bit for bit
    z = _native.SO100DrRanges(seed=9, mass=(1.1, 1.1), friction=(0.7, 0.7), delay=(3, 3), smoothing=(0.4, 0.4),
                              rate=(1.5, 1.5))
    _, drz, actz = _sample(env, z, ep)
    assert (drz[:, :2] == np.float32([1.1, 0.7])).all() and (actz == np.float32([3, 0.4, 1.5, 0])).all()


@pytest.mark.parametrize("n", SIZES)
def test_dr_sample_masks_and_null_outputs(n):
    from gym_so100 import _native
    env = _bare(n)
    r = _native.SO100DrRanges(seed=9, **RANGES)
    ep = np.arange(n) % 3
    _, full_dr, full_act = _sample(env, r, ep)
    i = np.arange(n)
    ma, mb = (i % 3 == 0).astype(np.uint8), (i % 4 == 1).astype(np.uint8) * 200      # any non-zero byte counts
    for a, b in ((ma, mb), (ma, None), (None, mb), (mb, ma), (np.zeros(n, np.uint8), None)):
        on = (np.zeros(n, bool) if a is None else a != 0) | (np.zeros(n, bool) if b is None else b != 0)
        rc, dr, act = _sample(env, r, ep, a, b)
        assert rc == 0
        assert np.array_equal(dr[on, :2], full_dr[on, :2]) and np.array_equal(act[on], full_act[on])
        assert (dr[~on] == 7.0).all() and (act[~on] == 7.0).all() and (dr[:, 2:] == 7.0).all()
    # a NULL output is skipped, the other is the full draw
    rc, dr, act = _sample(env, r, ep, dr=False)
    assert rc == 0 and (dr == 7.0).all() and np.array_equal(act, full_act)
    rc, dr, act = _sample(env, r, ep, act=False)
    assert rc == 0 and (act == 7.0).all() and np.array_equal(dr, full_dr)


@pytest.mark.parametrize("n", [5, 65, 257])
def test_dr_sample_does_not_depend_on_the_sharding(n):
    """env_offset = 3 on n - 3 envs equals rows 3.. of the full draw (n = 1 has no such rows)"""
    from gym_so100 import _native
    r = _native.SO100DrRanges(seed=9, **RANGES)
    ep = (np.arange(n) * 5) % 4
    _, dr, act = _sample(_bare(n), r, ep)
    rc, dr_s, act_s = _sample(_bare(n - 3, 3), r, ep[3:])
    assert rc == 0
    assert dr_s.tobytes() == dr[3:].tobytes() and act_s.tobytes() == act[3:].tobytes()
    _check_rows(dr_s, act_s, 9, np.arange(3, n), ep[3:])


def test_refusals_write_nothing():
    from gym_so100 import _native
    env = _bare(5)
    rc, dr, act = _sample(env, _native.SO100DrRanges(seed=9, **dict(RANGES, delay=(0, 8))))
    assert rc == -1 and "delay range" in env.lib.so100_last_error().decode()
    assert (dr == 7.0).all() and (act == 7.0).all()
    rc, dr, act = _sample(env, _native.SO100DrRanges(seed=9, **dict(RANGES, mass=(1.2, 0.8))), act=False)
    assert rc == -1 and "mass range" in env.lib.so100_last_error().decode() and (dr == 7.0).all()
    rc, _, _ = _sample(env, _native.SO100DrRanges(seed=9, **RANGES), dr=False, act=False)
    assert rc == -1 and "NULL dr_params and act_params" in env.lib.so100_last_error().decode()
    # so100_actuate on the weld variant: refused with its text, every output untouched
    P = _native.ptr
    ee = _env(5, variant="ee")
    hist = torch.full((8, 5, 6), 7.0, device="cuda")
    head = torch.full((5,), 9, dtype=torch.int32, device="cuda")
    y = torch.full((5, 6), 7.0, device="cuda")
    par = _dev(np.tile(np.float32([0, 1, 2, 0]), (5, 1)))
    cmd = torch.zeros(5, 6, device="cuda")
    rc = ee.lib.so100_actuate(ee._handle, P(ee.qpos), P(cmd), None, P(par), P(hist), P(head), P(y), ee._stream())
    torch.cuda.synchronize()
    assert rc == -1 and "so100_actuate: the model has ee = 1" in ee.lib.so100_last_error().decode()
    assert (hist == 7.0).all() and (head == 9).all() and (y == 7.0).all()
    rc = env.lib.so100_actuate(env._handle, P(env.qpos), P(cmd), None, P(par), P(hist), None, P(y), env._stream())
    torch.cuda.synchronize()
    assert rc == -1 and "NULL qpos, command" in env.lib.so100_last_error().decode()
    assert (hist == 7.0).all() and (y == 7.0).all()
    ee.close()


# ---------------------------------------------------------------------- so100_actuate
def _ref_run(model, oracle64):
    """the float32 and float64 restatements over all 257 envs and CALLS calls, computed once: per call (y32, y64, head,
    hist32, hist64, hist_hold, from_hold)"""
    if "run" not in _REF:
        q, cmd, re, par = act_ref.gpu_cases(ee_ref.rollout_states(oracle64, model, 257))
        a32, a64 = act_ref.Actuator(model, 257, np.float32), act_ref.Actuator(model, 257, np.float64)
        out = []
        for t in range(act_ref.CALLS):
            y32, y64 = a32(q[t], cmd[t], par, re[t]), a64(q[t], cmd[t], par, re[t])
            out.append((y32, y64, a32.head.copy(), a32.hist.copy(), a64.hist.copy(), a32.hist_hold.copy(),
                        a32.from_hold.copy()))
        _REF["run"] = out
    return _REF["run"]


@pytest.mark.parametrize("n", SIZES)
def test_actuate_matches_restatement(model, oracle64, n):
    from gym_so100 import _native
    P = _native.ptr
    env = _bare(n)
    q, cmd, re, par = act_ref.gpu_cases(ee_ref.rollout_states(oracle64, model, 257), n)
    ref = _ref_run(model, oracle64)
    exact = (par[:, 1] == 1) & (par[:, 2] >= 2)          # the envs whose applied action is claimed bit for bit
    assert exact[0] and (n == 1 or not exact.all())
    # garbage state: call 0 re-initialises every env
    hist = torch.full((8, n, 6), 7.0, device="cuda")
    head = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    y = torch.full((n, 6), 7.0, device="cuda")
    par_d = _dev(par)
    worst, compared = 0.0, 0
    for t in range(act_ref.CALLS):
        qd, cd, rd = _dev(q[t]), _dev(cmd[t]), _dev(re[t])
        rc = env.lib.so100_actuate(env._handle, P(qd), P(cd), P(rd), P(par_d), P(hist), P(head), P(y), env._stream())
        assert rc == 0, env.lib.so100_last_error().decode()
        torch.cuda.synchronize()
        y32, y64, rhead, h32, h64, hhold, yhold = (x[..., :n, :] if x.ndim > 1 else x[:n] for x in ref[t])
        yd, hd = y.cpu().numpy(), hist.cpu().numpy()
        assert np.array_equal(head.cpu().numpy(), rhead)
        # the ring: a command slot is clip(command) bit for bit in every env; a hold slot is within the bar
        assert np.array_equal(hd[~hhold].view(np.uint32), h32[~hhold].view(np.uint32))
        assert np.abs(hd - h64).max() <= BAR
        sel = exact[:, None] & ~yhold
        assert np.array_equal(yd[sel].view(np.uint32), y32[sel].view(np.uint32))
        compared += int(sel.sum())
        worst = max(worst, np.abs(yd - y64).max())
    print(f"n {n}: max |applied - float64 restatement| {worst:.3e} (bar {BAR:.3e}); {compared} values compared bitwise")
    assert worst <= BAR
    assert compared >= 6 * act_ref.CALLS // 4


def test_actuate_null_reinit_and_determinism(model, oracle64):
    """a NULL reinit re-initialises nothing; two runs from equal state give equal bytes"""
    from gym_so100 import _native
    P = _native.ptr
    n = 65
    env = _bare(n)
    q, cmd, re, par = act_ref.gpu_cases(ee_ref.rollout_states(oracle64, model, 257), n)
    a = act_ref.Actuator(model, n, np.float32)
    outs = []
    for rep in range(2):
        hist, head, y = torch.zeros(8, n, 6, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), \
            torch.zeros(n, 6, device="cuda")
        par_d = _dev(par)
        for t in range(10):
            qd, cd = _dev(q[t]), _dev(cmd[t])
            assert env.lib.so100_actuate(env._handle, P(qd), P(cd), None, P(par_d), P(hist), P(head), P(y),
                                         env._stream()) == 0
            torch.cuda.synchronize()
        outs.append((hist.cpu().numpy().tobytes(), head.cpu().numpy().tobytes(), y.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]
    for t in range(10):
        yr = a(q[t], cmd[t], par, None)                  # from the zero state: no hold value anywhere
    assert (np.frombuffer(outs[0][1], np.int32) == 10).all()
    exact = (par[:, 1] == 1) & (par[:, 2] >= 2)
    assert np.array_equal(np.frombuffer(outs[0][2], np.float32).reshape(n, 6)[exact], yr[exact])


# ---------------------------------------------------------------------- through SO100VecEnv
def _actions(n, steps, seed, k=6):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, size=(steps, n, k)).astype(np.float32)).cuda()


def _snapshot(env):
    torch.cuda.synchronize()
    return tuple(getattr(env, k).cpu().numpy().copy() for k in ("qpos", "qvel", "obs", "reward", "terminated", "truncated"))


def test_actuation_off_is_the_plain_env_bitwise():
    """an env with actuation=dict() (every range off) and the env without the key stay bit for bit equal in qpos, qvel,
    obs, reward, terminated and truncated through 20 auto-reset steps (the step's action noise is on in both: it is
    added after the actuator, as without it)"""
    n = 8
    a = _env(n, autoreset=True, max_episode_steps=7, domain_randomization=dict(actuation=dict()))
    plain = _env(n, autoreset=True, max_episode_steps=7, domain_randomization=dict(action_noise=0.05))
    assert plain._pre is False and a._pre is True
    assert a.dr_params.cpu().numpy().tobytes() == plain.dr_params.cpu().numpy().tobytes()
    assert (a.act_params.cpu().numpy() == np.float32([0, 1, 2, 0])).all()
    a.reset(seed=40)
    plain.reset(seed=40)
    acts = _actions(n, 20, 1) * 1.2                      # (beyond [-1, 1]: the actuator clips, as the step would)
    finished = 0
    for t in range(20):
        a.step(acts[t])
        plain.step(acts[t])
        sa, sp = _snapshot(a), _snapshot(plain)
        for x, y in zip(sa, sp):
            assert x.tobytes() == y.tobytes(), t
        assert torch.equal(a.actions, acts[t].clamp(-1, 1))
        finished += int(sa[5].sum())
    assert finished >= 2 * n
    a.close()
    plain.close()


def test_pure_delay_is_the_plain_env_fed_late():
    """delay (3, 3), auto-reset off: the env fed a_t equals the env without the model fed hold, hold, hold, a_0, a_1, ...
    bit for bit over 12 steps; `hold` is read back from ``actions`` after the first step"""
    n = 5
    dr = dict(mass=(0.8, 1.2), friction=(0.8, 1.2), action_noise=0.05)
    a = _env(n, domain_randomization=dict(dr, actuation=dict(delay=(3, 3))))
    plain = _env(n, domain_randomization=dr)
    a.reset(seed=50)
    plain.reset(seed=50)
    assert (a.act_params.cpu().numpy()[:, 0] == 3).all()
    acts = _actions(n, 12, 2)
    hold = None
    for t in range(12):
        a.step(acts[t])
        if t == 0:
            hold = a.actions.clone()
            assert float(hold.abs().max()) <= 1.0
        plain.step(hold if t < 3 else acts[t - 3])
        for x, y in zip(_snapshot(a), _snapshot(plain)):
            assert x.tobytes() == y.tobytes(), t
        assert torch.equal(a.actions, hold if t < 3 else acts[t - 3])
    assert (a.act_head.cpu().numpy() == 12).all()
    a.close()
    plain.close()


def _env_rows_ok(env, seed, rows, ranges):
    """dr_params / act_params rows `rows` of env against the restatement at the env's episode counters"""
    torch.cuda.synchronize()
    ep = env.episode.cpu().numpy()
    ids = np.arange(env.env_offset, env.env_offset + env.num_envs)
    _check_rows(env.dr_params.cpu().numpy(), env.act_params.cpu().numpy(), seed, ids, ep, rows, ranges)


PE = dict(per_episode=True, seed=77, mass=RANGES["mass"], friction=RANGES["friction"], action_noise=0.03,
          actuation={k: RANGES[k] for k in ("delay", "smoothing", "rate")})


def test_per_episode_resampling_state_path():
    n = 8
    env = _env(n, autoreset=True, max_episode_steps=3, env_offset=2, domain_randomization=PE)
    ptrs = (env.dr_params.data_ptr(), env.act_params.data_ptr())
    everyone = np.arange(n)
    _env_rows_ok(env, 77, everyone, RANGES)              # drawn at construction, episode counters as they are
    env.reset(seed=60)
    _env_rows_ok(env, 77, everyone, RANGES)
    acts = _actions(n, 13, 3)
    env.step(acts[12])
    # a masked reset redraws the masked envs only (and staggers the time limits of what follows)
    before = (env.dr_params.cpu().numpy().copy(), env.act_params.cpu().numpy().copy(), env.episode.cpu().numpy().copy())
    mask = everyone % 2 == 0
    env.reset(mask=mask)
    torch.cuda.synchronize()
    assert (env.episode.cpu().numpy()[mask] != before[2][mask]).all()
    assert np.array_equal(env.episode.cpu().numpy()[~mask], before[2][~mask])
    _env_rows_ok(env, 77, everyone[mask], RANGES)
    assert env.dr_params.cpu().numpy()[~mask].tobytes() == before[0][~mask].tobytes()
    assert env.act_params.cpu().numpy()[~mask].tobytes() == before[1][~mask].tobytes()
    assert (env.dr_params.cpu().numpy()[mask, :2] != before[0][mask, :2]).any()
    redrawn = 0
    for t in range(12):
        before = (env.dr_params.cpu().numpy().copy(), env.act_params.cpu().numpy().copy(),
                  env.episode.cpu().numpy().copy())
        env.step(acts[t])
        torch.cuda.synchronize()
        done = (env.terminated | env.truncated).cpu().numpy()
        assert np.array_equal(env.episode.cpu().numpy() != before[2], done)
        _env_rows_ok(env, 77, everyone[done], RANGES)
        assert env.dr_params.cpu().numpy()[~done].tobytes() == before[0][~done].tobytes()
        assert env.act_params.cpu().numpy()[~done].tobytes() == before[1][~done].tobytes()
        assert 0 < done.sum() < n or not done.any()      # the finished envs are never all of them here
        redrawn += int(done.sum())
    assert redrawn >= 3 * n
    dr = env.dr_params.cpu().numpy()
    assert (dr[:, 2] == np.float32(0.03)).all() and (dr[:, 3] == 0).all()
    assert (env.dr_params.data_ptr(), env.act_params.data_ptr()) == ptrs
    env.close()


def test_per_episode_resampling_pixel_path():
    n = 3
    env = _env(n, autoreset=True, max_episode_steps=3, obs_type="so100_pixels_agent_pos", observation_width=64,
               observation_height=48, domain_randomization=dict(PE, visual=dict(ambient=(0.9, 1.1))))
    assert env._dr_per_episode and not env._visual[1]    # the visual part's own per_episode stays its own
    env.reset(seed=61)
    everyone = np.arange(n)
    _env_rows_ok(env, 77, everyone, RANGES)
    acts = _actions(n, 4, 4)
    for t in range(4):
        before = (env.dr_params.cpu().numpy().copy(), env.act_params.cpu().numpy().copy(),
                  env.episode.cpu().numpy().copy())
        env.step(acts[t])
        torch.cuda.synchronize()
        done = (env.terminated | env.truncated).cpu().numpy()
        assert done.all() == (t == 2) and done.any() == (t == 2)
        assert np.array_equal(env.episode.cpu().numpy() != before[2], done)
        _env_rows_ok(env, 77, everyone[done], RANGES)
        assert env.dr_params.cpu().numpy()[~done].tobytes() == before[0][~done].tobytes()
        assert env.act_params.cpu().numpy()[~done].tobytes() == before[1][~done].tobytes()
        if t == 2:
            assert (env.dr_params.cpu().numpy()[:, :2] != before[0][:, :2]).any()
    env.close()


def test_without_per_episode_dr_params_is_the_host_draw_throughout():
    n = 8
    dr = dict(mass=(0.7, 1.3), friction=(0.5, 1.5), action_noise=0.02, seed=5)
    a = _env(n, autoreset=True, max_episode_steps=3, env_offset=4,
             domain_randomization=dict(dr, actuation=PE["actuation"]))
    plain = _env(n, autoreset=True, max_episode_steps=3, env_offset=4, domain_randomization=dr)
    want = plain.dr_params.cpu().numpy().tobytes()
    act0 = a.act_params.cpu().numpy().copy()
    _check_rows(None, act0, 5, np.arange(4, 4 + n), None, ranges=dict(PE["actuation"]))      # drawn once, episode 0
    a.reset(seed=62)
    acts = _actions(n, 7, 5)
    for t in range(7):
        a.step(acts[t])
        torch.cuda.synchronize()
        assert a.dr_params.cpu().numpy().tobytes() == want
        assert a.act_params.cpu().numpy().tobytes() == act0.tobytes()
    assert int(a.episode.max()) >= 2
    a.close()
    plain.close()


def test_get_state_set_state_reproduces_the_rollout():
    n = 5
    env = _env(n, autoreset=True, max_episode_steps=4, domain_randomization=PE)
    env.reset(seed=63)
    acts = _actions(n, 8, 6)
    for t in range(3):
        env.step(acts[t])
    st = env.get_state()
    assert set(st["actuation"]) == {"hist", "head", "params", "applied"}
    first = []
    for t in range(3, 8):
        env.step(acts[t])
        first.append(_snapshot(env)[0])
    env.set_state(**st)
    for t in range(3, 8):
        env.step(acts[t])
        assert _snapshot(env)[0].tobytes() == first[t - 3].tobytes(), t
    with pytest.raises(ValueError):
        _bare(5).set_state(st["qpos"], st["qvel"], actuation=st["actuation"])
    env.close()


def test_ee_delta_chain_runs_through_the_actuator():
    """action_mode="ee_delta" with a pure delay: the EE prologue writes the staging tensor, the actuator holds the pose
    for `delay` steps and then applies the joint command of `delay` steps earlier"""
    n = 5
    env = _env(n, action_mode="ee_delta", domain_randomization=dict(action_noise=0.0, actuation=dict(delay=(2, 2))))
    env.reset(seed=64)
    acts = _actions(n, 6, 7, k=5)
    cmds, hold = [], None
    for t in range(6):
        env.step(acts[t])
        cmds.append(env.act_command.clone())
        if t == 0:
            hold = env.actions.clone()
        assert torch.equal(env.actions, hold if t < 2 else cmds[t - 2].clamp(-1, 1))
    assert env.reinit.sum().item() == 0 and not torch.equal(cmds[0], cmds[5])
    env.close()


def test_sb3_adapter_takes_the_dict_and_steps():
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 4
    venv = SO100SB3VecEnv(n, task="so100_touch_cube", max_episode_steps=3, domain_randomization=PE)
    env = venv.venv
    assert env._act and env._dr_per_episode and env.act_params is not None
    venv.reset()
    acts = np.random.default_rng(8).uniform(-1, 1, size=(4, n, 6)).astype(np.float32)
    for t in range(4):
        obs, rew, dones, infos = venv.step(acts[t])
        assert np.asarray(obs).shape[0] == n and np.isfinite(np.asarray(rew)).all()
        assert np.asarray(dones).all() == (t == 2)
    _env_rows_ok(env, 77, np.arange(n), RANGES)
    assert int(env.episode.min()) >= 1
    venv.close()


def test_default_env_calls_neither_entry_point(monkeypatch):
    """with both new ctypes functions replaced by ones that raise, a default env (and one with today's DR dict) resets
    and steps"""
    from gym_so100 import _native
    lib = _native.load()

    def boom(*a):
        raise AssertionError("a new entry point was called by an env that has neither feature on")
    monkeypatch.setattr(lib, "so100_dr_sample", boom, raising=False)
    monkeypatch.setattr(lib, "so100_actuate", boom, raising=False)
    for kw in (dict(), dict(domain_randomization=dict(mass=(0.8, 1.2), action_noise=0.05)),
               dict(action_mode="ee_delta")):
        env = _env(4, autoreset=True, max_episode_steps=2, **kw)
        env.reset(seed=3)
        for t in range(3):
            env.step(torch.zeros(4, env.action_dim, device="cuda"))
        env.step_async_raw()
        env.reset(mask=np.array([1, 0, 1, 0], bool))
        torch.cuda.synchronize()
        assert env._pre is (kw.get("action_mode") == "ee_delta")
        env.close()
    with pytest.raises(AssertionError, match="a new entry point"):
        _env(4, domain_randomization=dict(per_episode=True))
