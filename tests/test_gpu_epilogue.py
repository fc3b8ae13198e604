"""The step kernel's epilogue (final_stage: auto-reset, GoalEnv goal sampling, the total_steps counter) and
so100_reset_kernel against host restatements (tests/dr_ref.py) and the fp64 oracle: what a reset produces, not only
that one happened.  Fused and split paths.  DESIGN.md §5."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dr_ref as R

pytestmark = pytest.mark.gpu

N = 37                 # a ragged tail wave (4 envs per wave)
OFFSET = 1000
T = 3                  # max_episode_steps
MODES = pytest.mark.parametrize("fused", [True, False], ids=["fused", "split"])


def _env(fused, **kw):
    from gym_so100 import SO100VecEnv
    env = SO100VecEnv(N, device="cuda:0", env_offset=OFFSET, max_episode_steps=T, **kw)
    env.fused = fused
    assert env.fused == fused
    return env


def _np(t):
    return t.detach().cpu().numpy()


def _check_reset_state(env, model, oracle64, rows, episode):
    """Envs `rows` hold the first state of their episode `episode[i]`: the RandomState(episode_seed) spawn bit for bit,
    the start pose, zero velocities and warm start, elapsed 0, the episode counter, and the oracle's observation."""
    torch.cuda.synchronize()
    qpos, qvel, warm, obs = _np(env.qpos), _np(env.qvel), _np(env.qacc_warmstart), _np(env.obs)
    elapsed, ep = _np(env.elapsed), _np(env.episode)
    start = np.array(model.start_qpos[:], np.float64).astype(np.float32)
    d = oracle64.new_data()
    for i in rows:
        assert ep[i] == episode[i], (i, ep[i], episode[i])
        spawn = oracle64.spawn_pose(int(R.episode_seed(env.base_seed, OFFSET + i, int(episode[i]))))
        np.testing.assert_array_equal(qpos[i, 6:13], spawn.astype(np.float32), err_msg=f"env {i} episode {episode[i]}")
        np.testing.assert_array_equal(qpos[i, :6], start)
        assert not qvel[i].any() and not warm[i].any() and elapsed[i] == 0
        oracle64.reset(model, d, spawn)
        np.testing.assert_allclose(obs[i], oracle64.observe(model, d), rtol=0, atol=2e-7)
    return qpos


@MODES
def test_autoreset_state_matches_restatement(fused, model, oracle64):
    """7 steps at max_episode_steps = 3 give two auto-resets: after each, every reset env holds RandomState(episode_seed(
    base seed, global env, new episode))'s spawn and the oracle's observation of it, and final_observation is the
    oracle's observation of the terminal state (abs 1e-5, the step-parity bar on qpos); then reset() with in-kernel
    seeds, and reset(mask) on half the envs with the other half untouched bit for bit."""
    env = _env(fused, seed=11)
    episode = np.zeros(N, np.int64)
    env.reset()
    episode += 1
    _check_reset_state(env, model, oracle64, range(N), episode)
    spawns = [_np(env.qpos)[:, 6:9].copy()]
    rng = np.random.default_rng(5)
    d = oracle64.new_data()
    resets, el = 0, np.zeros(N, np.int64)
    for k in range(1, 8):
        a = rng.uniform(-1, 1, (N, 6)).astype(np.float32)
        q0, v0, w0 = (_np(t).astype(np.float64) for t in (env.qpos, env.qvel, env.qacc_warmstart))
        obs, rew, term, trunc, info = env.step(torch.from_numpy(a).cuda())
        torch.cuda.synchronize()
        done = _np(term | trunc)
        el += 1
        np.testing.assert_array_equal(_np(trunc), el == T)
        assert np.array_equal(_np(info["_final_observation"]), done)
        el[done] = 0
        np.testing.assert_array_equal(_np(env.elapsed), el)
        rows = np.flatnonzero(done)
        if not len(rows):
            assert np.array_equal(_np(env.episode), episode)
            continue
        resets += 1
        episode[rows] += 1
        _check_reset_state(env, model, oracle64, rows, episode)
        assert torch.equal(obs, env.obs)
        final = _np(info["final_observation"])
        for i in rows:                                   # the terminal observation: the oracle's step from the same state
            oracle64.set_state(d, q0[i], v0[i], w0[i])
            ob, _, _ = oracle64.env_step(model, d, 0, a[i])
            np.testing.assert_allclose(final[i], ob, rtol=0, atol=1e-5)
        np.testing.assert_array_equal(_np(env.episode), episode)
        spawns.append(_np(env.qpos)[:, 6:9].copy())
    assert resets == 2 and (episode == 3).all()
    # distinct spawns across envs and across an env's consecutive episodes
    for s in spawns:
        assert len(np.unique(s[:, 0])) == N
    assert (spawns[0][:, :2] != spawns[1][:, :2]).all() and (spawns[1][:, :2] != spawns[2][:, :2]).all()

    # reset(mask): half the envs start a new episode, the others keep every bit of their state
    mask = np.arange(N) % 2 == 0
    before = {k: getattr(env, k).clone() for k in ("qpos", "qvel", "qacc_warmstart", "elapsed", "episode", "obs")}
    assert (before["elapsed"] > 0).all() and before["qvel"].abs().sum() > 0
    env.reset(mask=torch.from_numpy(mask))
    episode[mask] += 1
    _check_reset_state(env, model, oracle64, np.flatnonzero(mask), episode)
    other = torch.from_numpy(~mask).cuda()
    for k, t in before.items():
        assert torch.equal(getattr(env, k)[other], t[other]), k
    # reset() of every env with the in-kernel seeds
    env.reset()
    episode += 1
    _check_reset_state(env, model, oracle64, range(N), episode)
    env.close()


def _check_goals(env, model, oracle64, rows, episode, count):
    """desired_goal of envs `rows` equals the restated sample of (base seed, global env, episode) from the box that
    `count[i]` (the step count at sampling time) selects, within 2 fp32 ulps of max(|lo|, |hi|) (FMA contraction of
    lo + (hi - lo) * u and the fp32 c +- 0.03f); achieved_goal is the new spawn's cube site."""
    torch.cuda.synchronize()
    dg, ag, qpos, obs = _np(env.desired_goal), _np(env.achieved_goal), _np(env.qpos), _np(env.obs)
    d = oracle64.new_data()
    for i in rows:
        spawn = oracle64.spawn_pose(int(R.episode_seed(env.base_seed, OFFSET + i, int(episode[i]))))
        np.testing.assert_array_equal(qpos[i, 6:13], spawn.astype(np.float32))
        want = R.goal_sample(env.base_seed, OFFSET + i, int(episode[i]), spawn[:2], int(count[i]), model)
        lo, hi = R.goal_box(spawn[:2], int(count[i]), model)
        tol = 2 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
        err = np.abs(dg[i].astype(np.float64) - want)
        assert (err <= tol).all(), (i, int(count[i]), dg[i], want, err, tol)
        assert ((dg[i] >= lo - tol) & (dg[i] <= hi + tol)).all()
        oracle64.reset(model, d, spawn)
        np.testing.assert_allclose(ag[i], np.array(d.site_cube[:]), rtol=0, atol=2e-7)
        np.testing.assert_array_equal(ag[i], obs[i, :3])
    return dg


@MODES
def test_goal_sampling_and_curriculum_switch(fused, model, oracle64):
    """GoalEnv: the goal an auto-reset (and reset()) samples equals the host restatement, and the curriculum switches on
    the incremented counter: the terminal step that brings total_steps to exactly 5000 samples from the bin box
    (the reference increments in step() before reset() samples).  Counters set so the terminal step of the first
    episode brings them to 4998, 4999, 5000, 5001 and 0 across the envs."""
    env = _env(fused, task="so100_goal", seed=13)
    episode = np.zeros(N, np.int64)
    obs, _ = env.reset()
    episode += 1
    count = np.zeros(N, np.int64)
    hist = [[g] for g in _check_goals(env, model, oracle64, range(N), episode, count).copy()]      # per env: its goals
    at_terminal = np.array([4998, 4999, 5000, 5001, 0])[np.arange(N) % 5]
    count = at_terminal - T
    env.total_steps.copy_(torch.from_numpy(count.astype(np.int32)))
    a = torch.zeros(N, 6, device="cuda")
    sampled_at = set()
    for k in range(1, 2 * T + 1):
        obs, rew, term, trunc, info = env.step(a)
        torch.cuda.synchronize()
        count += 1
        np.testing.assert_array_equal(_np(env.total_steps), count)          # exactly +1 per step
        done = _np(term | trunc)
        rows = np.flatnonzero(done)
        for i in np.flatnonzero(~done):                                      # a goal lasts its episode
            np.testing.assert_array_equal(_np(env.desired_goal)[i], hist[i][-1])
        if len(rows):
            episode[rows] += 1
            dg = _check_goals(env, model, oracle64, rows, episode, count).copy()
            assert torch.equal(obs["desired_goal"], env.desired_goal) and torch.equal(obs["achieved_goal"], env.achieved_goal)
            for i in rows:
                hist[i].append(dg[i])
                sampled_at.add((int(count[i]), bool(count[i] >= 5000)))
                # independent of the restatement: the bin box from 5000 on, around the spawn's xy before
                if count[i] >= 5000:
                    assert ((dg[i] >= np.array(model.goal_bin_lo[:]) - 1e-6) & (dg[i] <= np.array(model.goal_bin_hi[:]) + 1e-6)).all()
                else:
                    assert (np.abs(dg[i, :2] - _np(env.qpos)[i, 6:8]) <= 0.03 + 1e-6).all() and 0.01 <= dg[i, 2] <= 0.05
    assert all(len(h) >= 3 for h in hist)                                    # two auto-resets or more per env
    # both sides of the switch were sampled by auto-resets, the exact 5000 among them
    assert {(4998, False), (4999, False), (5000, True), (5001, True), (0, False)} <= sampled_at
    # goals differ across envs, across lanes and across an env's consecutive episodes
    last = np.array([h[-1] for h in hist])
    assert len(np.unique(last[:, 0])) == N and (last[:, 0] != last[:, 1]).all() and (last[:, 1] != last[:, 2]).all()
    for h in hist:
        for g0, g1 in zip(h[:-1], h[1:]):
            assert (g0 != g1).all()

    # reset() samples by the counter as it stands (no increment): counters straddling 5000
    count = np.array([4999, 5000, 5001, 4998])[np.arange(N) % 4].astype(np.int64)
    env.total_steps.copy_(torch.from_numpy(count.astype(np.int32)))
    env.reset()
    episode += 1
    _check_goals(env, model, oracle64, range(N), episode, count)
    np.testing.assert_array_equal(_np(env.total_steps), count)
    mask = np.arange(N) % 3 == 0
    before = env.desired_goal.clone()
    env.reset(mask=torch.from_numpy(mask))
    episode[mask] += 1
    _check_goals(env, model, oracle64, np.flatnonzero(mask), episode, count)
    other = torch.from_numpy(~mask).cuda()
    assert torch.equal(env.desired_goal[other], before[other])
    env.close()
