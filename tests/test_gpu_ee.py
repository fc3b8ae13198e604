"""The Cartesian end-effector action mode on the GPU (csrc/so100_ee.hip, include/so100.h ABI 25):
so100_ee_jacobian and so100_ee_action against the float64 numpy restatement (tests/ee_ref.py) on the states of a 25-step
random rollout, the round trip through so100_unnormalize, masking and determinism, the refusals, and
SO100VecEnv(action_mode="ee_delta") / SO100SB3VecEnv in closed loop.

Bars: 4 F + 1e-6 on q_cmd, joint_action and ee_target, 4 F_J + 1e-7 on the Jacobian and ee_site, with F and F_J the
float32 restatement's own floors against its float64 self over these very states and actions (ee_ref.F_QCMD, F_JAC,
measured by tests/test_ee_cpu.py); the factor 4 covers FMA contraction and the kernel's association in the chain.
The sizes 65 and 257 cross a wave and a workgroup boundary of the kernel's one-env-per-lane mapping."""
import ctypes

import numpy as np
import pytest

import ee_ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SIZES = [6, 1, 65, 257]
BAR = 4 * ee_ref.F_QCMD + 1e-6
BAR_J = 4 * ee_ref.F_JAC + 1e-7
_REF = {}


def _env(n, **kw):
    from gym_so100 import SO100VecEnv
    kw.setdefault("autoreset", False)
    return SO100VecEnv(n, task="so100_touch_cube", device="cuda:0", **kw)


def _ctrl(model, **kw):
    from gym_so100 import _native
    return _native.SO100EeCtrl(**dict(ee_ref.default_control(model), **kw))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ee_action(env, ctrl, qpos, action, reinit, q_cmd, want_target=True):
    """one so100_ee_action launch on device copies of the inputs -> (rc, q_cmd, joint_action, ee_target) as numpy"""
    from gym_so100 import _native
    P = _native.ptr
    n = env.num_envs
    qc = _dev(q_cmd).clone()
    ja = torch.full((n, 6), 7.0, dtype=torch.float32, device="cuda")
    tg = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    qp, ac = _dev(qpos), _dev(action)                      # (held until the launch has run)
    ri = None if reinit is None else _dev(np.asarray(reinit, np.uint8))
    rc = env.lib.so100_ee_action(env._handle, ctypes.byref(ctrl), P(qp), P(ac), P(ri), P(qc), P(ja),
                                 P(tg) if want_target else None, env._stream())
    torch.cuda.synchronize()
    return rc, qc.cpu().numpy(), ja.cpu().numpy(), tg.cpu().numpy()


def _ref_action(model, oracle64, case):
    """the float64 restatement over all 257 envs with reinit set for the odd envs, computed once per action set"""
    if case not in _REF:
        qpos, q_cmd, acts = ee_ref.gpu_cases(oracle64, model, 257)
        _REF[case] = ee_ref.EeRef(oracle64, model).action(qpos, acts[case], q_cmd, np.arange(257) % 2)
    return _REF[case]


def _ref_jacobian(model, oracle64):
    if "jac" not in _REF:
        qpos, _, _ = ee_ref.gpu_cases(oracle64, model, 257)
        r = ee_ref.EeRef(oracle64, model)
        out = [r.jacobian(q[:5].astype(np.float64)) for q in qpos]
        _REF["jac"] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))
    return _REF["jac"]


def _jacobian(env, qpos):
    from gym_so100 import _native
    P = _native.ptr
    n = qpos.shape[0]
    ee = torch.zeros(n, 3, dtype=torch.float32, device="cuda")
    jac = torch.zeros(n, 3, 5, dtype=torch.float32, device="cuda")
    qp = _dev(qpos)                                        # (held until the launch has run)
    _native.check(env.lib.so100_ee_jacobian(env._handle, n, P(qp), P(ee), P(jac), env._stream()),
                  "so100_ee_jacobian")
    torch.cuda.synchronize()
    return ee.cpu().numpy(), jac.cpu().numpy()


# ---------------------------------------------------------------------- the two ops against the restatement
@pytest.mark.parametrize("n", SIZES)
def test_jacobian_matches_float64_restatement(model, oracle64, n):
    env = _env(n)
    qpos, _, _ = ee_ref.gpu_cases(oracle64, model, n)
    ee, jac = _jacobian(env, qpos)
    ee64, jac64 = _ref_jacobian(model, oracle64)
    d_ee, d_j = np.abs(ee - ee64[:n]).max(), np.abs(jac - jac64[:n]).max()
    print(f"n={n}: |ee - ref| {d_ee:.3e}, |J - ref| {d_j:.3e} (bar {BAR_J:.3e}), roll column {np.abs(jac[:, :, 4]).max():.3e}")
    assert d_ee <= BAR_J and d_j <= BAR_J
    assert np.abs(jac[:, :, 4]).max() <= BAR_J            # wrist roll turns about an axis through ee_site
    env.close()


@pytest.mark.parametrize("case", ["random", "corners"])
@pytest.mark.parametrize("n", SIZES)
def test_action_matches_float64_restatement(model, oracle64, n, case):
    env = _env(n)
    qpos, q_cmd, acts = ee_ref.gpu_cases(oracle64, model, n)
    a = acts[case]
    rc, qc, ja, tg = _ee_action(env, _ctrl(model), qpos, a, np.arange(n) % 2, q_cmd)
    assert rc == 0
    qc64, ja64, tg64 = (x[:n] for x in _ref_action(model, oracle64, case))
    d = [np.abs(x - y).max() for x, y in ((qc, qc64), (ja, ja64), (tg, tg64))]
    print(f"n={n} {case}: |q_cmd - ref| {d[0]:.3e}, |joint_action - ref| {d[1]:.3e}, |ee_target - ref| {d[2]:.3e} "
          f"(bar {BAR:.3e})")
    assert max(d) <= BAR
    # round trip: the joint actions are the commanded targets in the step's normalisation (a few float32 roundings at
    # a range width of at most 5.6), and the gripper passes through
    back = env.unnormalize(_dev(ja)).cpu().numpy()
    print(f"    |unnormalize(joint_action) - q_cmd| {np.abs(back[:, :5] - qc).max():.3e}")
    assert np.abs(back[:, :5] - qc).max() <= 4e-6
    assert np.array_equal(ja[:, 5], np.clip(a[:, 4], -1, 1))
    if case == "corners":
        assert np.array_equal(ja[:, 5], a[:, 4])
    assert (np.abs(ja) <= 1).all()
    env.close()


# ---------------------------------------------------------------------- masking and determinism
def test_reinit_mask_null_mask_determinism_and_batch_independence(model, oracle64):
    n = 8
    env, ctrl = _env(n), _ctrl(model)
    qpos, q_cmd, acts = ee_ref.gpu_cases(oracle64, model, n)
    a = acts["random"]
    half = (np.arange(n) % 2).astype(np.uint8)
    _, qc, ja, tg = _ee_action(env, ctrl, qpos, a, half, q_cmd)
    # reinit envs start from qpos[:5], the others from their q_cmd
    seeded = np.where(half[:, None] != 0, qpos[:, :5], q_cmd)
    _, qc2, ja2, tg2 = _ee_action(env, ctrl, qpos, a, np.zeros(n, np.uint8), seeded)
    assert np.array_equal(qc, qc2) and np.array_equal(ja, ja2) and np.array_equal(tg, tg2)
    _, qc0, _, _ = _ee_action(env, ctrl, qpos, a, np.zeros(n, np.uint8), q_cmd)
    assert not np.array_equal(qc0[1], qc[1]) and np.array_equal(qc0[0::2], qc[0::2])
    # a NULL reinit is all-zero
    _, qc3, ja3, tg3 = _ee_action(env, ctrl, qpos, a, None, q_cmd)
    assert np.array_equal(qc3, qc0)
    # two launches give equal bytes
    _, qc4, ja4, tg4 = _ee_action(env, ctrl, qpos, a, None, q_cmd)
    assert qc4.tobytes() == qc3.tobytes() and ja4.tobytes() == ja3.tobytes() and tg4.tobytes() == tg3.tobytes()
    # a NULL ee_target: the other outputs are what they are with it, and nothing is written to it
    _, qc5, ja5, tg5 = _ee_action(env, ctrl, qpos, a, None, q_cmd, want_target=False)
    assert np.array_equal(qc5, qc3) and np.array_equal(ja5, ja3) and (tg5 == 7.0).all()
    # 4 envs equal the first 4 of 8
    env4 = _env(4)
    _, qc6, ja6, tg6 = _ee_action(env4, ctrl, qpos[:4], a[:4], half[:4], q_cmd[:4])
    assert np.array_equal(qc6, qc[:4]) and np.array_equal(ja6, ja[:4]) and np.array_equal(tg6, tg[:4])
    env.close()
    env4.close()


def test_refusals_leave_every_output_untouched(model, oracle64):
    from gym_so100 import SO100VecEnv, _native
    n = 6
    env = _env(n)
    qpos, q_cmd, acts = ee_ref.gpu_cases(oracle64, model, n)
    a = acts["random"]

    def refused(e, ctrl, text):
        rc, qc, ja, tg = _ee_action(e, ctrl, qpos, a, None, q_cmd)
        assert rc == -1 and text in e.lib.so100_last_error().decode()
        assert np.array_equal(qc, q_cmd) and (ja == 7.0).all() and (tg == 7.0).all()
    refused(env, _ctrl(model, iters=0), "iters outside 1..8")
    refused(env, _ctrl(model, damping=float("nan")), "damping")
    refused(env, _ctrl(model, ws_lo=(0.0, 0.0, 1.0)), "workspace box")
    bad = _ctrl(model)
    bad.size = 4
    refused(env, bad, "so100_ee_ctrl.size 4, expected 52")
    ee_model = SO100VecEnv(n, task="so100_touch_cube", variant="ee", autoreset=False)
    refused(ee_model, _ctrl(model), "ee = 1")
    # NULL pointers with a live env
    P, ctrl = _native.ptr, _ctrl(model)
    t = [_dev(qpos), _dev(a), _dev(q_cmd).clone(), torch.full((n, 6), 7.0, dtype=torch.float32, device="cuda")]
    for k in range(4):
        args = [P(x) for x in t]
        args[k] = None
        rc = env.lib.so100_ee_action(env._handle, ctypes.byref(ctrl), args[0], args[1], None, args[2], args[3], None,
                                     env._stream())
        assert rc == -1 and "NULL qpos, action, q_cmd or joint_action" in env.lib.so100_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(t[2].cpu().numpy(), q_cmd) and (t[3] == 7.0).all()
    env.close()
    ee_model.close()


# ---------------------------------------------------------------------- SO100VecEnv(action_mode="ee_delta")
REACH = [(-1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (-1.0, 1.0, -0.5)]


def test_vec_env_reaches_in_free_space(model):
    """the CPU file's four reach cases (spawn seed 3, 8 full-scale steps, 22 of zero action), one env each, at its
    bars: ||ee(q_cmd) - goal|| <= 1 mm, ||site_ee - goal|| <= 15 mm"""
    env = _env(4, action_mode="ee_delta", max_episode_steps=0)
    assert env.action_dim == 5 and env.ee_joint_target.shape == (4, 5) and env.ee_target.shape == (4, 3)
    obs, _ = env.reset(seed=[3, 3, 3, 3])
    c = ee_ref.default_control(model)
    goal = obs[:, 6:9].cpu().numpy().astype(np.float64)
    a = np.zeros((4, 5), np.float32)
    a[:, :3] = REACH
    for k in range(30):
        if k < 8:
            goal = np.clip(goal + c["pos_scale"] * np.asarray(REACH), c["ws_lo"], c["ws_hi"])
        obs, *_ = env.step(a if k < 8 else np.zeros((4, 5), np.float32))
    qp = np.zeros((4, 13), np.float32)
    qp[:, :5] = env.ee_joint_target.cpu().numpy()
    ee_cmd, _ = _jacobian(env, qp)
    e_cmd = np.linalg.norm(ee_cmd - goal, axis=1)
    e_arm = np.linalg.norm(obs[:, 6:9].cpu().numpy() - goal, axis=1)
    print("command space mm", np.round(1e3 * e_cmd, 3), "arm mm", np.round(1e3 * e_arm, 3))
    assert (e_cmd <= 1e-3).all()
    assert (e_arm <= 15e-3).all()
    assert np.abs(env.ee_target.cpu().numpy() - ee_cmd).max() <= 1e-3    # zero action: the target rests at ee(q_cmd)
    with pytest.raises(ValueError):
        env.step(np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError):
        env.set_action_buffer(torch.zeros(4, 6, device="cuda"))
    env.close()


def test_step_is_untouched_joint_twin_bitwise():
    """a joint-mode env fed this env's `actions` tensor step by step: 20 auto-reset steps (episodes of 7) end with qpos,
    reward, terminated and truncated bit for bit equal"""
    n = 16
    ee = _env(n, action_mode="ee_delta", autoreset=True, max_episode_steps=7, seed=5)
    jt = _env(n, autoreset=True, max_episode_steps=7, seed=5)
    ee.reset(seed=11)
    jt.reset(seed=11)
    rng = np.random.default_rng(2)
    trunc_seen = 0
    for k in range(20):
        ee.step(rng.uniform(-1, 1, size=(n, 5)).astype(np.float32))
        jt.step(ee.actions.clone())
        for name in ("qpos", "qvel", "reward", "terminated", "truncated", "obs"):
            assert torch.equal(getattr(ee, name), getattr(jt, name)), (k, name)
        trunc_seen += int(ee.truncated.sum())
        assert torch.equal(ee.reinit.bool(), ee.terminated | ee.truncated)
    assert trunc_seen >= n                                 # the episodes did end and restart inside the comparison
    # the zero-copy action buffer feeds the prologue: the same step as step() from the same state
    st = ee.get_state()
    assert set(st) - set(jt.get_state()) == {"ee_joint_target"}
    a = torch.from_numpy(rng.uniform(-1, 1, size=(n, 5)).astype(np.float32)).cuda()
    ee.step(a)
    q1, t1 = ee.qpos.clone(), ee.ee_joint_target.clone()
    ee.set_state(**st)
    ee.set_action_buffer(a)
    ee.step_async_raw()
    assert torch.equal(ee.qpos, q1) and torch.equal(ee.ee_joint_target, t1)
    with pytest.raises(ValueError):
        jt.set_state(st["qpos"], st["qvel"], ee_joint_target=st["ee_joint_target"])
    ee.close()
    jt.close()


@pytest.mark.parametrize("obs_type", ["so100_state", "so100_pixels_agent_pos"])
def test_new_episode_starts_from_the_fresh_pose(model, oracle64, obs_type):
    """max_episode_steps=3: the step that ends the episodes sets reinit for them (state and pixel path), and the first
    step of the new episode seeds ee_joint_target from the fresh qpos, not from the finished episode's command"""
    n = 6
    kw = dict(observation_width=32, observation_height=24) if obs_type != "so100_state" else {}
    env = _env(n, action_mode="ee_delta", autoreset=True, max_episode_steps=3, obs_type=obs_type, **kw)
    env.reset(seed=20)
    assert (env.reinit == 1).all()
    rng = np.random.default_rng(4)
    for k in range(3):
        env.step(rng.uniform(-1, 1, size=(n, 5)).astype(np.float32))
        assert bool((env.reinit == 0).all()) == (k < 2)
    assert env.truncated.all() and (env.reinit == 1).all()
    fresh, stale = env.qpos.cpu().numpy(), env.ee_joint_target.cpu().numpy()
    assert np.abs(fresh[:, :5] - stale).max() > 0.05       # the old command is far from the new episode's pose
    a = rng.uniform(-1, 1, size=(n, 5)).astype(np.float32)
    env.step(a)
    want = ee_ref.EeRef(oracle64, model).action(fresh, a, stale, np.ones(n))[0]
    assert np.abs(env.ee_joint_target.cpu().numpy() - want).max() <= BAR
    assert (env.reinit == 0).all()
    env.close()


def test_masked_reset_reinitialises_only_its_envs(model, oracle64):
    n = 6
    env = _env(n, action_mode="ee_delta", max_episode_steps=0)
    env.reset(seed=30)
    rng = np.random.default_rng(6)
    for _ in range(4):
        env.step(rng.uniform(-1, 1, size=(n, 5)).astype(np.float32))
    assert (env.reinit == 0).all()
    mask = np.array([1, 0, 1, 0, 0, 0], bool)
    env.reset(mask=mask)
    assert np.array_equal(env.reinit.cpu().numpy() != 0, mask)
    qpos, q_cmd = env.qpos.cpu().numpy(), env.ee_joint_target.cpu().numpy()
    a = rng.uniform(-1, 1, size=(n, 5)).astype(np.float32)
    env.step(a)
    want = ee_ref.EeRef(oracle64, model).action(qpos, a, q_cmd, mask)[0]
    got = env.ee_joint_target.cpu().numpy()
    assert np.abs(got - want).max() <= BAR
    cont = ee_ref.EeRef(oracle64, model).action(qpos, a, q_cmd, None)[0]     # had the reset envs kept their command
    assert np.abs(got[mask] - cont[mask]).max() > 10 * BAR
    assert (env.reinit == 0).all()
    env.close()


def test_sb3_adapter_reports_the_five_dim_space_and_steps():
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 8
    env = SO100SB3VecEnv(n, task="so100_touch_cube", action_mode="ee_delta", ee_control={"iters": 3},
                         max_episode_steps=4)
    assert env.action_space.shape == (5,) and env.action_space.low.min() == -1 and env.action_space.high.max() == 1
    assert env.venv.ee_control["iters"] == 3
    obs = env.reset()
    rng = np.random.default_rng(8)
    dones_seen = 0
    for _ in range(5):
        obs, rew, dones, infos = env.step(rng.uniform(-1, 1, size=(n, 5)).astype(np.float32))
        assert obs.shape == (n, 15) and rew.shape == (n,) and np.isfinite(obs).all()
        dones_seen += int(dones.sum())
    assert dones_seen == n
    with pytest.raises(ValueError):
        env.step_async(np.zeros((n, 6), np.float32))
    assert SO100SB3VecEnv(2, task="so100_touch_cube").action_space.shape == (6,)
    env.close()
