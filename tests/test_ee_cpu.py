"""CPU checks of the Cartesian end-effector action mode (include/so100.h ABI 25): the struct mirror and
the argument-level refusals of so100_ee_action (each before any device work, so they answer without a device), the
ValueErrors of SO100VecEnv(action_mode=, ee_control=), and the definition itself, restated in numpy (tests/ee_ref.py) on
the oracle's kinematics: its Jacobian against central differences of the float64 oracle's site_ee, the closed loop on
the float64 oracle's env_step (free-space reach, an unreachable target), and the restatement's float32 floor, which sets
the bars of tests/test_gpu_ee.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import ee_ref
from gym_so100.vec_env import EE_CONTROL_DEFAULTS, ee_control_options      # (conftest puts the package on the path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(oracle, model):
    """the restatement under the product's default control record (SO100VecEnv(action_mode="ee_delta"))"""
    return ee_ref.EeRef(oracle, model, control=ee_control_options(None, model))


# ---------------------------------------------------------------------- struct and arguments
def test_struct_mirror_matches_library_and_header():
    from gym_so100 import _native
    lib = _native.load()
    assert _native.ABI_VERSION == 25 and lib.so100_abi_version() == 25
    assert lib.so100_ee_ctrl_bytes() == ctypes.sizeof(_native.SO100EeCtrl) == 52
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    body = re.search(r"typedef struct so100_ee_ctrl \{(.*?)\} so100_ee_ctrl;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _native.SO100EeCtrl._fields_]
    c = _native.SO100EeCtrl()
    assert c.size == 52 and c.iters == 2
    assert [c.pos_scale, c.rot_scale, c.damping, c.dq_max, c.lead_max] == \
        [np.float32(ee_ref.DEFAULTS[k]) for k in ("pos_scale", "rot_scale", "damping", "dq_max", "lead_max")]
    for fn in ("so100_ee_ctrl_bytes", "so100_ee_action", "so100_ee_jacobian"):
        assert fn in _native.EXPORTED_SYMBOLS


def _call(lib, ctrl, env=None, ptrs=(1, 1, 1, 1)):
    """so100_ee_action with fake non-NULL pointers: every check below returns before any of them is read"""
    q, a, qc, ja = (ctypes.c_void_p(p) if p else None for p in ptrs)
    rc = lib.so100_ee_action(env, None if ctrl is None else ctypes.byref(ctrl), q, a, None, qc, ja, None, None)
    return rc, lib.so100_last_error().decode()


REFUSALS = [
    (dict(iters=0), "iters outside 1..8"), (dict(iters=9), "iters outside 1..8"),
    (dict(pos_scale=0.0), "pos_scale must be finite and > 0"), (dict(pos_scale=float("nan")), "pos_scale"),
    (dict(rot_scale=-0.1), "rot_scale must be finite and >= 0"), (dict(rot_scale=float("inf")), "rot_scale"),
    (dict(damping=0.0), "damping must be finite and > 0"), (dict(damping=float("inf")), "damping"),
    (dict(dq_max=-1.0), "dq_max must be finite and > 0"), (dict(dq_max=float("nan")), "dq_max"),
    (dict(lead_max=0.0), "lead_max must be finite and > 0"), (dict(lead_max=float("inf")), "lead_max"),
    (dict(ws_lo=(0.0, 0.0, 0.7)), "workspace box"), (dict(ws_hi=(float("nan"), 1.0, 1.0)), "workspace box"),
    (dict(ws_lo=(-float("inf"), 0.0, 0.0)), "workspace box"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in REFUSALS])
def test_control_record_refusals(model, kw, text):
    from gym_so100 import _native
    lib = _native.load()
    good = dict(ee_ref.default_control(model))
    good.update(kw)
    rc, err = _call(lib, _native.SO100EeCtrl(**good))
    assert rc == -1 and "so100_ee_action" in err and text in err, err


def test_null_and_size_refusals(model):
    from gym_so100 import _native
    lib = _native.load()
    rc, err = _call(lib, None)
    assert rc == -1 and "NULL ctrl" in err
    c = _native.SO100EeCtrl(**ee_ref.default_control(model))
    c.size = 48
    c.iters = 99                                       # the size is checked first
    rc, err = _call(lib, c)
    assert rc == -1 and "so100_ee_ctrl.size 48, expected 52" in err
    c = _native.SO100EeCtrl(**ee_ref.default_control(model))
    rc, err = _call(lib, c)                            # a good record: the NULL env is what is left to refuse
    assert rc == -1 and "NULL env" in err
    assert lib.so100_ee_jacobian(None, 4, ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_void_p(1), None) == -1
    assert "so100_ee_jacobian: bad arguments" in lib.so100_last_error().decode()
    rc, err = _call(lib, _native.SO100EeCtrl(**dict(ee_ref.default_control(model), rot_scale=0.0)))
    assert "NULL env" in err                           # rot_scale may be 0


def test_vec_env_value_errors_need_no_device(monkeypatch):
    """every ValueError is raised before the library is loaded or a device touched"""
    from gym_so100 import SO100VecEnv, _native
    from gym_so100.sb3 import SO100SB3VecEnv

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_load)
    bad = [dict(action_mode="cartesian"), dict(action_mode="ee_delta", variant="ee"), dict(ee_control={"iters": 2}),
           dict(action_mode="ee_delta", ee_control={"gain": 1.0}), dict(action_mode="ee_delta", ee_control={"iters": 0}),
           dict(action_mode="ee_delta", ee_control={"iters": 2.5}), dict(action_mode="ee_delta", ee_control=[1]),
           dict(action_mode="ee_delta", ee_control={"pos_scale": 0.0}),
           dict(action_mode="ee_delta", ee_control={"damping": float("nan")}),
           dict(action_mode="ee_delta", ee_control={"rot_scale": -1.0}),
           dict(action_mode="ee_delta", ee_control={"lead_max": "x"}),
           dict(action_mode="ee_delta", ee_control={"ws_lo": (0, 0)}),
           dict(action_mode="ee_delta", ee_control={"ws_lo": (0, 0, 1.0), "ws_hi": (1, 1, 0.5)})]
    for kw in bad:
        with pytest.raises(ValueError):
            SO100VecEnv(4, **kw)
    for kw in bad[:1] + bad[2:5]:                        # (the adapter has no variant argument: it is the joint model's)
        with pytest.raises(ValueError):
            SO100SB3VecEnv(4, **kw)


def test_control_options_defaults(model):
    assert EE_CONTROL_DEFAULTS == ee_ref.DEFAULTS
    assert ee_control_options(None, model) == ee_ref.default_control(model)
    c = ee_control_options({"iters": 3, "rot_scale": 0, "ws_hi": (0.5, 0.9, 0.4)}, model)
    assert c["iters"] == 3 and c["rot_scale"] == 0.0 and c["ws_hi"] == (0.5, 0.9, 0.4)
    # the workspace default is the table geom's x / y extent (assets/so100_model.json) over z in [0, 0.6]
    from gym_so100.model import load_model_dict
    t = load_model_dict()["geoms"][0]
    assert t["name"] == "table"
    assert c["ws_lo"] == (t["pos"][0] - t["size"][0], t["pos"][1] - t["size"][1], 0.0)
    assert ee_ref.default_control(model)["ws_hi"] == (t["pos"][0] + t["size"][0], t["pos"][1] + t["size"][1], 0.6)


# ---------------------------------------------------------------------- Jacobian
def _random_poses(model, n, seed):
    rng = np.random.default_rng(seed)
    lo = np.array([model.jnt_range[j][0] for j in range(5)])
    hi = np.array([model.jnt_range[j][1] for j in range(5)])
    return lo + (hi - lo) * rng.uniform(0.02, 0.98, size=(n, 5))


def test_jacobian_matches_central_differences(model, oracle64):
    """J[:, j] = axis_j x (ee - anchor_j) against central differences (h = 1e-6: truncation ~1e-12, round-off ~1e-10)
    of the float64 oracle's site_ee on 16 random in-range poses: max |dJ| <= 1e-8; the roll column <= 1e-12"""
    r = _ref(oracle64, model)
    h, worst, roll = 1e-6, 0.0, 0.0
    for q in _random_poses(model, 16, 5):
        _, J = r.jacobian(q)
        fd = np.empty((3, 5))
        for j in range(5):
            qp, qm = q.copy(), q.copy()
            qp[j] += h
            qm[j] -= h
            fd[:, j] = (r.ee(qp) - r.ee(qm)) / (2 * h)
        worst = max(worst, np.abs(J - fd).max())
        roll = max(roll, np.abs(J[:, 4]).max())
    print(f"max |J - central differences| {worst:.3e}, max |roll column| {roll:.3e}")
    assert worst <= 1e-8
    assert roll <= 1e-12


def test_kinematics_stage_is_the_position_stage(model, oracle64):
    """ee_ref reads the frames after the oracle's kinematics stage alone: they are so100o_fwd_position's"""
    r = _ref(oracle64, model)
    q = _random_poses(model, 1, 9)[0]
    anchor, axis, ee = r.frames(q)
    d = oracle64.new_data()
    oracle64.set_state(d, list(q) + [0.0, 0.1, 0.5, 0.1, 1.0, 0.0, 0.0, 0.0], np.zeros(12), np.zeros(12))
    oracle64.call("so100o_fwd_position", model, d)
    assert np.array_equal(ee, np.array(d.site_ee[:]))
    assert np.array_equal(anchor, np.array([x[:] for x in d.xanchor]))
    assert np.array_equal(axis[:5], np.array([x[:] for x in d.xaxis])[:5])


# ---------------------------------------------------------------------- closed loop on the float64 oracle
def closed_loop(r, model, oracle64, direction, full, zero, seed=3):
    """spawn `seed`, TouchCube: `full` steps of the full-scale action (direction, 0, 0) then `zero` steps of zero action,
    each ee_ref.action (float64) then the oracle's env_step.  The goal is the first step's ee(q_cmd) moved by
    pos_scale * direction per full-scale step, clipped to the workspace as the definition clips.  Returns (goal,
    ee(q_cmd) at the end, site_ee at the end, per-step records (q [6], q_cmd [5]))."""
    d = oracle64.new_data()
    oracle64.reset(model, d, oracle64.spawn_pose(seed))
    q_cmd, goal, rec = np.zeros((1, 5), np.float32), None, []
    for k in range(full + zero):
        q = np.array(d.qpos[:], np.float64).astype(np.float32)[None]
        a = np.zeros((1, 5), np.float32)
        if k < full:
            a[0, :3] = direction
        if goal is None:
            goal = r.ee(q[0, :5].astype(np.float64))
        if k < full:
            goal = np.clip(goal + float(r.pos_scale) * np.asarray(direction, np.float64), r.ws_lo, r.ws_hi)
        qc, ja, _ = r.action(q, a, q_cmd, reinit=[k == 0])
        q_cmd = qc.astype(np.float32)
        rec.append((q[0, :6].astype(np.float64), q_cmd[0].astype(np.float64)))
        oracle64.env_step(model, d, 1, ja[0].astype(np.float32))
    return goal, r.ee(q_cmd[0].astype(np.float64)), np.array(d.site_ee[:], np.float64), rec


REACH = [(-1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (-1.0, 1.0, -0.5)]
REACH_CMD_BAR, REACH_ARM_BAR = 1e-3, 15e-3     # metres: ||ee(q_cmd) - goal||, ||site_ee - goal||


@pytest.mark.parametrize("direction", REACH, ids=[str(d) for d in REACH])
def test_free_space_reach(model, oracle64, direction):
    """8 full-scale steps then 22 of zero action: ||ee(q_cmd) - goal|| <= 1 mm, ||site_ee - goal|| <= 15 mm.
    This restatement measures 0.14 / 0.23 / 0.24 / 0.01 mm in command space and 5.1 / 8.3 / 8.6 / 5.5 mm at the arm
    for the four directions (the arm's residual is the position actuators' gravity sag, as in joint mode)."""
    r = _ref(oracle64, model)
    goal, ee_cmd, ee_arm, _ = closed_loop(r, model, oracle64, direction, 8, 22)
    e_cmd, e_arm = np.linalg.norm(ee_cmd - goal), np.linalg.norm(ee_arm - goal)
    print(f"direction {direction}: command space {1e3 * e_cmd:.3f} mm, arm {1e3 * e_arm:.3f} mm")
    assert e_cmd <= REACH_CMD_BAR
    assert e_arm <= REACH_ARM_BAR


def test_unreachable_target_does_not_wind_up(model, oracle64):
    """(1, 0, 0) for 30 steps runs into the arm's reach: at every step |q_cmd - q| <= lead_max + 1e-6 on the four
    positioning joints and q_cmd stays inside the joint ranges"""
    r = _ref(oracle64, model)
    goal, _, ee_arm, rec = closed_loop(r, model, oracle64, (1.0, 0.0, 0.0), 30, 0)
    lead = max(np.abs(qc[:4] - q[:4]).max() for q, qc in rec)
    print(f"left to the goal {np.linalg.norm(ee_arm - goal):.4f} m, max lead {lead:.6f} rad")
    assert np.linalg.norm(ee_arm - goal) > 0.05          # the target is out of reach
    assert lead <= float(r.lead_max) + 1e-6
    for _, qc in rec:
        assert (qc >= r.lo[:5]).all() and (qc <= r.hi[:5]).all()


# ---------------------------------------------------------------------- float32 floor
def test_float32_floor(model, oracle64, oracle32):
    """F = max |float32 restatement - float64 restatement| over the GPU test's states and actions; the constants of
    ee_ref (F_QCMD, F_JAC) that set the GPU bars are no smaller than what is measured here"""
    r64, r32 = _ref(oracle64, model), _ref(oracle32, model)
    qpos, q_cmd, acts = ee_ref.gpu_cases(oracle64, model, 257)
    f = np.zeros(3)
    for a in acts.values():
        out64, out32 = r64.action(qpos, a, q_cmd), r32.action(qpos, a, q_cmd)
        assert all(x.dtype == np.float32 for x in out32) and all(x.dtype == np.float64 for x in out64)
        f = np.maximum(f, [np.abs(x - y.astype(np.float64)).max() for x, y in zip(out64, out32)])
    fj = fe = 0.0
    for i in range(257):
        e64, j64 = r64.jacobian(qpos[i, :5].astype(np.float64))
        e32, j32 = r32.jacobian(qpos[i, :5])
        fj, fe = max(fj, np.abs(j64 - j32).max()), max(fe, np.abs(e64 - e32).max())
    print(f"float32 floor: q_cmd {f[0]:.3e}, joint_action {f[1]:.3e}, ee_target {f[2]:.3e}, Jacobian {fj:.3e}, "
          f"ee_site {fe:.3e}")
    assert max(f) <= ee_ref.F_QCMD
    assert max(fj, fe) <= ee_ref.F_JAC
    assert f[0] > 0 and fj > 0                           # the two precisions do differ: the floor measures something
