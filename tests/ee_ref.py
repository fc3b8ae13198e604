"""numpy restatement of the Cartesian end-effector action mode (include/so100.h so100_ee_action), with
the precision as a parameter: every quantity is computed in the dtype of the oracle it is given (Oracle(64): float64,
Oracle(32): float32), on that oracle's kinematics (Data.xanchor, Data.xaxis, Data.site_ee after the kinematics stage).
TEST INFRASTRUCTURE ONLY: tests/test_ee_cpu.py checks it against the oracle, tests/test_gpu_ee.py checks the HIP kernel
against it.

Inputs are what the kernel is given: float32 qpos, actions, q_cmd and the float32 control record, converted to the dtype;
the model's joint ranges are converted from the model's doubles, as so100_create converts them to float32.
"""
import ctypes

import numpy as np

# so100_ee_ctrl's defaults (include/so100.h; pos_scale and rot_scale: the reference's scripts/teleop_ee.py:53-64 key
# steps, 0.01 m and 10 degrees)
DEFAULTS = dict(iters=2, pos_scale=0.01, rot_scale=0.17453292, damping=0.02, dq_max=0.2, lead_max=0.5)
WS_Z = (0.0, 0.6)                 # the workspace box's z range over the table's x / y extent

# float32 floors of this restatement against its float64 self, over the GPU test's states and actions (gpu_cases(257):
# 2 x 257 envs), measured by tests/test_ee_cpu.py::test_float32_floor, which prints them and fails if a measured floor
# passes its constant.  The GPU bars are 4 F + 1e-6 (q_cmd, joint_action, ee_target) and 4 F_J + 1e-7 (Jacobian, ee).
F_QCMD = 2.5e-6                   # measured 2.08e-06 on q_cmd (joint_action 1.28e-06, ee_target 1.66e-07)
F_JAC = 2.0e-7                    # measured 1.75e-07 on the Jacobian (ee_site 1.52e-07)

STAGE_KIN = 0                     # oracle/so100_oracle.h SO100O_STAGE_KIN


def default_control(model):
    """The default control record as a dict: DEFAULTS plus the workspace box (the table's x / y extent, z in WS_Z)."""
    c = dict(DEFAULTS)
    c["ws_lo"] = (float(model.table_lo[0]), float(model.table_lo[1]), WS_Z[0])
    c["ws_hi"] = (float(model.table_hi[0]), float(model.table_hi[1]), WS_Z[1])
    return c


class EeRef:
    def __init__(self, oracle, model, control=None):
        self.o, self.model, self.dt = oracle, model, oracle.np_real
        self.d = oracle.new_data()
        self.d.qpos[9] = 1.0      # the cube's quaternion: identity (the arm's kinematics do not read it)
        c = default_control(model)
        c.update(control or {})
        dt = self.dt
        self.iters = int(c["iters"])
        for k in ("pos_scale", "rot_scale", "damping", "dq_max", "lead_max"):
            setattr(self, k, dt(np.float32(c[k])))
        self.ws_lo = np.asarray(c["ws_lo"], np.float32).astype(dt)
        self.ws_hi = np.asarray(c["ws_hi"], np.float32).astype(dt)
        self.lo = np.array([model.jnt_range[j][0] for j in range(6)], np.float64).astype(dt)
        self.hi = np.array([model.jnt_range[j][1] for j in range(6)], np.float64).astype(dt)
        oracle.lib.so100o_stage.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]

    # ------------------------------------------------------------------ kinematics (the oracle's)
    def frames(self, q5):
        """(anchor [6,3], axis [6,3], site_ee [3]) with the five arm joints at q5, in the oracle's precision"""
        d = self.d
        for k in range(5):
            d.qpos[k] = q5[k].item() if hasattr(q5[k], "item") else q5[k]
        self.o.lib.so100o_stage(self.o._p(self.model), self.o._p(d), STAGE_KIN)
        dt = self.dt
        return (np.array([r[:] for r in d.xanchor], dt), np.array([r[:] for r in d.xaxis], dt),
                np.array(d.site_ee[:], dt))

    def ee(self, q5):
        return self.frames(q5)[2]

    def jacobian(self, q5):
        """(site_ee [3], J [3,5]): J[:, j] = axis_j x (ee - anchor_j) for joints 0..4"""
        anchor, axis, ee = self.frames(q5)
        J = np.stack([np.cross(axis[j], ee - anchor[j]) for j in range(5)], axis=1).astype(self.dt)
        return ee, J

    # ------------------------------------------------------------------ the solve
    def dls(self, J, e):
        """J' (J J' + damping^2 I)^-1 e by Cholesky, in the dtype"""
        dt = self.dt
        A = (J @ J.T + self.damping * self.damping * np.eye(3, dtype=dt)).astype(dt)
        l00 = np.sqrt(A[0, 0]); l10 = A[1, 0] / l00; l20 = A[2, 0] / l00
        l11 = np.sqrt(A[1, 1] - l10 * l10); l21 = (A[2, 1] - l20 * l10) / l11
        l22 = np.sqrt(A[2, 2] - l20 * l20 - l21 * l21)
        y0 = e[0] / l00; y1 = (e[1] - l10 * y0) / l11; y2 = (e[2] - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22; x1 = (y1 - l21 * x2) / l11; x0 = (y0 - l10 * x1 - l20 * x2) / l00
        return (J.T @ np.array([x0, x1, x2], dt)).astype(dt)

    def action_one(self, q, a, q_cmd, reinit):
        """One env: q [6], a [5], q_cmd [5] in the dtype -> (q_cmd [5], joint_action [6], ee_target [3])"""
        dt = self.dt
        a = np.clip(a, dt(-1), dt(1))
        qc = q[:5].copy() if reinit else q_cmd.copy()
        p = np.clip(self.ee(qc) + self.pos_scale * a[:3], self.ws_lo, self.ws_hi)
        c = qc.copy()                                         # joints 0..3 move; c[4] stays the commanded roll
        for _ in range(self.iters):
            ee, J = self.jacobian(c)
            dq = self.dls(J[:, :4], p - ee)
            dq = dq * (self.dq_max / np.maximum(np.max(np.abs(dq)), self.dq_max))
            c[:4] = np.clip(c[:4] + dq, self.lo[:4], self.hi[:4])
        qc[:4] = q[:4] + np.clip(c[:4] - q[:4], -self.lead_max, self.lead_max)
        qc[4] = np.clip(qc[4] + self.rot_scale * a[3], self.lo[4], self.hi[4])
        ja = np.empty(6, dt)
        ja[:5] = np.clip(dt(2) * (qc - self.lo[:5]) / (self.hi[:5] - self.lo[:5]) - dt(1), dt(-1), dt(1))
        ja[5] = a[4]
        assert qc.dtype == dt and ja.dtype == dt and p.dtype == dt
        return qc, ja, p

    def action(self, qpos, action, q_cmd, reinit=None):
        """The batched call: qpos [N,13], action [N,5], q_cmd [N,5] (float32, as the kernel takes them), reinit [N] or
        None -> (q_cmd [N,5], joint_action [N,6], ee_target [N,3]) in the dtype"""
        dt = self.dt
        qpos, action, q_cmd = (np.asarray(x, np.float32).astype(dt) for x in (qpos, action, q_cmd))
        n = qpos.shape[0]
        out = [self.action_one(qpos[i, :6], action[i], q_cmd[i], reinit is not None and bool(reinit[i]))
               for i in range(n)]
        return tuple(np.stack([o[k] for o in out]) for k in range(3))


# ---------------------------------------------------------------------- shared test inputs
_CASES = {}


def rollout_states(oracle64, model, n, steps=25, seed=7):
    """qpos [n,13] float32 after a `steps`-step random joint-mode rollout of the float64 oracle from the spawns of seeds
    seed .. seed + n - 1 (TouchCube task), computed once per n"""
    key = ("states", n, steps, seed)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        acts = rng.uniform(-1, 1, size=(steps, n, 6)).astype(np.float32)
        datas = (oracle64.Data * n)()
        for i in range(n):
            oracle64.reset(model, datas[i], oracle64.spawn_pose(seed + i))
        oracle64.batch_run(model, datas, n, steps, 1, acts, 0)
        q = np.array([datas[i].qpos[:] for i in range(n)], np.float64)
        assert np.isfinite(q).all()
        _CASES[key] = q.astype(np.float32)
    return _CASES[key].copy()


def gpu_cases(oracle64, model, n=257):
    """The GPU tests' inputs, the first n of 257 envs: qpos from rollout_states, q_cmd = qpos[:, :5] + U(-0.1, 0.1)
    clipped to the joint ranges, and two action sets: uniform random in [-1.2, 1.2] (the clip is exercised) and every
    component at +-1.  Returns (qpos [n,13], q_cmd [n,5], {"random": [n,5], "corners": [n,5]}), float32."""
    key = ("cases", 257)
    if key not in _CASES:
        qpos = rollout_states(oracle64, model, 257)
        rng = np.random.default_rng(11)
        lo = np.array([model.jnt_range[j][0] for j in range(5)])
        hi = np.array([model.jnt_range[j][1] for j in range(5)])
        q_cmd = np.clip(qpos[:, :5] + rng.uniform(-0.1, 0.1, size=(257, 5)), lo, hi).astype(np.float32)
        acts = {"random": rng.uniform(-1.2, 1.2, size=(257, 5)).astype(np.float32),
                "corners": rng.choice(np.array([-1.0, 1.0], np.float32), size=(257, 5)).astype(np.float32)}
        _CASES[key] = (qpos, q_cmd, acts)
    qpos, q_cmd, acts = _CASES[key]
    return qpos[:n].copy(), q_cmd[:n].copy(), {k: v[:n].copy() for k, v in acts.items()}
