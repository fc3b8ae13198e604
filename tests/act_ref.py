"""numpy restatement of the device-side physical randomisation draw and of the actuation-latency model (include/so100.h
so100_dr_sample, so100_actuate), with the dtype as a parameter.  TEST INFRASTRUCTURE ONLY:
tests/test_act_cpu.py checks its properties and measures its float32 floor, tests/test_gpu_act.py checks the HIP kernels
against it.

The draws are views_ref.uniform's hash of (seed, global env id, episode, field): fields 1 mass, 2 friction, 4 delay,
5 smoothing, 6 rate."""
import numpy as np

import views_ref

MAX_DELAY, HIST = 7, 8             # SO100_ACT_MAX_DELAY, SO100_ACT_HIST
OFF = dict(delay=(0, 0), smoothing=(1.0, 1.0), rate=(2.0, 2.0))
F_MASS, F_FRICTION, F_DELAY, F_SMOOTHING, F_RATE = 1, 2, 4, 5, 6

# float32 floor of Actuator against its float64 self over the GPU test's inputs (gpu_cases: 257 envs, 20 calls), measured
# by tests/test_act_cpu.py::test_float32_floor, which prints it and fails if the measured floor passes the constant.  The
# GPU bar is 4 F_ACT + 1e-6.
F_ACT = 2.0e-7                     # measured 1.52e-07


def hash24(seed, ids, episode, field):
    """The integer behind views_ref.uniform: h >> 40 of the 64-bit hash h, so uniform = hash24 / 2^24 (exact)."""
    u = views_ref.uniform(seed, ids, episode, field)
    h = (u * float(1 << 24)).astype(np.uint64)
    assert np.array_equal(h.astype(np.float64) / float(1 << 24), u)
    return h


def draw_real(seed, ids, episode, field, rng, dtype=np.float64):
    """clip(lo + (hi - lo) u, lo, hi) in the dtype; the range is the float32 pair the device holds"""
    lo, hi = (dtype(np.float32(x)) for x in rng)
    u = views_ref.uniform(seed, ids, episode, field).astype(dtype)       # 24 bits: exact in float32
    return np.clip(lo + (hi - lo) * u, lo, hi).astype(dtype)


def draw_delay(seed, ids, episode, rng):
    """lo + (((h >> 40) * (hi - lo + 1)) >> 24), integer arithmetic"""
    lo, hi = int(rng[0]), int(rng[1])
    return lo + ((hash24(seed, ids, episode, F_DELAY) * np.uint64(hi - lo + 1)) >> np.uint64(24)).astype(np.int64)


def sample(seed, ids, episode=None, mass=(1.0, 1.0), friction=(1.0, 1.0), delay=(0, 0), smoothing=(1.0, 1.0),
           rate=(2.0, 2.0), dtype=np.float64):
    """(dr [N,2] = mass, friction; act [N,4] = delay, alpha, rate, 0) of global env ids `ids` at `episode` (None = 0)"""
    ids = np.asarray(ids, dtype=np.uint64)
    ep = np.zeros(len(ids), np.int64) if episode is None else np.asarray(episode)
    dr = np.stack([draw_real(seed, ids, ep, F_MASS, mass, dtype), draw_real(seed, ids, ep, F_FRICTION, friction, dtype)],
                  axis=1)
    act = np.stack([draw_delay(seed, ids, ep, delay).astype(dtype), draw_real(seed, ids, ep, F_SMOOTHING, smoothing, dtype),
                    draw_real(seed, ids, ep, F_RATE, rate, dtype), np.zeros(len(ids), dtype)], axis=1)
    return dr, act


class Actuator:
    """The state and the call of so100_actuate for n envs in `dtype`.  Inputs are what the kernel is given (float32 qpos,
    commands, parameters), converted to the dtype; the action ranges are converted from the model's doubles, as
    so100_create converts them to float32.  `from_hold` [n,6] marks the applied actions that descend from a `hold` value
    (which the bitwise claims leave aside: its division need not round alike on the device)."""

    def __init__(self, model, n, dtype=np.float32):
        self.dt, self.n = dtype, n
        self.lo = np.array(model.action_lo[:], np.float64).astype(np.float32).astype(dtype)
        self.hi = np.array(model.action_hi[:], np.float64).astype(np.float32).astype(dtype)
        self.hist = np.zeros((HIST, n, 6), dtype)
        self.head = np.zeros(n, np.int32)
        self.y = np.zeros((n, 6), dtype)
        self.hist_hold = np.zeros((HIST, n, 6), bool)
        self.from_hold = np.zeros((n, 6), bool)

    def hold(self, qpos):
        dt = self.dt
        q = np.asarray(qpos, np.float32).astype(dt)[:, :6]
        return np.clip(dt(2) * (q - self.lo) / (self.hi - self.lo) - dt(1), dt(-1), dt(1)).astype(dt)

    def __call__(self, qpos, command, params, reinit=None):
        """qpos [n,13], command [n,6], params [n,4] (delay, alpha, rate, -), reinit [n] or None -> applied action [n,6]"""
        dt, n = self.dt, self.n
        u = np.clip(np.asarray(command, np.float32).astype(dt), dt(-1), dt(1))
        p = np.asarray(params, np.float32)
        d = np.clip(p[:, 0], 0, MAX_DELAY).astype(np.int64)
        alpha, r = p[:, 1].astype(dt)[:, None], p[:, 2].astype(dt)[:, None]
        if reinit is not None:
            re = np.asarray(reinit).astype(bool)
            if re.any():
                h = self.hold(qpos)
                self.hist[:, re] = h[re]
                self.hist_hold[:, re] = True
                self.y[re] = h[re]
                self.from_hold[re] = True
                self.head[re] = 0
        e = np.arange(n)
        slot = self.head.astype(np.int64) % HIST
        self.hist[slot, e] = u
        self.hist_hold[slot, e] = False
        rd = (self.head.astype(np.int64) - d) % HIST
        v, v_hold = self.hist[rd, e], self.hist_hold[rd, e]
        self.head = self.head + np.int32(1)
        y = self.y
        w = np.where(alpha == dt(1), v, y + alpha * (v - y)).astype(dt)
        dy = w - y
        self.y = np.where(np.abs(dy) <= r, w, y + np.copysign(r, dy)).astype(dt)
        exact = (alpha == dt(1)) & (np.abs(dy) <= r)            # y is v itself
        self.from_hold = np.where(exact, v_hold, self.from_hold | v_hold)
        assert self.y.dtype == dt and self.hist.dtype == dt
        return self.y.copy()


# ---------------------------------------------------------------------- shared test inputs
CALLS = 20
_CASES = {}


def gpu_cases(qpos257, n=257):
    """The GPU test's inputs for the first n of 257 envs, from qpos257 [257,13] (ee_ref.rollout_states): per call a qpos
    (the rollout's state with the arm joints moved by U(-0.2, 0.2), so every re-initialisation holds another pose), a
    command in [-1.2, 1.2] (the clip is exercised) and a reinit byte (call 0: every env; later: 1 in 8, scattered), and per
    env the parameters sample() draws over delay (0, 7), smoothing (0.3, 1), rate (0.05, 2) with every fourth env's alpha
    set to 1 and rate to 2 (the envs the bitwise claim covers).  Returns (qpos [CALLS,n,13], command [CALLS,n,6], reinit
    [CALLS,n] uint8, params [n,4]), float32."""
    if "cases" not in _CASES:
        rng = np.random.default_rng(23)
        q = np.repeat(np.asarray(qpos257, np.float32)[None], CALLS, axis=0)
        q[:, :, :6] += rng.uniform(-0.2, 0.2, size=(CALLS, 257, 6)).astype(np.float32)
        cmd = rng.uniform(-1.2, 1.2, size=(CALLS, 257, 6)).astype(np.float32)
        re = (rng.uniform(size=(CALLS, 257)) < 0.125).astype(np.uint8)
        re[0] = 1
        _, act = sample(5, np.arange(257), None, delay=(0, 7), smoothing=(0.3, 1.0), rate=(0.05, 2.0), dtype=np.float32)
        act[::4, 1], act[::4, 2] = 1.0, 2.0
        _CASES["cases"] = (q, cmd, re, act.astype(np.float32))
    q, cmd, re, act = _CASES["cases"]
    return q[:, :n].copy(), cmd[:, :n].copy(), re[:, :n].copy(), act[:n].copy()
