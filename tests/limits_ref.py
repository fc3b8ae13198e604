"""State recipes and oracle probes of the joint-limit parity classes (TEST INFRASTRUCTURE, numpy + the CPU oracle only).

Shared by tests/test_gpu_limits.py, which steps the states on the GPU, and tests/test_limits_cpu.py, which checks on the
oracles alone that the states are what the classes say (layout, impedance zones, binding substeps, the fp32 edge) and
that the wrong models the GPU tests are meant to catch sit far from the right one.  DESIGN.md §5.

Every state is (qpos [13], qvel [12], qacc_warmstart [12]) in float64 holding fp32 values; the cube is parked clear of
everything (CUBE_PARK, as test_hull_table_parity parks it), and the action of a state holds its arm pose, each joint's
target clipped to its range.  A joint-limit row exists while a hinge is beyond an end of its range (margin 0:
dist = q - lo or hi - q below 0); its impedance climbs over the first `jnt_solimp[2]` (1e-3 rad) of depth (the ramp)
and is constant beyond (the plateau).
"""
import itertools

import numpy as np

from gym_so100.model import SO100Model

NH = 6
CUBE_PARK = np.array([2.0, 0.95, 0.6, 1, 0, 0, 0])
N = 46                       # no multiple of 4 (a ragged last fused wave) nor of 16 (a partly filled last PGS wave)
STEPS = 3
DEPTH = (1e-5, 4e-2)         # rad beyond the stop, log-uniform
EFC_LIMIT = 1                # oracle/so100_oracle.h SO100O_EFC_LIMIT
F32 = np.float32


def r32(x):
    """x rounded to fp32, as float64"""
    return np.asarray(x, np.float64).astype(F32).astype(np.float64)


def ranges(model):
    """(lo, hi) [6] of the hinges in float64 as the fp64 oracle reads them"""
    return np.array([r[0] for r in model.jnt_range]), np.array([r[1] for r in model.jnt_range])


def hold_action(model, arm):
    """the normalised action [6] float32 whose targets are the arm pose clipped to the joints' ranges"""
    lo, hi = ranges(model)
    alo, ahi = np.array(model.action_lo[:]), np.array(model.action_hi[:])
    return np.clip((np.clip(arm, lo, hi) - alo) / (ahi - alo) * 2 - 1, -1, 1).astype(F32)


def predicted_rows(model, qpos):
    """the kernel's rule restated: per hinge +1 (a row at the lower stop), -1 (at the upper stop) or 0, from the fp32
    joint position against the fp32-rounded range in fp32 arithmetic"""
    lo, hi = ranges(model)
    q = np.asarray(qpos, np.float64)[..., :NH].astype(F32)
    dlo, dhi = q - lo.astype(F32), hi.astype(F32) - q
    return np.where(dlo < 0, 1, np.where(dhi < 0, -1, 0))


# ------------------------------------------------------------------ wrong models
def widened(model, by=1.0):
    """every hinge range widened by `by` rad at both ends: no limit row at all (the kernel with its lim_on branch deleted)"""
    m = SO100Model.from_buffer_copy(model)
    for j in range(NH):
        m.jnt_range[j][0] -= by
        m.jnt_range[j][1] += by
    return m


def solref_scaled(model, f=1.1):
    """the limit rows' time constant times f (their K and B)"""
    m = SO100Model.from_buffer_copy(model)
    m.jnt_solref[0] *= f
    return m


def invweight_scaled(model, f=1.1):
    """the hinges' dof_invweight0 times f (the limit rows' R; the frictionloss rows' too)"""
    m = SO100Model.from_buffer_copy(model)
    for j in range(NH):
        m.dof_invweight0[j] *= f
    return m


def solimp_scaled(model, f):
    """the limit rows' impedance at depth 0 times f: moves the rows on the impedance ramp only"""
    m = SO100Model.from_buffer_copy(model)
    m.jnt_solimp[0] *= f
    return m


# ------------------------------------------------------------------ oracle probes
def step(oracle, model, state, action, rows=True):
    """One env step of `oracle`: (qpos, qvel, last_solve record, limit rows of the last substep's solve, their forces
    [6]: 0 where the hinge holds no row).  The env step's final position stage rebuilds the constraint rows, so the
    limit rows are read from a replay of its substeps (trace), which must end on the very qacc that the env step
    recorded for its last solve.  rows=False leaves the replay out (None, None)."""
    d = oracle.new_data()
    oracle.set_state(d, state[0], state[1], state[2])
    oracle.env_step(model, d, 0, np.asarray(action, F32))
    q, v = oracle.get_state(d)[:2]
    sol = oracle.last_solve(d)
    if not rows:
        return q, v, sol, None, None
    _, hinges, f, qacc = trace(oracle, model, state, action)[-1]
    assert np.array_equal(qacc, sol[3]), "the replayed substeps are not the env step's own"
    limf = np.zeros(NH)
    limf[hinges] = f
    return q, v, sol, len(hinges), limf


def trace(oracle, model, state, action, nsub=None):
    """The substeps of one env step, one at a time: per substep (arm qpos [6] the substep starts from, the hinges of
    its limit rows, their forces, the qacc [12] of its solve).  nsub: the number of substeps (default model.nsubstep)."""
    d = oracle.new_data()
    oracle.set_state(d, state[0], state[1], state[2])
    ctrl = oracle.unnormalize(model, action)
    for k in range(NH):
        d.ctrl[k] = float(ctrl[k])
    out = []
    for _ in range(model.nsubstep if nsub is None else nsub):
        q = np.array(d.qpos[:NH], np.float64)
        oracle.call("so100o_substep", model, d)
        rows = [i for i in range(d.nefc) if d.efc_type[i] == EFC_LIMIT]
        out.append((q, [d.efc_id[i] for i in rows], [d.efc_force[i] for i in rows], np.array(d.qacc[:], np.float64)))
    return out


def stop_margin(model, q):
    """the least distance [rad] of any hinge of arm pose q from an end of its range"""
    lo, hi = ranges(model)
    return min(np.abs(q[:NH] - lo).min(), np.abs(q[:NH] - hi).min())


def last_substep_margin(oracle64, model, state, action):
    """stop_margin of the pose the fp64 oracle's last substep of this env step starts from: where it is above 1e-6 the
    fp32 kernel and the fp64 oracle must hold the same limit rows in that substep"""
    return stop_margin(model, trace(oracle64, model, state, action)[-1][0])


def closed_loop(oracle, model, states, acts, steps=STEPS):
    """the states [steps][n] of `oracle`'s own run of the fixed actions, rounded to fp32 after each env step (the
    teacher-forced GPU steps start from fp32 states)"""
    out, cur = [], list(states)
    for _ in range(steps):
        out.append(cur)
        nxt = []
        for st, a in zip(cur, acts):
            d = oracle.new_data()
            oracle.set_state(d, *st)
            oracle.env_step(model, d, 0, a)
            q, v, w, _ = oracle.get_state(d)
            nxt.append((r32(q), r32(v), r32(w)))
        cur = nxt
    return out


# ------------------------------------------------------------------ a / b. seeded beyond the stop
TELL = 1e-4                  # the least wrong-model distance of a kept draw: 10 x the classes' median bar of 1e-5, the
                             # least at which the one-tenth criterion can hold for a GPU at the bar (test_gpu_dr.py)
SOLIMP_F = 1.02              # the factor of the jnt_solimp[0] wrong model (graded on the ramp states)


def qv_distance(oracle64, model, wrong, state, action):
    """the relative qvel distance max |vw - v| / (1 + |v|) of model `wrong` from `model` after one env step"""
    v, vw = step(oracle64, model, state, action, rows=False)[1], step(oracle64, wrong, state, action, rows=False)[1]
    return (np.abs(vw - v) / (1 + np.abs(v))).max()


def one_substep(model):
    m = SO100Model.from_buffer_copy(model)
    m.nsubstep = 1
    return m


def whole_step(model):
    """the model with the env's substeps per env step (build_model's default)"""
    from gym_so100 import constants as C
    m = SO100Model.from_buffer_copy(model)
    m.nsubstep = int(round(C.DT / model.timestep))
    return m


def off_table(oracle64, model, state, action):
    """Whether the arm stays clear of the table over the fp64 oracle's own STEPS closed-loop env steps, of one substep
    and of the whole number: no contact bit (the cube's pairs and the hull-table pairs 14..22) after any of them.
    The classes here are about the limit rows; a link folded over the table's edge is test_table_edge_parity's matter,
    and there the kernel's contact bits differ from the oracle's (joint-limit rows)."""
    d = oracle64.new_data()
    for m in (one_substep(model), whole_step(model)):
        oracle64.set_state(d, *state)
        for _ in range(STEPS):
            oracle64.env_step(m, d, 0, action)
            if oracle64.contact_bits(d):
                return False
    return True


def _arm_pose(model, rng):
    lo, hi = ranges(model)
    return np.clip(np.array(model.start_qpos[:]) + rng.normal(0, 0.15, NH), lo + 0.05, hi - 0.05)


def _state(arm, qvel6):
    qpos = np.concatenate([arm, CUBE_PARK])
    qvel = np.concatenate([qvel6, np.zeros(6)])
    return r32(qpos), r32(qvel), np.zeros(12)


def _beyond_one(oracle64, model, rng, rows, depth_hi=DEPTH[1]):
    """one class-a state with the (hinge, side) rows given (side 0: the lower stop), redrawn until the arm is off_table:
    (state, [(hinge, side, depth)]), or None after 8 draws (the rows that can be drawn at all succeed in 7 of 10)"""
    for _ in range(8):
        st, me = _beyond_draw(model, rng, rows, depth_hi)
        if off_table(oracle64, model, st, hold_action(model, st[0][:NH])):
            return st, me
    return None


def _beyond_draw(model, rng, rows, depth_hi):
    lo, hi = ranges(model)
    arm = _arm_pose(model, rng)
    vel = rng.normal(0, 0.5, NH)
    meta = []
    for k, (j, side) in enumerate(rows):
        depth = float(np.exp(rng.uniform(np.log(DEPTH[0]), np.log(depth_hi))))
        arm[j] = lo[j] - depth if side == 0 else hi[j] + depth
        # the first row of an env moves into its stop, the others do so two times in three, so that two thirds or more
        # of the rows push (a releasing row's force is 0, and with it every wrong model's distance)
        v = abs(rng.normal(0, 2.0)) * (1 if k == 0 or rng.uniform() < 2 / 3 else -1)
        v = v if side else -v
        vel[j] = v
        meta.append((j, side, depth))
    return _state(arm, vel), meta


def _beyond_kept(oracle64, model, wrong, rng, rows, depth_hi=DEPTH[1]):
    """_beyond_one redrawn until, on the fp64 oracle, the wrong model (of the one-substep model) sits TELL or more from
    the right one after one substep: an env none of whose rows pushes tells no wrong model apart"""
    m1 = one_substep(model)
    w1 = wrong(m1)
    for _ in range(8):
        kept = _beyond_one(oracle64, model, rng, rows, depth_hi)
        if kept is not None and qv_distance(oracle64, m1, w1, kept[0], hold_action(model, kept[0][0][:NH])) >= TELL:
            return kept
    return None


def _layout(n, rng):
    """Per env the (hinge, side) rows: none for every fourth env (i % 4 == 3: one env of each fused wave), otherwise 1 to
    3 hinges, the hinge sets pairwise distinct within each block of 16 consecutive envs (a PGS wave), sides at random."""
    subsets = [c for k in (1, 2, 3) for c in itertools.combinations(range(NH), k)]
    rows = [[] for _ in range(n)]
    for b0 in range(0, n, 16):
        envs = [i for i in range(b0, min(b0 + 16, n)) if i % 4 != 3]
        pick = rng.permutation(len(subsets))[:len(envs)]
        for i, s in zip(envs, pick):
            hinges = rng.permutation(subsets[s])
            rows[i] = [(int(j), int(rng.integers(2))) for j in hinges]
    return rows


def beyond_states(oracle64, model, n=N, seed=101, ramp=False):
    """Class a: the arm at start_qpos + N(0, 0.15) (0.05 rad or more inside the ranges), then 1 to 3 hinges per env beyond
    an end of their range by a depth log-uniform in DEPTH, joint velocities N(0, 0.5) rad/s and N(0, 2) on the limited
    hinges.  The layout is _layout's, redrawn until each of the 12 (hinge, side) combinations occurs twice or more and every
    env's rows can be drawn; an env's pose and velocities are redrawn until the arm stays clear of the table (off_table)
    and, for a limited env, the model without limits is told apart (_beyond_kept).
    An env whose rows cannot be drawn so (the shoulder or the elbow alone at its upper stop lays the arm on the table)
    takes another hinge set that its block does not hold yet; these two stops occur together with other hinges' rows.
    ramp: every depth log-uniform in [1e-5, 0.9e-3) instead, on the impedance ramp, and the draws kept are those that
    tell the jnt_solimp[0] x SOLIMP_F model apart (it moves nothing else); the count of the combinations is class a's
    condition alone.
    Returns (states, meta, actions [n, 6]); meta[i] = [(hinge, side, depth)]."""
    rng = np.random.default_rng(seed)
    wrong = (lambda m: solimp_scaled(m, SOLIMP_F)) if ramp else widened
    depth_hi = 0.9 * model.jnt_solimp[2] if ramp else DEPTH[1]
    subsets = [c for k in (1, 2, 3) for c in itertools.combinations(range(NH), k)]
    for _ in range(50):
        rows = _layout(n, rng)
        states, meta = [], []
        for i in range(n):
            kept = _beyond_kept(oracle64, model, wrong, rng, rows[i], depth_hi) if rows[i] else \
                _beyond_one(oracle64, model, rng, [])
            while kept is None:
                # these rows fold the arm onto the table or the Base whatever the pose (the shoulder or the elbow alone at
                # its upper stop): the env draws another hinge set, none that its block of 16 holds already
                b0 = i - i % 16
                used = {frozenset(j for j, _ in rows[k]) for k in range(b0, min(b0 + 16, n)) if k != i}
                free = [c for c in subsets if frozenset(c) not in used]
                rows[i] = [(int(j), int(rng.integers(2))) for j in rng.permutation(free[rng.integers(len(free))])]
                kept = _beyond_kept(oracle64, model, wrong, rng, rows[i], depth_hi)
            states.append(kept[0])
            meta.append(kept[1])
        count = np.zeros((NH, 2), int)
        for r in rows:
            for j, side in r:
                count[j, side] += 1
        if count.min() >= 2 or ramp:
            break
    assert count.min() >= 2 or ramp
    return states, meta, np.array([hold_action(model, s[0][:NH]) for s in states])


# ------------------------------------------------------------------ c. approach
def approach_states(oracle64, model, n=N, seed=202):
    """Class c: one hinge per env 0.002 to 0.03 rad inside a stop and moving towards it at 2 to 8 rad/s, everything else at
    rest; kept are the draws in which the fp64 oracle's own substeps show that hinge's row off at substep 1 and on by
    substep 8, and in which the model without limits stays TELL or more away at each of the fp64 oracle's own STEPS
    closed-loop env steps (a hinge that a contact stops short of its stop, or that has bounced back inside, tells no
    wrong model apart).  Returns (states, meta, actions, first binding substep per state (1-based), draws)."""
    rng = np.random.default_rng(seed)
    lo, hi = ranges(model)
    wide = widened(model)
    states, meta, first, draws = [], [], [], 0
    while len(states) < n:
        draws += 1
        assert draws <= 4 * n
        arm = _arm_pose(model, rng)
        j, side = (draws - 1) % NH, ((draws - 1) // NH) % 2
        gap, speed = rng.uniform(0.002, 0.03), rng.uniform(2.0, 8.0)
        arm[j] = lo[j] + gap if side == 0 else hi[j] - gap
        vel = np.zeros(NH)
        vel[j] = -speed if side == 0 else speed
        st = _state(arm, vel)
        act = hold_action(model, st[0][:NH])
        on = [j in t[1] for t in trace(oracle64, model, st, act)]
        if on[0] or not any(on[:8]) or not off_table(oracle64, model, st, act):
            continue
        run = closed_loop(oracle64, model, [st], [act])
        if min(qv_distance(oracle64, model, wide, s[0], act) for s in run) < TELL:
            continue
        states.append(st)
        meta.append([(j, side, -gap)])
        first.append(1 + on.index(True))
    return states, meta, np.array([hold_action(model, s[0][:NH]) for s in states]), np.array(first), draws


# ------------------------------------------------------------------ d. limit rows together with contacts
N_CONTACT = 26               # the 24 asked for and two more: no multiple of 4


def contact_states(oracle64, model, n=N_CONTACT, seed=404):
    """Class d: class-a draws (every env limited) whose first position stage holds a contact and drops none.
    Returns (states, meta, actions, draws)."""
    rng = np.random.default_rng(seed)
    subsets = [c for k in (1, 2, 3) for c in itertools.combinations(range(NH), k)]
    d = oracle64.new_data()
    states, meta, draws = [], [], 0
    while len(states) < n:
        draws += 1
        assert draws <= 40 * n
        rows = [(int(j), int(rng.integers(2))) for j in rng.permutation(subsets[rng.integers(len(subsets))])]
        kept = _beyond_one(oracle64, model, rng, rows)
        if kept is None:
            continue
        st, me = kept
        oracle64.set_state(d, *st)
        oracle64.call("so100o_fwd_position", model, d)
        if d.ncon >= 1 and not d.ncon_dropped:
            states.append(st)
            meta.append(me)
    return states, meta, np.array([hold_action(model, s[0][:NH]) for s in states]), draws


# ------------------------------------------------------------------ e. the fp32 edge
N_EDGE = 18
# (hinge, side) of the envs one ulp inside, then of those one ulp outside (the shoulder and the elbow at their upper
# stops lay the arm on the table: off_table)
EDGES = [(0, 0), (0, 1), (1, 0), (3, 1), (2, 0), (4, 1), (3, 0), (5, 1),
         (1, 0), (5, 1), (2, 0), (0, 1), (4, 0), (3, 1), (5, 0), (4, 1)]


def edge_states(oracle64, model, seed=505):
    """Class e: class-a poses without a limit, then one hinge per env exactly one fp32 ulp inside float32(limit) (envs
    0..7) or one ulp outside (envs 8..15), moving into the stop at 1 rad/s; the last two envs carry no edge.  Both stops
    occur in each group.  Returns (states, meta, actions, expected rows per env); meta[i] = [(hinge, side, +1 inside / -1
    outside)]."""
    rng = np.random.default_rng(seed)
    lo, hi = ranges(model)
    lo32, hi32 = lo.astype(F32), hi.astype(F32)
    states, meta, rows = [], [], []
    i = tries = 0
    while i < N_EDGE:
        tries += 1
        assert tries <= 40 * N_EDGE
        arm = _arm_pose(model, rng)
        vel = rng.normal(0, 0.5, NH)
        me = []
        if i < 16:
            j, side = EDGES[i]
            inside = i < 8
            if side == 0:
                q = np.nextafter(lo32[j], F32(np.inf if inside else -np.inf))
            else:
                q = np.nextafter(hi32[j], F32(-np.inf if inside else np.inf))
            arm[j] = float(q)
            vel[j] = -1.0 if side == 0 else 1.0
            me = [(j, side, 1 if inside else -1)]
        st = _state(arm, vel)
        if not off_table(oracle64, model, st, hold_action(model, st[0][:NH])):
            continue
        states.append(st)
        meta.append(me)
        rows.append(0 if (i >= 16 or i < 8) else 1)
        i += 1
    return states, meta, np.array([hold_action(model, s[0][:NH]) for s in states]), np.array(rows)


# ------------------------------------------------------------------ the classes, as both test files run them
NSUBSTEP = {"a": 1, "b": None, "c": None, "d": 1, "e": 1, "ramp": 1}      # None: the model's 10 substeps per env step

# Per class the wrong models its states must tell from the right one: name -> (copy of the model, the env steps
# graded).  The model without limits and the one with the rows' time constant x 1.1 are graded on every env step of
# the limited envs.  The rows' R x 1.1 moves a result by (1 - imp) of what the row itself does: it reaches 100 x the
# bar only in the env step in which the rows do their work, the first (measured: profiles/limit_rows.txt), and only
# over a whole env step (not in class a's single substep).  The impedance at depth 0 moves only rows on the ramp,
# which a pushed hinge leaves within one substep: graded on the ramp states' first substep.
WRONG = {
    "a": {"no limit rows": (widened, STEPS), "solref[0] x 1.1": (solref_scaled, STEPS)},
    "b": {"no limit rows": (widened, STEPS), "solref[0] x 1.1": (solref_scaled, STEPS),
          "invweight0 x 1.1": (invweight_scaled, 1)},
    "c": {"no limit rows": (widened, STEPS), "solref[0] x 1.1": (solref_scaled, STEPS),
          "invweight0 x 1.1": (invweight_scaled, 1)},
    "ramp": {f"solimp[0] x {SOLIMP_F}": (lambda m: solimp_scaled(m, SOLIMP_F), 1)},
    "d": {}, "e": {},
}


_CASES = {}


def cases(cls, oracle64, model):
    """(states, meta, actions [n, 6], info) of a class; info: what the class's recipe reports besides.  The states are
    drawn once per process on the Newton model (MuJoCo's solver) with the class's substeps, whichever solver `model`
    runs: both solvers are graded on the same states, and classes a and b share theirs."""
    from gym_so100.model import build_model
    key = "a" if cls == "b" else cls
    if key not in _CASES:
        _CASES[key] = _cases(key, oracle64, build_model(nsubstep=model.nsubstep))
    return _CASES[key]


def _cases(cls, oracle64, model):
    if cls in ("a", "b"):
        return beyond_states(oracle64, model) + ({},)
    if cls == "ramp":
        return beyond_states(oracle64, model, seed=303, ramp=True) + ({},)
    if cls == "c":
        s, m, a, first, draws = approach_states(oracle64, model)
        return s, m, a, dict(first=first, draws=draws)
    if cls == "d":
        s, m, a, draws = contact_states(oracle64, model)
        return s, m, a, dict(draws=draws)
    s, m, a, rows = edge_states(oracle64, model)
    return s, m, a, dict(rows=rows)


def graded(meta, steps, n_steps=STEPS):
    """the mask [n_steps * n] (step-major, as TF.states) of the env steps a wrong model is graded on: the limited envs'
    first `steps` env steps (an env without a limit row is at distance 0 from every wrong model)"""
    lim = np.array([len(me) > 0 for me in meta])
    return np.concatenate([lim if s < steps else np.zeros(len(meta), bool) for s in range(n_steps)])
