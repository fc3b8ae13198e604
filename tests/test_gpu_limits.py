"""GPU parity of the joint-limit constraint rows of the six arm hinges against the fp64 oracle.  DESIGN.md §5.

No other GPU test switches these rows on: the arm states of test_gpu_parity.py and test_gpu_dr.py are drawn inside the
ranges, and the position actuators target the ranges' own ends.  Here the states are made by tests/limits_ref.py from the
fp64 oracle alone (tests/test_limits_cpu.py checks them without a GPU), every class with both solvers, 46 envs (26 with
contacts, 18 at the edge: no multiple of 4, so the last fused wave is ragged and the last PGS wave partly filled), 3
teacher-forced env steps through test_gpu_parity's _step_all_builds (the fused builds 2 and 3, the split path and the
debug build bitwise equal), the cube parked clear of everything, the actions holding the arm pose:

a. 1 to 3 hinges per env seeded 1e-5 .. 4e-2 rad beyond a stop (0.58 of them on the impedance ramp, the rest on the
   plateau), some rows pushing and some releasing, one substep per env step; every fourth env without a row and the
   limited hinges differing within every 16 envs, which grades the fused kernel's lim_mask group shift and the PGS
   kernel's per-wave row mask;
b. the same states over whole env steps (10 substeps: rows switch off as the hinges are pushed back);
c. one hinge per env running into its stop at 2 to 8 rad/s: the row is off at substep 1 and on by substep 8;
d. class-a states that also hold a contact: frictionloss, limit and contact rows in one solve;
e. a hinge exactly one fp32 ulp inside or outside float32(limit).

Each class asserts the row count of the last substep (debug record: dbg[3] - 12 - 4 * dbg[0]) against the oracle's, the
bars of test_gpu_dr._step_parity_bars and test_gpu_parity._force_bars unchanged, and (`*_discrimination`, the scheme of
test_gpu_dr.py) that its states tell the right model from the wrong ones of limits_ref.WRONG: the model without limit
rows, which is the kernel with its lim_on branch deleted, sits 0.13 (one substep) to 1.0 .. 2.9 (an env step) from the
right one in relative qvel at the median, 10^4 .. 10^5 x the bar, so a kernel without the rows cannot pass.  The runs
are shared between a class's tests (module cache).

Every draw keeps the arm clear of the table on the fp64 oracle's own steps (limits_ref.off_table): a link folded over
the table's edge is test_table_edge_parity's matter, and after such a step the kernel's hull-table contact bits differ
from the oracle's, which these classes are not about.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import limits_ref as L
from test_gpu_dr import _check_discrimination, _check_input, _distance, _step_parity_bars
from test_gpu_parity import TF, _new_env, _set_states, _tf_run

pytestmark = pytest.mark.gpu

SOLVERS = ["newton", "pgs"]
_RUNS = {}


def _run(cls, solver, o64, o32):
    """The class's 3 teacher-forced env steps: (TF arrays, GPU limit-row count per env step, the oracle's, the fp64
    oracle's stop margin at the last substep per env step, wrong-model distances per env step, meta, info)."""
    key = (cls, solver)
    if key in _RUNS:
        return _RUNS[key]
    from gym_so100.model import build_model
    nsub = L.NSUBSTEP[cls]
    model = build_model(solver=solver, nsubstep=nsub)
    states, meta, acts, info = L.cases(cls, o64, model)
    n = len(states)
    assert n <= 48 and n % 4 != 0
    right = lambda k: (model, acts[k % n])
    wrongs = {name: (f(model), steps) for name, (f, steps) in L.WRONG[cls].items()}
    for name, (mw, steps) in wrongs.items():          # the inputs discriminate: before any GPU step
        lim = [i for i in range(n) if meta[i]]
        _check_input(f"{solver} limits {cls}, {name}, initial states",
                     _distance(o64, [states[i] for i in lim], lambda k: (model, acts[lim[k]]),
                               lambda k: (mw, acts[lim[k]]), "qv"), 1e-5)
    env = _new_env(n, solver, nsubstep=nsub)
    env.reset(seed=3)
    _set_states(env, states)
    res, rows_gpu = TF(), []
    for _ in range(L.STEPS):                          # one step per call: the debug record holds the last step's solve
        _tf_run(env, model, o64, o32, 1, lambda step: acts, res=res)
        dbg = env.debug.cpu().numpy()
        rows_gpu.append(dbg[:, 3] - 12 - 4 * dbg[:, 0])
    env.close()
    r = res.arrays()
    assert len(r.states) == L.STEPS * n
    rows_gpu = np.concatenate(rows_gpu)
    rows_ora = np.array([L.step(o64, model, st, st[3])[3] for st in r.states])
    margin = np.array([L.last_substep_margin(o64, model, st, st[3]) for st in r.states])
    dist = {name: _distance(o64, r.states, right, lambda k, mw=mw: (mw, acts[k % n]), "qv")
            for name, (mw, _) in wrongs.items()}
    _RUNS[key] = (r, rows_gpu, rows_ora, margin, dist, meta, info)
    return _RUNS[key]


def _check_rows(cls, solver, run, model):
    """1. Row presence: the GPU's limit-row count of the last substep against the fp64 oracle's."""
    r, rows_gpu, rows_ora, margin, _, _, _ = run
    assert np.array_equal(rows_gpu, np.round(rows_gpu)) and rows_gpu.min() >= 0 and rows_gpu.max() <= L.NH
    if L.NSUBSTEP[cls] == 1:
        # one substep: the rows are those of the state itself, for every env, and the rule is restated in numpy
        pred = np.array([np.abs(L.predicted_rows(model, st[0])).sum() for st in r.states])
        assert np.array_equal(rows_gpu, rows_ora), np.nonzero(rows_gpu != rows_ora)
        assert np.array_equal(rows_gpu, pred), np.nonzero(rows_gpu != pred)
        excluded = 0.0
    else:
        keep = margin > 1e-6
        excluded = 1 - keep.mean()
        assert excluded <= 0.05, excluded
        assert np.array_equal(rows_gpu[keep], rows_ora[keep]), np.nonzero(keep & (rows_gpu != rows_ora))
    print(f"[{solver} limits {cls}] limit rows in the last substep: non-zero in {np.mean(rows_gpu > 0):.3f} of "
          f"{len(rows_gpu)} env steps, {int(rows_gpu.sum())} rows (oracle {int(rows_ora.sum())}), mismatches "
          f"{int((rows_gpu != rows_ora).sum())}, env steps within 1e-6 rad of a stop {excluded:.3f}")
    return rows_gpu


def _check_parity(cls, solver, run, min_forces=-1):
    """2. Parity: the bars of _step_parity_bars / _force_bars; one substep with Newton also north_star's 1e-4 at the
    median, as test_arm_contact_substep_parity"""
    r = run[0]
    print("\n" + r.summary(f"{solver} limits {cls}"))
    sub_newton = L.NSUBSTEP[cls] == 1 and solver == "newton"
    _step_parity_bars(r, solver, min_forces=min_forces, median_abs=1e-4 if sub_newton else None)
    if sub_newton:
        assert np.median(r.qv) <= 1e-4 and np.median(r.qa) <= 1e-4


def _check_wrong_models(cls, solver, run):
    """3. Discrimination on the env steps limits_ref.WRONG grades (the limited envs')"""
    r, _, _, _, dist, meta, _ = run
    print()
    assert dist
    for name, d in dist.items():
        g = L.graded(meta, L.WRONG[cls][name][1])
        _check_discrimination(f"{solver} limits {cls}, {name}", r.qv[g], d[g], 1e-5)


def _model(cls, solver):
    from gym_so100.model import build_model
    return build_model(solver=solver, nsubstep=L.NSUBSTEP[cls])


# ----------------------------------------------------------------------------- a. beyond the stop, one substep
@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_beyond_substep_parity(solver, oracle64, oracle32):
    """a. 46 envs, 35 of them with 1 to 3 hinges 1e-5 .. 4e-2 rad beyond a stop, one substep per env step: every env's row
    count equals the oracle's and the numpy restatement of the kernel's rule, the rows run in more than half of the env
    steps, and the parity bars hold (fp32 restatement on the CPU: 1.3e-7 / 4.7e-7 median / p90 in relative qvel)."""
    run = _run("a", solver, oracle64, oracle32)
    rows = _check_rows("a", solver, run, _model("a", solver))
    assert np.mean(rows > 0) > 0.5
    _check_parity("a", solver, run)


@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_beyond_substep_discrimination(solver, oracle64, oracle32):
    """a. The model without limit rows (CPU oracle: 0.13 median in relative qvel after one substep) and the rows' time
    constant x 1.1 (1.6e-2) are told from the right one."""
    _check_wrong_models("a", solver, _run("a", solver, oracle64, oracle32))


# ----------------------------------------------------------------------------- b. the same states, whole env steps
@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_beyond_step_parity(solver, oracle64, oracle32):
    """b. Class a's states over whole env steps of 10 substeps: rows switch off as the hinges are pushed back, and on the
    fused path the warm start and the rows' hand-over live through that in registers.  The last substep's row count
    equals the oracle's wherever the fp64 oracle's hinges are more than 1e-6 rad from a stop (at most 5 % are not)."""
    run = _run("b", solver, oracle64, oracle32)
    _check_rows("b", solver, run, _model("b", solver))
    _check_parity("b", solver, run)


@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_beyond_step_discrimination(solver, oracle64, oracle32):
    """b. The model without limit rows (CPU oracle: 1.0 median after the first env step, 0.16 over the three), the rows'
    time constant x 1.1 (5.6e-2, 1.7e-2) and, on the first env step, the hinges' dof_invweight0 x 1.1 (the rows' R:
    1.6e-3) are told from the right one."""
    _check_wrong_models("b", solver, _run("b", solver, oracle64, oracle32))


# ----------------------------------------------------------------------------- c. approach
@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_approach_parity(solver, oracle64, oracle32):
    """c. One hinge per env 0.002 .. 0.03 rad inside a stop running into it at 2 .. 8 rad/s (46 of 55 draws kept by the
    fp64 oracle: the row off at substep 1 and on by substep 8; it first binds in substeps 2 .. 7), whole env steps."""
    run = _run("c", solver, oracle64, oracle32)
    first = run[6]["first"]
    print(f"\napproach: {len(first)} of {run[6]['draws']} draws kept, first binding substep histogram {np.bincount(first)}")
    assert first.min() >= 2 and first.max() <= 8
    rows = _check_rows("c", solver, run, _model("c", solver))
    assert np.mean(rows > 0) > 0.5
    _check_parity("c", solver, run)


@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_approach_discrimination(solver, oracle64, oracle32):
    """c. The model without limit rows (CPU oracle: 2.9 median after the first env step, 0.30 over the three), the rows'
    time constant x 1.1 (0.16, 4e-2) and, on the first env step, the hinges' dof_invweight0 x 1.1 (5.4e-3) are told
    from the right one."""
    _check_wrong_models("c", solver, _run("c", solver, oracle64, oracle32))


# ----------------------------------------------------------------------------- d. with contacts
@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_contact_parity(solver, oracle64, oracle32):
    """d. 26 class-a states whose first position stage holds a contact (the arm touching itself or the Base near its
    stops; 26 of 322 draws, the others holding no contact or touching the table) and drops none, one substep per env step: frictionloss, limit and contact rows in one
    solve, the per-contact forces graded by _force_bars."""
    run = _run("d", solver, oracle64, oracle32)
    r = run[0]
    ncon = np.array([len(p) for p in r.pairs])
    print(f"\nGPU contacts per env step: mean {ncon.mean():.1f}, env steps with any {np.mean(ncon > 0):.2f}")
    rows = _check_rows("d", solver, run, _model("d", solver))
    assert np.mean(rows > 0) > 0.5 and np.mean((rows > 0) & (ncon > 0)) > 0.5
    _check_parity("d", solver, run, min_forces=24)


# ----------------------------------------------------------------------------- e. the fp32 edge
@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_edge(solver, oracle64, oracle32):
    """e. A hinge exactly one fp32 ulp inside float32(limit) (8 envs: no row) or one ulp outside (8 envs: a row), both
    stops, 1 rad/s into the stop, one substep per env step: the double limit lies within half an ulp of its fp32
    rounding (tests/test_limits_cpu.py), so the fp32 kernel and the fp64 oracle decide alike."""
    run = _run("e", solver, oracle64, oracle32)
    rows = _check_rows("e", solver, run, _model("e", solver))
    assert np.array_equal(rows[:L.N_EDGE], run[6]["rows"])
    _check_parity("e", solver, run)


# ----------------------------------------------------------------------------- the impedance ramp
@pytest.mark.parametrize("solver", SOLVERS)
def test_limits_ramp_discrimination(solver, oracle64, oracle32):
    """Class a with every depth on the impedance ramp (1e-5 .. 0.9e-3 rad), graded on the first substep (a pushed hinge
    leaves the ramp within one): jnt_solimp[0] x 1.02, the impedance at depth 0, is told from the right model.  On the
    CPU oracle the factor 1.02 puts the wrong model 2.1e-3 (median) from the right one in relative qvel, 214 x the bar
    of 1e-5, so the factor is not raised.  The row counts and the parity bars are asserted on these states too."""
    run = _run("ramp", solver, oracle64, oracle32)
    _check_rows("ramp", solver, run, _model("ramp", solver))
    _check_parity("ramp", solver, run)
    _check_wrong_models("ramp", solver, run)
