"""CPU checks of the joint-limit parity classes (tests/limits_ref.py), from the oracles alone: the conditions on the
inputs of tests/test_gpu_limits.py (layout, ramp and plateau shares, pushing rows, class c's binding substeps, the fp32
edge's premise, no dropped contact, the 5 % cap on env steps within 1e-6 rad of a stop, every wrong-model distance), and
that the fp32 restatement of the oracle meets the parity bars against the fp64 oracle on these states: the bars are
known to be reachable by a correct fp32 implementation before a kernel is graded.  The fp32 oracle stands where the GPU
stands in the GPU tests, on the fp64 oracle's own closed-loop states rounded to fp32."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")     # (test_gpu_parity, whose TF record and bars are used here, imports it)

import limits_ref as L
from test_gpu_dr import _check_discrimination, _check_input, _distance, _step_parity_bars
from test_gpu_parity import NEAR0, TF, _force_err, _rel

SOLVERS = ["newton", "pgs"]
CLASSES = ["a", "b", "c", "d", "e", "ramp"]
_RUNS = {}


def _run(cls, solver, o64, o32):
    """The class on the CPU: a TF record with the fp32 oracle in the GPU's place (its floors: the fp32 oracle itself and
    the fp64 oracle under a 1-ulp input perturbation, as _tf_run computes them), the row counts of both oracles, the
    fp64 oracle's stop margin at the last substep, and the wrong-model distances, per env step (step-major)."""
    key = (cls, solver)
    if key in _RUNS:
        return _RUNS[key]
    from gym_so100.model import build_model
    model = build_model(solver=solver, nsubstep=L.NSUBSTEP[cls])
    states, meta, acts, info = L.cases(cls, o64, model)
    n = len(states)
    prng = np.random.default_rng(12345)
    r = TF()
    r.builds = ["fp32 oracle"]
    rows64, rows32, margin = [], [], []
    d = o64.new_data()
    for sts in L.closed_loop(o64, model, states, acts):
        for st, a in zip(sts, acts):
            oq, ov, s64, n64, _ = L.step(o64, model, st, a)
            fq, fv, s32, n32, _ = L.step(o32, model, st, a)
            pert = (st[0] * (1 + prng.normal(0, 2.0 ** -24, 13)), st[1] * (1 + prng.normal(0, 2.0 ** -24, 12)), st[2])
            _, pv, sp, _, _ = L.step(o64, model, pert, a)
            o64.set_state(d, *st)
            o64.call("so100o_fwd_position", model, d)
            r.near0.append(any(abs(d.con[c].dist) < NEAR0 for c in range(d.ncon)))
            for name, v in (("qp", np.abs(oq - fq).max()), ("qv", _rel(fv, ov)), ("qa", _rel(s32[3], s64[3]))):
                getattr(r, name).append(v)
                getattr(r, "f" + name).append(v)
            r.pqv.append(_rel(pv, ov))
            r.pqa.append(_rel(sp[3], s64[3]))
            same, psame = np.array_equal(s32[0], s64[0]), np.array_equal(sp[0], s64[0])
            r.same.append(same)
            r.fsame.append(same)
            r.psame.append(psame)
            if same and len(s64[0]):
                e = list(_force_err(s32[1], s64[1]))
                r.force += e
                r.fforce += e
            if psame and len(s64[0]):
                r.pforce += list(_force_err(sp[1], s64[1]))
            r.pairs.append(s32[0])
            r.drop_gpu.append(s32[4])
            r.drop_ora.append(s64[4])
            r.states.append((st[0], st[1], st[2], a))
            rows64.append(n64)
            rows32.append(n32)
            margin.append(L.last_substep_margin(o64, model, st, a))
    r = r.arrays()
    dist = {name: _distance(o64, r.states, lambda k: (model, acts[k % n]), lambda k, mw=f(model): (mw, acts[k % n]), "qv")
            for name, (f, _) in L.WRONG[cls].items()}
    _RUNS[key] = (model, states, meta, acts, info, r, np.array(rows64), np.array(rows32), np.array(margin), dist)
    return _RUNS[key]


# ----------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("solver", SOLVERS)
def test_beyond_states_layout(solver, oracle64, oracle32):
    """Class a: 46 fp32 states, no hinge more than 0.04 rad beyond a stop and the others 0.05 rad or more inside; every
    fourth env without a limit and the rest with 1 to 3; within each block of 16 envs the limited envs' hinge sets
    pairwise different; each of the 12 (hinge, side) combinations twice or more; a quarter or more of the depths on
    the impedance ramp and a quarter or more on the plateau; two thirds or more of the rows pushing (a non-zero force
    in the fp64 oracle's solve) and some releasing; class b runs the same states."""
    model, states, meta, acts, _, r, rows64, _, _, _ = _run("a", solver, oracle64, oracle32)
    n = len(states)
    assert n == L.N == 46 and n % 4 and n % 16
    lo, hi = L.ranges(model)
    count = np.zeros((L.NH, 2), int)
    for i, ((q, v, w), me) in enumerate(zip(states, meta)):
        assert np.array_equal(q, L.r32(q)) and np.array_equal(v, L.r32(v)) and not w.any()
        assert np.array_equal(q[6:], L.r32(L.CUBE_PARK)) and not v[6:].any()
        assert (len(me) == 0) == (i % 4 == 3) and len(me) <= 3
        limited = {j for j, _, _ in me}
        assert len(limited) == len(me)
        beyond = np.maximum(lo - q[:6], q[:6] - hi)
        for j in range(L.NH):
            assert (1e-5 * 0.98 <= beyond[j] <= 4e-2 * 1.001) if j in limited else (beyond[j] <= -0.05 + 1e-6)
        for j, side, depth in me:
            assert (q[j] < lo[j]) if side == 0 else (q[j] > hi[j])
            count[j, side] += 1
        assert np.array_equal(L.predicted_rows(model, q) != 0, np.isin(np.arange(L.NH), list(limited)))
        assert np.array_equal(acts[i], L.hold_action(model, q[:6])) and np.abs(acts[i]).max() <= 1
    for b0 in range(0, n, 16):
        sets = [frozenset(j for j, _, _ in me) for me in meta[b0:b0 + 16] if me]
        assert len(sets) >= 10 and len(set(sets)) == len(sets)
    assert count.min() >= 2, count
    depth = np.array([d for me in meta for _, _, d in me])
    ramp = np.mean(depth < model.jnt_solimp[2])
    force = np.concatenate([L.trace(oracle64, model, st, a)[0][2] for st, a in zip(states, acts)])
    for st, a, me in zip(states, acts, meta):          # the env step's limit rows (step checks its replay's qacc)
        hinges = [j for j, _, _ in me]
        nrow, limf = L.step(oracle64, model, st, a)[3:]
        assert nrow == len(me) and not np.delete(limf, hinges).any() and (limf >= 0).all()
    assert len(force) == len(depth) == rows64[:n].sum()
    push = np.mean(force > 0)
    print(f"\n[{solver} limits a] {len(depth)} rows in {sum(1 for me in meta if me)} of {n} envs, per (hinge, side) "
          f"{count.ravel()}; on the ramp {ramp:.2f}, pushing {push:.2f}")
    assert ramp >= 0.25 and 1 - ramp >= 0.25
    assert 2 / 3 <= push < 1
    sb = _run("b", solver, oracle64, oracle32)[1]
    assert all(np.array_equal(x, y) for s, t in zip(states, sb) for x, y in zip(s, t))


@pytest.mark.parametrize("solver", SOLVERS)
def test_approach_binding_substeps(solver, oracle64, oracle32):
    """Class c: one hinge 0.002 .. 0.03 rad inside a stop at 2 .. 8 rad/s towards it, everything else at rest; on the fp64
    oracle's substeps its row is off at substep 1 and on by substep 8; every hinge occurs, and 10 or more of the 12 stops."""
    model, states, meta, acts, info, _, rows64, _, _, _ = _run("c", solver, oracle64, oracle32)
    lo, hi = L.ranges(model)
    assert len(states) == 46 and info["draws"] <= 2 * len(states)
    for (q, v, w), me, a in zip(states, meta, acts):
        (j, side, _), = me
        gap = q[j] - lo[j] if side == 0 else hi[j] - q[j]
        assert 0.002 * 0.99 <= gap <= 0.03 * 1.01 and 2 <= abs(v[j]) <= 8 and (v[j] < 0) == (side == 0)
        assert np.count_nonzero(v) == 1 and not L.predicted_rows(model, q).any()
        on = [j in t[1] for t in L.trace(oracle64, model, (q, v, w), a)]
        assert not on[0] and any(on[:8])
    # (the shoulder never reaches its upper stop here: the arm meets the Base first, and such draws are not kept)
    combos = {(me[0][0], me[0][1]) for me in meta}
    assert {j for j, _ in combos} == set(range(L.NH)) and len(combos) >= 10
    print(f"\n[{solver} limits c] {len(states)} of {info['draws']} draws kept; first binding substep histogram "
          f"{np.bincount(info['first'])}")
    assert info["first"].min() >= 2 and info["first"].max() <= 8
    assert np.mean(rows64 > 0) > 0.5


@pytest.mark.parametrize("solver", SOLVERS)
def test_contact_states_hold_contacts_and_drop_none(solver, oracle64, oracle32):
    """Class d: every state limited, its first position stage holds a contact and drops none; no contact is dropped in
    the steps either, and limit and contact rows share the solve in more than half of the env steps."""
    model, states, meta, _, info, r, rows64, _, _, _ = _run("d", solver, oracle64, oracle32)
    d = oracle64.new_data()
    assert len(states) == L.N_CONTACT >= 24 and len(states) % 4
    for st, me in zip(states, meta):
        oracle64.set_state(d, *st)
        oracle64.call("so100o_fwd_position", model, d)
        assert d.ncon >= 1 and d.ncon_dropped == 0 and 1 <= len(me) <= 3
    ncon = np.array([len(p) for p in r.pairs])
    print(f"\n[{solver} limits d] {len(states)} of {info['draws']} draws kept; contacts per env step mean {ncon.mean():.1f}")
    assert r.drop_ora.sum() == 0 and r.drop_gpu.sum() == 0
    assert np.mean((rows64 > 0) & (ncon > 0)) > 0.5


def test_edge_premise(model, oracle64, oracle32):
    """Class e's premise: every double limit lies within half an fp32 ulp of its fp32 rounding, so a hinge one ulp outside
    float32(limit) is outside the double limit and one ulp inside is inside it: the fp32 rule (predicted_rows), the fp32
    oracle and the fp64 oracle hold the same rows.  No hinge sits on float32(limit) itself."""
    lo, hi = L.ranges(model)
    for lim in np.concatenate([lo, hi]):
        l32 = np.float32(lim)
        ulp = min(abs(float(np.nextafter(l32, np.float32(s) * np.inf)) - float(l32)) for s in (-1, 1))
        assert abs(float(l32) - lim) <= 0.5 * ulp
    m1 = L.one_substep(model)
    states, meta, acts, rows = L.edge_states(oracle64, m1)
    assert len(states) == L.N_EDGE and L.N_EDGE % 4 and rows[:8].sum() == 0 and rows[8:16].sum() == 8
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    for group in (meta[:8], meta[8:16]):
        assert {s for (_, s, _), in group} == {0, 1}
    for st, me, a, want in zip(states, meta, acts, rows):
        q32 = st[0][:6].astype(np.float32)
        assert not (q32 == lo32).any() and not (q32 == hi32).any()
        if me:
            (j, side, inside), = me
            edge = (lo32, hi32)[side][j]
            assert q32[j] == np.nextafter(edge, np.float32((1 if side == 0 else -1) * inside * np.inf))
            assert st[1][j] == (-1.0 if side == 0 else 1.0)
            assert ((q32[j] < edge) if side == 0 else (q32[j] > edge)) == (inside < 0)
            assert ((st[0][j] < lo[j]) if side == 0 else (st[0][j] > hi[j])) == (inside < 0)
        assert np.abs(L.predicted_rows(m1, st[0])).sum() == want
        assert L.step(oracle64, m1, st, a)[3] == want and L.step(oracle32, m1, st, a)[3] == want


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("solver", SOLVERS)
def test_row_counts_fp32_against_fp64(solver, cls, oracle64, oracle32):
    """The row-presence check of the GPU tests is reachable in fp32: over one substep the fp32 oracle, the fp64 oracle and
    the numpy restatement of the kernel's rule hold the same limit rows on every env step; over 10 substeps the fp32
    oracle's last substep holds the fp64 oracle's rows wherever the fp64 oracle's hinges are more than 1e-6 rad from a
    stop there, and at most 5 % of the env steps are not."""
    model, _, _, _, _, r, rows64, rows32, margin, _ = _run(cls, solver, oracle64, oracle32)
    if L.NSUBSTEP[cls] == 1:
        pred = np.array([np.abs(L.predicted_rows(model, st[0])).sum() for st in r.states])
        assert np.array_equal(rows64, rows32) and np.array_equal(rows64, pred)
    else:
        keep = margin > 1e-6
        print(f"\n[{solver} limits {cls}] env steps within 1e-6 rad of a stop at the last substep: {1 - keep.mean():.3f}")
        assert 1 - keep.mean() <= 0.05
        assert np.array_equal(rows64[keep], rows32[keep])


@pytest.mark.parametrize("cls", ["a", "b", "c", "ramp"])
@pytest.mark.parametrize("solver", SOLVERS)
def test_wrong_models_are_told_apart(solver, cls, oracle64, oracle32):
    """Every wrong model of limits_ref.WRONG sits 100 x the median bar (1e-5) or more from the right one at the median,
    on the initial states and on all graded env steps, and the fp32 oracle's error is under a tenth of that distance on
    90 % or more of them: the criterion of the GPU tests can be met in fp32."""
    _, states, meta, _, _, r, _, _, _, dist = _run(cls, solver, oracle64, oracle32)
    n = len(states)
    assert dist
    print()
    for name, d in dist.items():
        g = L.graded(meta, L.WRONG[cls][name][1])
        _check_input(f"{solver} limits {cls}, {name}, initial states", d[:n][g[:n]], 1e-5)
        _check_discrimination(f"{solver} limits {cls}, {name} (fp32 oracle)", r.qv[g], d[g], 1e-5)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("solver", SOLVERS)
def test_fp32_oracle_meets_the_parity_bars(solver, cls, oracle64, oracle32):
    """The bars of the GPU tests (_step_parity_bars, _force_bars; one substep with Newton: 1e-4 at the median of qvel, qacc
    and the contact forces) with the fp32 oracle in the GPU's place."""
    r = _run(cls, solver, oracle64, oracle32)[5]
    print("\n" + r.summary(f"{solver} limits {cls}, fp32 oracle"))
    sub_newton = L.NSUBSTEP[cls] == 1 and solver == "newton"
    _step_parity_bars(r, solver, min_forces=24 if cls == "d" else -1, median_abs=1e-4 if sub_newton else None)
    if sub_newton:
        assert np.median(r.qv) <= 1e-4 and np.median(r.qa) <= 1e-4
