"""GPU parity of domain randomisation (SO100_FLAG_DR: per-env cube mass scale, cube-pair friction scale, action-noise
sigma) against the fp64 oracle run on a per-env copy of the model (tests/dr_ref.py scaled_model) and fed the
host-restated action noise (dr_ref.action_noise).  DESIGN.md §5.

Every class steps the product builds through test_gpu_parity's _step_all_builds (bitwise equal to the debug build) and
applies the bars of the non-DR class it mirrors, the floors computed on the per-env scaled models.  Every class also
shows that its inputs tell the right model from the wrong one it is meant to catch (`*_discrimination`): the fp64
oracle runs the same states a second time on the wrong model, and

* the wrong oracle's median distance from the right one is at least 100 x the class's median bar (a condition on the
  inputs, from the oracle alone: asserted on the initial states before any GPU step, and again on all states);
* for at least 90 % of the env steps the GPU's error against the right oracle is under a tenth of that distance.

Half the envs sit at the corners (0.8, 1.2) / (1.2, 0.8) of the (mass, friction) ranges, the rest keep the scales the
env drew; the per-env models are built from the fp32 values of the env's own dr_params tensor.  The runs are shared
between a class's parity and discrimination tests (module cache).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dr_ref as R
from test_gpu_parity import TF, _force_bars, _new_env, _pressed_states, _set_states, _step_all_builds, _tf_run

pytestmark = pytest.mark.gpu

SOLVERS = ["newton", "pgs"]
DR_RANGES = dict(mass=(0.8, 1.2), friction=(0.8, 1.2))
_RUNS = {}


def _cached(key, make):
    if key not in _RUNS:
        _RUNS[key] = make()
    return _RUNS[key]


def _seat_corners(env):
    """dr_params[:, :2] of every second env set in place (before the first step) to the corners; returns the tensor's
    fp32 values, which the per-env models are built from"""
    n = env.num_envs
    idx = torch.arange(0, n, 2, device=env.dr_params.device)
    corners = torch.tensor([R.CORNERS[(i // 2) % 2] for i in range(0, n, 2)], dtype=torch.float32)
    ptr = env.dr_params.data_ptr()
    env.dr_params[idx, :2] = corners.to(env.dr_params.device)
    assert env.dr_params.data_ptr() == ptr
    torch.cuda.synchronize()
    return env.dr_params.cpu().numpy()


def _dr_env(n, solver, sigma=0.0, seed=3, **kw):
    env = _new_env(n, solver, seed=seed, domain_randomization=dict(action_noise=sigma, **DR_RANGES), **kw)
    p = _seat_corners(env)
    assert ((p[:, :2] >= 0.8) & (p[:, :2] <= 1.2)).all() and len(np.unique(p[:, 0])) > n // 2
    return env, p


def _models(base, p):
    return [R.scaled_model(base, p[i, 0], p[i, 1]) for i in range(len(p))]


def _all_pairs_friction(base, ms, fs):
    """the wrong model of class c: the friction scale on every pair, not on the cube's alone"""
    m = R.scaled_model(base, ms, 1.0)
    for p in range(len(m.pair_friction)):
        for k in range(3):
            m.pair_friction[p][k] *= float(fs)
    return m


def _inertia_unscaled(base, ms, fs):
    """a wrong model of class a: the mass scale on the cube's mass but not on its inertia"""
    m = R.scaled_model(base, ms, fs)
    for k in range(3):
        m.body_inertia[R.CUBE_BODY][k] = base.body_inertia[R.CUBE_BODY][k]
    return m


def _distance(o64, states, right, wrong, quantity):
    """Per state the wrong oracle's distance from the right one after one env step, from the fp64 oracle alone.
    right / wrong: k -> (model, action).  quantity "qv": the relative qvel distance; "force": the largest per-contact
    relative force distance (inf where the wrong model's contact list differs, 0 where neither holds a contact)."""
    out = []
    for k, st in enumerate(states):
        m, a = right(k)
        mw, aw = wrong(k)
        _, v, s = R.oracle_step(o64, m, st, a)
        _, vw, sw = R.oracle_step(o64, mw, st, aw)
        if quantity == "qv":
            out.append(R.rel_dist(vw, v))
        elif not np.array_equal(s[0], sw[0]):
            out.append(np.inf)
        else:
            out.append(R.force_dist(sw[1], s[1]).max() if len(s[0]) else 0.0)
    return np.array(out)


def _floor_median(o64, o32, states, right, quantity):
    """the median of the floors (fp32 restatement; fp64 under a 1-ulp input perturbation) on these states, as TF.floor"""
    rng = np.random.default_rng(4321)
    f32, fp = [], []
    for k, st in enumerate(states):
        m, a = right(k)
        _, v, s = R.oracle_step(o64, m, st, a)
        _, v32, s32 = R.oracle_step(o32, m, st, a)
        pert = (st[0] * (1 + rng.normal(0, 2.0 ** -24, 13)), st[1] * (1 + rng.normal(0, 2.0 ** -24, 12)), st[2])
        _, vp, sp = R.oracle_step(o64, m, pert, a)
        if quantity == "qv":
            f32.append(R.rel_dist(v32, v))
            fp.append(R.rel_dist(vp, v))
        else:
            if np.array_equal(s32[0], s[0]) and len(s[0]):
                f32 += list(R.force_dist(s32[1], s[1]))
            if np.array_equal(sp[0], s[0]) and len(s[0]):
                fp += list(R.force_dist(sp[1], s[1]))
    return max(np.median(x) if len(x) else 0.0 for x in (f32, fp))


def _gpu_force_err(r):
    """per env step of a TF the largest per-contact force error of the GPU (nan where TF graded no forces: a contact
    list that differs, or no contact)"""
    out, k0 = np.full(len(r.qv), np.nan), 0
    for k in range(len(r.qv)):
        if r.same[k] and r.fsame[k] and len(r.pairs[k]):
            nc = len(r.pairs[k])
            out[k] = np.max(r.force[k0:k0 + nc])
            k0 += nc
    assert k0 == len(r.force)
    return out


def _tells_apart(o64, m, mw, state, acts, quantity, least, pairs_ok=None):
    """Whether model mw stays `least` or more away from model m (_distance) at every step of the fp64 oracle's own
    closed-loop run of `acts` on m from `state` (and every step's contact pairs pass pairs_ok): the selection of input
    states, by the oracle alone."""
    s = state
    for a in acts:
        if _distance(o64, [s], lambda k: (m, a), lambda k: (mw, a), quantity)[0] < least:
            return False
        d = o64.new_data()
        o64.set_state(d, *s)
        o64.env_step(m, d, 0, a)
        if pairs_ok is not None and not pairs_ok(o64.last_solve(d)[0]):
            return False
        s = o64.get_state(d)[:3]
    return True


def _check_input(label, dist, median_bar):
    print(f"[{label}] wrong-oracle distance min / median / max {dist.min():.2e} / {np.median(dist):.2e} / {dist.max():.2e}; "
          f"median bar {median_bar:.2e}, ratio {np.median(dist) / median_bar:.0f}")
    assert np.median(dist) >= 100 * median_bar, (label, np.median(dist), median_bar)


def _check_discrimination(label, gpu_err, dist, median_bar):
    """dist: the wrong oracle's distance per env step; gpu_err: the GPU's error against the right oracle"""
    _check_input(label, dist, median_bar)
    ok = np.nan_to_num(gpu_err, nan=np.inf) < 0.1 * dist
    ratio = np.nan_to_num(gpu_err, nan=np.inf) / np.maximum(dist, 1e-300)
    print(f"[{label}] GPU error / wrong-oracle distance: median {np.median(ratio):.1e}, p90 {np.quantile(ratio, 0.9):.1e}; "
          f"under 0.1 in {ok.mean():.3f} of {len(ok)} env steps")
    assert ok.mean() >= 0.9, (label, ok.mean())


def _step_parity_bars(r, solver, min_forces, median_abs=None):
    """the bars of test_gpu_parity.test_step_parity_teacher_forced"""
    n = len(r.qv)
    assert np.median(r.qp) <= 1e-5 and np.median(r.qv) <= 1e-5
    assert np.quantile(r.qv, 0.9) <= 2 * r.floor("qv", 0.9) + 1e-4
    assert np.quantile(r.qv, 0.99) <= 2 * r.floor("qv", 0.99) + 1e-4
    assert r.qv.max() <= 2 * r.floor("qv", 1.0) + 1e-3
    assert np.mean(r.qv < 1e-4) >= min(np.mean(r.fqv < 1e-4), np.mean(r.pqv < 1e-4)) - 0.05
    assert r.rew_bad <= max(2, 0.005 * n)
    assert r.bit_bad <= max(4, 0.01 * n)
    assert len(r.force) > min_forces and r.same.mean() >= min(r.fsame.mean(), r.psame.mean()) - 0.03
    _force_bars(r, median_abs=median_abs)
    assert r.drop_gpu.sum() == 0 and r.drop_ora.sum() == 0


# ----------------------------------------------------------------------------- a. sliding and tumbling cube
def _run_sliding(solver, o64, o32):
    from gym_so100.model import build_model
    base = build_model(solver=solver)
    n = 24
    env, p = _dr_env(n, solver)
    models = _models(base, p)
    states = [R.sliding_cube_state(o64, models[i], 1000 + i) for i in range(n)]
    zero = np.zeros((n, 6), np.float32)
    right = lambda k: (models[k % n], zero[0])
    inert = [_inertia_unscaled(base, *p[i, :2]) for i in range(n)]
    wrongs = {"unscaled": lambda k: (base, zero[0]), "inertia unscaled": lambda k: (inert[k % n], zero[0])}
    for name, w in wrongs.items():          # the inputs discriminate: before any GPU step
        _check_input(f"{solver} sliding cube, {name}, initial states", _distance(o64, states, right, w, "qv"), 1e-5)
    env.reset(seed=3)
    _set_states(env, states)
    r = _tf_run(env, models, o64, o32, 3, lambda step: zero).arrays()
    env.close()
    return r, {name: _distance(o64, r.states, right, w, "qv") for name, w in wrongs.items()}


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_sliding_cube_parity(solver, oracle64, oracle32):
    """a. A cube sliding (0.3 m/s) and tumbling (N(0, 3 rad/s) per axis) on the table, 24 DR envs, 3 teacher-forced steps:
    the mass scale must reach the cube's mass and its inertia, the friction scale the cube-table pair.  Bars of
    test_step_parity_teacher_forced and _force_bars, the floors on the per-env models."""
    r, _ = _cached(("a", solver), lambda: _run_sliding(solver, oracle64, oracle32))
    print("\n" + r.summary(f"{solver} DR sliding cube"))
    _step_parity_bars(r, solver, min_forces=0)


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_sliding_cube_discrimination(solver, oracle64, oracle32):
    """a. The unscaled model, and the model with the mass scaled but the inertia not, are told from the right one: on
    the CPU oracle (tests/test_dr_ref_cpu.py) they sit 6e-3 (min) / 2e-2 (median) from it in relative qvel, the
    fp32 restatement 1e-6 / 4e-6 (median / max)."""
    r, dist = _cached(("a", solver), lambda: _run_sliding(solver, oracle64, oracle32))
    print()
    for name, d in dist.items():
        _check_discrimination(f"{solver} sliding cube, {name}", r.qv, d, 1e-5)


# ----------------------------------------------------------------------------- b. resting cube in the bin corner
BIN_SEED = 4      # the first env seed from 3 on whose drawn friction scales all lie 0.03 or more from 1 (asserted)


def _bin_corner_cases(o64, o32, base, p, n):
    """n states drawn from test_heavy_contact_parity's recipe (dr_ref.bin_corner_states) with their 3 actions each,
    U(-0.2, 0.2), taken by the oracle alone, before any GPU step.

    The cube of this recipe is wedged between two walls and the floor at friction 1: under Newton the normal forces are
    120 .. 250 N against a weight of 0.49 N, so the forces follow the penetration and the friction limit.  The mass scale
    alone moves them by 1e-4, the fp32 floor (tests/test_dr_ref_cpu.py), and the friction scale moves them only where a
    contact sits on its friction cone: with the recipe's first 16 draws the unscaled model is 1.5e-6 .. 9e-5 away in a
    quarter of the env steps, which no fp32 result can tell from the right one (the fp32 restatement in the GPU's place
    reaches a share of 0.73 there, as the GPU does).  A draw is therefore taken for env slot i only if, on the fp64
    oracle's own closed-loop steps with slot i's scales, the unscaled model's forces stay away from the right model's
    by 1e-3 or more (10 x the 1e-4 a per-contact force is held to at the median) and by 20 x the fp32 restatement's own
    error on that state (the GPU may be 2 x the floor off and must stay under a tenth of the distance) at each of
    the 3 steps.  Returns the states and the actions [3][n, 6]."""
    rng = np.random.default_rng(7)
    states, acts, tried = [], [], 0
    while len(states) < n and tried < 12 * n:
        qpos, qvel = R.bin_corner_states(base, n, rng)
        cand = rng.uniform(-0.2, 0.2, (n, 3, 6)).astype(np.float32)
        tried += n
        for j in range(n):
            i = len(states)
            if i == n:
                break
            m = R.scaled_model(base, *p[i, :2])
            s, ok = (qpos[j], qvel[j], np.zeros(12)), True
            for a in cand[j]:
                d = o64.new_data()
                o64.set_state(d, *s)
                o64.env_step(m, d, 0, a)
                sol, s32 = o64.last_solve(d), R.oracle_step(o32, m, s, a)[2]
                dist = _distance(o64, [s], lambda k: (m, a), lambda k: (base, a), "force")[0]
                floor = R.force_dist(s32[1], sol[1]).max() if np.array_equal(s32[0], sol[0]) and len(sol[0]) else np.inf
                if not dist >= max(1e-3, 20 * floor):
                    ok = False
                    break
                s = o64.get_state(d)[:3]
            if ok:
                states.append((qpos[j], qvel[j], np.zeros(12)))
                acts.append(cand[j])
    assert len(states) == n, (len(states), tried)
    print(f"bin corner: {n} of {tried} draws of the recipe taken")
    return states, [np.array([a[k] for a in acts]) for k in range(3)]


def _run_bin_corner(solver, o64, o32):
    from gym_so100.model import build_model
    base = build_model(solver=solver)
    n = 16
    env, p = _dr_env(n, solver, seed=BIN_SEED)
    assert (np.abs(p[:, 1] - 1) >= 0.03).all()      # a friction scale at 1 cannot tell the unscaled model apart
    models = _models(base, p)
    states, acts = _bin_corner_cases(o64, o32, base, p, n)
    right0 = lambda k: (models[k], acts[0][k])
    bar0 = 2 * _floor_median(o64, o32, states, right0, "force") + 1e-6
    _check_input(f"{solver} bin corner, unscaled, initial states",
                 _distance(o64, states, right0, lambda k: (base, acts[0][k]), "force"), bar0)
    env.reset(seed=5)
    _set_states(env, states)
    r = _tf_run(env, models, o64, o32, 3, lambda step: acts[step]).arrays()
    env.close()
    right = lambda k: (models[k % n], acts[k // n][k % n])
    return r, _distance(o64, r.states, right, lambda k: (base, acts[k // n][k % n]), "force")


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_bin_corner_parity(solver, oracle64, oracle32):
    """b. The cube pressed into a bin corner (draws of test_heavy_contact_parity's recipe taken by _bin_corner_cases, 16 DR
    envs, 3 steps): up to 13 contacts whose forces carry the scales.  That test's bars, the floors on the per-env models."""
    r, _ = _cached(("b", solver), lambda: _run_bin_corner(solver, oracle64, oracle32))
    ncon = np.array([len(p) for p in r.pairs])
    print(f"\nGPU ncon mean {ncon.mean():.1f} max {ncon.max():.0f}; " + r.summary(f"{solver} DR bin corner"))
    assert (ncon > 4).mean() > 0.5 and ncon.max() > 8
    assert np.median(r.qv) <= 2 * r.floor("qv", 0.5) + 1e-5
    assert np.quantile(r.qv, 0.9) <= 2 * r.floor("qv", 0.9) + 1e-4
    keep = ~r.near0 if solver == "pgs" else np.ones(len(r.qv), bool)
    assert keep.mean() >= 0.9
    assert r.qv[keep].max() <= 2 * r.floor("qv", 1.0) + 1e-3
    _force_bars(r)
    assert r.drop_gpu.sum() == 0 and r.drop_ora.sum() == 0


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_bin_corner_discrimination(solver, oracle64, oracle32):
    """b. The unscaled model is told from the right one by the per-contact forces (per env step: the largest per-contact
    relative distance), against the median bar of _force_bars, 2 x the floor's median + 1e-6.

    The states are those of the recipe on which the forces respond to the scales at all (_bin_corner_cases: a wedged
    cube's Newton forces do not carry the mass scale, and carry the friction scale only on the friction cone)."""
    r, dist = _cached(("b", solver), lambda: _run_bin_corner(solver, oracle64, oracle32))
    print()
    _check_discrimination(f"{solver} bin corner, unscaled", _gpu_force_err(r), dist, 2 * r.floor("force", 0.5) + 1e-6)


# ----------------------------------------------------------------------------- c. arm and pads sliding on the table
PAD_SHIFT = 0.05      # normalised action of the pan joint per step: the lateral shift of the pressed targets
PAD_STEPS = 4


def _pad_slide_cases(o64, base, p, n):
    """n pressed states (test_pad_contact_parity's recipe through _pressed_states) with their 4 actions each: the pressed
    target + N(0, 0.02) + a lateral shift of PAD_SHIFT per step on the pan joint, so the pads and links slide on the
    table and the friction rows are loaded.  A candidate is taken for env slot i if, on the fp64 oracle's own
    closed-loop steps with slot i's scales, the model with the friction scale on all pairs stays 1e-4 or more away
    (relative qvel) at each of the 4 steps: an arm that does not touch, or lifts off, cannot tell the two models apart
    (1e-4 = 10 x the class's median bar of 1e-5, the least distance at which the one-tenth criterion can hold for a
    GPU at the bar), and only while its contacts are with the table (the class: a link wedged against the bin is the
    box-hull class's matter).  The even slots take only candidates that hold a pad contact (two in five of those pressed on the
    table do; the rest rest on the links' hulls).  Selection by the oracle alone, before any GPU step."""
    from gym_so100.model import NPAIR_BOX, PAIR_MPR0, PAIR_PAD0
    rng = np.random.default_rng(13)

    def target(i):                     # test_pad_contact_parity's targets that press onto the table top
        return np.array([rng.uniform(-0.6, 0.6), rng.uniform(0.2, 1.3), rng.uniform(-1.4, -0.2),
                         rng.uniform(0.6, 1.6), rng.uniform(-1.5, 1.5), rng.uniform(-0.17, 1.5)])

    def on_table(pairs):               # the cube, the links' hulls and the pads against the table, nothing else
        return all(p == 8 or NPAIR_BOX <= p < PAIR_MPR0 or PAIR_PAD0 <= p < PAIR_PAD0 + 8 for p in pairs)
    states, acts, tried = [None] * n, [None] * n, 0
    while any(s is None for s in states) and tried < 8 * n:
        cs, ct = _pressed_states(base, o64, n, rng, target, [0.4, 0.95, 0.6, 1, 0, 0, 0])
        tried += n
        for st, tg in zip(cs, ct):
            pads = (R.oracle_step(o64, base, st, tg)[2][0] >= PAIR_PAD0).any()
            free = [i for i in range(n) if states[i] is None and (pads or i % 2)]
            if not free:
                continue
            i = min(free, key=lambda i: (i % 2, i)) if pads else free[0]
            m, mw = R.scaled_model(base, *p[i, :2]), _all_pairs_friction(base, *p[i, :2])
            a = tg + rng.normal(0, 0.02, (PAD_STEPS, 6))
            a[:, 0] += PAD_SHIFT * np.arange(1, PAD_STEPS + 1) * (1 if i % 4 < 2 else -1)
            a = a.astype(np.float32)
            if _tells_apart(o64, m, mw, st, a, "qv", 1e-4, pairs_ok=on_table):
                states[i], acts[i] = st, a
    assert all(s is not None for s in states), tried
    print(f"pad slide: {n} of {tried} pressed candidates taken")
    return states, np.array(acts)


def _run_pad_slide(solver, o64, o32):
    from gym_so100.model import PAIR_PAD0, build_model
    base = build_model(solver=solver)
    n = 16
    env, p = _dr_env(n, solver)
    models = _models(base, p)
    wrong_models = [_all_pairs_friction(base, *p[i, :2]) for i in range(n)]
    states, acts = _pad_slide_cases(o64, base, p, n)
    right = lambda k: (models[k % n], acts[k % n, k // n])
    wrong = lambda k: (wrong_models[k % n], acts[k % n, k // n])
    bar0 = 2 * _floor_median(o64, o32, states, right, "qv") + 1e-5
    _check_input(f"{solver} pad slide, friction on all pairs, initial states", _distance(o64, states, right, wrong, "qv"), bar0)
    env.reset(seed=3)
    _set_states(env, states)
    r = _tf_run(env, models, o64, o32, PAD_STEPS, lambda step: acts[:, step]).arrays()
    env.close()
    pad_ora = []
    for k, st in enumerate(r.states):                   # the oracle's pad contacts of the same solves
        m, a = right(k)
        pad_ora.append(int((R.oracle_step(o64, m, st, a)[2][0] >= PAIR_PAD0).sum()))
    pad_ora = np.array(pad_ora)
    return r, _distance(o64, r.states, right, wrong, "qv"), pad_ora


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_pad_slide_parity(solver, oracle64, oracle32):
    """c. The arm's pads and links pressed on the table and dragged sideways, 16 DR envs, 4 steps, the cube parked off the
    arm's way: the pairs without the cube must keep their friction.  Bars of test_pad_contact_parity."""
    from gym_so100.model import PAIR_PAD0
    r, _, pad_ora = _cached(("c", solver), lambda: _run_pad_slide(solver, oracle64, oracle32))
    pad_gpu = np.array([int((p >= PAIR_PAD0).sum()) for p in r.pairs])
    print(f"\nGPU pad contacts per env mean {pad_gpu.mean():.2f} (envs with any: {(pad_gpu > 0).mean():.2f}; oracle "
          f"{pad_ora.mean():.2f}, count mismatches {(pad_gpu != pad_ora).sum()}); " + r.summary(f"{solver} DR pad slide"))
    assert (pad_gpu > 0).sum() >= 10
    assert (pad_gpu != pad_ora).mean() <= 0.05
    assert np.median(r.qv) <= 2 * r.floor("qv", 0.5) + 1e-5
    assert np.quantile(r.qv, 0.9) <= 2 * r.floor("qv", 0.9) + 1e-4
    assert r.qv.max() <= 2 * r.floor("qv", 1.0) + 1e-3
    _force_bars(r)
    assert r.drop_gpu.sum() == 0 and r.drop_ora.sum() == 0


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_pad_slide_discrimination(solver, oracle64, oracle32):
    """c. The model with the friction scale on every pair (indistinguishable on cube-only states) is told from the right
    one.  Measured on the CPU oracle with a lateral shift of 0.03 / 0.1 per step on unselected touching states: the wrong
    model's median relative qvel distance is 1.0e-2 / 1.1e-2 (Newton) and 9.5e-3 / 1.1e-2 (PGS), 850 .. 920 x the median
    bar (2 x the floor's median 9e-7 + 1e-5); without a shift 4.9e-3 / 5.2e-3 (425 x / 453 x).  An env whose arm
    lifts off has distance 0, hence the selection of _pad_slide_cases."""
    r, dist, _ = _cached(("c", solver), lambda: _run_pad_slide(solver, oracle64, oracle32))
    print()
    _check_discrimination(f"{solver} pad slide, friction on all pairs", r.qv, dist, 2 * r.floor("qv", 0.5) + 1e-5)


# ----------------------------------------------------------------------------- d. random actions with noise
NOISE_SIGMA = 0.05
NOISE_OFFSET = 4096


def _noisy(env, sigma, episode, elapsed, i, act):
    """float32(a + sigma * hash_normal(key)): the action the kernel un-normalises for local env i"""
    z = R.action_noise(env.base_seed, env.env_offset + i, int(episode), int(elapsed), np.arange(6))
    return (np.asarray(act, np.float64) + float(sigma) * z).astype(np.float32)


def _run_noise_rollout(solver, o64, o32):
    from gym_so100 import SO100VecEnv
    from gym_so100.model import build_model
    base = build_model(solver=solver)
    n, T = 32, 5
    env = SO100VecEnv(n, device="cuda:0", autoreset=False, max_episode_steps=T, debug=True, solver=solver, seed=21,
                      env_offset=NOISE_OFFSET, domain_randomization=dict(action_noise=NOISE_SIGMA, **DR_RANGES))
    p = _seat_corners(env)
    models = _models(base, p)
    rng = np.random.default_rng(1000)
    lo, hi = np.array(base.action_lo[:]), np.array(base.action_hi[:])
    rows = np.arange(n)

    def act_fn(step):
        """random actions about the arm's pose, inside the actuators' linear range (kp 50 against a force limit of 3.5:
        0.07 rad, 0.04 of the action range; U(-1, 1) targets saturate every actuator, which hides the noise); the jaw
        of every 4th row at -1 / +1"""
        q = env.qpos[:, :6].cpu().numpy().astype(np.float64)
        a = np.clip((q - lo) / (hi - lo) * 2 - 1 + rng.uniform(-0.03, 0.03, (n, 6)), -1, 1)
        a[rows % 8 == 0, 5], a[rows % 8 == 4, 5] = -1.0, 1.0
        return a.astype(np.float32)
    res, fed, first = TF(), [], True
    for seg in (5, 5, 2):                             # episodes 1, 2, 3 (reset() starts a new one), elapsed 0 .. 4
        env.reset()
        # the jaw of the rows driven to -1 / +1 sits at that end of its range, so its actuator is not saturated and the
        # clamp of unnormalize (the noise pushes half of these targets past +-1) shows in the result
        q = env.qpos.clone()
        q[0::8, 5], q[4::8, 5] = float(np.float32(lo[5])), float(np.float32(hi[5]))
        env.set_state(q, env.qvel.clone())
        torch.cuda.synchronize()
        ep = env.episode.cpu().numpy()
        assert (env.elapsed == 0).all() and (ep == ep[0]).all()

        def oracle_act(step, i, a):
            fed.append(_noisy(env, p[i, 2], ep[i], step, i, a))
            return fed[-1]
        if first:                                     # the inputs discriminate: before any GPU step
            q0 = env.qpos.cpu().numpy().astype(np.float64)
            states = [(q0[i], np.zeros(12), np.zeros(12)) for i in range(n)]
            a0 = act_fn(0)
            rng = np.random.default_rng(1000)         # (the run draws the same actions again)
            _check_input(f"{solver} noisy rollout, noise-free action, initial states",
                         _distance(o64, states, lambda k: (models[k], _noisy(env, p[k, 2], ep[k], 0, k, a0[k])),
                                   lambda k: (models[k], a0[k]), "qv"), 1e-5)
            first = False
        _tf_run(env, models, o64, o32, seg, act_fn, res=res, oracle_act=oracle_act)
        assert (env.elapsed == seg).all() and bool(env.truncated.all()) == (seg == T)
    episodes = sorted(set(int(x) for x in env.episode.cpu().numpy()))
    env.close()
    r = res.arrays()
    assert episodes == [3] and len(fed) == len(r.states) == 12 * n
    dist = _distance(o64, r.states, lambda k: (models[k % n], fed[k]), lambda k: (models[k % n], r.states[k][3]), "qv")
    clamped = np.mean([np.any(np.abs(f) > 1) for f in fed])
    return r, dist, clamped


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_noise_rollout_parity(solver, oracle64, oracle32):
    """d. configs[4]'s workload: random actions with action noise sigma = 0.05 on 32 DR envs at env_offset 4096, 12
    teacher-forced steps over episodes 1..3 of 5 steps each (elapsed 0..4; the envs run without auto-reset as
    _step_all_builds needs, and reset() starts the next episode).  The oracle is fed float32(a + sigma *
    hash_normal(key)) of the host restatement.  The actions stay inside the actuators' linear range about the pose
    (_run_noise_rollout.act_fn), and a quarter of the rows hold the jaw at an end of its range with its action at
    -1 / +1, where the clamp of unnormalize acts on the noisy action.  Bars of test_step_parity_teacher_forced."""
    r, _, clamped = _cached(("d", solver), lambda: _run_noise_rollout(solver, oracle64, oracle32))
    print(f"\nenv steps with a noisy action component past +-1: {clamped:.2f}; " + r.summary(f"{solver} DR noisy rollout"))
    assert clamped > 0.05
    # (that test asks for more than 200 graded contacts in its 2,560 env steps: the same share of the 384 here; the cube
    # is spawned above the table and lands within the 5 steps of an episode)
    _step_parity_bars(r, solver, min_forces=200 * len(r.qv) // 2560, median_abs=1e-4 if solver == "newton" else None)


@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_noise_rollout_discrimination(solver, oracle64, oracle32):
    """d. The noise-free action is told from the noisy one: sigma = 0.05 moves a joint target by 0.05 to 0.1 rad, past the
    0.07 rad at which an actuator saturates."""
    r, dist, _ = _cached(("d", solver), lambda: _run_noise_rollout(solver, oracle64, oracle32))
    print()
    _check_discrimination(f"{solver} noisy rollout, noise-free action", r.qv, dist, 1e-5)


# ----------------------------------------------------------------------------- e. noise alone
@pytest.mark.parametrize("solver", SOLVERS)
def test_dr_noise_free_flight(solver, oracle64):
    """e. No contact (cube in the air, as test_free_flight_bit_close), unit scales, sigma = 0.05, env_offset 777: the GPU
    equals the fp64 oracle fed the host-noised action within that test's tolerances (qpos atol 2e-6; qvel atol 2e-4,
    rtol 1e-4), and the noise-free action is told from it: the distance and the GPU's error in units of the qvel
    tolerance (the class's bar: 1)."""
    from gym_so100.model import build_model
    model = build_model(solver=solver)
    n = 16
    env = _new_env(n, solver, seed=17, env_offset=777,
                   domain_randomization=dict(mass=(1.0, 1.0), friction=(1.0, 1.0), action_noise=NOISE_SIGMA))
    assert (env.dr_params[:, :2] == 1).all()
    env.reset(seed=7)
    qpos = env.qpos.clone()
    qpos[:, 8] = 0.6
    env.set_state(qpos, torch.zeros_like(env.qvel))
    torch.cuda.synchronize()
    lo, hi = np.array(model.action_lo[:]), np.array(model.action_hi[:])
    q0 = env.qpos.cpu().numpy().astype(np.float64)
    # the action that holds the pose: every actuator in its linear range, so the noise of every lane shows (a zero
    # action saturates three of the six: kp 50 against a force limit of 3.5)
    a = ((q0[:, :6] - lo) / (hi - lo) * 2 - 1).astype(np.float32)
    ep, el = env.episode.cpu().numpy(), env.elapsed.cpu().numpy()
    sigma = env.dr_params[:, 2].cpu().numpy()
    tol = lambda v, o: (np.abs(v - o) / (2e-4 + 1e-4 * np.abs(o))).max()
    ora, dist = [], []
    for i in range(n):                                # the oracle side first
        st = (q0[i], np.zeros(12), np.zeros(12))
        oq, ov, _ = R.oracle_step(oracle64, model, st, _noisy(env, sigma[i], ep[i], el[i], i, a[i]))
        ora.append((oq, ov))
        dist.append(tol(R.oracle_step(oracle64, model, st, a[i])[1], ov))
    dist = np.array(dist)
    _check_input(f"{solver} noisy free flight, noise-free action", dist, 1.0)
    _step_all_builds(env, a)
    gq, gv = env.qpos.cpu().numpy(), env.qvel.cpu().numpy()
    env.close()
    err = np.array([tol(gv[i], ora[i][1]) for i in range(n)])
    print(f"GPU qvel error in units of the tolerance: max {err.max():.2e}")
    for i in range(n):
        np.testing.assert_allclose(gq[i], ora[i][0], atol=2e-6)
        np.testing.assert_allclose(gv[i], ora[i][1], atol=2e-4, rtol=1e-4)
    assert np.mean(err < 0.1 * dist) >= 0.9
