"""CPU checks of the DR / epilogue test infrastructure (tests/dr_ref.py): the hashes' statistics over the action-noise
key space, and, on the oracle alone, how far the wrong DR models that tests/test_gpu_dr.py is meant to catch sit from
the right one: the discriminating power of those GPU tests, shown without a GPU."""
import ctypes

import numpy as np
import pytest

import dr_ref as R


# ----------------------------------------------------------------------------- hashes
def test_splitmix64_vectors():
    """the published first outputs of SplitMix64 seeded with 0 (the state advances by the golden gamma per draw)"""
    gamma = 0x9E3779B97F4A7C15
    assert int(R.splitmix64(0)) == 0xE220A8397B1DCDAF
    assert int(R.splitmix64(gamma)) == 0x6E789E6AA1B965F4
    assert int(R.splitmix64(2 * gamma)) == 0x06C45D188009454F
    x = np.arange(5, dtype=np.uint64)
    assert [int(v) for v in R.splitmix64(x)] == [int(R.splitmix64(int(v))) for v in x]
    from gym_so100.vec_env import _splitmix64
    assert np.array_equal(R.splitmix64(x), _splitmix64(x))
    assert 0 <= int(R.episode_seed(7, 1000, 3)) < 2 ** 32 and R.episode_seed(7, 1000, 3) != R.episode_seed(7, 1000, 4)
    assert R.episode_seed(7, 1000, 3) != R.episode_seed(7, 1001, 3) and R.episode_seed(8, 1000, 3) != R.episode_seed(7, 1000, 3)


def test_hash_normal_statistics_over_the_noise_key_space():
    """hash_normal over 202,752 keys of env x episode x elapsed x lane (64 x 8 x 66 x 6, env_offset 4096): mean within
    4 / sqrt(N) of 0, variance within 2 % of 1, lag-1 correlation along each of the four axes within 4 / sqrt(N),
    no duplicate key.  (The key layout holds elapsed < 2^17 and episode < 2^20 before keys alias: DESIGN.md §5.)"""
    env, ep, el, lane = np.meshgrid(np.arange(4096, 4096 + 64), np.arange(1, 9), np.arange(66), np.arange(6), indexing="ij")
    keys = R.action_noise_key(12345, env, ep, el, lane)
    n = keys.size
    assert n >= 200000 and len(np.unique(keys)) == n
    z = R.hash_normal(keys)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.7
    assert abs(z.mean()) <= 4 / np.sqrt(n)
    assert abs(z.var() - 1) <= 0.02
    zs = (z - z.mean()) / z.std()
    for ax in range(4):
        a, b = np.swapaxes(zs, 0, ax)[:-1], np.swapaxes(zs, 0, ax)[1:]
        assert abs((a * b).mean()) <= 4 / np.sqrt(a.size), ax
    # the lanes of one step and the steps of one lane draw different values
    assert (np.abs(np.diff(z, axis=3)) > 0).all() and (np.abs(np.diff(z, axis=2)) > 0).all()
    u = R.hash_uniform(keys)
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) <= 4 / np.sqrt(12 * n)
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))      # on the 2^-24 grid: exact in fp32


def test_goal_sample_boxes(model):
    lo_bin, hi_bin = np.array(model.goal_bin_lo[:]), np.array(model.goal_bin_hi[:])
    for count, binbox in ((0, False), (4999, False), (5000, True), (5001, True)):
        g = np.array([R.goal_sample(3, 1000 + i, 2, (0.1, 0.8), count, model) for i in range(64)])
        lo, hi = R.goal_box((0.1, 0.8), count, model)
        assert ((g >= lo) & (g <= hi)).all() and len(np.unique(g[:, 0])) == 64
        assert np.allclose(lo, lo_bin, atol=1e-7) == binbox
        if not binbox:
            assert np.allclose(lo, [0.07, 0.77, 0.01], atol=1e-7) and np.allclose(hi, [0.13, 0.83, 0.05], atol=1e-7)
    assert (R.goal_sample(3, 1000, 2, (0.1, 0.8), 0, model) != R.goal_sample(3, 1000, 3, (0.1, 0.8), 0, model)).all()


# ----------------------------------------------------------------------------- scaled_model
def test_scaled_model_touches_only_the_listed_fields(model):
    from gym_so100.model import NPAIR, SO100Model
    before = bytes(model)
    m = R.scaled_model(model, 0.8, 1.2)
    assert bytes(model) == before and isinstance(m, SO100Model)
    cube_pairs = [p for p in range(NPAIR) if R.CUBE_BODY in (model.pair_body1[p], model.pair_body2[p])]
    assert 0 < len(cube_pairs) < NPAIR
    for name, ctype in SO100Model._fields_:
        a, b = getattr(model, name), getattr(m, name)
        if not hasattr(a, "_length_"):
            assert a == b, name
            continue
        a = np.frombuffer(a, dtype=np.int32 if ctypes.sizeof(ctype) // max(1, _count(ctype)) == 4 else np.float64)
        b = np.frombuffer(b, dtype=a.dtype)
        if name == "body_mass":
            want = a.copy()
            want[R.CUBE_BODY] *= 0.8
        elif name == "body_inertia":
            want = a.copy().reshape(-1, 3)
            want[R.CUBE_BODY] *= 0.8
        elif name == "pair_friction":
            want = a.copy().reshape(-1, 3)
            want[cube_pairs] *= 1.2
        else:
            want = a
        assert np.array_equal(b, np.ravel(want)), name
    assert m.body_mass[R.CUBE_BODY] == model.body_mass[R.CUBE_BODY] * 0.8
    assert list(m.body_invweight0[R.CUBE_BODY]) == list(model.body_invweight0[R.CUBE_BODY])


def _count(ctype):
    n = 1
    while hasattr(ctype, "_length_"):
        n *= ctype._length_
        ctype = ctype._type_
    return n


# ----------------------------------------------------------------------------- DR sensitivity on the oracle alone
@pytest.mark.parametrize("solver", ["newton", "pgs"])
def test_sliding_cube_tells_wrong_models_apart(solver, oracle64, oracle32):
    """Class a of tests/test_gpu_dr.py (16 states from seeds 1000..1015 at the corners of the DR ranges, one env step of 10
    substeps): relative qvel distance from the right oracle, min / median over the states.

        wrong model         Newton             PGS
        unscaled            5.9e-3 / 2.4e-2    5.6e-3 / 2.2e-2
        inertia unscaled    7.0e-3 / 2.0e-2    8.0e-3 / 1.7e-2

    against the fp32 oracle's 1.1e-6 at the median and 4e-6 at worst.  Asserted: the median 1e-2 or more (1000 x the
    class's median bar of 1e-5, where the GPU test needs 100 x), every state 3e-3 or more and 100 x the fp32 oracle's worst."""
    from gym_so100.model import build_model
    base = build_model(solver=solver)
    zero = np.zeros(6, np.float32)
    dist = {"unscaled": [], "inertia unscaled": []}
    floor = []
    for k, seed in enumerate(range(1000, 1016)):
        ms, fs = R.CORNERS[k % 2]
        m = R.scaled_model(base, ms, fs)
        mi = R.scaled_model(base, ms, fs)
        for j in range(3):
            mi.body_inertia[R.CUBE_BODY][j] = base.body_inertia[R.CUBE_BODY][j]
        st = R.sliding_cube_state(oracle64, m, seed)
        v = R.oracle_step(oracle64, m, st, zero)[1]
        dist["unscaled"].append(R.rel_dist(R.oracle_step(oracle64, base, st, zero)[1], v))
        dist["inertia unscaled"].append(R.rel_dist(R.oracle_step(oracle64, mi, st, zero)[1], v))
        floor.append(R.rel_dist(R.oracle_step(oracle32, m, st, zero)[1], v))
    print(f"\n{solver}: fp32 floor median {np.median(floor):.1e} max {max(floor):.1e}")
    for name, d in dist.items():
        print(f"{solver} {name}: min {min(d):.1e} median {np.median(d):.1e}")
        assert np.median(d) >= 1e-2 and min(d) >= 3e-3 and min(d) >= 100 * max(floor), name
    assert np.median(floor) <= 1e-5


@pytest.mark.parametrize("solver", ["newton", "pgs"])
def test_bin_corner_forces_tell_the_unscaled_model_apart(solver, oracle64, oracle32):
    """Class b (test_heavy_contact_parity's recipe, 16 states at the corners of the DR ranges, one env step): per state the
    largest per-contact relative force distance of the unscaled model from the right one, against the fp32 oracle's.

    PGS: 0.47 or more in every state (fp32 oracle: 2.6e-3 at worst).
    Newton: 4e-3 .. 0.22 in 13 of the 16 states and 8e-5 .. 9e-5, the fp32 oracle's own error, in the other three.  The
    cube is wedged between two walls and the floor at friction 1 (normal forces of 120 .. 250 N against a weight of
    0.49 N), so Newton's minimiser sets the forces by the penetration and the friction limit: the mass scale alone
    moves them by 1e-4, and the friction scale only in the states where the limit binds.
    Asserted: the median 3e-2 or more for both solvers and 100 x the median bar of _force_bars (2 x the floor's median +
    1e-6); every state 0.1 or more under PGS; and under Newton the insensitivity to the mass scale itself (scales
    (0.8, 1) and (1.2, 1) within 1e-3 of the unscaled model in every state), so that the finding stays on record."""
    from gym_so100.model import build_model
    base = build_model(solver=solver)
    n = 16
    rng = np.random.default_rng(7)
    qpos, qvel = R.bin_corner_states(base, n, rng)
    act = rng.uniform(-0.2, 0.2, (n, 6)).astype(np.float32)

    def force_dist(m, mw, i):
        st = (qpos[i], qvel[i], np.zeros(12))
        s, sw = R.oracle_step(oracle64, m, st, act[i])[2], R.oracle_step(oracle64, mw, st, act[i])[2]
        return R.force_dist(sw[1], s[1]).max() if np.array_equal(s[0], sw[0]) else np.inf
    dist, floor = [], []
    for i in range(n):
        m = R.scaled_model(base, *R.CORNERS[i % 2])
        dist.append(force_dist(m, base, i))
        st = (qpos[i], qvel[i], np.zeros(12))
        s, s32 = R.oracle_step(oracle64, m, st, act[i])[2], R.oracle_step(oracle32, m, st, act[i])[2]
        assert len(s[0]) >= 12 and np.array_equal(s[0], s32[0])
        floor += list(R.force_dist(s32[1], s[1]))
    dist = np.array(dist)
    print(f"\n{solver}: unscaled-model force distance min {dist.min():.1e} median {np.median(dist):.1e} max {dist.max():.1e}; "
          f"fp32 floor median {np.median(floor):.1e} max {max(floor):.1e}")
    assert np.median(dist) >= 3e-2 and np.median(dist) >= 100 * (2 * np.median(floor) + 1e-6)
    if solver == "pgs":
        assert dist.min() >= 0.1
    else:
        mass_only = np.array([max(force_dist(R.scaled_model(base, ms, 1.0), base, i) for ms in (0.8, 1.2)) for i in range(n)])
        print(f"newton: mass scale alone, max {mass_only.max():.1e}")
        assert mass_only.max() < 1e-3
