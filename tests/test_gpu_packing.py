"""Env packing of the fused step (so100_step.hip so100_order_kernel): before each launch the envs of
every block of 64 consecutive envs (aligned to the start of the block's XCD range) are ranked by their last step's solver
cost and cut into the waves' quartets, so envs that need a second Newton pass or hold long contact lists share a wave
instead of making three cheap wave-mates wait.  A schedule only: which envs share a wave must never change a result.
Ragged sizes (a multiple of neither 4 nor 64, blocks cut short by the XCD range boundaries), more than 256 groups (the
order kernel runs), packing forced on (auto leaves it off for grids that are resident at once)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PACK_BLOCK = 64
XCDS = 8
OUTPUTS = ("qpos", "qvel", "obs", "qacc_warmstart", "elapsed", "episode")


def _ranges(n):
    """(first group, groups) of each XCD range: XCD x runs the launch slots 8 r + x."""
    ng = (n + 3) // 4
    out, start = [], 0
    for x in range(XCDS):
        cnt = (ng - x + XCDS - 1) // XCDS
        out.append((start, cnt))
        start += cnt
    return out


def _check_order(order, n):
    ng = (n + 3) // 4
    assert order.shape == (4 * ng,)
    real = order[(order >= 0) & (order < n)]
    assert np.array_equal(np.sort(real), np.arange(n)), "the order is not a permutation of the envs"
    assert np.all(order[(order < 0) | (order >= n)] >= n) and order.size - real.size == 4 * ng - n, "padding"
    quart = order.reshape(ng, 4)
    for x, (start, cnt) in enumerate(_ranges(n)):
        q = quart[x::XCDS]
        assert q.shape[0] == cnt
        blk = (q - 4 * start) // PACK_BLOCK
        assert np.all((q >= 4 * start) & (q < 4 * (start + cnt))), "a quartet left its XCD range"
        assert np.all(blk == blk[:, :1]), "a quartet holds envs of two blocks"


def _make(n, pack, **kw):
    from gym_so100 import SO100VecEnv
    kw.setdefault("seed", 7)
    env = SO100VecEnv(n, device="cuda:0", **kw)
    env.env_packing = pack
    assert env.fused and env.env_packing == bool(pack)
    return env


@pytest.mark.parametrize("n", [1173, 2051])
def test_packed_order_is_a_permutation(n):
    env = _make(n, True, autoreset=False, max_episode_steps=0)
    env.reset(seed=7)
    g = torch.Generator(device="cuda").manual_seed(0)
    for step in range(6):
        e0 = env.elapsed.clone()
        env.step(torch.rand(n, 6, generator=g, device="cuda") * 2 - 1)
        torch.cuda.synchronize()
        order = env.env_order()
        _check_order(order, n)
        assert torch.equal(env.elapsed - e0, torch.ones_like(e0)), "an env was stepped other than once"
    natural = np.sort(order.reshape(-1, 4), axis=1)
    assert np.any(natural[:, 1:] - natural[:, :-1] != 1) or np.any(natural[:, 0] % 4 != 0), \
        "the quartets are still the natural groups: the remaining tests would pass vacuously"
    env.close()


@pytest.mark.parametrize("variant,task,dr", [("joint", "so100_cube_to_bin", False), ("joint", "so100_goal", True),
                                               ("ee", "so100_touch_cube", False)])
def test_packed_bitwise_against_split(variant, task, dr):
    n = 1173
    kw = dict(task=task, seed=7, max_episode_steps=3, variant=variant,
              domain_randomization=(dict(mass=(0.8, 1.2), friction=(0.8, 1.2), action_noise=0.05) if dr else None))
    fused = _make(n, True, **kw)
    from gym_so100 import SO100VecEnv
    split = SO100VecEnv(n, device="cuda:0", **kw)
    split.fused = False
    assert not split.fused
    for e in (fused, split):
        e.reset(seed=500)
    if variant == "ee":
        gm = torch.Generator(device="cuda").manual_seed(3)
        pos = fused.mocap[:, :3] + (torch.rand(n, 3, generator=gm, device="cuda") - 0.5) * 0.08
        for e in (fused, split):
            e.set_mocap(pos)
    g = torch.Generator(device="cuda").manual_seed(5)
    for _ in range(8):
        a = torch.rand(n, 6, generator=g, device="cuda") * 2 - 1
        rf, rs = fused.step(a), split.step(a)
        torch.cuda.synchronize()
        for name, x, y in zip(("obs", "reward", "terminated", "truncated"), rf[:4], rs[:4]):
            if isinstance(x, dict):
                for k in x:
                    assert torch.equal(x[k], y[k]), (name, k)
            else:
                assert torch.equal(x, y), name
        for name in OUTPUTS:
            assert torch.equal(getattr(fused, name), getattr(split, name)), name
    order = fused.env_order().reshape(-1, 4)
    assert np.any(order[:, 0] % 4 != 0) or np.any(np.diff(order, axis=1)[order[:, 1:] < n] != 1), "packing never moved an env"
    fused.close()
    split.close()


@pytest.fixture(scope="module")
def long_lists(model, oracle64):
    from test_gpu_parity import _long_list_states
    states, targets, _ = _long_list_states(model, oracle64, 16)
    return states, targets


@pytest.mark.parametrize("debug", [False, True])
def test_packed_bitwise_on_off_long_lists(debug, long_lists):
    """Packing on against off on envs whose contact lists pass the 16 held on chip (the pool path, newton_solve<true>
    chosen per wave): a quarter of the envs start from the long-lists pool test's folded poses."""
    n = 1173
    states, targets = long_lists
    runs = []
    for pack in (True, False):
        env = _make(n, pack, autoreset=False, max_episode_steps=0, debug=debug)
        env.reset(seed=3)
        q, v, w = (t.cpu().numpy().copy() for t in (env.qpos, env.qvel, env.qacc_warmstart))
        act = np.random.default_rng(5).uniform(-1, 1, (n, 6)).astype(np.float32)
        for i in range(0, n, 4):                         # every fourth env: one long list per natural group
            s = states[(i // 4) % len(states)]
            q[i], v[i], w[i] = s[0], s[1], s[2]
            act[i] = targets[(i // 4) % len(targets)]
        env.set_state(q, v, w)
        act = torch.from_numpy(act).cuda()
        longest, drops, outs = 0, 0, []
        for step in range(4):
            r = env.step(act)
            torch.cuda.synchronize()
            longest = max(longest, int(env.contact_counts().max().item()))
            drops += int(env.ncon_dropped.sum().item())
            outs.append([t.cpu().numpy().copy() for t in r[1:4]] +
                        [getattr(env, name).cpu().numpy().copy() for name in OUTPUTS + (("debug",) if debug else ())])
        runs.append((outs, env.contact_counts().cpu().numpy().copy(), env.env_order().copy()))
        assert drops == 0
        assert longest > 16, "no env held more than the 16 contacts kept on chip: the pool path was not reached"
        env.close()
    for so, sf in zip(runs[0][0], runs[1][0]):
        for a, b in zip(so, sf):
            assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][2], runs[1][2]), "the two runs used the same order"


def test_packed_separation_cache():
    """The convex pairs' separating-direction cache is per env: 12 packed steps (the envs change rows and waves) against
    the natural quartets.  A slot indexed by the row would only ever hold a stale certificate, which no state can show;
    the contact lists would, so the per-env contact counts are compared after every step."""
    n = 1173
    runs = []
    for pack in (True, False):
        env = _make(n, pack, autoreset=False, max_episode_steps=0)
        env.reset(seed=21)
        g = torch.Generator(device="cuda").manual_seed(9)
        counts = []
        for _ in range(12):
            env.step(torch.rand(n, 6, generator=g, device="cuda") * 2 - 1)
            counts.append(env.contact_counts().cpu().numpy().copy())
        runs.append((np.array(counts), env.qpos.cpu().numpy().copy(), env.qvel.cpu().numpy().copy()))
        env.close()
    assert np.array_equal(runs[0][0], runs[1][0]), "per-env contact counts differ between the packed and the natural order"
    assert runs[0][0].max() > 0
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
