"""The step kernels' hull support on the GPU (so100_hull_support_probe, include/so100.h) and the fused step built on
it.  The probe runs hull_support over test_hull_cells.py's direction families for every hull, through the cells'
block table (use_cells 1, the fused 2-wave build's path: one block load per support; 2, the 3-wave builds': the cell's
entry, then its block) and by the whole-hull scan (0, the split step's): all return the same vertex index and the same
point bits, the first maximal vertex of the fp32 FMA scores.  Then the fused
step's product builds (2 and 3 waves per SIMD) and its debug build against the split step on the benchmark's
random-action workload, bit for bit, on states where the mesh pairs (pair ids >= 14) are in contact."""
import ctypes

import numpy as np
import pytest
import torch

import test_hull_cells as thc
from gym_so100 import _native
from gym_so100.model import NHULL_ALL

pytestmark = pytest.mark.gpu


def P(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def probe_env():
    from gym_so100 import SO100VecEnv
    env = SO100VecEnv(4, device="cuda:0")
    yield env
    env.close()


@pytest.mark.parametrize("k", range(NHULL_ALL))
def test_probe_cells_and_scan_give_the_first_maximal_vertex(model, probe_env, k):
    env = probe_env
    X = thc.hull_verts(model, k)
    d = thc.directions(np.random.default_rng(100 + k), X)
    n = len(d)
    assert n > 10000                                         # (about 12 K; the last workgroup is ragged when n % 16)
    full = np.argmax(thc.scores(d, X, True), axis=1)         # first maximal vertex of the FMA scores
    dd = torch.from_numpy(d).cuda().contiguous()
    outs = []
    for use_cells in (1, 0, 2):
        out = torch.full((n, 4), -3.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _native.check(env.lib.so100_hull_support_probe(env._handle, k, P(dd), n, use_cells, P(out)),
                      "so100_hull_support_probe")
        outs.append(out.cpu().numpy())
    cells, scan, entry = outs
    np.testing.assert_array_equal(cells.view(np.uint32), scan.view(np.uint32))
    np.testing.assert_array_equal(entry.view(np.uint32), scan.view(np.uint32))
    for got in outs:
        np.testing.assert_array_equal(got[:, 3].view(np.int32), full)
        np.testing.assert_array_equal(got[:, :3].view(np.uint32), X[full].view(np.uint32))


def test_probe_rejects_a_hull_out_of_range(probe_env):
    env = probe_env
    z = torch.zeros(16, 4, device="cuda")
    assert env.lib.so100_hull_support_probe(env._handle, NHULL_ALL, P(z), 1, 1, P(z)) == -1
    assert "hull index out of range" in env.lib.so100_last_error().decode()
    # a zero direction has no cell: both paths scan the hull and return its first vertex among equal (zero) scores
    assert env.lib.so100_hull_support_probe(env._handle, 0, P(z), 1, 3, P(z)) == -1
    for use_cells in (1, 0, 2):
        out = torch.full((1, 4), -3.0, device="cuda")
        _native.check(env.lib.so100_hull_support_probe(env._handle, 0, P(z), 1, use_cells, P(out)), "probe")
        assert out.cpu().numpy()[0, 3:].view(np.int32)[0] == 0


def _mesh_contact(debug):
    """per env: the debug rows show a contact of a pair >= 14 (the mesh pairs: table-hull and the convex pairs)"""
    ncon = debug[:, 0].to(torch.int64)
    ids = debug[:, 48:64]
    hit = ((ids >= 14) & (torch.arange(16, device=debug.device)[None, :] < ncon[:, None])).any(dim=1)
    ovf = debug[:, _native.SO100_DBG_OVF + 1::6]
    c = torch.arange(ovf.shape[1], device=debug.device)[None, :] + 16
    return hit | ((ovf >= 14) & (c < ncon[:, None])).any(dim=1)


def test_fused_builds_match_split_on_the_bench_workload():
    """256 envs of the benchmark's workload (reset seed 1000, U[-1, 1] actions), 20 compared steps after 40: the fused
    product builds 2 and 3 equal the split step in state and outputs, the fused debug build in its debug rows too; at
    least 16 envs hold a mesh-pair contact at some compared step (the bench runs 0.32 narrowphase items per env step)."""
    from gym_so100 import SO100VecEnv
    n, warm, steps = 256, 40, 20
    kw = dict(device="cuda:0", seed=0)
    split, fdbg = SO100VecEnv(n, debug=True, **kw), SO100VecEnv(n, debug=True, **kw)
    f2, f3 = SO100VecEnv(n, **kw), SO100VecEnv(n, **kw)
    split.fused, fdbg.fused, f2.fused, f3.fused = False, True, True, True
    f2.fused_build, f3.fused_build = 2, 3
    assert not split.fused and fdbg.fused_build == 1 and f2.fused_build == 2 and f3.fused_build == 3
    envs = (split, fdbg, f2, f3)
    for e in envs:
        e.reset(seed=1000)
    g = torch.Generator(device="cuda").manual_seed(0)
    touched = torch.zeros(n, dtype=torch.bool, device="cuda")
    for it in range(warm + steps):
        a = torch.rand(n, 6, generator=g, device="cuda") * 2 - 1
        res = [e.step(a) for e in envs]
        if it < warm:
            continue
        torch.cuda.synchronize()
        touched |= _mesh_contact(split.debug)
        for name, e, r in zip(("debug build", "build 2", "build 3"), envs[1:], res[1:]):
            for what, x, y in zip(("obs", "reward", "terminated", "truncated"), r[:4], res[0][:4]):
                assert torch.equal(x, y), (it, name, what)
            for what in ("qpos", "qvel", "qacc_warmstart", "obs", "elapsed", "episode"):
                assert torch.equal(getattr(e, what), getattr(split, what)), (it, name, what)
        assert torch.equal(fdbg.debug, split.debug), (it, "debug rows")
    count = int(touched.sum())
    print(f"{count} of {n} envs held a mesh-pair contact at a compared step")
    for e in envs:
        e.close()
    assert count >= 16, count
