"""The support cells' block table (so100_hull_blocks, include/so100.h): the table the fused step's hull support reads,
one block of 16 entries per cube-map cell, behind the device model.  A block is the cell's list padded with its last
candidate when the list has 1..16 candidates, and 16 sentinel entries (index SO100_HULL_BLK_NONE) otherwise; the
kernel's lookup (the block alone when it holds a list, else the cell's list, else the whole hull) with the kernel's
fp32 FMA scores returns the full scan's first maximal vertex over test_hull_cells.py's direction families, and at
least 90 % of those directions are served by the block alone, so the lookup is not checked on its fallback only.
The shares on the shipped model, per hull 0..9 (these families put a quarter of their directions on cell boundaries
and axes): 0.891 0.874 0.835 0.808 1.000 0.921 1.000 1.000 0.864 0.935, 0.912 of all directions; the hulls below 0.9
(0..3 and 8) have cells whose lists are longer than a block, and those cells keep the list path.
CPU only (a host function of the C-ABI library)."""
import ctypes

import numpy as np
import pytest

import test_hull_cells as thc
from gym_so100 import _native
from gym_so100.model import NHULL_ALL

NCELL = _native.HULL_NCELL
BLK = _native.HULL_BLK
NONE = _native.HULL_BLK_NONE


@pytest.fixture(scope="module")
def tables(model):
    lib = _native.load()
    n = lib.so100_hull_cells(ctypes.byref(model), None, None, 0)
    assert n > 0, lib.so100_last_error()
    cells = np.zeros(NHULL_ALL * NCELL, np.uint32)
    cand = np.zeros((n, 4), np.float32)
    assert lib.so100_hull_cells(ctypes.byref(model), ctypes.c_void_p(cells.ctypes.data),
                                ctypes.c_void_p(cand.ctypes.data), n) == n
    nb = lib.so100_hull_blocks(ctypes.byref(model), None, 0)
    assert nb == NHULL_ALL * NCELL * BLK, lib.so100_last_error()
    blk = np.full((nb, 4), 7.0, np.float32)
    assert lib.so100_hull_blocks(ctypes.byref(model), ctypes.c_void_p(blk.ctypes.data), nb) == nb
    assert lib.so100_hull_blocks(ctypes.byref(model), ctypes.c_void_p(blk.ctypes.data), nb - 1) == -1
    assert lib.so100_hull_blocks(None, None, 0) == -1
    return cells, cand, blk.reshape(NHULL_ALL * NCELL, BLK, 4)


def test_abi_and_symbols():
    lib = _native.load()
    assert lib.so100_abi_version() == _native.ABI_VERSION      # (additions only: the version stays)
    for fn in ("so100_hull_blocks", "so100_hull_support_probe"):
        assert fn in _native.EXPORTED_SYMBOLS and hasattr(lib, fn)
    assert lib.so100_hull_support_probe(None, 0, ctypes.c_void_p(1), 1, 1, ctypes.c_void_p(1)) == -1
    assert "so100_hull_support_probe: bad arguments" in lib.so100_last_error().decode()


def test_every_block_is_its_cells_padded_list_or_the_sentinel(tables):
    cells, cand, blk = tables
    cnt, start = (cells & 255).astype(np.int64), (cells >> 8).astype(np.int64)
    has = (cnt >= 1) & (cnt <= BLK)
    assert has.any() and (~has).any(), "both kinds of block occur in the model"
    src = start[:, None] + np.minimum(np.arange(BLK)[None, :], np.maximum(cnt, 1)[:, None] - 1)
    want = cand[np.where(has[:, None], src, 0)]
    np.testing.assert_array_equal(blk[has].view(np.uint32), want[has].view(np.uint32))
    np.testing.assert_array_equal(blk[~has][:, :, :3].view(np.uint32), 0)
    np.testing.assert_array_equal(blk[~has][:, :, 3].view(np.uint32), NONE)
    # no block that holds a list carries the sentinel index
    assert np.all(blk[has][:, :, 3].view(np.uint32) != NONE)


def fma_scores_rows(d, P):
    """sup_score of direction r against its own candidates P[r] (rows x candidates x 3), fp32 FMA rounding"""
    d64, P64 = d.astype(np.float64), P.astype(np.float64)
    t = (d64[:, None, 0] * P64[:, :, 0]).astype(np.float32).astype(np.float64)
    t = (d64[:, None, 1] * P64[:, :, 1] + t).astype(np.float32).astype(np.float64)
    return (d64[:, None, 2] * P64[:, :, 2] + t).astype(np.float32)


@pytest.mark.parametrize("k", range(NHULL_ALL))
def test_block_lookup_gives_the_scan_support(model, tables, k):
    cells, cand, blk = tables
    X = thc.hull_verts(model, k)
    d = thc.directions(np.random.default_rng(100 + k), X)
    c = k * NCELL + thc.cell_of(d)
    b = blk[c]                                                # rows x 16 x 4
    idx = b[:, :, 3].view(np.int32)
    took = idx[:, 0] != NONE
    print(f"hull {k}: {len(d)} directions, {took.mean():.4f} served by the block alone")
    assert took.any() and len(d) > 10000
    S = thc.scores(d, X, True)
    full = np.argmax(S, axis=1)                               # the scan's first maximal vertex
    # the block path: the 16 lanes' (score, index) maximum, the lower index among equal scores
    sb = fma_scores_rows(d[took], b[took][:, :, :3])
    ib = idx[took].astype(np.int64)
    best = sb.max(axis=1, keepdims=True)
    got = np.where(sb == best, ib, np.iinfo(np.int64).max).min(axis=1)
    np.testing.assert_array_equal(got, full[took])
    np.testing.assert_array_equal(b[took][np.arange(took.sum()), np.argmax(ib == got[:, None], axis=1), :3], X[got])
    # a sentinel block: the cell's list when it has one, else the whole hull (which is `full` itself)
    e = cells[c]
    for r in np.nonzero(~took)[0]:
        n, s = int(e[r] & 255), int(e[r] >> 8)
        assert n == 0 or n > BLK
        if n:
            li = cand[s:s + n, 3].view(np.int32)
            assert li[np.argmax(S[r, li])] == full[r]


def test_nine_in_ten_directions_take_the_block_path(model, tables):
    """over every hull's direction families together (the per-hull shares: the module docstring)"""
    _, _, blk = tables
    took = []
    for k in range(NHULL_ALL):
        d = thc.directions(np.random.default_rng(100 + k), thc.hull_verts(model, k))
        took.append(blk[k * NCELL + thc.cell_of(d), 0, 3].view(np.uint32) != NONE)
    share = np.concatenate(took).mean()
    print(f"{sum(len(t) for t in took)} directions, {share:.4f} served by the block alone; per hull "
          + " ".join(f"{t.mean():.3f}" for t in took))
    assert share >= 0.9, share
