"""What the float64 restatements alone say of the synthetic rasteriser meshes (tests/raster_synth_ref.py), before any
GPU run: the measured margins DELTA and EPS and the depth error (float32 numpy on the float32 oracle's frames against
float64 on the float64 oracle's), the share of pixels the margin rule leaves out, the per-band list counts of the
overflow meshes by the kernel's own box rule, that every listed triangle is visible on kept pixels, that the dyadic
cases are exact in float32, and that each deliberately broken restatement differs from the right one on kept pixels."""
import numpy as np
import pytest

import raster_synth_ref as S


@pytest.fixture(scope="module")
def fr64(model, oracle64):
    return S.frames(oracle64, model)


@pytest.fixture(scope="module")
def fr32(model, oracle32):
    return S.frames(oracle32, model)


@pytest.fixture(scope="module")
def cases(fr64):
    return S.cases(fr64[0][S.LINK])


def disagree(case, a, b):
    """bool [H, W]: the pixels on which two renders of a case differ in colour, label or winner (multisampled: also in
    the resolved colour or any sample's winner)."""
    if case["msaa"] is not None:                           # (a multisampled case is drawn by that launch alone)
        return np.any(a["rgb_msaa"] != b["rgb_msaa"], axis=-1) | np.any(a["swin"] != b["swin"], axis=0)
    d = (a["label"] != b["label"]) | (a["win"] != b["win"])
    if case["kind"] != "lit":                              # (the lit case's colours are graded by their share)
        d |= np.any(a["rgb"] != b["rgb"], axis=-1)
    return d


def test_the_cube_and_world_frames_are_exact(fr64, fr32):
    for fr in fr64 + fr32:
        assert np.array_equal(fr[0][0], np.eye(3)) and np.array_equal(fr[0][1], np.zeros(3))
        assert np.array_equal(fr[S.CUBE][0], np.eye(3))
        assert np.array_equal(np.asarray(fr[S.CUBE][1], np.float32), np.array(S.CUBE_POS, np.float32))
    assert not np.allclose(fr64[0][S.LINK][0], fr64[1][S.LINK][0])           # the arm does move between the envs


def test_measured_margins_shares_and_depth_error(cases, fr64, fr32):
    """The smallest DELTA and EPS at which float32 agrees with float64 on every kept pixel, by a fixed point: start at
    0, 0; a kept pixel that disagrees raises EPS to its depth gap when that gap is under 1e-4 (a depth flip), else DELTA
    to its edge distance (a coverage flip).  Then, at FACTOR times those: agreement on every kept pixel, the shares
    left out inside the caps, and the depth error of float32 on kept pixels."""
    delta = eps = 0.0
    pairs = []
    for name, case in cases.items():
        if case["exact"]:
            continue
        r64, r32 = S.reference(case, fr64, 64), S.reference(case, fr32, 32)
        for a, b in zip(r64, r32):
            pairs.append((name, case, a, b, disagree(case, a, b)))
        if "shift" in case:
            for a, b in zip(S.reference(case, fr64, 64, shifted=True), S.reference(case, fr32, 32, shifted=True)):
                pairs.append((name + "/shifted", case, a, b, disagree(case, a, b)))
    for _ in range(1000):
        moved = False
        for name, case, a, b, bad in pairs:
            hit = bad & (a["edge"] > delta) & (a["gap"] > eps)
            if not hit.any():
                continue
            moved = True
            flip = hit & (a["gap"] < 1e-4)
            if flip.any():
                eps = max(eps, float(a["gap"][flip].max()))
            if (hit & ~flip).any():
                delta = max(delta, float(a["edge"][hit & ~flip].max()))
        if not moved:
            break
    assert not moved
    nbad = sum(int(p[4].sum()) for p in pairs)
    print(f"measured DELTA {delta:.3g} px, EPS {eps:.3g} over {len(pairs)} images, {nbad} disagreeing pixels")
    worst_rel, worst_share, worst_share_msaa = 0.0, 0.0, 0.0
    for name, case, a, b, bad in pairs:
        keep = a["keep"]
        assert not (bad & keep).any(), name
        share = 1.0 - float(keep.mean())
        if case["msaa"] is None:
            worst_share = max(worst_share, share)
            assert share <= S.SHARE_CAP, (name, share)
        else:
            worst_share_msaa = max(worst_share_msaa, share)
            assert share <= S.SHARE_CAP_MSAA, (name, share)
        fg = keep & (a["win"] >= 0)
        assert np.all(a["depth"][a["win"] < 0] == 0.0) and np.all(a["label"][a["win"] < 0] == 255)
        if fg.any() and case["msaa"] is None:              # (the multisampled launch has no depth sink)
            rel = np.abs(b["depth"][fg].astype(np.float64) - a["depth"][fg]) / a["depth"][fg]
            worst_rel = max(worst_rel, float(rel.max()))
    print(f"left out at DELTA {S.DELTA:.3g}, EPS {S.EPS:.3g}: at most {worst_share:.4f} of an image, "
          f"{worst_share_msaa:.4f} multisampled; float32's largest relative depth error on kept pixels {worst_rel:.3g}")
    # the constants of the module docstring are these measurements, rounded up
    assert 0.8 * S.DELTA_MEASURED <= delta <= S.DELTA_MEASURED, delta
    assert 0.8 * S.EPS_MEASURED <= eps <= S.EPS_MEASURED, eps
    assert 0.8 * S.DEPTH_REL_MEASURED <= worst_rel <= S.DEPTH_REL_MEASURED, worst_rel
    assert S.FACTOR == 4 and S.DELTA == 4 * max(S.DELTA_MEASURED, S.DELTA_FLOOR)
    assert S.DEPTH_REL_BAR == 4 * S.DEPTH_REL_MEASURED and S.EPS == max(4 * S.EPS_MEASURED, 2 * S.DEPTH_REL_BAR)


def test_exact_cases_are_exact_in_float32(cases, fr64, fr32):
    """The dyadic meshes: float32 set-up equals float64 bit for bit, so do the images; every pixel is then graded."""
    for name, case in cases.items():
        if not case["exact"]:
            continue
        assert S.world_only(case["mesh"]) and case["W"] == 128 and case["H"] == 64
        p64 = S.project(case["mesh"], fr64[0], case["cam"], 128, 64, np.float64)
        p32 = S.project(case["mesh"], fr32[0], case["cam"], 128, 64, np.float32)
        for a, b in zip(p64[:3], p32[:3]):
            live = p64[3]
            assert np.array_equal(a[live].astype(np.float32), b[live]), name
            assert np.array_equal(b[live] * 1024, np.round(b[live] * 1024)), name      # on the dyadic grid
        assert np.array_equal(p64[3], p32[3])
        a, b = S.reference(case, fr64, 64)[0], S.render(case, fr64[0], np.float64)
        assert a["depth"].dtype == np.float32
        print(f"{name}: float64 (tan(pi/4) = 1 - 1.1e-16) differs from the exact float32 on "
              f"{int(disagree(case, a, b).sum())} pixels")
        assert a["keep"].all()
        fg = (a["win"] >= 0) & (b["win"] == a["win"])
        rel = np.abs(b["depth"][fg].astype(np.float64) - a["depth"][fg]) / a["depth"][fg]
        assert rel.max() <= S.DEPTH_REL_BAR / 4, (name, rel.max())


def test_ties_take_the_smaller_colour_then_the_smaller_label(cases, fr64):
    t, r, s = (S.reference(cases[k], fr64)[0] for k in ("ties", "ties_reversed", "ties_single"))
    for key in ("rgb", "label"):
        assert np.array_equal(t[key], r[key]), key
    assert np.array_equal(t["depth"].view(np.uint32), r["depth"].view(np.uint32))
    assert np.array_equal(t["depth"].view(np.uint32), s["depth"].view(np.uint32))      # the single triangle's depth bits
    assert np.array_equal(t["win"] >= 0, s["win"] >= 0)
    for x, y, colour, label in cases["ties"]["expect"]:
        got = int(t["rgb"][y, x, 0]) | int(t["rgb"][y, x, 1]) << 8 | int(t["rgb"][y, x, 2]) << 16
        assert (got, int(t["label"][y, x])) == (colour, label), (x, y)
    m4, m4r = S.reference(cases["ties_msaa4"], fr64)[0], S.reference(cases["ties_reversed_msaa4"], fr64)[0]
    assert np.array_equal(m4["rgb_msaa"], m4r["rgb_msaa"])


def test_list_counts_land_where_intended(cases, fr64, fr32):
    """By the kernel's own box rule, in float64 and float32 alike: band 0 of an overflow mesh lists exactly its count,
    all with boxes well clear of the thresholds; every listed triangle is the winner on at least 4 kept pixels (one
    pixel with all its samples in the multisampled meshes: a 64 x 16 band has 1024 pixels for more than 768
    triangles)."""
    for name, case in cases.items():
        if case["kind"] not in ("overflow", "msaa_overflow"):
            continue
        b64, b32 = S.list_counts(case, fr64[0], np.float64), S.list_counts(case, fr32[0], np.float32)
        for x, y in zip(b64, b32):
            for u, v in zip(x[1:], y[1:]):
                assert np.array_equal(u, v), name
        ref = S.reference(case, fr64)[0]
        keep = ref["keep"]
        (y0, y1), keys = b64[0][0], b64[0][-1]
        live = keys[keys > 0]
        if case["msaa"] is None:
            listed = b64[0][1]
            print(f"{name}: band rows {y0}..{y1 - 1} lists {len(listed)}; other bands {[len(b[1]) for b in b64[1:]]}")
            assert len(listed) == case["count"] == len(case["mesh"]["body"])
            assert live.min() >= 1.25 * S.BIG_PX
            wins = np.bincount(ref["win"][y0:y1][keep[y0:y1] & (ref["win"][y0:y1] >= 0)], minlength=len(keys))
            assert wins[listed].min() >= 4, (name, wins[listed].min())
        else:
            wide, mid = b64[0][1], b64[0][2]
            print(f"{name}: band rows {y0}..{y1 - 1} lists {len(wide)} wide, {len(mid)} mid")
            assert (len(wide), len(mid)) == (case["nwide"], case["nmid"])
            assert not np.any((live > 0.9 * S.BIG_PX) & (live < 1.1 * S.BIG_PX))
            assert not np.any((live > 0.9 * S.WIDE_KEYS) & (live < 1.1 * S.WIDE_KEYS))
            tag = name.split("_")[1]
            assert (len(wide) > S.BIG_CAP) == (tag == "wide") and (len(mid) > S.MID_CAP) == (tag == "mid")
            if tag == "under":
                assert len(wide) >= S.BIG_CAP - 8 and len(mid) >= S.MID_CAP - 70
            own = np.all(ref["swin"] == ref["swin"][0], axis=0) & keep        # every sample one triangle's
            wins = np.bincount(ref["swin"][0][y0:y1][own[y0:y1] & (ref["swin"][0][y0:y1] >= 0)], minlength=len(keys))
            assert wins[wide].min() >= 1 and wins[mid].min() >= 1, name


def test_near_plane_expectations(cases, fr64):
    case = cases["near_96x72"]
    ref = S.reference(case, fr64)[0]
    wins = np.bincount(ref["win"][ref["keep"] & (ref["win"] >= 0)], minlength=len(case["visible"]))
    print("near plane: kept pixels won per triangle", wins.tolist())
    assert np.array_equal(wins >= 4, case["visible"]) and np.all(wins[~case["visible"]] == 0)
    assert np.all(np.bincount(ref["win"].ravel(), minlength=len(wins))[~case["visible"]] == 0)
    assert not np.any(ref["win"] < 0)                                        # the backdrop fills the image
    sx, sy, iz, ok = S.project(case["mesh"], fr64[0], case["cam"], 96, 72)
    assert np.array_equal(ok, case["beyond"])
    big = np.abs(np.stack([sx, sy])).max(axis=(0, 2))
    assert 1e6 < big[9] < 1e8 < big[10] < 1e9, big


def test_each_broken_restatement_differs_on_kept_pixels(cases, fr64):
    # the unbroken rasteriser of the variants is the restatement
    for name in ("near_96x72", "ties", "edges", "random_129x33"):
        ref = S.reference(cases[name], fr64)[0]
        rgb, lab = S.draw(cases[name], fr64[0])
        assert np.array_equal(rgb, ref["rgb"]) and np.array_equal(lab, ref["label"]), name
    for name, rule in (("near_96x72", "near_ge"), ("near_96x72", "clip_vertex"), ("ties", "tie_larger"),
                       ("ties_reversed", "tie_larger"), ("edges", "exclusive")):
        ref = S.reference(cases[name], fr64)[0]
        rgb, lab = S.draw(cases[name], fr64[0], rule)
        diff = (np.any(rgb != ref["rgb"], axis=-1) | (lab != ref["label"])) & ref["keep"]
        print(f"{name} with {rule}: {int(diff.sum())} kept pixels differ")
        assert diff.sum() >= 4, (name, rule)
    # one that drops what its lists cannot take
    for name, case in cases.items():
        if case["kind"] not in ("overflow", "msaa_overflow"):
            continue
        drop = S.overflow_drops(case, fr64[0])
        over = case.get("count", 0) > S.BIG_CAP or case.get("nwide", 0) > S.BIG_CAP or case.get("nmid", 0) > S.MID_CAP
        assert bool(drop) == over, (name, len(drop))
        if not drop:
            continue
        ref = S.reference(case, fr64)[0]
        keepers = np.setdiff1d(np.arange(len(case["mesh"]["body"])), drop)
        got = S.render(case, fr64[0], mesh=S.subset_mesh(case["mesh"], keepers))
        key = "rgb" if case["msaa"] is None else "rgb_msaa"
        diff = np.any(got[key] != ref[key], axis=-1) & ref["keep"]
        print(f"{name} without its {len(drop)} overflowing triangles: {int(diff.sum())} kept pixels differ")
        assert diff.sum() >= len(drop), name
