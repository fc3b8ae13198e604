"""Cast shadows (ABI 23: so100_shadow, so100_render_shadow, so100_render_casters, so100_shadow_bytes) without a device:
the numpy restatement (tests/render_shadow_ref.py) against a known answer, its light = -1 and self-shadowing
properties, the float32 floor the GPU test's bar is built on, and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import render_aux_ref as A
import render_ref
import render_shadow_ref as S
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R
from gym_so100.sb3 import SO100SB3VecEnv

CUBE_A = 0.04                # the cube's side (so100_render.npz body 8: +-0.02)


@pytest.fixture(scope="module")
def scene():
    return R.load_scene()


def lifted_frames(oracle, model, x, y, z):
    return A.frames_of(oracle, model, np.array([0, 0, 0, 0, 0, 0, x, y, z, 1, 0, 0, 0], np.float64))


def project(cam, P, W, H):
    c = (np.asarray(P) - cam["pos"]) @ cam["mat"]
    th = np.tan(0.5 * np.radians(cam["fovy"]))
    return np.array([(c[0] / -c[2] / (th * W / H) * 0.5 + 0.5) * W, (0.5 - c[1] / -c[2] / th * 0.5) * H])


# --------------------------------------------------------------------------------------------------- known answer
@pytest.mark.parametrize("map_size", [32, 64])
@pytest.mark.parametrize("W,H", [(64, 48), (96, 72)])
def test_lifted_cube_drops_its_shadow_where_the_light_puts_it(scene, model, oracle64, W, H, map_size):
    """Only the cube casts.  Its centre at height h over the table (z = 0) is moved by h * d_xy / -d_z: the shadow on
    the table is point-symmetric about that point, so the shadowed table pixels' centroid is its projection, to within a
    pixel (sampling at pixel centres) and a texel (the map's sampling).  The shadow of a cube of side a under a light
    whose horizontal shift per unit height is (sx, sy) is the square swept along a * (sx, sy): area a^2 (1 + |sx| +
    |sy|); the count may miss it by one pixel row of the shadow's extent, widened by a texel."""
    lab, _ = R.segment_labels(scene)
    cast = (np.asarray(scene["body"]) == 8).astype(np.uint8)
    cam = render_ref.camera_dict(R.make_camera(scene, "top"))
    cx, cy, h = 0.25, 0.45, 0.15
    fr, ee = lifted_frames(oracle64, model, cx, cy, h)
    sh = S.shadow_dict(R.make_shadow(scene, map_size=map_size))
    assert sh["light"] == R.SHADOW_LIGHT == 1
    img, dep, lb, mask = S.render(scene["tri"], scene["body"], scene["rgb"], lab, cast, fr, cam, W, H, sh, target=ee)
    d = cam["light_dir"][1]
    shift = np.array([d[0], d[1]]) / -d[2]
    centre = np.array([cx + h * shift[0], cy + h * shift[1], 0.0])
    p0 = project(cam, centre, W, H)
    m_per_px = 1.0 / np.linalg.norm(project(cam, centre + [1.0, 0, 0], W, H) - p0)
    texel_px = 2.0 * sh["radius"] / map_size / m_per_px
    on_table = mask & (lb == 0)
    ys, xs = np.nonzero(on_table)
    got = np.array([xs.mean() + 0.5, ys.mean() + 0.5])
    area_px = CUBE_A ** 2 * (1 + abs(shift[0]) + abs(shift[1])) / m_per_px ** 2
    row_px = (CUBE_A * (1 + abs(shift[0])) + 2.0 * sh["radius"] / map_size) / m_per_px
    print(f"{W}x{H} map {map_size}: centroid {got}, analytic {p0}; count {len(xs)}, analytic area {area_px:.1f} px, "
          f"row {row_px:.1f} px, texel {texel_px:.2f} px")
    assert np.linalg.norm(got - p0) <= 1.0 + texel_px
    assert abs(len(xs) - area_px) <= row_px
    # shadowed pixels take the dark image's colour, the others the full image's; depth and labels are the plain ones
    full, dep0, lb0 = A.render(scene["tri"], scene["body"], scene["rgb"], lab, fr, cam, W, H, target=ee)
    assert np.array_equal(dep, dep0) and np.array_equal(lb, lb0)
    assert np.array_equal(img[~mask], full[~mask]) and np.all(np.any(img[on_table] != full[on_table], axis=-1))
    assert np.all(img[on_table].astype(int) <= full[on_table].astype(int))


# ---------------------------------------------------------------------------------------------------- properties
def test_no_light_no_shadow_and_no_self_shadowing(scene, model, oracle64):
    lab, _ = R.segment_labels(scene)
    cam = render_ref.camera_dict(R.make_camera(scene, "top"))
    W, H = 64, 48
    fr, ee = A.frames_of(oracle64, model, S.LIFTED.astype(np.float64))
    plain = A.render(scene["tri"], scene["body"], scene["rgb"], lab, fr, cam, W, H, target=ee)
    off = S.shadow_dict(R.make_shadow(scene, light=-1))
    img, dep, lb, mask = S.render(scene["tri"], scene["body"], scene["rgb"], lab, R.shadow_casters(scene), fr, cam, W, H,
                                  off, target=ee)
    assert not mask.any() and np.array_equal(img, plain[0]) and np.array_equal(dep, plain[1])
    # the table alone in the scene's map (a caster array of its 12 triangles) would shadow itself nowhere: it is flat,
    # and with the default casters it is not even drawn into the map
    cast = R.shadow_casters(scene)
    mat, _ = R.material_ids(scene)
    assert int((cast == 0).sum()) == 12 and np.all(mat[cast == 0] == R.MATERIALS.index("table"))
    sh = S.shadow_dict(R.make_shadow(scene))
    empty = np.zeros_like(cast)
    img, dep, lb, mask = S.render(scene["tri"], scene["body"], scene["rgb"], lab, empty, fr, cam, W, H, sh, target=ee)
    assert not mask.any()
    # the defaults: the lifted cube's top face (the cube's pixels nearest the camera) is lit, the table under it is not
    img, dep, lb, mask = S.render(scene["tri"], scene["body"], scene["rgb"], lab, cast, fr, cam, W, H, sh, target=ee)
    top_depth = cam["pos"][2] - (float(S.LIFTED[8]) + CUBE_A / 2)
    top = (lb == 9) & (np.abs(dep - top_depth) < 1e-4)
    assert top.sum() >= 4 and not mask[top].any()
    assert (mask & (lb == 0)).sum() > 0
    half = S.shadow_dict(R.make_shadow(scene, bias=0.0))
    assert half["bias"] == 0.0 and sh["bias"] == pytest.approx(0.01)


def test_default_bounds_cover_the_workspace(scene):
    c, r = R.shadow_bounds(scene)
    tri = np.asarray(scene["tri"], np.float64)
    mat, _ = R.material_ids(scene)
    binv = tri[mat == R.MATERIALS.index("bin")].reshape(-1, 3)
    assert np.all(np.linalg.norm(binv - c, axis=1) <= r)
    for x in (-0.25, -0.15):
        for y in (0.3, 0.6):
            assert np.linalg.norm(np.array([x, y, 0.05]) - c) + np.sqrt(3) * 0.02 <= r
    assert 0.4 < r < 0.8


# ------------------------------------------------------------------------------------------- the float32 floor
def test_float32_floor(scene, model, oracle64, oracle32):
    """The share of pixels (among those whose label agrees) at which the float32 restatement's mask, on oracle32's
    frames, differs from the float64 one, per image of render_aux_ref.SCENE_SETS and of the lifted-cube state: the
    worst is what render_shadow_ref.MASK_F32_FLOOR records."""
    lab, _ = R.segment_labels(scene)
    cast = R.shadow_casters(scene)
    sh = S.shadow_dict(R.make_shadow(scene))
    sets = [(c, w, h, q, [im[1:] for im in i64], [im[1:] for im in i32]) for (c, w, h, q, i64), (_, _, _, _, i32) in
            zip(A.reference(model, oracle64, 64), A.reference(model, oracle32, 32))]
    worst = 0.0
    for W, H in ((64, 48), (96, 72)):
        cam = render_ref.camera_dict(R.make_camera(scene, "top"))
        pair = []
        for o, dt in ((oracle64, np.float64), (oracle32, np.float32)):
            fr, ee = A.frames_of(o, model, S.LIFTED.astype(np.float64))
            pair.append([A.render(scene["tri"], scene["body"], scene["rgb"], lab, fr, cam, W, H, dtype=dt)[1:]])
        sets.append(("top", W, H, S.LIFTED[None], pair[0], pair[1]))
    for name, W, H, qpos, i64, i32 in sets:
        cam = render_ref.camera_dict(R.make_camera(scene, name))
        for k, q in enumerate(qpos):
            masks = []
            for o, dt, (dep, lb) in ((oracle64, np.float64, i64[k]), (oracle32, np.float32, i32[k])):
                fr, ee = A.frames_of(o, model, q.astype(np.float64))
                f = S.light_frame(cam["light_dir"][sh["light"]], np.dtype(dt).type)
                smap = S.shadow_map(scene["tri"], scene["body"], cast, fr, f, sh["center"], sh["radius"],
                                    sh["map_size"], dt)
                masks.append(S.shadow_mask(dep, lb, cam, W, H, smap, f, sh["center"], sh["radius"], sh["bias"],
                                           target=ee, dtype=dt))
            same = i64[k][1] == i32[k][1]
            diff = int(((masks[0] != masks[1]) & same).sum())
            print(f"{name} {W}x{H} env {k}: shadowed {int(masks[0].sum())} ({masks[0].mean():.4f}), float32 differs at "
                  f"{diff} pixels ({diff / (W * H):.2e}), labels differ at {int((~same).sum())}")
            worst = max(worst, diff / (W * H))
    print(f"worst share {worst:.3e}; recorded {S.MASK_F32_FLOOR:.3e}")
    assert worst <= S.MASK_F32_FLOOR


# ------------------------------------------------------------------------------------------------------ bindings
def test_bindings_and_refusals_without_a_device(scene):
    for sym in ("so100_shadow_bytes", "so100_render_casters", "so100_render_shadow"):
        assert sym in _native.EXPORTED_SYMBOLS
    lib = _native.load()
    assert _native.ABI_VERSION >= 23 and lib.so100_abi_version() == _native.ABI_VERSION
    assert lib.so100_shadow_bytes() == ctypes.sizeof(_native.SO100Shadow) == 40
    s = R.make_shadow(scene)
    assert s.size == 40 and s.light == 1 and s.map_size == 64 and s.shadow_out is None
    # the library's own refusals that come before the env is looked at (no device work)
    cams = _native.SO100Cams([R.make_camera(scene, "top")], [0])
    out = _native.SO100ImageOut(hwc=ctypes.c_void_p(16))
    aux = _native.SO100AuxOut()

    def call(sh, width=64):
        return lib.so100_render_shadow(None, None, None, ctypes.byref(cams), None, width, 48, ctypes.byref(out),
                                       ctypes.byref(aux), None if sh is None else ctypes.byref(sh), None)
    assert call(None) != 0 and b"NULL shadow" in lib.so100_last_error()
    bad = R.make_shadow(scene)
    bad.size = 36
    assert call(bad) != 0 and b"so100_shadow" in lib.so100_last_error()
    assert call(R.make_shadow(scene)) != 0 and b"NULL env" in lib.so100_last_error()
    assert lib.so100_render_casters(None, None, 0) != 0
    # the Python layer's ValueErrors
    for kw in (dict(map_size=128), dict(map_size=0), dict(map_size=36), dict(light=3), dict(light=-2),
               dict(radius=0.0), dict(radius=float("inf")), dict(bias=-0.1), dict(bias=float("nan")),
               dict(center=(0.0, float("nan"), 0.0)), dict(center=(0.0, 1.0))):
        with pytest.raises(ValueError):
            R.make_shadow(scene, **kw)
    with pytest.raises(ValueError):
        R.shadow_options(scene, {"texels": 64})
    with pytest.raises(ValueError):
        R.shadow_options(scene, "yes")
    assert R.shadow_options(scene, False) is None and R.shadow_options(scene, None) is None
    assert R.shadow_options(scene, {"map_size": 32, "bias": 0.02}).map_size == 32
    with pytest.raises(ValueError):
        SO100VecEnv(2, shadows=True)                               # state observations: no pixels
    with pytest.raises(ValueError):
        SO100VecEnv(2, obs_type="so100_pixels_agent_pos", shadows={"map_size": 100})
    with pytest.raises(ValueError):
        SO100SB3VecEnv(2, shadows=True)
