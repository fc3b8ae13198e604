"""Multisample anti-aliasing (ABI 24: so100_msaa, so100_render_msaa, so100_msaa_bytes) without a device: the numpy
restatement (tests/render_msaa_ref.py) against render_aux_ref at one sample, against the box mean of its own image at
twice the size under the ordered grid, in float32 against float64, against a known answer, and the bindings, refusals
and option checks that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_aux_ref as A
import render_msaa_ref as M
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R
from gym_so100.sb3 import SO100SB3VecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARE_CAP = 0.01                     # differing pixels per image, the cap of the other render tests


def oracle_of(bits, oracle64, oracle32):
    return oracle64 if bits == 64 else oracle32


def test_default_patterns_are_the_issues_and_exact_in_float32():
    assert R.AA_PATTERNS[4] == M.ROTATED4 and R.AA_PATTERNS[2] == M.DIAG2 and R.AA_PATTERNS[1] == M.CENTRE1
    for pat in R.AA_PATTERNS.values():
        a = np.asarray(pat, np.float64)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.all(np.abs(a) < 0.5)


@pytest.mark.parametrize("bits", [64, 32])
def test_one_centre_sample_is_render_aux_ref(model, oracle64, oracle32, bits):
    o = oracle_of(bits, oracle64, oracle32)
    ref = A.reference(model, o, bits)[:3]
    got = M.reference(model, o, bits, M.CENTRE1)
    assert [(s[0], s[1], s[2], len(s[4])) for s in got] == [("top", 96, 72, 6), ("front_close", 64, 48, 3),
                                                            ("angle", 37, 29, 2)]
    for (name, w, h, _, imgs), (_, _, _, _, aux) in zip(got, ref):
        for k, img in enumerate(imgs):
            assert np.array_equal(img, aux[k][0]), (name, k)


@pytest.mark.parametrize("bits", [64, 32])
def test_ordered_grid_is_the_box_mean_of_the_image_at_twice_the_size(model, oracle64, oracle32, bits):
    """Sample (x + 0.5 -+ 0.25) of the W x H image is the centre of a pixel of the 2W x 2H image, and scaling the screen
    coordinates by two is exact: every sample key is the larger image's pixel key."""
    o = oracle_of(bits, oracle64, oracle32)
    got = M.reference(model, o, bits, M.ORDERED4)
    big = M.reference(model, o, bits, M.CENTRE1, scale=2)
    for (name, w, h, _, imgs), (_, _, _, _, hi) in zip(got, big):
        for k, img in enumerate(imgs):
            diff = int(np.any(img != M.box_mean(hi[k]), axis=-1).sum())
            print(f"float{bits} {name} {w}x{h} env {k}: {diff} pixels differ from the box mean")
            assert diff == 0, (name, k)


@pytest.mark.parametrize("pattern", ["rotated4", "ordered4"])
def test_float32_against_float64(model, oracle64, oracle32, pattern):
    off = M.ROTATED4 if pattern == "rotated4" else M.ORDERED4
    r64 = M.reference(model, oracle64, 64, off)
    r32 = M.reference(model, oracle32, 32, off)
    worst = 0.0
    for (name, w, h, _, a), (_, _, _, _, b) in zip(r64, r32):
        for k in range(len(a)):
            share = float(np.any(a[k] != b[k], axis=-1).mean())
            print(f"{pattern} {name} {w}x{h} env {k}: float32 differs in {share:.4f} of the pixels")
            worst = max(worst, share)
    assert worst <= SHARE_CAP


def test_four_samples_change_the_image(model, oracle64):
    one = M.reference(model, oracle64, 64, M.CENTRE1)
    four = M.reference(model, oracle64, 64, M.ROTATED4)
    for (name, w, h, _, a), (_, _, _, _, b) in zip(one, four):
        for k in range(len(a)):
            share = float(np.any(a[k] != b[k], axis=-1).mean())
            print(f"{name} {w}x{h} env {k}: 4 samples differ from 1 in {share:.4f} of the pixels")
            assert share > 0.02, (name, k)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [5, 11])
def test_vertical_edge_at_a_quarter_pixel(dtype, k):
    """One triangle whose right edge is the vertical x = k + 0.25 and whose other edges lie far outside the image.  The
    ordered grid's samples of column k are at x = k + 0.25 (on the edge: inclusive, covered) and k + 0.75 (outside): two
    of four samples, half the colour rounded half up.  Columns left of k are full, columns right of it empty."""
    dt = np.dtype(dtype).type
    W, H = 16, 8
    sx = np.array([[k + 0.25, k + 0.25, -300.0]], dt)
    sy = np.array([[-50.0, 60.0, 5.0]], dt)
    iz = np.ones((1, 3), dt)
    rgb = (201, 100, 51)
    col = np.array([rgb[0] | (rgb[1] << 8) | (rgb[2] << 16)], np.uint32)
    smp = M.raster(sx, sy, iz, np.array([True]), col, W, H, M.ORDERED4, dt)
    img = M.resolve(smp)
    assert np.all(img[:, :k] == np.array(rgb, np.uint8))
    assert np.all(img[:, k] == np.array([(c * 2 + 2) // 4 for c in rgb], np.uint8))      # 101, 50, 26
    assert np.all(img[:, k + 1:] == 0)
    # one centre sample: column k's centre k + 0.5 is outside
    one = M.resolve(M.raster(sx, sy, iz, np.array([True]), col, W, H, M.CENTRE1, dt))
    assert np.all(one[:, :k] == np.array(rgb, np.uint8)) and np.all(one[:, k:] == 0)


# ------------------------------------------------------------------------------------------------------ bindings
def test_bindings_and_the_struct_mirror():
    for sym in ("so100_msaa_bytes", "so100_render_msaa"):
        assert sym in _native.EXPORTED_SYMBOLS
    lib = _native.load()
    assert _native.ABI_VERSION >= 24 and lib.so100_abi_version() == _native.ABI_VERSION
    assert lib.so100_msaa_bytes() == ctypes.sizeof(_native.SO100Msaa) == 40
    assert _native.SO100_MSAA_MAX == 4
    hdr = open(os.path.join(ROOT, "include", "so100.h")).read()
    assert re.search(r"#define SO100_MSAA_MAX 4\b", hdr)
    body = re.search(r"typedef struct so100_msaa \{(.*?)\} so100_msaa;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+)", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in _native.SO100Msaa._fields_] == ["size", "samples", "offset"]
    assert _native.SO100Msaa.samples.offset == 4 and _native.SO100Msaa.offset.offset == 8
    a = R.make_antialias()
    assert a.size == 40 and a.samples == 4
    assert [tuple(p) for p in a.offset] == list(M.ROTATED4)


def test_argument_level_refusals_come_before_the_env():
    lib = _native.load()
    scene = R.load_scene()
    cams = _native.SO100Cams([R.make_camera(scene, "top")], [0])
    hwc = _native.SO100ImageOut(hwc=ctypes.c_void_p(16))

    def call(ms, width=64, height=48, out=hwc, cams=cams):
        rc = lib.so100_render_msaa(None, None, None, None if cams is None else ctypes.byref(cams), None, width, height,
                                   None if out is None else ctypes.byref(out),
                                   None if ms is None else ctypes.byref(ms), None)
        return rc, lib.so100_last_error()

    def refused(text, *a, **kw):
        rc, err = call(*a, **kw)
        assert rc != 0 and text in err, (text, err)
    refused(b"NULL msaa", None)
    bad = R.make_antialias()
    bad.size = 36
    refused(b"so100_msaa", bad)
    # a wrong size is found before anything else is looked at, a wrong so100_cams after it
    refused(b"so100_msaa", bad, cams=None)
    for s in (0, 3, 5, 8, -1):
        refused(b"samples %d, expected 1, 2 or 4" % s, _native.SO100Msaa(s, M.ROTATED4))
    for v in (0.5, -0.5, 0.75, float("nan"), float("inf")):
        refused(b"offset[1][0] must be finite and inside (-0.5, 0.5)", _native.SO100Msaa(2, ((0.0, 0.0), (v, 0.0))))
        refused(b"offset[0][1] must be finite and inside (-0.5, 0.5)", _native.SO100Msaa(1, ((0.0, v),)))
    # offsets past `samples` are not read
    refused(b"NULL env", _native.SO100Msaa(2, ((0.0, 0.0), (0.25, 0.25), (9.0, 9.0), (float("nan"), 0.0))))
    refused(b"width 1025 * samples 4 > 4096", R.make_antialias(4), width=1025, height=2)
    refused(b"NULL env", R.make_antialias(4), width=1024, height=2)
    refused(b"width 2049 * samples 2 > 4096", R.make_antialias(2), width=2049, height=2)
    refused(b"NULL env", R.make_antialias(1), width=4096, height=2)
    refused(b"NULL out", R.make_antialias(), out=None)
    refused(b"no colour sink", R.make_antialias(), out=_native.SO100ImageOut())
    # what so100_render_cams refuses for the same arguments
    refused(b"NULL cams", R.make_antialias(), cams=None)
    refused(b"ncam 0", R.make_antialias(), cams=_native.SO100Cams([], []))
    refused(b"frame_body[0] 9", R.make_antialias(), cams=_native.SO100Cams([R.make_camera(scene, "top")], [9]))
    refused(b"bad image size", R.make_antialias(), width=0)
    refused(b"bad image size", R.make_antialias(1), width=4097, height=1)
    badout = _native.SO100ImageOut(hwc=ctypes.c_void_p(16))
    badout.size = 8
    refused(b"so100_image_out", R.make_antialias(), out=badout)
    refused(b"flat_pitch", R.make_antialias(), out=_native.SO100ImageOut(flat=ctypes.c_void_p(16), flat_pitch=10))
    refused(b"NULL env", R.make_antialias())
    # the cams launch refuses as before
    aux = _native.SO100AuxOut()
    assert lib.so100_render_cams(None, None, None, ctypes.byref(cams), None, 64, 48, ctypes.byref(hwc),
                                 ctypes.byref(aux), None) != 0 and b"so100_render_cams: NULL env" in lib.so100_last_error()


def test_antialias_options():
    assert R.antialias_options(False) is None and R.antialias_options(None) is None
    a = R.antialias_options(True)
    assert a.samples == 4 and [tuple(p) for p in a.offset] == list(M.ROTATED4)
    a = R.antialias_options(2)
    assert a.samples == 2 and [tuple(p) for p in a.offset][:2] == list(M.DIAG2)
    assert R.antialias_options(4).samples == 4
    a = R.antialias_options({"samples": 4, "offsets": M.ORDERED4})
    assert [tuple(p) for p in a.offset] == list(M.ORDERED4)
    assert R.antialias_options({"samples": 1}).samples == 1
    assert R.antialias_options({}).samples == 4
    for bad in (3, 8, 1, 0, "yes", 4.0, (4,), {"sample": 4}, {"samples": 3}, {"samples": 2, "offsets": M.ORDERED4},
                {"samples": 2, "offsets": ((0.0, 0.0), (0.5, 0.0))},
                {"samples": 2, "offsets": ((0.0, 0.0), (float("nan"), 0.0))}, {"samples": True}):
        with pytest.raises(ValueError):
            R.antialias_options(bad)
    with pytest.raises(ValueError):
        R.make_antialias(4, offsets=((0.0, 0.0),) * 3)


class _NoDevice:
    """A venv whose every attribute use is a device use: the renderers must refuse before touching it"""

    def __getattr__(self, name):
        raise AssertionError(f"device use: venv.{name}")


def test_value_errors_without_a_device():
    for cls in (R.CameraRenderer, R.MultiCameraRenderer):
        with pytest.raises(ValueError, match="shadows"):
            cls(_NoDevice(), 64, 48, antialias=True, shadows=True)
        with pytest.raises(ValueError):
            cls(_NoDevice(), 64, 48, antialias=3)
        with pytest.raises(ValueError):
            cls(_NoDevice(), 64, 48, antialias={"samples": 4, "offsets": M.DIAG2})
        with pytest.raises(ValueError, match="4096"):
            cls(_NoDevice(), 1025, 2, antialias=4)
    with pytest.raises(ValueError, match="antialias"):
        SO100VecEnv(2, antialias=True)                              # state observations: no pixels
    with pytest.raises(ValueError):
        SO100VecEnv(2, obs_type="so100_pixels_agent_pos", antialias=3)
    with pytest.raises(ValueError, match="shadows"):
        SO100VecEnv(2, obs_type="so100_pixels_agent_pos", antialias=True, shadows=True)
    with pytest.raises(ValueError, match="4096"):
        SO100VecEnv(2, obs_type="so100_pixels_agent_pos", antialias=True, observation_width=2048,
                    observation_height=2)
    with pytest.raises(ValueError, match="antialias"):
        SO100SB3VecEnv(2, antialias=True)
    with pytest.raises(ValueError):
        SO100SB3VecEnv(2, obs_type="so100_pixels_agent_pos", antialias="yes")
