"""Depth and segmentation images (ABI 21: so100_render_aux, so100_aux_out, so100_render_labels) without a device: the
exported symbols, the ctypes mirror of so100_aux_out against the callee's own size and the header, the argument checks
that come before any device call, the segmentation classes of the committed asset, the options' argument checks, and
what the reference alone says of the GPU tests' bars (tests/render_aux_ref.py, float32 against float64 arithmetic on
the hand-set scenes of tests/test_gpu_render_aux.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_aux_ref as A
import render_ref
from gym_so100 import _native
from gym_so100 import render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("so100_aux_out_bytes", "so100_render_labels", "so100_render_aux")


def call(lib, out, aux, views=None):
    cam = _native.SO100Camera()
    rc = lib.so100_render_aux(None, None, None, ctypes.byref(cam), views, 8, 8,
                              None if out is None else ctypes.byref(out), None if aux is None else ctypes.byref(aux),
                              None)
    return rc, lib.so100_last_error()


def test_symbols_and_abi():
    lib = _native.load()
    assert _native.ABI_VERSION >= 21 and lib.so100_abi_version() == _native.ABI_VERSION
    for name in NEW:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_aux_out_mirror_follows_the_header_and_the_callee():
    lib = _native.load()
    assert lib.so100_aux_out_bytes() == ctypes.sizeof(_native.SO100AuxOut)
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    body = re.search(r"typedef struct so100_aux_out \{(.*?)\} so100_aux_out;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decl == ["uint32_t size", "float* depth", "uint8_t* label"]
    assert [f[0] for f in _native.SO100AuxOut._fields_] == [d.split()[-1] for d in decl]


def test_struct_sizes_are_checked_first():
    """Either struct's size is compared with the callee's sizeof before anything else: the mirrors' sizes pass (the call
    goes on to refuse the NULL env), any other size is refused in so100_image_out's wording."""
    lib = _native.load()
    out, aux = _native.SO100ImageOut(hwc=1 << 20), _native.SO100AuxOut(depth=1 << 20, label=1 << 20)
    assert aux.size == ctypes.sizeof(_native.SO100AuxOut)
    rc, err = call(lib, out, aux)
    assert rc != 0 and b"so100_render_aux: NULL env" in err and b"size" not in err
    for wrong in (0, aux.size - 8, aux.size + 8):
        aux.size = wrong
        rc, err = call(lib, out, aux)
        assert rc != 0 and b"so100_aux_out.size %d, expected %d" % (wrong, ctypes.sizeof(aux)) in err, err
    aux.size = ctypes.sizeof(aux)
    for wrong in (0, out.size + 8):
        out.size = wrong
        rc, err = call(lib, out, aux)
        assert rc != 0 and b"so100_image_out.size %d, expected %d" % (wrong, ctypes.sizeof(out)) in err, err


def test_null_env_no_sink_and_missing_labels():
    lib = _native.load()
    # out may be NULL when aux has a sink, and aux's sinks may be NULL when out has one: both reach the env check
    for out, aux in ((None, _native.SO100AuxOut(depth=1 << 20)), (None, _native.SO100AuxOut(label=1 << 20)),
                     (_native.SO100ImageOut(chw=1 << 20), _native.SO100AuxOut())):
        rc, err = call(lib, out, aux)
        assert rc != 0 and b"so100_render_aux: NULL env" in err, err
    # no sink at all across both structs
    for out, aux in ((_native.SO100ImageOut(), _native.SO100AuxOut()), (None, _native.SO100AuxOut()), (None, None),
                     (_native.SO100ImageOut(), None)):
        rc, err = call(lib, out, aux)
        assert rc != 0 and b"so100_render_aux: no sink (hwc, chw, flat, depth and label are all NULL)" in err, err
    # labels: the upload's own checks; the refusal of a label sink without uploaded labels needs an env and is reached
    # in tests/test_gpu_render_aux.py, here only its text is looked up in the library
    lab = (ctypes.c_uint8 * 4)()
    assert lib.so100_render_labels(None, lab, 4) != 0 and b"so100_render_labels: bad arguments" in lib.so100_last_error()
    assert lib.so100_render_labels(None, None, 4) != 0 and b"so100_render_labels" in lib.so100_last_error()
    blob = open(_native.LIB_PATH, "rb").read()
    assert b"no labels (so100_render_labels)" in blob and b"so100_render_labels: label 255 is the background's" in blob


def test_segment_labels_of_the_committed_asset():
    scene = R.load_scene()
    lab, names = R.segment_labels(scene)
    assert lab.dtype == np.uint8 and lab.shape == scene["body"].shape and R.SEG_BACKGROUND == 255
    assert np.bincount(lab).tolist() == [12, 60, 604, 612, 566, 596, 638, 601, 320, 12]
    assert tuple(names) == ("table", "bin", "Base", "link1", "link2", "link3", "link4", "link5", "link6", "cube")
    body, (mat, _) = scene["body"], R.material_ids(scene)
    assert np.all(body[lab <= 1] == 0) and np.all(mat[lab == 0] == 0) and np.all(mat[lab == 1] == 1)
    assert np.all(body[lab >= 2] == lab[lab >= 2] - 1)
    odd = dict(scene, body=scene["body"].copy())
    odd["body"][100] = 9                                 # no such body: fits no class
    with pytest.raises(ValueError, match="fit no segmentation class"):
        R.segment_labels(odd)


def test_depth_and_segmentation_need_pixel_observations():
    """Refused at argument level: before the library is loaded or a device touched."""
    from gym_so100 import SO100VecEnv
    for kw in (dict(depth=True), dict(segmentation=True)):
        with pytest.raises(ValueError, match="so100_pixels_agent_pos"):
            SO100VecEnv(4, obs_type="so100_state", device="cuda:99", **kw)


def test_float64_helper_draws_render_refs_colours(model, oracle64):
    """The new key leaves the colour image alone: the float64 helper's RGB is render_ref.render's, bit for bit, on
    every scene."""
    scene = R.load_scene()
    for name, w, h, qpos, imgs in A.reference(model, oracle64, 64):
        cam = render_ref.camera_dict(R.make_camera(scene, name))
        for q, (rgb, dep, lab) in zip(qpos, imgs):
            fr, ee = A.frames_of(oracle64, model, q.astype(np.float64))
            old = render_ref.render(scene["tri"], scene["body"], scene["rgb"], fr, cam, w, h, target=ee)
            assert np.array_equal(rgb, old), (name, w, h)


def test_reference_alone_is_inside_the_gpu_bars(model, oracle64, oracle32):
    """What the number format alone costs (float32 numpy on oracle32's frames against float64 on oracle64's), which the
    GPU tests' bars come from: label and colour shares inside the 1 % silhouette cap, every class in some 96x72 `top`
    scene, background depth 0, foreground depth inside the scene, and the depth error on agreeing foreground pixels
    within a quarter of DEPTH_REL_BAR (= 4 x the largest per-set maximum)."""
    r64, r32 = A.reference(model, oracle64, 64), A.reference(model, oracle32, 32)
    worst = 0.0
    seen = []
    for (name, w, h, _, i64), (_, _, _, _, i32) in zip(r64, r32):
        mx = 0.0
        for (rgb_a, dep_a, lab_a), (rgb_b, dep_b, lab_b) in zip(i64, i32):
            assert (lab_a != lab_b).mean() < 0.01 and np.any(rgb_a != rgb_b, axis=-1).mean() < 0.01
            bg = lab_a == A.BACKGROUND
            assert np.all(dep_a[bg] == 0.0) and dep_a.dtype == np.float32
            assert 0.3 < dep_a[~bg].min() and dep_a[~bg].max() < 1.1
            same = (lab_a == lab_b) & ~bg
            rel = np.abs(dep_b[same].astype(np.float64) - dep_a[same]) / dep_a[same]
            mx = max(mx, float(rel.max()))
            if (name, w, h) == ("top", 96, 72):
                seen.append(set(np.unique(lab_a).tolist()))
        print(f"{name} {w}x{h}: float32 helper's largest relative depth error {mx:.3g}")
        worst = max(worst, mx)
    assert worst <= A.DEPTH_REL_BAR / 4, worst
    assert worst >= A.DEPTH_REL_BAR / 8, worst        # the constant is 4 x this maximum, not a looser round number
    assert sum(s == set(range(10)) | {A.BACKGROUND} for s in seen) >= 1, seen
