"""Per-env views (ABI 20: so100_view, so100_render_views, so100_render_materials, so100_views_sample) without a device:
the exported symbols, the ctypes mirrors against the callee's own sizes and the header, the argument checks that come
before any device call, the material ids of the committed asset, and the visual option's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from gym_so100 import _native
from gym_so100 import render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("so100_view_bytes", "so100_render_materials", "so100_render_views", "so100_views_sample")


def test_symbols_and_abi():
    lib = _native.load()
    assert _native.ABI_VERSION >= 20 and lib.so100_abi_version() == _native.ABI_VERSION
    for name in NEW:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_view_mirror_has_the_callee_size_and_the_header_layout():
    lib = _native.load()
    assert lib.so100_view_bytes() == ctypes.sizeof(_native.SO100View) == 160
    assert _native.VIEW_WORDS == 40 and _native.SO100_NMATERIAL == len(R.MATERIALS) == 5
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    for struct, mirror in (("so100_view", _native.SO100View), ("so100_view_dr", _native.SO100ViewDR)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"\[.*", "", n.strip()) for d in body.split(";") if d.strip()
                 for n in d.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in mirror._fields_], struct
    # dword offsets the device records are decoded by (tests/views_ref.py)
    V = _native.SO100View
    assert [getattr(V, f).offset // 4 for f in ("pos", "mat", "fovy", "head_ambient", "light_diffuse", "light_dir",
                                                 "rgb", "reserved")] == [0, 3, 12, 13, 15, 19, 31, 36]


def test_view_dr_size_is_checked_first():
    lib = _native.load()
    dr = _native.SO100ViewDR(seed=1)
    assert dr.size == ctypes.sizeof(_native.SO100ViewDR)
    cam = _native.SO100Camera()
    rgb = (ctypes.c_uint32 * 5)()
    rc = lib.so100_views_sample(None, ctypes.byref(dr), ctypes.byref(cam), rgb, None, None, 1 << 20, None)
    assert rc != 0 and b"so100_views_sample: NULL env" in lib.so100_last_error()
    for wrong in (0, dr.size - 4, dr.size + 8):
        dr.size = wrong
        rc = lib.so100_views_sample(None, ctypes.byref(dr), ctypes.byref(cam), rgb, None, None, 1 << 20, None)
        err = lib.so100_last_error()
        assert rc != 0 and b"so100_view_dr.size %d, expected %d" % (wrong, ctypes.sizeof(dr)) in err, err


def test_null_arguments_are_rejected():
    lib = _native.load()
    cam = _native.SO100Camera()
    out = _native.SO100ImageOut(hwc=1 << 20)
    err = lib.so100_last_error
    assert lib.so100_views_sample(None, None, ctypes.byref(cam), None, None, None, None, None) != 0
    assert b"so100_views_sample: NULL dr" in err()
    assert lib.so100_render_materials(None, None, 4) != 0 and b"so100_render_materials" in err()
    ids = (ctypes.c_uint8 * 4)()
    assert lib.so100_render_materials(None, ids, 4) != 0 and b"so100_render_materials" in err()
    assert lib.so100_render_views(None, None, None, ctypes.byref(cam), 1 << 20, 8, 8, None, None) != 0
    assert b"so100_render_views: NULL out" in err()
    assert lib.so100_render_views(None, None, None, ctypes.byref(cam), 1 << 20, 8, 8, ctypes.byref(out), None) != 0
    assert b"so100_render_views: NULL env" in err()
    out.size -= 8
    assert lib.so100_render_views(None, None, None, ctypes.byref(cam), 1 << 20, 8, 8, ctypes.byref(out), None) != 0
    assert b"so100_image_out.size" in err()


def test_material_ids_of_the_committed_asset():
    scene = R.load_scene()
    ids, base = R.material_ids(scene)
    assert ids.dtype == np.uint8 and ids.shape == scene["body"].shape
    assert np.bincount(ids, minlength=5).tolist() == [12, 60, 2160, 1777, 12]
    for k in range(5):                                   # one base colour per material, and it is the asset's
        assert np.all(scene["rgb"][ids == k] == base[k]), R.MATERIALS[k]
    np.testing.assert_array_equal(base, np.array([[.2, .2, .2], [.5, .5, .5], [1, 1, 1], [.1, .1, .1], [1, 0, 0]],
                                                 np.float32))
    assert [hex(x) for x in R.pack_rgb8(base)] == ["0x333333", "0x808080", "0xffffff", "0x1a1a1a", "0xff"]
    odd = dict(scene, rgb=scene["rgb"].copy())
    odd["rgb"][100] = [0.3, 0.3, 0.3]                    # fits no material
    with pytest.raises(ValueError, match="fit no material"):
        R.material_ids(odd)
    odd = dict(scene, rgb=scene["rgb"].copy())
    t = int(np.nonzero(ids == 4)[0][0])
    odd["rgb"][t] = [0.0, 1.0, 0.0]                      # a second cube colour
    with pytest.raises(ValueError, match="base colours"):
        R.material_ids(odd)


def test_view_ranges_from_the_dict():
    dr = R.view_ranges(dict(camera_pos=0.03, camera_rot_deg=3.0, fovy=(0.9, 1.1), lights=(0.6, 1.4),
                            colors={"cube": (0.5, 1.0)}), seed=(1 << 64) + 5)
    assert dr.seed == 5 and dr.size == ctypes.sizeof(dr)
    assert dr.cam_pos == np.float32(0.03) and dr.cam_rot == np.float32(np.radians(3.0)) and dr.light_rot == 0.0
    assert list(dr.fovy) == [np.float32(0.9), np.float32(1.1)] and list(dr.ambient) == [1.0, 1.0]
    assert all(list(p) == [np.float32(0.6), np.float32(1.4)] for p in dr.light)
    assert [list(p) for p in dr.color] == [[1.0, 1.0]] * 4 + [[0.5, 1.0]]
    for bad in (dict(fov=(1, 1)), dict(fovy=(1.1, 0.9)), dict(camera_pos=-1.0), dict(colors={"floor": (1, 1)})):
        with pytest.raises(ValueError):
            R.view_ranges(bad, 0)


def test_visual_randomisation_needs_pixel_observations():
    """Refused at argument level: before the library is loaded or a device touched (ValueError, not the library's or
    the device's error)."""
    from gym_so100 import SO100VecEnv
    with pytest.raises(ValueError, match="so100_pixels_agent_pos"):
        SO100VecEnv(4, obs_type="so100_state", domain_randomization={"visual": {"fovy": (0.9, 1.1)}},
                    device="cuda:99")
    with pytest.raises(ValueError, match="unknown keys"):
        SO100VecEnv(4, obs_type="so100_pixels_agent_pos", domain_randomization={"visual": {"fov": (0.9, 1.1)}},
                    device="cuda:99")
