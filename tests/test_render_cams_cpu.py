"""Several cameras in one launch (ABI 22: so100_cams, so100_render_cams, so100_cams_bytes) without a device: the exported
symbols, the ctypes mirror of so100_cams against the callee's own size and the header, every refusal that comes before
any device call, the ``cameras=`` argument checks of the env and the SB3 adapter, and what the reference alone says of
the GPU test's bars for the two mounted cameras (tests/render_cams_ref.py: float32 numpy on oracle32's frames against
float64 on oracle64's, at 64x48 on the 12 states of render_aux_ref.scene_states())."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_aux_ref as A
import render_cams_ref as C
from gym_so100 import _native
from gym_so100 import render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("so100_cams_bytes", "so100_render_cams")
BIG = 1 << 20                            # a non-NULL sink address: never dereferenced, every call here is refused


def cams_of(n=1, frame_body=()):
    cam = _native.SO100Camera()
    cam.fovy, cam.nlight = 45.0, 0
    return _native.SO100Cams([cam] * n, frame_body)


def call(lib, cams, out, aux, w=8, h=8, views=None):
    rc = lib.so100_render_cams(None, None, None, None if cams is None else ctypes.byref(cams), views, w, h,
                               None if out is None else ctypes.byref(out), None if aux is None else ctypes.byref(aux),
                               None)
    return rc, lib.so100_last_error()


def test_symbols_and_abi():
    lib = _native.load()
    assert _native.ABI_VERSION >= 22 and lib.so100_abi_version() == _native.ABI_VERSION
    for name in NEW:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert R.CAMERAS == ("top", "angle", "left_pillar", "right_pillar", "front_close")
    assert R.MOUNTED_CAMERAS == ("left_wrist",)


def test_cams_mirror_follows_the_header_and_the_callee():
    lib = _native.load()
    assert lib.so100_cams_bytes() == ctypes.sizeof(_native.SO100Cams)
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    assert int(re.search(r"#define SO100_MAX_CAMS (\d+)", src).group(1)) == _native.SO100_MAX_CAMS == 4
    body = re.search(r"typedef struct so100_cams \{(.*?)\} so100_cams;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decl == ["uint32_t size", "int32_t ncam", "so100_camera cam[SO100_MAX_CAMS]",
                    "int32_t frame_body[SO100_MAX_CAMS]"]
    assert [f[0] for f in _native.SO100Cams._fields_] == [d.split()[-1].split("[")[0] for d in decl]
    c = cams_of(3, (0, 6, 8))
    assert c.size == ctypes.sizeof(c) and c.ncam == 3 and list(c.frame_body) == [0, 6, 8, 0]
    assert c.cam[2].fovy == 45.0 and c.cam[3].fovy == 0.0


def test_struct_sizes_are_checked_first():
    """Each of the three structs' sizes is compared with the callee's sizeof before anything else of it is read: the
    mirrors' sizes pass (the call goes on to refuse the NULL env), any other size is refused even when everything else
    is wrong too."""
    lib = _native.load()
    out, aux = _native.SO100ImageOut(hwc=BIG), _native.SO100AuxOut(depth=BIG, label=BIG)
    rc, err = call(lib, cams_of(2), out, aux)
    assert rc != 0 and b"so100_render_cams: NULL env" in err and b"size" not in err
    for wrong in (0, ctypes.sizeof(_native.SO100Cams) - 4, ctypes.sizeof(_native.SO100Cams) + 136):
        cams = cams_of(9, (77,))                     # ncam and frame_body are bad too: the size is what is reported
        cams.size = wrong
        rc, err = call(lib, cams, out, aux)
        assert rc != 0 and b"so100_cams.size %d, expected %d" % (wrong, ctypes.sizeof(cams)) in err, err
    for wrong in (0, aux.size + 8):
        bad = _native.SO100AuxOut(depth=BIG)
        bad.size = wrong
        rc, err = call(lib, cams_of(9), out, bad)
        assert rc != 0 and b"so100_aux_out.size %d, expected %d" % (wrong, ctypes.sizeof(aux)) in err, err
    for wrong in (0, out.size + 8):
        bad = _native.SO100ImageOut(hwc=BIG)
        bad.size = wrong
        rc, err = call(lib, cams_of(9), bad, aux)
        assert rc != 0 and b"so100_image_out.size %d, expected %d" % (wrong, ctypes.sizeof(out)) in err, err


def test_argument_refusals():
    lib = _native.load()
    out, aux = _native.SO100ImageOut(hwc=BIG), _native.SO100AuxOut(depth=BIG)
    rc, err = call(lib, None, out, aux)
    assert rc != 0 and b"so100_render_cams: NULL cams" in err
    for n in (0, -1, 5):
        cams = cams_of(1)
        cams.ncam = n
        rc, err = call(lib, cams, out, aux)
        assert rc != 0 and b"so100_render_cams: ncam %d, expected 1..4" % n in err, err
    for fb in (-1, 9, 100):
        rc, err = call(lib, cams_of(3, (0, 8, fb)), out, aux)
        assert rc != 0 and b"so100_render_cams: frame_body[2] %d, expected 0 (world) or 1..8" % fb in err, err
    # a frame_body beyond ncam is not looked at; 0..8 pass (on to the NULL env)
    for fbs in ((0, 0, 77), (8, 1, 0)):
        rc, err = call(lib, cams_of(2, fbs), out, aux)
        assert rc != 0 and b"so100_render_cams: NULL env" in err, err
    # flat_pitch counts every camera's 3HW floats
    for k, pitch, ok in ((1, 192, True), (2, 383, False), (2, 384, True), (4, 767, False), (4, 768, True)):
        rc, err = call(lib, cams_of(k), _native.SO100ImageOut(flat=BIG, flat_pitch=pitch), None)
        assert rc != 0 and (b"NULL env" if ok else b"so100_render_cams: flat_pitch < ncam*3*H*W") in err, (k, pitch, err)
    # so does the image size: width * height * ncam <= 1 << 22
    for k, w, h, ok in ((1, 2048, 2048, True), (2, 2048, 2048, False), (2, 2048, 1024, True), (4, 1024, 1024, True),
                        (4, 1024, 1025, False), (3, 4096, 342, False), (1, 4097, 1, False), (1, 0, 8, False)):
        rc, err = call(lib, cams_of(k), out, aux, w=w, h=h)
        assert rc != 0 and (b"NULL env" if ok else b"so100_render_cams: bad image size") in err, (k, w, h, err)
    # what so100_render_aux refuses: no sink at all across both structs, then the NULL env
    for o, a in ((_native.SO100ImageOut(), _native.SO100AuxOut()), (None, _native.SO100AuxOut()), (None, None),
                 (_native.SO100ImageOut(), None)):
        rc, err = call(lib, cams_of(2), o, a)
        assert rc != 0 and b"so100_render_cams: no sink (hwc, chw, flat, depth and label are all NULL)" in err, err
    for o, a in ((None, _native.SO100AuxOut(label=BIG)), (_native.SO100ImageOut(chw=BIG), None)):
        rc, err = call(lib, cams_of(2), o, a)
        assert rc != 0 and b"so100_render_cams: NULL env" in err, err
    # the two refusals that need an env's mesh are reached on the GPU (tests/test_gpu_render_cams.py); here their texts
    blob = open(_native.LIB_PATH, "rb").read()
    assert b"no labels (so100_render_labels)" in blob and b"no materials (so100_render_materials)" in blob


def test_cameras_argument_checks():
    """Refused at argument level: before the library is loaded or a device touched."""
    from gym_so100 import SO100VecEnv
    from gym_so100.sb3 import SO100SB3VecEnv
    pix = dict(obs_type="so100_pixels_agent_pos", device="cuda:99")
    with pytest.raises(ValueError, match="so100_pixels_agent_pos"):
        SO100VecEnv(4, obs_type="so100_state", device="cuda:99", cameras=("top", "left_wrist"))
    with pytest.raises(ValueError, match="camera 'wrist'"):
        SO100VecEnv(4, cameras=("top", "wrist"), **pix)
    with pytest.raises(ValueError, match=r"1\.\.4 cameras"):
        SO100VecEnv(4, cameras=(), **pix)
    with pytest.raises(ValueError, match=r"1\.\.4 cameras"):
        SO100VecEnv(4, cameras=("top",) * 5, **pix)
    with pytest.raises(ValueError, match="tuple of camera names"):
        SO100VecEnv(4, cameras="top", **pix)
    with pytest.raises(ValueError, match="so100_pixels_agent_pos"):
        SO100SB3VecEnv(4, device="cuda:99", cameras=("top",))
    with pytest.raises(ValueError, match="channels_first=True"):
        SO100SB3VecEnv(4, cameras=("top", "left_wrist"), **pix)
    # camera 0 keeps the seed (one camera reproduces CameraRenderer's records); the others get their own
    seeds = [R.camera_seed(7, c) for c in range(4)]
    assert seeds[0] == 7 and len(set(seeds)) == 4 and all(0 <= s < 1 << 64 for s in seeds)
    assert R.camera_seed(7, 1) != R.camera_seed(8, 1) and R.camera_seed(-1, 0) == (1 << 64) - 1


def test_mounted_cameras():
    scene = R.load_scene()
    w = R.camera_by_name(scene, "left_wrist")
    assert (w.frame_body, list(w.pos), w.fovy, w.track) == (6, [0.0, 0.0, pytest.approx(0.55)], 20.0, 1)
    top = R.make_camera(scene, "top")
    assert (w.nlight, w.znear, w.head_ambient) == (top.nlight, top.znear, top.head_ambient)
    assert not hasattr(R.camera_by_name(scene, "top"), "frame_body")
    r = R.make_mounted_camera(scene, 3, (0.1, 0.2, 0.3), mat=np.eye(3)[[1, 2, 0]], fovy=60)
    assert (r.frame_body, r.track, r.fovy, list(r.mat)) == (3, 0, 60.0, [0, 1, 0, 0, 0, 1, 1, 0, 0])
    for body in (0, 9):
        with pytest.raises(ValueError, match="rides on body"):
            R.make_mounted_camera(scene, body, (0, 0, 0))
    # the numpy frame: a world camera is returned as it is, a mounted one moves with its body
    Rb = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    frames = [(np.eye(3), np.zeros(3))] * 3 + [(Rb, np.array([1.0, 2, 3]))]
    cam = {"pos": np.array([0.1, 0.2, 0.3]), "mat": np.eye(3), "track": 0}
    assert C.world_camera(cam, 0, frames) is cam
    wc = C.world_camera(cam, 3, frames)
    assert np.allclose(wc["pos"], [0.8, 2.1, 3.3]) and np.array_equal(wc["mat"], Rb)
    wt = C.world_camera(dict(cam, track=1), 3, frames)
    assert np.allclose(wt["pos"], wc["pos"]) and wt["mat"] is cam["mat"]          # the tracking rule sets it later


@pytest.mark.parametrize("name", ["left_wrist", "rigid"])
def test_reference_alone_is_inside_the_gpu_bars(model, oracle64, oracle32, name):
    """What the number format alone costs on the mounted cameras' images: label and colour shares inside the 1 %
    silhouette cap per env, a real foreground, and the float32 depth maximum inside 5.9e-5, the per-set maximum that
    render_aux_ref.DEPTH_REL_BAR is 4 x of, so that bar holds for the GPU test as it is."""
    r64, r32 = C.reference(model, oracle64, 64, name), C.reference(model, oracle32, 32, name)
    assert len(r64) == len(r32) == 12
    worst, fg, ncls = 0.0, [], []
    for (rgb_a, dep_a, lab_a), (rgb_b, dep_b, lab_b) in zip(r64, r32):
        assert (lab_a != lab_b).mean() <= 0.01 and np.any(rgb_a != rgb_b, axis=-1).mean() <= 0.01
        bg = lab_a == A.BACKGROUND
        assert np.all(dep_a[bg] == 0.0) and dep_a.dtype == np.float32
        same = (lab_a == lab_b) & ~bg
        rel = np.abs(dep_b[same].astype(np.float64) - dep_a[same]) / dep_a[same]
        worst = max(worst, float(rel.max()))
        fg.append(float((~bg).mean()))
        ncls.append(len(set(np.unique(lab_a).tolist()) - {A.BACKGROUND}))
    print(f"{name}: foreground share {min(fg):.2f}-{max(fg):.2f}, classes {min(ncls)}-{max(ncls)}, float32 helper's "
          f"largest relative depth error {worst:.3g}")
    assert worst <= 5.9e-5 and C.DEPTH_REL_BAR == A.DEPTH_REL_BAR, worst
    assert min(ncls) >= 3
    if name == "left_wrist":
        assert min(fg) >= 0.05 and max(fg) > 0.5
    else:
        assert sum(f >= 0.05 for f in fg) >= 6              # foreground >= 5 % in at least half the states
