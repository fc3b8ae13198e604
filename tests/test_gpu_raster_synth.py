"""The rasteriser's body (csrc/so100_render.h) on synthetic meshes, through every launch that shares it, held to the
restatements exactly on kept pixels (tests/raster_synth_ref.py: the meshes, the margin rule and its measured bars;
tests/test_raster_synth_cpu.py has judged the references before).

Per mesh: so100_render; so100_render_to on its hwc, chw and flat sinks under a mask; so100_render_aux without views and
with identity view records; so100_render_cams with two cameras, the second mounted on the cube; so100_render_shadow
with light = -1; and for the multisampled cases so100_render_msaa with the same two cameras.  On kept pixels colour
(hence the winning triangle, see raster_synth_ref) and label are exact and depth is within DEPTH_REL_BAR; the background
is 0, 0.0f and 255; a masked env keeps its sentinel; every launch's colour sinks equal so100_render's bit for bit on all
pixels; a second launch of the same inputs is bitwise the first, list overflow included.

The env is this module's own: so100_render_mesh replaces the mesh and drops the labels, materials and casters, which
are uploaded again after each mesh."""
import ctypes

import numpy as np
import pytest
import torch

import raster_synth_ref as S
from gym_so100 import SO100VecEnv, _native

pytestmark = pytest.mark.gpu
N = S.N_ENVS
SENT8, SENTF = 0xA5, -7.0


@pytest.fixture(scope="module")
def env():
    e = SO100VecEnv(N, autoreset=False, max_episode_steps=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fr64(model, oracle64):
    return S.frames(oracle64, model)


@pytest.fixture(scope="module")
def cases(fr64):
    return S.cases(fr64[0][S.LINK])


def upload(env, mesh):
    lib, h, T = env.lib, env._handle, len(mesh["body"])
    _native.check(lib.so100_render_mesh(h, mesh["tri"].ctypes.data, mesh["body"].ctypes.data, mesh["rgb"].ctypes.data, T),
                  "so100_render_mesh")
    _native.check(lib.so100_render_materials(h, mesh["material"].ctypes.data, T), "so100_render_materials")
    _native.check(lib.so100_render_labels(h, mesh["label"].ctypes.data, T), "so100_render_labels")
    cast = np.ones(T, np.uint8)
    _native.check(lib.so100_render_casters(h, cast.ctypes.data, T), "so100_render_casters")


def sinks(K, W, H, dev, keys=("hwc", "chw", "flat", "depth", "label")):
    """Sentinel-filled sinks of N envs x K cameras (K None: no camera axis)."""
    k = () if K is None else (K,)
    full = {"hwc": ((N, *k, H, W, 3), SENT8, torch.uint8), "chw": ((N, *k, 3, H, W), SENT8, torch.uint8),
            "flat": ((N, (K or 1) * 3 * W * H + 3), SENTF, torch.float32), "depth": ((N, *k, H, W), SENTF, torch.float32),
            "label": ((N, *k, H, W), 77, torch.uint8)}
    return {key: torch.full(full[key][0], full[key][1], dtype=full[key][2], device=dev) for key in keys}


def structs(t):
    out = _native.SO100ImageOut(hwc=_native.ptr(t.get("hwc")), chw=_native.ptr(t.get("chw")),
                                flat=_native.ptr(t.get("flat")), flat_pitch=t["flat"].shape[1] if "flat" in t else 0)
    return out, _native.SO100AuxOut(depth=_native.ptr(t.get("depth")), label=_native.ptr(t.get("label")))


def launch(env, which, cam, W, H, q, t, views=None, mask=None, msaa=None):
    """One raw C-ABI launch: which = "render" / "to" / "aux" (cam: so100_camera) or "cams" / "shadow" / "msaa" (cam:
    so100_cams)."""
    lib, out_aux = env.lib, structs(t)
    out, aux = out_aux
    head = (env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cam))
    if which == "render":
        rc = lib.so100_render(*head, W, H, _native.ptr(t["hwc"]), env._stream())
    elif which == "to":
        rc = lib.so100_render_to(*head, W, H, ctypes.byref(out), env._stream())
    elif which == "aux":
        rc = lib.so100_render_aux(*head, _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux), env._stream())
    elif which == "cams":
        rc = lib.so100_render_cams(*head, _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux), env._stream())
    elif which == "shadow":
        sh = _native.SO100Shadow(light=-1, map_size=8, center=(0.0, 0.0, 0.0), radius=1.0, bias=0.0)
        rc = lib.so100_render_shadow(*head, _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux),
                                     ctypes.byref(sh), env._stream())
    else:
        ms = _native.SO100Msaa(len(msaa), msaa)
        rc = lib.so100_render_msaa(*head, _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(ms), env._stream())
    _native.check(rc, "so100_render_" + which)


def two_cameras(case):
    """(so100_cams, view records [2, N, 40]): the case's camera in the world, and on the cube the camera that stands
    case["shift"] (default nothing) beside it: its position is held in the cube's frame."""
    cam = case["cam"]
    local = np.asarray(cam["pos"]) + np.asarray(case.get("shift", (0.0, 0.0, 0.0))) - np.asarray(S.CUBE_POS)
    cams = _native.SO100Cams([S.camera_struct(cam), S.camera_struct(cam, pos=local)], [0, S.CUBE])
    return cams, np.stack([S.view_words(cam, N), S.view_words(cam, N, pos=local)])


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def packed(img):
    img = img.astype(np.uint32)
    return img[..., 0] | (img[..., 1] << 8) | (img[..., 2] << 16)


def colour_sinks_agree(t, hwc, envs, where):
    """chw and flat are the hwc bytes (flat: numpy's float32 byte / 255, sentinel beyond), and hwc is `hwc` bit for bit
    on all pixels of `envs`."""
    a = t["hwc"].cpu().numpy()
    assert np.array_equal(a[envs], hwc[envs]), where
    if "chw" in t:
        assert np.array_equal(np.moveaxis(t["chw"].cpu().numpy(), -3, -1)[envs], a[envs]), where
    if "flat" in t:
        f = t["flat"].cpu().numpy()
        assert np.all(f[:, -3:] == SENTF), where
        assert np.array_equal(f[:, :-3].reshape(a.shape)[envs], (a.astype(np.float32) / np.float32(255))[envs]), where


def grade(case, ref, rgb, depth=None, label=None, where="", expect_rgb=None, colours=True):
    """One env's image against its reference on kept pixels: colour and label exact, depth within the bar, the
    background exactly 0, 0.0f, 255.  The lit case's colours are graded by their share (under 1 %), as the real
    scene's are.  expect_rgb: packed colours to hold the image to instead of the reference's; colours=False:
    none (the lit case under the view records' colours)."""
    keep, win = ref["keep"], ref["win"]
    want = packed(ref["rgb"]) if expect_rgb is None else expect_rgb
    got = packed(rgb)
    if not colours:
        pass
    elif case["kind"] == "lit":
        assert float((got != want)[keep].mean()) < 0.01, where
    else:
        bad = (got != want) & keep
        assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.all(got[keep & (win < 0)] == 0), where
    if label is not None:
        bad = (label != ref["label"]) & keep
        assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    if depth is not None:
        fg = keep & (win >= 0)
        assert np.all(depth[keep & (win < 0)] == 0.0) and depth.dtype == np.float32, where
        rel = np.abs(depth[fg].astype(np.float64) - ref["depth"][fg]) / ref["depth"][fg]
        if fg.any():
            assert rel.max() <= S.DEPTH_REL_BAR, (where, float(rel.max()))


def palette_reference(case, refs, fr64):
    """[env] of (reference, packed colours) for a launch with view records, which colours triangle t PALETTE[material
    [t]]: off a tie the winner is the same triangle, so the colours follow from the reference's winner; an exact case
    (ties among them) is drawn again with those colours."""
    mesh = case["mesh"]
    out = []
    for e, ref in enumerate(refs):
        if case["exact"]:
            r = S.render(case, fr64[e], np.float32, mesh=S.palette_mesh(mesh))
            r["keep"] = ref["keep"]
            out.append((r, packed(r["rgb"])))
        else:
            col = np.where(ref["win"] >= 0, S.PALETTE[mesh["material"][np.maximum(ref["win"], 0)]], 0)
            out.append((ref, None if case["kind"] == "lit" else col.astype(np.uint32)))
    return out


@pytest.mark.parametrize("name", S.SINGLE)
def test_single_sample_launches(env, cases, fr64, name):
    case = cases[name]
    W, H, dev = case["W"], case["H"], env.device
    refs = S.reference(case, fr64)
    upload(env, case["mesh"])
    q = torch.from_numpy(S.qpos()).to(dev)
    cam = S.camera_struct(case["cam"])
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    every, unmasked = [0, 1, 2], [0, 2]

    # so100_render, twice: against the reference, and deterministic
    a, b = sinks(None, W, H, dev, ("hwc",)), sinks(None, W, H, dev, ("hwc",))
    launch(env, "render", cam, W, H, q, a)
    launch(env, "render", cam, W, H, q, b)
    torch.cuda.synchronize()
    assert torch.equal(a["hwc"], b["hwc"])
    hwc = a["hwc"].cpu().numpy()
    for e in every:
        grade(case, refs[e], hwc[e], where=(name, "render", e))

    # so100_render_to under a mask: three sinks, env 1 keeps its sentinels
    t = sinks(None, W, H, dev, ("hwc", "chw", "flat"))
    launch(env, "to", cam, W, H, q, t, mask=mask)
    torch.cuda.synchronize()
    colour_sinks_agree(t, hwc, unmasked, (name, "to"))
    assert bool((t["hwc"][1] == SENT8).all()) and bool((t["chw"][1] == SENT8).all()) and bool((t["flat"][1] == SENTF).all())

    # so100_render_aux without views, twice
    t, u = sinks(None, W, H, dev), sinks(None, W, H, dev)
    launch(env, "aux", cam, W, H, q, t)
    launch(env, "aux", cam, W, H, q, u)
    torch.cuda.synchronize()
    for key in t:
        assert same_bits(t[key], u[key]), (name, "aux twice", key)
    colour_sinks_agree(t, hwc, every, (name, "aux"))
    dep, lab = t["depth"].cpu().numpy(), t["label"].cpu().numpy()
    for e in every:
        grade(case, refs[e], hwc[e], dep[e], lab[e], where=(name, "aux", e))

    # so100_render_aux with identity view records (the materials' colours) under the mask
    pal = palette_reference(case, refs, fr64)
    views = torch.from_numpy(S.view_words(case["cam"], N)).to(dev)
    v = sinks(None, W, H, dev)
    launch(env, "aux", cam, W, H, q, v, views=views, mask=mask)
    torch.cuda.synchronize()
    vh, vd, vl = v["hwc"].cpu().numpy(), v["depth"].cpu().numpy(), v["label"].cpu().numpy()
    colour_sinks_agree(v, vh, unmasked, (name, "aux views"))
    for e in unmasked:
        grade(case, pal[e][0], vh[e], vd[e], vl[e], where=(name, "aux views", e), expect_rgb=pal[e][1],
              colours=case["kind"] != "lit")
    assert np.all(vh[1] == SENT8) and np.all(vd[1] == SENTF) and np.all(vl[1] == 77)
    if not case["exact"]:                                   # off a tie the colours decide nothing else
        assert np.array_equal(vd[unmasked].view(np.uint32), dep[unmasked].view(np.uint32))
        assert np.array_equal(vl[unmasked], lab[unmasked])

    # so100_render_cams: the world camera and the one mounted on the cube; so100_render_shadow with nothing casting
    cams, vw = two_cameras(case)
    c, s = sinks(2, W, H, dev), sinks(2, W, H, dev)
    launch(env, "cams", cams, W, H, q, c)
    launch(env, "shadow", cams, W, H, q, s)
    torch.cuda.synchronize()
    for key in c:
        assert same_bits(c[key], s[key]), (name, "shadow is cams", key)
    ch, cd, cl = c["hwc"].cpu().numpy(), c["depth"].cpu().numpy(), c["label"].cpu().numpy()
    colour_sinks_agree(c, ch, every, (name, "cams"))
    assert np.array_equal(ch[:, 0], hwc), (name, "cams camera 0")
    assert np.array_equal(cd[:, 0].view(np.uint32), dep.view(np.uint32)) and np.array_equal(cl[:, 0], lab)
    refs1 = S.reference(case, fr64, shifted=True) if "shift" in case else refs
    if "shift" not in case:
        assert np.array_equal(ch[:, 1], hwc) and np.array_equal(cd[:, 1].view(np.uint32), dep.view(np.uint32))
    else:
        assert not np.array_equal(ch[:, 1], hwc)
    for e in every:
        grade(case, refs1[e], ch[e, 1], cd[e, 1], cl[e, 1], where=(name, "cams mounted", e))
    # and with view records under the mask
    cv = sinks(2, W, H, dev)
    launch(env, "cams", cams, W, H, q, cv, views=torch.from_numpy(vw).to(dev), mask=mask)
    torch.cuda.synchronize()
    for key in ("hwc", "depth", "label"):
        assert same_bits(cv[key][unmasked, 0], v[key][unmasked]), (name, "cams views", key)
    assert bool((cv["hwc"][1] == SENT8).all()) and bool((cv["depth"][1] == SENTF).all())
    if "shift" not in case:
        assert same_bits(cv["hwc"][unmasked, 1], v["hwc"][unmasked]), (name, "cams views mounted")


@pytest.mark.parametrize("name", S.MULTI)
def test_multisampled_launch(env, cases, fr64, name):
    case = cases[name]
    W, H, dev = case["W"], case["H"], env.device
    ref = S.reference(case, fr64)[0]                        # (these meshes are on the world body: one image)
    assert S.world_only(case["mesh"])
    upload(env, case["mesh"])
    q = torch.from_numpy(S.qpos()).to(dev)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    cams, vw = two_cameras(case)
    keys = ("hwc", "chw", "flat")
    a, b, m = sinks(2, W, H, dev, keys), sinks(2, W, H, dev, keys), sinks(2, W, H, dev, keys)
    launch(env, "msaa", cams, W, H, q, a, msaa=case["msaa"])
    launch(env, "msaa", cams, W, H, q, b, msaa=case["msaa"])
    launch(env, "msaa", cams, W, H, q, m, msaa=case["msaa"], mask=mask)
    torch.cuda.synchronize()
    for key in keys:
        assert same_bits(a[key], b[key]), (name, "twice", key)
        assert same_bits(a[key][[0, 2]], m[key][[0, 2]]), (name, "mask", key)
    assert bool((m["hwc"][1] == SENT8).all()) and bool((m["chw"][1] == SENT8).all()) and bool((m["flat"][1] == SENTF).all())
    hwc = a["hwc"].cpu().numpy()
    colour_sinks_agree(a, hwc, [0, 1, 2], name)
    want, keep = packed(ref["rgb_msaa"]), ref["keep"]
    for e in range(N):
        for c in range(2):
            bad = (packed(hwc[e, c]) != want) & keep
            assert not bad.any(), (name, e, c, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # with view records: the resolved mean of the samples' palette colours
    smp = np.where(ref["swin"] >= 0, S.PALETTE[case["mesh"]["material"][np.maximum(ref["swin"], 0)]], 0).astype(np.uint32)
    if case["exact"]:
        smp = packed(S.render(case, fr64[0], np.float32, mesh=S.palette_mesh(case["mesh"]))["smp"])
    mean = sum((((smp >> (8 * k)) & 0xFF).sum(axis=0) + len(smp) // 2) // len(smp) << (8 * k) for k in range(3))
    v = sinks(2, W, H, dev, ("hwc",))
    launch(env, "msaa", cams, W, H, q, v, views=torch.from_numpy(vw).to(dev), msaa=case["msaa"])
    torch.cuda.synchronize()
    vh = v["hwc"].cpu().numpy()
    for e in range(N):
        for c in range(2):
            bad = (packed(vh[e, c]) != mean) & keep
            assert not bad.any(), (name, "views", e, c, int(bad.sum()))


def test_a_tie_keeps_the_single_triangles_depth_bits(env, cases):
    """The duplicates of the ties mesh, in either mesh order, leave the depth image of the mesh that states each
    triangle once, bit for bit; colour and label are the same in both orders."""
    dev = env.device
    q = torch.from_numpy(S.qpos()).to(dev)
    got = {}
    for name in ("ties", "ties_reversed", "ties_single"):
        case = cases[name]
        upload(env, case["mesh"])
        t = sinks(None, 128, 64, dev, ("hwc", "depth", "label"))
        launch(env, "aux", S.camera_struct(case["cam"]), 128, 64, q, t)
        torch.cuda.synchronize()
        got[name] = t
    for key in ("hwc", "depth", "label"):
        assert same_bits(got["ties"][key], got["ties_reversed"][key]), key
    assert same_bits(got["ties"]["depth"], got["ties_single"]["depth"])
    assert float(got["ties"]["depth"].max()) > 3.9 and int((got["ties"]["label"] != 255).sum()) > 1000
    hwc, lab = got["ties"]["hwc"][0].cpu().numpy(), got["ties"]["label"][0].cpu().numpy()
    for x, y, colour, label in cases["ties"]["expect"]:
        assert (int(packed(hwc[y, x])), int(lab[y, x])) == (colour, label), (x, y)
