"""Depth and segmentation images (C-ABI so100_render_aux, csrc/so100_render_aux.hip; DESIGN.md 3.7 "Depth and labels").

1. colour is untouched: the hwc / chw / flat sinks of so100_render_aux are so100_render_to's (views NULL) and
   so100_render_views' (identity and sampled records) bit for bit;
2. labels against the float64 reference (tests/render_aux_ref.py): < 1 % of an env's pixels differ, every class occurs;
3. depth against it on the pixels whose labels agree: within DEPTH_REL_BAR (4 x what float32 numpy costs on these
   scenes, measured by tests/test_render_aux_cpu.py), background exactly 0;
4. nothing is written outside an env's span of either sink, at odd sizes, odd byte offsets and under a mask;
5. determinism, and permuted states and view records give the permuted images;
6. through SO100VecEnv: the options change nothing else, the terminal images show the terminal state, and the cube's
   label lies where the image is red;
7. the refusals that need an env: a label sink without labels, views without materials.

The scenes are hand-set states (render_aux_ref.scene_states), not rollouts, so the CPU test has judged them before."""
import ctypes

import numpy as np
import pytest
import torch

import render_aux_ref as A
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R

pytestmark = pytest.mark.gpu
PIX = "so100_pixels_agent_pos"
RANGES = dict(camera_pos=0.03, camera_rot_deg=float(np.degrees(0.05)), fovy=(0.9, 1.1), ambient=(0.6, 1.4),
              headlight=(0.6, 1.4), lights=(0.6, 1.4), light_rot_deg=float(np.degrees(0.17)), colors=(0.6, 1.2))
SENT8, SENTF = 0xA5, -7.0
_ENVS = {}


def state_env(n):
    """n state-mode envs that only lend their handle to renderers (never stepped); built once per n."""
    if n not in _ENVS:
        _ENVS[n] = SO100VecEnv(n, autoreset=False, max_episode_steps=0)
    return _ENVS[n]


def colour_sinks(n, W, H, dev):
    return {"hwc": torch.full((n, H, W, 3), SENT8, dtype=torch.uint8, device=dev),
            "chw": torch.full((n, 3, H, W), SENT8, dtype=torch.uint8, device=dev),
            "flat": torch.full((n, 3 * W * H + 3), SENTF, dtype=torch.float32, device=dev)}


def image_out(t):
    return _native.SO100ImageOut(hwc=_native.ptr(t.get("hwc")), chw=_native.ptr(t.get("chw")),
                                 flat=_native.ptr(t.get("flat")), flat_pitch=t["flat"].shape[1] if "flat" in t else 0)


def launch(r, which, q, t, views=None, mask=None, depth=None, label=None):
    """One raw C-ABI launch of renderer r's env: which = "to" / "views" / "aux"; depth / label are device addresses."""
    v = r.venv
    out = image_out(t)
    head = (v._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(r.camera))
    if which == "to":
        rc = v.lib.so100_render_to(*head, r.width, r.height, ctypes.byref(out), v._stream())
    elif which == "views":
        rc = v.lib.so100_render_views(*head, _native.ptr(views), r.width, r.height, ctypes.byref(out), v._stream())
    else:
        aux = _native.SO100AuxOut(depth=depth, label=label)
        rc = v.lib.so100_render_aux(*head, _native.ptr(views), r.width, r.height, ctypes.byref(out), ctypes.byref(aux),
                                    v._stream())
    _native.check(rc, "so100_render_" + which)


# ------------------------------------------------------------------------------------------ 1. colour is untouched
@pytest.mark.parametrize("k", range(len(A.SCENE_SETS)))
def test_colour_sinks_are_the_other_launches(k):
    name, W, H, qpos = A.scene_states()[k]
    n = len(qpos)
    env = state_env(n)
    r = R.CameraRenderer(env, W, H, camera=name)
    q = torch.from_numpy(qpos).to(env.device)
    cases = [("to", None)]
    if (W, H) in ((37, 29), (96, 72)):
        cases += [("views", r.identity_views().clone()), ("views", r.sample_views(RANGES, 5).clone())]
        r.views = None
    for which, views in cases:
        a, b = colour_sinks(n, W, H, env.device), colour_sinks(n, W, H, env.device)
        dep = torch.full((n, H, W), SENTF, dtype=torch.float32, device=env.device)
        lab = torch.full((n, H, W), 77, dtype=torch.uint8, device=env.device)
        launch(r, which, q, a, views=views)
        launch(r, "aux", q, b, views=views, depth=dep.data_ptr(), label=lab.data_ptr())
        torch.cuda.synchronize()
        for key in a:
            assert torch.equal(a[key], b[key]), (which, key)
        assert int(a["hwc"].max()) > 0 and bool((a["flat"][:, -3:] == SENTF).all())
        assert float(dep.min()) >= 0.0 and int((lab == 77).sum()) == 0
        # a colour sink alone through the aux kernel, and the aux sinks alone: the same bytes again
        c = {"hwc": torch.full_like(a["hwc"], SENT8)}
        dep2, lab2 = torch.full_like(dep, SENTF), torch.full_like(lab, 77)
        launch(r, "aux", q, c, views=views)
        launch(r, "aux", q, {}, views=views, depth=dep2.data_ptr(), label=lab2.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(c["hwc"], a["hwc"]) and torch.equal(dep2, dep) and torch.equal(lab2, lab)


# ------------------------------------------------------------------------------ 2, 3. labels and depth against float64
def test_labels_and_depth_match_the_float64_reference(model, oracle64):
    ref = A.reference(model, oracle64, 64)
    full = 0
    for name, W, H, qpos, imgs in ref:
        n = len(qpos)
        env = state_env(n)
        r = R.CameraRenderer(env, W, H, camera=name, depth=True, segmentation=True)
        img = r.render(qpos=torch.from_numpy(qpos).to(env.device))
        torch.cuda.synchronize()
        img, dep, lab = img.cpu().numpy(), r.depth.cpu().numpy(), r.segmentation.cpu().numpy()
        worst_lab = worst_rel = 0.0
        for i, (rgb0, dep0, lab0) in enumerate(imgs):
            share = float((lab[i] != lab0).mean())
            worst_lab = max(worst_lab, share)
            bg = lab[i] == R.SEG_BACKGROUND
            same = (lab[i] == lab0) & ~bg
            rel = np.abs(dep[i][same].astype(np.float64) - dep0[same]) / dep0[same]
            worst_rel = max(worst_rel, float(rel.max()))
            print(f"{name} {W}x{H} env {i}: label-diff share {share:.4f}, colour-diff share "
                  f"{float(np.any(img[i] != rgb0, axis=-1).mean()):.4f}, largest relative depth error {rel.max():.3g}, "
                  f"median {np.median(rel):.3g}")
            assert share < 0.01, (name, i, share)
            assert np.any(img[i] != rgb0, axis=-1).mean() < 0.01
            assert np.all(dep[i][bg] == 0.0) and np.all(dep[i][~bg] > 0.3) and np.all(dep[i][~bg] < 1.1)
            assert rel.max() <= A.DEPTH_REL_BAR, (name, i, float(rel.max()))
            if (name, W, H) == ("top", 96, 72) and set(np.unique(lab[i]).tolist()) == set(range(10)) | {255}:
                full += 1
        print(f"SET {name} {W}x{H}: worst label-diff share {worst_lab:.4f}, GPU depth maximum {worst_rel:.3g} "
              f"(bar {A.DEPTH_REL_BAR:.3g})")
    assert full >= 1                          # every class 0-9 and the background in one 96x72 top image


# ---------------------------------------------------------------------------------- 4. nothing outside the spans
@pytest.mark.parametrize("W,H", [(37, 29), (99, 45), (2050, 2)])
def test_nothing_is_written_outside_the_spans(W, H):
    n = 5
    env = state_env(n)
    r = R.CameraRenderer(env, W, H, camera="top")
    qpos =np.concatenate([s[3] for s in A.scene_states()])[:n].copy()
    q = torch.from_numpy(qpos).to(env.device)
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=env.device)
    keep = mask.bool().cpu()
    # the plain images of all five envs
    dep0 = torch.zeros(n, H, W, dtype=torch.float32, device=env.device)
    lab0 = torch.zeros(n, H, W, dtype=torch.uint8, device=env.device)
    launch(r, "aux", q, {}, depth=dep0.data_ptr(), label=lab0.data_ptr())
    span = n * H * W
    for off in (1, 2, 3):
        # label: a slice at byte offset `off` of a sentinel-filled tensor; depth: at float offset `off` (4-byte aligned)
        lab_buf = torch.full((span + 8,), SENT8, dtype=torch.uint8, device=env.device)
        dep_buf = torch.full((span + 8,), SENTF, dtype=torch.float32, device=env.device)
        chw_buf = torch.full((3 * span + 8,), SENT8, dtype=torch.uint8, device=env.device)
        t = {"chw": chw_buf[off:off + 3 * span].view(n, 3, H, W)}
        launch(r, "aux", q, t, mask=mask, depth=dep_buf.data_ptr() + 4 * off, label=lab_buf.data_ptr() + off)
        torch.cuda.synchronize()
        for buf, sent, ref in ((lab_buf, SENT8, lab0), (dep_buf, SENTF, dep0)):
            b = buf.cpu()
            assert bool((b[:off] == sent).all()) and bool((b[off + span:] == sent).all()), (off, buf.dtype)
            got = b[off:off + span].view(n, H, W)
            assert torch.equal(got[keep], ref.cpu()[keep]), (off, buf.dtype)
            assert bool((got[~keep] == sent).all()), (off, buf.dtype)           # masked-out envs are intact
        c = chw_buf.cpu()
        assert bool((c[:off] == SENT8).all()) and bool((c[off + 3 * span:] == SENT8).all())
        assert bool((c[off:off + 3 * span].view(n, 3, H, W)[~keep] == SENT8).all())
    if H > 2:                                 # (the one-row bands' strip is nearly all background)
        assert int((lab0 != R.SEG_BACKGROUND).sum()) > 0 and float(dep0.max()) > 0.3


# ------------------------------------------------------------------------------- 5. determinism and permutation
def test_deterministic_and_per_env():
    name, W, H, qpos = A.scene_states()[0]
    n = len(qpos)
    env = state_env(n)
    r = R.CameraRenderer(env, W, H, camera=name)
    perm = torch.tensor([3, 0, 5, 1, 4, 2], device=env.device)
    q = torch.from_numpy(qpos).to(env.device)
    views = r.sample_views(RANGES, 9).clone()
    r.views = None

    def draw(q, views):
        dep = torch.zeros(n, H, W, dtype=torch.float32, device=env.device)
        lab = torch.zeros(n, H, W, dtype=torch.uint8, device=env.device)
        launch(r, "aux", q, {}, views=views, depth=dep.data_ptr(), label=lab.data_ptr())
        torch.cuda.synchronize()
        return dep, lab

    first = {}
    for tag, vw in (("plain", None), ("views", views)):
        d0, l0 = draw(q, vw)
        d1, l1 = draw(q, vw)
        assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(l0, l1)
        dp, lp = draw(q[perm].contiguous(), None if vw is None else vw[perm].contiguous())
        assert torch.equal(dp.view(torch.int32), d0[perm].view(torch.int32)) and torch.equal(lp, l0[perm])
        first[tag] = d0
    assert not torch.equal(first["plain"], first["views"])        # the records do move the camera
    assert not torch.equal(first["plain"][0], first["plain"][1])  # and the envs differ


# ---------------------------------------------------------------------------------------------- 6. SO100VecEnv
def test_vec_env_options_change_nothing_else():
    kw = dict(obs_type=PIX, observation_width=64, observation_height=48, seed=3)
    a = SO100VecEnv(4, **kw)
    b = SO100VecEnv(4, depth=True, segmentation=True, **kw)
    oa, _ = a.reset(seed=5)
    ob, _ = b.reset(seed=5)
    assert set(ob) == set(oa) | {"depth", "segmentation"}
    assert ob["depth"].shape == (4, 48, 64) and ob["depth"].dtype == torch.float32
    assert ob["segmentation"].shape == (4, 48, 64) and ob["segmentation"].dtype == torch.uint8
    g = torch.Generator().manual_seed(0)
    for _ in range(30):
        act = torch.rand(4, 6, generator=g) * 2 - 1
        oa, ra, ta, ua, ia = a.step(act)
        ob, rb, tb, ub, ib = b.step(act)
        for x, y in ((a.qpos, b.qpos), (a.qvel, b.qvel), (a.obs, b.obs), (ra, rb), (ta, tb), (ua, ub),
                     (oa["pixels"], ob["pixels"]), (oa["agent_pos"], ob["agent_pos"])):
            assert torch.equal(x, y)
        # the cube's label lies where the image is red, and nowhere else (the base view): the cube is the one
        # body whose colour has G = B = 0 < R.  Its lit top face is R > 200; a side face is darker (R 146-196 in the
        # float64 reference's own images of these spawns), so "R > 200" alone holds one way only
        px, seg = ob["pixels"], ob["segmentation"]
        red = (px[..., 0] > 0) & (px[..., 1] == 0) & (px[..., 2] == 0)
        assert torch.equal(seg == 9, red)
        assert bool((seg[(px[..., 0] > 200) & (px[..., 1] == 0) & (px[..., 2] == 0)] == 9).all())
        assert bool(((ob["depth"] == 0) == (seg == R.SEG_BACKGROUND)).all())
    assert int((ob["segmentation"] == 9).sum()) > 0
    g2 = SO100VecEnv(2, task="so100_goal", depth=True, segmentation=True, **kw)
    og, _ = g2.reset(seed=1)
    assert og["observation"].shape == (2, 64 * 48 * 3 + 6) and og["depth"].shape == (2, 48, 64) and \
        og["segmentation"].shape == (2, 48, 64)


def test_vec_env_terminal_images_show_the_terminal_state():
    kw = dict(obs_type=PIX, observation_width=64, observation_height=48, seed=3)
    a = SO100VecEnv(4, max_episode_steps=5, depth=True, segmentation=True, **kw)
    twin = SO100VecEnv(4, autoreset=False, max_episode_steps=0, **kw)       # the same states, never reset
    a.reset(seed=5)
    twin.reset(seed=5)
    g = torch.Generator().manual_seed(1)
    for t in range(5):
        act = torch.rand(4, 6, generator=g) * 2 - 1
        prev = a.qpos.clone()
        ob, _, term, trunc, info = a.step(act)
        twin.step(act)
        if t < 4:
            assert torch.equal(a.qpos, twin.qpos) and not bool((term | trunc).any())
    done = term | trunc
    assert bool(done.all()) and torch.equal(info["_final_observation"], done)
    fin = info["final_observation"]
    assert set(fin) == {"pixels", "agent_pos", "depth", "segmentation"}
    px = torch.zeros_like(a.pixels)
    dep, seg = torch.zeros_like(a.depth), torch.zeros_like(a.segmentation)
    a.renderer.render(qpos=twin.qpos, out=px, depth=dep, segmentation=seg)
    torch.cuda.synchronize()
    assert torch.equal(fin["pixels"], px) and torch.equal(fin["segmentation"], seg)
    assert torch.equal(fin["depth"].view(torch.int32), dep.view(torch.int32))
    assert not torch.equal(ob["depth"], fin["depth"]) and not torch.equal(a.qpos, prev)     # the new episode's images


# --------------------------------------------------------------------------------------------------- 7. refusals
def test_label_sink_needs_labels_and_views_need_materials():
    env = SO100VecEnv(2, autoreset=False, max_episode_steps=0)
    r = R.CameraRenderer(env, 16, 12)
    scene = R.load_scene()
    tri = np.ascontiguousarray(scene["tri"], dtype=np.float32)
    body = np.ascontiguousarray(scene["body"], dtype=np.int32)
    rgb = np.ascontiguousarray(scene["rgb"], dtype=np.float32)
    # a new mesh drops the labels and the materials of the one before
    _native.check(env.lib.so100_render_mesh(env._handle, tri.ctypes.data, body.ctypes.data, rgb.ctypes.data, len(body)),
                  "so100_render_mesh")
    dep = torch.full((2, 12, 16), SENTF, dtype=torch.float32, device=env.device)
    lab = torch.full((2, 12, 16), SENT8, dtype=torch.uint8, device=env.device)
    views = torch.zeros(2, _native.VIEW_WORDS, dtype=torch.int32, device=env.device)
    with pytest.raises(RuntimeError, match=r"so100_render_aux: no labels \(so100_render_labels\)"):
        launch(r, "aux", env.qpos, {}, depth=dep.data_ptr(), label=lab.data_ptr())
    with pytest.raises(RuntimeError, match=r"so100_render_aux: no materials \(so100_render_materials\)"):
        launch(r, "aux", env.qpos, {}, views=views, depth=dep.data_ptr())
    bad = np.full(len(body), 255, dtype=np.uint8)
    assert env.lib.so100_render_labels(env._handle, bad.ctypes.data, len(bad)) != 0
    assert b"label 255" in env.lib.so100_last_error()
    assert env.lib.so100_render_labels(env._handle, bad.ctypes.data, len(bad) - 1) != 0
    assert b"the mesh has" in env.lib.so100_last_error()
    torch.cuda.synchronize()
    assert bool((dep == SENTF).all()) and bool((lab == SENT8).all())      # refused before any device work
    launch(r, "aux", env.qpos, {}, depth=dep.data_ptr())                   # depth alone needs neither
    torch.cuda.synchronize()
    assert float(dep.max()) > 0.3
