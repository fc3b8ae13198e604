"""Several cameras in one launch (C-ABI so100_render_cams, csrc/so100_render_cams.hip; DESIGN.md 3.7 "Cameras").

1. K = 1 with a world camera is so100_render_aux bit for bit in all five sinks;
2. K = 3 is three so100_render_aux launches: slot (env, c) of every sink is camera c's launch with views[c];
3. the mounted cameras (left_wrist, and a rigid mount) against the float64 reference (tests/render_cams_ref.py) on the
   12 states the CPU test has judged; the same cameras treated as world cameras fail that acceptance;
4. nothing is written outside a slot's span, at odd sizes, odd byte offsets and under a mask;
5. determinism, and permuted states and records give the permuted images;
6. through SO100VecEnv(cameras=...): nothing else changes, camera 0 is the default env's image, the terminal images, the
   flat observation, the per-camera view records and their independence of the sharding;
7. through SO100SB3VecEnv(cameras=...): spaces, host arrays, terminal_observation;
8. the refusals that need an env."""
import ctypes

import numpy as np
import pytest
import torch

import render_aux_ref as A
import render_cams_ref as C
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R

pytestmark = pytest.mark.gpu
PIX = "so100_pixels_agent_pos"
RANGES = dict(camera_pos=0.03, camera_rot_deg=float(np.degrees(0.05)), fovy=(0.9, 1.1), ambient=(0.6, 1.4),
              headlight=(0.6, 1.4), lights=(0.6, 1.4), light_rot_deg=float(np.degrees(0.17)), colors=(0.6, 1.2))
SENT8, SENTF = 0xA5, -7.0
SINKS = ("hwc", "chw", "flat", "depth", "label")
_ENVS = {}


def state_env(n):
    """n state-mode envs that only lend their handle to renderers (never stepped); built once per n."""
    if n not in _ENVS:
        _ENVS[n] = SO100VecEnv(n, autoreset=False, max_episode_steps=0)
    return _ENVS[n]


def sinks(n, K, W, H, dev):
    """The five sinks of n envs x K cameras, sentinel-filled; flat has 3 floats more per env than the launch fills.
    K = None: so100_render_aux's shapes (no camera axis)."""
    k = () if K is None else (K,)
    return {"hwc": torch.full((n, *k, H, W, 3), SENT8, dtype=torch.uint8, device=dev),
            "chw": torch.full((n, *k, 3, H, W), SENT8, dtype=torch.uint8, device=dev),
            "flat": torch.full((n, (K or 1) * 3 * W * H + 3), SENTF, dtype=torch.float32, device=dev),
            "depth": torch.full((n, *k, H, W), SENTF, dtype=torch.float32, device=dev),
            "label": torch.full((n, *k, H, W), 77, dtype=torch.uint8, device=dev)}


def structs(t):
    out = _native.SO100ImageOut(hwc=_native.ptr(t.get("hwc")), chw=_native.ptr(t.get("chw")),
                                flat=_native.ptr(t.get("flat")), flat_pitch=t["flat"].shape[1] if "flat" in t else 0)
    return out, _native.SO100AuxOut(depth=_native.ptr(t.get("depth")), label=_native.ptr(t.get("label")))


def launch_cams(env, cams, W, H, q, t, views=None, mask=None):
    out, aux = structs(t)
    _native.check(env.lib.so100_render_cams(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cams),
                                            _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux),
                                            env._stream()), "so100_render_cams")


def launch_aux(env, cam, W, H, q, t, views=None, mask=None):
    out, aux = structs(t)
    _native.check(env.lib.so100_render_aux(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cam),
                                           _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux),
                                           env._stream()), "so100_render_aux")


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def qpos_of(n, dev):
    return torch.from_numpy(C.states()[:n].copy()).to(dev)


# ------------------------------------------------------------------------------------- 1. K = 1 is the aux launch
@pytest.mark.parametrize("name", ["top", "front_close"])
@pytest.mark.parametrize("W,H", [(37, 29), (96, 72)])
def test_one_world_camera_is_the_aux_launch(name, W, H):
    n = 3
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=(name,))
    assert r.frame_body == (0,)
    q = qpos_of(n, env.device)
    for views in (None, r.identity_views().clone(), r.sample_views(RANGES, 5).clone()):
        r.views = None
        a, b = sinks(n, None, W, H, env.device), sinks(n, 1, W, H, env.device)
        launch_aux(env, r.cameras[0], W, H, q, a, views=None if views is None else views[0])
        launch_cams(env, r.cams, W, H, q, b, views=views)
        torch.cuda.synchronize()
        for key in SINKS:
            assert same_bits(a[key], b[key].view(a[key].shape)), (name, key, views is not None)
        assert int(a["hwc"].max()) > 0 and bool((a["flat"][:, -3:] == SENTF).all())
        assert int((a["label"] == 77).sum()) == 0 and float(a["depth"].min()) >= 0.0


def test_one_camera_reproduces_camera_renderers_records():
    env = state_env(3)
    one, multi = R.CameraRenderer(env, 16, 12, camera="angle"), R.MultiCameraRenderer(env, 16, 12, cameras=("angle",))
    assert torch.equal(one.sample_views(RANGES, 11), multi.sample_views(RANGES, 11)[0])


# -------------------------------------------------------------------------- 2. K = 3 is three aux launches
@pytest.mark.parametrize("W,H", [(37, 29), (64, 48)])
def test_three_cameras_are_three_aux_launches(W, H):
    n, names = 6, ("top", "angle", "front_close")
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=names)
    q = qpos_of(n, env.device)
    npx = 3 * W * H
    for views in (r.identity_views().clone(), r.sample_views(RANGES, 5).clone()):
        r.views = None
        assert views.shape == (3, n, _native.VIEW_WORDS)
        b = sinks(n, 3, W, H, env.device)
        launch_cams(env, r.cams, W, H, q, b, views=views)
        for c in range(3):
            a = sinks(n, None, W, H, env.device)
            launch_aux(env, r.cameras[c], W, H, q, a, views=views[c])
            torch.cuda.synchronize()
            for key in ("hwc", "chw", "depth", "label"):
                assert same_bits(a[key], b[key][:, c].contiguous()), (key, c)
            assert same_bits(a["flat"][:, :npx].contiguous(), b["flat"][:, c * npx:(c + 1) * npx].contiguous()), c
            assert int(a["hwc"].max()) > 0
        assert bool((b["flat"][:, 3 * npx:] == SENTF).all())
        assert not torch.equal(b["hwc"][:, 0], b["hwc"][:, 1])          # the cameras do differ
    assert not torch.equal(views[0, :, 13:], views[1, :, 13:])          # and so do their records' draws


# ---------------------------------------------------------------- 3. mounted cameras against the float64 reference
def violations(img, dep, lab, ref):
    """The acceptance of one camera's images of the 12 states against ref = [(rgb, depth, label)]: per env the shares
    of pixels whose label and whose colour differ <= 1 %, the relative depth error on foreground pixels with agreeing
    labels <= the bar, background exactly 0 / 255.  Returns what is violated, as text."""
    bad = []
    for i, (rgb0, dep0, lab0) in enumerate(ref):
        ls, cs = float((lab[i] != lab0).mean()), float(np.any(img[i] != rgb0, axis=-1).mean())
        bg = lab[i] == R.SEG_BACKGROUND
        same = (lab[i] == lab0) & ~bg
        rel = np.abs(dep[i][same].astype(np.float64) - dep0[same]) / dep0[same]
        mx = float(rel.max()) if rel.size else 0.0
        print(f"env {i}: label-diff share {ls:.4f}, colour-diff share {cs:.4f}, largest relative depth error {mx:.3g}")
        if ls > 0.01:
            bad.append(f"env {i}: label share {ls:.4f}")
        if cs > 0.01:
            bad.append(f"env {i}: colour share {cs:.4f}")
        if mx > C.DEPTH_REL_BAR:
            bad.append(f"env {i}: depth {mx:.3g}")
        if not (np.all(dep[i][bg] == 0.0) and np.all(img[i][bg] == 0) and np.all(dep[i][~bg] > 0.0)):
            bad.append(f"env {i}: background")
    return bad


def test_mounted_cameras_match_the_float64_reference(model, oracle64):
    n, W, H = 12, C.W, C.H
    env = state_env(n)
    scene = R.load_scene()
    mounted = C.mounted_cameras(R, scene)
    names = ("left_wrist", "rigid")
    r = R.MultiCameraRenderer(env, W, H, cameras=tuple(mounted[k][0] for k in names), depth=True, segmentation=True)
    assert r.frame_body == (6, 6) and [c.track for c in r.cameras] == [1, 0]
    q = qpos_of(n, env.device)
    img = r.render(qpos=q).cpu().numpy()
    dep, lab = r.depth.cpu().numpy(), r.segmentation.cpu().numpy()
    # the same two cameras with frame_body ignored: pos and mat taken as the world's
    world = _native.SO100Cams(r.cameras, (0, 0))
    t = sinks(n, 2, W, H, env.device)
    launch_cams(env, world, W, H, q, t)
    torch.cuda.synchronize()
    for c, name in enumerate(names):
        ref = C.reference(model, oracle64, 64, name)
        print(f"--- {name}")
        assert violations(img[:, c], dep[:, c], lab[:, c], ref) == []
        fg = (lab[:, c] != R.SEG_BACKGROUND).mean(axis=(1, 2))
        assert (fg >= 0.05).sum() >= 6
        print(f"--- {name} as a world camera")
        assert violations(t["hwc"][:, c].cpu().numpy(), t["depth"][:, c].cpu().numpy(), t["label"][:, c].cpu().numpy(),
                          ref) != []


# ---------------------------------------------------------------------------------- 4. nothing outside the spans
@pytest.mark.parametrize("W,H", [(37, 29), (2050, 2)])
def test_nothing_is_written_outside_the_spans(W, H):
    n, K = 5, 2
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top", "left_wrist"))
    q = qpos_of(n, env.device)
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8, device=env.device)
    keep = mask.bool().cpu()
    ref = sinks(n, K, W, H, env.device)                  # the plain images of all five envs
    launch_cams(env, r.cams, W, H, q, ref)
    pitch, px = ref["flat"].shape[1], n * K * H * W
    span = {"hwc": 3 * px, "chw": 3 * px, "label": px, "depth": px, "flat": n * pitch}
    for off in (1, 2, 3):
        # the byte sinks at byte offset `off` of a sentinel-filled tensor, the float sinks at float offset `off`
        buf = {k: torch.full((span[k] + 8,), SENTF if k in ("depth", "flat") else SENT8, dtype=ref[k].dtype,
                             device=env.device) for k in SINKS}
        t = {k: buf[k][off:off + span[k]].view(ref[k].shape) for k in SINKS}
        assert all(t[k].data_ptr() == buf[k].data_ptr() + off * buf[k].element_size() for k in SINKS)
        launch_cams(env, r.cams, W, H, q, t, mask=mask)
        torch.cuda.synchronize()
        for k in SINKS:
            b, sent = buf[k].cpu(), (SENTF if k in ("depth", "flat") else SENT8)
            assert bool((b[:off] == sent).all()) and bool((b[off + span[k]:] == sent).all()), (off, k)
            got = b[off:off + span[k]].view(ref[k].shape)
            assert same_bits(got[keep].contiguous(), ref[k].cpu()[keep].contiguous()), (off, k)
            assert bool((got[~keep] == sent).all()), (off, k)            # every slot of a masked-out env is intact
        assert bool((buf["flat"][off:off + span["flat"]].view(n, pitch)[:, K * 3 * W * H:] == SENTF).all())
    if H > 2:                                 # (the one-row bands' strip is nearly all background)
        assert int((ref["label"] != R.SEG_BACKGROUND).sum()) > 0 and float(ref["depth"].max()) > 0.1


# ------------------------------------------------------------------------------- 5. determinism and permutation
def test_deterministic_and_per_env():
    n, W, H = 6, 37, 29
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top", "left_wrist"))
    perm = torch.tensor([3, 0, 5, 1, 4, 2], device=env.device)
    q = qpos_of(n, env.device)
    views = r.sample_views(RANGES, 9).clone()
    r.views = None

    def draw(q, views):
        t = sinks(n, 2, W, H, env.device)
        launch_cams(env, r.cams, W, H, q, t, views=views)
        torch.cuda.synchronize()
        return t

    for vw in (None, views):
        t0, t1 = draw(q, vw), draw(q, vw)
        tp = draw(q[perm].contiguous(), None if vw is None else vw[:, perm].contiguous())
        for k in SINKS:
            assert same_bits(t0[k], t1[k]), k
            assert same_bits(tp[k], t0[k][perm].contiguous()), k
        assert not torch.equal(t0["hwc"][0], t0["hwc"][1])


# ---------------------------------------------------------------------------------------------- 6. SO100VecEnv
KW = dict(obs_type=PIX, observation_width=64, observation_height=48, seed=3)
NAMES = ("top", "left_wrist")


def test_vec_env_cameras_change_nothing_else():
    a = SO100VecEnv(4, **KW)
    b = SO100VecEnv(4, cameras=NAMES, **KW)
    assert a.camera_names is None and b.camera_names == NAMES
    oa, _ = a.reset(seed=5)
    ob, _ = b.reset(seed=5)
    assert set(ob) == set(oa) and ob["pixels"].shape == (4, 2, 48, 64, 3) and ob["pixels"].dtype == torch.uint8
    g = torch.Generator().manual_seed(0)
    for _ in range(30):
        act = torch.rand(4, 6, generator=g) * 2 - 1
        oa, ra, ta, ua, ia = a.step(act)
        ob, rb, tb, ub, ib = b.step(act)
        for x, y in ((a.qpos, b.qpos), (a.qvel, b.qvel), (a.obs, b.obs), (ra, rb), (ta, tb), (ua, ub),
                     (oa["pixels"], ob["pixels"][:, 0]), (oa["agent_pos"], ob["agent_pos"])):
            assert torch.equal(x, y)
    assert int(ob["pixels"][:, 1].max()) > 0 and not torch.equal(ob["pixels"][:, 0], ob["pixels"][:, 1])
    c = SO100VecEnv(2, cameras=NAMES, channels_first=True, depth=True, segmentation=True, **KW)
    oc, _ = c.reset(seed=5)
    assert oc["pixels"].shape == (2, 2, 3, 48, 64) and oc["depth"].shape == oc["segmentation"].shape == (2, 2, 48, 64)
    assert torch.equal(oc["pixels"].permute(0, 1, 3, 4, 2), b.reset(seed=5)[0]["pixels"][:2])
    assert bool(((oc["depth"] == 0) == (oc["segmentation"] == R.SEG_BACKGROUND)).all())


def test_vec_env_terminal_images_show_the_terminal_state():
    a = SO100VecEnv(4, max_episode_steps=5, cameras=NAMES, depth=True, segmentation=True, **KW)
    twin = SO100VecEnv(4, autoreset=False, max_episode_steps=0, **KW)       # the same states, never reset
    a.reset(seed=5)
    twin.reset(seed=5)
    g = torch.Generator().manual_seed(1)
    for t in range(5):
        act = torch.rand(4, 6, generator=g) * 2 - 1
        ob, _, term, trunc, info = a.step(act)
        twin.step(act)
    done = term | trunc
    assert bool(done.all()) and torch.equal(info["_final_observation"], done)
    fin = info["final_observation"]
    assert set(fin) == {"pixels", "agent_pos", "depth", "segmentation"}
    assert fin["pixels"].shape == (4, 2, 48, 64, 3) and fin["depth"].shape == fin["segmentation"].shape == (4, 2, 48, 64)
    for c, name in enumerate(NAMES):                    # a direct render of the terminal qpos, camera by camera
        one = R.MultiCameraRenderer(twin, 64, 48, cameras=(name,), depth=True, segmentation=True)
        px = one.render(qpos=twin.qpos)
        torch.cuda.synchronize()
        assert torch.equal(fin["pixels"][:, c], px[:, 0]) and torch.equal(fin["segmentation"][:, c],
                                                                          one.segmentation[:, 0])
        assert same_bits(fin["depth"][:, c].contiguous(), one.depth[:, 0].contiguous())
    assert not torch.equal(ob["depth"], fin["depth"])                    # the new episode's images


def test_vec_env_flat_observation():
    e = SO100VecEnv(3, cameras=NAMES, flat_pixels=True, **KW)
    ob, _ = e.reset(seed=5)
    e.step(torch.zeros(3, 6))
    npx = 3 * 64 * 48
    assert e.pixels_flat.shape == (3, 2 * npx + 6)
    flat, pix = e.pixels_flat.cpu().numpy(), e.pixels.cpu().numpy()
    for c in range(2):
        want = pix[:, c].reshape(3, -1).astype(np.float32) / np.float32(255.0)
        assert np.array_equal(flat[:, c * npx:(c + 1) * npx].view(np.uint32), want.view(np.uint32)), c
    assert np.array_equal(flat[:, 2 * npx:], e.obs[:, 9:15].cpu().numpy())
    g = SO100VecEnv(2, task="so100_goal", cameras=NAMES, flat_pixels=True, **KW)
    og, _ = g.reset(seed=1)
    assert og["observation"] is g.pixels_flat and og["observation"].shape == (2, 2 * npx + 6)
    h = SO100VecEnv(2, task="so100_goal", cameras=NAMES, **KW)            # without the flag: built by torch per call
    oh, _ = h.reset(seed=1)
    assert oh["observation"].shape == (2, 2 * npx + 6)
    assert torch.equal((oh["observation"][:, :2 * npx] * 255).round().to(torch.uint8), g.pixels.reshape(2, -1))
    assert torch.equal(oh["observation"][:, 2 * npx:], og["observation"][:, 2 * npx:])


def test_vec_env_visual_records_per_camera_and_sharding():
    dr = dict(visual=dict(RANGES, seed=21))
    whole = SO100VecEnv(8, cameras=NAMES, domain_randomization=dr, **KW)
    v = whole.renderer.views
    assert v.shape == (2, 8, _native.VIEW_WORDS)
    # words 13.. are the headlight, lights and colours: the same base in both cameras, drawn from different seeds
    assert not torch.equal(v[0, :, 13:], v[1, :, 13:])
    single = SO100VecEnv(8, domain_randomization=dr, **KW)                # camera 0 draws CameraRenderer's records
    assert torch.equal(v[0], single.renderer.views)
    halves = [SO100VecEnv(4, cameras=NAMES, domain_randomization=dr, env_offset=o, **KW) for o in (0, 4)]
    assert torch.equal(torch.cat([h.renderer.views for h in halves], dim=1), v)
    whole.reset(seed=5)
    single.reset(seed=5)
    assert torch.equal(whole.pixels[:, 0], single.pixels)


# ------------------------------------------------------------------------------------------------ 7. the adapter
def test_sb3_adapter():
    from gym_so100.sb3 import SO100SB3VecEnv
    n, W, H, limit = 4, 32, 24, 3
    px = dict(obs_type=PIX, observation_width=W, observation_height=H)
    env = SO100SB3VecEnv(n, seed=3, max_episode_steps=limit, channels_first=True, cameras=NAMES, **px)
    ref = SO100VecEnv(n, seed=3, max_episode_steps=0, autoreset=False, channels_first=True, cameras=NAMES, **px)
    sp = env.observation_space
    assert sp["pixels"].shape == (6, H, W) and sp["pixels"].dtype == np.uint8 and sp["agent_pos"].shape == (6,)
    env.seed(7)
    obs = env.reset()
    r_obs, _ = ref.reset(seed=7)
    assert obs["pixels"].shape == (n, 6, H, W) and obs["pixels"].dtype == np.uint8
    np.testing.assert_array_equal(obs["pixels"], r_obs["pixels"].reshape(n, 6, H, W).cpu().numpy())
    rng = np.random.default_rng(0)
    for t in range(limit):
        prev, kept = obs, obs["pixels"].copy()
        a = rng.uniform(-1, 1, size=(n, 6)).astype(np.float32)
        obs, rew, dones, infos = env.step(a)
        r_obs, _, _, _, _ = ref.step(torch.from_numpy(a))
        r_pix = r_obs["pixels"].reshape(n, 6, H, W).cpu().numpy()
        # the host array is the device tensor; the one of the call before is still what it was (two pinned buffers)
        np.testing.assert_array_equal(obs["pixels"], env.venv.pixels.reshape(n, 6, H, W).cpu().numpy())
        np.testing.assert_array_equal(prev["pixels"], kept)
        assert not np.shares_memory(obs["pixels"], prev["pixels"])
        if t < limit - 1:
            assert not dones.any()
            np.testing.assert_array_equal(obs["pixels"], r_pix)
    assert dones.all()
    for i in range(n):
        term = infos[i]["terminal_observation"]
        assert set(term) == {"pixels", "agent_pos"} and term["pixels"].shape == (6, H, W)
        np.testing.assert_array_equal(term["pixels"], r_pix[i])
        np.testing.assert_array_equal(term["agent_pos"], r_obs["agent_pos"][i].cpu().numpy())
    assert np.stack(env.get_images()).shape == (n, H, W, 3)
    goal = SO100SB3VecEnv(2, task="so100_goal", cameras=NAMES, **px)
    assert goal.observation_space["observation"].shape == (2 * 3 * W * H + 6,)
    og = goal.reset()
    np.testing.assert_array_equal(og["observation"], goal.venv.pixels_flat.cpu().numpy())
    env.close()
    ref.close()
    goal.close()


# --------------------------------------------------------------------------------------------------- 8. refusals
def test_label_sink_needs_labels_and_views_need_materials():
    env = SO100VecEnv(2, autoreset=False, max_episode_steps=0)
    r = R.MultiCameraRenderer(env, 16, 12, cameras=NAMES)
    scene = R.load_scene()
    tri = np.ascontiguousarray(scene["tri"], dtype=np.float32)
    body = np.ascontiguousarray(scene["body"], dtype=np.int32)
    rgb = np.ascontiguousarray(scene["rgb"], dtype=np.float32)
    # a new mesh drops the labels and the materials of the one before
    _native.check(env.lib.so100_render_mesh(env._handle, tri.ctypes.data, body.ctypes.data, rgb.ctypes.data, len(body)),
                  "so100_render_mesh")
    t = sinks(2, 2, 16, 12, env.device)
    views = torch.zeros(2, 2, _native.VIEW_WORDS, dtype=torch.int32, device=env.device)
    with pytest.raises(RuntimeError, match=r"so100_render_cams: no labels \(so100_render_labels\)"):
        launch_cams(env, r.cams, 16, 12, env.qpos, t)
    with pytest.raises(RuntimeError, match=r"so100_render_cams: no materials \(so100_render_materials\)"):
        launch_cams(env, r.cams, 16, 12, env.qpos, {"depth": t["depth"]}, views=views)
    torch.cuda.synchronize()
    assert bool((t["depth"] == SENTF).all()) and bool((t["label"] == 77).all())     # refused before any device work
    launch_cams(env, r.cams, 16, 12, env.qpos, {"depth": t["depth"]})                # depth alone needs neither
    torch.cuda.synchronize()
    assert float(t["depth"].max()) > 0.1 and float(t["depth"].min()) >= 0.0
