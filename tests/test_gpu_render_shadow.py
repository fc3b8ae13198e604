"""Cast shadows in the render launch (C-ABI so100_render_shadow, csrc/so100_render_shadow.hip; DESIGN.md 3.7 "Shadows").

1. the contract, bit for bit: pixels == where(shadow, dark, full) with full / dark two so100_render_cams images (dark:
   the casting light's diffuse 0), depth and labels the cams launch's, in every sink, nothing written outside;
2. the mask against the float64 reference (tests/render_shadow_ref.py), per image;
3. light = -1 is the cams launch;
4. masks, determinism, env independence, map sizes;
5. through SO100VecEnv(shadows=...) and SO100SB3VecEnv(shadows=...)."""
import ctypes

import numpy as np
import pytest
import torch

import render_aux_ref as A
import render_ref
import render_shadow_ref as S
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R
from gym_so100.sb3 import SO100SB3VecEnv

pytestmark = pytest.mark.gpu
PIX = "so100_pixels_agent_pos"
RANGES = dict(camera_pos=0.03, camera_rot_deg=float(np.degrees(0.05)), fovy=(0.9, 1.1), ambient=(0.6, 1.4),
              headlight=(0.6, 1.4), lights=(0.6, 1.4), light_rot_deg=float(np.degrees(0.17)), colors=(0.6, 1.2))
SENT8, SENTF, PAD = 0xA5, -7.0, 8
KEYS = ("hwc", "chw", "flat", "depth", "label", "shadow")
LIFT = 3                     # the env of every state batch that holds the lifted-cube state
VIEW_DIFFUSE = 15            # so100_view: pos 3, mat 9, fovy, head_ambient, head_diffuse, then light_diffuse[4]
_ENVS, _STATES = {}, {}


def state_env(n):
    """n state-mode envs that only lend their handle to renderers (never stepped); built once per n."""
    if n not in _ENVS:
        _ENVS[n] = SO100VecEnv(n, autoreset=False, max_episode_steps=0)
    return _ENVS[n]


def states(n, dev):
    """float32 [n, 13] on dev: the first n of 8 envs' states after a 25-step random rollout, env LIFT replaced by the
    lifted-cube state (set through qpos, never stepped).  The rollout runs once."""
    if "q" not in _STATES:
        env = SO100VecEnv(8, seed=4, autoreset=False)
        env.reset(seed=4)
        rng = np.random.default_rng(1)
        for _ in range(25):
            env.step(torch.from_numpy(rng.uniform(-1, 1, size=(8, 6)).astype(np.float32)).to(env.device))
        q = env.qpos.clone()
        q[LIFT] = torch.from_numpy(S.LIFTED).to(q.device)
        torch.cuda.synchronize()
        _STATES["q"] = q.cpu()
        env.close()
    return _STATES["q"][:n].clone().to(dev)


def sinks(n, K, W, H, dev, off=0):
    """The six sinks of n envs x K cameras as slices, at element offset `off`, of sentinel-filled buffers with PAD
    elements to spare; flat has 3 floats more per env than the launch fills.  Returns (views, buffers)."""
    px = n * K * H * W
    shape = {"hwc": (n, K, H, W, 3), "chw": (n, K, 3, H, W), "flat": (n, K * 3 * W * H + 3), "depth": (n, K, H, W),
             "label": (n, K, H, W), "shadow": (n, K, H, W)}
    size = {"hwc": 3 * px, "chw": 3 * px, "flat": n * (K * 3 * W * H + 3), "depth": px, "label": px, "shadow": px}
    buf = {k: torch.full((size[k] + PAD,), SENTF if k in ("flat", "depth") else SENT8,
                         dtype=torch.float32 if k in ("flat", "depth") else torch.uint8, device=dev) for k in KEYS}
    return {k: buf[k][off:off + size[k]].view(shape[k]) for k in KEYS}, buf


def padding_intact(buf, t, off):
    for k in KEYS:
        s = SENTF if k in ("flat", "depth") else SENT8
        if not (bool((buf[k][:off] == s).all()) and bool((buf[k][off + t[k].numel():] == s).all())):
            return False
    return bool((t["flat"][:, -3:] == SENTF).all())


def structs(t):
    out = _native.SO100ImageOut(hwc=_native.ptr(t.get("hwc")), chw=_native.ptr(t.get("chw")),
                                flat=_native.ptr(t.get("flat")), flat_pitch=t["flat"].shape[1] if "flat" in t else 0)
    return out, _native.SO100AuxOut(depth=_native.ptr(t.get("depth")), label=_native.ptr(t.get("label")))


def launch_cams(env, cams, W, H, q, t, views=None, mask=None):
    out, aux = structs(t)
    _native.check(env.lib.so100_render_cams(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cams),
                                            _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux),
                                            env._stream()), "so100_render_cams")


def launch_shadow(env, cams, W, H, q, t, sh, views=None, mask=None):
    out, aux = structs(t)
    sh.shadow_out = _native.ptr(t.get("shadow"))
    return env.lib.so100_render_shadow(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cams),
                                       _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux), ctypes.byref(sh),
                                       env._stream())


def without_light(r, light, views):
    """(cams, views) of renderer r with `light`'s diffuse 0 in every camera and every record"""
    cams = _native.SO100Cams(r.cameras, r.frame_body)
    for c in range(r.ncam):
        cams.cam[c].light_diffuse[light] = 0.0
    if views is not None:
        views = views.clone()
        views.view(torch.float32)[..., VIEW_DIFFUSE + light] = 0.0
    return cams, views


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def contract_holds(env, r, q, sh, t, views=None):
    """t: the shadow launch's sinks.  Draws full and dark with so100_render_cams and returns what of the contract is
    violated, as text."""
    n, K, H, W = t["shadow"].shape
    full, _ = sinks(n, K, W, H, q.device)
    dark, _ = sinks(n, K, W, H, q.device)
    launch_cams(env, r.cams, W, H, q, full, views=views)
    dcams, dviews = without_light(r, sh.light, views)
    launch_cams(env, dcams, W, H, q, dark, views=dviews)
    torch.cuda.synchronize()
    m = t["shadow"].bool()
    bad = []
    if not torch.equal(t["hwc"], torch.where(m[..., None], dark["hwc"], full["hwc"])):
        bad.append("hwc")
    if not torch.equal(t["chw"], t["hwc"].permute(0, 1, 4, 2, 3)):
        bad.append("chw")
    npx = K * 3 * H * W
    unit = t["hwc"].cpu().numpy().reshape(n, npx).astype(np.float32) / np.float32(255)     # numpy's float32 division
    if not np.array_equal(t["flat"][:, :npx].cpu().numpy().view(np.uint32), unit.view(np.uint32)):
        bad.append("flat")
    for k in ("depth", "label"):
        if not same_bits(t[k], full[k]):
            bad.append(k)
    if int(t["shadow"].max()) > 1 or bool((m & (t["label"] == R.SEG_BACKGROUND)).any()):
        bad.append("shadow values")
    return bad


# ----------------------------------------------------------------------------------- 1. the contract, bit for bit
@pytest.mark.parametrize("W,H,names,sampled", [(64, 48, ("top",), False), (96, 72, ("top",), False),
                                               (37, 29, ("top", "left_wrist"), False), (64, 48, ("top",), True)])
def test_pixels_are_dark_where_shadowed_and_full_elsewhere(W, H, names, sampled):
    n, K = 6, len(names)
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=names, shadows=True)
    q = states(n, env.device)
    views = r.sample_views(RANGES, 9).clone() if sampled else None
    r.views = None
    for off in (0, 1, 3):
        t, buf = sinks(n, K, W, H, env.device, off)
        assert launch_shadow(env, r.cams, W, H, q, t, r.shadows, views=views) == 0
        torch.cuda.synchronize()
        assert contract_holds(env, r, q, r.shadows, t, views=views) == [], (off,)
        assert padding_intact(buf, t, off), off
        share = t["shadow"].float().mean(dim=(2, 3))
        print(f"{W}x{H} {names} offset {off}: shadowed share per (env, camera) {share.cpu().numpy().round(4).tolist()}")
        assert int(t["shadow"][:, 0].sum()) > 0 and int(t["hwc"].max()) > 0
    # the renderer's own call is the same launch
    r2 = R.MultiCameraRenderer(env, W, H, cameras=names, shadows=True, shadow_mask=True, depth=True, segmentation=True)
    img = r2.render(qpos=q, views=views)
    torch.cuda.synchronize()
    assert torch.equal(img, t["hwc"]) and torch.equal(r2.shadow, t["shadow"]) and same_bits(r2.depth, t["depth"])


# ------------------------------------------------------------------- 2. the mask against the float64 reference
@pytest.mark.parametrize("W,H", [(64, 48), (96, 72)])
def test_mask_matches_the_float64_reference(model, oracle64, W, H):
    n = 4
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top",), shadows=True, shadow_mask=True, segmentation=True)
    q = states(n, env.device)
    r.render(qpos=q)
    torch.cuda.synchronize()
    mask, lab = r.shadow[:, 0].cpu().numpy().astype(bool), r.segmentation[:, 0].cpu().numpy()
    scene = R.load_scene()
    labels, _ = R.segment_labels(scene)
    cast, sh = R.shadow_casters(scene), S.shadow_dict(r.shadows)
    cam = render_ref.camera_dict(r.cameras[0])
    frame = S.light_frame(cam["light_dir"][sh["light"]], np.float64)
    bar = 2.0 * S.MASK_F32_FLOOR * W * H + 2.0
    bad = []
    for i in range(n):
        fr, ee = A.frames_of(oracle64, model, q[i].cpu().numpy().astype(np.float64))
        _, dep0, lab0 = A.render(scene["tri"], scene["body"], scene["rgb"], labels, fr, cam, W, H, target=ee)
        smap = S.shadow_map(scene["tri"], scene["body"], cast, fr, frame, sh["center"], sh["radius"], sh["map_size"])
        m0 = S.shadow_mask(dep0, lab0, cam, W, H, smap, frame, sh["center"], sh["radius"], sh["bias"], target=ee)
        same = lab[i] == lab0
        excluded, diff = float((~same).mean()), int(((mask[i] != m0) & same).sum())
        print(f"{W}x{H} env {i}: reference shadowed share {m0.mean():.4f}, labels differ at {excluded:.4f} of the pixels, "
              f"the mask at {diff} pixels (bar {bar:.1f})")
        assert m0.sum() >= 10.0 * bar                                  # enough shadow to judge the mask by
        if excluded > 0.01:
            bad.append(f"env {i}: excluded {excluded:.4f}")
        if diff > bar:
            bad.append(f"env {i}: {diff} pixels differ")
    assert bad == []
    assert int((mask[LIFT] & (lab[LIFT] == 0)).sum()) > 0            # the lifted cube's shadow lies on the table


# ------------------------------------------------------------------------------------------------ 3. light = -1
def test_no_casting_light_is_the_cams_launch():
    n, K, W, H = 4, 2, 37, 29
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top", "left_wrist"), shadows={"light": -1})
    q = states(n, env.device)
    t, buf = sinks(n, K, W, H, env.device, 1)
    a, _ = sinks(n, K, W, H, env.device)
    assert launch_shadow(env, r.cams, W, H, q, t, r.shadows) == 0
    launch_cams(env, r.cams, W, H, q, a)
    torch.cuda.synchronize()
    for k in ("hwc", "chw", "flat", "depth", "label"):
        assert same_bits(t[k], a[k]), k
    assert int(t["shadow"].max()) == 0 and padding_intact(buf, t, 1)


# ------------------------------------------------------------------------------------ 4. other kernel behaviour
def test_mask_determinism_independence_and_map_sizes():
    W, H = 64, 48
    e4, e8 = state_env(4), state_env(8)
    r4 = R.MultiCameraRenderer(e4, W, H, cameras=("top",), shadows=True)
    r8 = R.MultiCameraRenderer(e8, W, H, cameras=("top",), shadows=True)
    q4, q8 = states(4, e4.device), states(8, e8.device)
    a, _ = sinks(4, 1, W, H, e4.device)
    b, _ = sinks(4, 1, W, H, e4.device)
    c, _ = sinks(8, 1, W, H, e8.device)
    assert launch_shadow(e4, r4.cams, W, H, q4, a, r4.shadows) == 0
    assert launch_shadow(e4, r4.cams, W, H, q4, b, r4.shadows) == 0
    assert launch_shadow(e8, r8.cams, W, H, q8, c, r8.shadows) == 0
    torch.cuda.synchronize()
    for k in KEYS:
        assert same_bits(a[k], b[k]), k                                # two launches
        assert same_bits(a[k], c[k][:4].contiguous()), k               # 4 envs are the first 4 of 8
    # a masked-out env is untouched in every sink
    m, buf = sinks(4, 1, W, H, e4.device, 1)
    mask = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=e4.device)
    assert launch_shadow(e4, r4.cams, W, H, q4, m, r4.shadows, mask=mask) == 0
    torch.cuda.synchronize()
    for k in KEYS:
        s = SENTF if k in ("flat", "depth") else SENT8
        assert bool((m[k][1] == s).all()) and bool((m[k][3] == s).all()), k
        assert same_bits(m[k][0], a[k][0]) and same_bits(m[k][2], a[k][2]), k
    assert padding_intact(buf, m, 1)
    # both map sizes run, agree on depth and labels and differ in the mask somewhere
    small = R.make_shadow(R.load_scene(), map_size=32)
    d, _ = sinks(4, 1, W, H, e4.device)
    assert launch_shadow(e4, r4.cams, W, H, q4, d, small) == 0
    torch.cuda.synchronize()
    assert same_bits(d["depth"], a["depth"]) and torch.equal(d["label"], a["label"])
    assert int(d["shadow"].sum()) > 0 and not torch.equal(d["shadow"], a["shadow"])
    assert contract_holds(e4, r4, q4, small, d) == []


def test_refusals_with_an_env():
    W, H = 16, 12
    env = state_env(4)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top",), shadows=True)
    q = states(4, env.device)
    t, buf = sinks(4, 1, W, H, env.device)
    scene = R.load_scene()

    def refused(sh, **kw):
        rc = launch_shadow(env, r.cams, kw.get("W", W), H, q, t, sh)
        return rc != 0 and env.lib.so100_last_error().decode()
    for field, value, text in (("light", 3, "light"), ("light", -2, "light"), ("map_size", 128, "map_size"),
                               ("map_size", 20, "map_size"), ("radius", 0.0, "radius"),
                               ("radius", float("inf"), "radius"), ("bias", -1.0, "bias"),
                               ("bias", float("nan"), "bias"), ("size", 44, "so100_shadow")):
        sh = R.make_shadow(scene)
        setattr(sh, field, value)
        msg = refused(sh)
        assert msg and text in msg, (field, value, msg)
    # casters belong to the mesh: a new mesh drops them, and the launch then refuses
    R.MultiCameraRenderer(env, W, H, cameras=("top",))
    msg = refused(R.make_shadow(scene))
    assert msg and "casters" in msg
    torch.cuda.synchronize()
    assert all(bool((buf[k] == (SENTF if k in ("flat", "depth") else SENT8)).all()) for k in KEYS)   # no launch happened
    with pytest.raises(ValueError):
        R.CameraRenderer(env, W, H, shadow_mask=True)


# ------------------------------------------------------------------------------------------------------ 5. envs
def test_vec_env_with_shadows():
    n, W, H, limit = 4, 64, 48, 5
    kw = dict(obs_type=PIX, observation_width=W, observation_height=H, seed=11, max_episode_steps=limit)
    on, off = SO100VecEnv(n, shadows=True, **kw), SO100VecEnv(n, **kw)
    twin = SO100VecEnv(n, seed=11, max_episode_steps=limit, autoreset=False)      # the terminal states
    assert on.renderer.shadows is not None and off.renderer.shadows is None
    o1, _ = on.reset(seed=11)
    o0, _ = off.reset(seed=11)
    twin.reset(seed=11)
    rng = np.random.default_rng(2)
    own = torch.empty_like(on.pixels)
    for step in range(20):
        a = torch.from_numpy(rng.uniform(-1, 1, size=(n, 6)).astype(np.float32)).to(on.device)
        o1, r1, t1, u1, i1 = on.step(a)
        o0, r0, t0, u0, i0 = off.step(a)
        if step < limit:
            twin.step(a)
        torch.cuda.synchronize()
        assert same_bits(o1["agent_pos"], o0["agent_pos"]) and same_bits(r1, r0)
        assert torch.equal(t1, t0) and torch.equal(u1, u0) and same_bits(on.qpos, off.qpos)
        on.renderer.render(qpos=on.qpos, out=own)
        torch.cuda.synchronize()
        assert torch.equal(own, o1["pixels"])
        if step == limit - 1:
            # every env's episode ends here: final_pixels is the shadowed image of the terminal state
            assert bool(u1.all()) and same_bits(i1["final_observation"]["agent_pos"], twin.obs[:, 9:15])
            r = R.MultiCameraRenderer(state_env(n), W, H, cameras=("top",), shadows=True)
            t, _ = sinks(n, 1, W, H, on.device)
            assert launch_shadow(state_env(n), r.cams, W, H, twin.qpos, t, r.shadows) == 0
            torch.cuda.synchronize()
            assert contract_holds(state_env(n), r, twin.qpos, r.shadows, t) == []
            assert torch.equal(i1["final_observation"]["pixels"], t["hwc"][:, 0]) and int(t["shadow"].sum()) > 0
    # the lifted cube: the two envs' images differ
    q = states(n, on.device)
    a, b = on.renderer.render(qpos=q).clone(), off.renderer.render(qpos=q).clone()
    torch.cuda.synchronize()
    assert not torch.equal(a[LIFT], b[LIFT])
    for e in (on, off, twin):
        e.close()


@pytest.mark.parametrize("channels_first,cameras", [(False, None), (True, None), (True, ("top", "left_wrist"))])
def test_sb3_forwards_shadows(channels_first, cameras):
    n, W, H = 2, 32, 24
    kw = dict(seed=3, obs_type=PIX, observation_width=W, observation_height=H, channels_first=channels_first,
              cameras=cameras)
    on, off = SO100SB3VecEnv(n, shadows=True, **kw), SO100SB3VecEnv(n, **kw)
    assert on.venv.renderer.shadows is not None and off.venv.renderer.shadows is None
    a, b = on.reset()["pixels"], off.reset()["pixels"]
    K = 1 if cameras is None else len(cameras)
    assert a.shape == ((n, 3 * K, H, W) if channels_first else (n, H, W, 3))
    assert np.array_equal(a, on.venv.pixels.cpu().numpy().reshape(a.shape)) and not np.array_equal(a, b)
    own = torch.empty_like(on.venv.pixels)
    on.venv.renderer.render(out=own)
    torch.cuda.synchronize()
    assert torch.equal(own, on.venv.pixels)
    obs, _, _, _ = on.step(np.zeros((n, 6), np.float32))
    assert obs["pixels"].shape == a.shape
    on.close()
    off.close()
