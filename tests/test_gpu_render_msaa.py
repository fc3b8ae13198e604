"""Multisample anti-aliasing in the render launch (C-ABI so100_render_msaa, csrc/so100_render_msaa.hip; DESIGN.md 3.7
"Anti-aliasing").

1. one sample at the pixel centre is so100_render_cams, bit for bit, in every colour sink;
2. the ordered grid against the box mean of the so100_render_cams image at twice the size (the image does not depend on
   the banding);
3. the default patterns against the float64 restatement (tests/render_msaa_ref.py);
4. sinks, masks, nothing written outside, refusals that involve an env;
5. determinism and env independence;
6. through SO100VecEnv(antialias=...) and SO100SB3VecEnv(antialias=...)."""
import ctypes

import numpy as np
import pytest
import torch

import render_aux_ref as A
import render_cams_ref as C
import render_msaa_ref as M
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R
from gym_so100.sb3 import SO100SB3VecEnv

pytestmark = pytest.mark.gpu
PIX = "so100_pixels_agent_pos"
RANGES = dict(camera_pos=0.03, camera_rot_deg=float(np.degrees(0.05)), fovy=(0.9, 1.1), ambient=(0.6, 1.4),
              headlight=(0.6, 1.4), lights=(0.6, 1.4), light_rot_deg=float(np.degrees(0.17)), colors=(0.6, 1.2))
SENT8, SENTF, PAD = 0xA5, -7.0, 8
KEYS = ("hwc", "chw", "flat")
SHARE_CAP = 0.01                 # differing pixels per image
_ENVS, _STATES = {}, {}


def state_env(n):
    """n state-mode envs that only lend their handle to renderers (never stepped); built once per n."""
    if n not in _ENVS:
        _ENVS[n] = SO100VecEnv(n, autoreset=False, max_episode_steps=0)
    return _ENVS[n]


def states(n, dev):
    """float32 [n, 13] on dev: the first n of 8 envs' states after a 25-step random rollout, which runs once."""
    if "q" not in _STATES:
        env = SO100VecEnv(8, seed=4, autoreset=False)
        env.reset(seed=4)
        rng = np.random.default_rng(1)
        for _ in range(25):
            env.step(torch.from_numpy(rng.uniform(-1, 1, size=(8, 6)).astype(np.float32)).to(env.device))
        torch.cuda.synchronize()
        _STATES["q"] = env.qpos.clone().cpu()
        env.close()
    return _STATES["q"][:n].clone().to(dev)


def sinks(n, K, W, H, dev, off=0):
    """The three colour sinks of n envs x K cameras as slices, at element offset `off`, of sentinel-filled buffers with
    PAD elements to spare; flat has 3 floats more per env than the launch fills.  Returns (views, buffers)."""
    px = n * K * H * W
    shape = {"hwc": (n, K, H, W, 3), "chw": (n, K, 3, H, W), "flat": (n, K * 3 * W * H + 3)}
    size = {"hwc": 3 * px, "chw": 3 * px, "flat": n * (K * 3 * W * H + 3)}
    buf = {k: torch.full((size[k] + PAD,), SENTF if k == "flat" else SENT8,
                         dtype=torch.float32 if k == "flat" else torch.uint8, device=dev) for k in KEYS}
    return {k: buf[k][off:off + size[k]].view(shape[k]) for k in KEYS}, buf


def padding_intact(buf, t, off):
    for k in KEYS:
        s = SENTF if k == "flat" else SENT8
        if not (bool((buf[k][:off] == s).all()) and bool((buf[k][off + t[k].numel():] == s).all())):
            return False
    return bool((t["flat"][:, -3:] == SENTF).all())


def image_out(t):
    return _native.SO100ImageOut(hwc=_native.ptr(t.get("hwc")), chw=_native.ptr(t.get("chw")),
                                 flat=_native.ptr(t.get("flat")), flat_pitch=t["flat"].shape[1] if "flat" in t else 0)


def launch_cams(env, cams, W, H, q, t, views=None, mask=None):
    out, aux = image_out(t), _native.SO100AuxOut()
    _native.check(env.lib.so100_render_cams(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cams),
                                            _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(aux),
                                            env._stream()), "so100_render_cams")


def launch_msaa(env, cams, W, H, q, t, ms, views=None, mask=None):
    out = image_out(t)
    return env.lib.so100_render_msaa(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cams),
                                     _native.ptr(views), W, H, ctypes.byref(out), ctypes.byref(ms), env._stream())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def sinks_agree(t):
    """chw and flat hold hwc's bytes: what is violated, as text"""
    n, K, H, W, _ = t["hwc"].shape
    bad = []
    if not torch.equal(t["chw"], t["hwc"].permute(0, 1, 4, 2, 3)):
        bad.append("chw")
    npx = K * 3 * H * W
    unit = t["hwc"].cpu().numpy().reshape(n, npx).astype(np.float32) / np.float32(255)     # numpy's float32 division
    if not np.array_equal(t["flat"][:, :npx].cpu().numpy().view(np.uint32), unit.view(np.uint32)):
        bad.append("flat")
    return bad


def box_mean(img):
    """uint8 [..., 2H, 2W, 3] device tensor -> the round-half-up mean of every 2 x 2 block, uint8 [..., H, W, 3]"""
    *lead, h2, w2, _ = img.shape
    s = img.to(torch.int32).reshape(*lead, h2 // 2, 2, w2 // 2, 2, 3).sum(dim=(-4, -2))
    return ((s + 2) // 4).to(torch.uint8)


def diff_share(a, b):
    """share of differing pixels per image of two uint8 [..., H, W, 3] arrays -> [...]"""
    a, b = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (a, b))
    return np.any(a != b, axis=-1).mean(axis=(-2, -1))


# ------------------------------------------------------------------------- 1. one centre sample is the cams launch
@pytest.mark.parametrize("names", [("top",), ("front_close",), ("top", "left_wrist")])
@pytest.mark.parametrize("W,H", [(37, 29), (96, 72)])
def test_one_centre_sample_is_the_cams_launch_bit_for_bit(W, H, names):
    n, K = 6, len(names)
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=names)
    q = states(n, env.device)
    ident = r.identity_views().clone()
    sampled = r.sample_views(RANGES, 9).clone()
    r.views = None
    one = R.make_antialias(1)
    for what, views in (("no views", None), ("identity", ident), ("sampled", sampled)):
        t, buf = sinks(n, K, W, H, env.device, 1)
        a, _ = sinks(n, K, W, H, env.device)
        assert launch_msaa(env, r.cams, W, H, q, t, one, views=views) == 0
        launch_cams(env, r.cams, W, H, q, a, views=views)
        torch.cuda.synchronize()
        for k in KEYS:
            assert same_bits(t[k], a[k]), (what, k)
        assert padding_intact(buf, t, 1) and int(t["hwc"].max()) > 0, what


# ----------------------------------------------------------------------------------------------- 2. ordered grid
@pytest.mark.parametrize("names", [("top",), ("top", "left_wrist")])
@pytest.mark.parametrize("W,H", [(64, 48), (96, 72), (37, 29)])
def test_ordered_grid_is_the_box_mean_of_the_cams_image_at_twice_the_size(W, H, names):
    """64x48 x 4 samples is three bands, the 128x96 cams image three bands of other rows; the two launches also send
    their triangles to different phases.  0 differing pixels expected; the cap allows for a last bit of a depth."""
    n, K = 6, len(names)
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=names)
    q = states(n, env.device)
    t, _ = sinks(n, K, W, H, env.device)
    hi, _ = sinks(n, K, 2 * W, 2 * H, env.device)
    assert launch_msaa(env, r.cams, W, H, q, t, R.make_antialias(4, M.ORDERED4)) == 0
    launch_cams(env, r.cams, 2 * W, 2 * H, q, hi)
    torch.cuda.synchronize()
    want = box_mean(hi["hwc"])
    count = np.any(t["hwc"].cpu().numpy() != want.cpu().numpy(), axis=-1).sum(axis=(-2, -1))
    print(f"{W}x{H} {names}: differing pixels per (env, camera) {count.tolist()}")
    assert float(diff_share(t["hwc"], want).max()) <= SHARE_CAP
    assert sinks_agree(t) == []


# ------------------------------------------------------------------ 3. default patterns against float64
@pytest.mark.parametrize("S", [4, 2])
def test_default_pattern_matches_the_float64_restatement(model, oracle64, S):
    pattern = R.AA_PATTERNS[S]
    worst = 0.0
    for name, W, H, qpos, imgs in M.reference(model, oracle64, 64, pattern):
        n = len(qpos)
        env = state_env(n)
        q = torch.from_numpy(qpos).to(env.device)
        r = R.MultiCameraRenderer(env, W, H, cameras=(name,), antialias=S)
        got = r.render(qpos=q)[:, 0].clone()
        plain = R.MultiCameraRenderer(env, W, H, cameras=(name,)).render(qpos=q)[:, 0].clone()
        torch.cuda.synchronize()
        share = diff_share(got, np.stack(imgs))
        moved = diff_share(got, plain)
        print(f"S={S} {name} {W}x{H}: differs from float64 in {share.round(4).tolist()} of the pixels, from the "
              f"one-sample image in {moved.round(4).tolist()}")
        worst = max(worst, float(share.max()))
        if S == 4:
            assert float(moved.min()) > 0.02, name
    # the wrist camera, mounted on Fixed_Jaw
    ref = M.reference_wrist(model, oracle64, pattern)
    n = len(ref)
    env = state_env(n)
    q = torch.from_numpy(C.states()[:n]).to(env.device)
    got = R.MultiCameraRenderer(env, C.W, C.H, cameras=("left_wrist",), antialias=S).render(qpos=q)[:, 0].clone()
    torch.cuda.synchronize()
    share = diff_share(got, np.stack(ref))
    print(f"S={S} left_wrist {C.W}x{C.H}: differs from float64 in {share.round(4).tolist()} of the pixels")
    assert max(worst, float(share.max())) <= SHARE_CAP


# ------------------------------------------------------------------------------------------------------ 4. sinks
@pytest.mark.parametrize("W,H", [(37, 29), (99, 45), (1024, 2)])
def test_sinks_at_odd_offsets_under_a_mask(W, H):
    """1024 x 2 at 4 samples: a band is exactly one row.  K = 2, envs 1 and 3 masked out."""
    n, K = 4, 2
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top", "left_wrist"))
    q = states(n, env.device)
    ms = R.make_antialias(4)
    full, _ = sinks(n, K, W, H, env.device)
    assert launch_msaa(env, r.cams, W, H, q, full, ms) == 0
    mask = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=env.device)
    for off in (0, 1, 3):
        t, buf = sinks(n, K, W, H, env.device, off)
        assert launch_msaa(env, r.cams, W, H, q, t, ms, mask=mask) == 0
        torch.cuda.synchronize()
        for k in KEYS:
            s = SENTF if k == "flat" else SENT8
            assert bool((t[k][1] == s).all()) and bool((t[k][3] == s).all()), (off, k)
            if k == "flat":
                assert same_bits(t[k][0, :-3], full[k][0, :-3]) and same_bits(t[k][2, :-3], full[k][2, :-3]), off
            else:
                assert torch.equal(t[k][0], full[k][0]) and torch.equal(t[k][2], full[k][2]), (off, k)
        assert padding_intact(buf, t, off), off
    assert sinks_agree(full) == [] and int(full["hwc"].max()) > 0
    # each sink alone holds the same bytes
    for k in KEYS:
        alone, _ = sinks(n, K, W, H, env.device)
        assert launch_msaa(env, r.cams, W, H, q, {k: alone[k]}, ms) == 0
        torch.cuda.synchronize()
        assert same_bits(alone[k], full[k]), k


def test_refusals_with_an_env_leave_the_sinks_untouched():
    n, K, W, H = 4, 1, 16, 12
    env = state_env(n)
    r = R.MultiCameraRenderer(env, W, H, cameras=("top",))
    q = states(n, env.device)
    t, buf = sinks(n, K, W, H, env.device)

    def refused(rc):
        return rc != 0 and env.lib.so100_last_error().decode()
    msg = refused(launch_msaa(env, r.cams, W, H, None, t, R.make_antialias()))
    assert msg and "bad arguments" in msg
    cams = _native.SO100Cams(r.cameras, r.frame_body)
    cams.cam[0].fovy = 0.0
    msg = refused(launch_msaa(env, cams, W, H, q, t, R.make_antialias()))
    assert msg and "bad camera 0" in msg
    for s in (3, 8):
        msg = refused(launch_msaa(env, r.cams, W, H, q, t, _native.SO100Msaa(s, M.ROTATED4)))
        assert msg and "samples" in msg
    msg = refused(launch_msaa(env, r.cams, W, H, q, t, _native.SO100Msaa(2, ((0.0, 0.5), (0.0, 0.0)))))
    assert msg and "offset[0][1]" in msg
    fresh = SO100VecEnv(n, autoreset=False, max_episode_steps=0)          # no mesh uploaded
    rc = launch_msaa(fresh, r.cams, W, H, q, t, R.make_antialias())
    assert rc != 0 and "no render mesh" in fresh.lib.so100_last_error().decode()
    fresh.close()
    torch.cuda.synchronize()
    assert all(bool((buf[k] == (SENTF if k == "flat" else SENT8)).all()) for k in KEYS)      # no launch happened
    with pytest.raises(ValueError):
        R.CameraRenderer(env, W, H, antialias=True, shadows=True)


# -------------------------------------------------------------------------- 5. determinism and independence
def test_determinism_env_independence_and_permutation():
    W, H, names = 64, 48, ("top", "left_wrist")
    K = len(names)
    e4, e8 = state_env(4), state_env(8)
    r4 = R.MultiCameraRenderer(e4, W, H, cameras=names)
    r8 = R.MultiCameraRenderer(e8, W, H, cameras=names)
    q4, q8 = states(4, e4.device), states(8, e8.device)
    ms = R.make_antialias(4)
    a, _ = sinks(4, K, W, H, e4.device)
    b, _ = sinks(4, K, W, H, e4.device)
    c, _ = sinks(8, K, W, H, e8.device)
    assert launch_msaa(e4, r4.cams, W, H, q4, a, ms) == 0
    assert launch_msaa(e4, r4.cams, W, H, q4, b, ms) == 0
    assert launch_msaa(e8, r8.cams, W, H, q8, c, ms) == 0
    torch.cuda.synchronize()
    for k in KEYS:
        assert same_bits(a[k], b[k]), k                                # two launches
        assert same_bits(a[k], c[k][:4].contiguous()), k               # 4 envs are the first 4 of 8
    # permuted states and records give permuted images
    views = r8.sample_views(RANGES, 5).clone()
    r8.views = None
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=e8.device)
    d, _ = sinks(8, K, W, H, e8.device)
    e, _ = sinks(8, K, W, H, e8.device)
    assert launch_msaa(e8, r8.cams, W, H, q8, d, ms, views=views) == 0
    assert launch_msaa(e8, r8.cams, W, H, q8[perm].contiguous(), e, ms, views=views[:, perm].contiguous()) == 0
    torch.cuda.synchronize()
    for k in KEYS:
        assert same_bits(e[k], d[k][perm].contiguous()), k
    assert not torch.equal(d["hwc"], c["hwc"])                         # the records were used


# ------------------------------------------------------------------------------------------------------ 6. envs
@pytest.mark.parametrize("cameras", [None, ("top", "left_wrist")])
def test_vec_env_with_antialias(cameras):
    n, W, H, limit = 4, 64, 48, 5
    kw = dict(obs_type=PIX, observation_width=W, observation_height=H, seed=11, max_episode_steps=limit,
              depth=True, segmentation=True, cameras=cameras)
    on, off = SO100VecEnv(n, antialias=True, **kw), SO100VecEnv(n, **kw)
    twin = SO100VecEnv(n, seed=11, max_episode_steps=limit, autoreset=False)      # the terminal states
    assert on.renderer.antialias is not None and on.renderer.antialias.samples == 4 and off.renderer.antialias is None
    names = ("top",) if cameras is None else cameras
    K = len(names)
    direct = R.MultiCameraRenderer(state_env(n), W, H, cameras=names)
    o1, _ = on.reset(seed=11)
    o0, _ = off.reset(seed=11)
    twin.reset(seed=11)
    torch.cuda.synchronize()
    assert same_bits(o1["depth"], o0["depth"]) and torch.equal(o1["segmentation"], o0["segmentation"])
    assert not torch.equal(o1["pixels"], o0["pixels"])
    rng = np.random.default_rng(2)
    for step in range(20):
        a = torch.from_numpy(rng.uniform(-1, 1, size=(n, 6)).astype(np.float32)).to(on.device)
        o1, r1, t1, u1, i1 = on.step(a)
        o0, r0, t0, u0, i0 = off.step(a)
        if step < limit:
            twin.step(a)
        torch.cuda.synchronize()
        assert same_bits(o1["agent_pos"], o0["agent_pos"]) and same_bits(r1, r0)
        assert torch.equal(t1, t0) and torch.equal(u1, u0) and same_bits(on.qpos, off.qpos)
        assert same_bits(o1["depth"], o0["depth"]) and torch.equal(o1["segmentation"], o0["segmentation"])
        t, _ = sinks(n, K, W, H, on.device)
        assert launch_msaa(state_env(n), direct.cams, W, H, on.qpos, t, R.make_antialias(4)) == 0
        torch.cuda.synchronize()
        assert torch.equal(t["hwc"].view(o1["pixels"].shape), o1["pixels"])
        if step == limit - 1:
            # every env's episode ends here: final_pixels is the anti-aliased image of the terminal state
            assert bool(u1.all()) and same_bits(i1["final_observation"]["agent_pos"], twin.obs[:, 9:15])
            assert launch_msaa(state_env(n), direct.cams, W, H, twin.qpos, t, R.make_antialias(4)) == 0
            torch.cuda.synchronize()
            f1, f0 = i1["final_observation"], i0["final_observation"]
            assert torch.equal(f1["pixels"], t["hwc"].view(f1["pixels"].shape))
            assert same_bits(f1["depth"], f0["depth"]) and torch.equal(f1["segmentation"], f0["segmentation"])
    for e in (on, off, twin):
        e.close()


def test_camera_renderer_is_the_k1_launch():
    n, W, H = 4, 37, 29
    env = state_env(n)
    q = states(n, env.device)
    r = R.CameraRenderer(env, W, H, channels_first=True, antialias=2, depth=True)
    flat = torch.full((n, 3 * W * H + 6), SENTF, device=env.device)
    img = r.render(qpos=q, flat=flat)
    plain = R.CameraRenderer(env, W, H, depth=True)
    plain.render(qpos=q)
    t, _ = sinks(n, 1, W, H, env.device)
    assert launch_msaa(env, _native.SO100Cams([r.camera], [0]), W, H, q, t, R.make_antialias(2)) == 0
    torch.cuda.synchronize()
    assert torch.equal(img, t["chw"][:, 0]) and same_bits(flat[:, :3 * W * H], t["flat"][:, :3 * W * H])
    assert bool((flat[:, 3 * W * H:] == SENTF).all()) and same_bits(r.depth, plain.depth)


@pytest.mark.parametrize("channels_first,cameras", [(False, None), (True, None), (True, ("top", "left_wrist"))])
def test_sb3_forwards_antialias(channels_first, cameras):
    n, W, H = 2, 32, 24
    kw = dict(seed=3, obs_type=PIX, observation_width=W, observation_height=H, channels_first=channels_first,
              cameras=cameras)
    on, off = SO100SB3VecEnv(n, antialias=True, **kw), SO100SB3VecEnv(n, **kw)
    assert on.venv.renderer.antialias is not None and off.venv.renderer.antialias is None
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
