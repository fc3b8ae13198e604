"""Per-env views (C-ABI so100_render_views / so100_views_sample, csrc/so100_render_views.hip and so100_views.hip;
DESIGN.md 3.7): camera, lights and colours per env.

1. identity views draw what so100_render / so100_render_to draw, bit for bit, in every sink and under a mask;
2. random views against the numpy rasteriser (tests/render_ref.py) fed the GPU's own records read back;
3. per-env independence: records and states permuted give the permuted images;
4. the sampler against its float64 restatement (tests/views_ref.py), its ranges, sharding, mask and episode;
5. through SO100VecEnv: images only, fixed records, per-episode resampling and the terminal image;
6. through SO100SB3VecEnv;
7. the C-ABI's refusals (NULL views, a wrong triangle count or material id, no materials, a bad range) and the
   masked reset's resampling.

The states of test 2 are made on the CPU (start pose + uniform joint offsets, the reference's cube spawn) and handed to
the render launch, so its seed can be accepted on the CPU before any GPU step: a seed is taken only if, in the float64
reference alone, no visible face's val * 255 lies within 1e-3 of a half-integer (such a face may round to the other
level in float32: a whole face off by one, which the cap on differing pixels would hide) and no sampled colour channel
lies that near one either (the device's record then holds the same byte).  The search starts at a seed found that way
beforehand; the check itself runs every time."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import render_ref
import views_ref
from gym_so100 import SO100VecEnv, _native, constants, utils
from gym_so100 import render as R

pytestmark = pytest.mark.gpu
NBODY = 9
RANGES = dict(camera_pos=0.03, camera_rot_deg=float(np.degrees(0.05)), fovy=(0.9, 1.1), ambient=(0.6, 1.4),
              headlight=(0.6, 1.4), lights=(0.6, 1.4), light_rot_deg=float(np.degrees(0.17)), colors=(0.6, 1.2))
PIX = "so100_pixels_agent_pos"
SENTINEL = 0xA5


# ---------------------------------------------------------------------------------------------- CPU side
@functools.lru_cache(maxsize=None)
def scene_parts():
    scene = R.load_scene()
    material, base = R.material_ids(scene)
    return scene, material, np.ascontiguousarray(R.pack_rgb8(base), dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def cpu_model():
    from gym_so100.model import build_model
    from oracle.oracle import Oracle
    return build_model(), Oracle(64)


def frames_of(qpos):
    """(body frames, ee_site) of one state from the float64 oracle's forward kinematics."""
    m, o = cpu_model()
    d = o.new_data()
    o.reset(m, d, np.array(qpos[6:13], np.float64))
    for k in range(6):
        d.qpos[k] = float(qpos[k])
    o.call("so100o_fwd_position", m, d)
    return [(np.array(d.xmat[b][:]).reshape(3, 3), np.array(d.xpos[b][:])) for b in range(NBODY)], \
        np.array(d.site_ee[:])


def cpu_states(n, seed):
    """float32 [n, 13]: the start pose with joint offsets in +-0.3 rad and the reference's cube spawn (utils.py)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 13))
    q[:, :6] = np.array(constants.SO100_START_ARM_POSE) + rng.uniform(-0.3, 0.3, (n, 6))
    for i in range(n):
        q[i, 6:13] = utils.sample_box_pose(100 * seed + i)
    return q.astype(np.float32)


def accepted_seed(camera, n, W, H, start, stop=None):
    """The first seed >= start that the module docstring's rule accepts for cpu_states(n, W) under RANGES."""
    scene, material, base_rgb = scene_parts()
    cam = R.make_camera(scene, camera)
    q = cpu_states(n, W).astype(np.float64)
    fr = [frames_of(q[i]) for i in range(n)]
    seed = start
    while stop is None or seed < stop:
        rec = views_ref.sample(R.view_ranges(RANGES, seed), cam, base_rgb, np.arange(n))
        lev = rec["rgb_level"]
        ok = not np.any(np.abs(lev - np.floor(lev) - 0.5) < 1e-3)
        if ok:
            for k in ("pos", "mat", "fovy", "head_ambient", "head_diffuse", "light_diffuse", "light_dir"):
                rec[k] = rec[k].astype(np.float32).astype(np.float64)          # as the device holds them
            for i in range(n):
                vis, near = views_ref.faces_near_rounding(scene, material, rec, i, cam, fr[i][0], fr[i][1], W, H)
                assert vis > 20
                if near:
                    ok = False
                    break
        if ok:
            return seed
        seed += 1
    return None


# ---------------------------------------------------------------------------------------------- GPU side
_ROLLED = {}


def rolled(n):
    """n pixel envs after reset and a 10-step random rollout; never auto-reset.  Built once and left unchanged."""
    if n not in _ROLLED:
        env = SO100VecEnv(n, obs_type=PIX, observation_width=37, observation_height=29, autoreset=False,
                          max_episode_steps=0)
        g = torch.Generator().manual_seed(n)
        env.reset(seed=70 + n)
        for _ in range(10):
            env.step(torch.rand(n, 6, generator=g) * 2 - 1)
        torch.cuda.synchronize()
        _ROLLED[n] = env
    return _ROLLED[n]


def sinks_of(kind, n, W, H, dev):
    """sentinel-filled sink tensors of a launch: dict name -> tensor, and the flat pitch"""
    npix = 3 * W * H
    t = {}
    if kind in ("hwc", "hwc+flat"):
        t["hwc"] = torch.full((n, H, W, 3), SENTINEL, dtype=torch.uint8, device=dev)
    if kind == "chw":
        t["chw"] = torch.full((n, 3, H, W), SENTINEL, dtype=torch.uint8, device=dev)
    if kind == "hwc+flat":
        t["flat"] = torch.full((n, npix + 3), -7.0, dtype=torch.float32, device=dev)
    return t, npix + 3 if "flat" in t else 0


def launch(env, cam, W, H, t, pitch, views=None, mask=None, qpos=None):
    out = _native.SO100ImageOut(hwc=_native.ptr(t.get("hwc")), chw=_native.ptr(t.get("chw")),
                                flat=_native.ptr(t.get("flat")), flat_pitch=pitch)
    q = env.qpos if qpos is None else qpos
    if views is None:
        rc = env.lib.so100_render_to(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cam), W, H,
                                     ctypes.byref(out), env._stream())
    else:
        rc = env.lib.so100_render_views(env._handle, _native.ptr(q), _native.ptr(mask), ctypes.byref(cam),
                                        _native.ptr(views), W, H, ctypes.byref(out), env._stream())
    torch.cuda.synchronize()
    assert rc == 0, env.lib.so100_last_error()


def same_bits(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("kind", ["hwc", "chw", "hwc+flat"])
@pytest.mark.parametrize("camera", ["top", "front_close"])
@pytest.mark.parametrize("W,H", [(37, 29), (96, 72)])
def test_identity_views_equal_the_old_kernels(W, H, camera, kind):
    n = 5
    env = rolled(n)
    r = R.CameraRenderer(env, W, H, camera=camera)
    views = r.identity_views()
    old, pitch = sinks_of(kind, n, W, H, env.device)
    new, _ = sinks_of(kind, n, W, H, env.device)
    launch(env, r.camera, W, H, old, pitch)
    launch(env, r.camera, W, H, new, pitch, views=views)
    if kind == "hwc":                                   # so100_render itself
        r.views = None
        assert torch.equal(old["hwc"], r.render())
    for k in old:
        assert bool((old[k].view(torch.uint8) != SENTINEL).any()), k
        assert same_bits(new[k], old[k]), k
    # masked launch into sentinel-filled sinks
    on = [1, 0, 1, 1, 0]
    mask = torch.tensor(on, dtype=torch.uint8, device=env.device)
    got, _ = sinks_of(kind, n, W, H, env.device)
    fresh, _ = sinks_of(kind, n, W, H, env.device)
    launch(env, r.camera, W, H, got, pitch, views=views, mask=mask)
    for k in got:
        for i in range(n):
            assert same_bits(got[k][i], (old if on[i] else fresh)[k][i]), (k, i)


SHAPES = [("top", 6, 96, 72, 15), ("front_close", 3, 64, 48, 0), ("top", 2, 640, 480, 81)]


@pytest.mark.parametrize("camera,n,W,H,start", SHAPES)
def test_random_views_match_numpy_rasteriser(camera, n, W, H, start):
    seed = accepted_seed(camera, n, W, H, start)                   # on the CPU, before any GPU step
    print(f"{camera} {n} x {W}x{H}: seed {seed}")
    scene, material, _ = scene_parts()
    q = cpu_states(n, W)
    env = SO100VecEnv(n, obs_type=PIX, observation_width=W, observation_height=H, autoreset=False,
                      max_episode_steps=0)
    r = R.CameraRenderer(env, W, H, camera=camera)
    qd = torch.from_numpy(q).to(env.device)
    plain = r.render(qpos=qd).clone()
    views = r.sample_views(RANGES, seed)
    img = r.render(qpos=qd).cpu().numpy()
    torch.cuda.synchronize()
    plain = plain.cpu().numpy()
    rec = views_ref.decode(views.cpu().numpy())
    worst = 0.0
    for i in range(n):
        fr, ee = frames_of(q[i].astype(np.float64))
        ref = render_ref.render(scene["tri"], scene["body"], views_ref.triangle_rgb(rec, i, material), fr,
                                views_ref.camera_dict(rec, i, r.camera), W, H, target=ee)
        share = np.any(img[i] != ref, axis=-1).mean()
        moved = np.any(img[i] != plain[i], axis=-1).mean()
        print(f"env {i}: differing pixels {share:.4f} of the image; against the unrandomised image {moved:.4f}")
        worst = max(worst, share)
        assert share < 0.01, (i, share)
        assert moved > 0.10, (i, moved)
    print(f"worst share of differing pixels {worst:.4f}")


def test_records_and_states_permuted_give_permuted_images():
    n, W, H = 6, 96, 72
    env = rolled(n)
    r = R.CameraRenderer(env, W, H)
    views = r.sample_views(RANGES, 11)
    a = r.render().clone()
    perm = torch.tensor([3, 0, 5, 1, 4, 2], device=env.device)
    b = r.render(qpos=env.qpos[perm].contiguous(), out=torch.zeros_like(a), views=views[perm].contiguous())
    torch.cuda.synchronize()
    assert not torch.equal(a[0], a[1])
    assert torch.equal(b, a[perm])


def test_sampler_matches_the_float64_restatement():
    n, off, seed = 64, 1000, 12345
    _, _, base_rgb = scene_parts()
    env = SO100VecEnv(n, obs_type=PIX, observation_width=16, observation_height=12, env_offset=off)
    r = env.renderer
    ep = torch.arange(n, dtype=torch.int32, device=env.device) % 5
    got = views_ref.decode(r.sample_views(RANGES, seed, episode=ep).cpu().numpy())
    dr = R.view_ranges(RANGES, seed)
    ref = views_ref.sample(dr, r.camera, base_rgb, off + np.arange(n), ep.cpu().numpy())
    worst = {}
    for k in ("mat", "light_dir"):                      # entries of magnitude <= 1: absolute
        nl = r.camera.nlight
        g, w = (got[k][:, :nl], ref[k][:, :nl]) if k == "light_dir" else (got[k], ref[k])
        worst[k] = np.abs(g - w).max()
        assert worst[k] <= 2e-6, (k, worst[k])
    for k in ("pos", "fovy", "head_ambient", "head_diffuse", "light_diffuse"):
        nl = r.camera.nlight
        g, w = (got[k][:, :nl], ref[k][:, :nl]) if k == "light_diffuse" else (got[k], ref[k])
        nz = w != 0
        assert np.array_equal(g[~nz], w[~nz])
        worst[k] = np.abs(g[nz] / w[nz] - 1.0).max()
        assert worst[k] <= 2e-6, (k, worst[k])
    chan = lambda x: np.stack([(x >> (8 * c)) & 0xFF for c in range(3)], axis=-1).astype(np.int64)
    dc = np.abs(chan(got["rgb"]) - chan(ref["rgb"]))
    print("sampler maxima against float64:", {k: float(f"{v:.3g}") for k, v in worst.items()},
          f"colour channels exact {int((dc == 0).sum())} of {dc.size}, worst {int(dc.max())} level")
    assert dc.max() <= 1
    assert not got["reserved"].any() and not (got["rgb"] >> 24).any()
    # orthonormal frames
    mtm = np.einsum("nji,njk->nik", got["mat"], got["mat"])
    assert np.abs(mtm - np.eye(3)).max() <= 1e-5
    assert np.all(np.linalg.det(got["mat"]) > 0.999)
    # every value inside its range (float32 arithmetic is monotonic: the bounds are the formula at the range's ends)
    f32 = np.float32
    cam = r.camera
    pos0, hw = np.array(cam.pos[:], f32), f32(dr.cam_pos)
    p = got["pos"].astype(f32)
    assert np.all(p >= pos0 - hw) and np.all(p <= pos0 + hw) and np.ptp(p, axis=0).min() > 0.5 * hw
    for k, base, pair in (("fovy", cam.fovy, dr.fovy), ("head_ambient", cam.head_ambient, dr.ambient),
                          ("head_diffuse", cam.head_diffuse, dr.headlight)):
        v = got[k].astype(f32)
        assert np.all(v >= f32(base) * f32(pair[0])) and np.all(v <= f32(base) * f32(pair[1])), k
        assert np.ptp(v) > 0.5 * f32(base) * (f32(pair[1]) - f32(pair[0])), k
    for l in range(cam.nlight):
        v, b = got["light_diffuse"][:, l].astype(f32), f32(cam.light_diffuse[l])
        assert np.all(v >= b * f32(dr.light[l][0])) and np.all(v <= b * f32(dr.light[l][1]))
    mat0 = np.array(cam.mat[:], np.float64).reshape(3, 3)
    rel = np.einsum("ji,njk->nik", mat0, got["mat"])
    ang = np.arccos(np.clip((np.trace(rel, axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert ang.max() <= np.sqrt(3) * dr.cam_rot + 1e-5 and ang.max() > 0.3 * dr.cam_rot
    d0 = np.array([cam.light_dir[l][:] for l in range(cam.nlight)], np.float64)
    cosang = np.clip(np.einsum("nlk,lk->nl", got["light_dir"][:, :cam.nlight], d0), -1, 1)
    assert np.arccos(cosang).max() <= np.sqrt(3) * dr.light_rot + 1e-5
    for m in range(views_ref.NMAT):
        for c in range(3):
            b = ((int(base_rgb[m]) >> (8 * c)) & 0xFF) / 255.0
            lo, hi = (np.floor(np.clip(b * float(s), 0, 1) * 255 + 0.5) for s in dr.color[m])
            v = chan(got["rgb"])[:, m, c]
            assert np.all(v >= lo - 1) and np.all(v <= hi + 1), (m, c)      # one level: the colour tolerance


def test_sampler_zero_width_sharding_mask_and_episode():
    dev = "cuda:0"
    kw = dict(obs_type=PIX, observation_width=16, observation_height=12)
    whole = SO100VecEnv(8, **kw)
    # zero-width ranges: the base camera, lights and colours bit for bit (front_close's mat has signed zeros)
    for name in ("top", "front_close"):
        r = R.CameraRenderer(whole, 16, 12, camera=name)
        w = r.identity_views().cpu().numpy()
        one = _native.SO100View()
        cam = r.camera
        one.pos[:], one.mat[:], one.fovy = cam.pos[:], cam.mat[:], cam.fovy
        one.head_ambient, one.head_diffuse = cam.head_ambient, cam.head_diffuse
        one.light_diffuse[:] = cam.light_diffuse[:]
        for l in range(_native.SO100_MAX_LIGHTS):
            one.light_dir[l][:] = cam.light_dir[l][:]
        one.rgb[:] = [int(x) for x in r.base_rgb]
        want = np.frombuffer(bytes(one), dtype=np.int32)
        assert np.array_equal(w, np.tile(want, (8, 1))), name
    # sharding: 8 envs at offset 0 = 4 at offset 0 and 4 at offset 4
    ep = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3], dtype=torch.int32, device=dev)
    full = whole.renderer.sample_views(RANGES, 5, episode=ep).clone()
    for off in (0, 4):
        part = SO100VecEnv(4, env_offset=off, **kw)
        got = part.renderer.sample_views(RANGES, 5, episode=ep[off:off + 4].contiguous())
        assert torch.equal(got, full[off:off + 4]), off
    assert not torch.equal(full[:4], full[4:])
    # a masked launch leaves the other records untouched and gives the masked ones what the full launch gave
    r = whole.renderer
    r.views.fill_(0x5A5A5A5A)
    mask = torch.tensor([1, 0, 0, 1, 1, 0, 1, 0], dtype=torch.bool, device=dev)
    got = r.sample_views(RANGES, 5, episode=ep, mask=mask).clone()
    assert torch.equal(got[mask], full[mask]) and bool((got[~mask] == 0x5A5A5A5A).all())
    # the episode number: another one changes every env's draws, the same one repeats them; None = 0
    again = r.sample_views(RANGES, 5, episode=ep).clone()
    other = r.sample_views(RANGES, 5, episode=ep + 1).clone()
    assert torch.equal(again, full)
    assert bool((other != full).any(dim=1).all())
    zero = r.sample_views(RANGES, 5, episode=torch.zeros_like(ep)).clone()
    assert torch.equal(r.sample_views(RANGES, 5), zero)
    assert not torch.equal(r.sample_views(RANGES, 6), zero)            # and the seed
    torch.cuda.synchronize()


def test_vec_env_visual_randomisation_touches_images_only():
    n, W, H, T = 8, 64, 48, 30
    phys = dict(mass=(1.0, 1.0), friction=(1.0, 1.0), action_noise=0.0)
    kw = dict(obs_type=PIX, observation_width=W, observation_height=H, max_episode_steps=7, seed=3)
    vis = dict(RANGES, seed=21)
    off = SO100VecEnv(n, domain_randomization=dict(phys), **kw)
    fix = SO100VecEnv(n, domain_randomization=dict(phys, visual=vis), **kw)
    per = SO100VecEnv(n, domain_randomization=dict(phys, visual=dict(vis, per_episode=True)), **kw)
    twin = SO100VecEnv(n, domain_randomization=dict(phys), autoreset=False, max_episode_steps=7, seed=3)
    assert off.renderer.views is None
    views0 = fix.renderer.views.clone()
    obs = [e.reset(seed=9)[0] for e in (off, fix, per)]
    assert not torch.equal(obs[0]["pixels"], obs[1]["pixels"]) and not torch.equal(obs[1]["pixels"], obs[2]["pixels"])
    g = torch.Generator().manual_seed(4)
    tmp = torch.zeros_like(per.pixels)
    dones = 0
    for t in range(T):
        act = torch.rand(n, 6, generator=g) * 2 - 1
        v_prev, ep_prev = per.renderer.views.clone(), per.episode.clone()
        twin.set_state(**per.get_state())
        twin.step(act)
        res = [e.step(act) for e in (off, fix, per)]
        for e, (o, rew, term, trunc, info) in zip((fix, per), res[1:]):
            assert torch.equal(e.qpos, off.qpos) and torch.equal(e.qvel, off.qvel) and torch.equal(e.obs, off.obs)
            assert torch.equal(rew, res[0][1]) and torch.equal(term, res[0][2]) and torch.equal(trunc, res[0][3])
            assert torch.equal(o["agent_pos"], res[0][0]["agent_pos"])
        assert torch.equal(fix.renderer.views, views0)                  # per_episode false: never resampled
        done = res[2][2] | res[2][3]
        assert torch.equal(twin.qpos[~done], per.qpos[~done])           # the twin steps as the env does
        changed = (per.renderer.views != v_prev).any(dim=1)
        assert torch.equal(per.episode != ep_prev, done)
        assert torch.equal(changed, done)                               # exactly where the episode counter moved
        assert torch.equal(res[2][0]["pixels"], per.renderer.render(out=tmp))      # pixels: the records of now
        if bool(done.any()):
            dones += int(done.sum())
            # the terminal image: the final state (the twin's, stepped without a reset) under the record before
            per.renderer.render(qpos=twin.qpos, out=tmp, views=v_prev)
            assert torch.equal(res[2][4]["final_observation"]["pixels"][done], tmp[done])
            per.renderer.render(qpos=twin.qpos, out=tmp)
            assert not torch.equal(per.final_pixels[done], tmp[done])   # not under the new one
    torch.cuda.synchronize()
    assert dones >= 4 * n


def test_sb3_adapter_takes_the_visual_dict():
    from gym_so100.sb3 import SO100SB3VecEnv
    n, W, H = 4, 40, 30
    phys = dict(mass=(0.9, 1.1), friction=(0.9, 1.1), action_noise=0.0)
    kw = dict(seed=3, max_episode_steps=5, obs_type=PIX, observation_width=W, observation_height=H)
    a = SO100SB3VecEnv(n, domain_randomization=dict(phys, visual=dict(RANGES, per_episode=True)), **kw)
    b = SO100SB3VecEnv(n, domain_randomization=dict(phys), **kw)
    for e in (a, b):
        e.seed(7)
    oa, ob = a.reset(), b.reset()
    rng = np.random.default_rng(0)
    for t in range(4):
        for o in (oa, ob):
            assert o["pixels"].shape == (n, H, W, 3) and o["pixels"].dtype == np.uint8
            assert o["agent_pos"].shape == (n, 6) and o["agent_pos"].dtype == np.float32
        np.testing.assert_array_equal(oa["agent_pos"], ob["agent_pos"])
        for i in range(n):
            assert np.any(oa["pixels"][i] != ob["pixels"][i], axis=-1).mean() > 0.10, (t, i)
        if t == 3:
            break
        act = rng.uniform(-1, 1, size=(n, 6)).astype(np.float32)
        (oa, ra, da, ia), (ob, rb, db, ib) = a.step(act), b.step(act)
        assert ra.shape == (n,) and ra.dtype == np.float32 and da.shape == (n,) and da.dtype == bool
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(da, db)
        assert len(ia) == n


def test_refusals_and_masked_reset():
    n, W, H = 4, 16, 12
    env = SO100VecEnv(n, obs_type=PIX, observation_width=W, observation_height=H, max_episode_steps=0,
                      domain_randomization=dict(mass=(1.0, 1.0), friction=(1.0, 1.0), action_noise=0.0,
                                                visual=dict(RANGES, per_episode=True)))
    r, lib, err = env.renderer, env.lib, env.lib.so100_last_error
    env.reset(seed=1)
    # a masked reset draws the masked envs' records again and no others
    before = r.views.clone()
    mask = torch.tensor([0, 1, 1, 0], dtype=torch.bool, device=env.device)
    env.reset(mask=mask)
    assert torch.equal((r.views != before).any(dim=1), mask)
    # the C-ABI's refusals: nothing is drawn by a refused call
    hwc = torch.full((n, H, W, 3), SENTINEL, dtype=torch.uint8, device=env.device)
    out = _native.SO100ImageOut(hwc=_native.ptr(hwc))

    def render_views(views):
        return lib.so100_render_views(env._handle, _native.ptr(env.qpos), None, ctypes.byref(r.camera),
                                      _native.ptr(views), W, H, ctypes.byref(out), env._stream())
    assert render_views(None) != 0 and b"NULL views" in err()
    scene, material, _ = scene_parts()
    ids = np.ascontiguousarray(material)
    assert lib.so100_render_materials(env._handle, ids.ctypes.data, len(ids) - 1) != 0 and b"ntri" in err()
    bad = ids.copy()
    bad[7] = 5
    assert lib.so100_render_materials(env._handle, bad.ctypes.data, len(bad)) != 0 and b"out of range" in err()
    assert render_views(r.views) == 0                      # the refused uploads left the ids in place
    torch.cuda.synchronize()
    drawn = hwc.clone()
    assert torch.equal(drawn, r.render(out=torch.zeros_like(hwc)))
    # a new mesh drops the ids of the mesh before it
    tri = np.ascontiguousarray(scene["tri"], dtype=np.float32)
    body = np.ascontiguousarray(scene["body"], dtype=np.int32)
    rgb = np.ascontiguousarray(scene["rgb"], dtype=np.float32)
    assert lib.so100_render_mesh(env._handle, tri.ctypes.data, body.ctypes.data, rgb.ctypes.data, len(body)) == 0
    hwc.fill_(SENTINEL)
    assert render_views(r.views) != 0 and b"no materials" in err()
    torch.cuda.synchronize()
    assert bool((hwc == SENTINEL).all())
    assert lib.so100_render_materials(env._handle, ids.ctypes.data, len(ids)) == 0
    assert render_views(r.views) == 0
    torch.cuda.synchronize()
    assert torch.equal(hwc, drawn)
    # a bad range is refused by the sampler before any launch
    dr = R.view_ranges(RANGES, 1)
    dr.fovy[0], dr.fovy[1] = 1.1, 0.9
    rgb5 = np.ascontiguousarray(r.base_rgb)
    assert lib.so100_views_sample(env._handle, ctypes.byref(dr), ctypes.byref(r.camera), rgb5.ctypes.data, None, None,
                                  _native.ptr(r.views), env._stream()) != 0 and b"bad range" in err()
    with pytest.raises(ValueError):
        r.render(views=r.views[:, :39])
    with pytest.raises(ValueError):
        env.set_domain_randomization(visual={"lights": (2.0, 1.0)})
