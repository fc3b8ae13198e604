"""The render launch's sinks (C-ABI so100_render_to, csrc/so100_render.hip band -> image phase): the channel-first
image and the flattened float32 image / 255 against the [N,H,W,3] image of so100_render, which
tests/test_gpu_render.py pins to the numpy rasteriser.  Every comparison is bitwise: the rasteriser resolves depth
with LDS atomicMin on (depth, colour) keys, so an image does not depend on thread order, and the sinks are copies of
the same band.

Sizes: 37x29 is odd (3HW = 3219: every env's planes start at another byte alignment; one band); 99x45 has two bands
of 41 and 4 rows, the second starting at byte 4,059 of a plane; 2050x2 has one row per band and a band length that
is no multiple of 4.  The dword path of the chw sink, its byte head and tail, and the band offsets are all taken."""
import ctypes

import numpy as np
import pytest
import torch

from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R

pytestmark = pytest.mark.gpu

# byte / 255 as the reference divides it (env.py:267-270: astype(np.float32) / 255.0)
TABLE = np.arange(256, dtype=np.float32) / np.float32(255)
_STATES = {}


def state(n):
    """n envs after reset(seed) and 8 random-action steps; never auto-reset.  Built once per n and left unchanged."""
    if n not in _STATES:
        env = SO100VecEnv(n, obs_type="so100_pixels_agent_pos", observation_width=37, observation_height=29,
                          autoreset=False, max_episode_steps=0)
        g = torch.Generator().manual_seed(n)
        env.reset(seed=40 + n)
        for _ in range(8):
            env.step(torch.rand(n, 6, generator=g) * 2 - 1)
        torch.cuda.synchronize()
        _STATES[n] = env
    return _STATES[n]


def render_to(env, W, H, hwc=None, chw=None, flat=None, pitch=0, mask=None, size=None, camera=None):
    """so100_render_to on env's state; the sinks are tensors (or views: only their data_ptr is passed)."""
    sinks = _native.SO100ImageOut(hwc=_native.ptr(hwc), chw=_native.ptr(chw), flat=_native.ptr(flat), flat_pitch=pitch)
    if size is not None:
        sinks.size = size
    cam = env.renderer.camera if camera is None else camera
    rc = env.lib.so100_render_to(env._handle, _native.ptr(env.qpos), _native.ptr(mask), ctypes.byref(cam), W, H,
                                 ctypes.byref(sinks), env._stream())
    torch.cuda.synchronize()
    return rc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("W,H,drawn", [(37, 29, True), (99, 45, True), (2050, 2, False)])
def test_chw_is_hwc_permuted(W, H, drawn):
    env = state(8)
    hwc = R.CameraRenderer(env, W, H).render().clone()
    r = R.CameraRenderer(env, W, H, channels_first=True)
    assert r.pixels.shape == (8, 3, H, W)
    chw = r.render()
    torch.cuda.synchronize()
    if drawn:
        assert bool(hwc.any())
    assert torch.equal(chw, hwc.permute(0, 3, 1, 2))


def test_three_sinks_in_one_launch():
    env, W, H = state(8), 99, 45
    n, npix = 8, 3 * W * H
    ref = R.CameraRenderer(env, W, H).render().clone()           # so100_render
    hwc = torch.full((n, H, W, 3), 0xA5, dtype=torch.uint8, device=env.device)
    chw = torch.full((n, 3, H, W), 0xA5, dtype=torch.uint8, device=env.device)
    flat = torch.full((n, npix + 6), -7.0, dtype=torch.float32, device=env.device)
    assert render_to(env, W, H, hwc=hwc, chw=chw, flat=flat, pitch=npix + 6) == 0
    assert bool(ref.any())
    assert torch.equal(hwc, ref)
    assert torch.equal(chw, ref.permute(0, 3, 1, 2))
    f = flat.cpu().numpy()
    np.testing.assert_array_equal(bits(f[:, :npix]), bits(TABLE[ref.cpu().numpy().reshape(n, -1)]))
    assert (f[:, npix:] == -7.0).all()                            # beyond 3HW: never written


def test_masked_envs_and_neighbours_are_untouched():
    env, W, H = state(6), 37, 29
    n, npix = 6, 3 * W * H
    ref = R.CameraRenderer(env, W, H).render().clone()
    big_h = torch.full((8, H, W, 3), 0xA5, dtype=torch.uint8, device=env.device)
    big_c = torch.full((8, 3, H, W), 0xA5, dtype=torch.uint8, device=env.device)
    big_f = torch.full((8, npix + 1), -7.0, dtype=torch.float32, device=env.device)
    on = [1, 0, 1, 1, 0, 1]
    mask = torch.tensor(on, dtype=torch.uint8, device=env.device)
    assert render_to(env, W, H, hwc=big_h[1:7], chw=big_c[1:7], flat=big_f[1:7], pitch=npix + 1, mask=mask) == 0
    for t in (big_h, big_c):
        assert bool((t[0] == 0xA5).all()) and bool((t[7] == 0xA5).all())
    assert bool((big_f[0] == -7.0).all()) and bool((big_f[7] == -7.0).all())
    assert bool((big_f[:, npix] == -7.0).all())
    want_f = TABLE[ref.cpu().numpy().reshape(n, -1)]
    got_f = big_f[1:7, :npix].cpu().numpy()
    for i in range(n):
        if on[i]:
            assert torch.equal(big_h[1 + i], ref[i]), i
            assert torch.equal(big_c[1 + i], ref[i].permute(2, 0, 1)), i
            np.testing.assert_array_equal(bits(got_f[i]), bits(want_f[i]))
        else:
            assert bool((big_h[1 + i] == 0xA5).all()) and bool((big_c[1 + i] == 0xA5).all()), i
            assert (got_f[i] == -7.0).all(), i


def test_tracking_camera_chw():
    env, W, H = state(8), 37, 29
    hwc = R.CameraRenderer(env, W, H, camera="front_close").render().clone()
    chw = R.CameraRenderer(env, W, H, camera="front_close", channels_first=True).render()
    torch.cuda.synchronize()
    assert bool(hwc.any())
    assert torch.equal(chw, hwc.permute(0, 3, 1, 2))


def test_channels_first_env_steps_like_the_default():
    N = 8
    kw = dict(obs_type="so100_pixels_agent_pos", observation_width=48, observation_height=36, max_episode_steps=5,
              seed=7)
    a = SO100VecEnv(N, **kw)
    b = SO100VecEnv(N, channels_first=True, **kw)
    oa, _ = a.reset(seed=5)
    ob, _ = b.reset(seed=5)
    assert ob["pixels"].shape == (N, 3, 36, 48) and b.final_pixels.shape == (N, 3, 36, 48)
    assert torch.equal(ob["pixels"], oa["pixels"].permute(0, 3, 1, 2))
    g = torch.Generator().manual_seed(0)
    saw_done = False
    for t in range(12):
        act = torch.rand(N, 6, generator=g) * 2 - 1
        oa, ra, ta, ua, ia = a.step(act)
        ob, rb, tb, ub, ib = b.step(act)
        assert torch.equal(b.qpos, a.qpos) and torch.equal(rb, ra)
        assert torch.equal(tb, ta) and torch.equal(ub, ua)
        assert torch.equal(ob["agent_pos"], oa["agent_pos"])
        assert torch.equal(ob["pixels"], oa["pixels"].permute(0, 3, 1, 2))
        done = ta | ua
        assert torch.equal(ib["_final_observation"], done)
        if bool(done.any()):
            saw_done = True
            fa, fb = ia["final_observation"]["pixels"], ib["final_observation"]["pixels"]
            assert fb.shape == (N, 3, 36, 48)
            assert torch.equal(fb[done], fa[done].permute(0, 3, 1, 2))
            assert not torch.equal(fb[done], ob["pixels"][done])
    assert saw_done


def test_goal_env_flat_pixels_observation():
    N, W, H = 8, 32, 24
    npix = 3 * W * H
    env = SO100VecEnv(N, task="so100_goal", obs_type="so100_pixels_agent_pos", observation_width=W,
                      observation_height=H, max_episode_steps=3, flat_pixels=True)

    def check(obs):
        o = obs["observation"]
        assert o.shape == (N, npix + 6) and o.dtype == torch.float32 and o.data_ptr() == ptr0
        want = np.concatenate([TABLE[env.pixels.cpu().numpy().reshape(N, -1)], env.obs[:, 9:15].cpu().numpy()], axis=1)
        np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(want))

    obs, _ = env.reset(seed=3)
    ptr0 = obs["observation"].data_ptr()
    assert ptr0 == env.pixels_flat.data_ptr()
    check(obs)
    assert float(obs["observation"][:, :npix].max()) > 0
    g = torch.Generator().manual_seed(1)
    dones = 0
    for t in range(6):
        obs, rew, term, trunc, info = env.step(torch.rand(N, 6, generator=g) * 2 - 1)
        check(obs)
        dones += int((term | trunc).sum())
    assert dones >= 2 * N                                        # two TimeLimit rounds: auto-resets were drawn too


def test_refusals():
    with pytest.raises(ValueError):
        SO100VecEnv(4, task="so100_goal", obs_type="so100_pixels_agent_pos", observation_width=16,
                    observation_height=12, channels_first=True)
    env, W, H = state(8), 37, 29
    n, npix = 8, 3 * W * H
    r_h, r_c = R.CameraRenderer(env, W, H), R.CameraRenderer(env, W, H, channels_first=True)
    with pytest.raises(ValueError):
        r_h.render(out=torch.zeros_like(r_c.pixels))
    with pytest.raises(ValueError):
        r_c.render(out=torch.zeros_like(r_h.pixels))
    with pytest.raises(ValueError):
        r_h.render(flat=torch.zeros(n, npix - 1, device=env.device))
    hwc = torch.full((n, H, W, 3), 0xA5, dtype=torch.uint8, device=env.device)
    flat = torch.full((n, npix), -7.0, dtype=torch.float32, device=env.device)
    err = env.lib.so100_last_error
    assert render_to(env, W, H) != 0 and b"no sink" in err()
    assert render_to(env, W, H, flat=flat, pitch=npix - 1) != 0 and b"flat_pitch" in err()
    assert render_to(env, W, H, hwc=hwc, size=ctypes.sizeof(_native.SO100ImageOut) - 8) != 0 and b"size" in err()
    assert bool((hwc == 0xA5).all()) and bool((flat == -7.0).all())          # a refused call draws nothing
    assert render_to(env, W, H, hwc=hwc) == 0 and torch.equal(hwc, r_h.render())


def test_demo_recorder_takes_a_channels_first_env():
    """The recorder hands over channel-first pixels (record_teleop.py:163-184): the same episodes from either env."""
    from gym_so100.demos import DemoRecorder
    kw = dict(obs_type="so100_pixels_agent_pos", observation_width=48, observation_height=36, max_episode_steps=4)
    envs = [SO100VecEnv(4, **kw), SO100VecEnv(4, channels_first=True, **kw)]
    recs = [DemoRecorder(e, env_ids=[0, 2], max_episodes=2) for e in envs]
    g = torch.Generator().manual_seed(0)
    for e in envs:
        e.reset(seed=0)
    for t in range(5):
        act = torch.rand(4, 6, generator=g) * 2 - 1
        for e, rec in zip(envs, recs):
            obs, r, term, trunc, info = e.step(act)
            rec.add(act, obs, r, term, trunc, info)
    a, b = (rec.demonstrations for rec in recs)
    assert len(a) == len(b) == 2
    for ea, eb in zip(a, b):
        assert len(ea["observations"]) == len(eb["observations"]) == 4
        for oa, ob in zip(ea["observations"], eb["observations"]):
            assert ob["pixels"].shape == (1, 3, 36, 48) and oa["pixels"].any()
            np.testing.assert_array_equal(ob["pixels"], oa["pixels"])
            np.testing.assert_array_equal(ob["agent_pos"], oa["agent_pos"])
