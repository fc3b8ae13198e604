"""Render-sink timings (profiles/render_layouts.txt).  usage: render_layouts_bench.py <tree> <tag> launch|extras
<tree>: the checkout whose package and library to load (this one, or the parent commit's in a git worktree, run
interleaved); <tag> labels the JSON lines.
launch: HIP events around single render launches (hwc in either tree; chw and all three sinks in the new one)
extras: GoalEnv pixel step with / without flat_pixels; adapter step channels_first vs HWC + numpy transpose"""
import ctypes
import json
import os
import statistics
import sys
import time

tree, tag, mode = sys.argv[1:4]
sys.path.insert(0, os.path.join(os.path.abspath(tree), "gym-so100-c_amd"))
import numpy as np
import torch
from gym_so100 import SO100VecEnv, _native
from gym_so100 import render as R

SIZES = [(4096, 64, 48), (2048, 640, 480)]
REPS = 10


def ev_time(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def emit(**kw):
    if "ms" in kw:
        v = kw["ms"]
        kw.update(min=min(v), median=statistics.median(v), max=max(v))
    kw.update(tag=tag, lib=_native.source_hash())
    print(json.dumps(kw), flush=True)


def prepared(n, w, h, **kw):
    env = SO100VecEnv(n, obs_type="so100_pixels_agent_pos", observation_width=w, observation_height=h, **kw)
    env.reset(seed=1)
    act = torch.rand(n, 6, device=env.device) * 2 - 1
    for _ in range(3):
        env.step(act)
    torch.cuda.synchronize()
    return env, act


if mode == "launch":
    for n, w, h in SIZES:
        env, _ = prepared(n, w, h, autoreset=False, max_episode_steps=0)
        emit(what="hwc", n=n, w=w, h=h, ms=ev_time(lambda: env.renderer.render()))
        if hasattr(_native, "SO100ImageOut"):
            rc = R.CameraRenderer(env, w, h, channels_first=True)
            emit(what="chw", n=n, w=w, h=h, ms=ev_time(lambda: rc.render()))
            del rc
            torch.cuda.empty_cache()
            hwc = env.pixels
            chw = torch.empty(n, 3, h, w, dtype=torch.uint8, device=env.device)
            flat = torch.empty(n, 3 * w * h + 6, dtype=torch.float32, device=env.device)
            sinks = _native.SO100ImageOut(hwc=_native.ptr(hwc), chw=_native.ptr(chw), flat=_native.ptr(flat),
                                          flat_pitch=flat.shape[1])
            cam = env.renderer.camera

            def all3():
                rcode = env.lib.so100_render_to(env._handle, _native.ptr(env.qpos), None, ctypes.byref(cam), w, h,
                                                ctypes.byref(sinks), env._stream())
                assert rcode == 0
            emit(what="hwc+chw+flat", n=n, w=w, h=h, ms=ev_time(all3))
            sinks2 = _native.SO100ImageOut(hwc=_native.ptr(hwc), flat=_native.ptr(flat), flat_pitch=flat.shape[1])

            def two():
                assert env.lib.so100_render_to(env._handle, _native.ptr(env.qpos), None, ctypes.byref(cam), w, h,
                                               ctypes.byref(sinks2), env._stream()) == 0
            emit(what="hwc+flat", n=n, w=w, h=h, ms=ev_time(two))
            del chw, flat
        env.close()
        del env
        torch.cuda.empty_cache()
else:
    from gym_so100.sb3 import SO100SB3VecEnv
    for n, w, h in SIZES:
        for fp in (False, True):
            env, act = prepared(n, w, h, task="so100_goal", flat_pixels=fp)

            def step():
                o = env.step(act)[0]["observation"]
                assert o.shape[1] == 3 * w * h + 6
            emit(what="goal_step flat_pixels=%s" % fp, n=n, w=w, h=h, ms=ev_time(step, reps=REPS))
            env.close()
            del env
            torch.cuda.empty_cache()
        reps = 10 if w < 100 else 3
        for cf in (False, True):
            env = SO100SB3VecEnv(n, obs_type="so100_pixels_agent_pos", observation_width=w, observation_height=h,
                                 channels_first=cf)
            env.reset()
            a = np.random.default_rng(0).uniform(-1, 1, size=(n, 6)).astype(np.float32)
            env.step(a)
            ts, tt = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                obs = env.step(a)[0]
                t1 = time.perf_counter()
                if not cf:
                    x = np.ascontiguousarray(obs["pixels"].transpose(0, 3, 1, 2))
                t2 = time.perf_counter()
                ts.append((t1 - t0) * 1e3)
                tt.append((t2 - t1) * 1e3)
            emit(what="adapter_step channels_first=%s" % cf, n=n, w=w, h=h, ms=ts)
            if not cf:
                emit(what="numpy transpose to contiguous NCHW", n=n, w=w, h=h, ms=tt)
            env.close()
            del env
            torch.cuda.empty_cache()
