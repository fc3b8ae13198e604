"""Depth and label sink timings (profiles/render_aux.txt).  usage: render_aux_bench.py <tree> <tag>
<tree>: the checkout whose package and library to load (this one, or the parent commit's exported beside it, run
interleaved); <tag> labels the JSON lines.
HIP events around single launches, 3 warm-up launches, then 10 timed ones: the hwc-only render launch in either tree;
in a tree with so100_render_aux also the aux launch with the hwc sink alone, with hwc + label, hwc + depth, hwc + depth
+ label, and the last with sampled view records."""
import json
import os
import statistics
import sys

tree, tag = sys.argv[1:3]
sys.path.insert(0, os.path.join(os.path.abspath(tree), "gym-so100-c_amd"))
import torch
from gym_so100 import SO100VecEnv, _native

SIZES = [(4096, 64, 48), (2048, 640, 480)]
REPS = 10
RANGES = dict(camera_pos=0.03, camera_rot_deg=2.865, fovy=(0.9, 1.1), ambient=(0.6, 1.4), headlight=(0.6, 1.4),
              lights=(0.6, 1.4), light_rot_deg=9.74, colors=(0.6, 1.2))


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
        out.append(round(e0.elapsed_time(e1), 4))
    return out


def emit(**kw):
    v = kw["ms"]
    kw.update(min=min(v), median=round(statistics.median(v), 4), max=max(v), tag=tag, lib=_native.source_hash())
    print(json.dumps(kw), flush=True)


for n, w, h in SIZES:
    env = SO100VecEnv(n, obs_type="so100_pixels_agent_pos", observation_width=w, observation_height=h,
                      autoreset=False, max_episode_steps=0)
    env.reset(seed=1)
    act = torch.rand(n, 6, device=env.device) * 2 - 1
    for _ in range(3):
        env.step(act)
    torch.cuda.synchronize()
    r = env.renderer
    emit(what="hwc", n=n, w=w, h=h, ms=ev_time(lambda: r.render()))
    if hasattr(_native, "SO100AuxOut"):
        import ctypes
        dep = torch.zeros(n, h, w, dtype=torch.float32, device=env.device)
        seg = torch.zeros(n, h, w, dtype=torch.uint8, device=env.device)
        sinks = _native.SO100ImageOut(hwc=_native.ptr(r.pixels))

        def aux_hwc_only():                  # the aux kernel with no aux sink (render() would take so100_render)
            aux = _native.SO100AuxOut()
            env.lib.so100_render_aux(env._handle, _native.ptr(env.qpos), None, ctypes.byref(r.camera), None, w, h,
                                     ctypes.byref(sinks), ctypes.byref(aux), env._stream())
        emit(what="aux hwc only", n=n, w=w, h=h, ms=ev_time(aux_hwc_only))
        emit(what="aux hwc + label", n=n, w=w, h=h, ms=ev_time(lambda: r.render(segmentation=seg)))
        emit(what="aux hwc + depth", n=n, w=w, h=h, ms=ev_time(lambda: r.render(depth=dep)))
        emit(what="aux hwc + depth + label", n=n, w=w, h=h, ms=ev_time(lambda: r.render(depth=dep, segmentation=seg)))
        r.sample_views(RANGES, 1)
        emit(what="aux hwc + depth + label, sampled views", n=n, w=w, h=h,
             ms=ev_time(lambda: r.render(depth=dep, segmentation=seg)))
        r.views = None
        del dep, seg
    env.close()
    del env, r
    torch.cuda.empty_cache()
