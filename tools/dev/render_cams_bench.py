"""Multi-camera launch timings (profiles/render_cams.txt).
usage: render_cams_bench.py <tree> <tag>            one process: JSON lines on stdout
       render_cams_bench.py --report <lines file>   the table of the collected lines on stdout
<tree>: the checkout whose package and library to load (this one, or the parent commit's exported beside it, run
interleaved); <tag> labels the JSON lines.
HIP events around single launches, 3 warm-up launches, then 10 timed ones: the hwc-only render launch in either tree at
4,096 x 64x48 and 2,048 x 640x480; in a tree with so100_render_cams also, at 4,096 x 64x48 and 1,024 x 160x120 (where N
alone leaves part of the chip empty), the one K = 3 launch (top, angle, front_close; hwc sink) and the three
so100_render_aux launches it replaces, in sequence between one pair of events, each of the three alone, and the one
launch again (the first case of a size starts from an idle device; the repeat does not)."""
import json
import os
import statistics
import sys

REPS = 10
NAMES = ("top", "angle", "front_close")


def ev_time(torch, fn, reps=REPS, warm=3):
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


def measure(tree, tag):
    sys.path.insert(0, os.path.join(os.path.abspath(tree), "gym-so100-c_amd"))
    import ctypes
    import torch
    from gym_so100 import SO100VecEnv, _native
    from gym_so100 import render as R

    def emit(**kw):
        v = kw["ms"]
        kw.update(min=min(v), median=round(statistics.median(v), 4), max=max(v), tag=tag, lib=_native.source_hash())
        print(json.dumps(kw), flush=True)

    def stepped(n, w, h):
        env = SO100VecEnv(n, obs_type="so100_pixels_agent_pos", observation_width=w, observation_height=h,
                          autoreset=False, max_episode_steps=0)
        env.reset(seed=1)
        act = torch.rand(n, 6, device=env.device) * 2 - 1
        for _ in range(3):
            env.step(act)
        torch.cuda.synchronize()
        return env

    for n, w, h in ((4096, 64, 48), (2048, 640, 480)):
        env = stepped(n, w, h)
        emit(what="hwc", n=n, w=w, h=h, ms=ev_time(torch, lambda: env.renderer.render()))
        env.close()
        del env
        torch.cuda.empty_cache()
    if not hasattr(R, "MultiCameraRenderer"):
        return
    for n, w, h in ((4096, 64, 48), (1024, 160, 120)):
        env = stepped(n, w, h)
        r = R.MultiCameraRenderer(env, w, h, cameras=NAMES)
        one = torch.zeros(n, h, w, 3, dtype=torch.uint8, device=env.device)
        sink, aux = _native.SO100ImageOut(hwc=_native.ptr(one)), _native.SO100AuxOut()

        def aux_launch(c):
            env.lib.so100_render_aux(env._handle, _native.ptr(env.qpos), None, ctypes.byref(r.cameras[c]), None, w, h,
                                     ctypes.byref(sink), ctypes.byref(aux), env._stream())

        emit(what="cams K=3, one launch", n=n, w=w, h=h, ms=ev_time(torch, lambda: r.render()))
        emit(what="aux x 3, in sequence", n=n, w=w, h=h, ms=ev_time(torch, lambda: [aux_launch(c) for c in range(3)]))
        for c, name in enumerate(NAMES):
            emit(what=f"aux {name}", n=n, w=w, h=h, ms=ev_time(torch, lambda: aux_launch(c)))
        # the one launch once more, after the others: the first case of a size starts from an idle device
        emit(what="cams K=3, again", n=n, w=w, h=h, ms=ev_time(torch, lambda: r.render()))
        env.close()
        del env, r, one
        torch.cuda.empty_cache()


def report(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    keys = []
    for r in rows:
        k = (r["tag"], r["what"], r["n"], r["w"], r["h"])
        if k not in keys:
            keys.append(k)
    print(f"{'side':8s} {'what':24s} {'envs x image':18s} runs  process medians              pooled min / median / max")
    for k in keys:
        sel = [r for r in rows if (r["tag"], r["what"], r["n"], r["w"], r["h"]) == k]
        pooled = [x for r in sel for x in r["ms"]]
        meds = " ".join(f"{r['median']:.4f}" for r in sel)
        print(f"{k[0]:8s} {k[1]:24s} {k[2]:5d} x {k[3]}x{k[4]:<8d} {len(sel):4d}  {meds:28s} "
              f"{min(pooled):.4f} / {statistics.median(pooled):.4f} / {max(pooled):.4f}")
    print("\nraw repeats (one JSON line per process and case):")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    if sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        measure(*sys.argv[1:3])
