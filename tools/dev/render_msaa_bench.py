"""Multisampled launch timings (profiles/render_msaa.txt).
usage: render_msaa_bench.py <tree> <tag>            one process: JSON lines on stdout
       render_msaa_bench.py --report <lines file>   the table of the collected lines on stdout
<tree>: the checkout whose package and library to load (this one, or the parent commit's exported beside it, run
interleaved); <tag> labels the JSON lines.
HIP events around single launches, 3 warm-up launches, then 10 timed ones, at 4,096 x 64x48, 1,024 x 160x120 and
2,048 x 640x480: in either tree the K = 1 so100_render_cams launch of the `top` camera at W x H (hwc sink; the yardstick)
and what anti-aliasing costs without so100_render_msaa: the same launch at 2W x 2H followed by the torch resolve to uint8
(reshape to 2 x 2 blocks, int16 sum, + 2, // 4), timed as one unit; in a tree with so100_render_msaa also that launch
at 2 and 4 samples (default patterns) and with the ordered grid, and the cams launch again (the first case of a size
starts from an idle device).  At 4,096 x 64x48 also K = 3 (top, angle, front_close): cams and 2 / 4 samples."""
import json
import os
import statistics
import sys

REPS = 10
SIZES = ((4096, 64, 48), (1024, 160, 120), (2048, 640, 480))


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
    import torch
    from gym_so100 import SO100VecEnv, _native
    from gym_so100 import render as R

    def emit(**kw):
        v = kw["ms"]
        kw.update(min=min(v), median=round(statistics.median(v), 4), max=max(v), tag=tag, lib=_native.source_hash())
        print(json.dumps(kw), flush=True)

    def stepped(n):
        env = SO100VecEnv(n, autoreset=False, max_episode_steps=0)
        env.reset(seed=1)
        act = torch.rand(n, 6, device=env.device) * 2 - 1
        for _ in range(3):
            env.step(act)
        torch.cuda.synchronize()
        return env

    has = hasattr(R, "make_antialias")
    for n, w, h in SIZES:
        env = stepped(n)
        for names in (("top",), ("top", "angle", "front_close")) if (w, h) == (64, 48) else (("top",),):
            K = len(names)
            plain = R.MultiCameraRenderer(env, w, h, cameras=names)
            emit(what=f"cams K={K}", n=n, w=w, h=h, ms=ev_time(torch, lambda: plain.render()))
            if K == 1:
                big = R.MultiCameraRenderer(env, 2 * w, 2 * h, cameras=names)

                def pooled():
                    img = big.render()
                    s = img.view(n, K, h, 2, w, 2, 3).to(torch.int16).sum(dim=(3, 5))
                    return ((s + 2) // 4).to(torch.uint8)
                emit(what=f"cams 2Wx2H + torch resolve K={K}", n=n, w=w, h=h, ms=ev_time(torch, pooled))
                del big
                torch.cuda.empty_cache()
            if has:
                cases = [("msaa 2", 2), ("msaa 4", 4)]
                if K == 1:
                    cases.append(("msaa 4 ordered", {"samples": 4, "offsets": ((-.25, -.25), (.25, -.25), (-.25, .25),
                                                                               (.25, .25))}))
                for label, opt in cases:
                    r = R.MultiCameraRenderer(env, w, h, cameras=names, antialias=opt)
                    emit(what=f"{label} K={K}", n=n, w=w, h=h, ms=ev_time(torch, lambda: r.render()))
                    del r
                emit(what=f"cams K={K}, again", n=n, w=w, h=h, ms=ev_time(torch, lambda: plain.render()))
            del plain
        env.close()
        del env
        torch.cuda.empty_cache()


def report(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    keys = []
    for r in rows:
        k = (r["tag"], r["what"], r["n"], r["w"], r["h"])
        if k not in keys:
            keys.append(k)
    print(f"{'side':8s} {'what':34s} {'envs x image':18s} runs  process medians              pooled min / median / max")
    for k in keys:
        sel = [r for r in rows if (r["tag"], r["what"], r["n"], r["w"], r["h"]) == k]
        pooled = [x for r in sel for x in r["ms"]]
        meds = " ".join(f"{r['median']:.4f}" for r in sel)
        print(f"{k[0]:8s} {k[1]:34s} {k[2]:5d} x {k[3]}x{k[4]:<8d} {len(sel):4d}  {meds:28s} "
              f"{min(pooled):.4f} / {statistics.median(pooled):.4f} / {max(pooled):.4f}")
    print("\nraw repeats (one JSON line per process and case):")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    if sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        measure(*sys.argv[1:3])
