"""Fused-kernel wave timeline with packing off / on (needs the -DSO100_TIMELINE variant via SO100_LIB): launch span,
resident waves, in-kernel clock (shader cycles per 100-MHz tick), and the mean wave's cycles by phase.
usage: SO100_LIB=.../libso100_hip_timeline.so python tools/dev/pack_timeline.py [n_envs] [out]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-so100-c_amd"))
import torch
from gym_so100 import SO100VecEnv, _native

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
out = sys.argv[2] if len(sys.argv) > 2 else f"pack_timeline_{n}.txt"
lines = [f"lib {_native.source_hash()} (-DSO100_TIMELINE, the debug build of the fused kernel)  envs {n}"]
for pack in (False, True):
    env = SO100VecEnv(n, device="cuda:0", seed=0, debug=True)
    env.env_packing = pack
    env.reset(seed=1000)
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = [(torch.rand(n, 6, generator=g, device="cuda") * 2 - 1).contiguous() for _ in range(16)]
    acc = []
    for i in range(36):
        env.step(pool[i % 16])
        if i < 32:
            continue
        torch.cuda.synchronize()
        q = np.minimum(env.env_order().reshape(-1, 4)[:, 0], n - 1)     # a row of each wave
        d = env.debug[:, 88:95].cpu().numpy()[q]
        u = d[:, :4].copy().view(np.uint32).astype(np.uint64)
        t0, t1 = u[:, 0] | (u[:, 1] << 32), u[:, 2] | (u[:, 3] << 32)
        s, e = (t0 - t0.min()).astype(np.float64) * 0.01, (t1 - t0.min()).astype(np.float64) * 0.01
        dur = e - s
        asm, newt, fin = d[:, 4].astype(np.float64), d[:, 5].astype(np.float64), d[:, 6].astype(np.float64)
        tot = asm + newt + fin
        ts = np.linspace(0, e.max(), 21)[:-1]
        conc = [int(((s <= t) & (e > t)).sum()) for t in ts]
        acc.append([e.max(), dur.mean(), dur.max(), dur.sum() / e.max(), tot.sum() / (dur.sum() * 1e3), asm.mean(), newt.mean(),
                    fin.mean(), tot.mean()])
        lines.append(f"packing {int(pack)} step {i}: span {e.max():.0f} us  wave us mean {dur.mean():.0f} p99 "
                     f"{np.percentile(dur, 99):.0f} max {dur.max():.0f}  mean resident waves {dur.sum() / e.max():.0f}  "
                     f"resident over the span (20 samples) {conc}")
    m = np.mean(acc, axis=0)
    lines.append(f"packing {int(pack)} mean of 4 steps: span {m[0]:.0f} us  mean wave {m[1]:.0f} us  longest wave {m[2]:.0f} us  "
                 f"mean resident waves {m[3]:.0f}  in-kernel clock {m[4]:.3f} GHz  mean wave kcycles: assembly {m[5] / 1e3:.0f} "
                 f"newton {m[6] / 1e3:.0f} epilogue {m[7] / 1e3:.0f} total {m[8] / 1e3:.0f}")
    env.close()
open(out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
