"""Packing checkpoint: per-env solver cost (so100_env_cost) over steps of the bench workload; wave maxima with identity
quartets and with quartets re-formed in blocks from the previous step's keys.
The costs are recorded while packing is on; an env's cost does not depend on its wave-mates, so the identity quartets are
evaluated on the same record.
usage: python tools/dev/pack_predictor.py [n_envs] [warmup] [steps] [out]"""
import ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gym-so100-c_amd"))
import torch
from gym_so100 import SO100VecEnv, _native

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 30
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 21
out = sys.argv[4] if len(sys.argv) > 4 else f"pack_predictor_{n}.txt"
dev = torch.device("cuda", 0)
env = SO100VecEnv(n, task="so100_cube_to_bin", device=str(dev), seed=0, env_offset=0)
env.env_packing = True
env.reset(seed=1000)
g = torch.Generator(device=dev)
g.manual_seed(0)
pool = [(torch.rand(n, 6, generator=g, device=dev) * 2 - 1).contiguous() for _ in range(16)]
lib = _native.load()
rec = []
for i in range(warm + steps):
    env.set_action_buffer(pool[i % 16])
    env.step_async_raw()
    if i >= warm:
        buf = np.zeros(n, dtype=np.uint32)
        _native.check(lib.so100_env_cost(env._handle, buf.ctypes.data_as(ctypes.c_void_p), n), "so100_env_cost")
        rec.append(buf)
torch.cuda.synchronize(dev)
rec = np.stack(rec)
it = (rec >> 24).astype(np.int64)
con = ((rec >> 12) & 4095).astype(np.int64)
npi = (rec & 4095).astype(np.int64)
ids = np.arange(n)


def quartets(key, block):
    """env ids ranked by descending key (ties: env id) inside each block of `block` envs, as rows of 4."""
    nb = (n + block - 1) // block
    pad = nb * block
    k = np.full(pad, -1, dtype=np.int64)
    k[:n] = key
    k = k.reshape(nb, block)
    o = np.argsort(-k, axis=1, kind="stable") + (np.arange(nb) * block)[:, None]
    return o.reshape(-1, 4)


def wave_sum_max(v, q):
    vv = np.concatenate([v, np.zeros(q.max() + 1 - n if q.max() >= n else 0, dtype=v.dtype)])
    return vv[q].max(1).sum()


def wave_np_rounds(v, q):
    vv = np.concatenate([v, np.zeros(q.max() + 1 - n if q.max() >= n else 0, dtype=v.dtype)])
    return ((vv[q].sum(1) + 3) // 4).sum(), ((vv[q].sum(1) + 3) // 4).max()


nw = (n + 3) // 4
ident = quartets(-ids, 4)   # identity quartets
lines = [f"lib {_native.source_hash()}  envs {n}  warmup {warm}  recorded steps {steps}  waves {nw}",
         f"per env and step, mean: Newton loop passes {it.mean():.3f}  contacts {con.mean():.3f}  narrowphase items {npi.mean():.3f}",
         "per wave and step (sum over the step's 10 substeps of each env, then the max over the wave's 4 envs):",
         "step  passes: identity  pack64(prev key)  pack256(prev key)  pack64(oracle)   contacts: identity  pack64   "
         "np rounds/wave: identity  pack64 (max identity, max pack64)   corr(passes t, t+1)"]
acc = []
for t in range(1, steps):
    key = rec[t - 1].astype(np.int64)
    q64, q256, qor = quartets(key, 64), quartets(key, 256), quartets(it[t], 64)
    a = [wave_sum_max(it[t], ident) / nw, wave_sum_max(it[t], q64) / nw, wave_sum_max(it[t], q256) / nw,
         wave_sum_max(it[t], qor) / nw, wave_sum_max(con[t], ident) / nw, wave_sum_max(con[t], q64) / nw]
    r0, m0 = wave_np_rounds(npi[t], ident)
    r1, m1 = wave_np_rounds(npi[t], q64)
    a += [r0 / nw, r1 / nw, float(m0), float(m1), float(np.corrcoef(it[t - 1], it[t])[0, 1])]
    acc.append(a)
    lines.append(f"{t:3d}  " + "  ".join(f"{x:9.3f}" for x in a))
m = np.mean(acc, axis=0)
lines.append("mean " + "  ".join(f"{x:9.3f}" for x in m))
lines.append(f"passes saved per wave and step: pack64 {m[0] - m[1]:.3f}  pack256 {m[0] - m[2]:.3f}  oracle64 {m[0] - m[3]:.3f}")
# fraction of envs per pass count, and how much of a step's extra passes sit in envs that had extra passes the step before
h = np.bincount(it[-1], minlength=30)[:30]
lines.append("histogram of passes per env (last step): " + " ".join(f"{k}:{v}" for k, v in enumerate(h) if v))
open(out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
