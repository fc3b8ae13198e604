"""Timings of the uniform replay buffer's launches beside the same rules written as torch ops on the same arrays
(profiles/uniform_replay.txt).  The torch restatement lives here only: it is not on the product path.
usage: replay_bench.py [envs [slots_per_env]]      one process: a table on stdout, then one JSON line per case
8,192 envs x 64 x 48 pixel observations by default, so100_touch_cube, T = 32 slots per env, the ring filled by T + 8
random steps.  Every figure: 3 warm-up calls, then 6 blocks of 50 calls back to back between two HIP events, divided by
50; the median block is reported, the others are in the JSON line.
  "step"              step() of a pixel env of the same size without a buffer, the yardstick of the push's share.
  "hip push"          UniformReplay.after_step: one so100_replay_push.
  "torch push"        the same rules as index_put / where over the buffer's own arrays.
  "hip sample"        UniformReplay.sample(B, augment=pad) with the scan forced before it: so100_replay_scan,
                      so100_replay_sample and the allocation of the ten output tensors.
  "hip sample kernel" so100_replay_sample alone into preallocated outputs (no scan, no allocation).
  "torch sample"      cumsum, draws from torch's generator, searchsorted, the index gather of both images, and for pad > 0
                      F.pad(mode="replicate") and a per-row crop by advanced indexing, back to uint8 in the env's layout.
Bytes over time is given as a share of the 8 TB/s HBM peak for the two kernels named in each line."""
import ctypes
import json
import os
import statistics
import sys

BLOCKS, BLOCK_CALLS = 6, 50
HBM_PEAK = 8.0e12
BATCHES = (256, 4096)
PADS = (0, 4)


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_push(torch, env, rp, ar, command):
    """so100_replay_push's rules as torch ops over the buffer's own arrays"""
    st, T = rp.store, rp.T
    c, k = st["meta"][0].long(), st["meta"][1].long()
    done = (env.terminated | env.truncated).bool()
    drop = env.diverged.bool()
    st["next_obs"][c, ar] = torch.where(done[:, None], env.final_obs, env.obs)
    flat, final = env.pixels.view(rp.n, -1), env.final_pixels.view(rp.n, -1)
    st["next_img"][c, ar] = torch.where(done[:, None], final, flat)
    st["action"][c, ar] = command
    st["reward"][c, ar] = env.reward
    st["terminated"][c, ar] = env.terminated.to(torch.uint8)
    c2 = torch.where(drop, c, (c + 1) % T)
    k2 = torch.where(drop, k, (k + 1).clamp(max=T - 1))
    st["obs"][c2, ar] = env.obs
    st["obs_img"][c2, ar] = flat
    st["meta"][0].copy_(c2)
    st["meta"][1].copy_(k2)


def make_torch_sample(torch, env, rp, g):
    """so100_replay_scan + so100_replay_sample as torch ops; the draws are torch's own generator"""
    import torch.nn.functional as F
    st, T, n = rp.store, rp.T, rp.n
    planes, H, W, chan = rp.layout
    d = env.device
    # does replicate padding take bytes here?  If not the images go through float32, as a DrQ implementation would
    try:
        F.pad(torch.zeros(1, 1, 4, 4, dtype=torch.uint8, device=d), (1, 1, 1, 1), mode="replicate")
        via = torch.uint8
    except Exception:
        via = torch.float32

    def shift(img, B, pad):
        # [B, P] bytes -> [B, planes * chan, H, W], padded, cropped per row at (dx, dy), and back
        x = img.view(B, planes, H, W, chan).permute(0, 1, 4, 2, 3).reshape(B, planes * chan, H, W).to(via)
        x = F.pad(x, (pad, pad, pad, pad), mode="replicate")
        S = 2 * pad + 1
        dx = torch.randint(0, S, (B,), device=d, generator=g)
        dy = torch.randint(0, S, (B,), device=d, generator=g)
        ys = (dy[:, None] + torch.arange(H, device=d))[:, None, :, None]
        xs = (dx[:, None] + torch.arange(W, device=d))[:, None, None, :]
        x = x[torch.arange(B, device=d)[:, None, None, None], torch.arange(planes * chan, device=d)[None, :, None, None],
              ys, xs]
        x = x.view(B, planes, chan, H, W).permute(0, 1, 3, 4, 2).to(torch.uint8)
        return x.reshape(B, *rp.image_shape), dx, dy

    def sample(B, pad):
        c, k = st["meta"][0].long(), st["meta"][1].long()
        prefix = torch.cumsum(k, 0)
        total = prefix[-1]
        r = (torch.rand(B, dtype=torch.float64, device=d, generator=g) * total).long()
        e = torch.searchsorted(prefix, r, right=True).clamp_(max=n - 1)
        slot = (c[e] - k[e] + r - (prefix[e] - k[e])) % T
        obs, nxt = st["obs"][slot, e], st["next_obs"][slot, e]
        img, nimg = st["obs_img"][slot, e], st["next_img"][slot, e]
        if pad:
            img, dx, dy = shift(img, B, pad)
            nimg, dx2, dy2 = shift(nimg, B, pad)
            sh = torch.stack([dx, dy, dx2, dy2], 1).int()
        else:
            img, nimg = img.view(B, *rp.image_shape), nimg.view(B, *rp.image_shape)
            sh = torch.zeros(B, 4, dtype=torch.int32, device=d)
        return dict(pixels=img, next_pixels=nimg, state=obs, next_state=nxt, agent_pos=obs[:, 9:15],
                    next_agent_pos=nxt[:, 9:15], actions=st["action"][slot, e], rewards=st["reward"][slot, e],
                    dones=st["terminated"][slot, e].float(), env=e.int(), slot=slot.int(), shift=sh)
    return sample, str(via).replace("torch.", "")


def main(n, T):
    import torch
    from gym_so100 import SO100VecEnv, _native
    from gym_so100.model import NOBS
    rows = []

    def measure(name, fn, bytes_moved=None, kernel=None):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        blocks = [timed(torch, fn, BLOCK_CALLS) / BLOCK_CALLS * 1e3 for _ in range(BLOCKS)]
        us = statistics.median(blocks)
        row = dict(name=name, us_per_call=round(us, 3), blocks_us=[round(b, 3) for b in blocks], n=n, T=T,
                   lib=_native.source_hash())
        line = f"  {name}: {us:.1f} us per call (blocks {min(blocks):.1f} .. {max(blocks):.1f})"
        if bytes_moved:
            share = bytes_moved / (us * 1e-6) / HBM_PEAK
            row.update(bytes=bytes_moved, kernel=kernel, hbm_share=round(share, 4))
            line += f"; {bytes_moved / 1e6:.2f} MB over that time = {100 * share:.1f} % of the HBM peak ({kernel})"
        print(line, flush=True)
        rows.append(row)
        return us

    kw = dict(task="so100_touch_cube", obs_type="so100_pixels_agent_pos", observation_width=64, observation_height=48,
              seed=1)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    plain = SO100VecEnv(n, **kw)
    plain.reset()
    a = torch.rand(n, 6, device=plain.device, generator=g) * 2 - 1
    print(f"{n} envs x 64 x 48 RGB, so100_touch_cube, T = {T} slots per env, library {_native.source_hash()}")
    step_us = measure("step: step() of a pixel env without a buffer", lambda: plain.step(a))
    plain.close()
    del plain
    torch.cuda.empty_cache()

    env = SO100VecEnv(n, uniform_replay=dict(buffer_size=n * T, augment=True, seed=5), **kw)
    rp = env.uniform_replay
    env.reset()
    for _ in range(T + 8):
        env.step(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
    P = rp.P
    print(f"  the ring: {rp.size():,} valid transitions of {rp.capacity:,}; "
          f"{sum(t.numel() * t.element_size() for t in rp.store.values()) / 2 ** 30:.2f} GiB; P = {P} bytes per image")
    ar = torch.arange(n, device=env.device)
    floats = 4 * (2 * NOBS + NOBS + 2 * rp.action_dim + 2) + 4
    hip_push = measure("hip push: so100_replay_push", lambda: rp.after_step(env.actions),
                       n * (3 * P + floats), "so100_replay_push_kernel: P bytes read, 2 P written per env")
    tor_push = measure("torch push: the same rules as device ops", lambda: torch_push(torch, env, rp, ar, env.actions))
    print(f"  push / step = {100 * hip_push / step_us:.2f} % of the step; torch / hip = {tor_push / hip_push:.2f}x")
    torch_sample, via = make_torch_sample(torch, env, rp, g)
    print(f"  (torch sample: replicate padding through {via})")

    def scan_sample(B, pad):
        rp._dirty = True
        return rp.sample(B, augment=pad)

    def direct(B, pad):
        raw = {"obs": (B, NOBS), "next_obs": (B, NOBS), "actions": (B, rp.action_dim), "rewards": (B,), "dones": (B,)}
        out = {k: torch.empty(*s, device=env.device) for k, s in raw.items()}
        out.update({k: torch.empty(B, dtype=torch.int32, device=env.device) for k in ("env", "slot")})
        out["shift"] = torch.empty(B, 4, dtype=torch.int32, device=env.device)
        out.update({k: torch.empty(B, P, dtype=torch.uint8, device=env.device) for k in ("pixels", "next_pixels")})
        rec = _native.SO100ReplayOut(**{k: _native.ptr(t) for k, t in out.items()})
        rp._scan()

        def call():
            rp._rec.pad = pad
            _native.check(env.lib.so100_replay_sample(env._handle, ctypes.byref(rp._rec), B, ctypes.c_uint64(7),
                                                      ctypes.byref(rec), env._stream()), "so100_replay_sample")
        return call, out

    for B in BATCHES:
        for pad in PADS:
            hip = measure(f"hip sample: scan + sample, batch {B}, pad {pad}", lambda: scan_sample(B, pad))
            call, keep = direct(B, pad)
            measure(f"hip sample kernel alone, batch {B}, pad {pad}", call, B * (4 * P + 2 * floats),
                    "so100_replay_sample_kernel: 2 P bytes gathered, 2 P written per row")
            tor = measure(f"torch sample: cumsum + draws + gathers{' + pad + crop' if pad else ''}, batch {B}, pad {pad}",
                          lambda: torch_sample(B, pad))
            print(f"  torch / hip, scan + sample, batch {B}, pad {pad}: {tor / hip:.2f}x")
            del keep
    env.close()
    print("\nraw (one JSON line per case):")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.abspath(os.path.join(here, "..", "..", "gym-so100-c_amd")))
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8192, int(sys.argv[2]) if len(sys.argv) > 2 else 32)
