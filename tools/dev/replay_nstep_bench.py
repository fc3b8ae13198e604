"""Timings of the uniform replay buffer's n-step launches (so100_replay_push_nstep, so100_replay_scan +
so100_replay_sample_nstep) beside the plain launches on the same arrays and beside the same arithmetic written as torch
ops (profiles/nstep_replay.txt).  The torch restatement lives here only: it is not on the product path.
usage: replay_nstep_bench.py [--tree ROOT] [--plain-only] [--envs N[,N..]] [--obs state,pixels] [--batches B[,B..]]
  --tree ROOT    import gym_so100 from that checkout (default: this one); with --plain-only this times a build of another
                 commit with the same code
  --plain-only   only so100_replay_push / so100_replay_scan / so100_replay_sample, on a buffer built without n_step
One process: a table on stdout, then one JSON line per case.  so100_touch_cube, episodes of 12 steps (so the ring holds
ends of episodes), the ring filled by T + 8 random steps; T = 32 slots per env for state observations, 20 for 64 x 48
pixel observations.  Every figure: 3 warm-up calls, then 6 blocks of 50 calls (20 where a call takes more than a
millisecond) back to back between two HIP events, divided by the calls; the median block is reported, the others are in
the JSON line.
  "push plain / nstep"     one so100_replay_push / so100_replay_push_nstep on the same arrays.
  "scan + sample ..."      UniformReplay.sample(B) with the scan forced before it: the scan, the sample launch and the
                           allocation of the output tensors; plain, and n_step = 1, 3, 16.
  "kernel alone ..."       the sample launch alone into preallocated outputs (no scan, no allocation).
  "torch n-step"           cumsum, draws from torch's generator, searchsorted, then the n rows of `ends` and reward
                           gathered by index, a cumulative mask, the weighted sum, and the gathers of both ends of the
                           window (images unshifted: pad 0 on both sides of this comparison)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

BLOCKS = 6
NSTEPS = (1, 3, 16)
GAMMA = 0.99


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_torch_nstep(torch, rp, g):
    """scan + so100_replay_sample_nstep as torch ops over the buffer's own arrays, pad 0; the draws are torch's"""
    st, T, n, d = rp.store, rp.T, rp.n, rp.ends.device

    def sample(B, n_step, gamma):
        c, k = st["meta"][0].long(), st["meta"][1].long()
        prefix = torch.cumsum(k, 0)
        r = (torch.rand(B, dtype=torch.float64, device=d, generator=g) * prefix[-1]).long()
        e = torch.searchsorted(prefix, r, right=True).clamp_(max=n - 1)
        kidx = r - (prefix[e] - k[e])
        slot = (c[e] - k[e] + kidx) % T
        j = torch.arange(n_step, device=d)
        win = (slot[:, None] + j) % T                                        # [B, n_step]
        stop = (rp.ends[win, e[:, None]] != 0) | (kidx[:, None] + j + 1 >= k[e][:, None])
        alive = torch.cumprod(torch.cat([torch.ones_like(stop[:, :1]), ~stop[:, :-1]], 1).long(), 1)   # slot j is in
        w = torch.full((n_step,), gamma, device=d).pow(j.float())
        rewards = (st["reward"][win, e[:, None]] * alive * w).sum(1)
        m = alive.sum(1)
        last = (slot + m - 1) % T
        out = dict(actions=st["action"][slot, e], rewards=rewards, dones=st["terminated"][last, e].float(),
                   discounts=torch.full((B,), gamma, device=d).pow(m.float()), n_steps=m.int(), last_slot=last.int(),
                   env=e.int(), slot=slot.int(), obs=st["obs"][slot, e], next_obs=st["next_obs"][last, e])
        if rp.P:
            out["pixels"] = st["obs_img"][slot, e].view(B, *rp.image_shape)
            out["next_pixels"] = st["next_img"][last, e].view(B, *rp.image_shape)
        return out
    return sample


def main(args):
    import torch
    from gym_so100 import SO100VecEnv, _native
    from gym_so100.model import NOBS
    rows = []
    lib_hash = _native.source_hash()

    def measure(name, fn, **tags):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls = 50 if timed(torch, fn, 2) / 2 < 1.0 else 20
        blocks = [timed(torch, fn, calls) / calls * 1e3 for _ in range(BLOCKS)]
        us = statistics.median(blocks)
        rows.append(dict(name=name, us_per_call=round(us, 3), blocks_us=[round(b, 3) for b in blocks], lib=lib_hash,
                         **tags))
        print(f"  {name}: {us:.1f} us per call (blocks {min(blocks):.1f} .. {max(blocks):.1f})", flush=True)
        return us

    for n in args.envs:
        for obs in args.obs:
            pixels = obs == "pixels"
            T = 20 if pixels else 32
            kw = dict(task="so100_touch_cube", max_episode_steps=12, seed=1)
            if pixels:
                kw.update(obs_type="so100_pixels_agent_pos", observation_width=64, observation_height=48)
            ur = dict(buffer_size=n * T, seed=5)
            if not args.plain_only:
                ur.update(n_step=3, gamma=GAMMA)
            g = torch.Generator(device="cuda:0").manual_seed(3)
            env = SO100VecEnv(n, uniform_replay=ur, **kw)
            rp = env.uniform_replay
            env.reset()
            for _ in range(T + 8):
                env.step(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
            tags = dict(n=n, T=T, obs=obs)
            P = rp.P
            print(f"{n} envs, {obs} observations{' (64 x 48 RGB)' if pixels else ''}, T = {T}, library {lib_hash}: "
                  f"{rp.size():,} valid transitions of {rp.capacity:,}"
                  + ("" if args.plain_only else f", {int((rp.ends != 0).sum().item()):,} `ends` bytes set"))
            nrec = None if args.plain_only else rp._nstep

            def plain(fn):
                """fn on the plain launches of the same buffer"""
                def call():
                    rp._nstep = None
                    try:
                        return fn()
                    finally:
                        rp._nstep = nrec
                return call

            base = measure("push plain: so100_replay_push", plain(lambda: rp.after_step(env.actions)), **tags)
            if not args.plain_only:
                us = measure("push nstep: so100_replay_push_nstep", lambda: rp.after_step(env.actions), **tags)
                print(f"  push nstep - plain: {us - base:+.2f} us")
                torch_nstep = make_torch_nstep(torch, rp, g)

            def scan_sample(B, **k):
                rp._dirty = True
                return rp.sample(B, augment=False, **k)

            def direct(B, n_step):
                """the sample launch alone into preallocated outputs; n_step None: so100_replay_sample"""
                shape = {"obs": (B, NOBS), "next_obs": (B, NOBS), "actions": (B, rp.action_dim), "rewards": (B,),
                         "dones": (B,)}
                out = {k: torch.empty(*s, device=env.device) for k, s in shape.items()}
                out.update({k: torch.empty(B, dtype=torch.int32, device=env.device) for k in ("env", "slot")})
                out["shift"] = torch.empty(B, 4, dtype=torch.int32, device=env.device)
                if P:
                    out.update({k: torch.empty(B, P, dtype=torch.uint8, device=env.device)
                                for k in ("pixels", "next_pixels")})
                rec = _native.SO100ReplayOut(**{k: _native.ptr(t) for k, t in out.items()})
                rp._scan()
                rp._rec.pad = 0
                if n_step is None:
                    def call():
                        _native.check(env.lib.so100_replay_sample(env._handle, ctypes.byref(rp._rec), B,
                                                                  ctypes.c_uint64(7), ctypes.byref(rec), env._stream()),
                                      "so100_replay_sample")
                    return call, out
                more = {"discounts": torch.empty(B, device=env.device),
                        "nsteps": torch.empty(B, dtype=torch.int32, device=env.device),
                        "last_slot": torch.empty(B, dtype=torch.int32, device=env.device)}
                mrec = _native.SO100ReplayNstepOut(**{k: _native.ptr(t) for k, t in more.items()})
                ns = _native.SO100ReplayNstep(n_step=n_step, gamma=GAMMA, ends=_native.ptr(rp.ends))

                def call():
                    _native.check(env.lib.so100_replay_sample_nstep(env._handle, ctypes.byref(rp._rec), ctypes.byref(ns),
                                                                    B, ctypes.c_uint64(7), ctypes.byref(rec),
                                                                    ctypes.byref(mrec), env._stream()),
                                  "so100_replay_sample_nstep")
                return call, (out, more)

            for B in args.batches:
                t = dict(tags, batch=B)
                whole = measure(f"scan + sample plain, batch {B}", plain(lambda: scan_sample(B)), **t)
                call, keep = direct(B, None)
                alone = measure(f"kernel alone plain, batch {B}", call, **t)
                if args.plain_only:
                    continue
                for k in NSTEPS:
                    us = measure(f"scan + sample n_step {k}, batch {B}", lambda: scan_sample(B, n_step=k), **t, n_step=k)
                    call, keep = direct(B, k)
                    ka = measure(f"kernel alone n_step {k}, batch {B}", call, **t, n_step=k)
                    tor = measure(f"torch n-step {k}: cumsum + draws + window gathers + masked sum, batch {B}",
                                  lambda: torch_nstep(B, k, GAMMA), **t, n_step=k)
                    print(f"  n_step {k}, batch {B}: scan + sample - plain {us - whole:+.2f} us, kernel alone - plain "
                          f"{ka - alone:+.2f} us, torch / hip (scan + sample) {tor / us:.2f}x")
                del keep
            env.close()
            del env, rp
            torch.cuda.empty_cache()
    print("\nraw (one JSON line per case):")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.abspath(os.path.join(here, "..", "..")))
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--envs", default="8192,65536", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--obs", default="state,pixels", type=lambda s: s.split(","))
    ap.add_argument("--batches", default="256,65536", type=lambda s: [int(x) for x in s.split(",")])
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "gym-so100-c_amd"))
    main(a)
