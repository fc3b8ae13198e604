"""Timings of prioritised replay in the uniform replay buffer (so100_replay_push_per, so100_replay_per_scan,
so100_replay_sample_per, so100_replay_per_update) beside the plain and n-step launches of the same process on the same
arrays, and beside the same rules written as torch ops (profiles/per_replay.txt).  The torch restatement lives here
only: it is not on the product path.
usage: replay_per_bench.py [--tree ROOT] [--envs N[,N..]] [--obs state,pixels] [--batches B[,B..]] [--n-step K]
One process: a table on stdout, then one JSON line per case.  so100_touch_cube, episodes of 12 steps, the ring filled by
T + 8 random steps; T = 300 slots per env for state observations, 20 for 64 x 48 pixel observations (--state-T, --pixel-T).
After the fill the priorities of 16 batches of 65,536 sampled rows are updated from random |td| values, so the sums are not
those of equal priorities.  Every figure: 3 warm-up calls, then 6 blocks of 50 calls (20 where a call takes more than a
millisecond) back to back between two HIP events, divided by the calls; the median block is reported, the others are in
the JSON line.
  "push plain / per"        one push launch on the same arrays, without and with the priorities.
  "count scan", "priority scan"   so100_replay_scan, so100_replay_per_scan (two launches) alone.
  "kernel alone ..."        the sample launch alone into preallocated outputs (no scan, no allocation): plain, n-step,
                            and both with the prioritised pick.
  "scan + sample ..."       UniformReplay.sample(B) with the scans forced before it.
  "update_priorities"       UniformReplay.update_priorities on a sampled batch's env and slot (two launches).
  "torch ..."               per-env sums and a float64 cumsum, draws from torch's generator, searchsorted over the envs,
                            a cumsum and a comparison over the env's T slots, the gathers (images unshifted), probs and
                            weights; and for the update pow, a scatter of zeros and scatter_reduce(amax)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

BLOCKS = 6
GAMMA = 0.99


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_torch_per(torch, rp, g):
    """scan + so100_replay_sample_per and so100_replay_per_update as torch ops over the buffer's own arrays"""
    st, T, n, d = rp.store, rp.T, rp.n, rp.prio.device

    def sample(B, beta):
        prio = rp.prio.long() & 0xFFFFFFFF                                  # [T, n]
        c, k = st["meta"][0].long(), st["meta"][1].long()
        env_sum = prio.sum(0).double()
        prefix = torch.cumsum(env_sum, 0)
        r = torch.rand(B, dtype=torch.float64, device=d, generator=g) * prefix[-1]
        e = torch.searchsorted(prefix, r, right=True).clamp_(max=n - 1)
        rr = r - (prefix[e] - env_sum[e])
        j = torch.arange(T - 1, device=d)
        slots = (c[e][:, None] - k[e][:, None] + j) % T                      # [B, T - 1], oldest first
        q = prio[slots, e[:, None]] * (j < k[e][:, None])
        kidx = (torch.cumsum(q.double(), 1) <= rr[:, None]).sum(1).clamp_(max=T - 2)
        slot = slots.gather(1, kidx[:, None])[:, 0]
        probs = (q.gather(1, kidx[:, None])[:, 0].double() / prefix[-1]).float()
        w = (k.sum().float() * probs).pow(-beta)
        out = dict(actions=st["action"][slot, e], rewards=st["reward"][slot, e], dones=st["terminated"][slot, e].float(),
                   env=e.int(), slot=slot.int(), obs=st["obs"][slot, e], next_obs=st["next_obs"][slot, e], probs=probs,
                   weights=w / w.max())
        if rp.P:
            out["pixels"] = st["obs_img"][slot, e].view(B, *rp.image_shape)
            out["next_pixels"] = st["next_img"][slot, e].view(B, *rp.image_shape)
        return out

    def update(e, s, td):
        e, s = e.long(), s.long()
        c, k = st["meta"][0].long(), st["meta"][1].long()
        ok = ((s - (c[e] - k[e])) % T) < k[e]
        q = ((td.abs() + rp.eps).pow(rp.alpha) * 65536).round().clamp_(1, 4294967295).long()
        flat = (s * n + e)[ok]
        p = (rp.prio.long() & 0xFFFFFFFF).view(-1)
        p[flat] = 0
        p.scatter_reduce_(0, flat, q[ok], "amax")
        rp.prio.view(-1).copy_(p.int())                                      # (wraps past 2^31 as the stored bits do)
        rp.max_prio[0] = torch.maximum(rp.max_prio[0].long() & 0xFFFFFFFF, q[ok].max()).int()
    return sample, update


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
            T = args.pixel_T if pixels else args.state_T
            kw = dict(task="so100_touch_cube", max_episode_steps=12, seed=1)
            if pixels:
                kw.update(obs_type="so100_pixels_agent_pos", observation_width=64, observation_height=48)
            ur = dict(buffer_size=n * T, seed=5, n_step=args.n_step, gamma=GAMMA, prioritized=True)
            g = torch.Generator(device="cuda:0").manual_seed(3)
            env = SO100VecEnv(n, uniform_replay=ur, **kw)
            rp = env.uniform_replay
            env.reset()
            for _ in range(T + 8):
                env.step(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
            for _ in range(16):
                b = rp.sample(65536, augment=False)
                rp.update_priorities(b["env"], b["slot"], torch.rand(65536, device=env.device, generator=g).pow(4) * 10)
            tags = dict(n=n, T=T, obs=obs)
            P = rp.P
            rp._scan()
            print(f"{n} envs, {obs} observations{' (64 x 48 RGB)' if pixels else ''}, T = {T}, library {lib_hash}: "
                  f"{rp.size():,} valid transitions of {rp.capacity:,}, priority sum "
                  f"{int(rp.prio_sum[n].item()) / 65536:,.1f}, {4 * T * n / 1e6:.1f} MB of priorities")
            nrec, prec = rp._nstep, rp._per

            def without(fn, per=True, nstep=True):
                """fn on the launches of the same buffer without the priorities and / or the n-step record"""
                def call():
                    rp._per, rp._nstep = (prec if per else None), (nrec if nstep else None)
                    try:
                        return fn()
                    finally:
                        rp._per, rp._nstep = prec, nrec
                return call

            push = lambda: rp.after_step(env.actions)  # noqa: E731
            base = measure("push plain: so100_replay_push", without(push, per=False, nstep=False), **tags)
            basen = measure("push n-step: so100_replay_push_nstep", without(push, per=False), **tags)
            us = measure("push per: so100_replay_push_per (with the n-step record)", push, **tags)
            print(f"  push per - plain {us - base:+.2f} us, per - n-step {us - basen:+.2f} us")
            h, s = env._handle, env._stream()
            measure("count scan: so100_replay_scan", lambda: _native.check(
                env.lib.so100_replay_scan(h, ctypes.byref(rp._rec), s), "scan"), **tags)
            measure("priority scan: so100_replay_per_scan (two launches)", lambda: _native.check(
                env.lib.so100_replay_per_scan(h, ctypes.byref(rp._rec), ctypes.byref(prec), s), "per_scan"), **tags)
            torch_sample, torch_update = make_torch_per(torch, rp, g)

            def scan_sample(B):
                rp._dirty = True
                if rp._per is not None:
                    rp._per_dirty = True
                return rp.sample(B, augment=False)

            def direct(B, per, nstep):
                """the sample launch alone into preallocated outputs"""
                shape = {"obs": (B, NOBS), "next_obs": (B, NOBS), "actions": (B, rp.action_dim), "rewards": (B,),
                         "dones": (B,)}
                out = {k: torch.empty(*sh, device=env.device) for k, sh in shape.items()}
                out.update({k: torch.empty(B, dtype=torch.int32, device=env.device) for k in ("env", "slot")})
                out["shift"] = torch.empty(B, 4, dtype=torch.int32, device=env.device)
                if P:
                    out.update({k: torch.empty(B, P, dtype=torch.uint8, device=env.device)
                                for k in ("pixels", "next_pixels")})
                rec = _native.SO100ReplayOut(**{k: _native.ptr(t) for k, t in out.items()})
                more = {"discounts": torch.empty(B, device=env.device),
                        "nsteps": torch.empty(B, dtype=torch.int32, device=env.device),
                        "last_slot": torch.empty(B, dtype=torch.int32, device=env.device)}
                mrec = _native.SO100ReplayNstepOut(**{k: _native.ptr(t) for k, t in more.items()})
                pout = {k: torch.empty(B, device=env.device) for k in ("probs", "weights")}
                porec = _native.SO100ReplayPerOut(**{k: _native.ptr(t) for k, t in pout.items()})
                rp._scan()
                rp._rec.pad = 0
                R, ns = ctypes.byref(rp._rec), ctypes.byref(nrec)
                if per:
                    fn = lambda: env.lib.so100_replay_sample_per(  # noqa: E731
                        h, R, ctypes.byref(prec), ns if nstep else None, B, ctypes.c_uint64(7), ctypes.byref(rec),
                        ctypes.byref(mrec) if nstep else None, ctypes.byref(porec), s)
                elif nstep:
                    fn = lambda: env.lib.so100_replay_sample_nstep(h, R, ns, B, ctypes.c_uint64(7), ctypes.byref(rec),  # noqa: E731
                                                                   ctypes.byref(mrec), s)
                else:
                    fn = lambda: env.lib.so100_replay_sample(h, R, B, ctypes.c_uint64(7), ctypes.byref(rec), s)  # noqa: E731
                return (lambda: _native.check(fn(), "sample")), (out, more, pout)

            for B in args.batches:
                t = dict(tags, batch=B)
                alone = {}
                for per in (False, True):
                    for nstep in (False, True):
                        call, keep = direct(B, per, nstep)
                        name = ("per" if per else "uniform") + (f" n_step {args.n_step}" if nstep else "")
                        alone[per, nstep] = measure(f"kernel alone {name}, batch {B}", call, **t)
                print(f"  batch {B}: kernel alone per - uniform {alone[True, False] - alone[False, False]:+.2f} us, "
                      f"with n_step {alone[True, True] - alone[False, True]:+.2f} us")
                whole = measure(f"scan + sample uniform n_step {args.n_step}, batch {B}",
                                without(lambda: scan_sample(B), per=False), **t)
                us = measure(f"scans + sample per n_step {args.n_step}, batch {B}", lambda: scan_sample(B), **t)
                tor = measure(f"torch per sample: sums + cumsum + searchsorted + walk + gathers, batch {B}",
                              lambda: torch_sample(B, 0.4), **t)
                print(f"  batch {B}: scans + sample per - uniform {us - whole:+.2f} us, torch / hip {tor / us:.2f}x")
                b = rp.sample(B, augment=False)
                td = torch.rand(B, device=env.device, generator=g).pow(4) * 10
                up = measure(f"update_priorities, batch {B}", lambda: rp.update_priorities(b["env"], b["slot"], td), **t)
                tup = measure(f"torch update: pow + scatter + scatter_reduce(amax), batch {B}",
                              lambda: torch_update(b["env"], b["slot"], td), **t)
                print(f"  batch {B}: torch / hip update {tup / up:.2f}x")
                del keep, b
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
    ap.add_argument("--envs", default="8192,65536", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--obs", default="state,pixels", type=lambda s: s.split(","))
    ap.add_argument("--batches", default="256,65536", type=lambda s: [int(x) for x in s.split(",")])
    ap.add_argument("--n-step", default=3, type=int)
    ap.add_argument("--state-T", default=300, type=int)
    ap.add_argument("--pixel-T", default=20, type=int)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "gym-so100-c_amd"))
    main(a)
