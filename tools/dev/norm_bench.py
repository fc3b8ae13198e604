"""Timings of the running normaliser's launches, beside the same arithmetic as torch ops on the device and as float64
numpy on the host, and the default env's A/B (profiles/normalize.txt).
usage: norm_bench.py kernel <tag>                        one process: JSON lines on stdout
       norm_bench.py ab <tag> <label> [<package dir>]    one process: the default env's step rate with the package in
                                                         <package dir> (default: this tree's), JSON lines on stdout
       norm_bench.py --report <lines file>               the table of the collected lines on stdout
At 8,192 and 65,536 envs, for the state env (CubeToBin, [N,15]) and the GoalEnv (three keys, 21 columns), auto-reset,
normalize=dict(reward=True) (every launch the option can make), after 30 random steps:
  kernel  "hip": HIP events around what one step adds (Normalizer.after_step: update, apply, the masked apply of the
          final observation, the three launches of the return path), 3 warm-up then 10 timed single calls, then 6 blocks
          of 50 calls back to back (the figure a training loop sees: launches overlap the host's enqueue); and each entry
          point alone the same way.  "torch": the same float64 arithmetic as torch ops on the device, no host
          synchronisation (the count is a device scalar), timed the same way.  "numpy": tests/norm_ref.py's
          VecNormalizeRef.step on host arrays of the same shapes, perf_counter, 3 warm-up then 10 timed (what SB3's
          VecNormalize costs per step, the copies to and from the device not counted).  "step": step_async_raw of a
          default env, 6 blocks of 50 steps, the yardstick of each launch's share.
  ab      a default env (normalize=None): env steps/s of step_async_raw, 6 blocks of 50 steps between HIP events after
          30 warm-up steps, the same seeds and actions in every process.  Run it alternately on this tree and on a
          checkout of the parent commit built beside it; the trajectories are the same, so the rates compare.
Run each in 3 processes; --report pools them."""
import ctypes
import json
import os
import statistics
import sys
import time

SIZES = (8192, 65536)
KINDS = (("state", "so100_cube_to_bin"), ("goal", "so100_goal"))
REPS, BLOCKS, BLOCK_CALLS = 10, 6, 50
SPREAD = 0.4                                # % run-to-run spread of the parent's bench line (profiles/r06_bench_repeats.txt)
OPTS = dict(reward=True)


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_step(torch, env, st):
    """one step's normalisation as torch ops in float64 on the device: st = dict(keys=[(src, out, final_src, final_out)],
    mean/var/count per key, ret, ret_mean/var/count, reward_norm)"""
    eps, clip = 1e-8, 10.0
    done = env.terminated | env.truncated
    for k in st["keys"]:
        x = k["src"].double()
        b = x.shape[0]
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        delta, tot = bm - k["mean"], k["count"] + b
        k["var"] = (k["var"] * k["count"] + bv * b + delta * delta * k["count"] * b / tot) / tot
        k["mean"] = k["mean"] + delta * b / tot
        k["count"] = tot
        sd = torch.sqrt(k["var"] + eps)
        k["out"].copy_(((x - k["mean"]) / sd).clamp_(-clip, clip))
        if k["final_src"] is not None:
            f = ((k["final_src"].double() - k["mean"]) / sd).clamp_(-clip, clip).float()
            torch.where(done[:, None], f, k["final_out"], out=k["final_out"])
    r = env.reward.double()
    st["ret"].mul_(0.99).add_(r)
    g = st["ret"]
    b = g.shape[0]
    bm, bv = g.mean(), g.var(unbiased=False)
    delta, tot = bm - st["ret_mean"], st["ret_count"] + b
    st["ret_var"] = (st["ret_var"] * st["ret_count"] + bv * b + delta * delta * st["ret_count"] * b / tot) / tot
    st["ret_mean"] = st["ret_mean"] + delta * b / tot
    st["ret_count"] = tot
    st["reward_norm"].copy_((r / torch.sqrt(st["ret_var"] + eps)).clamp_(-clip, clip))
    st["ret"].masked_fill_(done, 0.0)


def torch_state(torch, env):
    d, n = env.device, env.num_envs
    f64 = torch.float64
    keys = []
    for name, src, off, dim in env._norm.keys:
        keys.append(dict(src=src[:, off:off + dim], out=torch.zeros(n, dim, device=d), mean=torch.zeros(dim, dtype=f64, device=d),
                         var=torch.ones(dim, dtype=f64, device=d), count=torch.full((), 1e-4, dtype=f64, device=d),
                         final_src=None, final_out=None))
    keys[0]["final_src"] = env.final_obs
    keys[0]["final_out"] = torch.zeros(n, keys[0]["src"].shape[1], device=d)
    one = lambda v: torch.full((), v, dtype=f64, device=d)
    return dict(keys=keys, ret=torch.zeros(n, dtype=f64, device=d), ret_mean=one(0.0), ret_var=one(1.0),
                ret_count=one(1e-4), reward_norm=torch.zeros(n, device=d))


def kernel(tag):
    import torch
    from gym_so100 import SO100VecEnv, _native
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
    import norm_ref
    P = _native.ptr

    def emit(n, kind, what, single, blocks, unit_calls):
        print(json.dumps(dict(what="kernel", kind=kind, n=n, tag=tag, name=what, single_ms=single,
                              block_ms_per_call=[round(b / unit_calls, 6) for b in blocks],
                              lib=_native.source_hash())), flush=True)

    def measure(n, kind, what, fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        single = [round(timed(torch, fn, 1), 5) for _ in range(REPS)]
        blocks = [timed(torch, fn, BLOCK_CALLS) for _ in range(BLOCKS)]
        emit(n, kind, what, single, blocks, BLOCK_CALLS)

    for n in SIZES:
        for kind, task in KINDS:
            env = SO100VecEnv(n, task=task, autoreset=True, seed=1, normalize=OPTS)
            env.reset()
            g = torch.Generator(device=env.device).manual_seed(3)
            for _ in range(30):
                env.actions.copy_(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
                env.step_async_raw()
            torch.cuda.synchronize()
            nm, s = env._norm, env._stream()
            p = nm._p
            measure(n, kind, "hip: all launches of a step", nm.after_step)
            measure(n, kind, "hip: so100_norm_update", lambda: env.lib.so100_norm_update(
                env._handle, ctypes.byref(nm._norm), n, None, p["stats"], p["work"], s))
            measure(n, kind, "hip: so100_norm_apply", lambda: env.lib.so100_norm_apply(
                env._handle, ctypes.byref(nm._norm), n, None, p["stats"], s))
            measure(n, kind, "hip: so100_norm_apply (final observation, done mask)", lambda: env.lib.so100_norm_apply(
                env._handle, ctypes.byref(nm._final), n, p["done"], p["stats"], s))
            measure(n, kind, "hip: so100_norm_return", lambda: env.lib.so100_norm_return(
                env._handle, ctypes.byref(nm._ret_args[True]), n, P(env.reward), P(env.terminated), P(env.truncated),
                p["ret"], p["ret_stats"], p["work"], p["reward_norm"], s))
            st = torch_state(torch, env)
            measure(n, kind, "torch: the same arithmetic as device ops", lambda: torch_step(torch, env, st))
            # the host restatement over arrays of the same shapes
            keys = {name: dim for name, _, _, dim in nm.keys}
            ref = norm_ref.VecNormalizeRef(keys, n, reward=True, record=False)
            raw = {name: src[:, off:off + dim].cpu().numpy() for name, src, off, dim in nm.keys}
            first = nm.keys[0][0]
            final = {first: env.final_obs[:, :keys[first]].cpu().numpy()}
            rew, term, trunc = env.reward.cpu().numpy(), env.terminated.cpu().numpy(), env.truncated.cpu().numpy()
            host = []
            for i in range(3 + REPS):
                t0 = time.perf_counter()
                ref.step(raw, rew, term, trunc, final=final)
                if i >= 3:
                    host.append(round((time.perf_counter() - t0) * 1e3, 5))
            emit(n, kind, "numpy: tests/norm_ref.py on the host", host, [], 1)
            env.close()
            del env
            torch.cuda.empty_cache()
            # the yardstick: a default env's step
            env = SO100VecEnv(n, task=task, autoreset=True, seed=1)
            env.reset()
            env.actions.copy_(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
            for _ in range(30):
                env.step_async_raw()
            torch.cuda.synchronize()
            blocks = [timed(torch, env.step_async_raw, BLOCK_CALLS) for _ in range(BLOCKS)]
            emit(n, kind, "step: a default env's step_async_raw", [], blocks, BLOCK_CALLS)
            env.close()
            del env
            torch.cuda.empty_cache()


def ab(tag, label):
    import torch
    from gym_so100 import SO100VecEnv, _native
    for n in SIZES:
        env = SO100VecEnv(n, autoreset=True, seed=1)
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(3)
        env.actions.copy_(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
        for _ in range(30):
            env.step_async_raw()
        torch.cuda.synchronize()

        def block():
            for _ in range(BLOCK_CALLS):
                env.step_async_raw()

        rate = [round(n * BLOCK_CALLS / timed(torch, block, 1) * 1e3) for _ in range(BLOCKS)]
        print(json.dumps(dict(what="ab", label=label, n=n, tag=tag, rate=rate, qpos_sum=float(env.qpos.double().sum()),
                              lib=_native.source_hash())), flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()


def report(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{") and '"what"' in line]
    med = statistics.median
    for n in SIZES:
        for kind, _ in KINDS:
            k = [r for r in rows if r["what"] == "kernel" and r["n"] == n and r["kind"] == kind]
            step = [x for r in k if r["name"].startswith("step:") for x in r["block_ms_per_call"]]
            step_us = med(step) * 1e3 if step else None
            if step_us:
                print(f"{kind} env, {n:6d} envs: a default env's step_async_raw {step_us:.1f} us per step "
                      f"(median of {len(step)} blocks of {BLOCK_CALLS})")
            names = []
            for r in k:
                if r["name"] not in names and not r["name"].startswith("step:"):
                    names.append(r["name"])
            for name in names:
                rs = [r for r in k if r["name"] == name]
                single = [x for r in rs for x in r["single_ms"]]
                block = [x for r in rs for x in r["block_ms_per_call"]]
                line = f"  {name}: single calls median {med(single) * 1e3:.1f} us (min {min(single) * 1e3:.1f}, max " \
                       f"{max(single) * 1e3:.1f}; {len(rs)} processes x {REPS})"
                if block:
                    line += f"; back to back {med(block) * 1e3:.1f} us per call"
                    if step_us:
                        line += f" = {100 * med(block) * 1e3 / step_us:.2f} % of the env step"
                print(line)
        a = {lab: [x for r in rows if r["what"] == "ab" and r["n"] == n and r["label"] == lab for x in r["rate"]]
             for lab in ("this", "parent")}
        if a["this"] and a["parent"]:
            mt, mp = med(a["this"]), med(a["parent"])
            sums = {r["qpos_sum"] for r in rows if r["what"] == "ab" and r["n"] == n}
            d = 100 * (mt / mp - 1)
            print(f"default env step_async_raw, {n:6d} envs: this tree median {mt / 1e6:.3f} M env steps/s (min "
                  f"{min(a['this']) / 1e6:.3f}, max {max(a['this']) / 1e6:.3f}), parent {mp / 1e6:.3f} (min "
                  f"{min(a['parent']) / 1e6:.3f}, max {max(a['parent']) / 1e6:.3f}): {d:+.2f} % "
                  f"({'inside' if abs(d) <= SPREAD else 'OUTSIDE'} the parent's {SPREAD} % run-to-run spread); "
                  f"every process ended in the same state: {len(sums) == 1}")
    print("\nraw (one JSON line per process and case):")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    if sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        here = os.path.dirname(os.path.abspath(__file__))
        pkg = sys.argv[4] if len(sys.argv) > 4 else os.path.join(here, "..", "..", "gym-so100-c_amd")
        sys.path.insert(0, os.path.abspath(pkg))
        if sys.argv[1] == "kernel":
            kernel(sys.argv[2])
        else:
            ab(sys.argv[2], sys.argv[3])
