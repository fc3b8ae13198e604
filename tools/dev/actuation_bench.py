"""Actuation prologue and physical-randomisation sampler timings, and the default env's A/B (profiles/actuation.txt).
usage: actuation_bench.py kernel <tag>                    one process: JSON lines on stdout
       actuation_bench.py ab <tag> <label> [<package dir>] one process: the default env's step rate with the package in
                                                          <package dir> (default: this tree's), JSON lines on stdout
       actuation_bench.py --report <lines file>           the table of the collected lines on stdout
At 8,192 and 65,536 envs (CubeToBin, auto-reset, the benchmark's task):
  kernel  an env with per_episode and every actuation range on, after 30 random steps: HIP events around single
          so100_actuate launches and single so100_dr_sample launches as a step makes them (masks terminated / truncated;
          and once over every env, as a full reset makes it), 3 warm-up then 10 timed each;
  ab      a default env (no randomisation, joint mode): env steps/s of step_async_raw, 6 blocks of 50 steps between HIP
          events after 30 warm-up steps, the same seeds and actions in every process.  Run it alternately on this tree
          and on a checkout of the parent commit built beside it; the trajectories are the same, so the rates compare.
Run each in 3 processes; --report pools them.  The lines of `bench.py --steps 300 --warmup 30` of the same box may be
appended to the lines file: the report then prints the kernels as a share of that env step."""
import ctypes
import json
import os
import statistics
import sys

SIZES = (8192, 65536)
REPS, BLOCKS, BLOCK_STEPS = 10, 6, 50
EE_US = {8192: 13.1, 65536: 14.5}          # so100_ee_action's recorded medians (profiles/ee_action.txt)
SPREAD = 0.4                                # % run-to-run spread of the parent's bench line (profiles/r06_bench_repeats.txt)
ACTUATION = dict(delay=(0, 7), smoothing=(0.3, 1.0), rate=(0.05, 2.0))


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel(tag):
    import torch
    from gym_so100 import SO100VecEnv, _native
    P = _native.ptr
    for n in SIZES:
        env = SO100VecEnv(n, autoreset=True, seed=1, domain_randomization=dict(per_episode=True, actuation=ACTUATION))
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(3)
        for _ in range(30):
            env.act_command.copy_(torch.rand(n, 6, device=env.device, generator=g) * 2.4 - 1.2)
            env.step_async_raw()
        torch.cuda.synchronize()

        def actuate():
            env.lib.so100_actuate(env._handle, P(env.qpos), P(env.act_command), P(env.reinit), P(env.act_params),
                                  P(env.act_hist), P(env.act_head), P(env.actions), env._stream())

        def sample(masked):
            def launch():
                env.lib.so100_dr_sample(env._handle, ctypes.byref(env._dr_ranges), P(env.episode),
                                        P(env.terminated) if masked else None, P(env.truncated) if masked else None,
                                        P(env.dr_params), P(env.act_params), env._stream())
            return launch

        for what, fn in (("so100_actuate", actuate), ("so100_dr_sample (a step's masks)", sample(True)),
                         ("so100_dr_sample (every env)", sample(False))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = [round(timed(torch, fn, 1), 5) for _ in range(REPS)]
            print(json.dumps(dict(what="kernel", kernel=what, n=n, tag=tag, ms=ms, lib=_native.source_hash())),
                  flush=True)
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
            for _ in range(BLOCK_STEPS):
                env.step_async_raw()

        rate = [round(n * BLOCK_STEPS / timed(torch, block, 1) * 1e3) for _ in range(BLOCKS)]
        print(json.dumps(dict(what="ab", label=label, n=n, tag=tag, rate=rate, qpos_sum=float(env.qpos.double().sum()),
                              lib=_native.source_hash())), flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()


def report(path):
    rows, bench = [], {}
    for line in open(path):
        if not line.startswith("{"):
            continue
        r = json.loads(line)
        if "what" in r:
            rows.append(r)
        elif "roofline" in r or "value" in r:          # a bench.py line
            n, v = r.get("config", {}).get("envs_total"), r.get("value")
            if n and v:
                bench[int(n)] = float(v)
    for n, v in sorted(bench.items()):
        print(f"bench.py --gpus 1 --total-envs {n:6d} --steps 300 --warmup 30: {v / 1e6:.3f} M env steps/s, "
              f"{n / v * 1e6:.1f} us per step")
    for n in SIZES:
        for name in sorted({r["kernel"] for r in rows if r["what"] == "kernel"}):
            k = [r for r in rows if r["what"] == "kernel" and r["n"] == n and r["kernel"] == name]
            pooled = [x for r in k for x in r["ms"]]
            if not pooled:
                continue
            med = statistics.median(pooled) * 1e3
            meds = " ".join("%.1f" % (statistics.median(r["ms"]) * 1e3) for r in k)
            share = f"; {100 * med / (n / bench[n] * 1e6):.2f} % of the env step" if n in bench else ""
            print(f"{name}, {n:6d} envs: {len(k)} processes x {REPS} launches, process medians {meds} us; pooled median "
                  f"{med:.1f} us, min {min(pooled) * 1e3:.1f}, max {max(pooled) * 1e3:.1f} (so100_ee_action: "
                  f"{EE_US[n]} us){share}")
        a = {lab: [x for r in rows if r["what"] == "ab" and r["n"] == n and r["label"] == lab for x in r["rate"]]
             for lab in ("this", "parent")}
        if a["this"] and a["parent"]:
            mt, mp = statistics.median(a["this"]), statistics.median(a["parent"])
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
