"""End-effector action prologue timings (profiles/ee_action.txt).
usage: ee_action_bench.py <tag>                    one process: JSON lines on stdout
       ee_action_bench.py --report <lines file>    the table of the collected lines on stdout
At 8,192 and 65,536 envs (CubeToBin, auto-reset, the benchmark's task), after 30 random ee_delta steps:
  kernel  HIP events around single so100_ee_action launches (3 warm-up, then 10 timed), random actions;
  rate    env steps/s of step_async_raw in ee_delta mode (prologue + so100_step + the reinit copy) against the bare
          so100_step launch (what joint mode's step_async_raw is) on the same trajectory: per block of 50 steps the joint
          actions are recorded once, then the block is run again from its start state in either mode (the joint one fed
          the recorded actions; both end in the recorded qpos bit for bit), 6 blocks, the order alternating, HIP events
          around each block.
Run it in 3 processes; --report pools them."""
import ctypes
import json
import statistics
import sys

SIZES = (8192, 65536)
REPS, BLOCKS, BLOCK_STEPS = 10, 6, 50


def measure(tag):
    import torch
    from gym_so100 import SO100VecEnv, _native
    P = _native.ptr
    for n in SIZES:
        env = SO100VecEnv(n, action_mode="ee_delta", autoreset=True, seed=1)
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(3)
        for _ in range(30):
            env.ee_actions.copy_(torch.rand(n, 5, device=env.device, generator=g) * 2 - 1)
            env.step_async_raw()
        torch.cuda.synchronize()

        def prologue():
            env.lib.so100_ee_action(env._handle, ctypes.byref(env._ee_ctrl), P(env.qpos), P(env.ee_actions),
                                    P(env.reinit), P(env.ee_joint_target), P(env.actions), P(env.ee_target),
                                    env._stream())

        def bare_step():
            env.lib.so100_step(env._handle, ctypes.byref(env._buf), env._flags, env._stream())

        def timed(fn, count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(3):
            prologue()
        torch.cuda.synchronize()
        ms = [round(timed(prologue, 1), 5) for _ in range(REPS)]
        print(json.dumps(dict(what="kernel", n=n, tag=tag, ms=ms, lib=_native.source_hash())), flush=True)
        # the same workload for both: record the block's joint actions (untimed), then from the block's start state time
        # the block in ee_delta mode and as bare steps fed the recorded actions (bit for bit the same trajectory)
        rec = torch.zeros(BLOCK_STEPS, n, 6, device=env.device)
        ee_rate, joint_rate, same = [], [], True

        def ee_block():
            for _ in range(BLOCK_STEPS):
                env.step_async_raw()

        def joint_block():
            for k in range(BLOCK_STEPS):
                env._buf.action = P(rec[k])
                bare_step()
            env._buf.action = P(env.actions)

        for blk in range(BLOCKS):
            env.ee_actions.copy_(torch.rand(n, 5, device=env.device, generator=g) * 2 - 1)
            start, flags = env.get_state(), env.reinit.clone()
            for k in range(BLOCK_STEPS):
                env.step_async_raw()
                rec[k].copy_(env.actions)
            end_qpos = env.qpos.clone()
            for fn, out in ((ee_block, ee_rate), (joint_block, joint_rate))[::1 if blk % 2 == 0 else -1]:
                env.set_state(**start)
                env.reinit.copy_(flags)
                torch.cuda.synchronize()
                out.append(round(n * BLOCK_STEPS / timed(fn, 1) * 1e3))
                same = same and bool(torch.equal(env.qpos, end_qpos))
        print(json.dumps(dict(what="rate", n=n, tag=tag, ee_delta=ee_rate, joint=joint_rate,
                              same_trajectory=same, lib=_native.source_hash())), flush=True)
        env.close()
        del env
        torch.cuda.empty_cache()


def report(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    for n in SIZES:
        k = [r for r in rows if r["what"] == "kernel" and r["n"] == n]
        pooled = [x for r in k for x in r["ms"]]
        if pooled:
            meds = " ".join("%.1f" % (statistics.median(r["ms"]) * 1e3) for r in k)
            print(f"so100_ee_action, {n:6d} envs: {len(k)} processes x {REPS} launches, process medians "
                  f"{meds} us; pooled median "
                  f"{statistics.median(pooled) * 1e3:.1f} us, min {min(pooled) * 1e3:.1f}, max {max(pooled) * 1e3:.1f}")
        r = [x for x in rows if x["what"] == "rate" and x["n"] == n]
        ee = [x for y in r for x in y["ee_delta"]]
        jt = [x for y in r for x in y["joint"]]
        if ee:
            me, mj = statistics.median(ee), statistics.median(jt)
            print(f"step_async_raw, {n:6d} envs: ee_delta median {me / 1e6:.3f} M env steps/s (min {min(ee) / 1e6:.3f}, "
                  f"max {max(ee) / 1e6:.3f}), bare so100_step {mj / 1e6:.3f} (min {min(jt) / 1e6:.3f}, max "
                  f"{max(jt) / 1e6:.3f}): {100 * (me / mj - 1):+.2f} %; every timed block ended in the recorded qpos bit "
                  f"for bit: {all(y.get('same_trajectory') for y in r)}")
    print("\nraw (one JSON line per process and case):")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    if sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        import os
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "gym-so100-c_amd"))
        measure(sys.argv[1])
