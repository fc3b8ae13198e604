"""Timings of the hindsight replay buffer's launches beside the same operations written as torch ops on the device
(profiles/her_replay.txt).  The torch restatement lives here only: it is not on the product path.
usage: her_bench.py kernel <tag>            one process: JSON lines on stdout
       her_bench.py --report <lines file>   the table of the collected lines (and of bench.py's lines in it) on stdout
At 8,192 and 65,536 envs, GoalEnv, T = 300 slots per env, episodes capped at 20 steps, after 60 random steps (every env
holds closed episodes):
  "hip push"     HerReplay.after_step (one so100_her_push): 3 warm-up then 10 timed single calls between HIP events, then 6
                 blocks of 50 calls back to back (what a training loop sees: launches overlap the host's enqueue).
  "hip sample"   HerReplay.sample(B) with the scan forced before it (a push happened), B = 256 and 65,536: so100_her_scan,
                 so100_her_sample and the allocation of the twelve output tensors; and sample alone (no push since).
  "torch ..."    the same operations as torch ops on the same arrays, no host synchronisation, timed the same way.
  "step"         step_async_raw of a default GoalEnv of the same size, the yardstick of each share.
Run it in 3 processes; --report pools them."""
import json
import os
import statistics
import sys

SIZES = (8192, 65536)
T, CAP = 300, 20
BATCHES = (256, 65536)
REPS, BLOCKS, BLOCK_CALLS = 10, 6, 50


def timed(torch, fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_push(torch, env, st, ar):
    """so100_her_push's rules as torch ops over the buffer's own arrays"""
    lo, count, open_len = st["meta"][0].long(), st["meta"][1].long(), st["meta"][2].long()
    full = count + open_len == T
    L = st["length"][lo, ar].long().clamp(min=1)
    evict = full & (count > 0)
    lo = torch.where(evict, (lo + L) % T, lo)
    count = torch.where(evict, count - L, count)
    open_len = torch.where(full & ~evict, torch.zeros_like(open_len), open_len)
    cur = (lo + count + open_len) % T
    fin = env.terminated | env.truncated
    st["obs"][cur, ar] = st["stage_obs"]
    st["next_obs"][cur, ar] = torch.where(fin[:, None], env.final_obs, env.obs)
    st["goal"][cur, ar] = st["stage_goal"]
    st["action"][cur, ar] = env.actions
    st["reward"][cur, ar] = env.reward
    st["terminated"][cur, ar] = env.terminated.to(torch.uint8)
    st["offset"][cur, ar] = open_len.int()
    open_len = open_len + 1
    first = (cur - (open_len - 1)) % T
    close = fin & ~env.diverged
    st["length"][first, ar] = torch.where(close, open_len.int(), st["length"][first, ar])
    count = torch.where(close, count + open_len, count)
    open_len = torch.where(fin | env.diverged, torch.zeros_like(open_len), open_len)
    st["meta"][0].copy_(lo)
    st["meta"][1].copy_(count)
    st["meta"][2].copy_(open_len)
    st["stage_obs"].copy_(env.obs)
    st["stage_goal"].copy_(env.desired_goal)


def torch_sample(torch, env, st, B, nrel, threshold, g):
    """so100_her_scan + so100_her_sample ("future") as torch ops; the draws are torch's own generator"""
    lo, count = st["meta"][0].long(), st["meta"][1].long()
    prefix = torch.cumsum(count, 0)
    total = prefix[-1]
    r = (torch.rand(B, dtype=torch.float64, device=env.device, generator=g) * total).long()
    e = torch.searchsorted(prefix, r, right=True).clamp_(max=count.shape[0] - 1)
    slot = (lo[e] + r - (prefix[e] - count[e])) % T
    off = st["offset"][slot, e].long()
    first = (slot - off) % T
    ln = st["length"][first, e].long()
    j = off + (torch.rand(B, dtype=torch.float64, device=env.device, generator=g) * (ln - off)).long()
    gslot = (first + j) % T
    obs, nxt = st["obs"][slot, e], st["next_obs"][slot, e]
    rel = torch.arange(B, device=env.device) < nrel
    goal = torch.where(rel[:, None], st["next_obs"][gslot, e, 0:3], st["goal"][slot, e])
    dist = torch.linalg.norm(nxt[:, 0:3] - goal, dim=1)
    reward = torch.where(rel, torch.where(dist < threshold, 0.0, -1.0).float(), st["reward"][slot, e])
    return dict(observation=obs, achieved_goal=obs[:, 0:3].contiguous(), desired_goal=goal, next_observation=nxt,
                next_achieved_goal=nxt[:, 0:3].contiguous(), next_desired_goal=goal.clone(),
                actions=st["action"][slot, e], rewards=reward, dones=st["terminated"][slot, e].float(),
                env=e.int(), slot=slot.int(), goal_slot=torch.where(rel, gslot, -torch.ones_like(gslot)).int())


def kernel(tag):
    import torch
    from gym_so100 import SO100VecEnv, _native

    def emit(n, what, single, blocks, unit_calls):
        print(json.dumps(dict(what="kernel", n=n, tag=tag, name=what, single_ms=single,
                              block_ms_per_call=[round(b / unit_calls, 6) for b in blocks],
                              lib=_native.source_hash())), flush=True)

    def measure(n, what, fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        single = [round(timed(torch, fn, 1), 5) for _ in range(REPS)]
        blocks = [timed(torch, fn, BLOCK_CALLS) for _ in range(BLOCKS)]
        emit(n, what, single, blocks, BLOCK_CALLS)

    for n in SIZES:
        env = SO100VecEnv(n, task="so100_goal", seed=1, max_episode_steps=CAP, replay=dict(buffer_size=n * T, seed=5))
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(3)
        for _ in range(3 * CAP):
            env.step(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
        rp = env.replay
        valid = rp.size()
        print(json.dumps(dict(what="fill", n=n, tag=tag, valid=valid, capacity=rp.capacity)), flush=True)

        def scan_sample(B):
            rp._dirty = True
            return rp.sample(B)
        st = rp.store
        ar = torch.arange(n, device=env.device)
        thr = float(env.model.goal_threshold)
        # the samples first, on the buffer as 60 steps left it; the pushes (the same transition again and again) after
        for B in BATCHES:
            measure(n, f"hip sample: scan + sample, batch {B}", lambda: scan_sample(B))
            measure(n, f"hip sample: sample alone, batch {B}", lambda: rp.sample(B))
            nrel = int(rp.her_ratio * B)
            measure(n, f"torch sample: cumsum + draws + gathers, batch {B}",
                    lambda: torch_sample(torch, env, st, B, nrel, thr, g))
        measure(n, "hip push: so100_her_push", lambda: rp.after_step(env.actions))
        measure(n, "torch push: the same rules as device ops", lambda: torch_push(torch, env, st, ar))
        env.close()
        del env, rp, st
        torch.cuda.empty_cache()
        env = SO100VecEnv(n, task="so100_goal", seed=1, max_episode_steps=CAP)
        env.reset()
        env.actions.copy_(torch.rand(n, 6, device=env.device, generator=g) * 2 - 1)
        for _ in range(30):
            env.step_async_raw()
        torch.cuda.synchronize()
        blocks = [timed(torch, env.step_async_raw, BLOCK_CALLS) for _ in range(BLOCKS)]
        emit(n, "step: a default GoalEnv's step_async_raw", [], blocks, BLOCK_CALLS)
        env.close()
        del env
        torch.cuda.empty_cache()


def report(path):
    lines = [line.strip() for line in open(path)]
    rows = [json.loads(x) for x in lines if x.startswith("{") and '"what"' in x]
    med = statistics.median
    for n in SIZES:
        k = [r for r in rows if r["what"] == "kernel" and r["n"] == n]
        fill = [r for r in rows if r["what"] == "fill" and r["n"] == n]
        step = [x for r in k if r["name"].startswith("step:") for x in r["block_ms_per_call"]]
        step_us = med(step) * 1e3 if step else None
        if step_us:
            print(f"GoalEnv, {n:6d} envs, T = {T} ({fill[0]['valid']:,} valid of {fill[0]['capacity']:,} slots): a default "
                  f"env's step_async_raw {step_us:.1f} us per step (median of {len(step)} blocks of {BLOCK_CALLS})")
        names = []
        for r in k:
            if r["name"] not in names and not r["name"].startswith("step:"):
                names.append(r["name"])
        pooled = {}
        for name in names:
            rs = [r for r in k if r["name"] == name]
            single = [x for r in rs for x in r["single_ms"]]
            block = [x for r in rs for x in r["block_ms_per_call"]]
            pooled[name] = med(block) * 1e3
            line = f"  {name}: single calls median {med(single) * 1e3:.1f} us (min {min(single) * 1e3:.1f}, max " \
                   f"{max(single) * 1e3:.1f}; {len(rs)} processes x {REPS}); back to back {med(block) * 1e3:.1f} us per call"
            if step_us:
                line += f" = {100 * med(block) * 1e3 / step_us:.2f} % of the env step"
            print(line)
        pairs = [("hip push: so100_her_push", "torch push: the same rules as device ops")] + \
                [(f"hip sample: scan + sample, batch {B}", f"torch sample: cumsum + draws + gathers, batch {B}")
                 for B in BATCHES]
        for h, t in pairs:
            if h in pooled and t in pooled:
                print(f"  ratio torch / hip, back to back, {h.split(':')[0]}{h.split(',')[-1] if ',' in h else ''}: "
                      f"{pooled[t] / pooled[h]:.2f}x")
    bench = [json.loads(x.split(" ", 1)[1]) | {"label": x.split(" ", 1)[0]} for x in lines
             if x.startswith(("this {", "parent {"))]
    if bench:
        field = next((f for f in ("env_steps_per_sec", "steps_per_sec", "value", "throughput") if f in bench[0]), None)
        if field:
            a = {lab: [b[field] for b in bench if b["label"] == lab] for lab in ("this", "parent")}
            if a["this"] and a["parent"]:
                mt, mp = med(a["this"]), med(a["parent"])
                print(f"\nbench.py --gpus 1 --steps 300 --warmup 30, alternating processes, {field}: this tree median "
                      f"{mt:,.0f} (min {min(a['this']):,.0f}, max {max(a['this']):,.0f}; {len(a['this'])} runs), parent "
                      f"{mp:,.0f} (min {min(a['parent']):,.0f}, max {max(a['parent']):,.0f}; {len(a['parent'])} runs): "
                      f"{100 * (mt / mp - 1):+.2f} %; the parent's own spread (max - min) / median "
                      f"{100 * (max(a['parent']) - min(a['parent'])) / mp:.2f} %")
    print("\nraw (one JSON line per process and case):")
    for x in lines:
        if x.startswith(("{", "this {", "parent {")):
            print(x)


if __name__ == "__main__":
    if sys.argv[1] == "--report":
        report(sys.argv[2])
    else:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path.insert(0, os.path.abspath(os.path.join(here, "..", "..", "gym-so100-c_amd")))
        kernel(sys.argv[2])
