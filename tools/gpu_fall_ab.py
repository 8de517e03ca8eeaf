#!/usr/bin/env python3
"""What a fall rule costs on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_fall_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--out profiles/fall_rule_ab.json]

Legs `rule_off` (no rule: the argument block carries the four words, the kernel skips the test) and `rule_tilt` (tilt 0.8 rad, which
never fires under this drive: the leg reports how many envs it ended, 0), interleaved R times, each run in a child process of its
own under `timeout -k 10 S`; the first run that fails ends the tool.  A run prints one JSON line: env-steps/s of K back-to-back
step() calls under an action table.  The parent then prints the medians and min-max spreads and writes them to --out.  The
difference separates the cost of evaluating the rule from the cost of carrying it (which bench.py against the parent commit
measures).  Information only: one machine, one session.  No threshold.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, RANGES = 4096, 4
LEGS = ["rule_off", "rule_tilt"]


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, fall={"tilt": 0.8} if name == "rule_tilt" else None)
    env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    acts = synthetic_actions(N, 0, warmup + steps, env.action_dim, env.device)
    for t in range(warmup):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"leg": name, "envs": N, "ranges": RANGES, "fall": env.engine.query("fall"), "timed_steps": steps,
           "env_steps_per_s": round(N * steps / dt), "envs_ended_by_the_rule": int((env.end_cause() != 0).sum().item()),
           "episodes_ended": env.solver_stats()["episodes_ended"]}
    print(json.dumps(out), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--out", default="", help="write the summary (JSON) here")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps, args.warmup)
        return 0
    runs = {name: [] for name in LEGS}
    for _ in range(args.repeats):
        for name in LEGS:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(f"{name}: exit status {p.returncode}; no further runs", flush=True)
                return p.returncode
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    rates = {k: [r["env_steps_per_s"] for r in v] for k, v in runs.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    out = {"workload": "flamingo_light_v1 x %d, flat, %d ranges, deferred join" % (N, RANGES), "timed_steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "summary": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in rates.items()},
           "envs_ended_by_the_rule": max(r["envs_ended_by_the_rule"] for r in runs["rule_tilt"]),
           "rule_cost_percent": round(100.0 * (1.0 - med["rule_tilt"] / med["rule_off"]), 2)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
