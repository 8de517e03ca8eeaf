#!/usr/bin/env python3
"""What latency lines cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join), against the
same scenario table stripped of its latency:

    python tools/gpu_latency_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Legs, interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the first run that fails ends the tool:
  table     one scenario with a command keyframe and no latency: scenario_step_kernel ahead of the step, nothing behind it
  latency   the same scenario with two latency items: every command two control steps late (latency_act_kernel ahead of the step;
            the observation has last_action, so actfault_obs_kernel behind it) and the IMU's ang_vel one step late plus 0..2 steps
            of jitter (latency_obs_kernel behind the step)
A run prints one JSON line: the seconds and env-steps/s of K back-to-back step() calls under an action table.  The parent then prints
the medians, the min-max spreads and the cost per step of the latency leg over the table leg.  Information only: one machine, one
session; no threshold.
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
LEGS = ["table", "latency"]
LATENCY = [[0, 1 << 29, "action", "*", 2], [0, 1 << 29, "ang_vel", "*", 1, 2]]


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    cfg = workload_config("light_flat", N)
    scn = [{"commands": [[0, 0.5, 0.0, 0.0, 0.0]], **({"latency": LATENCY} if name == "latency" else {})}]
    env = BatchedEnv(cfg, num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES, deferred_join=True, failure_traces=False,
                     scenarios=scn)
    env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    acts = synthetic_actions(N, 0, warmup + steps, env.action_dim, env.device)   # a table: every step's action rows outlive the step
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
    print(json.dumps({"leg": name, "envs": N, "ranges": RANGES, "latency_items": env.engine.query("latency"), "latency_depth": env.engine.query("latency_depth"),
                      "timed_steps": steps, "seconds": round(dt, 6), "env_steps_per_s": round(N * steps / dt)}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--json", default=None, help="also write the runs and the summary here")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps, args.warmup)
        return 0
    secs, runs = {name: [] for name in LEGS}, []
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
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            secs[name].append(runs[-1]["seconds"])
    med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
    summary = {"summary": {k: {"median_s": med[k], "min_s": min(v), "max_s": max(v), "median_env_steps_per_s": round(N * args.steps / med[k]),
                               "spread_percent": round(100.0 * (max(v) - min(v)) / med[k], 2)} for k, v in secs.items()},
               "latency_us_per_step": round(1e6 * (med["latency"] - med["table"]) / args.steps, 2),
               "latency_over_table_percent": round(100.0 * (med["latency"] / med["table"] - 1.0), 2)}
    print(json.dumps(summary), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 4 ranges, deferred join; two latency items (all actions 2 steps, ang_vel 1 + 0..2 steps)",
                       "steps": args.steps, "warmup": args.warmup, "runs": runs, **summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
