#!/usr/bin/env python3
"""What the episode ledger costs on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_ledger_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S]

Legs `ledger_off` and `ledger_4` (BatchedEnv(ledger=4)), interleaved R times, each run in a child process of its own under
`timeout -k 10 S`; the first run that fails ends the tool.  A run prints one JSON line: env-steps/s of K back-to-back step() calls
under an action table, and for `ledger_4` the ledger's episode count and the time of one BatchedEnv.ledger() read.  The parent then
prints the medians and min-max spreads.  Information only: one machine, one session; no threshold.
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
LEGS = ["ledger_off", "ledger_4"]


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    slots = 4 if name == "ledger_4" else None
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, ledger=slots)
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
    out = {"leg": name, "envs": N, "ranges": RANGES, "ledger_slots": env.engine.query("ledger_slots"), "timed_steps": steps,
           "env_steps_per_s": round(N * steps / dt)}
    if slots:
        t0 = time.perf_counter()
        led = env.ledger()
        out["ledger_read_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        out["episodes"], out["lost"] = len(led), int(led.lost.sum())
        out["episodes_ended_meta"] = env.solver_stats()["episodes_ended"]
    print(json.dumps(out), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps, args.warmup)
        return 0
    rates = {name: [] for name in LEGS}
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
            rates[name].append(json.loads(p.stdout.strip().splitlines()[-1])["env_steps_per_s"])
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    print(json.dumps({"summary": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in rates.items()},
                      "ledger_cost_percent": round(100.0 * (1.0 - med["ledger_4"] / med["ledger_off"]), 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
