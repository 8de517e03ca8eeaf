#!/usr/bin/env python3
"""What failure traces cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_ftrace_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Legs `off`, `ledger_4` (the yardstick: one small launch per range and step, BatchedEnv(ledger=4)) and `ftrace_50_2`
(BatchedEnv(failure_traces=(50, 2))), interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the first
run that fails ends the tool.  A run prints one JSON line: env-steps/s of K back-to-back step() calls under an action table, and for
`ftrace_50_2` the frame size, the bytes the recorder writes per env-step (4 F for the frame: the outcome part behind the step, the
state part of the next frame), the buffer bytes and the time of one BatchedEnv.failure_traces() read.  The parent then prints the
medians and min-max spreads.  Information only: one machine, one session; no threshold.
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
FRAMES, KEEP = 50, 2
LEGS = ["off", "ledger_4", "ftrace_50_2"]


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, ledger=4 if name == "ledger_4" else None,
                     failure_traces=(FRAMES, KEEP) if name == "ftrace_50_2" else False)
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
    out = {"leg": name, "envs": N, "ranges": RANGES, "ledger_slots": env.engine.query("ledger_slots"),
           "ftrace_frames": env.engine.query("ftrace_frames"), "timed_steps": steps, "env_steps_per_s": round(N * steps / dt)}
    if name == "ftrace_50_2":
        F = env.engine.query("ftrace_frame_words")
        out["frame_words"], out["bytes_per_env_step"] = F, 4 * (4 + env.nq + env.nv + env.action_dim + env.command_dim + env.info_dim)
        out["buffer_bytes"] = 4 * N * (KEEP + 1) * (16 + FRAMES * F)
        t0 = time.perf_counter()
        tr = env.failure_traces(include_open=True)
        out["read_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        out["summary"] = tr.summary()
    print(json.dumps(out), flush=True)
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
    rates, runs = {name: [] for name in LEGS}, []
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
            rates[name].append(runs[-1]["env_steps_per_s"])
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    summary = {"summary": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in rates.items()},
               "ledger_cost_percent": round(100.0 * (1.0 - med["ledger_4"] / med["off"]), 2),
               "ftrace_cost_percent": round(100.0 * (1.0 - med["ftrace_50_2"] / med["off"]), 2)}
    print(json.dumps(summary), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 4 ranges, deferred join", "steps": args.steps, "warmup": args.warmup,
                       "runs": runs, **summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
