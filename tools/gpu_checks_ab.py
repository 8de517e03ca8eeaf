#!/usr/bin/env python3
"""What scenario checks cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_checks_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Legs `off`, `ledger_4` (the yardstick: one small launch per range and step, BatchedEnv(ledger=4)), `ledger_4_table` (the ledger and a
scenario table of four rows whose checks are not armed: what the table itself costs) and `ledger_4_checks_8` (the same table with its 8
checks per scenario armed, check_slots=4), interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the
first run that fails ends the tool.  A run prints one JSON line: env-steps/s of K back-to-back step() calls under an action table, and
for the checks leg the record size, the accumulator and ring bytes, the time of one BatchedEnv.verdicts() read and its summary counts.
The parent then prints the medians and min-max spreads.  Information only: one machine, one session; no threshold.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, RANGES, SLOTS = 4096, 4, 4
LEGS = ["off", "ledger_4", "ledger_4_table", "ledger_4_checks_8"]


def table():
    """Four scenarios of 8 checks each: a speed command, a push over [150, 155), and the questions the scenario asks."""
    out = []
    for c, v in ((0.5, 1.0), (0.5, 2.0), (1.0, 1.0), (1.0, 2.0)):
        out.append({"commands": [[0, c, 0.0, 0.0, 0.0]], "pushes": [[150, 155, v, 0.0, 0.0]],
                    "checks": [[155, 255, "tracking_error", 0, "settle", "<", 0.2, "recovers"], [0, 400, "up", 0, "always", ">", 0.8, "upright"],
                               [0, 400, "torque_max", 0, "always", "<", 40.0, "torque"], [50, 150, "tracking_error", 0, "mean", "<", 0.2, "tracks"],
                               [0, 400, "abs_info", "ang_vel_yaw", "always", "<", 2.0, "yaw_rate"], [0, 400, "qpos", 2, "always", ">", 0.2, "height"],
                               [155, 255, "abs_qvel", 1, "settle", "<", 0.3, "sideways"], [0, 400, "info", "action_diff_RMSE", "mean", "<", 1.0, "smooth"]]})
    return out


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    scn = table() if name in ("ledger_4_table", "ledger_4_checks_8") else None
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, ledger=None if name == "off" else 4, failure_traces=False, scenarios=scn,
                     check_slots=SLOTS if name == "ledger_4_checks_8" else None)
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
    out = {"leg": name, "envs": N, "ranges": RANGES, "ledger_slots": env.engine.query("ledger_slots"), "scenario_rows": env.engine.query("scenario_rows"),
           "check_items": env.engine.query("scenario_check_items"), "timed_steps": steps, "env_steps_per_s": round(N * steps / dt)}
    if name == "ledger_4_checks_8":
        W, I = env.engine.query("scenario_check_words"), env.engine.query("scenario_check_items")
        out["record_words"], out["accumulator_bytes"], out["ring_bytes"] = W, N * (I * 20 + 16), 4 * N * SLOTS * W
        t0 = time.perf_counter()
        v = env.verdicts(include_open=True)
        out["read_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        out["summary"] = v.counts()
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
    cost = lambda k: round(100.0 * (1.0 - med[k] / med["off"]), 2)   # noqa: E731
    summary = {"summary": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in rates.items()},
               "ledger_cost_percent": cost("ledger_4"), "table_cost_percent": cost("ledger_4_table"), "checks_cost_percent": cost("ledger_4_checks_8")}
    print(json.dumps(summary), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 4 ranges, deferred join", "steps": args.steps, "warmup": args.warmup,
                       "runs": runs, **summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
