#!/usr/bin/env python3
"""What response curves cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_curves_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Legs, interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the first run that fails ends the tool:
  table_long     a scenario table of four rows whose curves are not armed, the default time limit: no episode ends inside the run
  curves_long    the same with its 4 curve items per scenario armed (T = 100, B = 32): a sample per item and step, never a fold
  table_short    the table unarmed under a time limit of 100 control steps: every env ends an episode every 100 steps, all in one step
  curves_short   armed: the same samples, and every 100th step folds 4096 episodes of 4 x 100 bins into the cells of four scenarios
  table_s1       one scenario, unarmed, 100-step limit
  curves_s1      armed: every env folds into the SAME cells in the same step (the contended case)
A run prints one JSON line: the seconds and env-steps/s of K back-to-back step() calls under an action table, and for the armed legs
the cell and stage bytes, the time of one BatchedEnv.curves() read and its summary.  The parent then prints the medians and min-max
spreads, the sampling cost per step (curves_long - table_long) and the cost of one fold step ((curves_short - table_short) less the
sampling, over the fold steps of the run), each against the unarmed table of the same leg.  Information only: one machine, one
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

N, RANGES, LIMIT = 4096, 4, 100
LEGS = ["table_long", "curves_long", "table_short", "curves_short", "table_s1", "curves_s1"]


def table(n_scn):
    """Scenarios of 4 curve items each over the first 100 steps of an episode: a speed command, a push over [50, 55), and the signals
    an operator reads off the reference's plot."""
    out = []
    for c, v in ((0.5, 1.0), (0.5, 2.0), (1.0, 1.0), (1.0, 2.0))[:n_scn]:
        out.append({"commands": [[0, c, 0.0, 0.0, 0.0]], "pushes": [[50, 55, v, 0.0, 0.0]],
                    "curves": [[0, 100, 1, "tracking_error", 0, 0.0, 1.5, 32, "velocity_error"], [0, 100, 1, "up", 0, 0.5, 1.0, 32, "upright"],
                               [0, 100, 1, "torque_max", 0, 0.0, 60.0, 32, "torque"], [0, 100, 1, "abs_info", "ang_vel_yaw", 0.0, 3.0, 32, "yaw_rate"]]})
    return out


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    kind, variant = name.split("_")
    cfg = workload_config("light_flat", N)
    if variant != "long":
        cfg["env"]["max_duration"] = LIMIT / 50.0                               # 50 control steps a second
    env = BatchedEnv(cfg, num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES, deferred_join=True, failure_traces=False,
                     scenarios=table(1 if variant == "s1" else 4), curves=kind == "curves")
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
    out = {"leg": name, "envs": N, "ranges": RANGES, "scenario_rows": env.engine.query("scenario_rows"), "curve_items": env.engine.query("scenario_curve_items"),
           "timed_steps": steps, "seconds": round(dt, 6), "env_steps_per_s": round(N * steps / dt),
           "fold_steps": 0 if variant == "long" else (warmup + steps) // LIMIT - warmup // LIMIT}
    if kind == "curves":
        out["cell_bytes"], out["stage_bytes"] = 4 * env.engine.query("scenario_curve_words"), 4 * N * env.engine.query("scenario_curve_stage_words")
        t0 = time.perf_counter()
        cv = env.curves()
        out["read_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        out["summary"] = cv.summary()
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
    folds = {r["leg"]: r["fold_steps"] for r in runs}
    us = lambda x: round(1e6 * x, 2)   # noqa: E731
    sample = (med["curves_long"] - med["table_long"]) / args.steps
    fold = lambda v: ((med[f"curves_{v}"] - med[f"table_{v}"]) - sample * args.steps) / max(folds[f"curves_{v}"], 1)   # noqa: E731
    summary = {"summary": {k: {"median_s": med[k], "min_s": min(v), "max_s": max(v), "median_env_steps_per_s": round(N * args.steps / med[k])}
                           for k, v in secs.items()},
               "step_us_table_long": us(med["table_long"] / args.steps),
               "sampling_us_per_step": us(sample), "sampling_cost_percent": round(100.0 * (med["curves_long"] / med["table_long"] - 1.0), 2),
               "fold_step_us": us(fold("short")), "fold_step_us_s1": us(fold("s1")),
               "curves_short_cost_percent": round(100.0 * (med["curves_short"] / med["table_short"] - 1.0), 2),
               "curves_s1_cost_percent": round(100.0 * (med["curves_s1"] / med["table_s1"] - 1.0), 2)}
    print(json.dumps(summary), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 4 ranges, deferred join", "steps": args.steps, "warmup": args.warmup,
                       "runs": runs, **summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
