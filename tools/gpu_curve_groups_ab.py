#!/usr/bin/env python3
"""What splitting the response curves into groups costs on the headline workload (flamingo_light_v1 x 4096 on flat ground, four
ranges, deferred join), against the same curves armed WITHOUT groups (tools/gpu_curves_ab.py measures those against an unarmed table):

    python tools/gpu_curve_groups_ab.py [--steps K] [--warmup W] [--repeats R] [--groups G] [--timeout S] [--json OUT.json]

Legs, interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the first run that fails ends the tool:
  table_long     four scenarios whose curves are not armed, the default time limit: no episode ends inside the run
  flat_long      their 4 curve items per scenario armed (T = 100, B = 32), no groups: a sample per item and step, never a fold
  groups_long    armed and split into G groups (env i carries word i mod G): the same samples, never a fold
  table_short    unarmed under a time limit of 100 control steps: every env ends an episode every 100 steps, all in one step
  flat_short     armed, no groups: every 100th step folds 4096 episodes of 4 x 100 bins into the cells of four scenarios
  groups_short   armed with G groups: the same adds, spread over G planes
A run prints one JSON line: the seconds and env-steps/s of K back-to-back step() calls under an action table, and for the armed legs
the cell bytes, the time of one BatchedEnv.curves() read and its summary.  The parent then prints the medians and min-max spreads; per
variant the sampling cost per step and the cost of one fold step against the unarmed table, and the difference groups - flat of
both.  Information only: one machine, one session; no threshold.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_curves_ab import LIMIT, N, RANGES, table  # noqa: E402  (the same table, fleet and time limit)

LEGS = ["table_long", "flat_long", "groups_long", "table_short", "flat_short", "groups_short"]


def leg(name, steps, warmup, groups):
    import numpy as np
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    kind, variant = name.split("_")
    cfg = workload_config("light_flat", N)
    if variant != "long":
        cfg["env"]["max_duration"] = LIMIT / 50.0                               # 50 control steps a second
    env = BatchedEnv(cfg, num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES, deferred_join=True, failure_traces=False,
                     scenarios=table(4), curves=kind != "table")
    if kind == "groups":
        env.set_curve_groups(torch.tensor(np.arange(N, dtype=np.int32) % groups, device=env.device), groups)
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
    out = {"leg": name, "envs": N, "ranges": RANGES, "curve_items": env.engine.query("scenario_curve_items"),
           "groups": env.engine.query("scenario_curve_groups"), "timed_steps": steps, "seconds": round(dt, 6), "env_steps_per_s": round(N * steps / dt),
           "fold_steps": 0 if variant == "long" else (warmup + steps) // LIMIT - warmup // LIMIT}
    if kind != "table":
        out["cell_bytes"] = 4 * max(out["groups"], 1) * env.engine.query("scenario_curve_words")
        t0 = time.perf_counter()
        cv = env.curves()
        out["read_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        s = cv.summary()
        out["summary"] = {k: v for k, v in s.items() if k != "by_group"}
        if "by_group" in s:
            out["episodes_by_group"] = {k: v["episodes"] for k, v in s["by_group"].items()}
    print(json.dumps(out), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--json", default=None, help="also write the runs and the summary here")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps, args.warmup, args.groups)
        return 0
    secs, runs = {name: [] for name in LEGS}, []
    for _ in range(args.repeats):
        for name in LEGS:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--groups", str(args.groups)]
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(f"{name}: exit status {p.returncode}; no further runs", flush=True)
                return p.returncode
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            secs[name].append(runs[-1]["seconds"])
    med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
    folds = max({r["leg"]: r["fold_steps"] for r in runs}["flat_short"], 1)
    us = lambda x: round(1e6 * x, 2)   # noqa: E731
    sample = {k: (med[f"{k}_long"] - med["table_long"]) / args.steps for k in ("flat", "groups")}
    fold = {k: ((med[f"{k}_short"] - med["table_short"]) - sample[k] * args.steps) / folds for k in ("flat", "groups")}
    summary = {"summary": {k: {"median_s": med[k], "min_s": min(v), "max_s": max(v), "median_env_steps_per_s": round(N * args.steps / med[k])}
                           for k, v in secs.items()},
               "groups": args.groups, "fold_steps": folds, "step_us_table_long": us(med["table_long"] / args.steps),
               "sampling_us_per_step": {k: us(v) for k, v in sample.items()}, "fold_step_us": {k: us(v) for k, v in fold.items()},
               "groups_minus_flat_sampling_us_per_step": us(sample["groups"] - sample["flat"]),
               "groups_minus_flat_fold_step_us": us(fold["groups"] - fold["flat"]),
               "groups_over_flat_long_percent": round(100.0 * (med["groups_long"] / med["flat_long"] - 1.0), 2),
               "groups_over_flat_short_percent": round(100.0 * (med["groups_short"] / med["flat_short"] - 1.0), 2)}
    print(json.dumps(summary), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 4 ranges, deferred join, 100-step time limit in the short legs", "steps": args.steps,
                       "warmup": args.warmup, "runs": runs, **summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
