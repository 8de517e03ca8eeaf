#!/usr/bin/env python3
"""Two builds of libcosim_hip.so against each other on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges,
deferred join), for a change that should cost nothing:

    python tools/gpu_lib_ab.py --other PATH/libcosim_hip.so [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Legs, each timed with the library in the tree ("this") and with the other one ("other"), alternated R times; every run is a child
process of its own under `timeout -k 10 S`, and the first run that fails ends the tool:
  off         bench.py's headline loop: no observer armed
  observers   a scenario table of four rows (tools/gpu_curves_ab.py) with its curves and one check per scenario armed, an episode ledger
              and failure traces: every step ends in the four observer launches per range
A run prints one JSON line with the seconds of K back-to-back step() calls under an action table.  The parent prints, per leg and
library, the median and the min-max spread; the other library's spread is the run-to-run noise a difference has to leave to count.
Information only: one machine, one session; no threshold.
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
LEGS = ["off", "observers"]


def leg(name, lib, steps, warmup):
    import torch
    import cosim_amd.engine as engine
    if lib:
        engine.LIB_PATH = os.path.abspath(lib)                                    # before the first load of the process
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    from gpu_curves_ab import table
    kw = {"ledger": 0, "failure_traces": False}
    if name == "observers":
        scn = table(4)
        for sc in scn:
            sc["checks"] = [[0, 100, "tracking_error", 0, "settle", "<", 0.3, "tracks"]]
        kw = {"ledger": 8, "failure_traces": (16, 2), "scenarios": scn, "check_slots": 4, "curves": True}
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES, deferred_join=True, **kw)
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
    print(json.dumps({"leg": name, "lib": "other" if lib else "this", "envs": N, "ranges": RANGES, "timed_steps": steps, "seconds": round(dt, 6),
                      "env_steps_per_s": round(N * steps / dt), "ledger_slots": env.engine.query("ledger_slots"),
                      "ftrace_frames": env.engine.query("ftrace_frames"), "check_items": env.engine.query("scenario_check_items"),
                      "curve_items": env.engine.query("scenario_curve_items")}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--other", required=True, help="the library to compare the tree's with")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--json", default=None, help="also write the runs and the summary here")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.lib, args.steps, args.warmup)
        return 0
    if not os.path.isfile(args.other):
        raise SystemExit(f"{args.other}: no such library")
    secs, runs = {(name, lib): [] for name in LEGS for lib in ("other", "this")}, []
    for _ in range(args.repeats):
        for name in LEGS:
            for lib in ("other", "this"):
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--other", args.other, "--leg", name,
                       "--lib", args.other if lib == "other" else "", "--steps", str(args.steps), "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
                sys.stdout.write(p.stdout)
                sys.stdout.flush()
                if p.returncode != 0:
                    print(f"{name} / {lib}: exit status {p.returncode}; no further runs", flush=True)
                    return p.returncode
                runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
                secs[name, lib].append(runs[-1]["seconds"])
    summary = {}
    for name in LEGS:
        row = {lib: {"median_s": sorted(v)[len(v) // 2], "min_s": min(v), "max_s": max(v), "median_env_steps_per_s": round(N * args.steps / sorted(v)[len(v) // 2])}
               for lib, v in ((lib, secs[name, lib]) for lib in ("other", "this"))}
        row["this_median_inside_other_spread"] = row["other"]["min_s"] <= row["this"]["median_s"] <= row["other"]["max_s"]
        summary[name] = row
    print(json.dumps({"summary": summary}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 4 ranges, deferred join", "other": os.path.basename(args.other), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
                       "runs": runs, "summary": summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.exit(main())
