#!/usr/bin/env python3
"""What parameter windows cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_scnparams_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--out profiles/scnparams_ab.json]

Legs `no_table`, `scenarios` (a 64-scenario sweep: 4 commands x 2 push speeds x 2 directions x 1 push time x 4 empty window lists,
mode cycle) and `scenarios_windows` (the same sweep with 4 window lists: none, limp actuators, a slippery floor, binding joints),
interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the first run that fails ends the tool.  A run
prints one JSON line: env-steps/s of K back-to-back step() calls under an action table.  The parent then prints the medians and
min-max spreads and writes them to --out; `windows_cost_percent` is the third leg against the second.  The expectation from the code
is one small launch per stream group and step plus 2 x 384 B per env-step of traffic.  Information only: one machine, one session.
No threshold.
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
LEGS = ["no_table", "scenarios", "scenarios_windows"]
WINDOWS = [[],
           [[100, 150, "kp", "*", "scale", 0.0], [100, 150, "kd", "*", "scale", 0.0]],
           [[50, 300, "geom_friction", "*", "scale", 0.3]],
           [[0, 200, "dof_frictionloss", "*", "scale", 3.0], [20, 40, "kp", 0, "set", 1.0]]]


def leg(name, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.scenario import sweep
    table = None
    if name != "no_table":
        table = list(sweep([[0.5, 0, 0, 0], [1.0, 0, 0, 0], [0.3, 0, 0.5, 0], [0.0, 0, -0.5, 0]], [0.3, 0.6], [0.0, 1.5707963], [(50, 55)],
                           params=WINDOWS if name == "scenarios_windows" else [[]] * len(WINDOWS)))
        assert len(table) == 64
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, scenarios=table, scenario_mode="cycle")
    env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    acts = synthetic_actions(N, 0, warmup + steps, env.action_dim, env.device)
    for t in range(warmup):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    inside = None
    if name == "scenarios_windows":                                 # the windows do something: after the warm-up some effective word differs from its base
        base = env.snapshot().rows.cpu().numpy()[:, env.engine.query("state_stride"):]
        inside = int((env.effective_params() != base).any(axis=1).sum())
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"leg": name, "envs": N, "ranges": RANGES, "scenario_rows": env.engine.query("scenario_rows"),
           "scenario_param_items": env.engine.query("scenario_param_items"), "timed_steps": steps, "env_steps_per_s": round(N * steps / dt)}
    if inside is not None:
        out["envs_inside_a_window_after_warmup"] = inside
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
    out = {"workload": "flamingo_light_v1 x %d, flat, %d ranges, deferred join" % (N, RANGES), "timed_steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "summary": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in rates.items()},
           "scenarios_cost_percent": round(100.0 * (1.0 - med["scenarios"] / med["no_table"]), 2),
           "windows_cost_percent": round(100.0 * (1.0 - med["scenarios_windows"] / med["scenarios"]), 2)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
