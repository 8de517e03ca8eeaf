#!/usr/bin/env python3
"""What the limit search costs under a captured graph (flamingo_light_v1 x 4096 on flat ground, a 16-scenario push table, a random
MLP policy, one control step -- policy, step, observers -- captured and replayed):

    python tools/gpu_search_ab.py --other PATH/libcosim_hip.so [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Legs, alternated R times, every run a child process of its own under `timeout -k 10 S`; the first run that fails ends the tool:
  parent      the other library (the parent commit's build), the table's search items carried but not armed
  not_armed   the library in the tree, the same: nothing may have moved for callers who do not use the search
  armed       the library in the tree with the search armed (search=4): scenario_search_step_kernel in the place of
              scenario_step_kernel, search_step_kernel behind every step
A run prints one JSON line with the seconds of K replays.  The parent process prints, per leg, the median and the min-max spread, and
whether the median of `not_armed` lies inside the spread of `parent` (the run-to-run noise a difference has to leave to count).
Information only: one machine, one session; no threshold.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SLOTS = 4096, 4
LEGS = ["parent", "not_armed", "armed"]


def table():
    """16 scenarios: four commands x four push directions, a push over [40, 45), each with a bisection on the push scale."""
    import math
    from cosim_amd.scenario import sweep
    item = {"lo": 0.25, "hi": 8.0, "rule": "staircase", "trials": 1000, "targets": ["pushes"], "fail_on": ["tilt"]}
    return list(sweep([[0.5, 0, 0, 0], [1.0, 0, 0, 0], [0.5, 0, 0.5, 0], [0.0, 0, 0, 0]], [1.0], [0.0, math.pi / 2, math.pi, -math.pi / 2], [(40, 45)],
                      search=[item]))


def leg(name, lib, steps, warmup):
    import torch
    import cosim_amd.engine as engine
    if lib:
        engine.LIB_PATH = os.path.abspath(lib)                                    # before the first load of the process
    from bench import workload_config
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.fall import FallRule
    from cosim_amd.policy import build_policy, write_random_mlp
    cfg = workload_config("light_flat", N)
    cfg["env"]["max_duration"] = 4.0                                               # 200-step episodes: the push lies inside every one
    env = BatchedEnv(cfg, num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, scenarios=table(), fall=FallRule(tilt=0.8, grace=0),
                     search=SLOTS if name == "armed" else None)
    path = os.path.join(tempfile.mkdtemp(prefix="cosim_policy_"), "actor.onnx")
    write_random_mlp(path, env.state_dim, env.action_dim, seed=1234)
    policy = build_policy({"policy": {"use_lstm": False}}, path, num_envs=N, device=env.device)
    env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    action = torch.zeros((N, env.action_dim), dtype=torch.float32, device=env.device)

    def one_step():
        action.copy_(policy.get_action(env.state))
        env.step(action)
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        for _ in range(3):
            one_step()
    torch.cuda.current_stream(env.device).wait_stream(side)
    torch.cuda.synchronize(env.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step()
    for _ in range(warmup):
        graph.replay()
    torch.cuda.synchronize(env.device)
    t0 = time.perf_counter()
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize(env.device)
    dt = time.perf_counter() - t0
    out = {"leg": name, "lib": "other" if lib else "this", "envs": N, "scenario_rows": env.engine.query("scenario_rows"), "timed_steps": steps,
           "seconds": round(dt, 6), "env_steps_per_s": round(N * steps / dt), "episodes_ended": int(env.solver_stats()["episodes_ended"])}
    if name == "armed":
        out["search"] = env.search(include_trials=False).counts()
    print(json.dumps(out), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--other", required=True, help="the parent commit's library")
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
    secs, runs = {name: [] for name in LEGS}, []
    for _ in range(args.repeats):
        for name in LEGS:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--other", args.other, "--leg", name,
                   "--lib", args.other if name == "parent" else "", "--steps", str(args.steps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                print(f"{name}: exit status {p.returncode}; no further runs", flush=True)
                return p.returncode
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            secs[name].append(runs[-1]["seconds"])
    med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
    summary = {k: {"median_s": med[k], "min_s": min(v), "max_s": max(v), "median_env_steps_per_s": round(N * args.steps / med[k])} for k, v in secs.items()}
    summary["not_armed_median_inside_parent_spread"] = summary["parent"]["min_s"] <= med["not_armed"] <= summary["parent"]["max_s"]
    summary["armed_cost_percent"] = round(100.0 * (med["armed"] / med["not_armed"] - 1.0), 2)
    print(json.dumps({"summary": summary}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "light_flat x 4096, 16 scenarios, one captured control step replayed", "other": os.path.basename(args.other),
                       "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "runs": runs, "summary": summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
