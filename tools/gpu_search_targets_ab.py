#!/usr/bin/env python3
"""What the limit search's new targets and criteria cost, and that nothing moved for callers who do not use them:

    python tools/gpu_search_targets_ab.py --other PATH/libcosim_hip.so [--steps K] [--warmup W] [--repeats R] [--timeout S] [--json OUT.json]

Part 1, `python bench.py --gpus 1` (the flagship workload: no scenario table, so nothing new is launched), alternated R times:
  bench_parent   the other library (the parent commit's build)
  bench_this     the library in the tree
Part 2, flamingo_light_v1 x 4096 on flat ground, a 16-scenario table with a push, parameter windows, observation faults, action faults
and a check in every row, a random MLP
policy, one control step -- policy, step, observers -- captured and replayed, alternated R times:
  pushes_parent  the other library, a staircase on the pushes that fails on tilt: what the parent commit could search
  pushes_this    the library in the tree, the same table
  marked_this    the library in the tree, the staircase on the pushes AND the marked parameter windows, observation faults and action
                 faults (the three *_search_step_kernel forms in the place of the plain ones, the observation-fault launch behind
                 the search's), failing on tilt or on the row's check (search_step_checks_kernel in the place of search_step_kernel),
                 the checks armed in every leg
  level1_parent  as pushes_parent, with the level held near 1 (lo 0.999, hi 1.001)
  level1_marked  as marked_this, with the same bounds: the level moves, the physics barely does, so the difference to level1_parent
                 is what the launches cost.  (Between pushes_parent and marked_this the level also scales friction, kp and the
                 faults by 0.25 .. 8, which changes how often the robots fall and how much the solver works.)
Every run is a child process of its own under `timeout -k 10 S`; the first run that fails ends the tool.  The parent process prints,
per leg, the median and the min-max spread, and whether the median of `bench_this` / `pushes_this` lies inside the spread of the
parent's runs.  `marked_this` is recorded with no bound.  Information only: one machine, one session.
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
BENCH_LEGS = ["bench_parent", "bench_this"]
STEP_LEGS = ["pushes_parent", "pushes_this", "marked_this", "level1_parent", "level1_marked"]


def table(marked, level1=False):
    """16 scenarios: four commands x four push directions, a push over [40, 45); in every row a friction and a kp window, a gyro bias
    and encoder noise, a bias, a noise and a drop on the actuators and a check on the tracking error; a staircase on the push scale,
    with `marked` also on all those items and failing on the check too."""
    import math
    from cosim_amd.scenario import sweep
    faults = [[0, 200, "*", "bias", 0.02], [0, 200, "*", "noise", 0.05], [20, 120, "*", "drop", 0.05]]
    checks = [[60, 199, "tracking_error", 0, "settle", "<", 0.5, "recovers"]]
    params = [[0, 200, "geom_friction", "*", "scale", 1.0], [0, 200, "kp", "*", "scale", 1.0]]
    obs = [[0, 200, "ang_vel", "*", "bias", 0.02], [0, 200, "dof_pos", "*", "noise", 0.01]]
    item = {"lo": 0.25, "hi": 8.0, "rule": "staircase", "trials": 1000, "targets": ["pushes"], "fail_on": ["tilt"]}
    if level1:
        item = dict(item, lo=0.999, hi=1.001)
    if marked:
        item = dict(item, targets=["pushes", "params", "faults", "action_faults"], fail_on=["tilt", "check:recovers"])
    return list(sweep([[0.5, 0, 0, 0], [1.0, 0, 0, 0], [0.5, 0, 0.5, 0], [0.0, 0, 0, 0]], [1.0], [0.0, math.pi / 2, math.pi, -math.pi / 2], [(40, 45)],
                      params=[params], checks=[checks], faults=[obs], action_faults=[faults], search=[item]))


def use(lib):
    import cosim_amd.engine as engine
    if lib:
        engine.LIB_PATH = os.path.abspath(lib)                                    # before the first load of the process


def bench_leg(name, lib, steps, warmup):
    import runpy
    use(lib)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def step_leg(name, lib, steps, warmup):
    import torch
    use(lib)
    from bench import workload_config
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.fall import FallRule
    from cosim_amd.policy import build_policy, write_random_mlp
    cfg = workload_config("light_flat", N)
    cfg["env"]["max_duration"] = 4.0                                               # 200-step episodes: the push lies inside every one
    env = BatchedEnv(cfg, num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, scenarios=table(name.endswith("marked") or name == "marked_this", name.startswith("level1")),
                     fall=FallRule(tilt=0.8, grace=0), search=SLOTS, check_slots=SLOTS)
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
           "seconds": round(dt, 6), "env_steps_per_s": round(N * steps / dt), "episodes_ended": int(env.solver_stats()["episodes_ended"]),
           "search_targets": env.engine.query("search_targets") if not lib else None, "search": env.search(include_trials=False).counts()}
    print(json.dumps(out), flush=True)
    env.close()


def spread(secs, work):
    med = {k: sorted(v)[len(v) // 2] for k, v in secs.items()}
    return med, {k: {"median_s": med[k], "min_s": min(v), "max_s": max(v), "median_env_steps_per_s": round(work / med[k])} for k, v in secs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--other", required=True, help="the parent commit's library")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per run")
    ap.add_argument("--json", default=None, help="also write the runs and the summary here")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        (bench_leg if args.leg in BENCH_LEGS else step_leg)(args.leg, args.lib, args.steps, args.warmup)
        return 0
    if not os.path.isfile(args.other):
        raise SystemExit(f"{args.other}: no such library")
    bench_lines, runs = {name: [] for name in BENCH_LEGS}, []
    secs = {name: [] for name in STEP_LEGS}
    for legs in (BENCH_LEGS, STEP_LEGS):
        for _ in range(args.repeats):
            for name in legs:
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--other", args.other, "--leg", name,
                       "--lib", args.other if name.endswith("_parent") else "", "--steps", str(args.steps), "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
                sys.stdout.write(p.stdout)
                sys.stdout.flush()
                if p.returncode != 0:
                    print(f"{name}: exit status {p.returncode}; no further runs", flush=True)
                    return p.returncode
                line = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
                if legs is BENCH_LEGS:
                    bench_lines[name].append(line)
                else:
                    runs.append(line)
                    secs[name].append(line["seconds"])
    summary = {}
    key = next((k for k in ("env_steps_per_s", "steps_per_s", "value") if bench_lines["bench_parent"] and k in bench_lines["bench_parent"][0]), None)
    if key:
        rate = {name: [ln[key] for ln in lines] for name, lines in bench_lines.items()}
        mid = sorted(rate["bench_this"])[len(rate["bench_this"]) // 2]
        summary["bench"] = {"metric": key, **{name: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for name, v in rate.items()},
                            "this_median_inside_parent_spread": min(rate["bench_parent"]) <= mid <= max(rate["bench_parent"]),
                            "this_over_parent": round(mid / sorted(rate["bench_parent"])[len(rate["bench_parent"]) // 2], 4)}
    med, summary["step"] = spread(secs, N * args.steps)
    summary["step"]["pushes_this_median_inside_parent_spread"] = summary["step"]["pushes_parent"]["min_s"] <= med["pushes_this"] <= summary["step"]["pushes_parent"]["max_s"]
    summary["step"]["marked_cost_percent_over_pushes_parent"] = round(100.0 * (med["marked_this"] / med["pushes_parent"] - 1.0), 2)
    summary["step"]["level1_marked_cost_percent_over_level1_parent"] = round(100.0 * (med["level1_marked"] / med["level1_parent"] - 1.0), 2)
    print(json.dumps({"summary": summary}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"workload": "bench.py --gpus 1; light_flat x 4096, 16 scenarios, one captured control step replayed", "other": os.path.basename(args.other),
                       "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "bench_lines": bench_lines, "runs": runs, "summary": summary}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
