#!/usr/bin/env python3
"""What observation faults cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join), and
that nothing differs while none are set:

    python tools/gpu_obsfaults_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--parent DIR] [--trace] [--out profiles/obsfault_ab.json]

Faults on: legs `no_table`, `scenarios` (a 64-scenario sweep: 4 commands x 2 push speeds x 2 directions x 1 push time x 4 empty fault
lists, mode cycle) and `scenarios_faults` (the same sweep with 4 fault lists of about ten expanded items each: a gyro bias and lost IMU
packets, encoder noise and a frozen encoder, a stuck gravity vector, a scaled action echo), interleaved R times.  A run prints one JSON
line: env-steps/s of K back-to-back step() calls under an action table.  `faults_cost_percent` is the third leg against the second.
Faults off (`--parent DIR`, a checkout of the parent commit with its library built): the default `python bench.py` there and here,
interleaved R times, and `bench.py --dump-outputs` of both compared byte for byte.  `--trace`: one more run of the third leg under
`rocprofv3 --kernel-trace` (no counters in that run) for the kernel's own duration.  Every run is a child process of its own under
`timeout -k 10 S`; the first run that fails ends the tool.  Information only: one machine, one session.  No threshold.
"""
import argparse
import csv
import filecmp
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, RANGES = 4096, 4
LEGS = ["no_table", "scenarios", "scenarios_faults"]
FAULTS = [[[100, 400, "ang_vel", "*", "bias", 0.05], [100, 1000, "ang_vel", "*", "drop", 0.2], [0, 1000, "dof_vel", "*", "noise", 0.02]],
          [[50, 75, "dof_pos", "*", "hold", 0.0], [0, 1000, "dof_vel", "*", "noise", 0.05], [200, 300, "dof_vel", "*", "scale", 0.0]],
          [[0, 1000, "projected_gravity", "*", "set", 0.0], [0, 1000, "ang_vel", "*", "scale", 1.1], [120, 130, "last_action", "*", "hold", 0.0]],
          [[0, 1000, "last_action", "*", "scale", 0.5], [0, 1000, "dof_pos", "*", "bias", 0.01], [0, 1000, "dof_vel", "*", "drop", 0.1]]]


def leg(name, steps, warmup):
    import numpy as np
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.scenario import scenario_rows, sweep
    table = None
    if name != "no_table":
        table = list(sweep([[0.5, 0, 0, 0], [1.0, 0, 0, 0], [0.3, 0, 0.5, 0], [0.0, 0, -0.5, 0]], [0.3, 0.6], [0.0, 1.5707963], [(50, 55)],
                           faults=FAULTS if name == "scenarios_faults" else [[]] * len(FAULTS)))
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
    if name == "scenarios_faults":                                  # the faults do something: envs whose row holds an item at their clock
        buf = torch.zeros((N, 16), dtype=torch.float32, device=env.device)
        env.engine.get("meta", buf.data_ptr(), env._stream())
        torch.cuda.synchronize()
        meta = buf.view(torch.int32).cpu().numpy()
        rows = scenario_rows(64, "cycle", env.env_id0 + np.arange(N), meta[:, 11])
        inside = int(sum(any(t0 <= meta[i, 0] < t1 for t0, t1, *_ in env.scenario_table.faults[rows[i]]) for i in range(N)))
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"leg": name, "envs": N, "ranges": RANGES, "scenario_rows": env.engine.query("scenario_rows"), "obs_faults": env.engine.query("obs_faults"),
           "timed_steps": steps, "env_steps_per_s": round(N * steps / dt), "finite": bool(torch.isfinite(env.state).all().item())}
    if inside is not None:
        out["envs_under_a_holding_item_after_warmup"] = inside
        out["items_per_row"] = sorted({len(f) for f in env.scenario_table.faults})
    print(json.dumps(out), flush=True)
    env.close()


def child(cmd, timeout, cwd=ROOT):
    """One run under its own time limit; (exit status, stdout)."""
    p = subprocess.run(["timeout", "-k", "10", str(timeout)] + cmd, cwd=cwd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout[-4000:])
    sys.stdout.flush()
    return p.returncode, p.stdout


def last_json(text):
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise ValueError("no JSON line in the run's output")


def faults_off(parent, repeats, timeout):
    """bench.py of the parent checkout and of this one: the medians of `repeats` interleaved default runs, and --dump-outputs of one
    short run each, compared file by file."""
    trees = {"parent": os.path.abspath(parent), "this": ROOT}
    vals = {k: [] for k in trees}
    for _ in range(repeats):
        for k, d in trees.items():
            rc, out = child([sys.executable, "bench.py"], timeout, cwd=d)
            if rc != 0:
                return rc, None
            vals[k].append(last_json(out)["value"])
    tmp = tempfile.mkdtemp(prefix="obsfault_dump_")
    try:
        for k, d in trees.items():
            rc, _ = child([sys.executable, "bench.py", "--steps", "50", "--warmup", "10", "--dump-outputs", os.path.join(tmp, k)], timeout, cwd=d)
            if rc != 0:
                return rc, None
        names = sorted(os.listdir(os.path.join(tmp, "parent")))
        same = names == sorted(os.listdir(os.path.join(tmp, "this"))) and len(names) > 0
        _, mismatch, errors = filecmp.cmpfiles(os.path.join(tmp, "parent"), os.path.join(tmp, "this"), names, shallow=False)
        dump = {"files": names, "byte_identical": bool(same and not mismatch and not errors), "differing": mismatch + errors}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    return 0, {"bench": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in vals.items()},
               "this_over_parent": round(med["this"] / med["parent"], 4), "dump_outputs": dump}


def kernel_trace(steps, warmup, timeout):
    """One run of the third leg under rocprofv3 --kernel-trace: mean / median duration of the table kernels, microseconds."""
    tmp = tempfile.mkdtemp(prefix="obsfault_trace_")
    try:
        rc, _ = child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--leg",
                       "scenarios_faults", "--steps", str(steps), "--warmup", str(warmup)], timeout)
        if rc != 0:
            return rc, None
        dur = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    for k in ("obsfault_step_kernel", "scenario_step_kernel", "scnparams_step_kernel"):
                        if k in name:
                            dur.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
        return 0, {k: {"launches": len(v), "mean_us": round(sum(v) / len(v), 2), "median_us": round(sorted(v)[len(v) // 2], 2),
                       "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in dur.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per run")
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built: run the faults-off legs")
    ap.add_argument("--trace", action="store_true", help="one more run under rocprofv3 --kernel-trace")
    ap.add_argument("--out", default="", help="write the summary (JSON) here")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one run
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps, args.warmup)
        return 0
    rates, last = {name: [] for name in LEGS}, {}
    for _ in range(args.repeats):
        for name in LEGS:
            rc, out = child([sys.executable, os.path.abspath(__file__), "--leg", name, "--steps", str(args.steps), "--warmup", str(args.warmup)],
                            args.timeout)
            if rc != 0:
                print(f"{name}: exit status {rc}; no further runs", flush=True)
                return rc
            last[name] = last_json(out)
            rates[name].append(last[name]["env_steps_per_s"])
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    out = {"workload": "flamingo_light_v1 x %d, flat, %d ranges, deferred join" % (N, RANGES), "timed_steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "summary": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in rates.items()},
           "obs_faults": last["scenarios_faults"]["obs_faults"], "items_per_row": last["scenarios_faults"]["items_per_row"],
           "envs_under_a_holding_item_after_warmup": last["scenarios_faults"]["envs_under_a_holding_item_after_warmup"],
           "scenarios_cost_percent": round(100.0 * (1.0 - med["scenarios"] / med["no_table"]), 2),
           "faults_cost_percent": round(100.0 * (1.0 - med["scenarios_faults"] / med["scenarios"]), 2)}
    if args.trace:
        rc, out["kernel_trace_us"] = kernel_trace(args.steps, args.warmup, args.timeout)
        if rc != 0:
            print(f"kernel trace: exit status {rc}; no further runs", flush=True)
            return rc
    if args.parent:
        rc, out["faults_off"] = faults_off(args.parent, args.repeats, args.timeout)
        if rc != 0:
            print(f"faults off: exit status {rc}; no further runs", flush=True)
            return rc
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
