#!/usr/bin/env python3
"""What action faults cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_actfault_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--trace] [--out profiles/actfault_ab.json]

Three fleets in ONE process, stepped in alternating blocks of K steps, R blocks each: `table` (a 64-scenario sweep: 4 commands x 2 push
speeds x 2 directions x 1 push time x 4 empty action-fault lists, mode cycle), `table_faults` (the same sweep with 4 action-fault
lists of 7 to 9 expanded items each, every scenario under several holding items at every clock: a saturating output, jitter, lost
packets, a stuck channel, a bias) and `table_identity` (the same lists with values that leave every action word as it was -- scale 1,
bias 0, noise 0, drop 0, a clip bound nothing reaches --, so the two kernels do the same walk and the same draws while the robots do
what the fleet of `table` does: the kernels' own cost, apart from what the faults do to the physics the step kernels then solve).
The number to compare both against is `table` of the same run: with no faults set the engine launches what its parent launched.
`--trace`: one more run of the same loop as a child process under `rocprofv3 --kernel-trace` (no counters in that run) for the two
kernels' own durations.  The child runs under `timeout -k 10 S`; a run that fails ends the tool.  Information only: one machine, one
session.  No threshold.
"""
import argparse
import csv
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
LEGS = ["table", "table_faults", "table_identity"]
T1 = 1 << 30                                                        # the windows hold at every clock an episode reaches
FAULTS = [[[0, T1, "*", "clip", 0.6], [0, T1, "*", "noise", 0.02], [100, T1, 0, "bias", 0.05]],
          [[0, T1, "*", "drop", 0.2], [50, 75, 1, "hold", 0.0], [0, T1, 2, "scale", 0.9], [0, T1, 3, "scale", 0.9]],
          [[0, T1, "*", "noise", 0.05], [0, T1, "*", "clip", 0.5]],
          [[0, T1, "*", "bias", 0.01], [0, T1, "*", "drop", 0.1], [200, 300, 0, "set", 0.0]]]
IDENTITY = {"clip": ("clip", 1.0e30), "noise": ("noise", 0.0), "bias": ("bias", 0.0), "drop": ("drop", 0.0), "hold": ("drop", 0.0),
            "scale": ("scale", 1.0), "set": ("scale", 1.0)}
SAME = [[[t0, t1, j, *IDENTITY[op]] for t0, t1, j, op, _ in lst] for lst in FAULTS]


def fleet(name):
    from bench import workload_config
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.scenario import sweep
    table = list(sweep([[0.5, 0, 0, 0], [1.0, 0, 0, 0], [0.3, 0, 0.5, 0], [0.0, 0, -0.5, 0]], [0.3, 0.6], [0.0, 1.5707963], [(50, 55)],
                       action_faults={"table_faults": FAULTS, "table_identity": SAME}.get(name, [[]] * len(FAULTS))))
    assert len(table) == 64
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, scenarios=table, scenario_mode="cycle")
    env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    return env


def run(steps, warmup, repeats):
    import numpy as np
    import torch
    from bench import synthetic_actions
    from cosim_amd.scenario import scenario_rows
    envs = {name: fleet(name) for name in LEGS}
    acts = synthetic_actions(N, 0, warmup + steps, envs["table"].action_dim, envs["table"].device)
    for env in envs.values():
        for t in range(warmup):
            env.step(acts[t])
        env.join()
    torch.cuda.synchronize()
    env = envs["table_faults"]                                      # the faults do something: envs whose row holds an item at their clock
    buf = torch.zeros((N, 16), dtype=torch.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    torch.cuda.synchronize()
    meta = buf.view(torch.int32).cpu().numpy()
    rows = scenario_rows(64, "cycle", env.env_id0 + np.arange(N), meta[:, 11])
    inside = int(sum(any(t0 <= meta[i, 0] < t1 for t0, t1, *_ in env.scenario_table.action_faults[rows[i]]) for i in range(N)))
    rates = {name: [] for name in LEGS}
    for _ in range(repeats):
        for name in LEGS:
            env = envs[name]
            t0 = time.perf_counter()
            for t in range(warmup, warmup + steps):
                env.step(acts[t])
            env.join()
            torch.cuda.synchronize()
            rates[name].append(round(N * steps / (time.perf_counter() - t0)))
    changed = {k: int((envs[k].effective_action() != acts[warmup + steps - 1]).any(dim=1).sum().item()) for k in LEGS[1:]}
    ended = {k: int(e.solver_stats()["episodes_ended"]) for k, e in envs.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    out = {"workload": "flamingo_light_v1 x %d, flat, %d ranges, deferred join" % (N, RANGES), "timed_steps": steps, "warmup": warmup, "repeats": repeats,
           "summary": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in rates.items()},
           "action_faults": envs["table_faults"].engine.query("action_faults"), "action_faults_without": envs["table"].engine.query("action_faults"),
           "items_per_row": sorted({len(f) for f in envs["table_faults"].scenario_table.action_faults}),
           "envs_under_a_holding_item_after_warmup": inside, "envs_whose_last_action_was_changed": changed, "episodes_ended": ended,
           "finite": bool(all(torch.isfinite(e.state).all().item() for e in envs.values())),
           "faults_cost_percent": round(100.0 * (1.0 - med["table_faults"] / med["table"]), 2),
           "kernels_cost_percent": round(100.0 * (1.0 - med["table_identity"] / med["table"]), 2)}
    for e in envs.values():
        e.close()
    return out


def kernel_trace(steps, warmup, timeout):
    """The same loop once more under rocprofv3 --kernel-trace: mean / median duration of the small kernels ahead of and behind the
    step, microseconds."""
    tmp = tempfile.mkdtemp(prefix="actfault_trace_")
    try:
        cmd = ["timeout", "-k", "10", str(timeout), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--steps", str(steps), "--warmup", str(warmup), "--repeats", "1"]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout[-2000:])
        if p.returncode != 0:
            return p.returncode, None
        dur = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    for k in ("actfault_step_kernel", "actfault_obs_kernel", "scenario_step_kernel"):
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
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the traced run")
    ap.add_argument("--trace", action="store_true", help="one more run under rocprofv3 --kernel-trace")
    ap.add_argument("--out", default="", help="write the summary (JSON) here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)   # the traced run: the loop alone
    args = ap.parse_args()
    out = run(args.steps, args.warmup, args.repeats)
    print(json.dumps(out), flush=True)
    if args.child:
        return 0
    if args.trace:
        rc, out["kernel_trace_us"] = kernel_trace(args.steps, args.warmup, args.timeout)
        if rc != 0:
            print(f"kernel trace: exit status {rc}; no further runs", flush=True)
            return rc
        print(json.dumps(out["kernel_trace_us"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
