#!/usr/bin/env python3
"""What rotation costs a policy table in the closed loop (flamingo_light_v1 x 4096 on the plane in four env ranges, K = 3 actors with
hidden (256, 128), 50-step episodes so that the time limit ends them inside the run):

    python tools/gpu_policy_rotate_ab.py [--steps K] [--warmup W] [--repeats R] [--timeout S] [--parent-tree DIR] [--json OUT.json]
    python tools/gpu_policy_rotate_ab.py --kernel-csv kernel_stats.csv --mode eager --json OUT.json   # add kernel times to OUT.json

Legs: `static` (PolicyTable, the assignment fixed for the run) and `rotate` (the same files with rotate_every=1: the regroup launch
ahead of every grouped launch), each in the modes `eager` (Runner.test), `graph` (Runner.test_graphed) and `pipelined`
(Runner.test_pipelined over the four ranges).  With --parent-tree, a checkout of the parent commit with its library built, `parent` is
the static leg run from that tree: the code before this feature.  The legs are interleaved R times, each run in a child process of its
own under `timeout -k 10 S`; the first run that fails ends the tool.  A run prints one JSON line with the env-steps/s of K control
steps after W warm-up steps, timed by a host clock around work that ends in a device synchronise.  The parent process prints medians
and min-max spreads and the ratios the design document quotes.  --kernel-csv reads the kernel statistics a kernel-trace profile of
ONE `rotate` run in mode --mode wrote (a run of its own: tracing slows the loop; start it as `... --leg rotate --mode eager` behind the
profiler's `--`) and stores calls, total and mean time per launch of poltab_regroup_kernel and mlp_grouped_kernel.  Information only: one machine, one session; no threshold.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, K, RANGES = 4096, 3, 4
MODES = ["eager", "graph", "pipelined"]
KERNELS = ("poltab_regroup_kernel", "mlp_grouped_kernel")


def leg(name, mode, steps, warmup, root):
    sys.path.insert(0, root)
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    from cosim_amd.policy import PolicyTable, write_random_mlp
    from cosim_amd.runner import Runner
    cfg = make_config("flamingo_light_v1", num_envs=N, seed=1234, max_duration=1.0)
    env = BatchedEnv(cfg, num_envs=N, seed=1234, auto_reset=True, **({"ranges": RANGES, "deferred_join": True} if mode == "pipelined" else {}))
    d = tempfile.mkdtemp(prefix="cosim_rotate_ab_")
    files = [os.path.join(d, f"actor{k}.onnx") for k in range(K)]
    for k, f in enumerate(files):
        write_random_mlp(f, env.state_dim, env.action_dim, hidden=(256, 128), seed=50 + k)
    policy = PolicyTable(files, num_envs=N, device=env.device, assign="interleave", ranges=env.range_list,
                         **({"rotate_every": 1} if name == "rotate" else {}))
    run = Runner(env, policy)
    run.update_command(0, 0.5)
    go = {"eager": lambda n: run.test(max_steps=n), "graph": lambda n: run.test_graphed(n, warmup=3), "pipelined": lambda n: run.test_pipelined(n)}[mode]
    go(max(warmup, 4))
    torch.cuda.synchronize()
    episodes0 = env.solver_stats()["episodes_ended"]
    t0 = time.perf_counter()
    go(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"leg": name, "mode": mode, "envs": N, "policies": K, "steps": steps, "warmup": warmup, "seconds": round(dt, 4),
                      "env_steps_per_s": N * steps / dt, "episodes_ended": env.solver_stats()["episodes_ended"] - episodes0,
                      "device": torch.cuda.get_device_name(0)}))
    env.close()


def kernel_times(path):
    """Calls and mean nanoseconds per launch of the two kernels, out of a kernel-statistics CSV (columns Name, Calls, AverageNs ...)."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    calls, total = int(row["Calls"]), float(row["TotalDurationNs"])
                    c = out.setdefault(k, {"calls": 0, "total_ns": 0.0})
                    c["calls"] += calls
                    c["total_ns"] += total
    for c in out.values():
        c["mean_us_per_launch"] = c["total_ns"] / c["calls"] / 1000.0
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120, help="seconds one run may take")
    ap.add_argument("--parent-tree", default="", help="a checkout of the parent commit with its library built: adds the leg `parent`")
    ap.add_argument("--kernel-csv", default="", help="kernel statistics of a kernel-trace profile of one `rotate` run: merged into --json")
    ap.add_argument("--json", default="")
    ap.add_argument("--leg", default="", help="run one leg in this process (static | rotate) and print its JSON line")
    ap.add_argument("--mode", default="eager", choices=MODES, help="the mode of --leg, or the mode the --kernel-csv profile ran")
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.mode, args.steps, args.warmup, args.root)
        return 0
    if args.kernel_csv:
        with open(args.json) as f:
            out = json.load(f)
        kt = kernel_times(args.kernel_csv)
        missing = [k for k in KERNELS if k not in kt]
        if missing:
            print(f"{args.kernel_csv}: no row for {missing}", file=sys.stderr)
            return 1
        # both kernels are launched equally often (once per control step, pipelined: once per range and step), so the ratio of the
        # totals is the ratio of their times per control step
        out.setdefault("kernel_trace", {})[args.mode] = {**kt, "regroup / grouped, time per control step": kt[KERNELS[0]]["total_ns"] / kt[KERNELS[1]]["total_ns"],
                                                         "note": f"one `rotate` run in mode {args.mode} under a kernel trace of its own"}
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out["kernel_trace"][args.mode], indent=1))
        return 0
    legs = (["parent"] if args.parent_tree else []) + ["static", "rotate"]
    runs = []
    for r in range(args.repeats):
        for mode in MODES:
            for name in legs:
                root = os.path.abspath(args.parent_tree) if name == "parent" else ROOT
                p = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", "static" if name == "parent" else name,
                                    "--mode", mode, "--root", root, "--steps", str(args.steps), "--warmup", str(args.warmup)], capture_output=True, text=True)
                if p.returncode != 0:
                    print(f"{name} / {mode} (repeat {r}) ended with status {p.returncode}: stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                    return 1
                runs.append({**json.loads(p.stdout.strip().splitlines()[-1]), "leg": name, "repeat": r})
                print(json.dumps(runs[-1]), flush=True)
    summary, ratios = {}, {}
    for mode in MODES:
        for name in legs:
            v = sorted(x["env_steps_per_s"] for x in runs if x["leg"] == name and x["mode"] == mode)
            summary[f"{name} / {mode}"] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / v[len(v) // 2]}
        a = "parent" if args.parent_tree else "static"
        ratios[f"rotate / {a}, {mode}"] = summary[f"rotate / {mode}"]["median"] / summary[f"{a} / {mode}"]["median"]
        if args.parent_tree:
            ratios[f"static / parent, {mode}"] = summary[f"static / {mode}"]["median"] / summary[f"parent / {mode}"]["median"]
    out = {"workload": f"flamingo_light_v1 x {N}, plane, {K} actors (256, 128) interleaved, 50-step episodes, {RANGES} ranges when pipelined",
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "env_steps_per_s": summary, "ratios_of_medians": ratios, "runs": runs}
    print(json.dumps({k: out[k] for k in ("workload", "env_steps_per_s", "ratios_of_medians")}, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
