#!/usr/bin/env python3
"""The unchanged bench.py on the parent commit's tree against this tree's, alternating in one GPU call:

    python tools/gpu_range_streams_ab.py --parent DIR [--repeats 3] [--queues Q] [--sweep] [--timeout S] [--scratch DIR] [--json OUT.json]

DIR is a built checkout of the parent commit (its cosim_amd/libcosim_hip.so in place).  Legs, every run a child process under
`timeout -k 10 S`, the first run that fails ends the tool:
  * `parent` / `this`, interleaved --repeats times: `python bench.py` with its defaults (1000 steps, 100 warm-up);
  * `parent_streams1`, once: the parent with `--streams 1` -- one launch for the whole fleet, the floor any range arrangement must beat;
  * `parent_short` / `this_short`, once each: `--steps 20 --warmup 5`;
  * with --sweep: this tree with COSIM_RANGE_STREAMS = 1, 2, 3, 4, once each.
Every parent / this run also passes --dump-outputs, and the tool compares the arrays byte for byte (default and short runs).
--queues Q puts GPU_MAX_HW_QUEUES=Q in the children's environment; without it they inherit whatever the tool was started with, and
the JSON says which.  Prints and writes medians and min-max spreads; what to make of them is stated in DESIGN 5."""
import argparse
import filecmp
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree, extra, env, timeout, dump=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(tree, "bench.py"), *extra]
    if dump:
        os.makedirs(dump, exist_ok=True)
        cmd += ["--dump-outputs", dump]
    p = subprocess.run(cmd, cwd=tree, env=env, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(f"{' '.join(cmd)}: exit status {p.returncode}; no further runs", flush=True)
        sys.exit(p.returncode)
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    cfg, roof = line.get("config", {}), line.get("roofline", {})
    out = {"value": line["value"], "ms_per_step": line["ms_per_step"], "kernel_ms": roof.get("kernel_ms"), "timed_launches": roof.get("timed_launches")}
    out.update({k: cfg.get(k) for k in ("finite", "fixup_steps", "fleet_action_diff_RMSE", "fleet_abs_torque_0", "solver_per_substep", "max_contacts_per_env")})
    return out


def same_dumps(a, b):
    names = sorted(os.listdir(a))
    if names != sorted(os.listdir(b)) or not names:
        return False
    return all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in names)


def stats(runs):
    v = sorted(r["value"] for r in runs)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "min_max_spread": v[-1] - v[0], "min_max_spread_percent": 100.0 * (v[-1] - v[0]) / v[len(v) // 2]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", required=True, help="built checkout of the parent commit")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--queues", type=int, default=None, help="GPU_MAX_HW_QUEUES for the children (default: inherited)")
    ap.add_argument("--sweep", action="store_true", help="also COSIM_RANGE_STREAMS = 1..4 on this tree")
    ap.add_argument("--timeout", type=int, default=150, help="seconds per run")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "range_streams_ab"), help="where the --dump-outputs arrays go")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    env = dict(os.environ)
    env.pop("COSIM_RANGE_STREAMS", None)
    if a.queues is not None:
        env["GPU_MAX_HW_QUEUES"] = str(a.queues)
    tag = f"q{env.get('GPU_MAX_HW_QUEUES', 'unset')}"
    trees = {"parent": parent, "this": ROOT}
    res = {"command": "python bench.py (defaults), the parent commit's tree against this tree's, alternating in one GPU call",
           "GPU_MAX_HW_QUEUES": env.get("GPU_MAX_HW_QUEUES", "unset") + (" (given to the runs)" if a.queues is not None else " (as the call found it)"),
           "parent": {"runs": []}, "this": {"runs": []}}
    for rep in range(a.repeats):
        for who in ("parent", "this"):
            r = bench(trees[who], [], env, a.timeout, dump=os.path.join(a.scratch, f"{tag}_{who}_default_{rep}"))
            print(who, json.dumps(r), flush=True)
            res[who]["runs"].append(r)
    res["parent_streams1"] = bench(parent, ["--streams", "1"], env, a.timeout)
    print("parent_streams1", json.dumps(res["parent_streams1"]), flush=True)
    for who in ("parent", "this"):
        res[who + "_short"] = bench(trees[who], ["--steps", "20", "--warmup", "5"], env, a.timeout, dump=os.path.join(a.scratch, f"{tag}_{who}_short"))
        print(who + "_short", json.dumps(res[who + "_short"]), flush=True)
    if a.sweep:
        res["sweep_COSIM_RANGE_STREAMS"] = {}
        for p in (1, 2, 3, 4):
            res["sweep_COSIM_RANGE_STREAMS"][str(p)] = bench(ROOT, [], dict(env, COSIM_RANGE_STREAMS=str(p)), a.timeout)
            print("sweep", p, json.dumps(res["sweep_COSIM_RANGE_STREAMS"][str(p)]), flush=True)
    for who in ("parent", "this"):
        res[who].update(stats(res[who]["runs"]))
    res["outputs_byte_identical"] = {
        "default": all(same_dumps(os.path.join(a.scratch, f"{tag}_parent_default_{rep}"), os.path.join(a.scratch, f"{tag}_this_default_{rep}")) for rep in range(a.repeats)),
        "steps20_warmup5": same_dumps(os.path.join(a.scratch, f"{tag}_parent_short"), os.path.join(a.scratch, f"{tag}_this_short"))}
    pm, tm = res["parent"]["median"], res["this"]["median"]
    res["median_gap"] = tm - pm
    res["this_over_parent"] = tm / pm
    res["larger_min_max_spread"] = max(res["parent"]["min_max_spread"], res["this"]["min_max_spread"])
    res["medians_within_the_larger_spread"] = abs(tm - pm) <= res["larger_min_max_spread"]
    res["this_at_or_above_parent_streams1"] = tm >= res["parent_streams1"]["value"]
    print(json.dumps({k: v for k, v in res.items() if k not in ("parent", "this")}, indent=1), flush=True)
    print(json.dumps({"parent": {k: v for k, v in res["parent"].items() if k != "runs"}, "this": {k: v for k, v in res["this"].items() if k != "runs"}}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
