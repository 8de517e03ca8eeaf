#!/usr/bin/env python3
"""The unchanged bench.py on the parent commit's tree against this tree's, alternating in one GPU call (row-loop batching):

    python tools/gpu_rowloops_ab.py --parent DIR [--repeats 3] [--timeout S] [--scratch DIR] [--json OUT.json]

DIR is a built checkout of the parent commit (its cosim_amd/libcosim_hip.so in place).  Every run is a child process under
`timeout -k 10 S` with the queue setting the tool was started with; the first run that fails ends the tool.  Legs:
  * `parent` / `this`, interleaved --repeats times: `python bench.py` with its defaults (light_flat, 1000 steps, 100 warm-up);
  * one pair `--steps 20 --warmup 5`;
  * one pair each `--workload p_v3_flat --steps 200` and `--workload w4_rocky --steps 200`: kernels that must not get slower.
Every run passes --dump-outputs and the tool compares the arrays of each pair byte for byte, and the fleet statistics on the bench
lines.  Writes medians and min-max spreads; a gain is claimed only if the headline median rises by more than three times the larger
arm's min-max spread and roofline.kernel_ms falls with it."""
import argparse
import filecmp
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEET_STATS = ("finite", "fixup_steps", "fleet_action_diff_RMSE", "fleet_abs_torque_0", "solver_per_substep", "max_contacts_per_env")


def bench(tree, extra, env, timeout, dump):
    os.makedirs(dump, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(tree, "bench.py"), *extra, "--dump-outputs", dump]
    p = subprocess.run(cmd, cwd=tree, env=env, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print(f"{' '.join(cmd)}: exit status {p.returncode}; no further runs", flush=True)
        sys.exit(p.returncode)
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    cfg, roof = line.get("config", {}), line.get("roofline", {})
    out = {"value": line["value"], "ms_per_step": line["ms_per_step"], "kernel_ms": roof.get("kernel_ms"), "timed_launches": roof.get("timed_launches")}
    out.update({k: cfg.get(k) for k in FLEET_STATS})
    return out


def same_dumps(a, b):
    names = sorted(os.listdir(a))
    if names != sorted(os.listdir(b)) or not names:
        return False
    return all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in names)


def same_stats(a, b):
    return all(json.dumps(a[k]) == json.dumps(b[k]) for k in FLEET_STATS)


def stats(runs, key="value"):
    v = sorted(r[key] for r in runs)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "min_max_spread": v[-1] - v[0]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", required=True, help="built checkout of the parent commit")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per run")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "rowloops_ab"), help="where the --dump-outputs arrays go")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
    env = dict(os.environ)
    res = {"command": "python bench.py, the parent commit's tree against this tree's, alternating in one GPU call",
           "GPU_MAX_HW_QUEUES": env.get("GPU_MAX_HW_QUEUES", "unset") + " (as the call found it)", "headline": {"parent": {"runs": []}, "this": {"runs": []}}}
    same = {"default": True}
    for rep in range(a.repeats):
        pair = {}
        for who in ("parent", "this"):
            pair[who] = bench(trees[who], [], env, a.timeout, os.path.join(a.scratch, f"{who}_default_{rep}"))
            print(who, json.dumps(pair[who]), flush=True)
            res["headline"][who]["runs"].append(pair[who])
        same["default"] = same["default"] and same_dumps(os.path.join(a.scratch, f"parent_default_{rep}"), os.path.join(a.scratch, f"this_default_{rep}")) \
            and same_stats(pair["parent"], pair["this"])
    for tag, extra in (("steps20_warmup5", ["--steps", "20", "--warmup", "5"]), ("p_v3_flat_steps200", ["--workload", "p_v3_flat", "--steps", "200"]),
                       ("w4_rocky_steps200", ["--workload", "w4_rocky", "--steps", "200"])):
        res[tag] = {}
        for who in ("parent", "this"):
            res[tag][who] = bench(trees[who], extra, env, a.timeout, os.path.join(a.scratch, f"{who}_{tag}"))
            print(tag, who, json.dumps(res[tag][who]), flush=True)
        res[tag]["this_over_parent"] = res[tag]["this"]["value"] / res[tag]["parent"]["value"]
        same[tag] = same_dumps(os.path.join(a.scratch, f"parent_{tag}"), os.path.join(a.scratch, f"this_{tag}")) and same_stats(res[tag]["parent"], res[tag]["this"])
    h = res["headline"]
    for who in ("parent", "this"):
        h[who].update(stats(h[who]["runs"]))
        h[who]["kernel_ms_median"] = stats(h[who]["runs"], "kernel_ms")["median"]
    pm, tm = h["parent"]["median"], h["this"]["median"]
    spread = max(h["parent"]["min_max_spread"], h["this"]["min_max_spread"])
    res["outputs_byte_identical_and_fleet_statistics_equal"] = same
    res["median_gap"] = tm - pm
    res["this_over_parent"] = tm / pm
    res["larger_min_max_spread"] = spread
    res["gain_over_three_spreads"] = (tm - pm) > 3 * spread
    res["kernel_ms_fell"] = h["this"]["kernel_ms_median"] < h["parent"]["kernel_ms_median"]
    print(json.dumps({k: v for k, v in res.items() if k != "headline"}, indent=1), flush=True)
    print(json.dumps({who: {k: v for k, v in h[who].items() if k != "runs"} for who in ("parent", "this")}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
