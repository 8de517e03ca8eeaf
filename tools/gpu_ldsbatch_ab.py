#!/usr/bin/env python3
"""The unchanged bench.py on several built trees against this tree's, alternating in one GPU call (LDS batches): the
protocol of tools/gpu_rowloops_ab.py with more than two arms, so that the parts of a change are measured one against the other.

    python tools/gpu_ldsbatch_ab.py --arm parent=DIR [--arm NAME=DIR ...] [--repeats 3] [--timeout S] [--scratch DIR] [--json OUT.json]

Every DIR is a built checkout (its cosim_amd/libcosim_hip.so in place): the parent commit first, then trees that hold part of the change;
the last arm, "this", is this tree.  Legs: the arms interleaved --repeats times with `python bench.py` and its defaults; one run per arm
with `--steps 20 --warmup 5`; one run each of the first and the last arm with `--workload p_v3_flat --steps 200` and `--workload w4_rocky
--steps 200` (kernels that must not change).  Every run passes --dump-outputs; the arrays and the fleet statistics of every arm are
compared with the first arm's byte for byte.  Per pair of neighbouring arms: the median gap over the larger min-max spread of the two;
a part counts as a gain only where that ratio is above three."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_rowloops_ab import ROOT, bench, same_dumps, same_stats, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--arm", action="append", required=True, metavar="NAME=DIR")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per run")
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "ldsbatch_ab"), help="where the --dump-outputs arrays go")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    arms = [(x.split("=", 1)[0], os.path.abspath(x.split("=", 1)[1])) for x in a.arm] + [("this", ROOT)]
    names = [n for n, _ in arms]
    env = dict(os.environ)
    res = {"command": "python bench.py on every arm's tree, alternating in one GPU call", "arms": names,
           "GPU_MAX_HW_QUEUES": env.get("GPU_MAX_HW_QUEUES", "unset") + " (as the call found it)", "headline": {n: {"runs": []} for n in names}}
    same = True
    for rep in range(a.repeats):
        for n, tree in arms:
            r = bench(tree, [], env, a.timeout, os.path.join(a.scratch, f"{n}_default_{rep}"))
            print(n, json.dumps(r), flush=True)
            res["headline"][n]["runs"].append(r)
            if n != names[0]:
                same = same and same_dumps(os.path.join(a.scratch, f"{names[0]}_default_{rep}"), os.path.join(a.scratch, f"{n}_default_{rep}")) \
                    and same_stats(res["headline"][names[0]]["runs"][rep], r)
    for tag, extra, who in (("steps20_warmup5", ["--steps", "20", "--warmup", "5"], arms),
                            ("p_v3_flat_steps200", ["--workload", "p_v3_flat", "--steps", "200"], [arms[0], arms[-1]]),
                            ("w4_rocky_steps200", ["--workload", "w4_rocky", "--steps", "200"], [arms[0], arms[-1]])):
        res[tag] = {}
        for n, tree in who:
            res[tag][n] = bench(tree, extra, env, a.timeout, os.path.join(a.scratch, f"{n}_{tag}"))
            print(tag, n, json.dumps(res[tag][n]), flush=True)
            if n != who[0][0]:
                same = same and same_dumps(os.path.join(a.scratch, f"{who[0][0]}_{tag}"), os.path.join(a.scratch, f"{n}_{tag}")) \
                    and same_stats(res[tag][who[0][0]], res[tag][n])
    h = res["headline"]
    for n in names:
        h[n].update(stats(h[n]["runs"]))
        h[n]["kernel_ms_median"] = stats(h[n]["runs"], "kernel_ms")["median"]
    res["outputs_byte_identical_and_fleet_statistics_equal"] = same
    res["steps"] = []
    for (p, q) in list(zip(names[:-1], names[1:])) + ([(names[0], names[-1])] if len(names) > 2 else []):
        spread = max(h[p]["min_max_spread"], h[q]["min_max_spread"])
        gap = h[q]["median"] - h[p]["median"]
        res["steps"].append({"from": p, "to": q, "ratio": h[q]["median"] / h[p]["median"], "median_gap": gap, "larger_min_max_spread": spread,
                             "gap_over_spread": gap / spread if spread > 0 else None, "kernel_ms": [h[p]["kernel_ms_median"], h[q]["kernel_ms_median"]]})
    print(json.dumps({k: v for k, v in res.items() if k != "headline"}, indent=1), flush=True)
    print(json.dumps({n: {k: v for k, v in h[n].items() if k != "runs"} for n in names}), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
