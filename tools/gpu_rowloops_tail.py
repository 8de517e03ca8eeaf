#!/usr/bin/env python3
"""Who ends a launch of the headline fleet: per control step and range launch, the envs with the most Newton iterations, with their
constraint rows, beside the launch's means.

    python tools/gpu_rowloops_tail.py [--steps 60] [--warmup 100] [--ranges 4] [--json OUT.json]

The bench fleet (bench.py's light_flat: 4096 envs, same seed, same action table), stepped one control step at a time; the per-env
meta words (`engine.get("meta")`: [3] constraint rows summed over the substeps, [5] Newton iterations, [10] most contacts seen so
far) are differenced across each step.  A launch lasts as long as its slowest env and an env's time goes with its Newton iterations,
so the envs that top a launch's iteration count are taken as the ones it waits for.  Envs do not interact, so the fleet is stepped as
one launch and the launches of `--ranges` contiguous ranges are read off the same numbers."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--ranges", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from bench import WORKLOADS, synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    n = WORKLOADS["light_flat"][3]
    cfg = workload_config("light_flat", n)
    env = BatchedEnv(cfg, num_envs=n, device=0, seed=1234, auto_reset=True, env_id0=0, gain_noise=0.1)
    sub = int(env.cm.blob.frame_skip)
    acts = synthetic_actions(n, 0, a.warmup + a.steps, env.action_dim, env.device)
    env.receive_user_command(np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)[:max(env.command_dim, 1)])
    env.reset()
    buf = torch.zeros((n, 16), dtype=torch.float32, device=env.device)

    def meta():
        env.engine.get("meta", buf.data_ptr(), env._stream())
        torch.cuda.synchronize(env.device)
        return buf.view(torch.int32).cpu().numpy().astype(np.int64)

    for t in range(a.warmup):
        env.step(acts[t])
    S = a.ranges
    starts = [i * (n // S) + min(i, n % S) for i in range(S + 1)]
    launches = []
    m0 = meta()
    for t in range(a.warmup, a.warmup + a.steps):
        env.step(acts[t])
        m1 = meta()
        it, rows = m1[:, 5] - m0[:, 5], (m1[:, 3] - m0[:, 3]) / sub
        for i in range(S):
            sl = slice(starts[i], starts[i + 1])
            its, rws = it[sl], rows[sl]
            top = np.argsort(-its, kind="stable")[:4]
            launches.append({"step": t, "range": i, "mean_iterations": float(its.mean()), "max_iterations": int(its.max()),
                             "mean_rows_per_substep": float(rws.mean()),
                             "slowest": [{"env": int(starts[i] + e), "iterations": int(its[e]), "rows_per_substep": float(rws[e]),
                                          "max_contacts_so_far": int(m1[starts[i] + e, 10])} for e in top]})
        m0 = m1
    env.close()
    top_rows = np.array([l["slowest"][0]["rows_per_substep"] for l in launches])
    res = {"command": f"python tools/gpu_rowloops_tail.py --steps {a.steps} --warmup {a.warmup} --ranges {a.ranges}",
           "fleet": "bench.py light_flat, 4096 envs", "substeps_per_control_step": sub,
           "rows": "constraint rows (dense + dof rows) per substep, mean over the control step",
           "summary": {"launches": len(launches),
                       "mean_iterations_per_control_step": float(np.mean([l["mean_iterations"] for l in launches])),
                       "mean_of_max_iterations": float(np.mean([l["max_iterations"] for l in launches])),
                       "mean_rows_fleet": float(np.mean([l["mean_rows_per_substep"] for l in launches])),
                       "mean_rows_of_the_top_env": float(top_rows.mean()), "median_rows_of_the_top_env": float(np.median(top_rows)),
                       "launches_whose_top_env_has_over_40_rows": int((top_rows > 40).sum())},
           "launches": launches}
    print(json.dumps(res["summary"], indent=1), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
