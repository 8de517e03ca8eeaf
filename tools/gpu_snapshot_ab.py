#!/usr/bin/env python3
"""What the snapshots cost on the headline workload (flamingo_light_v1 x 4096 on flat ground, four ranges, deferred join):

    python tools/gpu_snapshot_ab.py [--steps K] [--warmup W] [--timeout S]

Legs, each in a child process of its own under `timeout -k 10 S`; the first leg that fails ends the run:
  history off / history (8, 10)   env-steps/s of K back-to-back step() calls under an action table (one JSON line each)
  snapshot / restore              time of one BatchedEnv.snapshot() and one BatchedEnv.restore() of the 4096 envs: median of 20
                                  calls, each between two device synchronisations (so the host side of the call is included)
Information only: one machine, one run.
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
LEGS = ["history_off", "history_8_10", "snapshot_restore"]


def make_env(history):
    import torch  # noqa: F401
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    env = BatchedEnv(workload_config("light_flat", N), num_envs=N, seed=1234, auto_reset=True, gain_noise=0.1, ranges=RANGES,
                     deferred_join=True, history=history)
    env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    return env, synthetic_actions


def leg(name, steps, warmup):
    import torch
    history = (8, 10) if name == "history_8_10" else None
    env, synthetic_actions = make_env(history)
    acts = synthetic_actions(N, 0, warmup + steps, env.action_dim, env.device)
    for t in range(warmup):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    if name == "snapshot_restore":
        snap_ms, rest_ms, restp_ms = [], [], []
        for _ in range(20):
            t0 = time.perf_counter()
            snap = env.snapshot()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            env.restore(snap)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            env.restore(snap, params=True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            snap_ms.append(1e3 * (t1 - t0)); rest_ms.append(1e3 * (t2 - t1)); restp_ms.append(1e3 * (t3 - t2))
        med = lambda v: round(sorted(v)[len(v) // 2], 4)
        print(json.dumps({"leg": name, "envs": N, "snapshot_floats": env.engine.query("snapshot_floats"),
                          "row_bytes_total": 4 * N * env.engine.query("snapshot_floats"), "snapshot_ms": med(snap_ms),
                          "restore_ms": med(rest_ms), "restore_with_params_ms": med(restp_ms), "calls": 20}), flush=True)
    else:
        t0 = time.perf_counter()
        for t in range(warmup, warmup + steps):
            env.step(acts[t])
        env.join()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"leg": name, "envs": N, "ranges": RANGES, "history": list(history) if history else None, "timed_steps": steps,
                          "env_steps_per_s": round(N * steps / dt)}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per leg")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # child process: one leg
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.steps, args.warmup)
        return 0
    for name in LEGS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"{name}: exit status {rc}; no further legs", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
