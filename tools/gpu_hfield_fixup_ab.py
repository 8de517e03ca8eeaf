#!/usr/bin/env python3
"""The heightfield fix-up ("hfield_fixup") off and on, same fleet, same action table:

    python tools/gpu_hfield_fixup_ab.py [--steps K] [--warmup W] [--timeout S]

Workloads: config 5 (humanoid_p_v0 on stairs_up_hard, position command, bench.py's 1024 envs and 4 range streams; split pipeline) and
flamingo_light_v1 x 4096 on stairs_up_easy (fused heightfield kernel).  Each (workload, setting) leg runs in a child process of its
own under `timeout -k 10 S`; the first leg that fails ends the run.  Per leg one line: env-steps/s of the timed steps, then
fixup_steps (control steps -- split pipeline: substeps -- redone), dropped_contacts, truncated_walks and max_contacts over the
warm-up and the timed steps.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [("humanoid_stairs", "humanoid_p_v0", "stairs_up_hard", 1024, 4), ("light_stairs", "flamingo_light_v1", "stairs_up_easy", 4096, 4)]


def leg(name, fixup, steps, warmup):
    import torch
    from bench import synthetic_actions, workload_config
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    _, robot, terrain, n, streams = next(x for x in LEGS if x[0] == name)
    cfg = workload_config(name, n) if name == "humanoid_stairs" else make_config(robot, terrain=terrain, num_envs=n, seed=1234)
    env = BatchedEnv(cfg, num_envs=n, seed=1234, auto_reset=True, gain_noise=0.1, ranges=streams, deferred_join=streams > 1,
                     hfield_fixup=bool(fixup))
    acts = synthetic_actions(n, 0, warmup + steps, env.action_dim, env.device)
    if env.command_dim == 2:
        env.receive_user_command(torch.empty((n, 2)).uniform_(-3, 3, generator=torch.Generator().manual_seed(0)).numpy())
    else:
        env.receive_user_command([0.5, 0.0, 0.0, 0.0][:max(env.command_dim, 1)])
    env.reset()
    for t in range(warmup):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        env.step(acts[t])
    env.join()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = env.solver_stats()
    print(json.dumps({"workload": name, "envs": n, "ranges": streams, "hfield_fixup": int(fixup),
                      "split": int(env.engine.query("split") > 0), "contact_slots": env.engine.query("contact_slots"),
                      "fixup_contact_slots": env.engine.query("fixup_contact_slots"), "timed_steps": steps,
                      "env_steps_per_s": round(n * steps / dt), "fixup_steps": st["fixup_steps"],
                      "dropped_contacts": st["dropped_contacts"], "truncated_walks": st["truncated_walks"],
                      "max_contacts": st["max_contacts"], "env_steps_total": n * (warmup + steps)}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--leg", nargs=2, metavar=("WORKLOAD", "FIXUP"), help=argparse.SUPPRESS)   # child process: one leg
    args = ap.parse_args()
    if args.leg:
        leg(args.leg[0], int(args.leg[1]), args.steps, args.warmup)
        return 0
    for name, *_ in LEGS:
        for fixup in (0, 1):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name, str(fixup),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"{name} hfield_fixup={fixup}: exit status {rc}; no further legs", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
