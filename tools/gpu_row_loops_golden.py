#!/usr/bin/env python3
"""Record what tests/test_gpu_row_loops.py compares against: two small plane fleets set into poses that cover the dense-row counts
the solver's row loops (J^T f, Hessian tile) branch on, stepped three control steps.

    python tools/gpu_row_loops_golden.py --commit HASH [--out DIR]     # on the GPU, from a built checkout of the commit to record

Writes DIR/row_loops_light_v1.npz and DIR/row_loops_p_v3.npz (default DIR: tests/golden): the poses, the actions, the dense-row
count of every env at its pose (`cosim_debug_forward`, D[7]) and, after each step, state / terminated / info / qpos / qvel / the
warm-start qacc, float32 bit for bit.  `commit` inside the file names the commit the bits are from: the files in the repository
were recorded on the parent of the commit that batched the row loops' LDS reads, and that change must not move a bit.

The poses come from a seeded search, so the tool needs no other input: the fp64 oracle proposes poses by contact count (upright,
tilted, on a side, upside down, dropped from a few centimetres in an arbitrary pose), the engine's own debug forward says how many
dense rows each has, and the fleet is picked by those:
  flamingo_light_v1, 32 envs: 6 equality rows + 4 per ground contact -> 6, 10, 14, 18 rows (below one batch of eight, both
      remainders 2 and 6 mod 8), 22, ten poses between 34 and 58, 62 rows (exactly 14 contacts: every slot) and more than 14
      contacts (the step is redone by the large-capacity kernel).
  flamingo_p_v3, 16 envs: 4 rows per contact, ground and robot-robot alike -> even and odd contact counts (0 and 4 mod 8).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = 3
PER_COUNT = 12  # candidate poses kept per oracle contact count
# (dense rows at the pose, lowest .. highest; oracle contacts, lowest .. highest; envs): what a fleet is made of.  The rows are the
# engine's own (debug forward on every candidate), the oracle only proposes.
FLEETS = {
    "light_v1": dict(robot="flamingo_light_v1", n=32, seed=7,
                     want=[(6, 6, 0, 0, 3), (10, 10, 0, 99, 4), (14, 14, 0, 99, 4), (18, 18, 0, 99, 2), (22, 22, 0, 99, 2), (34, 58, 0, 99, 10),
                           (62, 62, 14, 14, 5), (62, 62, 15, 99, 2)]),
    "p_v3": dict(robot="flamingo_p_v3", n=16, seed=11,
                 want=[(0, 0, 0, 0, 1), (4, 4, 0, 99, 2), (8, 8, 0, 99, 2), (12, 12, 0, 99, 2), (16, 16, 0, 99, 1), (20, 20, 0, 99, 2),
                       (24, 24, 0, 99, 1), (28, 28, 0, 99, 1), (32, 32, 0, 99, 1), (36, 64, 0, 99, 3)]),
}


def _quat(axis, ang):
    a = np.asarray(axis, dtype=np.float64)
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * a / np.linalg.norm(a)])


def model(name):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    f = FLEETS[name]
    cfg = make_config(f["robot"], random=PARITY_RANDOM, num_envs=f["n"])
    return cfg, compile_model(cfg)


def candidates(name, cm):
    """qpos [m, nq] (float32) and the oracle's contact count at each, at most PER_COUNT per count: named poses first, then seeded
    random drops; none deeper than 3 cm in the ground, so that three steps from rest stay finite."""
    from cosim_amd.model import get_field
    from oracle.oracle import Oracle
    f = FLEETS[name]
    b = cm.blob
    q0 = np.array(get_field(b, "init_qpos")[:b.nq])
    rng = np.random.default_rng(f["seed"])
    cands = []
    for dz in (0.03, 0.05, 0.0):                                   # dropped from a few cm, standing
        q = q0.copy(); q[2] += dz; cands.append(q)
    for ang in (0.05, 0.1, 0.2, 0.4, 0.8):                         # tilted
        for ax in ((1, 0, 0), (0, 1, 0)):
            for dz in (0.02, 0.0, -0.01):
                q = q0.copy(); q[3:7] = _quat(ax, ang); q[2] += dz; cands.append(q)
    for ax in ((1, 0, 0), (0, 1, 0)):                              # on a side, face down / up, upside down
        for ang in (np.pi / 2, -np.pi / 2, np.pi):
            for z in np.arange(0.02, 0.32, 0.01):
                q = q0.copy(); q[3:7] = _quat(ax, ang); q[2] = z; cands.append(q)
    for _ in range(30000):                                         # dropped in an arbitrary pose
        q = q0.copy()
        qu = rng.normal(size=4)
        q[2] = rng.uniform(0.03, 0.3)
        q[3:7] = qu / np.linalg.norm(qu)
        q[7:] += rng.uniform(-0.6, 0.6, size=q.size - 7)
        cands.append(q)
    o = Oracle(cm)
    kept, poses, counts = {}, [], []
    for q in cands:
        q = q.astype(np.float32).astype(np.float64)                # the pose the engine will hold
        o.reset(q)
        o.forward()
        c = o.contacts()
        if kept.get(len(c), 0) < PER_COUNT and (len(c) == 0 or c[:, 0].min() > -0.03):
            kept[len(c)] = kept.get(len(c), 0) + 1
            poses.append(q)
            counts.append(len(c))
    return np.array(poses, dtype=np.float32), np.array(counts, dtype=np.int32)


def dense_rows(cfg, cm, qpos):
    """The engine's dense-row count (debug forward, D[7]) of every pose."""
    from cosim_amd.batched_env import BatchedEnv
    n, nv = qpos.shape[0], cm.blob.nv
    env = BatchedEnv(cfg, num_envs=n, device=0, auto_reset=False, compiled=cm)
    try:
        env.reset()
        env.set_state(qpos=qpos, qvel=np.zeros((n, nv)), qacc_warmstart=np.zeros((n, nv)))
        return np.array([int(env.engine.debug_forward(e)[7]) for e in range(n)], dtype=np.int32)
    finally:
        env.close()


def pick(name, rows, counts):
    """Indices of the candidates the fleet is made of: per entry of `want` in candidate order, row counts not yet taken first."""
    taken = []
    for lo, hi, clo, chi, k in FLEETS[name]["want"]:
        fit = [i for i in range(len(rows)) if lo <= rows[i] <= hi and clo <= counts[i] <= chi and i not in taken]
        seen, first, rest = set(), [], []
        for i in fit:
            (rest if rows[i] in seen else first).append(i)
            seen.add(rows[i])
        assert len(fit) >= k, f"{name}: {len(fit)} candidate poses with {lo}..{hi} dense rows and {clo}..{chi} oracle contacts, {k} wanted"
        taken += (first + rest)[:k]
    assert len(taken) == FLEETS[name]["n"]
    return np.array(taken)


def actions(n, nu, seed):
    """[STEPS, n, nu] fixed nonzero actions."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 0.6, (STEPS, n, nu)) * rng.choice([-1.0, 1.0], (STEPS, n, nu))
    return a.astype(np.float32)


def run_fleet(cfg, cm, qpos, act, step_kernel=None):
    """Set the poses (zero velocity, zero warm start), read every env's dense-row count, step through `act`.  Returns
    (rows [n] int32, {array name: [STEPS, ...]}): everything as numpy, the floats as they are in memory."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    n, nv = qpos.shape[0], cm.blob.nv
    env = BatchedEnv(cfg, num_envs=n, device=0, auto_reset=False, compiled=cm)
    try:
        if step_kernel is not None:
            env.engine.set_param("step_kernel", np.array([float(step_kernel)]))
            assert env.engine.query("step_kernel") == step_kernel
        env.reset()
        env.set_state(qpos=qpos, qvel=np.zeros((n, nv)), qacc_warmstart=np.zeros((n, nv)))
        rows = np.array([int(env.engine.debug_forward(e)[7]) for e in range(n)], dtype=np.int32)
        env.set_state(qpos=qpos, qvel=np.zeros((n, nv)), qacc_warmstart=np.zeros((n, nv)))
        warm = torch.zeros((n, nv), dtype=torch.float32, device=env.device)
        out = {k: [] for k in ("state", "terminated", "info", "qpos", "qvel", "qacc_warmstart")}
        a = torch.tensor(act, device=env.device)
        for t in range(a.shape[0]):
            env.step(a[t])
            d = env.get_data()
            env.engine.get("qacc_warmstart", warm.data_ptr(), env._stream())
            torch.cuda.synchronize(env.device)
            for k, v in (("state", env.state), ("terminated", env.terminated), ("info", env.info_buf), ("qpos", d.qpos), ("qvel", d.qvel),
                         ("qacc_warmstart", warm)):
                out[k].append(v.cpu().numpy().copy())
        return rows, {k: np.stack(v) for k, v in out.items()}
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="hash of the checked-out commit (written into the files)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name, f in FLEETS.items():
        cfg, cm = model(name)
        cq, cc = candidates(name, cm)
        crows = dense_rows(cfg, cm, cq)
        print(name, "candidates (oracle contacts, dense rows):", sorted(set(zip(cc.tolist(), crows.tolist()))), flush=True)
        sel = pick(name, crows, cc)
        qpos, ncon = cq[sel], cc[sel]
        act = actions(f["n"], cm.blob.nu, f["seed"])
        rows, out = run_fleet(cfg, cm, qpos, act)
        print(name, "oracle contacts", ncon.tolist(), flush=True)
        print(name, "dense rows     ", rows.tolist(), flush=True)
        for k, v in out.items():
            if v.dtype == np.float32:
                print(f"  {k}: {v.shape}, finite {bool(np.isfinite(v).all())}", flush=True)
        path = os.path.join(a.out, f"row_loops_{name}.npz")
        np.savez_compressed(path, commit=np.array(a.commit), robot=np.array(f["robot"]), pose_qpos=qpos, actions=act, oracle_contacts=ncon,
                            dense_rows=rows, **out)
        print(path, os.path.getsize(path), "bytes", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
