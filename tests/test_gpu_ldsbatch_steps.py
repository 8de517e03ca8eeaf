"""Whole control steps with the batched LDS reads of the solver (KTraits::LDSB: M v, J v, the triangular solves from LDS) against the
one-wait-per-pair form.

The fleet kernels of flamingo_light_v1 on the plane carry the batched forms, the rollout kernel keeps the old ones (it passes
LDSB = false to env_body).  Both are meant to round every term the same way, so a table of control steps through the step loop and the
same table through env.rollout must give the same bits: states, flags, info rows, final qpos / qvel and the solver counters.  Half the
fleet starts from drop poses with 9 .. 14 ground contacts (up to 56 dense rows, several Newton iterations that reuse a factor); no step may leave the fleet kernel, whose large-capacity stand-in rounds differently."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, NCAND = 16, 12, 128


def _sin_table(steps, n, nu, seed):
    rng = np.random.default_rng(seed)
    amp, freq, ph = rng.uniform(0.1, 0.6, (n, nu)), rng.uniform(0.3, 2.0, (n, nu)), rng.uniform(0, 2 * np.pi, (n, nu))
    t = 0.02 * np.arange(steps)[:, None, None]
    return (amp * np.sin(2 * np.pi * freq * t + ph)).astype(np.float32)


def _meta(env):
    torch = env.torch
    meta = torch.zeros((env.num_envs, 16), dtype=torch.float32, device=env.device)
    env.engine.get("meta", meta.data_ptr(), env._stream())
    torch.cuda.synchronize(env.device)
    return meta.view(torch.int32).clone()


@pytest.fixture(scope="module")
def fleet():
    """Config, compiled model, action table and start states: envs 0 .. 7 at the initial pose, envs 8 .. 15 dropped in arbitrary poses (drawn
    as in the parity tests' drop poses) that meet between 9 and 14 ground contacts in some substep of the run and never more, so that
    every step stays in the fleet kernel.  The poses are picked by stepping NCAND candidates once under the action row the dropped envs share
    and reading each env's own counters (most contacts in a substep, steps redone by the large-capacity kernel)."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    cfg = make_config("flamingo_light_v1", random=PARITY_RANDOM, num_envs=N)
    cm = compile_model(cfg)
    nv = cm.blob.nv
    q0 = np.array(get_field(cm.blob, "init_qpos")[:cm.blob.nq])
    rng = np.random.default_rng(3)
    cand = np.stack([q0] * NCAND)
    for q in cand:
        quat = rng.normal(size=4)
        q[2] = rng.uniform(0.05, 0.25)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.3, 0.3, size=q.size - 7)
    table = _sin_table(STEPS, N, cm.blob.nu, 11)
    table[:, N // 2:] = table[:, N // 2:N // 2 + 1]                   # the dropped envs share one action row: one candidate run picks them all
    ccfg = make_config("flamingo_light_v1", random=PARITY_RANDOM, num_envs=NCAND)
    env = BatchedEnv(ccfg, num_envs=NCAND, auto_reset=False, compiled=cm)
    env.reset()
    env.set_state(cand, np.zeros((NCAND, nv)), np.zeros((NCAND, nv)))
    before = _meta(env)
    for t in range(STEPS):
        env.step(torch.tensor(np.repeat(table[t, N // 2][None], NCAND, axis=0), device=env.device))
    m = _meta(env)
    env.close()
    assert int(before[:, 10].max()) < 9                               # the reset at the initial pose: the maxima below are the run's
    most, fix = m[:, 10].cpu().numpy(), (m[:, 12] - before[:, 12]).cpu().numpy()
    poses = [i for i in range(NCAND) if 9 <= most[i] <= 14 and fix[i] == 0][:N // 2]
    assert len(poses) == N // 2, "too few candidate poses with 9 .. 14 contacts"
    qpos = np.concatenate([np.stack([q0] * (N // 2)), cand[poses]])
    return dict(cfg=cfg, cm=cm, qpos=qpos, table=table)


def _env(fleet, step_kernel):
    from cosim_amd.batched_env import BatchedEnv
    env = BatchedEnv(fleet["cfg"], num_envs=N, auto_reset=False, compiled=fleet["cm"])
    env.engine.set_param("step_kernel", np.array([float(step_kernel)]))
    assert env.engine.query("step_kernel") == step_kernel and env.engine.query("rollout") == 1
    env.reset()
    env.set_state(fleet["qpos"], np.zeros((N, fleet["cm"].blob.nv)), np.zeros((N, fleet["cm"].blob.nv)))
    return env


def _final(env):
    d = env.get_data()
    return {"qpos": d.qpos.clone(), "qvel": d.qvel.clone(), "meta": _meta(env)}, env.solver_stats()


def _bits(torch, x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("step_kernel", [1, 0])
def test_step_loop_with_batched_reads_equals_the_rollout_kernel_bit_for_bit(fleet, step_kernel):
    import torch
    a = _env(fleet, step_kernel)
    table = torch.tensor(fleet["table"], device=a.device)
    rows = {"states": [], "terminated": [], "truncated": [], "info": []}
    for t in range(STEPS):
        s, te, tr, _ = a.step(table[t])
        for k, v in zip(rows, (s, te, tr, a.info_buf)):
            rows[k].append(v.clone())
    fin_a, st_a = _final(a)
    a.close()
    b = _env(fleet, step_kernel)
    S, TE, TR, INF = b.rollout(table)
    fin_b, st_b = _final(b)
    b.close()
    print("solver counters, step loop:", st_a)
    print("solver counters, rollout:  ", st_b)
    for k, v in zip(rows, (S, TE, TR, INF)):
        assert torch.equal(_bits(torch, torch.stack(rows[k])), _bits(torch, v)), f"{k} differ between the step loop and the rollout"
    for k in fin_a:
        assert torch.equal(_bits(torch, fin_a[k]), _bits(torch, fin_b[k])), f"final {k} differs"
    assert st_a == st_b
    assert st_a["fixup_steps"] == 0 and st_a["dropped_contacts"] == 0 and st_a["nan_resets"] == 0
    assert st_a["max_contacts"] >= 9          # more than one batch of eight dense rows
    assert st_a["newton_iters"] > st_a["factorisations"] > 0   # some iterations solved with a factor read back from LDS
    assert torch.isfinite(S).all()

