"""The step-only instantiation of the dense plane fleet kernels against the general one (``cosim_set_param "step_kernel"`` 1 / 0).

Both are the same source with the kernel mode either compiled in as "step" or read from the argument block; a control step is the same
arithmetic in the same order in both, so everything a step produces must be the same bits: the state vector, the flags, every info
array, qpos / qvel and the solver counters.  Reset, debug forward and replay always run the general instantiation (covered by the
parity tests)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _make(robot, n, step_kernel, random=None, max_duration=120.0, **kw):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, repr(random), max_duration)
    if key not in _make.cache:
        cfg = make_config(robot, random=random, max_duration=max_duration, num_envs=n, seed=5)
        _make.cache[key] = (cfg, compile_model(cfg))
    cfg, cm = _make.cache[key]
    env = BatchedEnv(cfg, num_envs=n, seed=5, compiled=cm, **kw)
    has = env.engine.query("step_kernel")                           # the default: 1 where the fleet has the instantiation
    assert has == HAS_STEP_KERNEL[robot]
    env.engine.set_param("step_kernel", np.array([float(step_kernel)]))
    assert env.engine.query("step_kernel") == (step_kernel if has else 0)
    return env


_make.cache = {}
# which plane fleets step with a step-only instantiation by default
HAS_STEP_KERNEL = {"flamingo_light_v1": 1, "flamingo_p_v3": 0}


def _sin_table(steps, n, nu, seed):
    """Seeded sinusoid action table [steps, n, nu]: amplitude, frequency and phase drawn per env and actuator."""
    rng = np.random.default_rng(seed)
    amp, freq, ph = rng.uniform(0.1, 0.6, (n, nu)), rng.uniform(0.3, 2.0, (n, nu)), rng.uniform(0, 2 * np.pi, (n, nu))
    t = 0.02 * np.arange(steps)[:, None, None]
    return (amp * np.sin(2 * np.pi * freq * t + ph)).astype(np.float32)


def _meta(env):
    torch = env.torch
    buf = torch.zeros((env.num_envs, 16), dtype=torch.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    torch.cuda.synchronize(env.device)
    return buf.view(torch.int32).clone()


def _snap(env, info):
    """Clones of everything a step returned (the env hands out views of fixed buffers)."""
    out = {"state": env.state.clone(), "terminated": env.terminated.clone(), "truncated": env.truncated.clone(), "info_buf": env.info_buf.clone()}
    for k, v in info.items():
        if env.torch.is_tensor(v):
            out["info." + k] = v.clone()
    return out


def _final(env):
    d = env.get_data()
    return {"qpos": d.qpos.clone(), "qvel": d.qvel.clone(), "meta": _meta(env)}, env.solver_stats()


def _assert_same(torch, a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:   # the bit patterns: a non-finite value (the info row of an env that blew up) must match too
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), f"{what}: {k} differs between step_kernel 1 and 0"


def _run_steps(env, table, shards=None):
    """Step through the table; shards = [(first, count), ...]: every step as range launches on caller streams, joined after the last
    range has been issued (a deferred join: no range waits for another inside the step)."""
    torch = env.torch
    acts = torch.tensor(table, device=env.device)
    streams = [torch.cuda.Stream(device=env.device) for _ in (shards or [])]
    env.reset()
    torch.cuda.synchronize(env.device)
    rows = []
    for t in range(acts.shape[0]):
        if shards is None:
            _, _, _, info = env.step(acts[t])
        else:
            for (first, count), st in zip(shards, streams):
                with torch.cuda.stream(st):
                    env.step_range(first, count, acts[t])
            for st in streams:
                torch.cuda.current_stream(env.device).wait_stream(st)
            env.join()
            info = env._info(acts[t])
        rows.append(_snap(env, info))
        torch.cuda.synchronize(env.device)
    return rows


def _compare_runs(robot, steps, shards=None, seed=1):
    import torch
    res = []
    for sk in (1, 0):
        env = _make(robot, 8, sk, max_duration=0.4, auto_reset=True, gain_noise=0.1)   # GUI-default randomisation
        assert env.max_sim_step == 20
        rows = _run_steps(env, _sin_table(steps, 8, env.action_dim, seed), shards)
        fin, stats = _final(env)
        env.close()
        res.append((rows, fin, stats))
    (r1, f1, s1), (r0, f0, s0) = res
    for t, (a, b) in enumerate(zip(r1, r0)):
        _assert_same(torch, a, b, f"step {t}")
    _assert_same(torch, f1, f0, "final")
    assert s1 == s0
    # the time limit fell inside the run and the envs went on: the auto-reset path is part of what was compared
    trunc = torch.stack([r["truncated"] for r in r1])
    assert int(trunc.sum()) >= 8 * (steps // 20) and s1["episodes_ended"] >= 8 * (steps // 20)
    assert s1["nan_resets"] == 0 and s1["newton_iters"] > 0
    return s1


def test_light_v1_steps_with_time_limit_resets_are_the_same_bits():
    _compare_runs("flamingo_light_v1", 60)


def test_light_v1_two_uneven_ranges_are_the_same_bits():
    one = _compare_runs("flamingo_light_v1", 60)
    two = _compare_runs("flamingo_light_v1", 60, shards=[(0, 5), (5, 3)])
    assert one == two                                               # and the sharded run is the run


def test_p_v3_steps_are_the_same_bits():
    _compare_runs("flamingo_p_v3", 40, seed=2)


def test_a_non_finite_env_is_reset_by_both_kernels():
    import torch
    res = []
    for sk in (1, 0):
        env = _make("flamingo_light_v1", 8, sk, max_duration=0.4, auto_reset=True, gain_noise=0.1)
        table = torch.tensor(_sin_table(4, 8, env.action_dim, 3), device=env.device)
        env.reset()
        env.step(table[0])
        d = env.get_data()
        qvel = d.qvel.clone()
        qvel[3, 7] = float("nan")
        env.set_state(qvel=qvel)
        rows = []
        for t in range(1, 4):
            _, _, _, info = env.step(table[t])
            rows.append(_snap(env, info))
        fin, stats = _final(env)
        env.close()
        res.append((rows, fin, stats))
    (r1, f1, s1), (r0, f0, s0) = res
    for t, (a, b) in enumerate(zip(r1, r0)):
        _assert_same(torch, a, b, f"step {t + 1}")
    _assert_same(torch, f1, f0, "final")
    assert s1 == s0 and s1["nan_resets"] == 1
    assert r1[0]["terminated"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]   # the step that met the non-finite state ended that env's episode
    assert torch.isfinite(f1["qpos"]).all() and torch.isfinite(f1["qvel"]).all() and torch.isfinite(r1[0]["state"]).all()


@pytest.fixture(scope="module")
def drop_poses():
    """Eight pre-step states whose control step ends with more than 14 ground contacts: the robot dropped in an arbitrary pose, as
    in test_more_contacts_than_the_fleet_kernel_holds_are_redone_not_dropped (test_gpu_parity.py)."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    from oracle.oracle import Oracle
    cfg = make_config("flamingo_light_v1", random=PARITY_RANDOM, num_envs=8)
    cm = compile_model(cfg)
    q0 = np.array(get_field(cm.blob, "init_qpos")[:cm.blob.nq])
    o = Oracle(cm)
    rng = np.random.default_rng(3)
    R = dict(qpos=[], qvel=[], warm=[], act=[])
    for trial in range(200):
        q = q0.copy()
        quat = rng.normal(size=4)
        q[2] = rng.uniform(0.05, 0.25)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.3, 0.3, size=q.size - 7)
        o.reset(q)
        for t in range(2):
            a = 0.3 * np.sin(0.3 * t + np.arange(4))
            pre = (o.qpos.copy(), o.qvel.copy(), o.qacc_warmstart.copy(), a)
            o.control_step(a)
            if o.ncon > 14:
                for k, v in zip(("qpos", "qvel", "warm", "act"), pre):
                    R[k].append(v)
        if len(R["qpos"]) >= 8:
            break
    assert len(R["qpos"]) >= 8
    return dict(cfg=cfg, cm=cm, **{k: np.array(v[:8]) for k, v in R.items()})


def test_steps_the_fleet_kernel_gives_up_are_redone_the_same(drop_poses):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    res = []
    for sk in (1, 0):
        env = BatchedEnv(drop_poses["cfg"], num_envs=8, auto_reset=False, compiled=drop_poses["cm"])
        env.engine.set_param("step_kernel", np.array([float(sk)]))
        assert env.engine.query("step_kernel") == sk and env.engine.query("contact_slots") == 14
        env.reset()
        env.set_state(drop_poses["qpos"], drop_poses["qvel"], drop_poses["warm"])
        act = torch.tensor(drop_poses["act"], dtype=torch.float32, device=env.device)
        rows = []
        for t in range(2):
            _, _, _, info = env.step(act)
            rows.append(_snap(env, info))
        fin, stats = _final(env)
        env.close()
        res.append((rows, fin, stats))
    (r1, f1, s1), (r0, f0, s0) = res
    for t, (a, b) in enumerate(zip(r1, r0)):
        _assert_same(torch, a, b, f"step {t}")
    _assert_same(torch, f1, f0, "final")
    assert s1 == s0
    assert s1["fixup_steps"] > 0 and s1["dropped_contacts"] == 0 and s1["max_contacts"] > 14


def test_rollout_rows_are_the_same_bits():
    import torch
    res = []
    for sk in (1, 0):
        env = _make("flamingo_light_v1", 8, sk, max_duration=0.4, auto_reset=True, gain_noise=0.1)
        assert env.engine.query("rollout") == 1
        table = torch.tensor(_sin_table(8, 8, env.action_dim, 4), device=env.device)
        env.reset()
        states, term, trunc, inf = env.rollout(table)
        fin, stats = _final(env)
        env.close()
        res.append(({"states": states, "terminated": term, "truncated": trunc, "info": inf}, fin, stats))
    (r1, f1, s1), (r0, f0, s0) = res
    _assert_same(torch, r1, r0, "rollout")
    _assert_same(torch, f1, f0, "final")
    assert s1 == s0 and s1["step_count"] > 0


@pytest.fixture(scope="module")
def cubic_impedance():
    """flamingo_light_v1 with an impedance curve no cosim model has: from 0.5 with power 3, midpoint 0.3, and a 1 cm zone so that the
    resting penetration (2.8 mm) lies inside it.  Every impedance of the step then goes through the general powf branch of the curve, which no
    other test reaches; at z0 the penetration is below the midpoint (x = 0.28), 0.6 mm lower above it (x = 0.34)."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field, set_field
    from oracle.oracle import Oracle
    cfg = make_config("flamingo_light_v1", random=PARITY_RANDOM, num_envs=4)

    def model(power):
        cm = compile_model(cfg)
        for name in ("geom_solimp", "ground_solimp", "jnt_solimp", "dof_solimp"):
            a = np.array(get_field(cm.blob, name), dtype=np.float64)
            b = a.reshape(-1, 5).copy()
            b[:, 0], b[:, 2], b[:, 3], b[:, 4] = 0.5, 0.01, 0.3, power
            set_field(cm.blob, name, b.reshape(a.shape))
        return cm
    cm3, cm2 = model(3.0), model(2.0)
    q0 = np.array(get_field(cm3.blob, "init_qpos")[:cm3.blob.nq])
    poses, f3, f2 = [], [], []
    for dz in (0.0, -0.0006):
        q = q0.copy()
        q[2] += dz
        poses.append(q)
        for cm, out in ((cm3, f3), (cm2, f2)):
            o = Oracle(cm)
            o.reset(q)
            o.forward()
            out.append(o.qfrc_constraint.copy())
    return dict(cfg=cfg, cm=cm3, poses=np.array(poses), f3=np.array(f3), f2=np.array(f2))


def test_a_cubic_impedance_curve_follows_the_oracle_and_is_the_same_bits_in_both_kernels(cubic_impedance):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    C = cubic_impedance
    nv = 18
    # the bound of test_forward_stages_match_oracle on qfrc_constraint; the quadratic curve with the same midpoint is > 10 bounds away
    bound = 1e-3 + 1e-4 * np.abs(C["f3"])
    assert (np.abs(C["f3"] - C["f2"]) > 10 * bound).any(axis=1).all()
    res = []
    for sk in (1, 0):
        env = BatchedEnv(C["cfg"], num_envs=4, auto_reset=False, compiled=C["cm"])
        env.engine.set_param("step_kernel", np.array([float(sk)]))
        env.reset()
        env.set_state(qpos=np.repeat(C["poses"], 2, axis=0), qvel=np.zeros((4, nv)), qacc_warmstart=np.zeros((4, nv)))
        for i, e in enumerate((0, 2)):   # debug forward (the general instantiation) at the pose below / above the midpoint
            D = env.engine.debug_forward(e)
            assert (np.abs(D[1040:1040 + nv] - C["f3"][i]) <= bound[i]).all(), (i, D[1040:1040 + nv], C["f3"][i])
        act = torch.tensor(_sin_table(3, 4, env.action_dim, 6), device=env.device)
        rows = []
        for t in range(3):
            _, _, _, info = env.step(act[t])
            rows.append(_snap(env, info))
        fin, stats = _final(env)
        env.close()
        res.append((rows, fin, stats))
    (r1, f1, s1), (r0, f0, s0) = res
    for t, (a, b) in enumerate(zip(r1, r0)):
        _assert_same(torch, a, b, f"step {t}")
    _assert_same(torch, f1, f0, "final")
    assert s1 == s0 and torch.isfinite(f1["qpos"]).all()
