"""Every device allocation of the library has an owner (csrc/cosim_devbuf.h): one lifecycle of everything that allocates, with the
count of live allocations (``cosim_query "device_buffers"``, process-wide) read at every station.  flamingo_light_v1 on flat ground,
8 envs, 2 ranges: set, step, rewrite in place, lay out anew, clear, again; the policy tables; close.  Nothing is provoked: the count
after a clear is the count before the set, exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, CD = 8, 4


def _scenarios(k=0):
    """Two scenarios with every kind of item; ``k`` moves values and leaves every size."""
    f = 1.0 + 0.1 * k
    row0 = {"commands": [[0, 0.2 * f, 0.0, 0.0, 0.0], [6, 0.4 * f, 0.0, 0.0, 0.0]],
            "pushes": [[2, 5, 0.0, 1.0 * f, 0.0]],
            "params": [[0, 25, "kp", 0, "scale", 0.9 * f], [3, 20, "geom_friction", "*", "scale", 0.8]],
            "faults": [[0, 25, "ang_vel", "*", "bias", 0.05 * f]],
            "action_faults": [[0, 25, 0, "bias", 0.1 * f]],
            "latency": [[0, 100, "action", "*", 2 - k], [0, 100, "dof_vel", "*", 2 - k]],
            "checks": [[0, 25, "tracking_error", 0, "settle", "<", 0.3 * f, "tracks"]],
            "curves": [[0, 25, 1, "torque_max", 0, 0.0, 50.0 * f, 8, "torque"]],
            "search": {"lo": 1.0, "hi": 4.0 * f, "rule": "bisect", "trials": 3, "targets": ["pushes"], "fail_on": ["terminated"]}}
    row1 = {"commands": [[0, 0.3, 0.0, 0.0, 0.0]], "action_faults": [[1, 9, 1, "scale", 0.5 * f]],
            "checks": [[0, 25, "up", 0, "always", ">", 0.1, "upright"]], "curves": [[0, 12, 2, "up", 0, 0.0, 1.0, 4, "up"]]}
    return [row0, row1]


def _other_sizes():
    rows = _scenarios()
    rows[1]["pushes"] = [[1, 3, 0.5, 0.0, 0.0], [8, 9, 0.0, 0.5, 0.0]]
    rows[1]["latency"] = [[0, 50, "action", 0, 4]]
    rows.append({"commands": [[0, 0.1, 0.0, 0.0, 0.0]], "params": [[0, 9, "kd", 1, "scale", 1.1]],
                 "curves": [[0, 30, 1, "abs_info", 0, 0.0, 9.0, 16, "vx"], [0, 8, 1, "qvel", 2, -1.0, 1.0, 0, "vz"]]})
    return rows


def _env():
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    cfg = make_config("flamingo_light_v1", terrain="flat", random=None, max_duration=0.5)
    env = BatchedEnv(cfg, num_envs=N, compiled=compile_model(cfg), seed=3, auto_reset=True, ranges=2, ledger=0, failure_traces=False)
    assert env.command_dim == CD
    env.receive_user_command(np.array([0.3, 0.0, 0.1, 0.0], dtype=np.float32))
    return env


def _steps(env, k):
    act = env.torch.zeros((N, env.action_dim), device=env.device)
    for _ in range(k):
        env.step(act)
    env.join()
    env.torch.cuda.synchronize(env.device)


def _arm_step_clear(env, count):
    t = env.torch
    env.set_ledger(2)
    env.set_failure_traces((4, 1))
    env.engine.history_set(2, 1)
    env.set_spawn(np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.1], [1.0, 0.5, 0.2]], dtype=np.float32))
    env.set_scenarios(_scenarios(), check_slots=2, curves=True, search=2)
    q = env.engine.query
    assert q("ledger_slots") == 2 and q("ftrace_frames") == 4 and q("history_slots") == 2 and q("spawn_rows") == 3 and q("scenario_rows") == 2
    assert q("scenario_param_items") > 0 and q("obs_faults") > 0 and q("action_faults") > 0 and q("latency_action_items") > 0 and q("latency_obs_items") > 0
    assert q("scenario_check_slots") == 2 and q("scenario_curve_items") == 2 and q("search") == 1 and q("search_slots") == 2
    groups = t.tensor([0, 1] * (N // 2), dtype=t.int32, device=env.device)
    env.set_curve_groups(groups, n_groups=2)
    assert q("scenario_curve_groups") == 2
    env.reset()
    _steps(env, 3)
    armed = count()
    env.set_scenarios(_scenarios(1), check_slots=2, curves=True, search=2)                  # other values, the same sizes: in place
    assert count() == armed and q("scenario_curve_groups") == 2
    _steps(env, 1)
    env.set_scenarios(_other_sizes(), check_slots=3, curves=True, search=3)                 # other sizes and slot counts: laid out anew
    assert q("scenario_rows") == 3 and q("scenario_check_slots") == 3 and q("search_slots") == 3 and q("scenario_curve_groups") == 0
    _steps(env, 1)
    env.set_scenarios(None)
    env.set_ledger(0)
    env.set_failure_traces(None)
    env.engine.history_set(0, 1)
    env.set_spawn(None)
    assert q("scenario_rows") == 0 and q("ledger_slots") == 0 and q("ftrace_frames") == 0 and q("history_slots") == 0 and q("spawn_rows") == 0
    assert q("latency") == 0 and q("search") == 0 and q("scenario_curve_items") == 0 and q("scenario_check_items") == 0


def _recurrent_file(path, seed):
    from cosim_amd.onnx_io import write_recurrent_actor
    rng = np.random.default_rng(seed)
    I, H = 11, 8
    lstm = ((rng.standard_normal((4 * H, I)) / np.sqrt(I)).astype(np.float32), (rng.standard_normal((4 * H, H)) / np.sqrt(H)).astype(np.float32),
            (0.2 * rng.standard_normal(8 * H)).astype(np.float32))
    head = [((0.5 * rng.standard_normal((4, H)) / np.sqrt(H)).astype(np.float32), (0.5 * rng.standard_normal(4)).astype(np.float32), None, 0.3)]
    write_recurrent_actor(path, [], lstm, head)


def test_nothing_is_left_behind(tmp_path):
    import torch
    from cosim_amd.policy import PolicyTable, RecurrentPolicyTable, write_random_mlp
    a = _env()                                                                              # stays alive only to query
    count = lambda: a.engine.query("device_buffers")   # noqa: E731
    c0 = count()
    assert c0 > 0
    b = _env()
    b.reset()
    snap = b.snapshot()
    b.restore(snap, src=torch.arange(N, dtype=torch.int32, device=b.device).flip(0))       # the persistent error pair exists from here on
    c1 = count()
    assert c1 > c0
    for _ in range(2):
        _arm_step_clear(b, count)
        assert count() == c1
    files = [str(tmp_path / f"p{k}.onnx") for k in range(2)]
    for k, f in enumerate(files):
        write_random_mlp(f, 12, 4, hidden=(16,), seed=40 + k)
    rec = [str(tmp_path / f"r{k}.onnx") for k in range(2)]
    for k, f in enumerate(rec):
        _recurrent_file(f, 50 + k)
    assign = np.array([0, 1] * (N // 2))
    tab = PolicyTable(files, num_envs=N, device="cuda:0", assign=assign, rotate_every=1)
    rtab = RecurrentPolicyTable(rec, num_envs=N, device="cuda:0", assign=assign, rotate_every=1)
    assert tab._handle is not None and rtab._handle is not None and count() > c1
    out = tab.get_action(torch.zeros((N, 12), device="cuda:0"))
    rout = rtab.get_action(torch.zeros((N, 11), device="cuda:0"))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(rout).all())
    tab.close()
    rtab.close()
    assert count() == c1
    b.close()
    assert count() == c0
    a.close()
