"""The four observers together (episode ledger, failure traces, scenario checks, response curves: one begin hook behind reset / set /
restore and one step hook behind every range's step, csrc/cosim_engine.hip) against each of them armed alone.

Every observer kernel writes only its own buffers, so what one of them records does not depend on which others are armed: the same
script -- 130 flamingo_light_v1 on the plane (two full waves of 64 and two envs) in 2 ranges, auto-reset, a 25-step time limit and a
tilt rule, 40 steps from a fixed action table with a masked reset before step 10, a cosim_set of qvel before step 20 and a restore
that refuses one env before step 30 -- is run with all four armed and with each alone, and every buffer the engine hands out is
compared word for word."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS = 130, 40
SCN = [{"commands": [[0, 0.5, 0.0, 0.0, 0.0]],
        "checks": [[0, 25, "tracking_error", 0, "settle", "<", 0.3, "tracks"], [5, 20, "up", 0, "always", ">", 0.8, "upright"]],
        "curves": [[0, 25, 1, "info", "lin_vel_x", -1.0, 1.0, 8, "vx"], [0, 25, 2, "up", 0, 0.0, 1.0, 4, "upright"]]},
       {"checks": [[0, 25, "abs_info", "lin_vel_x", "mean", "<", 1.0, "vx"]], "curves": [[3, 20, 3, "qvel", 2, -1.0, 1.0, 0, "vz"]]},
       {"commands": [[0, 0.2, 0.0, 0.0, 0.0], [12, 0.6, 0.0, 0.2, 0.0]]},
       {"pushes": [[5, 10, 6.0, 0.0, 0.0]],                                   # throws the robot over: the tilt rule terminates it
        "checks": [[0, 25, "up", 0, "always", ">", 0.5, "stands"]], "curves": [[0, 25, 1, "torque_max", 0, 0.0, 20.0, 16, "torque"]]}]
ARMED = {"ledger": {"ledger": 4}, "traces": {"failure_traces": (8, 2)}, "checks": {"check_slots": 2}, "curves": {"curves": True}}
_MODEL = []


def _run(armed):
    """The script with the observers `armed` (names of ARMED); every buffer the engine hands out for them, as numpy words."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    from cosim_amd.fall import FallRule
    from cosim_amd.ftrace import HDR
    from cosim_amd.ledger import WORDS
    if not _MODEL:
        cfg = make_config("flamingo_light_v1", terrain="flat", max_duration=0.5)
        _MODEL.append((cfg, compile_model(cfg)))
    cfg, cm = _MODEL[0]
    kw = {"ledger": 0, "failure_traces": False}
    for name in armed:
        kw.update(ARMED[name])
    env = BatchedEnv(cfg, num_envs=N, compiled=cm, seed=3, auto_reset=True, ranges=2, scenarios=SCN, fall=FallRule(tilt=0.5), **kw)
    env.receive_user_command(np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)[:env.command_dim])
    table = torch.tensor(np.random.default_rng(11).uniform(-0.6, 0.6, size=(STEPS, N, env.action_dim)).astype(np.float32), device=env.device)
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    src = ((np.arange(N) * 7 + 3) % N).astype(np.int32)
    src[71] = N + 5                                                           # outside the snapshot: env 71 is refused and left alone
    snap = None
    env.reset()
    for k in range(STEPS):
        if k == 10:
            env.reset(mask)
        if k == 15:
            snap = env.snapshot()
        if k == 20:
            env.set_state(qvel=np.zeros((N, env.nv), dtype=np.float32))
        if k == 30:
            with pytest.raises(ValueError, match=r"source index of env 71 is outside \[0, 130\); 1 env\(s\) were left untouched"):
                env.restore(snap, src=src, mask=(np.arange(N) % 2).astype(np.uint8))
        env.step(table[k])
    env.join()
    t, eng, st, out = env.torch, env.engine, env._stream(), {}

    def buf(*shape):
        return t.empty(shape, dtype=t.int32, device=env.device)
    if "ledger" in armed:
        out["ledger"] = (buf(N, 4, WORDS), buf(N), buf(N, WORDS))
        eng.ledger_get(*(x.data_ptr() for x in out["ledger"]), st)
    if "traces" in armed:
        out["traces"] = (buf(N, 2 + 1, HDR + 8 * eng.query("ftrace_frame_words")), buf(N, 3), buf(N, HDR))
        eng.ftrace_get(*(x.data_ptr() for x in out["traces"]), st)
    if "checks" in armed:
        W = eng.query("scenario_check_words")
        out["checks"] = (buf(N, 2, W), buf(N), buf(N, W))
        eng.scenario_checks_get(*(x.data_ptr() for x in out["checks"]), st)
    if "curves" in armed:
        out["curves"] = (buf(eng.query("scenario_curve_words")),)
        eng.scenario_curves_get(out["curves"][0].data_ptr(), st)
        out["samples"] = env.curves().summary()["samples"]
    t.cuda.synchronize(env.device)
    out = {k: tuple(x.cpu().numpy() for x in v) if isinstance(v, tuple) else v for k, v in out.items()}
    env.close()
    return out


@pytest.fixture(scope="module")
def together():
    return _run(tuple(ARMED))


def test_each_artefact_is_there(together):
    rec, cnt, opn = together["ledger"]
    assert cnt.sum() > N, "every env ran into the time limit once; the pushed ones ended before it too"
    assert (rec[:, :, 2] & 1).any() and (rec[:, :, 2] & 2).any() and (opn[:, 2] & 16).all(), "terminated, truncated and open episodes"
    assert together["traces"][1][:, 1].sum() > 0, "no trace froze"
    assert together["checks"][1].sum() > N and together["checks"][0].any()
    assert together["samples"] > 0 and together["curves"][0].size > 0


@pytest.mark.parametrize("name", list(ARMED))
def test_all_armed_equals_armed_alone(together, name):
    alone = _run((name,))
    assert set(alone) - {"samples"} == {name}
    for what, a, b in zip(("records", "counts", "open"), together[name], alone[name]):
        assert a.shape == b.shape and a.dtype == b.dtype
        np.testing.assert_array_equal(a, b, err_msg=f"{name} {what}: all four armed against {name} alone")
