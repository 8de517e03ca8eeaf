"""Range streams (cosim_set_param "range_streams", csrc/cosim_ranges.h): R logical ranges carried by P <= R engine-owned streams, each
group of consecutive ranges stepped as ONE launch sequence over the union of its envs.  Envs never interact, so every comparison
here is bit for bit: P = 1, 2, 3, 4 over four ranges, and one range, give the same fleet.

Fleet: flamingo_light_v1 on the plane, 70 envs (ranges of 18, 18, 17, 17: uneven, and no group edge on a multiple of the fix-up
kernels' 64-env blocks), GUI-default domain randomisation + PD gains x U(0.9, 1.1), deferred join, auto-reset; max_duration = 0.5
puts the time limit in episode step 25, so 30 steps cross an auto-reset.  The extras test takes 96 envs like the tests it borrows
its tables from."""
import os

import numpy as np
import pytest

from scenario_cases import BASE, table5
from test_gpu_parity import parity   # noqa: F401  (the fixture: the model and rest pose the fix-up test of that file drops)

pytestmark = pytest.mark.gpu

N, R, K = 70, 4, 30
SIZES = [18, 18, 17, 17]
_CACHE = {}


def _model():
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    if "m" not in _CACHE:
        cfg = make_config("flamingo_light_v1", max_duration=0.5)            # GUI-default randomisation
        _CACHE["m"] = (cfg, compile_model(cfg))
    return _CACHE["m"]


def _fleet(n=N, ranges=R, streams=None, **kw):
    from cosim_amd.batched_env import BatchedEnv
    cfg, cm = _model()
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=7, auto_reset=True, gain_noise=0.1, ranges=ranges, deferred_join=ranges > 1,
                     streams=streams, **kw)
    env.receive_user_command(BASE)
    return env


def _actions(n, steps, seed=11):
    import torch
    a = np.random.default_rng(seed).uniform(-0.6, 0.6, size=(steps, n, 4)).astype(np.float32)
    return torch.tensor(a, device="cuda:0")                                 # a table: every step's rows outlive the step


def _final(env):
    """Everything a caller can read of the fleet after a run: outputs, physics state, counters (joins by itself)."""
    env.join()
    d = env.get_data()
    env.torch.cuda.synchronize(env.device)
    return dict(state=env.state.cpu().numpy().copy(), te=env.terminated.cpu().numpy().copy(), tr=env.truncated.cpu().numpy().copy(),
                info=env.info_buf.cpu().numpy().copy(), qpos=d.qpos.cpu().numpy().copy(), qvel=d.qvel.cpu().numpy().copy(),
                stats=env.solver_stats())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert a[k] == b[k], (what, k, a[k], b[k])
        else:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what} {k}")


def _run(env, acts, steps=K, record=False):
    rows = []
    for k in range(steps):
        env.step(acts[k])
        if record:
            env.join()
            env.torch.cuda.synchronize(env.device)
            rows.append((env.state.cpu().numpy().copy(), env.terminated.cpu().numpy().copy(), env.truncated.cpu().numpy().copy(),
                         env.info_buf.cpu().numpy().copy()))
    return rows


@pytest.fixture(scope="module")
def reference():
    """The fleet under four ranges on four streams -- the arrangement every earlier test of the suite ran -- computed once."""
    env = _fleet(streams=4)
    acts = _actions(N, K)
    env.reset()
    rows = _run(env, acts, record=True)
    fin = _final(env)
    env.close()
    assert fin["stats"]["episodes_ended"] >= N                              # the auto-reset happened inside the run
    return dict(acts=acts, rows=rows, final=fin)


@pytest.mark.parametrize("ranges, streams", [(4, 1), (4, 2), (4, 3), (1, None)])
def test_stream_counts_give_the_same_fleet(reference, ranges, streams):
    """30 steps with range_streams 1, 2, 3 (4 is the reference) and with ranges = 1: state, terminated, truncated, info of every
    step, the physics state and solver_stats() at the end."""
    env = _fleet(ranges=ranges, streams=streams)
    assert env.engine.query("ranges") == ranges and env.engine.query("range_streams") == (streams or 1)
    if ranges > 1:
        assert [c for _, c in env.range_list] == SIZES and [f for f, _ in env.range_list] == [0, 18, 36, 53]
    env.reset()
    rows = _run(env, reference["acts"], record=True)
    for k, (got, ref) in enumerate(zip(rows, reference["rows"])):
        for g, r, name in zip(got, ref, ("state", "terminated", "truncated", "info")):
            np.testing.assert_array_equal(_bits(g), _bits(r), err_msg=f"step {k} {name}")
    _same(_final(env), reference["final"], f"ranges {ranges} streams {streams}")
    env.close()


def test_back_to_back_steps_under_a_deferred_join(reference):
    """No join between the steps (what the bench does): the group chains of consecutive steps run ahead of each other."""
    env = _fleet(streams=2)
    env.reset()
    _run(env, reference["acts"])
    _same(_final(env), reference["final"], "deferred join")
    env.close()


def test_reported_streams():
    """cosim_query "range_streams" reports what was asked (clamped to the ranges); the stream handles of ``range_streams`` are equal
    inside a group and distinct across groups; auto follows the hardware queues the process was started with."""
    groups = {1: [0, 0, 0, 0], 2: [0, 0, 1, 1], 3: [0, 1, 2, 2], 4: [0, 1, 2, 3], 9: [0, 1, 2, 3]}   # range -> group: [g R / P, (g + 1) R / P)
    for asked, group in groups.items():
        env = _fleet(streams=asked)
        P = min(asked, R)
        assert env.engine.query("range_streams") == P and env.engine.query("ranges") == R
        assert len(env.range_streams) == R and len(env.range_list) == R
        h = [s.cuda_stream for s in env.range_streams]
        assert all(x != 0 for x in h)
        for i in range(R):
            for j in range(R):
                assert (h[i] == h[j]) == (group[i] == group[j]), (asked, i, j, h)
        assert [env.engine.range(i)[:2] for i in range(R)] == [(0, 18), (18, 18), (36, 17), (53, 17)]
        env.close()
    try:
        q = int(os.environ.get("GPU_MAX_HW_QUEUES", 4))
    except ValueError:
        q = 4
    q = q if q >= 1 else 4
    env = _fleet()                                                           # auto
    assert env.engine.query("range_streams") == min(R, max(1, q // 2))      # range_stream_count(4, Q), cosim_ranges.h
    env.engine.set_param("range_streams", np.array([3.0]))                  # set after "ranges": the streams are rebuilt
    assert env.engine.query("range_streams") == 3 and env.engine.query("ranges") == R
    env.engine.set_param("range_streams", np.array([0.0]))
    assert env.engine.query("range_streams") == min(R, max(1, q // 2))
    with pytest.raises(ValueError):
        env.engine.set_param("range_streams", np.array([-1.0]))
    env.close()
    one = _fleet(ranges=1)
    assert one.engine.query("range_streams") == 1 and one.range_streams == [None]
    one.close()


def _drop_poses(parity, want):   # noqa: F811
    """Poses of test_gpu_parity's fix-up test (the robot dropped on the ground in an arbitrary orientation, same generator and seed)
    that the oracle sees with more than 20 contacts after one control step: far beyond the fleet kernel's 14 slots."""
    from oracle.oracle import Oracle
    o = Oracle(parity["cm"])
    rng = np.random.default_rng(3)
    out = []
    for _ in range(200):
        q = parity["q0"].copy()
        quat = rng.normal(size=4)
        q[2] = rng.uniform(0.05, 0.25)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.3, 0.3, size=q.size - 7)
        o.reset(q)
        o.control_step(0.3 * np.sin(np.arange(4)))
        if o.ncon > 20:
            out.append(q)
        if len(out) == want:
            return np.array(out)
    raise AssertionError(f"only {len(out)} drop poses with more than 20 contacts")


def test_fixup_behind_a_group_launch(parity):   # noqa: F811
    """Envs of each group's SECOND range (ranges 1 and 3 under two streams) start from drop poses that overflow the 14 contact
    slots: the fix-up launch of a group scans the flags of the union (blocks of 64 from the group's first env, clamped to its end).
    fixup_steps > 0, nothing dropped, and the fleet equals the one stepped with one fix-up launch per range."""
    where = [20, 27, 35, 53, 60, 69]                                        # inside [18, 36) and [53, 70), both edges of the last
    poses = _drop_poses(parity, len(where))
    acts = _actions(N, 6, seed=5)
    got = {}
    for streams in (4, 2, 1):
        env = _fleet(streams=streams)
        assert env.engine.query("contact_slots") == 14 and env.engine.query("fixup_contact_slots") == 40
        env.reset()
        d = env.get_data()
        env.torch.cuda.synchronize(env.device)
        qpos, qvel = d.qpos.cpu().numpy().copy(), d.qvel.cpu().numpy().copy()
        qpos[where] = poses
        qvel[where] = 0.0
        env.set_state(qpos, qvel, np.zeros_like(qvel))
        _run(env, acts, steps=6)
        got[streams] = _final(env)
        env.close()
    st = got[4]["stats"]
    print("fixup_steps", st["fixup_steps"], "max_contacts", st["max_contacts"])
    assert st["fixup_steps"] >= len(where) and st["max_contacts"] > 14 and st["dropped_contacts"] == 0
    _same(got[2], got[4], "fix-up, two streams")
    _same(got[1], got[4], "fix-up, one stream")


def test_per_range_extras_follow_the_groups():
    """96 envs, four ranges, with a ledger, failure traces, a scenario table and a history ring all on: two streams against four.
    Ledger records, traces, applied commands, scenario rows and the ring's snapshots are equal, and so is the fleet after a restore
    from the ring."""
    n, steps = 96, 40
    acts = _actions(n, steps, seed=13)
    got = {}
    for streams in (4, 2):
        env = _fleet(n=n, streams=streams, ledger=4, failure_traces={"frames": 8, "keep": 2, "on": ("terminated", "truncated")},
                     scenarios=table5(), scenario_mode="cycle", history=(4, 5))
        assert env.engine.query("range_streams") == streams and env.engine.query("ledger_slots") == 4
        assert env.engine.query("ftrace_frames") == 8 and env.engine.query("scenario_rows") == 5 and env.engine.query("history_slots") == 4
        env.reset()
        cmds = []
        for k in range(steps):
            env.step(acts[k])
            if k % 7 == 3:
                env.join()
                env.torch.cuda.synchronize(env.device)
                cmds.append(env.applied_command.cpu().numpy().copy())
                cmds.append(np.asarray(env.scenario_rows()).astype(np.int64))
        led = env.ledger(include_open=True)
        tr = env.failure_traces(include_open=True)
        h0, h3 = env.history(0), env.history(3)
        env.torch.cuda.synchronize(env.device)
        out = dict(led_words=led.words.copy(), led_env=led.env.copy(), led_lost=led.lost.copy(), tr_headers=tr.headers.copy(),
                   tr_words=tr.words.copy(), tr_env=tr.env.copy(), tr_lost=tr.lost.copy(), h0=h0.rows.cpu().numpy().copy(),
                   h3=h3.rows.cpu().numpy().copy(), ages=np.array([h0.steps_ago, h3.steps_ago, h0.steps, h3.steps]))
        for i, c in enumerate(cmds):
            out[f"cmd{i}"] = c
        assert len(led.words) >= n and len(tr.words) >= n                   # every env ended an episode (time limit at step 25)
        assert h0.steps_ago == 0 and h3.steps_ago == 15
        env.restore(h3, params=True)                                        # back to step 25, then on: the restored fleet steps the same
        for k in range(25, 30):
            env.step(acts[k])
        out.update({"after_" + k: v for k, v in _final(env).items()})
        got[streams] = out
        env.close()
    _same(got[2], got[4], "extras")


def test_rollout_over_groups():
    """env.rollout of a 12-step table: two streams against four, and both against 12 calls of step()."""
    import torch
    steps = 12
    acts = _actions(N, steps, seed=17)
    ref = _fleet(streams=4)
    ref.reset()
    rows = _run(ref, acts, steps=steps, record=True)
    fin = _final(ref)
    ref.close()
    assert fin["stats"]["fixup_steps"] == 0                                 # (an abandoned env would finish in the large-capacity kernel)
    for streams in (4, 2):
        env = _fleet(streams=streams)
        assert env.engine.query("rollout") == 1
        env.reset()
        S, TE, TR, INF = env.rollout(acts)
        torch.cuda.synchronize()
        for k in range(steps):
            for g, r, name in zip((S[k], TE[k], TR[k], INF[k]), rows[k], ("state", "terminated", "truncated", "info")):
                np.testing.assert_array_equal(_bits(g.cpu().numpy()), _bits(r), err_msg=f"streams {streams} row {k} {name}")
        _same(_final(env), fin, f"rollout, {streams} streams")
        env.close()


def test_grouped_step_inside_a_captured_graph(reference):
    """One captured graph of three grouped steps (two fork edges, two join edges), replayed: the bits of the eager steps."""
    import torch
    env = _fleet(streams=2)
    acts = reference["acts"]
    env.reset()
    torch.cuda.synchronize()
    for k in range(3):                                                       # eager: steps 0..2, also the warm-up
        env.step(acts[k])
    env.join()
    torch.cuda.synchronize()
    buf = acts[3:6].clone()

    def chunk():
        for k in range(3):
            env.step(buf[k])
        env.join()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chunk()                                                              # capture only: steps 3..5 run at the first replay
    for c in range(1, K // 3):
        buf.copy_(acts[3 * c:3 * c + 3])
        g.replay()
    torch.cuda.synchronize()
    _same(_final(env), reference["final"], "graph")
    env.close()


def test_create_and_destroy_fifty_engines():
    """Teardown: engines with four ranges come and go (streams, done events and pacing events are destroyed with them)."""
    import torch
    for i in range(50):
        env = _fleet(n=8, streams=(i % 4) + 1)
        env.reset()
        env.step(torch.zeros((8, 4), device="cuda:0"))
        env.join()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(env.state).all())
        env.close()
