"""Episode ledger on the device (cosim_ledger_set / cosim_ledger_get, csrc/cosim_ledger.hip, and its BatchedEnv / reporter / CLI
surface) against its numpy twin (cosim_amd/ledger.py reference_ledger) fed with the step outputs recorded on the host.

Every comparison is EXACT (ledger.same_records): ints as ints, floats as float32 bits; where both sides are non-finite (the info row
of a step that ended in a non-finite state) "both non-finite" is enough.  Fleets are at most 96 envs and 80 steps; max_duration = 0.5
puts the time limit in step 25, as in test_gpu_snapshot.py; actions come from a fixed table.  Each test asserts that what it is about
-- an auto-reset, a termination, an overflow of the ring -- happened."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
CMD = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)


def _model(robot, terrain="flat", random=None, **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, json.dumps(random, sort_keys=True), json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, random=random, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _env(cfg, cm, n, seed=3, **kw):
    from cosim_amd.batched_env import BatchedEnv
    kw.setdefault("auto_reset", True)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=seed, **kw)
    env.receive_user_command(CMD[:env.command_dim] if env.command_dim != 2 else np.array([1.0, 0.5], dtype=np.float32))
    return env


def _table(env, steps, seed=11):
    import torch
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.6, 0.6, size=(steps, env.num_envs, env.action_dim)).astype(np.float32)
    return torch.tensor(a, device=env.device)


def _meta(env):
    """(meta word 4, spawn row or -1) of every env now."""
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    m = buf.view(t.int32).cpu().numpy()
    spawn = m[:, 14].copy() if env.engine.query("spawn_rows") > 0 else np.full(env.num_envs, -1, dtype=np.int32)
    return m[:, 4].copy(), spawn


class _Rec:
    """Step outputs of a run, recorded on the host step by step; ``between(k)`` hooks run before step k."""

    def __init__(self, env):
        self.env, self.info, self.te, self.tr, self.nan, self.spawn = env, [], [], [], [], []

    def run(self, table, k0, k1):
        env = self.env
        for k in range(k0, k1):
            n, s = _meta(env)
            self.nan.append(n); self.spawn.append(s)
            env.step(table[k])
            env.join()
            env.torch.cuda.synchronize(env.device)
            self.info.append(env.info_buf.cpu().numpy().copy())
            self.te.append(env.terminated.cpu().numpy().copy()); self.tr.append(env.truncated.cpu().numpy().copy())

    def twin(self, slots, **kw):
        from cosim_amd.ledger import reference_ledger
        env = self.env
        n, s = _meta(env)
        return reference_ledger(np.stack(self.info), np.stack(self.te), np.stack(self.tr), env.user_command.cpu().numpy(),
                                np.stack(self.nan + [n]), np.stack(self.spawn + [s]), slots, env.action_dim, env.command_dim,
                                env_id0=env.env_id0, **kw)

    def ended(self):
        return int((np.stack(self.te) | np.stack(self.tr)).astype(bool).sum())


def _assert_same(a, b):
    from cosim_amd.ledger import same_records
    diff = same_records(a, b)
    assert diff is None, diff


# ------------------------------------------------------------------------------------------------------------ 1: twin, dense kernel
def test_twin_dense_kernel_with_auto_resets():
    """flamingo_light_v1 flat, 96 envs (one full lane group of the ledger kernel and a 32-env tail), GUI-default randomisation, 60
    steps: two time limits per env."""
    from cosim_amd.reporter import FleetReporter
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)
    env = _env(cfg, cm, 96, ledger=4)
    assert env.engine.query("ledger_slots") == 4
    table = _table(env, 60)
    env.reset()
    ended0 = env.solver_stats()["episodes_ended"]
    rec = _Rec(env)
    rec.run(table, 0, 60)
    assert rec.ended() >= 2 * 96, "no auto-reset inside the run"
    led = env.ledger()
    _assert_same(led, rec.twin(4))
    assert len(led) == rec.ended() and int(led.lost.sum()) == 0 and (led.spawn_row == -1).all()
    assert len(led) + int(led.lost.sum()) == env.solver_stats()["episodes_ended"] - ended0
    assert set(led.length.tolist()) == {25} and set(led.flags.tolist()) == {2} and led.steps_seen.max() == 50
    assert np.isfinite(led.mean_abs_torque).all() and (led.peak_abs_torque > 0).all() and (led.mean_tracking_err_0 > 0).all()
    opn = env.ledger(include_open=True)
    _assert_same(opn, rec.twin(4, include_open=True))
    o = (opn.flags & 16) != 0
    assert int(o.sum()) == 96 and set(opn.length[o].tolist()) == {10} and set(opn.episode[o].tolist()) == {2}
    # the reporter's block is the ledger's summary
    s = FleetReporter(env).summary()["episodes"]
    assert s["episodes"] == len(led) and s["truncated"] == len(led) and s["terminated"] == 0 and s["length"]["p50"] == 25.0
    assert s["by_spawn_row"] == {"-1": {"episodes": len(led), "terminated": 0, "terminated_share": 0.0}}
    env.close()


# ------------------------------------------------------------------------------------------------------------ 2: terminations
def test_terminations_and_non_finite_resets():
    """flamingo_p_v3 (the robot with a contact termination) on the plane, 48 envs: every other env is laid on its side, env 1 gets a
    non-finite qvel.  set_state touches every env, so every env's first episode carries flag 8."""
    cfg, cm = _model("flamingo_p_v3", "flat", max_duration=0.5)
    env = _env(cfg, cm, 48, ledger=8)
    table = _table(env, 40)
    env.reset()
    d = env.get_data()
    env.torch.cuda.synchronize(env.device)
    qpos, qvel = d.qpos.cpu().numpy().copy(), d.qvel.cpu().numpy().copy()
    side = np.arange(48) % 2 == 0
    qpos[side, 3:7] = np.array([np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0], dtype=np.float32)   # rolled by 90 degrees
    qvel[1, 0] = np.nan
    env.set_state(qpos, qvel)
    rec = _Rec(env)
    rec.run(table, 0, 40)
    te, tr = np.stack(rec.te).astype(bool), np.stack(rec.tr).astype(bool)
    assert te[0, 1] and env.solver_stats()["nan_resets"] >= 1, "the non-finite state did not reset env 1"
    fell = te[:, side].any(axis=0)
    assert fell.all(), f"envs laid on their side that did not terminate: {np.nonzero(side)[0][~fell].tolist()}"
    led = env.ledger()
    _assert_same(led, rec.twin(8, begins=[(0, None, 8)]))
    assert int(led.lost.sum()) == 0 and len(led) == rec.ended()
    first = led.episode == 0
    assert ((led.flags[first] & 8) != 0).all() and ((led.flags[~first] & 8) == 0).all()
    e1 = led.env == 1
    assert led.flags[e1][0] == (1 | 4 | 8) and led.length[e1][0] == 1
    # a one-step episode's means are that step's values, whatever the non-finite state left in the info row (the velocimeter's
    # cutoff, an fminf / fmaxf pair, turns a NaN lin_vel_x into -cutoff)
    row = rec.info[0][1]
    for got, want in ((led.mean_action_diff_RMSE[e1][0], row[0]), (led.mean_lin_vel_x[e1][0], row[1])):
        assert (not np.isfinite(got) and not np.isfinite(want)) or np.float32(got).view(np.int32) == np.float32(want).view(np.int32)
    fallen = first & np.isin(led.env, np.nonzero(side)[0])
    assert (led.flags[fallen] == (1 | 8)).all() and (led.length[fallen] < 25).all()
    # every record's flags are the step outputs' of the step that ended it (steps_seen counts the env's rows)
    for r in range(len(led)):
        k, n = led.steps_seen[r] - 1, led.env[r]
        assert bool(led.flags[r] & 1) == te[k, n] and bool(led.flags[r] & 2) == tr[k, n]
    assert led.summary()["non_finite"] == env.solver_stats()["nan_resets"]
    env.close()


# ------------------------------------------------------------------------------------------------------------ 3: ring overflow
def test_ring_overflow_keeps_the_last_episodes():
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)
    env = _env(cfg, cm, 32, ledger=2)
    table = _table(env, 80)
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, 80)
    assert rec.ended() == 3 * 32, "not three ended episodes per env"
    led = env.ledger()
    assert (led.lost == 1).all() and len(led) == 2 * 32
    assert led.episode.reshape(32, 2).tolist() == [[1, 2]] * 32 and led.steps_seen.reshape(32, 2).tolist() == [[50, 75]] * 32
    _assert_same(led, rec.twin(2))
    _assert_same(env.ledger(include_open=True), rec.twin(2, include_open=True))
    env.close()


# ------------------------------------------------------------------------------------------------------------ 4: launch invariance
def test_every_launch_path_gives_the_same_ledger():
    """One action table through: 1 range; 4 ranges with deferred join; rollout(); step_range chains on four streams (the pattern of
    Runner.test_pipelined); a graph-captured step replayed.  64 envs, 40 steps."""
    import torch
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)
    n, K = 64, 40
    a = _env(cfg, cm, n, ledger=4)
    table = _table(a, K)
    a.reset()
    for k in range(K):
        a.step(table[k])
    ref = a.ledger(include_open=True)
    assert int(((ref.flags & 16) == 0).sum()) == n, "no auto-reset inside the run"
    a.close()

    b = _env(cfg, cm, n, ledger=4, ranges=4, deferred_join=True)
    assert b.engine.query("ranges") == 4
    b.reset()
    for k in range(K):
        b.step(table[k])
    _assert_same(b.ledger(include_open=True), ref)
    b.close()

    c = _env(cfg, cm, n, ledger=4)
    assert c.engine.query("rollout") == 1
    c.reset()
    c.rollout(table)
    _assert_same(c.ledger(include_open=True), ref)
    c.close()

    d = _env(cfg, cm, n, ledger=4)
    d.reset()
    streams = [torch.cuda.Stream(device=d.device) for _ in range(4)]
    torch.cuda.synchronize(d.device)
    for k in range(K):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                d.step_range(i * (n // 4), n // 4, table[k])
    torch.cuda.synchronize(d.device)
    _assert_same(d.ledger(include_open=True), ref)
    d.close()

    g = _env(cfg, cm, n, ledger=4)
    g.reset()
    buf = torch.empty((n, g.action_dim), device=g.device)
    side = torch.cuda.Stream(device=g.device)
    buf.copy_(table[0])
    torch.cuda.synchronize(g.device)
    side.wait_stream(torch.cuda.current_stream(g.device))
    with torch.cuda.stream(side):
        g.step(buf)                                                        # warm-up, eager: step 0
    torch.cuda.current_stream(g.device).wait_stream(side)
    torch.cuda.synchronize(g.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(buf)                                                        # recorded, not run: the ledger launch is part of the graph
    for k in range(1, K):
        buf.copy_(table[k])
        graph.replay()
    torch.cuda.synchronize(g.device)
    _assert_same(g.ledger(include_open=True), ref)
    g.close()


# ------------------------------------------------------------------------------------------------------------ 5: split pipeline
@pytest.mark.parametrize("fixup", [False, True], ids=["split", "split_fixup"])
def test_split_pipeline(fixup):
    """humanoid_p_v0 on stairs_up_hard: the ledger launch follows the last substep's launches (and their fix-up)."""
    cfg, cm = _model("humanoid_p_v0", "stairs_up_hard", max_duration=0.5, position_command=True)
    env = _env(cfg, cm, 8, ledger=4, **({"hfield_fixup": True} if fixup else {}))
    assert env.engine.query("split") > 0
    table = _table(env, 30)
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, 30)
    assert rec.ended() >= 8, "no episode ended inside the run"
    led = env.ledger(include_open=True)
    _assert_same(led, rec.twin(4, include_open=True))
    assert int(((led.flags & 16) == 0).sum()) == rec.ended()
    env.close()


# ------------------------------------------------------------------------------------------------------------ 6: spawn rows
def test_spawn_rows_per_episode():
    cfg, cm = _model("flamingo_light_v1", "rocky_easy", max_duration=0.5)
    env = _env(cfg, cm, 32, ledger=4, spawn={"pattern": "grid", "count": 5, "extent": 20.0, "per_episode": True})
    assert env.engine.query("spawn_rows") == 5 and env.engine.query("spawn_mode") == 1
    table = _table(env, 60)
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, 60)
    rows_before = np.stack(rec.spawn + [env.spawn_rows().astype(np.int32)])   # [61, 32]: env.spawn_rows() before step k
    assert rec.ended() >= 2 * 32
    led = env.ledger()
    _assert_same(led, rec.twin(4))
    done = (np.stack(rec.te) | np.stack(rec.tr)).astype(bool)
    expect = {}
    r = 0
    for n in range(32):
        start = 0
        for k in np.nonzero(done[:, n])[0]:
            assert led.env[r] == n and led.steps_seen[r] == k + 1
            assert led.spawn_row[r] == rows_before[start, n]              # what env.spawn_rows() returned at the episode's start
            e = expect.setdefault(int(rows_before[start, n]), [0, 0])
            e[0] += 1
            e[1] += int(np.stack(rec.te)[k, n] != 0)
            start = k + 1
            r += 1
    assert r == len(led) and len(expect) > 1, "every episode started from the same row"
    by = led.by_spawn_row()
    assert {k: (v["episodes"], v["terminated"]) for k, v in by.items()} == {k: tuple(v) for k, v in expect.items()}
    assert all(v["terminated_share"] == v["terminated"] / v["episodes"] for v in by.values())
    env.close()


# ------------------------------------------------------------------------------------------------------------ 7: host resets, restores
def test_masked_reset_and_restore():
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)
    n = 16
    env = _env(cfg, cm, n, ledger=4)
    table = _table(env, 52)
    lo, hi = np.arange(n) < 8, np.arange(n) >= 8
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, 10)
    snap = env.snapshot()
    rec.run(table, 10, 15)
    env.reset(mask=lo)                                                      # discards the 15-step open episode of envs 0..7 only
    opn = env.ledger(include_open=True)
    assert len(opn) == n and opn.length[lo].tolist() == [0] * 8 and opn.length[hi].tolist() == [15] * 8
    assert opn.steps_seen.tolist() == [15] * n and (opn.episode == 0).all() and (opn.flags == 16).all()
    assert (opn.words[lo, 5:] == 0).all()                                   # means 0 at length 0
    rec.run(table, 15, 27)                                                  # envs 8..15 reach the time limit in step 25
    before = env.ledger(include_open=True)
    assert before.env[(before.flags & 16) == 0].tolist() == list(range(8, 16))
    env.restore(snap, mask=hi)                                              # sim_step 10 again: 15 more steps to the time limit
    after = env.ledger(include_open=True)
    keep = np.isin(after.env, np.arange(8)) | ((after.flags & 16) == 0)
    np.testing.assert_array_equal(after.words[keep], before.words[keep])    # the others' rows and the ended records: untouched
    o = ~keep
    assert after.env[o].tolist() == list(range(8, 16)) and (after.flags[o] == (16 | 8)).all() and (after.length[o] == 0).all()
    assert (after.episode[o] == 1).all() and (after.steps_seen[o] == 27).all()
    rec.run(table, 27, 52)
    led = env.ledger()
    _assert_same(led, rec.twin(4, begins=[(15, lo, 0), (27, hi, 8)]))
    # envs 0..7: reset at 15 -> episodes of 25 steps end in steps 40 (and none later); envs 8..15: 25, then 15 steps with flag 8, then open
    assert led.length[np.isin(led.env, np.arange(8))].tolist() == [25] * 8
    assert led.length[led.env >= 8].reshape(8, 2).tolist() == [[25, 15]] * 8 and led.flags[led.env >= 8].reshape(8, 2).tolist() == [[2, 2 | 8]] * 8
    env.close()


# ------------------------------------------------------------------------------------------------------------ 8: refusals, lifecycle
def test_refusals_and_lifecycle():
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)
    env = _env(cfg, cm, 16)
    table = _table(env, 6)
    env.reset()
    assert env.engine.query("ledger_slots") == 0
    with pytest.raises(ValueError, match="no ledger"):
        env.ledger()
    for slots in (-1, 4097):
        with pytest.raises(ValueError, match="slots"):
            env.set_ledger(slots)
    env.step(table[0])
    env.set_ledger(3)                                                       # on a stepped fleet: the open episodes carry flag 8
    assert env.engine.query("ledger_slots") == 3
    opn = env.ledger(include_open=True)
    assert len(opn) == 16 and (opn.flags == (16 | 8)).all() and (opn.length == 0).all()
    with pytest.raises(ValueError, match="ledger"):
        env.rollout(table[1:3], info=False)
    with pytest.raises(ValueError, match="info_out_dev"):
        env.engine.step(table[1].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(), None,
                        env._stream())
    with pytest.raises(ValueError, match="info_out_dev"):
        env.engine.rollout(1, table[1:2].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(),
                           None, env._stream())
    env.step(table[1])
    assert env.ledger(include_open=True).length.tolist() == [1] * 16        # the refused calls stepped nothing
    env.reset()                                                             # a whole-fleet reset: the next ledger starts clean
    env.set_ledger(2)
    assert (env.ledger(include_open=True).flags == 16).all()
    env.set_ledger(0)                                                       # off: no ledger launch, and no info buffer is needed again
    assert env.engine.query("ledger_slots") == 0
    env.rollout(table[2:4], info=False)
    env.engine.step(table[4].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(), None,
                    env._stream())
    env.torch.cuda.synchronize(env.device)
    with pytest.raises(ValueError, match="no ledger"):
        env.ledger()
    assert env.solver_stats()["step_count"] == 16 * (1 + 1 + 1 + 1 + 2 + 1)   # two resets, steps 0 and 1, a 2-step rollout, one step
    env.close()


def test_single_env_adapter_gets_no_ledger():
    from cosim_amd.build import build_env
    cfg, _ = _model("flamingo_light_v1", "flat", max_duration=0.5)
    cfg = dict(cfg, engine=dict(cfg["engine"], num_envs=1, ledger=4))
    single = build_env(cfg)
    assert single.env.ledger_slots == 0 and single.env.engine.query("ledger_slots") == 0
    single.close()


def test_cli_ledger(tmp_path, capsys):
    from cosim_amd import cli
    from cosim_amd.ledger import EpisodeLedger
    report, out = tmp_path / "r.json", tmp_path / "episodes.npz"
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "16", "--steps", "60", "--max-duration", "0.5", "--seed", "5",
                     "--ledger", "4", "--ledger-out", str(out), "--report", str(report)]) == 0
    r = json.loads(report.read_text())
    led = EpisodeLedger.load(str(out))
    assert r["episodes"]["episodes"] == len(led) == r["episodes_ended"] >= 32 and r["episodes"]["lost"] == 0
    assert r["episodes"] == json.loads(json.dumps({**led.summary(), "by_spawn_row": {str(k): v for k, v in led.by_spawn_row().items()}}))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["episodes"]["episodes"] == len(led) and line["episodes"]["truncated"] == len(led)
