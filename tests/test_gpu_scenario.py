"""Scenario tables on the device (cosim_scenario_set, csrc/cosim_scenario.hip, and their BatchedEnv / ledger / reporter / CLI surface)
against a host-driven loop: an env with no table that is given, before every step, the command and the push the numpy twin
(cosim_amd/scenario.py reference_schedule) works out from the meta words read back from the device.

Every comparison is EXACT: float32 bits for floats, ints as ints.  Fleets are at most 96 envs, runs at most 80 steps; max_duration =
0.5 puts the time limit in episode step 25, as in test_gpu_ledger.py; actions come from a fixed table.  Each test asserts that what it
is about -- auto-resets, a push that changed qvel, a keyframe that fired -- happened."""
import json

import numpy as np
import pytest

from scenario_cases import BASE, CD, NEVER, TABLE5, table5, table5_variant

pytestmark = pytest.mark.gpu

_CACHE = {}
N, K, RESET_AT = 96, 60, 30
RESET_MASK = (np.arange(N) % 3 == 1)


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


def _env(cfg, cm, n, base=BASE, seed=3, **kw):
    from cosim_amd.batched_env import BatchedEnv
    kw.setdefault("auto_reset", True)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=seed, **kw)
    env.receive_user_command(np.asarray(base, dtype=np.float32))
    return env


def _actions(n, steps, nu, seed=11):
    return np.random.default_rng(seed).uniform(-0.6, 0.6, size=(steps, n, nu)).astype(np.float32)


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().copy()


def _qvel(env):
    d = env.get_data()
    env.torch.cuda.synchronize(env.device)
    return d.qvel.cpu().numpy().copy()


class _Run:
    """One run, recorded step by step.  ``device``: the env carries the table and the host only checks the twin against
    ``applied_command`` / ``scenario_rows()``; otherwise the host drives: twin -> receive_user_command + event("push") -> step."""

    def __init__(self, env, table, mode, base=BASE, device=True, check=True):
        self.env, self.table, self.mode, self.device, self.check = env, table, mode, device, check
        self.base = np.tile(np.asarray(base, dtype=np.float32), (env.num_envs, 1))
        self.gid = env.env_id0 + np.arange(env.num_envs)
        self.state, self.te, self.tr, self.info, self.cmd, self.row, self.pushed, self.nan = [], [], [], [], [], [], [], []
        self.clock = []                                             # meta word 0 before every step
        self.push_changed_qvel = False
        self.reset_state = None

    def _twin(self, meta, reset=False):
        from cosim_amd.scenario import reference_schedule
        t = np.zeros(len(meta), dtype=np.int64) if reset else meta[:, 0]
        return reference_schedule(self.table, self.mode, self.gid, t, meta[:, 11], self.base)

    def reset(self, mask):
        env, t = self.env, self.env.torch
        row, cmd, _, _ = self._twin(_meta(env), reset=True)
        if not self.device:
            env.receive_user_command(t.tensor(cmd, device=env.device))
        env.reset(mask=mask)
        t.cuda.synchronize(env.device)
        m = np.asarray(mask).astype(bool)
        if self.device and self.check:                              # the schedule restarts at 0 for the masked envs
            np.testing.assert_array_equal(env.applied_command.cpu().numpy()[m, :cmd.shape[1]].view(np.uint32), cmd[m].view(np.uint32))
            np.testing.assert_array_equal(env.scenario_rows()[m], row[m])
        self.reset_state = env.state.cpu().numpy()[m].copy()

    def steps(self, actions, k0, k1):
        env, t = self.env, self.env.torch
        for k in range(k0, k1):
            if self.check or not self.device:
                meta = _meta(env)
                row, cmd, mask, v = self._twin(meta)
                self.clock.append(meta[:, 0].copy())
                self.cmd.append(cmd); self.row.append(row); self.pushed.append(mask); self.nan.append(meta[:, 4].copy())
            if not self.device:
                env.receive_user_command(t.tensor(cmd, device=env.device))
                if mask.any():
                    before = None if self.push_changed_qvel else _qvel(env)
                    env.event("push", t.tensor(v, device=env.device), t.tensor(mask, device=env.device))
                    if before is not None:
                        after = _qvel(env)
                        assert (after[~mask] == before[~mask]).all()
                        self.push_changed_qvel = bool((after[mask, :3] != before[mask, :3]).any())
            env.step(t.tensor(actions[k], device=env.device))
            env.join()
            t.cuda.synchronize(env.device)
            self.record()
            if self.device and self.check:
                np.testing.assert_array_equal(env.applied_command.cpu().numpy()[:, :cmd.shape[1]].view(np.uint32), cmd.view(np.uint32),
                                              err_msg=f"applied_command, step {k}")
                np.testing.assert_array_equal(env.scenario_rows(), row, err_msg=f"scenario_rows, step {k}")

    def record(self):
        env = self.env
        self.state.append(env.state.cpu().numpy().copy()); self.info.append(env.info_buf.cpu().numpy().copy())
        self.te.append(env.terminated.cpu().numpy().copy()); self.tr.append(env.truncated.cpu().numpy().copy())

    def final(self):
        """The complete records after the run (state + parameter rows of every env)."""
        self.rows = self.env.snapshot().rows.cpu().numpy().copy()
        return self

    def ended(self):
        return int((np.stack(self.te) | np.stack(self.tr)).astype(bool).sum())


def _same(a, b, cols=slice(None), what=""):
    """State, flags and info of every step, and the final records: bit-identical."""
    assert len(a.state) == len(b.state) > 0
    for k in range(len(a.state)):
        for name in ("state", "info"):
            x, y = getattr(a, name)[k][cols].view(np.uint32), getattr(b, name)[k].view(np.uint32)
            assert np.array_equal(x, y), f"{what}{name} differs in step {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}"
        assert np.array_equal(a.te[k][cols], b.te[k]) and np.array_equal(a.tr[k][cols], b.tr[k]), f"{what}flags differ in step {k}"
    if getattr(a, "rows", None) is not None and getattr(b, "rows", None) is not None:
        x, y = a.rows[cols].view(np.uint32), b.rows.view(np.uint32)
        assert np.array_equal(x, y), f"{what}final records differ: envs {np.nonzero((x != y).any(axis=1))[0][:8]}"


def _light():
    return _model("flamingo_light_v1", "flat", max_duration=0.5)


def _reference(mode):
    """Test 1's device run, once per mode: flamingo_light_v1 flat, 96 envs, the five hand-written scenarios, 60 steps with a masked
    host reset before step 30, a ledger of 4 slots alongside (it changes no step output).  Shared, never modified."""
    key = ("reference", mode)
    if key not in _CACHE:
        cfg, cm = _light()
        env = _env(cfg, cm, N, scenarios=table5(), scenario_mode=mode, ledger=4)
        assert env.engine.query("scenario_rows") == 5 and env.engine.query("scenario_mode") == (1 if mode == "cycle" else 0)
        actions = _actions(N, K, env.action_dim)
        env.reset()
        run = _Run(env, table5(), mode)
        run.first_state = env.state.cpu().numpy().copy()
        run.steps(actions, 0, RESET_AT)
        run.reset(RESET_MASK)
        run.steps(actions, RESET_AT, K)
        run.final()
        run.ledger = env.ledger(include_open=True)
        run.open_rows = run._twin(_meta(env))[0]
        run.nan_after = _meta(env)[:, 4].copy()
        run.actions = actions
        env.close()
        run.env = None
        _CACHE[key] = run
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ 1: device = host-driven
@pytest.mark.parametrize("mode", ["env", "cycle"])
def test_device_schedule_equals_host_driven_loop(mode):
    a = _reference(mode)
    cfg, cm = _light()
    env = _env(cfg, cm, N)
    assert env.engine.query("scenario_rows") == 0 and env.applied_command is env.user_command
    env.receive_user_command(a.cmd[0])                              # the reset's state vector carries the scenario's first command
    env.reset()
    b = _Run(env, table5(), mode, device=False)
    np.testing.assert_array_equal(a.first_state.view(np.uint32), env.state.cpu().numpy().view(np.uint32))
    b.steps(a.actions, 0, RESET_AT)
    b.reset(RESET_MASK)
    b.steps(a.actions, RESET_AT, K)
    b.final()
    env.close()
    _same(a, b)
    np.testing.assert_array_equal(a.reset_state.view(np.uint32), b.reset_state.view(np.uint32))
    # what the test is about happened: auto-resets, pushes that changed qvel, keyframes (t = 3 after a pass-through, t = 24; never t = 25)
    done = (np.stack(a.te) | np.stack(a.tr)).astype(bool)
    assert a.ended() >= N and done[24].all() and set(np.stack(a.tr)[done].tolist()) == {1}
    cmd, row, pushed = np.stack(a.cmd), np.stack(a.row), np.stack(a.pushed)
    # the clock the schedule is keyed by counts control steps of the episode: k mod 25 where the host did not reset, k - 30 mod 25 after
    for k in range(K):
        assert (a.clock[k][~RESET_MASK] == k % 25).all() and (a.clock[k][RESET_MASK] == (k % 25 if k < RESET_AT else (k - RESET_AT) % 25)).all()
    assert b.push_changed_qvel and pushed.sum() >= 2 * (N // 5) * 3 and pushed[RESET_AT:].any()
    assert (cmd[0][row[0] == 1] == BASE).all() and (cmd[3][row[3] == 1, 0] == 1.0).all()
    assert (cmd[24][row[24] == 2, 0] == np.float32(0.8)).all() and (row[24] == 2).any() and not (cmd == np.float32(NEVER[0])).any()
    for r, c in zip(a.row, a.cmd):                                  # the twin the host fed B with is the one A was checked against
        assert r.dtype == np.int32 and c.dtype == np.float32
    assert all(np.array_equal(x, y) for x, y in zip(a.row, b.row)) and all(np.array_equal(x, y) for x, y in zip(a.cmd, b.cmd))
    gid = np.arange(N)
    if mode == "env":
        assert all((r == gid % 5).all() for r in a.row)
    else:   # one scenario per episode.  The host reset before step 30 does not count as an ended episode: the reset envs begin their
        # second scenario again and leave it in step 54, the others in step 49
        assert (a.row[0] == gid % 5).all() and (a.row[25] == (gid + 1) % 5).all() and (a.row[K - 1] == (gid + 2) % 5).all()
        assert (a.row[52] == (gid + 2) % 5)[~RESET_MASK].all() and (a.row[52] == (gid + 1) % 5)[RESET_MASK].all()


# ------------------------------------------------------------------------------------------------------------ 2: arrangements
def test_every_arrangement_gives_the_same_bits():
    """The cycle run of test 1 again: 4 ranges of 24 envs under a deferred join; step_range chains on four streams; one captured step
    replayed.  No host read between the steps of these runs."""
    import torch
    a = _reference("cycle")
    cfg, cm = _light()

    def drive(env, step):
        run = _Run(env, table5(), "cycle", check=False)
        env.reset()
        for k in range(K):
            if k == RESET_AT:
                env.join()
                run.reset(RESET_MASK)
            step(k)
            env.join()
            torch.cuda.synchronize(env.device)
            run.record()
        run.final()
        env.close()
        return run

    b = _env(cfg, cm, N, scenarios=table5(), scenario_mode="cycle", ranges=4, deferred_join=True)
    assert b.engine.query("ranges") == 4 and [c for _, c in b.range_list] == [24] * 4
    tb = torch.tensor(a.actions, device=b.device)
    _same(a, drive(b, lambda k: b.step(tb[k])), what="4 ranges, deferred join: ")

    d = _env(cfg, cm, N, scenarios=table5(), scenario_mode="cycle")
    streams = [torch.cuda.Stream(device=d.device) for _ in range(4)]

    def chains(k):
        torch.cuda.synchronize(d.device)
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                d.step_range(i * 24, 24, tb[k])
    _same(a, drive(d, chains), what="step_range chains: ")

    g = _env(cfg, cm, N, scenarios=table5(), scenario_mode="cycle")
    buf = torch.empty((N, g.action_dim), device=g.device)
    graph = []

    def replay(k):
        buf.copy_(tb[k])
        if k == 0:                                                  # warm-up, eager, on a side stream; then record the step
            side = torch.cuda.Stream(device=g.device)
            torch.cuda.synchronize(g.device)
            side.wait_stream(torch.cuda.current_stream(g.device))
            with torch.cuda.stream(side):
                g.step(buf)
            torch.cuda.current_stream(g.device).wait_stream(side)
            torch.cuda.synchronize(g.device)
            graph.append(torch.cuda.CUDAGraph())
            with torch.cuda.graph(graph[0]):
                g.step(buf)                                         # recorded, not run: the scenario launch is part of the graph
        else:
            graph[0].replay()
    _same(a, drive(g, replay), what="captured step: ")


def test_rewriting_the_table_in_place_between_replays():
    """A table of the same sizes is rewritten in place: the captured graph keeps its pointers and picks the new values up."""
    import torch
    cfg, cm = _light()
    n, steps, at = 32, 24, 9
    actions = _actions(n, steps, 4, seed=12)
    e = _env(cfg, cm, n, scenarios=table5(), scenario_mode="env")
    e.reset()
    ref = _Run(e, table5(), "env")
    ref.steps(actions, 0, at)
    e.set_scenarios(table5_variant(), "env")
    ref.table = table5_variant()
    ref.steps(actions, at, steps)
    ref.final()
    e.close()
    cmd, row = np.stack(ref.cmd), np.stack(ref.row)
    assert (cmd[at + 1][row[at + 1] == 1, 0] == np.float32(0.1)).all() and np.stack(ref.pushed)[:at].sum() > 0   # t = 10 >= 6: the variant's keyframe

    g = _env(cfg, cm, n, scenarios=table5(), scenario_mode="env")
    g.reset()
    run = _Run(g, table5(), "env", check=False)
    tb = torch.tensor(actions, device=g.device)
    buf = torch.empty((n, g.action_dim), device=g.device)
    buf.copy_(tb[0])
    side = torch.cuda.Stream(device=g.device)
    torch.cuda.synchronize(g.device)
    side.wait_stream(torch.cuda.current_stream(g.device))
    with torch.cuda.stream(side):
        g.step(buf)
    torch.cuda.current_stream(g.device).wait_stream(side)
    torch.cuda.synchronize(g.device)
    run.record()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(buf)
    for k in range(1, steps):
        if k == at:
            g.set_scenarios(table5_variant(), "env")
        buf.copy_(tb[k])
        graph.replay()
        torch.cuda.synchronize(g.device)
        run.record()
    run.final()
    g.close()
    _same(ref, run, what="rewritten table under a captured step: ")


# ------------------------------------------------------------------------------------------------------------ 3: split pipeline
def test_split_pipeline():
    """humanoid_p_v0 on stairs_up_hard with a position command: the scenario launch goes ahead of the first narrowphase launch, once
    per control step.  A target change at t = 4 and a push over t = 6 .. 8."""
    from cosim_amd.scenario import ScenarioTable
    cfg, cm = _model("humanoid_p_v0", "stairs_up_hard", max_duration=0.5, position_command=True)
    base = np.array([1.0, 0.5], dtype=np.float32)
    T = ScenarioTable([{"commands": [[4, 2.0, -1.0]], "pushes": [[6, 9, 0.3, -0.2, 0.0]]}, {}, {"commands": [[0, 1.5, 0.0]]}], 2)
    n, steps = 16, 12
    actions = _actions(n, steps, cm.blob.nu, seed=13)
    ea = _env(cfg, cm, n, base=base, scenarios=T, scenario_mode="env")
    assert ea.engine.query("split") > 0 and ea.command_dim == 2
    ea.reset()
    a = _Run(ea, T, "env", base=base)
    first = ea.state.cpu().numpy().copy()
    a.steps(actions, 0, steps)
    a.final()
    ea.close()
    eb = _env(cfg, cm, n, base=base)
    eb.receive_user_command(a.cmd[0])
    eb.reset()
    np.testing.assert_array_equal(first.view(np.uint32), eb.state.cpu().numpy().view(np.uint32))
    b = _Run(eb, T, "env", base=base, device=False)
    b.steps(actions, 0, steps)
    b.final()
    eb.close()
    _same(a, b)
    cmd, row, pushed = np.stack(a.cmd), np.stack(a.row), np.stack(a.pushed)
    done = (np.stack(a.te) | np.stack(a.tr)).astype(bool)
    first = (row[0] == 0) & ~done[:9].any(axis=0)                   # scenario 0, still in its first episode through step 8
    assert first.any() and b.push_changed_qvel and pushed[6:9][:, first].all() and not pushed[:6][:, first].any()
    assert (cmd[3][first] == base).all() and (cmd[4][first] == np.array([2.0, -1.0], dtype=np.float32)).all()


# ------------------------------------------------------------------------------------------------------------ 4: sharding
def test_shards_with_the_same_table_give_one_fleet():
    a = _reference("cycle")
    cfg, cm = _light()
    for lo, hi in ((0, 37), (37, N)):
        env = _env(cfg, cm, hi - lo, env_id0=lo, scenarios=table5(), scenario_mode="cycle")
        env.reset()
        run = _Run(env, table5(), "cycle")
        assert run.gid[0] == lo
        run.steps(a.actions[:, lo:hi], 0, RESET_AT)
        run.reset(RESET_MASK[lo:hi])
        run.steps(a.actions[:, lo:hi], RESET_AT, K)
        env.close()
        _same(a, run, cols=slice(lo, hi), what=f"shard [{lo}, {hi}): ")
        assert all(np.array_equal(x[lo:hi], y) for x, y in zip(a.row, run.row))


# ------------------------------------------------------------------------------------------------------------ 5: snapshot
def test_restored_snapshot_continues_its_schedule(tmp_path):
    from cosim_amd.snapshot import Snapshot
    cfg, cm = _light()
    n = 40
    actions = _actions(n, 50, 4, seed=14)
    env = _env(cfg, cm, n, scenarios=table5(), scenario_mode="cycle")
    env.reset()
    run = _Run(env, table5(), "cycle", check=False)
    for k in range(30):
        env.step(env.torch.tensor(actions[k], device=env.device))
    path = str(tmp_path / "snap.npz")
    env.snapshot().save(path)
    a = _Run(env, table5(), "cycle")
    a.steps(actions, 30, 50)
    a.final()
    env.close()
    assert np.stack(a.pushed).any() and a.ended() >= n and (np.stack(a.row)[0] == (np.arange(n) + 1) % 5).all()
    fresh = _env(cfg, cm, n, scenarios=table5(), scenario_mode="cycle")   # the table is not part of the snapshot: set it again
    fresh.restore(Snapshot.load(path, device=fresh.device))
    b = _Run(fresh, table5(), "cycle")
    b.steps(actions, 30, 50)
    b.final()
    fresh.close()
    _same(a, b, what="restored: ")
    del run


# ------------------------------------------------------------------------------------------------------------ 6: ledger
def test_ledger_records_carry_the_scenario_row():
    from cosim_amd.ledger import reference_ledger, same_records
    a = _reference("cycle")
    led = a.ledger
    kw = dict(include_open=True, begins=[(RESET_AT, RESET_MASK, 0)])
    twin = reference_ledger(np.stack(a.info), np.stack(a.te), np.stack(a.tr), np.stack(a.cmd), np.stack(a.nan + [a.nan_after]), None, 4, 4, CD,
                            scenario_rows=np.stack(a.row), open_scenario_rows=a.open_rows, **kw)
    diff = same_records(led, twin)
    assert diff is None, diff
    ended = led.ended()
    assert int(ended.sum()) == a.ended() and int(led.lost.sum()) == 0   # (the host reset discarded open episodes, it ended none)
    assert (led.words[:, 13] >= 1).all() and set(led.scenario.tolist()) == {0, 1, 2, 3, 4}
    # the record's row is the row of the episode that ended: env g's first episode ran scenario g mod 5
    first = ended & (led.episode == 0)
    assert (led.scenario[first] == led.env[first] % 5).all()
    # tracking means are against the applied command: the twin fed with the caller's constant command does not give these records
    base = reference_ledger(np.stack(a.info), np.stack(a.te), np.stack(a.tr), np.tile(BASE, (N, 1)), np.stack(a.nan + [a.nan_after]), None, 4, 4,
                            CD, scenario_rows=np.stack(a.row), open_scenario_rows=a.open_rows, **kw)
    assert "mean_tracking_err" in (same_records(led, base) or "")
    by = led.by_scenario()
    assert sorted(by) == [0, 1, 2, 3, 4] and sum(v["episodes"] for v in by.values()) == int(ended.sum())
    assert sum(v["episodes"] for v in by.values()) == len(led) - int((~ended).sum()) and all(v["terminated_share"] == v["terminated"] / v["episodes"] for v in by.values())


# ------------------------------------------------------------------------------------------------------------ 7: off means off
def test_cleared_table_leaves_no_trace():
    """An env that had a table -- one empty scenario, which passes the caller's command through and never pushes -- and cleared it:
    the steps with the table and the 30 after it are those of an env that never had one."""
    cfg, cm = _light()
    n = 32
    actions = _actions(n, 35, 4, seed=15)
    y = _env(cfg, cm, n)
    y.reset()
    ref = _Run(y, None, "env", device=False, check=False)
    x = _env(cfg, cm, n)
    x.reset()
    run = _Run(x, None, "env", check=False)
    t = x.torch
    x.set_scenarios([{}])
    assert x.engine.query("scenario_rows") == 1 and x.applied_command is not x.user_command
    for k in range(35):
        if k == 5:
            x.set_scenarios(None)
            assert x.engine.query("scenario_rows") == 0 and x.engine.query("scenario_mode") == 0 and x.applied_command is x.user_command
            assert (x.scenario_rows() == -1).all()
        for env, r in ((x, run), (y, ref)):
            env.step(t.tensor(actions[k], device=env.device))
            t.cuda.synchronize(env.device)
            r.record()
        if k == 4:
            assert (x.scenario_rows() == 0).all() and (x.applied_command.cpu().numpy()[:, :CD] == BASE).all()
    run.final(); ref.final()
    x.close(); y.close()
    _same(ref, run)
    assert ref.ended() >= n


# ------------------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_leave_the_env_stepping():
    cfg, cm = _light()
    n = 16
    actions = _actions(n, 6, 4, seed=16)
    env = _env(cfg, cm, n, scenarios=table5())
    t = env.torch
    tb = t.tensor(actions, device=env.device)
    env.reset()
    env.step(tb[0])
    with pytest.raises(ValueError, match="scenario table is set"):
        env.rollout(tb[1:3])
    with pytest.raises(ValueError, match="scenario table is set"):   # the C entry point refuses by itself
        env.engine.rollout(1, tb[1:2].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(),
                           env.info_buf.data_ptr(), env._stream())
    with pytest.raises(ValueError, match="mode must be"):
        env.set_scenarios(table5(), "episode")
    with pytest.raises(ValueError, match="commands_dev is NULL"):      # a reset needs the caller's command to pass through
        env.engine.reset(None, None, env.state.data_ptr(), env._stream())
    # malformed tables: refused on the host, by the Python table and by the engine itself, with the scenario and the row named
    with pytest.raises(ValueError, match=r"scenario 1, keyframe 1: time 2 does not increase"):
        env.set_scenarios([{}, {"commands": [[2, 1, 0, 0, 0], [2, 1, 0, 0, 0]]}])
    cmd_out, row_out = t.zeros((n, CD), device=env.device), t.zeros((n,), dtype=t.int32, device=env.device)
    i32, f32 = np.int32, np.float32

    def raw(key_adr, key_t, key_cmd, push_adr, push_t, push_v, mode=0):
        env.engine.scenario_set((np.array(key_adr, i32), np.array(key_t, i32), np.array(key_cmd, f32).reshape(-1, CD), np.array(push_adr, i32),
                                 np.array(push_t, i32).reshape(-1, 2), np.array(push_v, f32).reshape(-1, 3)), mode, cmd_out.data_ptr(),
                                row_out.data_ptr(), env._stream())
    with pytest.raises(ValueError, match=r"scenario 1, keyframe 1: time 4 does not increase \(previous 7\)"):
        raw([0, 0, 2], [7, 4], np.zeros((2, CD)), [0, 0, 0], [], [])
    with pytest.raises(ValueError, match=r"scenario 0, keyframe 0: command 2 is not finite"):
        raw([0, 1], [0], [[0, 0, np.nan, 0]], [0, 0], [], [])
    with pytest.raises(ValueError, match=r"scenario 2, push window 0: t1 3 is not after t0 3"):
        raw([0, 0, 0, 0], [], [], [0, 0, 0, 1], [[3, 3]], [[1, 0, 0]])
    with pytest.raises(ValueError, match=r"scenario 0, push window 1: velocity 1 is not finite"):
        raw([0, 0], [], [], [0, 2], [[0, 1], [1, 2]], [[1, 0, 0], [0, np.inf, 0]])
    with pytest.raises(ValueError, match=r"scenario 1: 65 keyframes, at most 64"):
        raw([0, 0, 65], list(range(65)), np.zeros((65, CD)), [0, 0, 0], [], [])
    with pytest.raises(ValueError, match=r"scenario 0: 65 push windows, at most 64"):
        raw([0, 0], [], [], [0, 65], [[k, k + 1] for k in range(65)], np.zeros((65, 3)))
    with pytest.raises(ValueError, match=r"65537 scenarios"):
        raw([0] * 65538, [], [], [0] * 65538, [], [])
    with pytest.raises(ValueError, match=r"shorter than their row addresses"):
        raw([0, 3], [0], np.zeros((1, CD)), [0, 0], [], [])
    # after the refusals the table that was set still holds and the env steps
    assert env.engine.query("scenario_rows") == 5 and env.scenario_mode == "env"
    env.step(tb[1])
    t.cuda.synchronize(env.device)
    assert (env.scenario_rows() == np.arange(n) % 5).all() and np.isfinite(env.state.cpu().numpy()).all()
    assert env.solver_stats()["step_count"] == n * 3                # the reset and two steps: the refused calls stepped nothing
    env.close()
    # mode cycle needs auto_reset: without it the episode count advances on every flagged step
    manual = _env(cfg, cm, n, auto_reset=False)
    with pytest.raises(ValueError, match="cycle needs auto_reset"):
        manual.set_scenarios(table5(), "cycle")
    assert manual.engine.query("scenario_rows") == 0 and manual.scenario_table is None
    manual.set_scenarios(table5(), "env")                          # mode env is fine without it
    manual.reset()
    manual.step(tb[0])
    t.cuda.synchronize(manual.device)
    assert (manual.scenario_rows() == np.arange(n) % 5).all()
    manual.close()


# ------------------------------------------------------------------------------------------------------------ 9: CLI
@pytest.mark.parametrize("path", ["--graph", "--pipelined"])
def test_cli_scenarios_on_the_fast_paths(tmp_path, capsys, path):
    """The two closed-loop paths that refuse host schedules run a scenario file, and the report breaks the episodes down by scenario."""
    import yaml
    from cosim_amd import cli
    scn, report = tmp_path / "scn.yaml", tmp_path / "r.json"
    scn.write_text(yaml.safe_dump({"scenarios": TABLE5}))
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", "--scenarios", str(scn), "--scenario-mode", "cycle", path, "--ledger", "4", "--report", str(report)]) == 0
    r = json.loads(report.read_text())
    by = r["episodes"]["by_scenario"]
    assert sorted(by) == ["0", "1", "2", "3", "4"] and sum(v["episodes"] for v in by.values()) == r["episodes"]["episodes"] >= 32
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["by_scenario"] == {k: {"episodes": v["episodes"], "terminated": v["terminated"]} for k, v in by.items()}
    assert line["control_steps"] == 60
