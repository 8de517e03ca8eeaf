"""Failure traces on the device (cosim_ftrace_set / cosim_ftrace_get, csrc/cosim_ftrace.hip, and their BatchedEnv / CLI surface)
against the numpy twin (cosim_amd/ftrace.py reference_traces) fed with what a host-driven loop reads after every step.

Every comparison is bit for bit (floats as their words): the feature only copies.  The common fleet is 70 flamingo_light_v1 on the
plane with a 25-step time limit, a tilt rule, a scenario table whose pushes knock some robots over, a ledger of 8 slots and traces
(8, 2), run for 80 control steps under auto-reset from a fixed action table.  The twin of that run must show a fall, a time limit,
a trace shorter than the window, one that wrapped, an env that lost a trace and an env without one -- asserted, so that no
comparison is empty."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, FRAMES, KEEP = 70, 80, 8, 2
TILT = 0.5
# row = env id mod 7.  0: never pushed (time limits only); 1, 4, 5: thrown over right after the reset (short episodes, many per
# env); 2: a side push early; 3, 6: a push in mid-episode (the window wraps before the fall)
SCN = [{}, {"pushes": [[0, 6, 6.0, 0.0, 0.0]]}, {"pushes": [[2, 7, 0.0, 5.0, 0.0]]}, {"pushes": [[10, 15, 3.0, 0.0, 0.0]]},
       {"pushes": [[0, 5, -6.0, 0.0, 0.0]]}, {"pushes": [[0, 4, 0.0, 6.0, 0.0]]}, {"pushes": [[15, 20, -3.0, 0.0, 0.0]]}]
CMD = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
_CACHE = {}


def _model(robot="flamingo_light_v1", terrain="flat", **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, max_duration=0.5, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _env(n=N, traces=(FRAMES, KEEP), on=None, model=None, **kw):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.fall import FallRule
    cfg, cm = model or _model()
    kw.setdefault("fall", FallRule(tilt=TILT))
    kw.setdefault("scenarios", SCN)
    kw.setdefault("ledger", 8)
    if traces is not None:
        kw["failure_traces"] = {"frames": traces[0], "keep": traces[1], **({"on": on} if on is not None else {})}
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=3, auto_reset=True, **kw)
    env.receive_user_command(CMD[:env.command_dim] if env.command_dim != 2 else np.array([1.0, 0.5], dtype=np.float32))
    return env


def _table(env, steps=STEPS, seed=11):
    import torch
    a = np.random.default_rng(seed).uniform(-0.6, 0.6, size=(steps, env.num_envs, env.action_dim)).astype(np.float32)
    return torch.tensor(a, device=env.device)


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().copy()


class _Rec:
    """A host-driven loop: before step k the state record (qpos, qvel, meta words 4 / 14) is read, after it the step's outputs, the
    applied command, the scenario rows and meta word 15.  ``twin`` feeds it all to reference_traces."""

    def __init__(self, env):
        self.env = env
        self.cols = {k: [] for k in ("qpos", "qvel", "m4", "m14", "act", "cmd", "info", "te", "tr", "m15", "rows", "state")}

    def _before(self):
        env, c = self.env, self.cols
        d = env.get_data()
        m = _meta(env)
        c["qpos"].append(d.qpos.cpu().numpy().copy()); c["qvel"].append(d.qvel.cpu().numpy().copy())
        c["m4"].append(m[:, 4].copy()); c["m14"].append(m[:, 14].copy())

    def run(self, table, k0, k1):
        env, c = self.env, self.cols
        for k in range(k0, k1):
            self._before()
            env.step(table[k])
            env.join()
            env.torch.cuda.synchronize(env.device)
            c["act"].append(table[k].cpu().numpy().copy()); c["info"].append(env.info_buf.cpu().numpy().copy())
            c["cmd"].append(env.applied_command.cpu().numpy()[:, :env.command_dim].copy())
            c["te"].append(env.terminated.cpu().numpy().copy()); c["tr"].append(env.truncated.cpu().numpy().copy())
            c["state"].append(env.state.cpu().numpy().copy())
            c["m15"].append(_meta(env)[:, 15].copy()); c["rows"].append(env.scenario_rows().astype(np.int32))

    def twin(self, frames, keep, on=None, **kw):
        from cosim_amd.ftrace import reference_traces
        env, c = self.env, {k: list(v) for k, v in self.cols.items()}
        d, m = env.get_data(), _meta(env)
        qpos, qvel = c["qpos"] + [d.qpos.cpu().numpy().copy()], c["qvel"] + [d.qvel.cpu().numpy().copy()]
        has_scn, has_fall = env.scenario_table is not None, env.fall_rule is not None
        open_rows = None
        if has_scn:
            S = len(env.scenario_table)
            open_rows = (env.env_id0 + np.arange(env.num_envs)) % S if env.scenario_mode == "env" else None
        return reference_traces(np.stack(qpos), np.stack(qvel), np.stack(c["act"]), np.stack(c["cmd"]), np.stack(c["info"]), np.stack(c["te"]),
                                np.stack(c["tr"]), np.stack(c["m4"] + [m[:, 4]]), None, np.stack(c["m15"]) if has_fall else None, frames, keep,
                                on, env_id0=env.env_id0, scenario_rows=np.stack(c["rows"]) if has_scn else None,
                                open_scenario_rows=open_rows, **kw)


def _assert_same(a, b, raw=True):
    """Kept traces, counters and open headers; ``raw``: also every word of every buffer (a run without host cuts)."""
    from cosim_amd.ftrace import same_traces
    diff = same_traces(a, b)
    assert diff is None, diff
    np.testing.assert_array_equal(a.counts, b.counts)
    assert (a.open_headers is None) == (b.open_headers is None)
    if a.open_headers is not None:
        np.testing.assert_array_equal(a.open_headers, b.open_headers)
    if raw:
        np.testing.assert_array_equal(a.buffers, b.buffers)


@pytest.fixture(scope="module")
def base():
    """The common run with the default selection, host-driven: (recorder, device traces with open windows, ledger with open rows)."""
    env = _env()
    assert env.engine.query("ftrace_frames") == FRAMES and env.engine.query("ftrace_keep") == KEEP and env.engine.query("ftrace_mask") == 1 | 4
    assert env.engine.query("ftrace_frame_words") == (4 + env.nq + env.nv + env.action_dim + env.command_dim + env.info_dim + 3) // 4 * 4
    table = _table(env)
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, STEPS)
    got, led = env.failure_traces(include_open=True), env.ledger(include_open=True)
    out = {"rec": rec, "got": got, "ledger": led, "table": table, "final": env.state.cpu().numpy().copy(),
           "by_scenario": led.by_scenario()}
    yield out
    env.close()


def _coverage(tw, te, tr):
    """What the fixture's run must contain, on the twin's result."""
    assert te.any() and tr.any(), "no fall or no time limit in the run"
    ended = tw.ended()
    assert (tw.frames[ended] < FRAMES).any(), "no trace shorter than the window"
    assert ((tw.length[ended] > FRAMES) & (tw.oldest[ended] != 0)).any(), "no trace whose ring wrapped"
    assert (tw.lost > 0).any(), "no env lost a trace"
    assert (tw.counts[:, 1] == 0).any(), "every env has a trace"


# ------------------------------------------------------------------------------------------------------------ 6: against the twin
def test_default_selection_equals_the_twin(base):
    rec, got = base["rec"], base["got"]
    tw = rec.twin(FRAMES, KEEP, include_open=True)
    te, tr = np.stack(rec.cols["te"]).astype(bool), np.stack(rec.cols["tr"]).astype(bool)
    _coverage(tw, te, tr)
    _assert_same(got, tw)
    ended = got.ended()
    assert ((got.flags[ended] & (1 | 32)) == (1 | 32)).all()               # every kept trace is a fall by tilt (a few in the time limit's step)
    assert int(ended.sum()) + int(got.lost.sum()) == int(te.sum())
    # the last frame of a trace is the step that ended the episode: its flags, its info row, the action it was given
    for r in np.nonzero(ended)[0][:40]:
        n, k, f = got.env[r], got.steps_seen[r] - 1, got.frames[r] - 1
        assert got.terminated[r, f] == 1 and got.t[r, f] == got.length[r]
        np.testing.assert_array_equal(got.info[r, f].view(np.int32), rec.cols["info"][k][n].view(np.int32))
        np.testing.assert_array_equal(got.action[r, f].view(np.int32), rec.cols["act"][k][n].view(np.int32))
        np.testing.assert_array_equal(got.qpos[r, f].view(np.int32), rec.cols["qpos"][k][n].view(np.int32))
    without = base["got"].select(env=0)
    assert len(without) == 1 and (without.flags == 16).all(), "env 0 is never pushed: only its open window"


@pytest.mark.parametrize("on", [("truncated",), ("tilt",)], ids=["truncated", "tilt"])
def test_other_selections_equal_the_twin(base, on):
    env = _env(on=on)
    env.reset()
    rec = _Rec(env)
    rec.run(base["table"], 0, STEPS)
    got = env.failure_traces(include_open=True)
    tw = rec.twin(FRAMES, KEEP, on, include_open=True)
    _assert_same(got, tw)
    ended = got.ended()
    assert ended.any() and (got.lost > 0).any() and ((got.flags[ended] & (2 if on == ("truncated",) else 32)) != 0).all()
    np.testing.assert_array_equal(env.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))   # the same run
    if on == ("tilt",):                                                    # here: the default selection's traces, under another mask
        np.testing.assert_array_equal(got.headers, base["got"].headers)
        np.testing.assert_array_equal(got.words, base["got"].words)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 7: launch paths
def _free_run(env, table, steps=STEPS):
    env.reset()
    for k in range(steps):
        env.step(table[k])
    env.join()
    env.torch.cuda.synchronize(env.device)


def test_every_launch_path_gives_the_same_buffers(base):
    """One launch per step (the fixture); two uneven ranges (33 + 37) on two streams; four ranges under a deferred join; step_range
    chains on the range streams; a captured graph replayed.  And a fleet without traces: the same state outputs."""
    import torch
    ref, table = base["got"], base["table"]

    def check(env):
        _assert_same(env.failure_traces(include_open=True), ref)
        np.testing.assert_array_equal(env.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))
        env.close()

    a = _env()
    a.reset()
    shards, streams = [(0, 33), (33, 37)], [torch.cuda.Stream(device=a.device) for _ in range(2)]
    torch.cuda.synchronize(a.device)
    for k in range(STEPS):
        for (first, count), st in zip(shards[::-1] if k % 2 else shards, streams[::-1] if k % 2 else streams):   # either order
            with torch.cuda.stream(st):
                a.step_range(first, count, table[k])
    torch.cuda.synchronize(a.device)
    check(a)

    b = _env(ranges=4, deferred_join=True)
    assert b.engine.query("ranges") == 4
    _free_run(b, table)
    check(b)

    c = _env(ranges=4, deferred_join=True)
    c.reset()
    torch.cuda.synchronize(c.device)
    for k in range(STEPS):
        for (first, count), st in zip(c.range_list, c.range_streams):
            with torch.cuda.stream(st):
                c.step_range(first, count, table[k])
            c.range_mark(c.range_list.index((first, count)))
    c.join()
    torch.cuda.synchronize(c.device)
    check(c)

    g = _env()
    g.reset()
    buf = torch.empty((N, g.action_dim), device=g.device)
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
        g.step(buf)                                                        # recorded, not run: the trace launch is part of the graph
    for k in range(1, STEPS):
        buf.copy_(table[k])
        graph.replay()
    torch.cuda.synchronize(g.device)
    check(g)

    off = _env(traces=None)
    assert off.engine.query("ftrace_frames") == 0
    off.reset()
    rec = base["rec"]
    for k in range(STEPS):
        off.step(table[k])
        for name, x in (("state", off.state), ("te", off.terminated), ("tr", off.truncated)):
            np.testing.assert_array_equal(x.cpu().numpy().view(np.uint8), rec.cols[name][k].view(np.uint8), err_msg=f"{name}, step {k}")
    off.close()


# ------------------------------------------------------------------------------------------------------------ 8: split pipeline
@pytest.mark.parametrize("fixup", [False, True], ids=["split", "split_fixup"])
def test_split_pipeline(fixup):
    """humanoid_p_v0 on stairs_up_hard, 8 envs, traces (4, 1) on "height": a height rule far above the robot fires as soon as its
    grace of 3 steps is over, so every env ends a 4-step episode three times in 12 steps.  The frame is wider than one wave."""
    from cosim_amd.fall import FallRule
    model = _model("humanoid_p_v0", "stairs_up_hard", position_command=True)
    env = _env(8, (4, 1), ("height",), model, fall=FallRule(height=5.0, grace=3), scenarios=None, ledger=4,
               **({"hfield_fixup": True} if fixup else {}))
    assert env.engine.query("split") > 0 and env.engine.query("ftrace_frame_words") > 64
    table = _table(env, 12)
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, 12)
    te = np.stack(rec.cols["te"]).astype(bool)
    assert te[3].all() and te[7].all() and te[11].all() and int(te.sum()) == 24, "the height rule did not fire in steps 4, 8 and 12"
    got = env.failure_traces(include_open=True)
    _assert_same(got, rec.twin(4, 1, ("height",), include_open=True))
    ended = got.ended()
    assert int(ended.sum()) == 8 and (got.lost == 2).all() and (got.flags[ended] == (1 | 64)).all() and (got.episode[ended] == 2).all()
    assert (got.frames[ended] == 4).all() and got.t[ended].tolist() == [[1, 2, 3, 4]] * 8
    env.close()


# ------------------------------------------------------------------------------------------------------------ 9: host cuts
def test_host_cuts_restart_the_window(base):
    """A masked reset before step 12, a masked restore before step 30 and a set_state of the whole fleet before step 47."""
    env = _env(traces=(FRAMES, 8), ledger=16)                              # (room for every trace and record of the 80 steps)
    table = base["table"]
    lo, hi = np.arange(N) < 30, np.arange(N) >= 45
    env.reset()
    rec = _Rec(env)
    rec.run(table, 0, 8)
    snap = env.snapshot()
    rec.run(table, 8, 12)
    before = env.failure_traces(include_open=True)
    env.reset(mask=lo)
    after = env.failure_traces(include_open=True)
    o = (after.flags & 16) != 0
    assert (after.length[o][lo] == 0).all() and (after.flags[o][lo] == 16).all() and (after.frames[o][lo] == 0).all()
    keep = ~(o & np.isin(after.env, np.nonzero(lo)[0]))
    np.testing.assert_array_equal(after.headers[keep], before.headers[keep])      # frozen traces and the other envs' windows: untouched
    np.testing.assert_array_equal(after.words[keep], before.words[keep])
    np.testing.assert_array_equal(after.counts, before.counts)
    rec.run(table, 12, 30)
    before = env.failure_traces(include_open=True)
    env.restore(snap, mask=hi)
    after = env.failure_traces(include_open=True)
    o = (after.flags & 16) != 0
    assert (after.flags[o][hi] == (16 | 8)).all() and (after.length[o][hi] == 0).all()
    keep = ~(o & np.isin(after.env, np.nonzero(hi)[0]))
    np.testing.assert_array_equal(after.headers[keep], before.headers[keep])
    np.testing.assert_array_equal(after.words[keep], before.words[keep])
    rec.run(table, 30, 47)
    d = env.get_data()
    env.torch.cuda.synchronize(env.device)
    env.set_state(d.qpos.clone(), d.qvel.clone())
    opn = env.failure_traces(include_open=True)
    o = (opn.flags & 16) != 0
    assert (opn.flags[o] == (16 | 8)).all() and (opn.length[o] == 0).all()
    rec.run(table, 47, STEPS)
    got, led = env.failure_traces(include_open=True), env.ledger(include_open=True)
    tw = rec.twin(FRAMES, 8, include_open=True, begins=[(12, lo, 0), (30, hi, 8), (47, None, 8)])
    _assert_same(got, tw, raw=False)
    assert got.ended().any() and ((got.flags[got.ended()] & 8) != 0).any(), "no trace of an episode that began at a cut"
    # nothing is kept for a cut episode, and flag 8 is where the ledger puts it
    at = got.join(led)
    assert (at >= 0).all()
    np.testing.assert_array_equal(led.flags[at], got.flags)
    np.testing.assert_array_equal(led.length[at], got.length)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 10: join
def test_join_with_the_ledger(base):
    got, led = base["got"], base["ledger"]
    at = got.join(led)
    assert (at >= 0).all() and len(set(at.tolist())) == len(got)
    np.testing.assert_array_equal(led.flags[at], got.flags)
    np.testing.assert_array_equal(led.length[at], got.length)
    np.testing.assert_array_equal(led.steps_seen[at], got.steps_seen)
    np.testing.assert_array_equal(led.scenario[at], got.scenario)
    np.testing.assert_array_equal(got.scenario, got.env % len(SCN))
    ended = got.ended()
    by = base["by_scenario"]
    for row in np.unique(got.scenario[ended]):
        assert by[int(row)]["fell"] >= int((got.scenario[ended] == row).sum()) > 0
    assert by[0]["fell"] == 0 and not (got.scenario[ended] == 0).any()
    s = got.summary()
    assert s["traces"] == int(ended.sum()) == s["terminated"] == s["tilt"] and s["truncated"] == int(((got.flags[ended] & 2) != 0).sum()) and s["open"] == N
    assert s["lost"] == int(got.lost.sum()) > 0


# ------------------------------------------------------------------------------------------------------------ 11: off means off
def test_off_means_off(base):
    table = base["table"]
    a, b = _env(), _env(traces=None)
    a.reset(); b.reset()
    for k in range(30):
        a.step(table[k]); b.step(table[k])
    assert len(a.failure_traces()) > 0
    a.set_failure_traces(None)
    assert a.engine.query("ftrace_frames") == 0 and a.engine.query("ftrace_keep") == 0 and a.engine.query("ftrace_mask") == 0
    with pytest.raises(ValueError, match="no failure traces are set"):
        a.failure_traces()
    with pytest.raises(ValueError, match="no failure traces are set"):
        a.engine.ftrace_get(a.state.data_ptr(), a.state.data_ptr(), None, a._stream())
    for k in range(30, 50):
        a.step(table[k]); b.step(table[k])
        for x, y in ((a.state, b.state), (a.terminated, b.terminated), (a.truncated, b.truncated), (a.info_buf, b.info_buf)):
            np.testing.assert_array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------ 12: refusals
def test_refusals():
    env = _env(16, ledger=None, scenarios=None)
    table = _table(env, 6)
    env.reset()
    with pytest.raises(ValueError, match="failure traces are set"):
        env.rollout(table[0:2])
    with pytest.raises(ValueError, match=r"cosim_rollout: failure traces are set"):
        env.engine.rollout(2, table[0:2].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(),
                           env.info_buf.data_ptr(), env._stream())
    with pytest.raises(ValueError, match=r"failure traces are set \(cosim_ftrace_set\) and info_out_dev is NULL"):
        env.engine.step(table[0].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(), None,
                        env._stream())
    env.step(table[0])
    assert env.failure_traces(include_open=True).length.tolist() == [1] * 16      # the refused calls stepped nothing
    for args, message in (((1025, 2, 1), "frames 1025 outside"), ((-1, 2, 1), "frames -1 outside"), ((8, 0, 1), "keep 0 outside"),
                          ((8, 65, 1), "keep 65 outside"), ((8, 2, 0), "on_mask 0 must be"), ((8, 2, 8), "on_mask 8 must be"),
                          ((8, 2, 256), "on_mask 256 must be")):
        with pytest.raises(ValueError, match=message):
            env.engine.ftrace_set(*args)
    assert env.engine.query("ftrace_frames") == FRAMES                      # a refused set leaves the traces as they were
    with pytest.raises(ValueError, match="null argument"):
        env.engine.ftrace_get(None, None, None, env._stream())
    with pytest.raises(ValueError, match="keep 65"):
        env.set_failure_traces((8, 65))
    env.set_failure_traces((4, 1), on=("truncated",))                       # on a stepped fleet: the open windows carry flag 8
    opn = env.failure_traces(include_open=True)
    assert (opn.flags == (16 | 8)).all() and env.engine.query("ftrace_mask") == 2 and opn.meta["window"] == 4
    env.set_failure_traces(None)
    env.rollout(table[2:4])                                                 # off: rollouts work again
    with pytest.raises(ValueError, match="no failure traces are set"):
        env.engine.ftrace_get(env.state.data_ptr(), env.state.data_ptr(), None, env._stream())
    env.close()


# ------------------------------------------------------------------------------------------------------------ 13: CLI
@pytest.mark.parametrize("mode", ["--graph", "--pipelined"])
def test_cli_writes_traces(tmp_path, capsys, mode):
    from cosim_amd import cli
    from cosim_amd.ftrace import FailureTraces
    out = tmp_path / "traces.npz"
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", mode, "--ledger", "4", "--failure-traces", "8", "2", "--failure-traces-on", "truncated", "tilt",
                     "--fall-tilt", "0.8", "--failure-traces-out", str(out)]) == 0
    tr = FailureTraces.load(str(out))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["failure_traces"] == tr.summary() and tr.meta["window"] == 8 and tr.meta["keep"] == 2 and tr.meta["on_mask"] == 2 | 32
    assert len(tr) == 2 * 32 and line["failure_traces"]["truncated"] + line["failure_traces"]["tilt"] >= 64     # two time limits per env at least
    assert line["episodes"]["episodes"] + line["episodes"]["lost"] == len(tr) + line["failure_traces"]["lost"]   # every end is selected
