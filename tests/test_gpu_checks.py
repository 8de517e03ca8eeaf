"""Scenario checks on the device (cosim_scenario_checks_set / cosim_scenario_checks_get, csrc/cosim_checks.hip, and their BatchedEnv /
CLI surface) against the numpy twin (cosim_amd/checks.py reference_checks) fed with what a host-driven loop reads around every step.

Every comparison is exact (floats as their words).  The common fleet is 24 flamingo_light_v1 on the plane with a 25-step time limit and
a tilt rule, run for 60 control steps under auto-reset from a fixed action table, under four scenarios: row 0 holds 64 items over
every signal, mode and comparison, row 1 a single item, row 2 none, row 3 a push that throws the robot over and five items.  The
bounds are the medians of each item's signal over its window in a dry run of the same seed (the engine is a bit-exact function of the
seed), so passes, fails, incompletes and a non-zero settle time all occur -- asserted, so that no comparison is empty."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, SLOTS = 24, 60, 2
CMD = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
WINDOWS = [(0, 10), (5, 20), (10, 25), (20, 30), (0, 25), (3, 4), (12, 18), (24, 25)]
SIGNALS = ["info", "abs_info", "tracking_error", "torque_max", "up", "qpos", "qvel", "abs_qvel"]
_CACHE = {}


def _model(robot="flamingo_light_v1"):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    if robot not in _CACHE:
        cfg = make_config(robot, terrain="flat", max_duration=0.5)
        _CACHE[robot] = (cfg, compile_model(cfg))
    return _CACHE[robot]


def _items(n, rng, dims):
    """n items cycling through the signals, modes and comparisons; the bound is filled in from the dry run."""
    info_dim, cd, nq, nv = dims
    out = []
    for k in range(n):
        sig = SIGNALS[k % 8]
        width = {"info": info_dim, "abs_info": info_dim, "tracking_error": min(cd, 3), "torque_max": 1, "up": 1, "qpos": nq, "qvel": nv, "abs_qvel": nv}[sig]
        t0, t1 = WINDOWS[(k // 8 + k) % len(WINDOWS)]
        out.append([t0, t1, sig, int(rng.integers(width)), ["always", "settle", "mean"][(k // 2) % 3], "<>"[(k // 3) % 2], 0.0, f"i{k}"])
    return out


def _scenarios(dims, bounds=None, seed=5):
    rng = np.random.default_rng(seed)
    scn = [{"commands": [[0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0][:1 + dims[1]]], "checks": _items(64, rng, dims)},
           {"checks": [[0, 25, "tracking_error", 0, "settle", "<", 0.0, "tracks"]]},
           {"commands": [[0, 0.2, 0.0, 0.0, 0.0, 0.0, 0.0][:1 + dims[1]]]},
           {"pushes": [[5, 10, 6.0, 0.0, 0.0]], "checks": _items(5, rng, dims)[:4] + [[0, 25, "up", 0, "always", ">", 0.0, "upright"]]}]
    if bounds is not None:
        for sc, b in zip(scn, bounds):
            for it, x in zip(sc.get("checks", []), b):
                it[6] = float(x)
    return scn


def _env(model=None, n=N, scenarios=None, mode="env", **kw):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.fall import FallRule
    cfg, cm = model or _model()
    kw.setdefault("fall", FallRule(tilt=0.5))
    kw.setdefault("ledger", 8)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=3, auto_reset=True, scenarios=scenarios, scenario_mode=mode, **kw)
    env.receive_user_command(CMD[:env.command_dim])
    return env


def _dims(env):
    return env.info_dim, env.command_dim, env.nq, env.nv


def _actions(env, steps=STEPS, seed=11):
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
    """A host-driven loop: before step k meta word 0 is read, after it the step's outputs, the applied command, the scenario rows and
    the state record.  ``twin`` feeds it all to reference_checks."""

    def __init__(self, env):
        self.env = env
        self.cols = {k: [] for k in ("clock", "info", "te", "tr", "cmd", "rows", "qpos", "qvel", "state")}
        self.begins = []

    def run(self, table, k0, k1):
        env, c = self.env, self.cols
        for k in range(k0, k1):
            c["clock"].append(_meta(env)[:, 0].copy())
            env.step(table[k])
            env.join()
            env.torch.cuda.synchronize(env.device)
            d = env.get_data()
            c["qpos"].append(d.qpos.cpu().numpy().copy()); c["qvel"].append(d.qvel.cpu().numpy().copy())
            c["info"].append(env.info_buf.cpu().numpy().copy()); c["state"].append(env.state.cpu().numpy().copy())
            c["cmd"].append(env.applied_command.cpu().numpy()[:, :max(env.command_dim, 1)].copy())
            c["te"].append(env.terminated.cpu().numpy().copy()); c["tr"].append(env.truncated.cpu().numpy().copy())
            c["rows"].append(env.scenario_rows().astype(np.int32))

    def stacked(self, name):
        return np.stack(self.cols[name])

    def twin(self, table, slots=SLOTS, k0=0, k1=None, include_open=True, **kw):
        """The twin over the recorded steps [k0, k1); the open rows are the live ones, so they go with the last segment only."""
        from cosim_amd.checks import reference_checks
        from cosim_amd.scenario import scenario_rows
        env, m = self.env, _meta(self.env)
        K = len(self.cols["info"])
        k1 = K if k1 is None else k1
        assert k1 == K or not include_open
        gid = env.env_id0 + np.arange(env.num_envs)
        col = lambda name: np.stack(self.cols[name][k0:k1])   # noqa: E731
        clock = np.stack(self.cols["clock"][k0:k1] + [m[:, 0] if k1 == K else self.cols["clock"][k1]])
        return reference_checks(table, col("info"), col("te"), col("tr"), col("cmd"), col("qpos"), col("qvel"), clock, col("rows"), slots,
                                env.action_dim, include_open=include_open, begins=[(k - k0, mk, f) for k, mk, f in self.begins if k0 < k <= k1],
                                env_id0=env.env_id0, open_scenario_rows=scenario_rows(len(table), env.scenario_mode, gid, m[:, 11]), **kw)


def _bounds(rec, scn, dims, nu):
    """Per item the median of its signal over its window in the recorded run, over the envs and steps that ran the item's row."""
    from cosim_amd.checks import _signal
    from cosim_amd.scenario import CHECK_SIGNALS, ScenarioTable
    T = ScenarioTable(scn, dims[1]).resolve_checks(None)
    info, cmd, qpos, qvel, clock, rows = (rec.stacked(k) for k in ("info", "cmd", "qpos", "qvel", "clock", "rows"))
    done = (rec.stacked("te") | rec.stacked("tr")) != 0
    out = []
    for s, items in enumerate(T.checks):
        b = []
        for t0, t1, sig, idx, *_ in items:
            sel = np.argwhere((rows == s) & (clock >= t0) & (clock < t1) & ~(done & (sig >= CHECK_SIGNALS["up"])))
            v = [_signal(sig, idx, info[k, i], cmd[k, i], qpos[k, i], qvel[k, i], nu) for k, i in sel]
            b.append(np.float32(np.median(np.asarray(v, dtype=np.float32))) if v else np.float32(0.0))
        out.append(b)
    return out


def _same(a, b):
    from cosim_amd.checks import same_verdicts
    diff = same_verdicts(a, b)
    assert diff is None, diff


def _coverage(v):
    """What the run must contain, on the twin's result."""
    from cosim_amd.checks import SETTLE
    e = v.ended()
    assert e.any() and (v.flags[e] & 1).any() and (v.flags[e] & 2).any(), "no fall or no time limit in the run"
    assert v.passed[e].any() and (v.failed[e] & v.valid[e]).any() and (v.incomplete[e] & v.valid[e]).any()
    assert ((v.mode[e] == SETTLE) & (v.settle_time[e] > 0) & v.passed[e]).any(), "no settle item with a non-zero settle time passed"
    assert (v.lost > 0).any(), "no env lost a record"
    assert {int(s) for s in v.scenario[e]} >= {0, 1, 3} and (v.valid[e].sum(axis=1) == 64).any() and (v.valid[e].sum(axis=1) == 1).any()


@pytest.fixture(scope="module")
def base():
    """The dry run (a table without checks), the bounds it gives, and the common run with the checks armed, host-driven."""
    dry = _env()
    dims = _dims(dry)
    scn0 = _scenarios(dims)
    dry.set_scenarios([{k: v for k, v in sc.items() if k != "checks"} for sc in scn0])
    acts = _actions(dry)
    dry.reset()
    rd = _Rec(dry)
    rd.run(acts, 0, STEPS)
    scn = _scenarios(dims, _bounds(rd, scn0, dims, dry.action_dim))
    env = _env(scenarios=scn, check_slots=SLOTS)
    assert env.engine.query("scenario_check_items") == 64 and env.engine.query("scenario_check_slots") == SLOTS
    assert env.engine.query("scenario_check_words") == 8 + 2 * 64
    env.reset()
    rec = _Rec(env)
    rec.run(acts, 0, STEPS)
    out = {"dry": rd, "dry_ledger": dry.ledger(include_open=True), "rec": rec, "got": env.verdicts(include_open=True), "scn": scn, "acts": acts,
           "ledger": env.ledger(include_open=True), "table": env.scenario_table, "final": env.state.cpu().numpy().copy(), "dims": dims}
    dry.close()
    yield out
    env.close()


# ------------------------------------------------------------------------------------------------------------ 1: against the twin
def test_device_records_equal_the_twin(base):
    tw = base["rec"].twin(base["table"])
    _coverage(tw)
    _same(base["got"], tw)
    # a verdict row joins the ledger's by (env, episode): the same length, flags and scenario
    v, led = base["got"], base["ledger"]
    j = v.join(led)
    assert (j >= 0).all() and np.array_equal(led.length[j], v.length) and np.array_equal(led.scenario[j], v.scenario)
    assert np.array_equal(led.flags[j] & (1 | 2 | 8 | 16), v.flags)


def test_mode_cycle_equals_the_twin(base):
    env = _env(scenarios=base["scn"], mode="cycle", check_slots=SLOTS)
    env.reset()
    rec = _Rec(env)
    rec.run(base["acts"], 0, STEPS)
    tw = rec.twin(env.scenario_table)
    e = tw.ended()
    assert len({int(s) for s in tw.scenario[e & (tw.env == 0)]}) > 1, "env 0 never changed its scenario"
    assert tw.passed[e].any() and (tw.failed[e] & tw.valid[e]).any() and (tw.incomplete[e] & tw.valid[e]).any()
    _same(env.verdicts(include_open=True), tw)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 2: launch paths
def _free_run(env, acts, k0=0, k1=STEPS):
    for k in range(k0, k1):
        env.step(acts[k])
    env.join()
    env.torch.cuda.synchronize(env.device)


@pytest.mark.parametrize("ranges,deferred", [(1, False), (2, False), (4, True)], ids=["1-range", "2-ranges", "4-ranges-deferred"])
def test_ranges_and_deferred_join_give_the_same_bits(base, ranges, deferred):
    env = _env(scenarios=base["scn"], check_slots=SLOTS, ranges=ranges, deferred_join=deferred)
    assert env.engine.query("ranges") == ranges
    env.reset()
    _free_run(env, base["acts"])
    _same(env.verdicts(include_open=True), base["got"])
    np.testing.assert_array_equal(env.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))
    env.close()


def test_captured_graph_with_an_in_place_rewrite_of_the_bounds(base):
    """A captured step replayed; after 30 steps the bounds are rewritten in place (the same counts: the device pointers stay, the
    graph picks the new values up, every env's episode begins anew with flag 8).  An eager env that does the same agrees with the
    twin -- the steps before the rewrite under the first bounds, those behind it under the second -- and with the graph."""
    import copy
    import torch
    slots = 8                                                              # no record is lost: both halves stay in the rings
    scn2 = copy.deepcopy(base["scn"])
    for sc in scn2:
        for it in sc.get("checks", []):
            it[6] = float(np.float32(it[6]) * np.float32(0.5))
    e = _env(scenarios=base["scn"], check_slots=slots)
    e.reset()
    rec = _Rec(e)
    rec.run(base["acts"], 0, 30)
    table1 = e.scenario_table
    count30 = np.bincount(e.verdicts().env, minlength=N)
    e.set_scenarios(scn2, check_slots=slots)
    rec.run(base["acts"], 30, STEPS)
    want = e.verdicts(include_open=True)
    assert (want.lost == 0).all()
    a, b = rec.twin(table1, slots, 0, 30, include_open=False), rec.twin(e.scenario_table, slots, 30, STEPS, initial_flags=8)
    assert len(a) == count30.sum() > 0 and (b.flags & 8).any() and len(a) + len(b) == len(want)
    before = want.episode < count30[want.env]
    np.testing.assert_array_equal(want.words[before], a.words)
    wb = want.words[~before].copy()
    wb[:, 0] -= count30[want.env[~before]].astype(np.int32)                # the twin of the second half counts its episodes from 0
    np.testing.assert_array_equal(wb, b.words)
    np.testing.assert_array_equal(want.env[~before], b.env)
    e.close()

    g = _env(scenarios=base["scn"], check_slots=slots)
    g.reset()
    buf = torch.empty((N, g.action_dim), device=g.device)
    side = torch.cuda.Stream(device=g.device)
    buf.copy_(base["acts"][0])
    torch.cuda.synchronize(g.device)
    side.wait_stream(torch.cuda.current_stream(g.device))
    with torch.cuda.stream(side):
        g.step(buf)                                                        # warm-up, eager: step 0
    torch.cuda.current_stream(g.device).wait_stream(side)
    torch.cuda.synchronize(g.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(buf)                                                        # recorded, not run: the checks launch is part of the graph
    for k in range(1, STEPS):
        if k == 30:
            torch.cuda.synchronize(g.device)
            g.set_scenarios(scn2, check_slots=slots)
        buf.copy_(base["acts"][k])
        graph.replay()
    torch.cuda.synchronize(g.device)
    _same(g.verdicts(include_open=True), want)
    np.testing.assert_array_equal(g.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))
    g.close()


# ------------------------------------------------------------------------------------------------------------ 3: host cuts
def test_masked_reset_and_restore(base):
    """A masked reset() before step 20 leaves no record for the cut episodes; a restore() before step 40 of a snapshot taken after
    step 12 yields flag 8 and a clock that starts from the restored meta word 0."""
    env = _env(scenarios=base["scn"], check_slots=8)
    env.reset()
    rec = _Rec(env)
    rec.run(base["acts"], 0, 12)
    snap = env.snapshot()
    clock12 = _meta(env)[:, 0].copy()
    rec.run(base["acts"], 12, 20)
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    env.reset(mask=mask)
    rec.begins.append((20, mask, 0))
    rec.run(base["acts"], 20, 40)
    rmask = (np.arange(N) % 4 == 1).astype(np.uint8)
    env.restore(snap, mask=rmask)
    rec.begins.append((40, rmask, 8))
    rec.run(base["acts"], 40, STEPS)
    assert np.array_equal(rec.cols["clock"][40][rmask != 0], clock12[rmask != 0]) and (clock12[rmask != 0] > 0).any()
    got, tw = env.verdicts(include_open=True), rec.twin(env.scenario_table, slots=8)
    _same(got, tw)
    assert (got.lost == 0).all()
    # the cut episodes are nowhere: env 0's records are whole episodes, and the first after the restore carries flag 8
    te = rec.stacked("te") | rec.stacked("tr")
    for i in np.nonzero(mask)[0][:4]:
        ended = got.ended() & (got.env == i)
        assert int(ended.sum()) == int(te[:, i].sum())
    r = np.nonzero(rmask)[0]
    flagged = [(got.flags[(got.env == i)] & 8).any() for i in r]
    assert all(flagged)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 4: the feature only reads
def test_outputs_are_byte_identical_with_and_without_checks(base):
    from cosim_amd.ledger import same_records
    rd, rec = base["dry"], base["rec"]                                      # never given checks / checks armed
    for name in ("state", "info", "te", "tr", "cmd", "rows", "qpos", "qvel", "clock"):
        np.testing.assert_array_equal(rd.stacked(name).view(np.uint8), rec.stacked(name).view(np.uint8), err_msg=name)
    assert same_records(base["dry_ledger"], base["ledger"]) is None
    np.testing.assert_array_equal(base["dry_ledger"].words, base["ledger"].words)
    un = _env(scenarios=base["scn"])                                        # the table holds checks, check_slots unset: nothing is armed
    assert un.check_slots == 0 and un.engine.query("scenario_check_items") == 0 and un.engine.query("scenario_check_words") == 0
    with pytest.raises(ValueError, match="no checks are armed"):
        un.verdicts()
    un.reset()
    r = _Rec(un)
    r.run(base["acts"], 0, STEPS)
    for name in ("state", "info", "te", "tr"):
        np.testing.assert_array_equal(r.stacked(name).view(np.uint8), rd.stacked(name).view(np.uint8), err_msg=name)
    np.testing.assert_array_equal(un.ledger(include_open=True).words, base["dry_ledger"].words)
    un.close()


# ------------------------------------------------------------------------------------------------------------ 5: another model
def test_humanoid_equals_the_twin():
    model = _model("humanoid_p_v0")
    dry = _env(model, n=8, scenarios=[{}])
    dims = _dims(dry)
    dry.close()
    rng = np.random.default_rng(2)
    items = _items(16, rng, dims)
    for k, it in enumerate(items):
        it[0], it[1], it[6] = k % 3, k % 3 + 2 + k % 5, [0.0, 0.05, 0.98, 1.0][k % 4]
    scn = [{"checks": items}, {"checks": items[:3]}, {}]
    env = _env(model, n=8, scenarios=scn, check_slots=2)
    assert env.engine.query("scenario_check_items") == 16
    acts = _actions(env, 10)
    env.reset()
    rec = _Rec(env)
    rec.run(acts, 0, 10)
    got, tw = env.verdicts(include_open=True), rec.twin(env.scenario_table, slots=2)
    assert tw.valid.any() and (tw.aux[tw.valid] != -1).any()
    _same(got, tw)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 6: CLI, engine messages
def test_cli_require_pass(base, tmp_path, capsys):
    yaml = pytest.importorskip("yaml")
    from cosim_amd import cli
    from cosim_amd.checks import Verdicts
    common = ["--num-envs", "8", "--steps", "30", "--max-duration", "0.5", "--seed", "3", "--ledger", "4", "--check-slots", "4"]
    strict = tmp_path / "strict.yaml"
    strict.write_text(yaml.safe_dump({"scenarios": [{"checks": [[0, 20, "torque_max", 0, "always", "<", 1e-6, "no_torque"]]}]}))
    out = tmp_path / "v.npz"
    assert cli.main(common + ["--scenarios", str(strict), "--require-pass", "--verdicts-out", str(out)]) == 3
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["checks"]["episodes"] >= 8 and line["checks"]["episodes_failed"] == line["checks"]["episodes"]
    v = Verdicts.load(str(out))
    assert len(v) == line["checks"]["episodes"] and v.failed[:, 0].all() and v.names[0] == ["no_torque"] and (v.aux[:, 0] == 0).all()
    loose = tmp_path / "loose.yaml"
    loose.write_text(yaml.safe_dump({"scenarios": [{"checks": [[0, 20, "torque_max", 0, "always", "<", 1e9, "any_torque"]]}]}))
    assert cli.main(common + ["--scenarios", str(loose), "--require-pass"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["checks"]["episodes_failed"] == 0 and line["checks"]["episodes_passed"] == line["checks"]["episodes"] >= 8
    assert cli.main(common + ["--scenarios", str(strict)]) == 0             # without --require-pass the status stays 0


@pytest.mark.parametrize("mode", ["--graph", "--pipelined"])
def test_cli_under_graph_and_pipelined(tmp_path, capsys, mode):
    """The checks launch is part of a captured step and of the per-range pipeline: every ended episode has its verdict, joined to
    the ledger's record by (env, episode)."""
    yaml = pytest.importorskip("yaml")
    from cosim_amd import cli
    from cosim_amd.checks import Verdicts
    from cosim_amd.ledger import EpisodeLedger
    scn = tmp_path / "scn.yaml"
    scn.write_text(yaml.safe_dump({"scenarios": [{"checks": [[0, 20, "torque_max", 0, "always", "<", 1e-6, "no_torque"],
                                                             [0, 30, "up", 0, "always", ">", -2.0, "upright"]]},
                                                 {"checks": [[5, 25, "abs_info", "lin_vel_x", "mean", "<", 1e9, "vx"]]}]}))
    out, led = tmp_path / "v.npz", tmp_path / "led.npz"
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", mode, "--ledger", "4", "--scenarios", str(scn), "--check-slots", "4", "--verdicts-out", str(out),
                     "--ledger-out", str(led), "--require-pass"]) == 3
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    v, ledger = Verdicts.load(str(out)), EpisodeLedger.load(str(led))
    assert len(v) == len(ledger) == line["checks"]["episodes"] >= 64 and (v.lost == 0).all()
    j = v.join(ledger)
    assert (j >= 0).all() and np.array_equal(ledger.length[j], v.length) and np.array_equal(ledger.scenario[j], v.scenario)
    even = v.scenario == 0
    assert v.failed[even, 0].all() and (v.aux[even, 0] == 0).all() and v.incomplete[even, 1].all() and not v.failed[even, 1].any()
    assert v.passed[~even, 0].all() and (v.aux[~even, 0] == 20).all()
    assert line["checks"]["episodes_failed"] == int(even.sum()) and line["checks"]["episodes_passed"] == int((~even).sum())


def test_engine_validation_and_missing_info(base):
    env = _env(scenarios=base["scn"], check_slots=SLOTS, ledger=0)          # (no ledger: its own message about info_out_dev comes first)
    T = env.scenario_table
    adr, t, sig, idx, mode, cmp, bound = (x.copy() for x in T.pack_checks())

    def bad(match, slots=SLOTS, **kw):
        arrs = {"adr": adr, "t": t, "sig": sig, "idx": idx, "mode": mode, "cmp": cmp, "bound": bound}
        arrs.update(kw)
        with pytest.raises(ValueError, match=match):
            env.engine.scenario_checks_set((arrs["adr"], arrs["t"], arrs["sig"], arrs["idx"], arrs["mode"], arrs["cmp"], arrs["bound"]), slots)
    k = 64                                                                  # scenario 1, item 0
    x = bound.copy(); x[k] = np.inf
    bad(r"scenario 1, check item 0: bound is not finite", bound=x)
    x = t.copy(); x[k] = (7, 7)
    bad(r"scenario 1, check item 0: t1 7 is not after t0 7", t=x)
    x = t.copy(); x[3] = (-1, 7)
    bad(r"scenario 0, check item 3: times outside \[0, 2\^30\)", t=x)
    x = sig.copy(); x[k] = 9
    bad(r"scenario 1, check item 0: unknown signal 9", sig=x)
    x = mode.copy(); x[k] = 3
    bad(r"scenario 1, check item 0: unknown mode 3", mode=x)
    x = cmp.copy(); x[k] = 2
    bad(r"scenario 1, check item 0: unknown cmp 2", cmp=x)
    x = idx.copy(); x[k] = 3
    bad(r"scenario 1, check item 0: index 3 out of range: tracking_error has 3 entries", idx=x)   # min(command_dim 4, 3)
    bad(r"slots 0 outside 1\.\.64", slots=0)
    bad(r"slots 65 outside 1\.\.64", slots=65)
    bad(r"3 scenarios, the table that is set has 4", adr=adr[:4])
    x = np.concatenate([[0, 65], np.full(3, 65)]).astype(np.int32)
    bad(r"scenario 0: 65 check items, at most 64", adr=x, t=np.tile(t[:1], (65, 1)), sig=np.repeat(sig[:1], 65), idx=np.repeat(idx[:1], 65),
        mode=np.repeat(mode[:1], 65), cmp=np.repeat(cmp[:1], 65), bound=np.repeat(bound[:1], 65))
    assert env.engine.query("scenario_check_items") == 64, "a refused call changed the checks that are set"
    env.reset()
    a = _actions(env, 1)
    with pytest.raises(ValueError, match="scenario checks are set .* info_out_dev is NULL"):
        env.engine.step(a[0].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(), None, env._stream())
    env.set_scenarios(base["scn"][:3], check_slots=SLOTS)                   # another S: the old checks are dropped, the new ones set
    assert env.engine.query("scenario_rows") == 3 and env.engine.query("scenario_check_items") == 64
    env.set_scenarios(base["scn"][:3])                                      # not armed: cleared
    assert env.engine.query("scenario_check_items") == 0 and env.check_slots == 0
    env.set_scenarios(None)
    with pytest.raises(ValueError, match="no scenario table is set"):
        env.engine.scenario_checks_set(T.pack_checks(), SLOTS)
    env.close()
