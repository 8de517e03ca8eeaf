"""Response curves on the device (cosim_scenario_curves_set / _get / _clear, csrc/cosim_curves.hip, and their BatchedEnv / CLI surface)
against the numpy twin (cosim_amd/curves.py reference_curves) fed with what a host-driven loop reads around every step.

Every comparison is exact (cells as words).  The common fleet is 24 flamingo_light_v1 on the plane with a 25-step time limit and a tilt
rule, run for 60 control steps under auto-reset from a fixed action table, under four scenarios: row 0 holds 8 items over every
signal, row 1 a single item, row 2 none, row 3 a push that throws the robot over and three items.  lo / hi of every item are the 10 %
and 90 % quantiles of its signal over its window in a dry run of the same seed (the engine is a bit-exact function of the seed), so
underflow and overflow rows, both outcome classes and thin bins all occur -- asserted, so that no comparison is empty."""
import copy
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS = 24, 60
CMD = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)
WINDOWS = [(0, 25, 1), (0, 25, 3), (5, 20, 2), (10, 25, 4), (3, 4, 1), (0, 24, 5), (12, 18, 1), (2, 25, 7)]
BINS = [4, 64, 0, 7, 1, 16, 33, 2]
SIGNALS = ["info", "abs_info", "tracking_error", "torque_max", "up", "qpos", "qvel", "abs_qvel"]
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


def _items(n, rng, dims, first=0):
    """n items cycling through the signals, windows and bin counts; lo / hi are filled in from the dry run."""
    info_dim, cd, nq, nv = dims
    out = []
    for k in range(first, first + n):
        sig = SIGNALS[k % 8]
        width = {"info": info_dim, "abs_info": info_dim, "tracking_error": min(cd, 3), "torque_max": 1, "up": 1, "qpos": nq, "qvel": nv, "abs_qvel": nv}[sig]
        t0, t1, every = WINDOWS[k % 8]
        out.append([t0, t1, every, sig, int(rng.integers(width)), 0.0, 1.0, BINS[k % 8], f"c{k}"])
    return out


def _scenarios(dims, lohi=None, seed=5):
    rng = np.random.default_rng(seed)
    cd = dims[1]
    scn = [{"commands": [[0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0][:1 + cd]], "curves": _items(8, rng, dims)},
           {"curves": [[0, 25, 1, "tracking_error", 0, 0.0, 1.0, 32, "tracks"]], "checks": [[0, 25, "tracking_error", 0, "settle", "<", 0.3, "chk"]]},
           {"commands": [[0, 0.2, 0.0, 0.0, 0.0, 0.0, 0.0][:1 + cd]]},
           {"pushes": [[5, 10, 6.0, 0.0, 0.0]], "curves": _items(2, rng, dims, first=4) + [[0, 25, 2, "up", 0, 0.0, 1.0, 8, "upright"]]}]
    if lohi is not None:
        for sc, b in zip(scn, lohi):
            for it, (lo, hi) in zip(sc.get("curves", []), b):
                it[5], it[6] = float(lo), float(hi)
    return scn


def _strip(scn, *keys):
    return [{k: v for k, v in sc.items() if k not in keys} for sc in scn]


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
    the state record.  ``twin`` feeds it all to reference_curves."""

    def __init__(self, env):
        self.env = env
        self.cols = {k: [] for k in ("clock", "info", "te", "tr", "cmd", "rows", "qpos", "qvel", "state")}
        self.begins, self.clears = [], []

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

    def twin(self, table, k0=0, k1=None):
        """The twin over the recorded steps [k0, k1)."""
        from cosim_amd.curves import reference_curves
        env = self.env
        K = len(self.cols["info"])
        k1 = K if k1 is None else k1
        col = lambda name: np.stack(self.cols[name][k0:k1])   # noqa: E731
        clock = np.stack(self.cols["clock"][k0:k1] + [_meta(env)[:, 0] if k1 == K else self.cols["clock"][k1]])
        return reference_curves(table, col("info"), col("te"), col("tr"), col("cmd"), col("qpos"), col("qvel"), clock, col("rows"), env.action_dim,
                                begins=[(k - k0, mk, f) for k, mk, f in self.begins if k0 < k <= k1],
                                clears=[k - k0 for k in self.clears if k0 < k <= k1])


def _lohi(rec, scn, dims, nu):
    """Per item the 10 % and 90 % quantiles of its signal over its window in the recorded run, over the envs and steps that ran the
    item's row, as float32."""
    from cosim_amd.checks import _signal
    from cosim_amd.scenario import CHECK_SIGNALS, ScenarioTable
    T = ScenarioTable(scn, dims[1]).resolve_curves(None)
    info, cmd, qpos, qvel, clock, rows = (rec.stacked(k) for k in ("info", "cmd", "qpos", "qvel", "clock", "rows"))
    done = (rec.stacked("te") | rec.stacked("tr")) != 0
    out = []
    for s, items in enumerate(T.curves):
        b = []
        for t0, t1, every, sig, idx, *_ in items:
            sel = np.argwhere((rows == s) & (clock >= t0) & (clock < t1) & ((clock - t0) % every == 0) & ~(done & (sig >= CHECK_SIGNALS["up"])))
            v = np.asarray([_signal(sig, idx, info[k, i], cmd[k, i], qpos[k, i], qvel[k, i], nu) for k, i in sel], dtype=np.float32)
            v = v[np.isfinite(v)]
            lo, hi = (np.float32(np.quantile(v, 0.1)), np.float32(np.quantile(v, 0.9))) if len(v) else (np.float32(0), np.float32(1))
            b.append((lo, hi if hi > lo else np.float32(lo + np.float32(1.0))))
        out.append(b)
    return out


def _same(a, b, what=""):
    from cosim_amd.curves import same_curves
    diff = same_curves(a, b)
    assert diff is None, what + diff


def _coverage(cv, rec):
    """What the run must contain, on the twin's result."""
    e = cv.episodes()
    assert e[:, 0].sum() > 0 and e[:, 1].sum() > 0, "an outcome class is empty: no fall or no time limit in the run"
    under = over = thin = 0
    for s, k in cv.items():
        c = cv[s, k]
        if c.bins > 0:
            under += int(c.hist()[0].sum())
            over += int(c.hist()[-1].sum())
        n = c.count() + c.nan()
        thin += int(((n > 0) & (n < n.max())).sum())
    assert under > 0 and over > 0, "no sample outside [lo, hi)"
    assert thin > 0, "no bin with fewer samples than episodes"
    info = rec.stacked("info")
    if np.isfinite(info).all() and np.isfinite(rec.stacked("qpos")).all() and np.isfinite(rec.stacked("qvel")).all():
        assert cv.summary()["nonfinite"] == 0                                 # a non-zero nan cell only if the run produced one
    assert {s for s, _ in cv.items()} == {0, 1, 3} and len(cv.items()) == 12


@pytest.fixture(scope="module")
def base():
    """The dry run (a table without curves or checks), the lo / hi it gives, and the common run with the curves armed, host-driven."""
    dry = _env()
    dims = _dims(dry)
    scn0 = _scenarios(dims)
    dry.set_scenarios(_strip(scn0, "curves", "checks"))
    acts = _actions(dry)
    dry.reset()
    rd = _Rec(dry)
    rd.run(acts, 0, STEPS)
    scn = _scenarios(dims, _lohi(rd, scn0, dims, dry.action_dim))
    env = _env(scenarios=scn, curves=True)
    assert env.curves_armed and env.engine.query("scenario_curve_items") == 12
    assert env.engine.query("scenario_curve_stage_words") == 25 + 9 + 8 + 4 + 1 + 5 + 6 + 4
    env.reset()
    rec = _Rec(env)
    rec.run(acts, 0, STEPS)
    got = env.curves()
    assert env.engine.query("scenario_curve_words") == got.cells.size
    out = {"dry": rd, "dry_ledger": dry.ledger(include_open=True), "rec": rec, "got": got, "scn": scn, "acts": acts,
           "ledger": env.ledger(include_open=True), "table": env.scenario_table, "final": env.state.cpu().numpy().copy(), "dims": dims}
    dry.close()
    yield out
    env.close()


# ------------------------------------------------------------------------------------------------------------ 1: against the twin
def test_device_cells_equal_the_twin(base):
    tw = base["rec"].twin(base["table"])
    _coverage(tw, base["rec"])
    _same(base["got"], tw)
    # the episodes folded are the ledger's ended episodes, class by class (every episode of rows 0, 1, 3 reaches its fullest bin or
    # ends ahead of it: the count can only be lower)
    led = base["ledger"]
    ended = (led.flags & 16) == 0
    assert 0 < base["got"].episodes().sum() <= int(ended.sum())


def test_mode_cycle_equals_the_twin(base):
    env = _env(scenarios=base["scn"], mode="cycle", curves=True)
    env.reset()
    rec = _Rec(env)
    rec.run(base["acts"], 0, STEPS)
    tw = rec.twin(env.scenario_table)
    assert len(set(rec.stacked("rows")[:, 0].tolist())) > 1, "env 0 never changed its scenario"
    assert tw.episodes()[:, 0].sum() > 0 and tw.episodes()[:, 1].sum() > 0
    _same(env.curves(), tw)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 2: launch paths
def _free_run(env, acts, k0=0, k1=STEPS):
    for k in range(k0, k1):
        env.step(acts[k])
    env.join()
    env.torch.cuda.synchronize(env.device)


def _shard_run(env, acts, shards, k0=0, k1=STEPS):
    """Every step as step_range launches on streams of their own, the shards in either order."""
    import torch
    streams = [torch.cuda.Stream(device=env.device) for _ in shards]
    torch.cuda.synchronize(env.device)
    for k in range(k0, k1):
        for (first, count), st in zip(shards[::-1] if k % 2 else shards, streams[::-1] if k % 2 else streams):
            with torch.cuda.stream(st):
                env.step_range(first, count, acts[k])
    torch.cuda.synchronize(env.device)


@pytest.mark.parametrize("ranges,deferred", [(1, False), (4, True)], ids=["1-range", "4-ranges-deferred"])
def test_ranges_and_deferred_join_give_the_same_bits(base, ranges, deferred):
    env = _env(scenarios=base["scn"], curves=True, ranges=ranges, deferred_join=deferred)
    assert env.engine.query("ranges") == ranges
    env.reset()
    _free_run(env, base["acts"])
    _same(env.curves(), base["got"])
    np.testing.assert_array_equal(env.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))
    env.close()


def test_two_uneven_ranges_and_step_range_chains_give_the_same_bits(base):
    a = _env(scenarios=base["scn"], curves=True)
    a.reset()
    _shard_run(a, base["acts"], [(0, 11), (11, 13)])
    _same(a.curves(), base["got"], "two uneven ranges: ")
    np.testing.assert_array_equal(a.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))
    a.close()
    import torch
    c = _env(scenarios=base["scn"], curves=True, ranges=4, deferred_join=True)
    c.reset()
    torch.cuda.synchronize(c.device)
    for k in range(STEPS):
        for (first, count), st in zip(c.range_list, c.range_streams):
            with torch.cuda.stream(st):
                c.step_range(first, count, base["acts"][k])
            c.range_mark(c.range_list.index((first, count)))
    c.join()
    torch.cuda.synchronize(c.device)
    _same(c.curves(), base["got"], "step_range chains: ")
    c.close()


def test_captured_graph_with_an_in_place_rewrite_of_lo_hi(base):
    """A captured step replayed: n replays equal n eager steps.  After 30 steps lo / hi are rewritten in place (the same counts and
    sizes: the device pointers stay, the graph picks the new values up, the cells are emptied and every env's episode begins anew).
    An eager env that does the same agrees with the twin of the steps behind the rewrite under the second table, and with the graph."""
    import torch
    scn2 = copy.deepcopy(base["scn"])
    for sc in scn2:
        for it in sc.get("curves", []):
            mid, half = 0.5 * (it[5] + it[6]), 0.25 * (it[6] - it[5])
            it[5], it[6] = float(np.float32(mid - half)), float(np.float32(mid + half))
    e = _env(scenarios=base["scn"], curves=True)
    e.reset()
    rec = _Rec(e)
    rec.run(base["acts"], 0, 30)
    _same(e.curves(), rec.twin(e.scenario_table, 0, 30), "the first 30 steps: ")
    assert e.curves().episodes().sum() > 0
    cells_ptr = e.engine.query("scenario_curve_words")
    e.set_scenarios(scn2, curves=True)
    assert e.engine.query("scenario_curve_words") == cells_ptr and e.curves().summary()["samples"] == 0, "the rewrite did not empty the cells"
    rec.run(base["acts"], 30, STEPS)
    want = e.curves()
    tw = rec.twin(e.scenario_table, 30, STEPS)
    assert tw.episodes().sum() > 0 and tw.lohi[0, 0] != base["got"].lohi[0, 0]
    _same(want, tw, "behind the rewrite: ")
    e.close()

    g = _env(scenarios=base["scn"], curves=True)
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
        g.step(buf)                                                        # recorded, not run: the curves launch is part of the graph
    for k in range(1, STEPS):
        if k == 30:
            torch.cuda.synchronize(g.device)
            _same(g.curves(), rec.twin(base["table"], 0, 30), "1 eager step and 29 replays: ")
            g.set_scenarios(scn2, curves=True)
        buf.copy_(base["acts"][k])
        graph.replay()
    torch.cuda.synchronize(g.device)
    _same(g.curves(), want, "the graph behind the rewrite: ")
    np.testing.assert_array_equal(g.state.cpu().numpy().view(np.int32), base["final"].view(np.int32))
    g.close()


@pytest.mark.parametrize("n_scn", [1, 3])
def test_many_waves_fold_into_the_same_cells(n_scn):
    """130 envs under S = 1 and S = 3: at the time limit every env of a scenario folds into the same cells in the same launch.  One
    launch per step against two shards of 67 + 63 envs (a range boundary inside a block of four waves, a tail block in each)."""
    dims_env = _env(n=4, scenarios=[{}])
    dims = _dims(dims_env)
    dims_env.close()
    rng = np.random.default_rng(8)
    rows = [_items(8, rng, dims), _items(3, rng, dims, first=3), _items(1, rng, dims, first=1)][:n_scn]
    for r in rows:
        for it in r:
            it[5], it[6] = (-0.3, 0.4) if it[3] in ("info", "tracking_error", "qpos", "qvel") else (0.05, 0.9)
    scn = [{"curves": r} for r in rows]
    steps = 30
    a = _env(n=130, scenarios=scn, curves=True)
    acts = _actions(a, steps)
    a.reset()
    rec = _Rec(a)
    rec.run(acts, 0, steps)
    got = a.curves()
    tr = rec.stacked("tr") != 0
    assert tr[24].sum() >= 8, "the time limit did not end many envs in one step"
    assert got.episodes()[:, 0].sum() >= tr[24].sum()
    _same(got, rec.twin(a.scenario_table), "one launch: ")
    a.close()
    b = _env(n=130, scenarios=scn, curves=True)
    b.reset()
    _shard_run(b, acts, [(0, 67), (67, 63)], 0, steps)
    _same(b.curves(), got, "67 + 63: ")
    b.close()


# ------------------------------------------------------------------------------------------------------------ 3: host cuts
def test_masked_reset_restore_and_clear(base):
    """A masked reset() before step 20 and a restore() before step 40 of a snapshot taken after step 12 discard what the envs they
    touch had staged; clear_curves() before step 48 empties the cells and begins every env anew."""
    env = _env(scenarios=base["scn"], curves=True)
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
    rec.run(base["acts"], 40, 48)
    assert np.array_equal(rec.cols["clock"][40][rmask != 0], clock12[rmask != 0]) and (clock12[rmask != 0] > 0).any()
    mid, tw_mid = env.curves(), rec.twin(env.scenario_table)
    _same(mid, tw_mid, "before the clear: ")
    assert same_or_none(mid, base["got"]) is not None, "the cuts changed nothing"
    env.clear_curves()
    assert env.curves().summary()["samples"] == 0 and env.curves().summary()["episodes"] == 0
    rec.clears.append(48)
    rec.run(base["acts"], 48, STEPS)
    got, tw = env.curves(), rec.twin(env.scenario_table)
    assert tw.summary()["samples"] > 0
    _same(got, tw, "behind the clear: ")
    env.close()


def same_or_none(a, b):
    from cosim_amd.curves import same_curves
    return same_curves(a, b)


# ------------------------------------------------------------------------------------------------------------ 4: the feature only reads
def test_outputs_are_byte_identical_with_and_without_curves(base):
    """States, flags, info, ledger records and verdicts: curves armed, carried but not armed, never given."""
    from cosim_amd.checks import same_verdicts
    rd, rec = base["dry"], base["rec"]                                      # never given curves / curves armed
    for name in ("state", "info", "te", "tr", "cmd", "rows", "qpos", "qvel", "clock"):
        np.testing.assert_array_equal(rd.stacked(name).view(np.uint8), rec.stacked(name).view(np.uint8), err_msg=name)
    np.testing.assert_array_equal(base["dry_ledger"].words, base["ledger"].words)
    runs = {}
    for name, scn, kw in (("armed", base["scn"], {"curves": True}), ("carried", base["scn"], {}), ("never", _strip(base["scn"], "curves"), {})):
        env = _env(scenarios=scn, check_slots=2, **kw)
        assert env.curves_armed == (name == "armed") and (env.engine.query("scenario_curve_items") > 0) == (name == "armed")
        if name != "armed":
            assert env.engine.query("scenario_curve_words") == 0 and env.engine.query("scenario_curve_stage_words") == 0
            with pytest.raises(ValueError, match="no curves are armed"):
                env.curves()
        env.reset()
        r = _Rec(env)
        r.run(base["acts"], 0, STEPS)
        runs[name] = (r, env.ledger(include_open=True), env.verdicts(include_open=True))
        if name == "armed":
            _same(env.curves(), base["got"])
        env.close()
    for name in ("carried", "never"):
        for col in ("state", "info", "te", "tr", "cmd", "rows"):
            np.testing.assert_array_equal(runs[name][0].stacked(col).view(np.uint8), runs["armed"][0].stacked(col).view(np.uint8), err_msg=f"{name} {col}")
        np.testing.assert_array_equal(runs[name][1].words, runs["armed"][1].words)
        assert same_verdicts(runs[name][2], runs["armed"][2]) is None
    assert len(runs["armed"][2]) > 0
    np.testing.assert_array_equal(runs["armed"][0].stacked("state").view(np.uint8), rd.stacked("state").view(np.uint8))


# ------------------------------------------------------------------------------------------------------------ 5: other models
def test_humanoid_equals_the_twin():
    model = _model("humanoid_p_v0")
    dry = _env(model, n=4, scenarios=[{}])
    dims = _dims(dry)
    dry.close()
    rng = np.random.default_rng(2)
    items = _items(8, rng, dims)
    for k, it in enumerate(items):
        it[0], it[1], it[2] = k % 3, k % 3 + 2 + k % 5, 1 + k % 2
        it[5], it[6] = [(-0.1, 0.1), (0.0, 0.05), (0.0, 0.5), (0.5, 20.0), (0.9, 1.0), (-0.2, 0.2), (-0.5, 0.5), (0.0, 0.5)][k]
    scn = [{"curves": items}, {"curves": items[:3]}, {}]
    env = _env(model, n=4, scenarios=scn, curves=True, fall=None)
    assert env.engine.query("scenario_curve_items") == 11
    acts = _actions(env, 30)
    env.reset()
    rec = _Rec(env)
    rec.run(acts, 0, 30)
    got, tw = env.curves(), rec.twin(env.scenario_table)
    assert tw.summary()["samples"] > 0
    _same(got, tw)
    env.close()


def test_split_pipeline_on_stairs_equals_the_twin():
    """humanoid_p_v0 on stairs_up_hard, 4 envs, a few steps: the curves launch follows the last substep's launches.  A height rule far
    above the robot ends every episode at once, so the few steps fold."""
    from cosim_amd.fall import FallRule
    model = _model("humanoid_p_v0", "stairs_up_hard", position_command=True)
    scn = [{"curves": [[0, 4, 1, "torque_max", 0, 0.0, 50.0, 8, "tq"], [0, 4, 2, "up", 0, 0.5, 1.0, 4, "up"], [0, 3, 1, "qvel", 2, -1.0, 1.0, 0, "vz"]]}, {}]
    env = _env(model, n=4, scenarios=scn, curves=True, fall=FallRule(height=5.0, grace=2))
    assert env.engine.query("split") > 0
    acts = _actions(env, 6)
    env.reset()
    rec = _Rec(env)
    rec.run(acts, 0, 6)
    got, tw = env.curves(), rec.twin(env.scenario_table)
    assert tw.episodes()[0, 1] > 0 and tw.summary()["samples"] > 0
    _same(got, tw)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 6: CLI, engine messages
@pytest.mark.parametrize("mode", ["--graph", "--pipelined"])
def test_cli_under_graph_and_pipelined(tmp_path, capsys, mode):
    """The curves launch is part of a captured step and of the per-range pipeline: every ended episode of the ledger that reached a
    curve's first bin is in its cells."""
    yaml = pytest.importorskip("yaml")
    from cosim_amd import cli
    from cosim_amd.curves import Curves
    from cosim_amd.ledger import EpisodeLedger
    scn = tmp_path / "scn.yaml"
    scn.write_text(yaml.safe_dump({"scenarios": [{"curves": [[0, 25, 1, "torque_max", 0, 0.0, 1.0e9, 8, "torque"],
                                                             [0, 25, 5, "up", 0, -2.0, 2.0, 4, "upright"]]},
                                                 {"curves": [[0, 25, 1, "abs_info", "lin_vel_x", 0.0, 1.0e9, 0, "vx"]]}]}))
    out, led = tmp_path / "c.npz", tmp_path / "led.npz"
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", mode, "--ledger", "4", "--scenarios", str(scn), "--curves", "--curves-out", str(out),
                     "--ledger-out", str(led)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    cv, ledger = Curves.load(str(out)), EpisodeLedger.load(str(led))
    assert cv.names == [["torque", "upright"], ["vx"]] and line["curves"]["items"] == 3
    for s in (0, 1):                                                       # bin 0 is sampled by every episode (info signals, t = 0)
        first = cv[s, 0]
        for cls, flag in ((0, 2), (1, 1)):
            want = int(((ledger.scenario == s) & ((ledger.flags & 3) == flag if cls == 0 else (ledger.flags & 1) != 0)).sum())
            assert int(first._count[cls, 0] + first._nan[cls, 0]) == want
    assert line["curves"]["episodes"] == len(ledger) >= 64 == 2 * 32
    assert line["curves"]["samples"] == cv.summary()["samples"] > 0


def test_engine_validation_and_missing_info(base):
    env = _env(scenarios=base["scn"], curves=True, ledger=0)                # (no ledger: its own message about info_out_dev comes first)
    T = env.scenario_table
    adr, t, sig, idx, lo, hi, bins = (x.copy() for x in T.pack_curves())

    def bad(match, **kw):
        arrs = {"adr": adr, "t": t, "sig": sig, "idx": idx, "lo": lo, "hi": hi, "bins": bins}
        arrs.update(kw)
        with pytest.raises(ValueError, match=match):
            env.engine.scenario_curves_set((arrs["adr"], arrs["t"], arrs["sig"], arrs["idx"], arrs["lo"], arrs["hi"], arrs["bins"]))
    k = 8                                                                   # scenario 1, item 0
    x = lo.copy(); x[k] = np.nan
    bad(r"scenario 1, curve item 0: lo / hi is not finite", lo=x)
    x = hi.copy(); x[k] = np.inf
    bad(r"scenario 1, curve item 0: lo / hi is not finite", hi=x)
    x = hi.copy(); x[k] = lo[k]
    bad(r"scenario 1, curve item 0: hi is not above lo", hi=x)
    x = t.copy(); x[k] = (7, 7, 1)
    bad(r"scenario 1, curve item 0: t1 7 is not after t0 7", t=x)
    x = t.copy(); x[3] = (-1, 7, 1)
    bad(r"scenario 0, curve item 3: times outside \[0, 2\^30\)", t=x)
    x = t.copy(); x[k] = (0, 25, 0)
    bad(r"scenario 1, curve item 0: every 0 is below 1", t=x)
    x = t.copy(); x[k] = (0, 1025, 1)
    bad(r"scenario 1, curve item 0: 1025 time bins, at most 1024", t=x)
    x = bins.copy(); x[k] = 65
    bad(r"scenario 1, curve item 0: bins 65 outside 0\.\.64", bins=x)
    x = sig.copy(); x[k] = 9
    bad(r"scenario 1, curve item 0: unknown signal 9", sig=x)
    x = idx.copy(); x[k] = 3
    bad(r"scenario 1, curve item 0: index 3 out of range: tracking_error has 3 entries", idx=x)   # min(command_dim 4, 3)
    bad(r"3 scenarios, the table that is set has 4", adr=adr[:4])
    x = np.concatenate([[0, 9], np.full(3, 9)]).astype(np.int32)
    bad(r"scenario 0: 9 curve items, at most 8", adr=x)
    assert env.engine.query("scenario_curve_items") == 12, "a refused call changed the curves that are set"
    env.reset()
    a = _actions(env, 1)
    with pytest.raises(ValueError, match="response curves are set .* info_out_dev is NULL"):
        env.engine.step(a[0].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(), None, env._stream())
    env.set_scenarios(base["scn"][:3], curves=True)                         # another S: the old curves are dropped, the new ones set
    assert env.engine.query("scenario_rows") == 3 and env.engine.query("scenario_curve_items") == 9
    env.set_scenarios(base["scn"][:3])                                      # not armed: cleared
    assert env.engine.query("scenario_curve_items") == 0 and not env.curves_armed
    with pytest.raises(ValueError, match="no curves are set"):
        env.engine.scenario_curves_clear()
    env.set_scenarios(None)
    with pytest.raises(ValueError, match="no scenario table is set"):
        env.engine.scenario_curves_set(T.pack_curves())
    env.close()
    # the design limit: 64 scenarios of 8 items x 2 classes x 72 x 1024 words are 288 MiB of cells; scenario 56 crosses 256 MiB
    big = _env(n=4, scenarios=[{}] * 64, ledger=0)
    n = 64 * 8
    with pytest.raises(ValueError, match=r"scenario 56, curve item \d: the cells would exceed 256 MiB"):
        big.engine.scenario_curves_set((np.arange(0, n + 1, 8, dtype=np.int32), np.tile(np.array([0, 1024, 1], dtype=np.int32), (n, 1)), np.zeros(n, np.int32),
                                        np.zeros(n, np.int32), np.zeros(n, np.float32), np.ones(n, np.float32), np.full(n, 64, np.int32)))
    assert big.engine.query("scenario_curve_items") == 0
    big.close()
