"""Response curves split by policy on the device (cosim_scenario_curves_groups, curves_step_grouped_kernel in csrc/cosim_curves.hip,
``BatchedEnv.set_curve_groups`` and the CLI's ``--curves-by policy``) against the numpy twin (``reference_curves(groups=...)``) fed with
what a loop reads around every step, the group words as the fold saw them included.

Every comparison is exact (cells as words).  The fleet is the curves tests': 24 flamingo_light_v1 on the plane with a 25-step time
limit and a tilt rule, 60 control steps under auto-reset, four scenarios (8 items, one item, none, a push with three items), lo / hi
from the 10 % / 90 % quantiles of a dry run -- here driven by K = 3 random 64 x 64 actors in a policy table.  Every test asserts what its
run must contain so that no comparison is empty: no lost episode (but in the guard test), every group folds an episode, two groups at
least hold both outcome classes, and under rotation every env ends episodes under two different policies at least."""
import copy
import json

import numpy as np
import pytest

from test_gpu_curves import N, STEPS, _Rec, _actions, _dims, _env, _lohi, _meta, _same, _scenarios, _strip

pytestmark = pytest.mark.gpu

K = 3
NAMES = ["p0", "p1", "p2"]


def _files(d, env, recurrent=False):
    from cosim_amd.policy import write_random_lstm, write_random_mlp
    files = [str(d / f"p{k}.onnx") for k in range(K)]
    for k, f in enumerate(files):
        if recurrent:
            write_random_lstm(f, env.state_dim, env.action_dim, hidden=32, head=(32,), seed=40 + k)
        else:
            write_random_mlp(f, env.state_dim, env.action_dim, hidden=(64, 64), seed=30 + k)
    return files


def _table(files, env, rotate=1, recurrent=False, **kw):
    from cosim_amd.policy import PolicyTable, RecurrentPolicyTable
    return (RecurrentPolicyTable if recurrent else PolicyTable)(files, num_envs=env.num_envs, device=env.device, rotate_every=rotate, **kw)


class _Loop:
    """What ``Runner.test`` reads around every step: ``before`` (its ``before_step``) meta word 0, ``after`` (its ``on_step``) the
    step's outputs as ``test_gpu_curves._Rec`` records them and the group words -- behind the step and the table's ``reset(mask)``,
    ahead of its next forward: what the fold of this step read."""

    def __init__(self, env, words):
        self.env, self.words = env, words
        self.cols = {k: [] for k in ("clock", "info", "te", "tr", "cmd", "rows", "qpos", "qvel", "state", "grp")}
        self.begins, self.clears = [], []

    def before(self, k):
        self.cols["clock"].append(_meta(self.env)[:, 0].copy())

    def after(self, k=None, *_):
        env, c = self.env, self.cols
        env.join()
        env.torch.cuda.synchronize(env.device)
        d = env.get_data()
        c["qpos"].append(d.qpos.cpu().numpy().copy()); c["qvel"].append(d.qvel.cpu().numpy().copy())
        c["info"].append(env.info_buf.cpu().numpy().copy()); c["state"].append(env.state.cpu().numpy().copy())
        c["cmd"].append(env.applied_command.cpu().numpy()[:, :max(env.command_dim, 1)].copy())
        c["te"].append(env.terminated.cpu().numpy().copy()); c["tr"].append(env.truncated.cpu().numpy().copy())
        c["rows"].append(env.scenario_rows().astype(np.int32))
        c["grp"].append(self.words.cpu().numpy().copy())

    def host(self, acts, k0, k1):
        """A host-driven loop over a fixed action table."""
        for k in range(k0, k1):
            self.before(k)
            self.env.step(acts[k])
            self.after(k)

    def stacked(self, name):
        return np.stack(self.cols[name])

    def twin(self, table, n_groups=K, names=None, k0=0, k1=None, envs=None):
        """The twin over the recorded steps [k0, k1) of the envs ``envs`` (a bool mask; default: all); ``n_groups = 0``: without groups."""
        from cosim_amd.curves import reference_curves
        env = self.env
        steps = len(self.cols["info"])
        k1 = steps if k1 is None else k1
        sel = np.ones(env.num_envs, dtype=bool) if envs is None else np.asarray(envs, dtype=bool)
        col = lambda name: np.stack(self.cols[name][k0:k1])[:, sel]   # noqa: E731
        clock = np.stack(self.cols["clock"][k0:k1] + [_meta(env)[:, 0] if k1 == steps else self.cols["clock"][k1]])[:, sel]
        more = {"groups": col("grp"), "n_groups": n_groups, "group_names": names} if n_groups else {}
        return reference_curves(table, col("info"), col("te"), col("tr"), col("cmd"), col("qpos"), col("qvel"), clock, col("rows"), env.action_dim,
                                begins=[(k - k0, None if mk is None else np.asarray(mk)[sel], f) for k, mk, f in self.begins if k0 < k <= k1],
                                clears=[k - k0 for k in self.clears if k0 < k <= k1], **more)


def _runner(env, tab):
    from cosim_amd.runner import Runner
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    return run


def _contents(cv, rec=None, rotating=False):
    """What a grouped run must contain."""
    assert cv.groups == K and cv.ungrouped == 0, f"{cv.ungrouped} episodes lost"
    eps = [p.episodes().sum(axis=0) for p in cv.by_group().values()]
    assert all(e.sum() > 0 for e in eps), f"a group folded no episode: {eps}"
    assert sum(1 for e in eps if e[0] > 0 and e[1] > 0) >= 2, f"fewer than two groups hold both outcome classes: {eps}"
    if rotating:
        done = (rec.stacked("te") | rec.stacked("tr")) != 0
        grp = rec.stacked("grp")
        for i in range(grp.shape[1]):
            assert len(set(grp[done[:, i], i].tolist())) >= 2, f"env {i} ended its episodes under one policy only"


@pytest.fixture(scope="module")
def fleet(tmp_path_factory):
    """The dry run under the rotating table (a scenario table without curves), the lo / hi it gives, and the common run: the curves
    armed and split by the rotating table through ``Runner.test``."""
    d = tmp_path_factory.mktemp("curve_groups")
    dry = _env()
    dims = _dims(dry)
    scn0 = _scenarios(dims)
    dry.set_scenarios(_strip(scn0, "curves", "checks"))
    files = _files(d, dry)
    tab0 = _table(files, dry)
    rd = _Loop(dry, tab0.policy_now)
    assert _runner(dry, tab0).test(max_steps=STEPS, before_step=rd.before, on_step=rd.after) == STEPS
    scn = _scenarios(dims, _lohi(rd, scn0, dims, dry.action_dim))
    dry_final = dry.state.cpu().numpy().copy()
    dry.close()
    env = _env(scenarios=scn, curves=True)
    tab = _table(files, env)
    words, n_groups, names = tab.curve_groups()
    assert words is tab.policy_now and n_groups == K and names == NAMES
    env.set_curve_groups(tab)
    assert env.engine.query("scenario_curve_groups") == K and env.engine.query("scenario_curve_items") == 12
    rec = _Loop(env, tab.policy_now)
    assert _runner(env, tab).test(max_steps=STEPS, before_step=rec.before, on_step=rec.after) == STEPS
    got = env.curves()
    assert got.cells.size == K * env.engine.query("scenario_curve_words") and env.curve_groups_lost() == 0
    out = {"files": files, "scn": scn, "dims": dims, "rec": rec, "got": got, "table": env.scenario_table, "final": env.state.cpu().numpy().copy(),
           "dry_final": dry_final, "ledger": env.ledger(include_open=True), "rfiles": _files(tmp_path_factory.mktemp("curve_groups_lstm"), env, True)}
    yield out
    env.close()


# ------------------------------------------------------------------------------------------------------------ 1: a static table
def test_static_assignment_equals_the_twin_and_the_per_policy_fleets(fleet):
    env = _env(scenarios=fleet["scn"], curves=True)
    tab = _table(fleet["files"], env, rotate=None)
    words, n_groups, names = tab.curve_groups()
    assert tab.curve_groups()[0] is words and words.dtype == env.torch.int32 and (words.cpu().numpy() == tab.policy_of_env).all()   # created once
    env.set_curve_groups(tab)
    rec = _Loop(env, words)
    assert _runner(env, tab).test(max_steps=STEPS, before_step=rec.before, on_step=rec.after) == STEPS
    got, tw = env.curves(), rec.twin(env.scenario_table, names=NAMES)
    _contents(tw)
    _same(got, tw)
    assert got.group_names == NAMES
    for g, name in enumerate(NAMES):                                       # plane g: the ungrouped curves of the envs policy g drives
        _same(got.group(name), rec.twin(env.scenario_table, 0, envs=tab.policy_of_env == g), f"plane {g}: ")
    env.close()


# ------------------------------------------------------------------------------------------------------------ 2: rotation
def test_rotation_through_runner_test_equals_the_twin(fleet):
    """The planes equal the twin fed the ``policy_now`` recorded behind every step; merged, they are the cells of the same run armed
    without groups, and the states agree: curves do not touch the physics."""
    rec, got = fleet["rec"], fleet["got"]
    tw = rec.twin(fleet["table"], names=NAMES)
    _contents(tw, rec, rotating=True)
    _same(got, tw)
    np.testing.assert_array_equal(fleet["final"].view(np.int32), fleet["dry_final"].view(np.int32))
    env = _env(scenarios=fleet["scn"], curves=True)                        # the same run, no groups
    tab = _table(fleet["files"], env)
    assert _runner(env, tab).test(max_steps=STEPS) == STEPS
    flat = env.curves()
    assert flat.groups == 1 and not flat.grouped and env.engine.query("scenario_curve_groups") == 0
    _same(got.merged(), flat, "the planes merged: ")
    _same(flat, rec.twin(fleet["table"], 0), "without groups: ")
    for s, k in flat.items():                                              # two-index access reads the merged planes
        np.testing.assert_array_equal(got[s, k].both("count"), flat[s, k].both("count"))
    np.testing.assert_array_equal(env.state.cpu().numpy().view(np.int32), fleet["final"].view(np.int32))
    env.close()


# ------------------------------------------------------------------------------------------------------------ 3: the other drivers
@pytest.mark.parametrize("driver", ["graphed", "pipelined-4-deferred", "1-range", "2-uneven-ranges"])
def test_other_drivers_give_the_same_bits(fleet, driver):
    import torch
    kw = {"graphed": {}, "pipelined-4-deferred": {"ranges": 4, "deferred_join": True}, "1-range": {"ranges": 1}, "2-uneven-ranges": {}}[driver]
    env = _env(scenarios=fleet["scn"], curves=True, **kw)
    shards = [(0, 11), (11, 13)]
    tab = _table(fleet["files"], env, ranges=env.range_list if driver.startswith("pipelined") else (shards if driver.startswith("2") else None))
    env.set_curve_groups(tab)                                              # ahead of the capture
    run = _runner(env, tab)
    if driver == "graphed":
        assert run.test_graphed(STEPS) == STEPS
    elif driver.startswith("pipelined"):
        assert env.engine.query("ranges") == 4 and run.test_pipelined(STEPS) == STEPS
    elif driver == "1-range":
        assert env.engine.query("ranges") == 1 and run.test(max_steps=STEPS) == STEPS
    else:                                                                  # each shard's chain forward -> step on a stream of its own
        env.receive_user_command(run.user_command)
        env.reset()
        action = torch.zeros((env.num_envs, env.action_dim), dtype=torch.float32, device=env.device)
        streams = [torch.cuda.Stream(device=env.device) for _ in shards]
        torch.cuda.synchronize(env.device)
        for k in range(STEPS):
            order = list(zip(range(len(shards)), shards, streams))
            for i, (first, count), st in (order[::-1] if k % 2 else order):
                with torch.cuda.stream(st):
                    tab.get_action_range(i, env.state, action, done=(env.terminated, env.truncated))
                    env.step_range(first, count, action)
    env.join()
    torch.cuda.synchronize(env.device)
    _same(env.curves(), fleet["got"], driver + ": ")
    assert env.curve_groups_lost() == 0
    np.testing.assert_array_equal(env.state.cpu().numpy().view(np.int32), fleet["final"].view(np.int32))
    env.close()


# ------------------------------------------------------------------------------------------------------------ 4: recurrent
def test_recurrent_rotating_table_equals_the_twin(fleet):
    env = _env(scenarios=fleet["scn"], curves=True)
    tab = _table(fleet["rfiles"], env, recurrent=True)
    env.set_curve_groups(tab)
    rec = _Loop(env, tab.policy_now)
    assert _runner(env, tab).test(max_steps=STEPS, before_step=rec.before, on_step=rec.after) == STEPS
    got, tw = env.curves(), rec.twin(env.scenario_table, names=NAMES)
    _contents(tw, rec, rotating=True)
    _same(got, tw)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 5: the guard
def test_words_outside_the_groups_touch_no_plane(fleet):
    """A hand-made tensor with -1 on env 4 (scenario 0, 8 items) and G on env 7 (scenario 3, the push)."""
    import torch
    env = _env(scenarios=fleet["scn"], curves=True)
    w = np.arange(N, dtype=np.int32) % K
    w[4], w[7] = -1, K
    words = torch.tensor(w, device=env.device)
    with pytest.raises(ValueError, match="a group tensor needs n_groups"):
        env.set_curve_groups(words)
    env.set_curve_groups(words, K)
    acts = _actions(env)
    env.reset()
    rec = _Loop(env, words)
    rec.host(acts, 0, STEPS)
    got, tw = env.curves(), rec.twin(env.scenario_table)
    done = (rec.stacked("te") | rec.stacked("tr")) != 0
    lost = int(done[:, 4].sum() + done[:, 7].sum())
    assert lost >= 4 and tw.ungrouped == lost and env.curve_groups_lost() == lost and got.ungrouped == lost and got.group_names == ["0", "1", "2"]
    _same(got, tw)
    keep = np.ones(N, dtype=bool)
    keep[[4, 7]] = False
    _same(got.merged(), rec.twin(env.scenario_table, 0, envs=keep), "the planes hold the other envs' episodes and nothing else: ")
    assert all(p.summary()["episodes"] > 0 for p in got.by_group().values())
    env.clear_curves()                                                      # the count goes back to zero with the cells
    assert env.curve_groups_lost() == 0 and env.curves().summary()["samples"] == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------ 6, 7: the feature only reads
def test_everything_but_the_cells_is_byte_identical(fleet):
    """Curves armed: an env that never heard of groups, one whose groups were set and cleared again, one with groups set.  Cells (the
    first two; the third's planes merged), states, flags, info, ledger records and verdicts are the same bytes."""
    import torch
    from cosim_amd.checks import same_verdicts
    runs = {}
    for name in ("never", "cleared", "grouped"):
        env = _env(scenarios=fleet["scn"], curves=True, check_slots=2)
        words = torch.tensor(np.arange(N, dtype=np.int32) % K, device=env.device)
        if name != "never":
            env.set_curve_groups(words, K, names=NAMES)
        if name == "cleared":
            env.set_curve_groups(None)
        assert env.engine.query("scenario_curve_groups") == (K if name == "grouped" else 0)
        acts = _actions(env)
        env.reset()
        r = _Rec(env)
        r.run(acts, 0, STEPS)
        runs[name] = (r, env.ledger(include_open=True), env.verdicts(include_open=True), env.curves())
        env.close()
    a = runs["never"]
    assert len(a[2]) > 0 and a[3].summary()["episodes"] > 0
    for name in ("cleared", "grouped"):
        b = runs[name]
        for col in ("state", "info", "te", "tr", "cmd", "rows", "qpos", "qvel", "clock"):
            np.testing.assert_array_equal(b[0].stacked(col).view(np.uint8), a[0].stacked(col).view(np.uint8), err_msg=f"{name} {col}")
        np.testing.assert_array_equal(b[1].words, a[1].words)
        assert same_verdicts(b[2], a[2]) is None
    assert runs["cleared"][3].groups == 1 and runs["cleared"][3].cells.tobytes() == a[3].cells.tobytes()
    assert runs["grouped"][3].groups == K and runs["grouped"][3].ungrouped == 0
    _same(runs["grouped"][3].merged(), a[3], "the planes merged: ")


# ------------------------------------------------------------------------------------------------------------ 8: mid-run operations
def test_mid_run_operations_with_groups_set(fleet):
    """A masked reset() before step 20, clear_curves() before step 30, an in-place rewrite of lo / hi before step 36 (the groups
    survive), a re-allocation before step 46 (the groups are dropped); the group words change at step 10.  The time limit ends the
    fleet's episodes in steps 24 and 49, those of the envs reset before step 20 in step 44."""
    import torch
    env = _env(scenarios=fleet["scn"], curves=True)
    words = torch.tensor(np.arange(N, dtype=np.int32) % K, device=env.device)
    env.set_curve_groups(words, K, names=NAMES)
    acts = _actions(env)
    env.reset()
    rec = _Loop(env, words)
    rec.host(acts, 0, 10)
    words.copy_((words + 1) % K)                                           # the contents may change between steps; the pointer stays
    rec.host(acts, 10, 20)
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    env.reset(mask=mask)
    rec.begins.append((20, mask, 0))
    rec.host(acts, 20, 30)
    mid, tw = env.curves(), rec.twin(env.scenario_table, names=NAMES)
    assert tw.summary()["episodes"] > 0 and all(p.summary()["samples"] > 0 for p in tw.by_group().values())
    _same(mid, tw, "behind the masked reset: ")
    env.clear_curves()
    assert env.curves().summary()["samples"] == 0 and env.curves().groups == K and env.engine.query("scenario_curve_groups") == K
    rec.clears.append(30)
    rec.host(acts, 30, 36)
    _same(env.curves(), rec.twin(env.scenario_table, names=NAMES), "behind the clear: ")
    scn2 = copy.deepcopy(fleet["scn"])
    for sc in scn2:
        for it in sc.get("curves", []):
            m, half = 0.5 * (it[5] + it[6]), 0.25 * (it[6] - it[5])
            it[5], it[6] = float(np.float32(m - half)), float(np.float32(m + half))
    env.set_scenarios(scn2, curves=True)                                    # the same counts and sizes: in place
    assert env.engine.query("scenario_curve_groups") == K and env._curve_groups is not None and env.curves().summary()["samples"] == 0
    rec.host(acts, 36, 46)
    got, tw = env.curves(), rec.twin(env.scenario_table, names=NAMES, k0=36, k1=46)
    assert got.groups == K and got.group_names == NAMES and tw.summary()["episodes"] > 0 and tw.lohi[0, 0] != fleet["got"].lohi[0, 0]
    _same(got, tw, "behind the in-place rewrite: ")
    env.set_scenarios(fleet["scn"][:3], curves=True)                        # another S: the curves are reallocated, the groups dropped
    assert env.engine.query("scenario_curve_groups") == 0 and env._curve_groups is None and env.curve_groups_lost() == 0
    rec.host(acts, 46, STEPS)
    got = env.curves()
    assert got.groups == 1 and not got.grouped and got.cells.size == env.engine.query("scenario_curve_words") and got.summary()["episodes"] > 0
    _same(got, rec.twin(env.scenario_table, 0, k0=46), "behind the re-allocation: ")
    env.set_scenarios(fleet["scn"][:3])                                     # not armed
    with pytest.raises(ValueError, match=r"set_curve_groups\(\): no curves are armed"):
        env.set_curve_groups(words, K)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 9: C ABI refusals
def test_engine_refusals(fleet):
    import torch
    env = _env(scenarios=fleet["scn"], curves=True)
    words = torch.zeros(N, dtype=torch.int32, device=env.device)
    for bad in (-1, 65, 1000):
        with pytest.raises(ValueError, match=rf"cosim_scenario_curves_groups: n_groups {bad} outside 0\.\.64"):
            env.engine.scenario_curves_groups(bad, words.data_ptr())
    with pytest.raises(ValueError, match=r"cosim_scenario_curves_groups: n_groups 3 with a null group_dev"):
        env.engine.scenario_curves_groups(3, None)
    assert env.engine.query("scenario_curve_groups") == 0 and env.engine.query("scenario_curve_ungrouped") == 0
    env.engine.scenario_curves_groups(64, words.data_ptr())
    assert env.engine.query("scenario_curve_groups") == 64
    env.engine.scenario_curves_groups(0, None)
    assert env.engine.query("scenario_curve_groups") == 0
    env.set_scenarios(fleet["scn"])                                         # carried, not armed
    with pytest.raises(ValueError, match=r"cosim_scenario_curves_groups: no curves are set"):
        env.engine.scenario_curves_groups(3, words.data_ptr())
    env.close()
    # the design limit: one scenario of 8 items x 2 classes x 72 x 1024 words is 4.5 MiB a plane; 64 planes cross 256 MiB, 32 do not
    big = _env(n=4, scenarios=[{}], ledger=0)
    n = 8
    big.engine.scenario_curves_set((np.array([0, n], dtype=np.int32), np.tile(np.array([0, 1024, 1], dtype=np.int32), (n, 1)), np.zeros(n, np.int32),
                                    np.zeros(n, np.int32), np.zeros(n, np.float32), np.ones(n, np.float32), np.full(n, 64, np.int32)))
    W = big.engine.query("scenario_curve_words")
    assert W == 2 * n * 72 * 1024
    w4 = torch.zeros(4, dtype=torch.int32, device=big.device)
    with pytest.raises(ValueError, match=rf"cosim_scenario_curves_groups: 64 planes of {W} words: the cells would exceed 256 MiB"):
        big.engine.scenario_curves_groups(64, w4.data_ptr())
    assert big.engine.query("scenario_curve_groups") == 0
    big.engine.scenario_curves_groups(32, w4.data_ptr())
    assert big.engine.query("scenario_curve_groups") == 32
    big.close()


# ------------------------------------------------------------------------------------------------------------ 10: CLI
def _cli_args(tmp_path, files):
    yaml = pytest.importorskip("yaml")
    scn = tmp_path / "scn.yaml"
    scn.write_text(yaml.safe_dump({"scenarios": [{"curves": [[0, 25, 1, "torque_max", 0, 0.0, 1.0e9, 8, "torque"],
                                                             [0, 25, 5, "up", 0, -2.0, 2.0, 4, "upright"]]},
                                                 {"curves": [[0, 25, 1, "abs_info", "lin_vel_x", 0.0, 1.0e9, 0, "vx"]]}]}))
    return ["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy", *files,
            "--scenarios", str(scn), "--curves"]


@pytest.mark.parametrize("mode", ["", "--graph", "--pipelined"])
def test_cli_curves_by_policy(tmp_path, capsys, fleet, mode):
    from cosim_amd import cli
    from cosim_amd.curves import Curves
    out, rep = tmp_path / "c.npz", tmp_path / "report.json"
    argv = _cli_args(tmp_path, fleet["files"]) + ["--policy-rotate", "1", "--curves-by", "policy", "--curves-out", str(out), "--report", str(rep)]
    assert cli.main(argv + ([mode] if mode else [])) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    by = json.loads(rep.read_text())["episodes"]["curves"]["by_policy"]
    cv = Curves.load(str(out))
    assert cv.groups == K and cv.group_names == NAMES and cv.ungrouped == 0 and cv.names == [["torque", "upright"], ["vx"]]
    assert list(by) == NAMES and set(line["curves"]["by_policy"]) == set(NAMES)
    for name in NAMES:                                                      # 25-step episodes, 60 steps, 32 envs: 64 ended episodes over 3 policies
        assert by[name] == cv.group(name).summary() and by[name]["episodes"] >= 10
        assert line["curves"]["by_policy"][name]["episodes"] == by[name]["episodes"]
    assert sum(by[name]["episodes"] for name in NAMES) == line["curves"]["episodes"] >= 64


def test_cli_curves_by_policy_needs_a_table(tmp_path, capsys, fleet):
    from cosim_amd import cli
    with pytest.raises(SystemExit):
        cli.main(_cli_args(tmp_path, fleet["files"][:1]) + ["--curves-by", "policy"])
    assert "--curves-by policy needs a policy table: several --policy files" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(_cli_args(tmp_path, fleet["files"])[:-1] + ["--curves-by", "policy"])
    assert "--curves-by policy needs --curves" in capsys.readouterr().err
