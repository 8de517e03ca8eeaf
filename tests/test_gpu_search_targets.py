"""What the limit search gained over its first form, on the device: the level multiplied into MARKED parameter windows, observation
faults and action faults (scnparams_ / obsfault_ / actfault_search_step_kernel), ``harder`` up / down and a check verdict as a failure criterion (search_step_checks_kernel), through
the BatchedEnv surface, against the numpy twins (cosim_amd/scenario.py reference_action_faults(level=...), cosim_amd/search.py
SearchTwin) fed with the device's own flags, meta words and verdict masks.

Every comparison is EXACT: float32 bits for floats, ints as ints.  flamingo_light_v1 on the plane, max_duration = 0.5 (25-step
episodes), actions from a fixed table, 70 envs in 2 ranges (a tail in the last 64-lane block, a range boundary inside a wave), at most
150 steps.

The marked rows need no calibration: ``set_points[k]`` of the info row is the action the step kernel was handed times the
actuator's action scale, so with a marked ``["set", v]`` on actuator k over the whole episode and a check ``always < B`` (or ``> B``)
on ``set_points[k]`` the outcome of an episode is a known monotone function of its level, with the limit ``L* = B / (v * scale[k])``.
No fall rule is set there, so every episode runs its 25 steps and its check is complete.
  row 0  action faults, no search item: nothing is marked
  row 1  harder up:   marked set 0.5 on actuator 0, check set_points[0] < B1, L* = 1.1 inside [0.5, 2.0]; staircase from 1.25
  row 2  harder down: marked set 0.5 on actuator 1, check set_points[1] > B2, L* = 0.8 inside [0.25, 1.75]; beside it a marked drop,
         a marked bias, a marked noise and an unmarked scale and hold in the same row
The rows of the parameter-window and observation-fault tests (``_scenarios3``) are decided the same way, by a marked action-fault
``set`` and a check beside the marked windows / faults, so they too hold passes, failures and reversals without calibration.
The physics row (test 5) is the staircase of tests/test_gpu_search.py on the lateral push under the bounds that file calibrated
(tilt 0.45: no tilt failure at level 1, all at level 20), failing on tilt or on a check that an episode the tilt rule cut short leaves
incomplete.  Observed on the device (70 envs x 150 steps): see the docstring of that test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, RANGES, STEPS, SLOTS, CD = 70, 2, 150, 8, 4
BASE = np.array([0.3, 0.0, 0.1, 0.0], dtype=np.float32)
PUSH = [[2, 5, 0.0, 1.0, 0.0]]
V, L1, L2 = 0.5, 1.1, 0.8
_CACHE = {}


def _model():
    if "model" not in _CACHE:
        from cosim_amd.compile import compile_model
        from cosim_amd.config import make_config
        cfg = make_config("flamingo_light_v1", terrain="flat", random=None, max_duration=0.5)
        _CACHE["model"] = (cfg, compile_model(cfg))
    return _CACHE["model"]


def _scale():
    """The action scale of every actuator, float32 ``[nu]``."""
    from cosim_amd.model import get_field
    _, cm = _model()
    return np.asarray(get_field(cm.blob, "ctl_scale"), dtype=np.float32)[:4]


def _bounds():
    s = _scale()
    return float(np.float32(L1 * V * float(s[0]))), float(np.float32(L2 * V * float(s[1])))


def _scenarios(search=True):
    B1, B2 = _bounds()
    row0 = {"commands": [[0, 0.2, 0.0, 0.0, 0.0]], "action_faults": [[0, 25, 0, "set", V], [3, 9, "*", "drop", 0.3]]}
    row1 = {"action_faults": [[0, 25, 0, "set", V]], "checks": [[0, 25, "info", "set_points[0]", "always", "<", B1, "bound"]]}
    row2 = {"action_faults": [[0, 25, 1, "set", V],                  # 0 marked: decides the outcome
                              [2, 20, "*", "drop", 0.3],             # 1 marked: the probability is 0.3 * level
                              [0, 25, 2, "bias", 0.1],               # 2 marked
                              [0, 25, 3, "scale", 0.5],              # 3 NOT marked, in the same row
                              [5, 12, 3, "noise", 0.2],              # 4 marked
                              [14, 18, 2, "hold", 0.0]],             # 5 never marked
            "checks": [[0, 25, "info", "set_points[0]", "mean", "<", 1e6, "never"],
                       [0, 25, "info", "set_points[1]", "always", ">", B2, "bound"]]}
    if search:
        row1["search"] = {"lo": 0.5, "hi": 2.0, "rule": "staircase", "trials": 1000, "targets": ["action_faults"], "fail_on": ["check:bound"]}
        row2["search"] = {"lo": 0.25, "hi": 1.75, "rule": "staircase", "trials": 1000, "targets": ["action_faults:0,1,2,4"],
                          "fail_on": ["check:1"], "harder": "down"}
    return [row0, row1, row2]


def _env(n=N, **kw):
    from cosim_amd.batched_env import BatchedEnv
    cfg, cm = _model()
    kw.setdefault("auto_reset", True)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=3, **kw)
    assert env.command_dim == CD
    env.receive_user_command(BASE)
    return env


def _actions():
    if "actions" not in _CACHE:
        import torch
        a = np.random.default_rng(11).uniform(-0.6, 0.6, size=(160, N, 4)).astype(np.float32)
        _CACHE["actions"] = a
        _CACHE["actions_dev"] = torch.tensor(a, device="cuda:0")
    return _CACHE["actions_dev"]


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().copy()


def _rows(scn, n=N):
    from cosim_amd.scenario import ScenarioTable
    from cosim_amd.search import search_rows
    return search_rows(ScenarioTable(scn, CD), "env", np.arange(n))


def _masks(verdicts):
    """(env, episode) -> (fail mask, incomplete mask) of the ended episodes a ``Verdicts`` holds."""
    w = verdicts.words
    u = lambda lo, hi: (w[:, lo].astype(np.int64) & 0xFFFFFFFF) | ((w[:, hi].astype(np.int64) & 0xFFFFFFFF) << 32)   # noqa: E731
    f, i = u(4, 5), u(6, 7)
    return {(int(e), int(o)): (int(a), int(b)) for e, o, a, b, fl in zip(verdicts.env, verdicts.episode, f, i, verdicts.flags) if not fl & 16}


def _run(env, steps=STEPS, pre=None):
    """An eager run recorded step by step: before every step the levels and the pre-step meta words, behind it the effective action,
    the outputs and the post-step meta words."""
    t, acts = env.torch, _actions()
    out = {k: [] for k in ("levels", "pre", "eff", "state", "info", "te", "tr", "meta")}
    for k in range(steps):
        if env.search_slots:
            out["levels"].append(env.search_levels().cpu().numpy().copy())
        out["pre"].append(_meta(env))
        env.step(acts[k][:env.num_envs])
        env.join()
        t.cuda.synchronize(env.device)
        eff = env.effective_action()
        out["eff"].append(None if eff is None else eff.cpu().numpy().copy())
        out["state"].append(env.state.cpu().numpy().copy()); out["info"].append(env.info_buf.cpu().numpy().copy())
        out["te"].append(env.terminated.cpu().numpy().copy()); out["tr"].append(env.truncated.cpu().numpy().copy())
        out["meta"].append(_meta(env))
    if env.search_slots:
        out["levels"].append(env.search_levels().cpu().numpy().copy())
    return out


def _twin_run(table, rows, run, masks, fall, slots=SLOTS):
    """SearchTwin over a recorded run, fed with the device's own flags, meta words and verdict masks; the levels before every step."""
    from cosim_amd import search as sr
    twin = sr.SearchTwin(table, slots, rows, fall=fall, flag=0, meta4=run["pre"][0][:, 4])
    levels, episode = [], np.zeros(len(rows), dtype=np.int64)
    for k in range(len(run["te"])):
        levels.append(twin.levels())
        ended = (run["te"][k] != 0) | (run["tr"][k] != 0)
        f, i = np.zeros(len(rows), dtype=np.uint64), np.zeros(len(rows), dtype=np.uint64)
        for e in np.nonzero(ended)[0]:
            if (int(e), int(episode[e])) in masks:
                f[e], i[e] = masks[(int(e), int(episode[e]))]
        twin.step(run["te"][k], run["tr"][k], run["meta"][k][:, 4], run["meta"][k][:, 15], f, i)
        episode += ended
    levels.append(twin.levels())
    return twin, levels


def _reference():
    """The eager device run the tests share, never modified: 70 envs in 2 ranges, the three scenarios with the search and the checks
    armed, no fall rule, 150 steps."""
    if "reference" not in _CACHE:
        env = _env(ranges=RANGES, scenarios=_scenarios(), search=SLOTS, check_slots=SLOTS)
        q = env.engine.query
        assert q("ranges") == RANGES and q("search") == 2 and q("search_targets") == 16 and q("search_checks") == 1
        assert q("action_faults_marked") == 1 + (1 + 4 + 1 + 1)       # row 1: the set; row 2: set, "*" drop (4 actuators), bias, noise
        env.reset()
        run = _run(env)
        run["result"], run["verdicts"] = env.search(), env.verdicts()
        run["table"] = env.scenario_table
        env.close()
        _CACHE["reference"] = run
    return _CACHE["reference"]


# ------------------------------------------------------------------------------------------------------------ 2 + 4: action faults, end to end
def test_marked_action_faults_equal_the_twin_at_every_step():
    """``effective_action()`` behind every step equals ``reference_action_faults(level=...)`` at the levels ``search_levels()`` gave
    before it -- the marked drop included --, the levels equal SearchTwin's at every step, and ``set_points`` is the effective action
    times the action scale."""
    from cosim_amd.scenario import reference_action_faults
    a = _reference()
    T, rows, gid = a["table"], _rows(_scenarios()), np.arange(N)
    twin, levels = _twin_run(T, rows, a, _masks(a["verdicts"]), fall=False)
    acts, s = _CACHE["actions"], _scale()
    prev = np.zeros((N, 4), dtype=np.float32)
    differs = dropped = 0
    for k in range(STEPS):
        np.testing.assert_array_equal(a["levels"][k].view(np.uint32), levels[k].view(np.uint32), err_msg=f"search_levels() before step {k}")
        pre = a["pre"][k]
        prev[pre[:, 0] == 0] = 0.0                                   # the step before ended the episode: the record's last action is zeros
        want = reference_action_faults(T, "env", gid, pre[:, 0], pre[:, 11], pre[:, 1], 3, acts[k], prev, level=a["levels"][k])
        plain = reference_action_faults(T, "env", gid, pre[:, 0], pre[:, 11], pre[:, 1], 3, acts[k], prev)
        assert np.array_equal(a["eff"][k].view(np.uint32), want.view(np.uint32)), f"effective action differs in step {k}: envs {np.nonzero((a['eff'][k] != want).any(axis=1))[0][:8]}"
        np.testing.assert_array_equal(a["eff"][k][rows == 0].view(np.uint32), plain[rows == 0].view(np.uint32))
        differs += int((want != plain).any(axis=1).sum())
        held = (rows == 2) & (pre[:, 0] >= 2) & (pre[:, 0] < 20) & (want[:, 0] == prev[:, 0]) & (prev[:, 0] != acts[k][:, 0])
        dropped += int(held.sum())
        sp = a["info"][k][:, 4 + 4:4 + 8]
        np.testing.assert_array_equal(sp.view(np.uint32), (want * s[None, :]).astype(np.float32).view(np.uint32))
        prev = want
    np.testing.assert_array_equal(a["levels"][STEPS].view(np.uint32), levels[STEPS].view(np.uint32))
    assert differs > 10 * N and dropped > N                          # the level changed what was applied; marked drops fired


def test_physics_free_rows_bracket_the_known_limit():
    """Rows 1 and 2: the records and rings equal the twin's, every env's bracket contains L*, trial flag 2048 is set exactly on the
    failed trials, and each row holds counted passes, counted failures and reversals -- for harder up and down."""
    from cosim_amd import search as sr
    a = _reference()
    T, rows = a["table"], _rows(_scenarios())
    twin, _ = _twin_run(T, rows, a, _masks(a["verdicts"]), fall=False)
    r = a["result"]
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows, table=T)
    assert sr.same_search(r, want) is None, sr.same_search(r, want)
    assert r.harder.tolist() == [int(x == 2) for x in rows] and r.by_scenario()[2]["harder"] == "down"
    assert r.by_scenario()[2]["targets"] == ["action_faults:0,1,2,4"] and r.by_scenario()[1]["fail_on"] == ["check:bound"]
    assert np.array_equal((r.flags & sr.BY_CHECK) != 0, r.counted & r.failed)
    trow = rows[r.trial_env]
    for row, limit in ((1, L1), (2, L2)):
        m = rows == row
        assert (r.trials[m] == 6).all() and not r.done[m].any()      # six 25-step episodes, every one a counted trial
        assert (r.fails[m] > 0).all() and (r.fails[m] < r.trials[m]).all() and (r.reversals[m] >= 2).all()
        lo_end, hi_end = np.minimum(r.bracket[m, 0], r.bracket[m, 1]), np.maximum(r.bracket[m, 0], r.bracket[m, 1])
        assert (lo_end < limit).all() and (limit < hi_end).all() and (hi_end - lo_end < 0.2).all()
        passed_below = r.bracket[m, 0] < r.bracket[m, 1]             # harder up: the highest pass lies below the lowest failure
        assert passed_below.all() if row == 1 else (~passed_below).all()
        t = trow == row
        assert (r.counted & r.failed & t).any() and (r.counted & ~r.failed & t).any() and (r.reversal & t).any()
        # the outcome is the known function of the level
        assert np.array_equal(r.failed[t], (r.trial_level[t] > limit) if row == 1 else (r.trial_level[t] < limit))
        assert (np.abs(r.threshold[m] - limit) < 0.1).all()
    assert not r.has_item[rows == 0].any()


# ------------------------------------------------------------------------------------------------------------ 1 + 3: parameter windows, observation faults
def _scenarios3(params=True, faults=True, obs_target=True):
    """Row 0: windows and faults, no item.  Row 1: marked windows (the friction scale of every geom is the level itself, kd of
    actuator 1 scaled by 1.2 * level) beside an unmarked one, harder down.  Row 2: marked observation faults (a gyro bias that touches
    clock 0, a drop on the joint velocities) beside an unmarked one, harder up.  Rows 1 and 2 are decided by a marked action-fault set
    and a check, as in ``_scenarios``.  ``obs_target=False`` keeps row 2's faults and takes them out of its search's targets: no
    observation fault is marked then."""
    B1, B2 = _bounds()
    P = [[0, 25, "geom_friction", "*", "scale", 1.0], [0, 25, "kd", 1, "scale", 1.2], [3, 20, "kp", 0, "scale", 0.9]]
    F = [[0, 25, "ang_vel", "*", "bias", 0.05], [2, 20, "dof_vel", "*", "drop", 0.2], [0, 25, "dof_pos", 0, "scale", 1.1]]
    row0 = {"commands": [[0, 0.2, 0.0, 0.0, 0.0]], "params": P, "faults": F}
    row1 = {"params": P, "action_faults": [[0, 25, 1, "set", V]], "checks": [[0, 25, "info", "set_points[1]", "always", ">", B2, "bound"]],
            "search": {"lo": 0.25, "hi": 1.75, "rule": "staircase", "trials": 1000, "targets": ["params:0,1", "action_faults"], "fail_on": ["check:bound"],
                       "harder": "down"}}
    row2 = {"faults": F, "action_faults": [[0, 25, 0, "set", V]], "checks": [[0, 25, "info", "set_points[0]", "always", "<", B1, "bound"]],
            "search": {"lo": 0.5, "hi": 2.0, "rule": "staircase", "trials": 1000, "targets": ["faults:0,1", "action_faults"], "fail_on": ["check:bound"]}}
    if not params:
        for r in (row0, row1):
            del r["params"]
        row1["search"]["targets"] = ["action_faults"]
    if not faults:
        for r in (row0, row2):
            del r["faults"]
        row2["search"]["targets"] = ["action_faults"]
    if not obs_target:
        row2["search"]["targets"] = ["action_faults"]
    return [row0, row1, row2]


def _run3(params=True, faults=True, drive=None, obs_target=True, steps=STEPS):
    """``steps`` (150) eager steps of ``_scenarios3`` with the search and the checks armed and a history ring; ``drive(env, k)`` runs
    before step k (and with k = -1 before the reset)."""
    from cosim_amd.scenario import fault_layout
    env = _env(ranges=RANGES, scenarios=_scenarios3(params, faults, obs_target), search=SLOTS, check_slots=SLOTS, history=(2, 1))
    q = env.engine.query
    marks_obs = faults and obs_target
    assert q("search_targets") == 16 | (4 if params else 0) | (8 if marks_obs else 0)
    assert (q("scenario_param_items_marked") > 0) == params and (q("obs_faults_marked") > 0) == marks_obs and (q("obs_faults") > 0) == faults
    queries = {name: q(name) for name in ("search", "search_targets", "obs_faults", "obs_faults_marked")}
    if drive:
        drive(env, -1)
    env.reset()
    env.join()
    env.torch.cuda.synchronize(env.device)
    obs0, meta0 = env.state.cpu().numpy().copy(), _meta(env)
    run = {k: [] for k in ("levels", "pre", "eff", "state", "info", "te", "tr", "meta", "par")}
    acts = _actions()
    for k in range(steps):
        run["levels"].append(env.search_levels().cpu().numpy().copy())
        run["pre"].append(_meta(env))
        if drive:
            drive(env, k)
        env.step(acts[k])
        env.join()
        env.torch.cuda.synchronize(env.device)
        run["par"].append(env.effective_params().copy())
        run["state"].append(env.state.cpu().numpy().copy()); run["info"].append(env.info_buf.cpu().numpy().copy())
        run["te"].append(env.terminated.cpu().numpy().copy()); run["tr"].append(env.truncated.cpu().numpy().copy())
        run["meta"].append(_meta(env))
        if k in (24, 60):                                            # behind a step that ended every episode, and one in mid-episode
            h, sn = env.history(0), env.snapshot()
            assert h.steps_ago == 0
            np.testing.assert_array_equal(h.rows.cpu().numpy().view(np.uint32), sn.rows.cpu().numpy().view(np.uint32),
                                          err_msg="the history ring's capture is the state the step left, faults applied")
    run["levels"].append(env.search_levels().cpu().numpy().copy())
    run.update(obs0=obs0, meta0=meta0, queries=queries, result=env.search(), verdicts=env.verdicts(), table=env.scenario_table, rows=env.snapshot().rows.cpu().numpy().copy(),
               lay=env.param_layout(), flay=fault_layout(env.fault_names()))
    env.close()
    return run


def _reference3():
    if "reference3" not in _CACHE:
        _CACHE["reference3"] = _run3()
    return _CACHE["reference3"]


def _clean3():
    """``_scenarios3`` without observation faults, never modified: the frames the observation-fault twins are fed with."""
    if "clean3" not in _CACHE:
        _CACHE["clean3"] = _run3(faults=False)
    return _CACHE["clean3"]


def _both_ways(r, rows, row):
    """Test 6: the recorded run of a searched row holds counted passes, counted failures and reversals."""
    t = rows[r.trial_env] == row
    assert (r.counted & r.failed & t).any() and (r.counted & ~r.failed & t).any() and (r.reversal & t).any()
    assert (r.fails[rows == row] > 0).all() and (r.fails[rows == row] < r.trials[rows == row]).all() and (r.reversals[rows == row] > 0).all()


def test_marked_params_equal_a_host_driven_fleet():
    """Fleet A carries marked windows (harder down) beside an unmarked one.  Fleet B has no windows: before every step (and the
    reset) the host gives it, through set_param, the records ``reference_params(level=B's own levels)`` works out.  ``effective_params()``
    of A equals the twin at SearchTwin's levels at every step, and every word of state, info, flags, levels and the final records
    of A and B agree."""
    from cosim_amd import search as sr
    from cosim_amd.scenario import reference_params
    a = _reference3()
    T, rows, gid = a["table"], _rows(_scenarios3()), np.arange(N)
    twin, levels = _twin_run(T, rows, a, _masks(a["verdicts"]), fall=False)
    lay = a["lay"]
    width = {"kp": 4, "kd": 4}
    state = {}

    def drive(env, k):
        if "base" not in state:
            state["base"] = env.effective_params().copy()           # no windows: the base records
            q = env.engine.query
            width.update(geom_friction=q("ngeom"), dof_frictionloss=q("nv"))
        meta = _meta(env)
        t = np.zeros(N, dtype=np.int64) if k < 0 else meta[:, 0]
        eff = reference_params(T, "env", gid, t, meta[:, 11], state["base"], lay, level=env.search_levels().cpu().numpy())
        for f, w in width.items():
            env.engine.set_param(f, np.ascontiguousarray(eff[:, lay[f]:lay[f] + w]))
        state.setdefault("eff", []).append(eff)
    b = _run3(params=False, drive=drive)
    base = state["base"]
    changed = 0
    for k in range(STEPS):
        np.testing.assert_array_equal(a["levels"][k].view(np.uint32), levels[k].view(np.uint32), err_msg=f"search_levels() before step {k}")
        np.testing.assert_array_equal(b["levels"][k].view(np.uint32), levels[k].view(np.uint32))
        pre = a["pre"][k]
        want = reference_params(T, "env", gid, pre[:, 0], pre[:, 11], base, lay, level=levels[k])
        assert np.array_equal(a["par"][k].view(np.uint32), want.view(np.uint32)), f"effective_params differ in step {k}"
        plain = reference_params(T, "env", gid, pre[:, 0], pre[:, 11], base, lay)
        np.testing.assert_array_equal(want[rows != 1].view(np.uint32), plain[rows != 1].view(np.uint32))
        changed += int((want != plain).any(axis=1).sum())
        for name in ("state", "info", "te", "tr"):
            x, y = a[name][k], b[name][k]
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), f"{name} differs in step {k}"
    S = a["rows"].shape[1] - base.shape[1]
    np.testing.assert_array_equal(a["rows"][:, :S].view(np.uint32), b["rows"][:, :S].view(np.uint32))
    assert changed > 5 * N
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows, table=T)
    assert sr.same_search(a["result"], want) is None, sr.same_search(a["result"], want)
    _both_ways(a["result"], rows, 1)
    assert a["result"].by_scenario()[1]["harder"] == "down"


def test_marked_obs_faults_equal_the_twin_and_take_the_new_level():
    """Every word of ``state`` of every observation equals ``reference_obs_faults(level=...)`` fed with the frames of a fleet without
    faults, the level of observation k being the one the search holds BEHIND step k - 1.  On a step that ended a counted trial and
    moved the level the returned observation (clock 0 of the next episode) carries the NEW level."""
    from cosim_amd import search as sr
    from cosim_amd.scenario import reference_obs_faults
    a = _reference3()
    c = _clean3()
    T, rows, gid = a["table"], _rows(_scenarios3()), np.arange(N)
    twin, levels = _twin_run(T, rows, a, _masks(a["verdicts"]), fall=False)
    lay = a["flay"]
    sd, S_ = lay["stacked_dim"], lay["stack_size"]
    frames = lambda st: np.concatenate([st[..., :sd], st[..., S_ * sd:]], axis=-1)   # noqa: E731
    meta = np.stack([a["meta0"]] + a["meta"])
    clean = np.stack([c["obs0"]] + c["state"])
    got = np.stack([a["obs0"]] + a["state"])
    level = np.stack(levels)                                         # [STEPS + 1, N]: observation k belongs to the episode that runs at levels[k]
    for k in range(STEPS + 1):
        np.testing.assert_array_equal(a["levels"][k].view(np.uint32), level[k].view(np.uint32))
    want = reference_obs_faults(T, "env", gid, meta[:, :, 0], meta[:, :, 11], meta[:, :, 1], 3, frames(clean), lay, level=level)
    for k in range(STEPS + 1):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), f"observation {k} differs: envs {np.nonzero((got[k] != want[k]).any(axis=1))[0][:8]}"
    plain = reference_obs_faults(T, "env", gid, meta[:, :, 0], meta[:, :, 11], meta[:, :, 1], 3, frames(clean), lay)
    np.testing.assert_array_equal(want[:, rows != 2].view(np.uint32), plain[:, rows != 2].view(np.uint32))
    assert (want[:, rows == 2] != plain[:, rows == 2]).any()
    # the new level: observation k + 1 (returned by step k) where step k ended a counted trial and the level moved
    e = int(T.faults[2][0][2])                                       # the first gyro element: under the marked bias alone
    seen = 0
    for k in range(STEPS):
        moved = (rows == 2) & (level[k + 1] != level[k])
        if not moved.any():
            continue
        assert (meta[k + 1][moved, 0] == 0).all() and ((a["te"][k] | a["tr"][k]) != 0)[moved].all()
        x = frames(clean[k + 1])[moved, e]
        new = (x + (np.float32(0.05) * level[k + 1][moved]).astype(np.float32)).astype(np.float32)
        old = (x + (np.float32(0.05) * level[k][moved]).astype(np.float32)).astype(np.float32)
        np.testing.assert_array_equal(got[k + 1][moved, e].view(np.uint32), new.view(np.uint32))
        assert (got[k + 1][moved, e] != old).all()
        seen += int(moved.sum())
    assert seen > 3 * int((rows == 2).sum())
    want_r = sr.SearchResult.from_raw(twin.state, twin.ring, rows, table=T)
    assert sr.same_search(a["result"], want_r) is None
    _both_ways(a["result"], rows, 2)
    # physics is the clean fleet's: the faults touch the observation alone
    for k in range(STEPS):
        assert np.array_equal(a["info"][k].view(np.uint32), c["info"][k].view(np.uint32)), f"info differs in step {k}"


def test_obs_fault_launch_order_is_unchanged_without_a_faults_target():
    """Test 8, the plain launch order (the observation-fault kernel ahead of the observers), which every caller without a ``faults``
    target is on.  The fleet of ``_scenarios3`` with its observation faults kept and row 2's search naming ``action_faults`` alone: no
    observation fault is marked (``search_targets & 8 == 0``, ``obs_faults_marked == 0``), the history ring's capture behind a step
    that ended every episode and behind one in mid-episode equals a snapshot -- the faulted state --, and every observation equals
    ``reference_obs_faults`` WITHOUT a level fed with the clean fleet's frames, although the search's levels are never 1 there.  Then
    the same faults with the search item carried but not armed: the capture is the faulted state there too."""
    from cosim_amd.scenario import reference_obs_faults
    steps = 61                                                       # _run3 compares the capture with a snapshot behind steps 24 and 60
    d = _run3(obs_target=False, steps=steps)
    qd = d["queries"]
    assert qd["search"] > 0 and qd["search_targets"] & 8 == 0 and qd["obs_faults_marked"] == 0 and qd["obs_faults"] > 0
    c = _clean3()
    T, rows, gid = d["table"], _rows(_scenarios3(obs_target=False)), np.arange(N)
    lay = d["flay"]
    sd, S_ = lay["stacked_dim"], lay["stack_size"]
    frames = lambda st: np.concatenate([st[..., :sd], st[..., S_ * sd:]], axis=-1)   # noqa: E731
    meta = np.stack([d["meta0"]] + d["meta"])
    clean = np.stack([c["obs0"]] + c["state"][:steps])
    got = np.stack([d["obs0"]] + d["state"])
    level = np.stack(d["levels"])
    for k in range(steps):                                           # the same physics and the same staircase as the clean fleet's
        np.testing.assert_array_equal(d["levels"][k].view(np.uint32), c["levels"][k].view(np.uint32))
        assert np.array_equal(d["info"][k].view(np.uint32), c["info"][k].view(np.uint32)), f"info differs in step {k}"
    args = (T, "env", gid, meta[:, :, 0], meta[:, :, 11], meta[:, :, 1], 3, frames(clean), lay)
    want = reference_obs_faults(*args)
    for k in range(steps + 1):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), f"observation {k} differs: envs {np.nonzero((got[k] != want[k]).any(axis=1))[0][:8]}"
    scaled = reference_obs_faults(_reference3()["table"], *args[1:], level=level)   # what the table with "faults:0,1" marked gives: the levels would show
    assert (scaled[:, rows == 2] != want[:, rows == 2]).any() and (want[:, rows == 2] != got[:, rows == 2]).sum() == 0
    # no search armed at all: the item is carried, the faults act, the capture holds them
    env = _env(ranges=RANGES, scenarios=_scenarios3(), history=(2, 1))
    q = env.engine.query
    assert q("search") == 0 and q("search_targets") == 0 and q("obs_faults_marked") == 0 and q("obs_faults") > 0
    env.reset()
    acts = _actions()
    for k in range(27):
        env.step(acts[k])
        if k in (24, 26):
            env.join()
            h, sn = env.history(0), env.snapshot()
            assert h.steps_ago == 0
            np.testing.assert_array_equal(h.rows.cpu().numpy().view(np.uint32), sn.rows.cpu().numpy().view(np.uint32))
    state, t0 = env.state.cpu().numpy().copy(), _meta(env)[:, 0]
    env.close()
    assert (t0 == 2).all()
    e = int(T.faults[0][0][2])                                       # the first gyro element of row 0: under the bias of 0.05
    plain = frames(c["state"][26])[:, e]                             # row 0 carries no search item: the clean fleet's row 0 is this fleet's
    np.testing.assert_array_equal(frames(state)[rows == 0, e].view(np.uint32), (plain[rows == 0] + np.float32(0.05)).astype(np.float32).view(np.uint32))


def test_a_refusal_part_way_through_set_scenarios_puts_the_marks_back(monkeypatch):
    """``set_scenarios`` unmarks the armed search's items before it sends the next table.  Where the engine then refuses that table
    the earlier table and its search still stand, and its items get their marks back; where that is refused too, the exception that
    leaves says which items the armed search no longer scales."""
    scn = _scenarios()
    env = _env(scenarios=scn, search=SLOTS, check_slots=SLOTS)
    q = env.engine.query
    assert q("action_faults_marked") == 8 and env._search_marked == ("action_faults",)
    old = env.scenario_table

    def refuse(*a, **kw):
        raise ValueError("cosim_scenario_set: refused for the test")
    monkeypatch.setattr(env.engine, "scenario_set", refuse)
    with pytest.raises(ValueError, match="refused for the test") as info:
        env.set_scenarios(scn, search=SLOTS, check_slots=SLOTS)
    assert "could not be put back" not in str(info.value)
    assert env.scenario_table is old and env._search_marked == ("action_faults",) and env.search_slots == SLOTS
    assert q("search") == 2 and q("search_targets") == 16 and q("action_faults_marked") == 8
    # the restore itself refused: the unmarking call passes, the one that would mark again does not
    send, calls = env._send_items, []

    def send_once(table, key, marks):
        calls.append(marks)
        if marks:
            raise ValueError('cosim_set_param "action_faults": refused for the test')
        send(table, key, marks)
    monkeypatch.setattr(env, "_send_items", send_once)
    with pytest.raises(ValueError, match="cosim_scenario_set: refused for the test") as info:
        env.set_scenarios(scn, search=SLOTS, check_slots=SLOTS)
    assert calls == [False, True]
    assert "marks of its action_faults items could not be put back" in str(info.value) and 'action_faults": refused for the test' in str(info.value)
    assert env.scenario_table is old and env._search_marked == () and q("search") == 2 and q("action_faults_marked") == 0
    monkeypatch.undo()
    env.set_scenarios(scn, search=SLOTS, check_slots=SLOTS)          # "until set_scenarios is called again"
    assert q("action_faults_marked") == 8 and env._search_marked == ("action_faults",)
    env.close()


def test_checks_armed_before_the_search_name_their_own_slot():
    """The checks run 30 steps (one ended episode) before the search is armed: the checks' episode ordinal is then one ahead of the
    search's, and the verdict a trial is judged by is the one of the checks' own ordinal."""
    from cosim_amd import search as sr
    scn = _scenarios()
    env = _env(ranges=RANGES, scenarios=scn, check_slots=SLOTS)
    env.reset()
    acts = _actions()
    for k in range(30):
        env.step(acts[k])
    env.set_scenarios(scn, search=SLOTS, check_slots=SLOTS)          # the checks are rewritten in place: their counters stay
    ver0 = env.verdicts()
    assert (np.bincount(ver0.env, minlength=N) == 1).all()
    env.reset()
    run = _run(env, steps=100)
    got, ver = env.search(), env.verdicts()
    T = env.scenario_table
    env.close()
    masks = {(e, o - 1): m for (e, o), m in _masks(ver).items() if o >= 1}      # the search's ordinal is the checks' minus one
    rows = _rows(scn)
    twin, _ = _twin_run(T, rows, run, masks, fall=False)
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows, table=T)
    assert sr.same_search(got, want) is None, sr.same_search(got, want)
    assert (got.trials[rows != 0] == 4).all() and (got.fails[rows != 0] > 0).all() and (got.fails[rows != 0] < 4).all()
    assert (ver.episode.max() == got.episode.max() + 1)


# ------------------------------------------------------------------------------------------------------------ 5: a check beside a fall flag
def test_check_criterion_beside_a_fall_flag_on_physics():
    """A staircase on the lateral push, failing on tilt or on the check "upright": up > 0.7 settled over [5, 24), which an episode the
    tilt rule cut short leaves incomplete.  The records equal SearchTwin fed with the device's own flags and ``env.verdicts()`` masks; the
    row holds counted passes, counted failures and reversals.
    Observed on the device, 70 envs x 150 steps, tilt 0.45, lo 1, hi 20, first step 12 from 10.5: share of the counted trials in the
    rings that failed, per level: 1.0, 1.75, 2.25: 0.00; 2.5: 0.26; 3.0: 1.00; 3.25: 0.78; 4.0: 0.61; 4.5: 1.00; 4.75: 0.94; 5.25: 1.00;
    5.5: 0.86; 6.25: 1.00; 7.0: 0.95; 10.0, 10.5, 13.0: 1.00 -- the calibration of tests/test_gpu_search.py (none at 1, all at 20)
    holds with the check beside the tilt flag; every env of the row has counted passes, counted failures and a reversal."""
    from cosim_amd import search as sr
    from cosim_amd.fall import FallRule
    scn = [{"commands": [[0, 0.2, 0.0, 0.0, 0.0]], "pushes": PUSH},
           {"pushes": PUSH, "checks": [[5, 24, "up", 0, "settle", ">", 0.7, "upright"]],
            "search": {"lo": 1.0, "hi": 20.0, "rule": "staircase", "trials": 1000, "step": 12.0, "min_step": 0.5, "targets": ["pushes"],
                       "fail_on": ["tilt", "check:upright"], "rev_skip": 1}}]
    env = _env(ranges=RANGES, scenarios=scn, search=SLOTS, check_slots=64, fall=FallRule(tilt=0.45, grace=0))
    assert env.engine.query("search_checks") == 1 and env.engine.query("search_targets") == 1
    env.reset()
    run = _run(env)
    got, ver = env.search(), env.verdicts()
    T = env.scenario_table
    env.close()
    assert (ver.lost == 0).all()                                     # every ended episode's verdict is still in the ring
    rows = _rows(scn)
    twin, levels = _twin_run(T, rows, run, _masks(ver), fall=True)
    for k in range(STEPS + 1):
        np.testing.assert_array_equal(run["levels"][k].view(np.uint32), levels[k].view(np.uint32), err_msg=f"search_levels() at step {k}")
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows, table=T)
    assert sr.same_search(got, want) is None, sr.same_search(got, want)
    one = rows == 1
    t = rows[got.trial_env] == 1
    print("physics row: fail share per level", {float(lv): float(got.failed[t & got.counted & (got.trial_level == lv)].mean())
                                                for lv in np.unique(got.trial_level[t & got.counted])})
    assert (got.fails[one] > 0).all() and (got.fails[one] < got.trials[one]).all() and (got.reversals[one] > 0).all()
    by_check = (got.flags & sr.BY_CHECK) != 0
    short = t & got.counted & (got.length < 24)                      # cut short by the tilt rule: the window [5, 24) is incomplete
    assert short.any() and by_check[short].all() and ((got.flags[short] & 32) != 0).all()
    assert not by_check[~t].any() and not by_check[~got.counted].any()


# ------------------------------------------------------------------------------------------------------------ 7: graph and pipelined
def test_graphed_and_pipelined_loops_give_the_eager_records(tmp_path):
    import torch
    from cosim_amd import search as sr
    from cosim_amd.policy import MLPPolicy, write_random_mlp
    from cosim_amd.runner import Runner
    f = str(tmp_path / "actor.onnx")
    outs = {}
    for kind in ("eager", "graphed", "pipelined"):
        env = _env(scenarios=_scenarios3(), search=SLOTS, check_slots=SLOTS, **({"ranges": 4, "deferred_join": True} if kind == "pipelined" else {"ranges": RANGES}))
        if kind == "eager":
            write_random_mlp(f, env.state_dim, env.action_dim, hidden=(64, 64), seed=31)
        run = Runner(env, MLPPolicy(f, device=env.device, fused=True))
        run.update_command(0, 0.3)
        steps = 80
        done = run.test(max_steps=steps) if kind == "eager" else run.test_graphed(steps) if kind == "graphed" else run.test_pipelined(steps)
        assert done == steps
        env.join()
        torch.cuda.synchronize()
        q = env.engine.query
        assert q("search_targets") == 4 | 8 | 16 and q("scenario_param_items_marked") > 0 and q("obs_faults_marked") > 0 and q("action_faults_marked") > 0
        outs[kind] = (env.search(), env.state.cpu().numpy().copy(), env.effective_action().cpu().numpy().copy(), env.effective_params().copy())
        env.close()
    e = outs["eager"]
    assert (e[0].trials[e[0].has_item] == 3).all() and (e[0].fails > 0).any() and (e[0].reversals > 0).any()
    for kind in ("graphed", "pipelined"):
        assert sr.same_search(outs[kind][0], e[0]) is None, (kind, sr.same_search(outs[kind][0], e[0]))
        np.testing.assert_array_equal(outs[kind][1].view(np.uint32), e[1].view(np.uint32))
        np.testing.assert_array_equal(outs[kind][2].view(np.uint32), e[2].view(np.uint32))
        np.testing.assert_array_equal(outs[kind][3].view(np.uint32), e[3].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ 8: nothing moves when unused
def test_items_that_are_not_armed_and_old_targets_launch_what_they_did():
    """A carried but unarmed search item marks nothing and changes nothing: the states and effective actions are those of the table
    without the item.  A search on the pushes alone leaves the action-fault launch as it was (no marked item, query words 0).
    tests/test_gpu_search.py pins the records of the old targets, tests/test_gpu_actfault.py the action faults without a search and
    tests/test_gpu_kernel_plan.py the kernel-plan answers of cosim_query."""
    acts = _actions()
    finals = []
    for scn in (_scenarios(search=True), _scenarios(search=False)):
        env = _env(ranges=RANGES, scenarios=scn, check_slots=SLOTS)
        q = env.engine.query
        assert q("search") == 0 and q("search_targets") == 0 and q("search_checks") == 0 and q("action_faults_marked") == 0
        env.reset()
        states, effs = [], []
        for k in range(40):
            env.step(acts[k])
            states.append(env.state.cpu().numpy().copy()); effs.append(env.effective_action().cpu().numpy().copy())
        finals.append((np.stack(states), np.stack(effs)))
        env.close()
    np.testing.assert_array_equal(finals[0][0].view(np.uint32), finals[1][0].view(np.uint32))
    np.testing.assert_array_equal(finals[0][1].view(np.uint32), finals[1][1].view(np.uint32))
    scn = _scenarios(search=False)
    scn[0]["pushes"] = PUSH
    scn[0]["search"] = {"lo": 1.0, "hi": 4.0, "rule": "bisect", "trials": 3, "targets": ["pushes"], "fail_on": ["terminated"]}
    env = _env(ranges=RANGES, scenarios=scn, search=SLOTS)
    q = env.engine.query
    assert q("search") == 1 and q("search_targets") == 1 and q("search_checks") == 0 and q("action_faults_marked") == 0
    assert len(env.scenario_table.pack_search(SLOTS)) == 2 + 11 * 3   # the short form reached the engine
    env.close()


# ------------------------------------------------------------------------------------------------------------ refusals and ordering
def test_engine_refusals_and_the_order_set_scenarios_keeps():
    from cosim_amd.scenario import _ACTION_FAULTS
    scn = _scenarios()
    env = _env(scenarios=scn, search=SLOTS, check_slots=SLOTS)
    T = env.scenario_table
    q = env.engine.query
    assert q("action_faults_marked") == 8
    # while marked items are set the search is neither replaced nor cleared
    for words in (T.pack_search(SLOTS), None):
        with pytest.raises(ValueError, match="action-fault items are marked for the search that is armed"):
            env.engine.search_set(words)
    # nor do the checks it fails on go
    with pytest.raises(ValueError, match="the limit search that is armed fails on a check"):
        env.engine.scenario_checks_set(None)
    # set_scenarios does the ordering: again in place (the records stay), then without the search, then without anything
    env.reset()
    acts = _actions()
    for k in range(30):
        env.step(acts[k])
    before = env.search(include_trials=False)
    env.set_scenarios(scn, search=SLOTS, check_slots=SLOTS)
    after = env.search(include_trials=False)
    assert q("action_faults_marked") == 8 and (after.trials[after.has_item] == 1).all()
    np.testing.assert_array_equal(before.state[:, :10], after.state[:, :10])   # levels, steps, counts and brackets stay
    env.set_scenarios(scn, check_slots=SLOTS)                        # carried, not armed
    assert q("search") == 0 and q("action_faults_marked") == 0 and q("action_faults") > 0
    # a marked table with no search armed is refused, and so is one whose search names other targets
    with pytest.raises(ValueError, match="no search whose targets name these items is armed"):
        env.engine.scenario_action_faults_set(T._pack_fault_items(_ACTION_FAULTS, marks=True))
    with pytest.raises(ValueError, match="names a check and the checks are not armed"):
        env.set_scenarios(scn, search=SLOTS)
    env.set_scenarios(scn, search=SLOTS, check_slots=SLOTS)
    env.set_scenarios(None)
    assert q("search") == 0 and q("scenario_rows") == 0 and q("action_faults_marked") == 0
    env.close()
