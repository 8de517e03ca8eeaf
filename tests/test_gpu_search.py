"""Limit search on the device (cosim_set_param "search", csrc/cosim_search.hip, and its BatchedEnv surface) against a host-driven
loop: an env with no table that is given, before every step, the command and the push the numpy twins work out
(cosim_amd/scenario.py reference_schedule(level=...), cosim_amd/search.py SearchTwin), the twin's record being advanced from that
env's own flags and meta words.

Every comparison is EXACT: float32 bits for floats, ints as ints.  flamingo_light_v1 on the plane, max_duration = 0.5 (25-step
episodes), actions from a fixed table, 70 envs in 2 ranges (a tail in the last 64-lane block, a range boundary inside a wave), at most
150 steps.  Three scenarios: row 0 without an item, row 1 a bisection on a lateral push over steps [2, 5) with 3 trials, row 2 a
staircase on commands and pushes.  An episode fails when the tilt rule ends it (FallRule(tilt = 0.45, grace = 0), fail_on tilt).

Calibration (one run of 70 envs x 100 steps per level, the push and the command scaled on the host, tilt 0.45): at level lo = 1.0 no
episode of 280 ended with the tilt cause in either row (share 0.000); at level hi = 20.0 every one of 560 did (share 1.000); in between
the share rises (8.0: 0.97, 12.0: 0.99).  At tilt 0.5 / 0.6 a few episodes survive even level 20 (shares 0.996 / 0.993), at tilt 0.35 and
below the unpushed robot already tilts past the rule under the action table (share 0.09 .. 0.5 at level 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, RANGES, STEPS, SLOTS, CD = 70, 2, 150, 4, 4
TILT, LO, HI = 0.45, 1.0, 20.0
BASE = np.array([0.3, 0.0, 0.1, 0.0], dtype=np.float32)
PUSH = [[2, 5, 0.0, 1.0, 0.0]]
_CACHE = {}


def _item(**kw):
    base = {"lo": LO, "hi": HI, "rule": "bisect", "trials": 3, "targets": ["pushes"], "fail_on": ["tilt"]}
    base.update(kw)
    return base


def _scenarios(search=True, hi=HI, lo=LO):
    row1 = {"pushes": PUSH}
    row2 = {"commands": [[3, 0.02, 0.0, 0.01, 0.0]], "pushes": PUSH}       # the caller's command passes through before step 3
    if search:
        row1["search"] = _item(hi=hi, lo=lo)
        # a first step of 12 from the middle runs into a bound at once: the clamp is reached on the first trial
        row2["search"] = _item(hi=hi, lo=lo, rule="staircase", trials=1000, step=12.0, min_step=0.5, targets=["commands", "pushes"], rev_skip=1)
    return [{"commands": [[0, 0.2, 0.0, 0.0, 0.0]], "pushes": PUSH}, row1, row2]


def _model():
    if "model" not in _CACHE:
        from cosim_amd.compile import compile_model
        from cosim_amd.config import make_config
        cfg = make_config("flamingo_light_v1", terrain="flat", random=None, max_duration=0.5)
        _CACHE["model"] = (cfg, compile_model(cfg))
    return _CACHE["model"]


def _env(n=N, **kw):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.fall import FallRule
    cfg, cm = _model()
    kw.setdefault("auto_reset", True)
    kw.setdefault("fall", FallRule(tilt=TILT, grace=0))
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=3, **kw)
    assert env.command_dim == CD
    env.receive_user_command(BASE)
    return env


def _actions():
    if "actions" not in _CACHE:
        import torch
        a = np.random.default_rng(11).uniform(-0.6, 0.6, size=(160, N, 4)).astype(np.float32)   # the table the calibration ran under
        _CACHE["actions"] = a
        _CACHE["actions_dev"] = torch.tensor(a, device="cuda:0")
    return _CACHE["actions_dev"]


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().copy()


def _table(scn):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(scn, CD)


def _rows(table, n=N):
    from cosim_amd.search import search_rows
    return search_rows(table, "env", np.arange(n))


class _Rec:
    """A run recorded step by step: the step outputs, and behind every step the done flags and meta words 4 and 15 a twin is
    advanced from."""

    def __init__(self, env):
        self.env = env
        self.state, self.te, self.tr, self.info, self.levels, self.meta = [], [], [], [], [], []

    def run(self, k0, k1, levels=False):
        env, t, acts = self.env, self.env.torch, _actions()
        for k in range(k0, k1):
            if levels:
                self.levels.append(env.search_levels().cpu().numpy().copy())
            env.step(acts[k][:env.num_envs])
            env.join()
            t.cuda.synchronize(env.device)
            self.record()

    def record(self):
        env = self.env
        self.state.append(env.state.cpu().numpy().copy()); self.info.append(env.info_buf.cpu().numpy().copy())
        self.te.append(env.terminated.cpu().numpy().copy()); self.tr.append(env.truncated.cpu().numpy().copy())
        self.meta.append(_meta(env))

    def advance(self, twin, k0, k1):
        for k in range(k0, k1):
            twin.step(self.te[k], self.tr[k], self.meta[k][:, 4], self.meta[k][:, 15])


def _reference():
    """The eager device run the tests share, never modified: 70 envs in 2 ranges, the three scenarios with the search armed, a ledger
    of SLOTS records alongside, 150 steps."""
    if "reference" not in _CACHE:
        env = _env(ranges=RANGES, scenarios=_scenarios(), search=SLOTS, ledger=SLOTS)
        assert env.engine.query("ranges") == RANGES and env.engine.query("search") == 2 and env.engine.query("search_slots") == SLOTS
        assert env.search_remaining() == len([r for r in _rows(_table(_scenarios())) if r != 0])
        env.reset()
        run = _Rec(env)
        run.first_state = env.state.cpu().numpy().copy()
        run.run(0, STEPS, levels=True)
        run.levels.append(env.search_levels().cpu().numpy().copy())
        run.rows = env.snapshot().rows.cpu().numpy().copy()
        run.result, run.ledger, run.remaining = env.search(), env.ledger(), env.search_remaining()
        env.close()
        run.env = None
        _CACHE["reference"] = run
    return _CACHE["reference"]


# ------------------------------------------------------------------------------------------------------------ 1: device = host-driven
def test_device_search_equals_host_driven_loop():
    """Fleet B has no table: before every step it is handed the command and the push of reference_schedule at the twin's levels, and
    the twin is advanced from B's own flags and meta words.  State, info and flags of every step, the final snapshot rows, the
    search records, the trial rings and the levels before every step are those of the device's search, bit for bit."""
    from cosim_amd import search as sr
    from cosim_amd.scenario import reference_schedule
    a = _reference()
    T = _table(_scenarios())
    rows, gid = _rows(T), np.arange(N)
    env = _env()
    t, acts = env.torch, _actions()
    base = np.tile(BASE, (N, 1))
    meta = _meta(env)
    twin = sr.SearchTwin(T, SLOTS, rows, fall=True, flag=0, meta4=meta[:, 4])
    _, cmd, _, _ = reference_schedule(T, "env", gid, np.zeros(N), meta[:, 11], base, level=twin.levels())
    env.receive_user_command(t.tensor(cmd, device=env.device))      # the reset's state vector carries the scenario's first command
    env.reset()
    t.cuda.synchronize(env.device)
    np.testing.assert_array_equal(a.first_state.view(np.uint32), env.state.cpu().numpy().view(np.uint32))
    meta = _meta(env)
    twin.begin(None, 0, meta[:, 4])
    b = _Rec(env)
    pushed = 0
    for k in range(STEPS):
        lv = twin.levels()
        np.testing.assert_array_equal(a.levels[k].view(np.uint32), lv.view(np.uint32), err_msg=f"search_levels() before step {k}")
        _, cmd, mask, v = reference_schedule(T, "env", gid, meta[:, 0], meta[:, 11], base, level=lv)
        env.receive_user_command(t.tensor(cmd, device=env.device))
        if mask.any():
            env.event("push", t.tensor(v, device=env.device), t.tensor(mask, device=env.device))
            pushed += int(mask.sum())
        env.step(acts[k])
        t.cuda.synchronize(env.device)
        b.record()
        meta = b.meta[-1]
        twin.step(b.te[-1], b.tr[-1], meta[:, 4], meta[:, 15])
    np.testing.assert_array_equal(a.levels[STEPS].view(np.uint32), twin.levels().view(np.uint32))
    rows_b = env.snapshot().rows.cpu().numpy()
    env.close()
    for k in range(STEPS):
        for name in ("state", "info"):
            x, y = getattr(a, name)[k].view(np.uint32), getattr(b, name)[k].view(np.uint32)
            assert np.array_equal(x, y), f"{name} differs in step {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}"
        assert np.array_equal(a.te[k], b.te[k]) and np.array_equal(a.tr[k], b.tr[k]), f"flags differ in step {k}"
    assert np.array_equal(a.rows.view(np.uint32), rows_b.view(np.uint32))
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows)
    assert sr.same_search(a.result, want) is None, sr.same_search(a.result, want)
    assert a.remaining == twin.remaining and pushed > 3 * N


# ------------------------------------------------------------------------------------------------------------ 2: what it is about happened
def test_the_reference_run_reaches_what_the_tests_are_about():
    from cosim_amd import search as sr
    r = _reference().result
    rows = r.scenario
    assert (r.counted & r.failed).any() and (r.counted & ~r.failed).any()              # counted trials of both outcomes (in the rings)
    assert (r.fails > 0).any() and (r.trials - r.fails > 0).any()
    assert (r.reversals > 0).any() and r.reversal.any()                                  # at least one env reversed
    one = rows == 1
    assert r.done[one].all() and (r.trials[one] == 3).all() and (r.uncounted[one] > 0).any()   # done, then an episode that was not counted
    late = (~r.counted) & (rows[r.trial_env] == 1)
    assert late.any() and (r.flags[late] & 8 == 0).all()                                 # uncounted because the budget was spent, not for flag 8
    assert not r.done[rows == 2].any() and not r.has_item[rows == 0].any() and (r.uncounted[rows == 0] == r.episodes[rows == 0]).all()
    lv = np.concatenate([np.asarray(x)[rows == 2] for x in _reference().levels])
    assert (lv == np.float32(LO)).any() or (lv == np.float32(HI)).any()                  # a level hit a clamp
    assert ((r.level[rows != 0] >= LO) & (r.level[rows != 0] <= HI)).all()
    assert r.summary()["envs"] == int((rows != 0).sum()) and sorted(r.by_scenario()) == [1, 2]
    assert (r.state[:, sr.LENGTH] < 25).all() and (r.state[:, 15] == 0).all()


# ------------------------------------------------------------------------------------------------------------ 3: host cuts, ledger ordinals
def test_reset_and_restore_in_mid_episode_keep_the_ledgers_ordinals():
    """A masked reset() before step 30 leaves no trial for the cut episodes; a restore() before step 70 of a snapshot taken behind
    step 12 yields uncounted trials with flag 8 whose level did not move; every trial joins the ledger's record of the same
    (env, episode) with the same flags and length."""
    from cosim_amd import search as sr
    env = _env(ranges=RANGES, scenarios=_scenarios(), search=4, ledger=4)
    T, rows = env.scenario_table, _rows(_table(_scenarios()))
    env.reset()
    twin = sr.SearchTwin(T, 4, rows, fall=True, flag=0, meta4=_meta(env)[:, 4])
    rec = _Rec(env)
    rec.run(0, 12)
    snap = env.snapshot()
    rec.run(12, 30)
    rec.advance(twin, 0, 30)
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    open_len = twin.state[:, sr.LENGTH].copy()
    env.reset(mask=mask)
    twin.begin(mask, 0, _meta(env)[:, 4])
    rec.run(30, 70)
    rec.advance(twin, 30, 70)
    rmask = (np.arange(N) % 4 == 1).astype(np.uint8)
    before = twin.levels()
    env.restore(snap, mask=rmask)
    twin.begin(rmask, 8, _meta(env)[:, 4])
    np.testing.assert_array_equal(env.search_levels().cpu().numpy().view(np.uint32), before.view(np.uint32))   # the level does not move
    rec.run(70, 110)
    rec.advance(twin, 70, 110)
    got, led = env.search(), env.ledger()
    env.close()
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows)
    assert sr.same_search(got, want) is None, sr.same_search(got, want)
    assert (open_len[mask != 0] > 0).any() and np.array_equal(got.lost, led.lost)      # both rings keep the last four
    # the cut episodes left no trial: every trial's length is that of an episode that ran to its end from a begin
    j = got.join(led)
    assert len(got) == len(led) and (j >= 0).all() and np.array_equal(np.sort(j), np.arange(len(led)))
    assert np.array_equal(got.flags & 255, led.flags[j]) and np.array_equal(got.length, led.length[j])       # the ledger's flags, restated
    assert np.array_equal(got.episodes, np.bincount(led.env, minlength=N) + led.lost)
    # the restored envs: one trial with flag 8 each (where the ring still holds it), uncounted, and the trial behind it ran at the same level
    f8 = (got.flags & 8) != 0
    assert f8.any() and (rmask[got.trial_env[f8]] != 0).all() and (np.bincount(got.trial_env[f8], minlength=N) <= 1).all() and not got.counted[f8].any()
    assert ((twin.ring[:, :, 2] & 8) != 0).sum() == f8.sum()
    nxt = np.nonzero(f8)[0] + 1
    ok = (nxt < len(got)) & (got.trial_env[np.minimum(nxt, len(got) - 1)] == got.trial_env[f8])
    assert ok.any() and np.array_equal(got.trial_level[nxt[ok]].view(np.uint32), got.trial_level[np.nonzero(f8)[0][ok]].view(np.uint32))
    assert (got.uncounted[(rmask != 0) & (rows == 2)] == 1).all()


# ------------------------------------------------------------------------------------------------------------ 4: graph, deferred join, in-place rewrite
def _graph_run(env, rewrite=None):
    import torch
    acts = _actions()
    buf = torch.empty((N, env.action_dim), device=env.device)
    side = torch.cuda.Stream(device=env.device)
    buf.copy_(acts[0])
    torch.cuda.synchronize(env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        env.step(buf)                                                # warm-up, eager: step 0
    torch.cuda.current_stream(env.device).wait_stream(side)
    torch.cuda.synchronize(env.device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.step(buf)                                                # recorded, not run: the search launches are part of the graph
    for k in range(1, STEPS):
        if rewrite is not None and k == rewrite[0]:
            torch.cuda.synchronize(env.device)
            env.set_scenarios(rewrite[1], search=SLOTS)
        buf.copy_(acts[k])
        graph.replay()
    torch.cuda.synchronize(env.device)


def test_captured_graph_and_deferred_join_give_the_eager_records():
    from cosim_amd import search as sr
    a = _reference()
    g = _env(ranges=RANGES, scenarios=_scenarios(), search=SLOTS, ledger=SLOTS)
    g.reset()
    _graph_run(g)
    assert sr.same_search(g.search(), a.result) is None, sr.same_search(g.search(), a.result)
    np.testing.assert_array_equal(g.state.cpu().numpy().view(np.uint32), a.state[-1].view(np.uint32))
    g.close()
    d = _env(ranges=4, deferred_join=True, scenarios=_scenarios(), search=SLOTS)
    d.reset()
    acts = _actions()
    for k in range(STEPS):
        d.step(acts[k])
    d.join()
    d.torch.cuda.synchronize(d.device)
    assert sr.same_search(d.search(), a.result) is None, sr.same_search(d.search(), a.result)
    assert d.search_remaining() == a.remaining
    np.testing.assert_array_equal(d.state.cpu().numpy().view(np.uint32), a.state[-1].view(np.uint32))
    d.close()


def test_in_place_rewrite_of_the_bounds_keeps_the_records_and_reaches_the_graph():
    """Before step 75 the bounds are rewritten (the same scenarios have items, the same slots): the records stay, the next trial is
    clamped into the new bounds.  An eager env agrees with the twin carried across the rewrite, a captured graph with the eager env."""
    from cosim_amd import search as sr
    a = _reference()
    scn2 = _scenarios(hi=6.0, lo=2.0)
    e = _env(ranges=RANGES, scenarios=_scenarios(), search=SLOTS)
    e.reset()
    rows = _rows(_table(_scenarios()))
    twin = sr.SearchTwin(e.scenario_table, SLOTS, rows, fall=True, flag=0, meta4=_meta(e)[:, 4])
    rec = _Rec(e)
    rec.run(0, 75)
    rec.advance(twin, 0, 75)
    before = e.search(include_trials=False)
    e.set_scenarios(scn2, search=SLOTS)
    after = e.search(include_trials=False)
    np.testing.assert_array_equal(before.state, after.state)       # in place: nothing of the records moved
    twin.table = e.scenario_table
    rec.run(75, STEPS)
    rec.advance(twin, 75, STEPS)
    got = e.search()
    want = sr.SearchResult.from_raw(twin.state, twin.ring, rows)
    assert sr.same_search(got, want) is None, sr.same_search(got, want)
    two = rows == 2
    assert ((got.level[two] >= 2.0) & (got.level[two] <= 6.0)).all() and (got.episodes > before.episodes).all()
    assert sr.same_search(got, a.result) is not None                # the new bounds changed the run
    # other slots, or an item more or less: the search begins anew
    e.set_scenarios(scn2, search=SLOTS + 1)
    fresh = e.search()
    assert len(fresh) == 0 and (fresh.trials == 0).all() and (fresh.episodes == 0).all() and (fresh.level[two] == np.float32(4.0)).all()
    e.close()
    g = _env(ranges=RANGES, scenarios=_scenarios(), search=SLOTS)
    g.reset()
    _graph_run(g, rewrite=(75, scn2))
    assert sr.same_search(g.search(), got) is None, sr.same_search(g.search(), got)
    g.close()


# ------------------------------------------------------------------------------------------------------------ 5: not armed
def test_items_that_are_not_armed_change_nothing():
    acts = _actions()
    finals = []
    for scn in (_scenarios(search=True), _scenarios(search=False)):
        env = _env(ranges=RANGES, scenarios=scn)
        assert env.engine.query("search") == 0 and env.engine.query("search_slots") == 0 and env.search_slots == 0
        assert env.scenario_table.has_search == ("search" in scn[1])
        for call in (env.search, env.search_remaining, env.search_levels):
            with pytest.raises(ValueError, match="no search is armed"):
                call()
        env.reset()
        states = []
        for k in range(60):
            env.step(acts[k])
            states.append(env.state.cpu().numpy().copy())
        finals.append((np.stack(states), env.snapshot().rows.cpu().numpy().copy()))
        env.close()
    np.testing.assert_array_equal(finals[0][0].view(np.uint32), finals[1][0].view(np.uint32))
    np.testing.assert_array_equal(finals[0][1].view(np.uint32), finals[1][1].view(np.uint32))
    # armed and disarmed again: the engine forgets the search
    env = _env(scenarios=_scenarios(), search=2)
    assert env.engine.query("search") == 2
    env.set_scenarios(_scenarios())
    assert env.engine.query("search") == 0 and env.search_slots == 0
    env.set_scenarios(_scenarios(), search=2)
    env.set_scenarios(None)
    assert env.engine.query("search") == 0 and env.engine.query("scenario_rows") == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------ 6: the remaining word
def test_search_remaining_counts_down_to_zero():
    scn = _scenarios()
    scn[1]["search"]["trials"] = 2
    scn[2]["search"]["trials"] = 2
    env = _env(ranges=RANGES, scenarios=scn, search=SLOTS)
    armed = int((_rows(_table(scn)) != 0).sum())
    env.reset()
    acts = _actions()
    seen = [env.search_remaining()]
    assert seen[0] == armed
    for k in range(60):
        env.step(acts[k])
        if k in (11, 27, 59):
            r = env.search(include_trials=False)
            seen.append(env.search_remaining())
            assert seen[-1] == int((r.has_item & ~r.done).sum())
    assert seen[-1] == 0 and seen == sorted(seen, reverse=True) and 0 < seen[2] < armed
    r = env.search()
    assert (r.trials[r.has_item] == 2).all() and r.done[r.has_item].all()
    env.close()


# ------------------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_reach_cosim_last_error():
    T = _table(_scenarios())
    words = T.pack_search(SLOTS)
    env = _env(scenarios=_scenarios())
    who = 'cosim_set_param "search": '
    with pytest.raises(ValueError) as e:                             # S mismatch
        env.engine.search_set(_table(_scenarios() + [{}]).pack_search(SLOTS))
    assert str(e.value) == who + "4 scenarios, the table that is set has 3"
    bad = words.copy()
    bad[2 + 8 * 3 + 1] = 3                                           # row 1 has no keyframe
    with pytest.raises(ValueError) as e:
        env.engine.search_set(bad)
    assert str(e.value) == who + "scenario 1: the target is the commands and the scenario has no keyframe"
    bad = words.copy()
    bad[2 + 7 * 3 + 2] = 0
    with pytest.raises(ValueError) as e:
        env.engine.search_set(bad)
    assert str(e.value) == who + "scenario 2: trials 0 outside 1..2^20"
    assert env.engine.query("search") == 0
    env.set_scenarios(_scenarios(), mode="cycle")
    with pytest.raises(ValueError) as e:
        env.engine.search_set(words)
    assert str(e.value).startswith(who + "the scenario mode is cycle")
    with pytest.raises(ValueError, match="mode is cycle"):
        env.set_scenarios(_scenarios(), mode="cycle", search=SLOTS)
    env.set_scenarios(None)
    with pytest.raises(ValueError) as e:
        env.engine.search_set(words)
    assert str(e.value).startswith(who + "no scenario table is set")
    env.engine.search_set(None)                                      # clearing nothing is no error
    env.close()
    env = _env(scenarios=_scenarios(), auto_reset=False)
    with pytest.raises(ValueError) as e:
        env.engine.search_set(words)
    assert str(e.value).startswith(who + "the search needs auto_reset")
    env.close()
    # a fall bit in fail_on with no fall rule set is accepted and never fires
    env = _env(scenarios=_scenarios(), search=SLOTS, fall=None)
    assert env.engine.query("fall") == 0 and env.engine.query("search") == 2
    env.reset()
    acts = _actions()
    for k in range(30):
        env.step(acts[k])
    r = env.search()
    assert (r.fails == 0).all() and (r.trials[r.has_item] == 1).all() and not ((r.flags >> 5) & 7).any()
    env.close()
