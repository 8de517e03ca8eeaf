"""Limit search on the host (no GPU): the rule of csrc/cosim_search.h compiled as plain C++ (once more with address and
undefined-behaviour sanitizers) and driven lane by lane against the numpy twin, bit for bit; hand-written expectations of the twin;
the scaled schedule against ``reference_schedule(level=...)``; packing, every ``ValueError``, the validator's messages; the sweep axis;
``SearchResult`` on synthetic records."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CD = 4
i32, f32 = np.int32, np.float32

PUSH = [[2, 5, 0.0, 1.0, 0.0]]
CMDS = [[0, 0.5, 0.0, 0.25, 0.0], [10, -1.0, 0.5, 0.0, 0.0]]


def item(**kw):
    base = {"lo": 0.0, "hi": 4.0, "rule": "bisect", "trials": 3, "targets": ["pushes"], "fail_on": ["terminated"]}
    base.update(kw)
    return base


def table4():
    """Row 0 has no item; 1 bisects with a small budget; 2 is a staircase on both targets whose step reaches d_min and whose first
    reversal is left out of the mean; 3 fails on a fall bit alone."""
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable([
        {"commands": CMDS, "pushes": PUSH},
        {"pushes": PUSH, "search": item()},
        {"commands": CMDS, "pushes": PUSH,
         "search": item(lo=0.5, hi=3.0, start=1.0, step=1.0, min_step=0.25, rule="staircase", trials=1000, targets=["commands", "pushes"],
                        fail_on=["terminated", "nonfinite"], rev_skip=1)},
        {"pushes": PUSH, "search": item(rule="bisect", trials=6, fail_on=["tilt"])},
    ], CD)


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    """tests/search_lanes.cpp + csrc/cosim_search.h + csrc/cosim_tables.h as a plain C++ program (no HIP, no GPU)."""
    out = str(tmp_path_factory.mktemp("search") / ("search_lanes_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "search_lanes.cpp")])
    return out


def _run(exe, words):
    return subprocess.run([exe], input=" ".join(str(int(w)) for w in words), capture_output=True, text=True, check=True).stdout


def _ints(a):
    return np.ascontiguousarray(a).astype(np.int64).reshape(-1).tolist()


# ------------------------------------------------------------------------------------------------------------ the rule, lane by lane
def _scripted(rng, N, K, p_end):
    """K events for N lanes: steps with random done flags, meta word 4 that moves now and then, random fall causes, and host cuts."""
    events, meta4 = [], np.zeros(N, dtype=np.int64)
    for k in range(K):
        if k in (17, 41, 90):                                      # a reset of some envs / a restore of others / a reset of all
            mask = None if k == 90 else rng.random(N) < 0.4
            events.append(("begin", mask, 8 if k == 41 else 0, meta4.copy()))
        te, tr = rng.random(N) < p_end, rng.random(N) < p_end / 3
        meta4 = meta4 + ((rng.random(N) < 0.05) & (te | tr))
        events.append(("step", te, tr, meta4.copy(), rng.choice([0, 0, 1, 2, 4, 5], size=N)))
    return events


def _lanes_rule(exe, T, slots, rows, events, fall, flag, meta4):
    N = len(rows)
    words = [0] + T.pack_search(slots).tolist() + [int(fall), flag, N] + _ints(rows) + _ints(meta4)
    for ev in events:
        if ev[0] == "step":
            words += [1] + _ints(ev[1]) + _ints(ev[2]) + _ints(ev[3]) + _ints(ev[4])
        else:
            words += [2, ev[2]] + _ints(np.ones(N) if ev[1] is None else ev[1]) + _ints(ev[3])
    lines = _run(exe, words + [-1]).strip().splitlines()
    rec = np.array([[int(x) for x in ln.split()[1:]] for ln in lines[:N]], dtype=i32)
    ring = np.array([[int(x) for x in ln.split()[1:]] for ln in lines[N:2 * N]], dtype=i32).reshape(N, slots, 4)
    return rec, ring, int(lines[2 * N].split()[1])


@pytest.mark.parametrize("fall,flag", [(True, 0), (False, 8)])
def test_rule_as_host_cpp_equals_the_twin(exe, fall, flag):
    """Scripted outcome sequences through the functions the kernels call: records, rings and the remaining word equal the twin's word
    for word, and the sequences reach every branch of the rule."""
    from cosim_amd import search as sr
    T = table4()
    rng = np.random.default_rng(11)
    N, K, slots = 23, 140, 2
    rows = np.arange(N) % 4
    meta4 = np.zeros(N, dtype=np.int64)
    events = _scripted(rng, N, K, 0.35)
    rec, ring, rem = _lanes_rule(exe, T, slots, rows, events, fall, flag, meta4)
    state, tring, trem = sr.reference_search(T, slots, rows, events, fall=fall, flag=flag, meta4=meta4)
    np.testing.assert_array_equal(rec, state)
    np.testing.assert_array_equal(ring, tring)
    assert rem == trem == int(((state[:, sr.STATUS] & (sr.HAS_ITEM | sr.DONE)) == sr.HAS_ITEM).sum())
    res = sr.SearchResult.from_raw(state, tring, rows)
    # what the sequences were written to reach
    assert (state[rows == 0][:, :10] == 0).all() and (state[rows == 0, sr.UNCOUNTED] == state[rows == 0, sr.EPISODE]).all()   # rows without an item
    assert res.done[rows == 1].all() and (res.trials[rows == 1] == 3).all() and (res.uncounted[rows == 1] > 0).all()      # the budget ended mid-sequence
    assert not res.done[rows == 2].any() and (res.episodes > slots).all() and (res.lost > 0).all()                         # ring wrap
    st = res.state[rows == 2]
    assert (st[:, sr.REVERSALS] > 1).all() and (st[:, sr.REV_N] == st[:, sr.REVERSALS] - 1).all()                          # rev_skip = 1
    assert (res.step[rows == 2] == f32(0.25)).all()                                                                        # step reached d_min
    assert (res.fails[rows == 3] > 0).any() == fall                                                                        # a fall bit alone
    if not fall:
        assert (res.level[rows == 3] == f32(3.96875)).all() and res.done[rows == 3].all()                                  # six passes from 2: 4 - 2^-5


def test_rule_reaches_both_clamps_and_freezes(exe):
    """Outcomes that only fail, then only pass: the level runs into lo and into hi and stays inside; past the budget it is frozen,
    an episode that began at a restore is not counted and does not move it, and a host cut leaves no trial."""
    from cosim_amd import search as sr
    from cosim_amd.scenario import ScenarioTable
    T = ScenarioTable([{"pushes": PUSH, "search": item(rule="staircase", trials=12, step=1.5, min_step=0.5)}], CD)
    z, one = np.zeros(2, dtype=np.int64), np.ones(2, dtype=bool)
    fail_pass = np.array([True, False])                            # env 0 fails every episode, env 1 passes every one
    end = ("step", fail_pass, ~fail_pass, z, z)                    # terminated / truncated
    mid = ("step", ~one, ~one, z, z)
    events = [mid, end, end, end, mid, ("begin", one, 8, z), mid, end, end, mid, ("begin", [True, False], 0, z), end]
    rec, ring, rem = _lanes_rule(exe, T, 8, [0, 0], events, False, 0, z)
    state, tring, trem = sr.reference_search(T, 8, [0, 0], events, meta4=z)
    np.testing.assert_array_equal(rec, state)
    np.testing.assert_array_equal(ring, tring)
    res = sr.SearchResult.from_raw(state, tring, [0, 0])
    lv = res.trial_level.reshape(2, -1)
    # start 2, step 1.5: 2 -> 0.5 -> 0 (clamped at lo) / 2 -> 3.5 -> 4 (clamped at hi); the restored episode ran at the clamp, uncounted
    assert lv[0].tolist() == [2.0, 0.5, 0.0, 0.0, 0.0, 0.0] and lv[1].tolist() == [2.0, 3.5, 4.0, 4.0, 4.0, 4.0]
    assert res.counted.reshape(2, -1).tolist() == [[True, True, True, False, True, True]] * 2
    assert (res.flags.reshape(2, -1)[:, 3] & 8).all() and res.uncounted.tolist() == [1, 1]
    assert res.length.reshape(2, -1).tolist() == [[2, 1, 1, 2, 1, 1], [2, 1, 1, 2, 1, 2]]    # env 0's cut step left no trial and no length
    assert res.level.tolist() == [0.0, 4.0] and res.trials.tolist() == [5, 5] and rem == trem == 2
    # the budget: 12 trials in all, then frozen
    more = events + [end] * 9
    state2, tring2, trem2 = sr.reference_search(T, 8, [0, 0], more, meta4=z)
    rec2, ring2, rem2 = _lanes_rule(exe, T, 8, [0, 0], more, False, 0, z)
    np.testing.assert_array_equal(rec2, state2)
    np.testing.assert_array_equal(ring2, tring2)
    assert rem2 == trem2 == 0 and state2[:, sr.TRIALS].tolist() == [12, 12] and state2[:, sr.UNCOUNTED].tolist() == [3, 3]
    assert (state2[:, sr.STATUS] & sr.DONE).all()


# ------------------------------------------------------------------------------------------------------------ the twin, by hand
def _levels(T, outcomes):
    """The levels one env runs at over a sequence of outcomes ('P' / 'F'), and the final twin."""
    from cosim_amd.search import SearchTwin
    tw = SearchTwin(T, 4, [0])
    out = [float(tw.levels()[0])]
    for o in outcomes:
        tw.step([o == "F"], [o == "P"], [0])
        out.append(float(tw.levels()[0]))
    return out, tw


def test_twin_against_hand_written_sequences():
    from cosim_amd import search as sr
    from cosim_amd.scenario import ScenarioTable
    T = ScenarioTable([{"pushes": PUSH, "search": item(trials=100)}], CD)                    # bisect on [0, 4]: start 2, step 1
    lv, tw = _levels(T, "PPFP")
    assert lv == [2.0, 3.0, 3.5, 3.25, 3.375]
    res = sr.SearchResult.from_raw(tw.state, tw.ring, [0])
    assert res.bracket.tolist() == [[3.25, 3.5]] and res.threshold.tolist() == [3.375]       # both reversals: (3.5 + 3.25) / 2
    assert res.reversals.tolist() == [2] and res.fails.tolist() == [1] and res.trials.tolist() == [4] and not res.done[0]
    assert res.failed.tolist() == [False, False, True, False] and res.reversal.tolist() == [False, False, True, True]
    # a staircase on [0, 8] from 4 with step 2: the step halves on a reversal, BEFORE the move
    S = ScenarioTable([{"pushes": PUSH, "search": item(hi=8.0, start=4.0, step=2.0, min_step=0.25, rule="staircase", trials=100)}], CD)
    lv, tw = _levels(S, "PPFPF")
    assert lv == [4.0, 6.0, 8.0, 7.0, 7.5, 7.25]
    res = sr.SearchResult.from_raw(tw.state, tw.ring, [0])
    assert res.reversals.tolist() == [3] and res.threshold.tolist() == [f32((8.0 + 7.0 + 7.5) / 3)] and res.step.tolist() == [0.25]
    # with two reversals skipped only the third counts; with none and only passes there is no threshold, with a bracket its middle
    S2 = ScenarioTable([{"pushes": PUSH, "search": item(hi=8.0, start=4.0, step=2.0, min_step=0.25, rule="staircase", trials=100, rev_skip=2)}], CD)
    res = sr.SearchResult.from_raw(*(lambda tw: (tw.state, tw.ring))(_levels(S2, "PPFPF")[1]), [0])
    assert res.threshold.tolist() == [7.5] and res.state[0, sr.REV_N] == 1
    res = sr.SearchResult.from_raw(*(lambda tw: (tw.state, tw.ring))(_levels(S2, "PP")[1]), [0])
    assert np.isnan(res.threshold[0]) and res.bracket[0, 0] == 6.0 and np.isnan(res.bracket[0, 1])
    res = sr.SearchResult.from_raw(*(lambda tw: (tw.state, tw.ring))(_levels(S2, "PPF")[1]), [0])
    assert res.threshold.tolist() == [7.0] and res.bracket.tolist() == [[6.0, 8.0]]          # one skipped reversal: the bracket's middle


# ------------------------------------------------------------------------------------------------------------ the scaled schedule
def _lanes_apply(exe, table, gid_off, env, ep, t, targets, level, cmd_in, quat):
    key_adr, key_t, key_cmd, push_adr, push_t, push_v = table.pack()
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(i32).reshape(-1).tolist()   # noqa: E731
    words = [1, len(table), 0, table.command_dim, gid_off, len(key_t), len(push_t)]
    words += key_adr.tolist() + key_t.tolist() + u(key_cmd) + push_adr.tolist() + push_t.reshape(-1).tolist() + u(push_v) + [len(env)]
    for i in range(len(env)):
        words += [int(env[i]), int(ep[i]), int(t[i]), int(targets[i])] + u(level[i]) + u(cmd_in[i]) + u(quat[i])
    rows = np.array([[int(x) for x in ln.split()] for ln in _run(exe, words).strip().splitlines()], dtype=np.int64)
    cd = table.command_dim
    return (rows[:, 0].astype(i32), rows[:, 1].astype(bool), rows[:, 2:2 + cd].astype(i32).view(f32), rows[:, 2 + cd:].astype(i32).view(f32))


def test_scaled_schedule_equals_the_twin(exe):
    """``scenario_apply_scaled`` on every (env, t) of a table with every targets combination at several levels: rows and commands
    equal ``reference_schedule(level=...)`` exactly -- a passed-through caller's command unscaled --; the push equals
    ``push_reference`` of the twin's scaled velocity to 1e-6 relative (the host compiler's contraction is not the GPU's: the device
    bits are pinned by tests/test_gpu_search.py); level 1.0 gives the bits of the unscaled expressions, level 0.0 zeros."""
    from cosim_amd.scenario import SEARCH_TARGETS, ScenarioTable, push_reference, reference_schedule
    late = [[3, 0.5, -0.25, 0.125, 1.0]]                           # the caller's command passes through before t = 3
    T = ScenarioTable([
        {"commands": late, "pushes": PUSH},
        {"commands": late, "pushes": PUSH, "search": item(targets=["pushes"])},
        {"commands": late, "pushes": PUSH, "search": item(targets=["commands"])},
        {"commands": late, "pushes": PUSH + [[4, 7, -0.5, 0.25, 0.125]], "search": item(targets=["pushes", "commands"])},
    ], CD)
    rng = np.random.default_rng(3)
    env, t, lv = (x.reshape(-1) for x in np.meshgrid(np.arange(8), np.arange(0, 9), np.array([1.0, 0.0, 0.37, 3.25], dtype=f32), indexing="ij"))
    n = len(env)
    lv = lv.astype(f32)
    cmd_in = rng.uniform(-1, 1, size=(n, CD)).astype(f32)
    quat = rng.normal(size=(n, 4)).astype(f32)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True).astype(f32)
    r_row, r_cmd, r_mask, r_v = reference_schedule(T, "env", 5 + env, t, np.zeros(n), cmd_in, level=lv)
    targets = np.array([sum(SEARCH_TARGETS[x] for x in T.search[r]["targets"]) if T.search[r] else 0 for r in r_row])
    row, pushed, cmd, qvel = _lanes_apply(exe, T, 5 % 4, env, np.zeros(n), t, targets, lv, cmd_in, quat)
    np.testing.assert_array_equal(row, r_row)
    np.testing.assert_array_equal(cmd.view(i32), r_cmd.view(i32))
    np.testing.assert_array_equal(pushed, r_mask)
    assert set(targets.tolist()) == {0, 1, 2, 3}
    np.testing.assert_array_equal(cmd[t < 3], cmd_in[t < 3])       # pass-through: never scaled
    want = push_reference(quat[r_mask], r_v[r_mask])
    scale = np.maximum(np.linalg.norm(r_v[r_mask].astype(np.float64), axis=1, keepdims=True), 1e-30)
    assert (np.abs(qvel[r_mask].astype(np.float64) - want) <= 1e-6 * scale).all()
    # against the unscaled schedule: level 1.0 is the identity bit for bit, level 0.0 gives zero words where the target is named
    u_row, u_cmd, u_mask, u_v = reference_schedule(T, "env", 5 + env, t, np.zeros(n), cmd_in)
    _, _, cmd0, qvel0 = _lanes_apply(exe, T, 5 % 4, env, np.zeros(n), t, np.zeros(n), lv, cmd_in, quat)
    np.testing.assert_array_equal(cmd0.view(i32), u_cmd.view(i32))
    one = lv == 1.0
    np.testing.assert_array_equal(cmd[one].view(i32), cmd0[one].view(i32))
    np.testing.assert_array_equal(qvel[one].view(i32), qvel0[one].view(i32))
    zero = lv == 0.0
    assert (r_v[zero & r_mask & ((targets & 1) != 0)] == 0).all() and (qvel[zero & r_mask & ((targets & 1) != 0)] == 0).all()
    assert (cmd[zero & (t >= 3) & ((targets & 2) != 0)] == 0).all()
    np.testing.assert_array_equal(r_v[(targets & 1) == 0], u_v[(targets & 1) == 0])
    np.testing.assert_array_equal(r_cmd[(targets & 2) == 0], u_cmd[(targets & 2) == 0])


# ------------------------------------------------------------------------------------------------------------ packing and refusals
def test_packing_round_trip_and_defaults(tmp_path):
    import yaml
    from cosim_amd.scenario import ScenarioTable
    T = table4()
    assert T.has_search and not ScenarioTable([{"pushes": PUSH}], CD).has_search
    it = T.search[1]
    assert (it["start"], it["step"], it["min_step"], it["rev_skip"]) == (2.0, 1.0, 4.0 / 256, 0)         # the defaults
    w = T.pack_search(5)
    assert w.dtype == i32 and w.shape == (2 + 11 * 4,) and w[:2].tolist() == [4, 5] and w[2:6].tolist() == [0, 1, 1, 1]
    cols = w[2:].reshape(11, 4)
    assert cols[1:6].view(f32)[:, 2].tolist() == [0.5, 3.0, 1.0, 1.0, 0.25]
    assert cols[6:, 2].tolist() == [1, 1000, 3, 1 | 4, 1] and cols[6:, 3].tolist() == [0, 6, 1, 32, 0] and (cols[:, 0] == 0).all()
    back = T.search_from_words(w)
    assert back.to_list() == T.to_list() and back.search == T.search
    np.testing.assert_array_equal(back.pack_search(5), w)
    path = tmp_path / "scn.yaml"
    path.write_text(yaml.safe_dump({"scenarios": T.to_list()}))
    assert ScenarioTable.build(str(path), CD).to_list() == T.to_list()
    for slots in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="search slots"):
            T.pack_search(slots)
    with pytest.raises(ValueError, match="search table of 3 scenarios"):
        T.search_from_words(np.array([3, 1] + [0] * 33))


@pytest.mark.parametrize("change,match", [
    ({"lo": 4.0}, "lo < hi"), ({"hi": float("inf")}, "finite"), ({"lo": "x"}, "must be numbers"), ({"start": 5.0}, "outside"),
    ({"step": 0.0}, "0 < min_step <= step"), ({"min_step": 2.0}, "0 < min_step <= step"), ({"min_step": -1.0}, "0 < min_step <= step"),
    ({"rule": "newton"}, "unknown rule"), ({"trials": 0}, "trials"), ({"trials": (1 << 20) + 1}, "trials"), ({"trials": 2.5}, "trials"),
    ({"targets": []}, "targets"), ({"targets": ["torque"]}, "targets"), ({"targets": "pushes"}, "targets"), ({"targets": ["pushes", "pushes"]}, "targets"),
    ({"fail_on": []}, "fail_on"), ({"fail_on": ["truncated"]}, "fail_on"), ({"rev_skip": 256}, "rev_skip"), ({"rev_skip": -1}, "rev_skip"),
    ({"targets": ["commands"]}, "has no keyframe"), ({"bound": 1.0}, "keys out of"),
])
def test_every_value_error_names_the_scenario(change, match):
    from cosim_amd.scenario import ScenarioTable
    with pytest.raises(ValueError, match=match) as e:
        ScenarioTable([{}, {"pushes": PUSH, "search": item(**change)}], CD)
    assert "scenario 1, search" in str(e.value)


def test_more_value_errors():
    from cosim_amd.scenario import ScenarioTable
    with pytest.raises(ValueError, match="scenario 0, search.*has no push window"):
        ScenarioTable([{"commands": CMDS, "search": item()}], CD)
    with pytest.raises(ValueError, match="scenario 0, search.*'trials' is missing"):
        ScenarioTable([{"pushes": PUSH, "search": {"lo": 0, "hi": 1, "rule": "bisect", "targets": ["pushes"], "fail_on": ["tilt"]}}], CD)
    with pytest.raises(ValueError, match="scenario 0, search.*a mapping"):
        ScenarioTable([{"pushes": PUSH, "search": [0, 1]}], CD)


def _validate(exe, T, words, mode=0, auto_reset=1):
    key_adr, _, _, push_adr, _, _ = T.pack()
    out = _run(exe, [2, len(T), mode, auto_reset] + key_adr.tolist() + push_adr.tolist() + list(words)).strip().splitlines()
    return out


def test_validator_messages_and_packing(exe):
    from cosim_amd.scenario import ScenarioTable
    T = table4()
    w = T.pack_search(3)
    out = _validate(exe, T, w)
    assert out[0] == "OK 3"
    cols = w[2:].reshape(11, 4)
    for k, ln in enumerate(out[1:]):                               # the image: the eleven arrays one behind the other, read through patched pointers
        f = [int(x) for x in ln.split()[1:]]
        assert f[0] == 4 * k and f[1:] == cols[k].tolist()
    who = 'cosim_set_param "search": '

    def err(words, T=T, **kw):
        out = _validate(exe, T, words, **kw)
        assert len(out) == 1 and out[0].startswith("ERR " + who), out
        return out[0][4 + len(who):]

    def changed(col, s, value, dtype=i32):
        c = w.copy()
        c[2 + col * 4 + s] = np.array([value], dtype=dtype).view(i32)[0]
        return c

    assert err(w, mode=1).startswith("the scenario mode is cycle")
    assert err(w, auto_reset=0).startswith("the search needs auto_reset")
    assert err(T.pack_search(3), T=ScenarioTable([{"pushes": PUSH}] * 3, CD)) == "4 scenarios, the table that is set has 3"
    assert err(changed(0, 0, 0) * 0 + np.concatenate([[4, 3], np.zeros(44, dtype=i32)])) == "the table holds no search item (the one word 0 clears the search)"
    bad_slots = w.copy()
    bad_slots[1] = 65
    assert err(bad_slots) == "slots 65 outside 1..64"
    assert err(changed(0, 2, 2)) == "scenario 2: has 2 is neither 0 nor 1"
    assert err(changed(1, 1, np.nan, f32)) == "scenario 1: lo / hi is not finite"
    assert err(changed(2, 2, 0.5, f32)) == "scenario 2: hi is not above lo"
    assert err(changed(3, 1, 4.5, f32)) == "scenario 1: the start level lies outside [lo, hi]"
    assert err(changed(4, 3, 0.001, f32)) == "scenario 3: the steps must hold 0 < d_min <= d0"
    assert err(changed(5, 3, 0.0, f32)) == "scenario 3: the steps must hold 0 < d_min <= d0"
    assert err(changed(6, 1, 2)) == "scenario 1: unknown rule 2 (0 bisect, 1 staircase)"
    assert err(changed(7, 1, 0)) == "scenario 1: trials 0 outside 1..2^20"
    assert err(changed(8, 1, 4)) == "scenario 1: targets 4 names nothing (1 pushes | 2 commands)"
    assert err(changed(9, 1, 2)).startswith("scenario 1: fail_mask 2 must be a non-empty set")
    assert err(changed(9, 1, 0)).startswith("scenario 1: fail_mask 0 must be a non-empty set")
    assert err(changed(10, 3, 256)) == "scenario 3: rev_skip 256 outside 0..255"
    assert err(changed(8, 1, 3)) == "scenario 1: the target is the commands and the scenario has no keyframe"
    no_push = ScenarioTable([{"commands": CMDS}] * 4, CD)
    assert err(w, T=no_push) == "scenario 1: the target is the pushes and the scenario has no push window"
    assert _validate(exe, T, changed(9, 3, 32 | 64 | 128))[0] == "OK 3"     # fall bits are not refused, whatever rule is set


def test_sweep_search_axis_is_innermost():
    from cosim_amd.scenario import ScenarioTable, sweep
    C, V, W = [[0.5, 0, 0, 0], [1.0, 0, 0, 0]], [0.3, 0.6], [(5, 8)]
    A = [[], [[0, 5, "*", "scale", 0.5]]]
    L = [None, item(), item(rule="staircase")]
    full = list(sweep(C, V, (0.0,), W, action_faults=A, search=L))
    assert len(full) == 2 * 2 * 1 * 1 * 2 * 3 == 24
    assert ["search" in sc for sc in full[:6]] == [False, True, True] * 2 and full[2]["search"]["rule"] == "staircase"
    assert ["action_faults" in sc for sc in full[:6]] == [False] * 3 + [True] * 3
    T = ScenarioTable(full, CD)
    assert sum(it is not None for it in T.search) == 16 and len(list(sweep(C, V, (0.0,), W))) == 4


# ------------------------------------------------------------------------------------------------------------ the container
def _synthetic(env_id0, N, slots, seed):
    from cosim_amd import search as sr
    T = table4()
    rng = np.random.default_rng(seed)
    rows = sr.search_rows(T, "env", np.arange(env_id0, env_id0 + N))
    events = _scripted(rng, N, 60, 0.4)
    state, ring, _ = sr.reference_search(T, slots, rows, events, fall=True)
    return sr.SearchResult.from_raw(state, ring, rows, env_id0), state, ring


def test_search_result_save_load_merge_join(tmp_path):
    from cosim_amd import search as sr
    a, sa, ra = _synthetic(0, 9, 3, 1)
    b, sb, rb = _synthetic(9, 7, 3, 2)
    assert a.env.tolist() == list(range(9)) and a.scenario.tolist() == [g % 4 for g in range(9)]
    assert len(a) == int(np.minimum(sa[:, sr.EPISODE], 3).sum()) and a.lost.tolist() == np.maximum(sa[:, sr.EPISODE] - 3, 0).tolist()
    assert (np.diff(a.trial_env) >= 0).all() and all((np.diff(a.episode[a.trial_env == e]) == 1).all() for e in range(9))
    path = str(tmp_path / "search.npz")
    a.save(path)
    back = sr.SearchResult.load(path)
    assert sr.same_search(a, back) is None and back.slots == 3 and back.env_id0 == 0
    assert np.array_equal(back.threshold, a.threshold, equal_nan=True)
    m = b.merge(a)                                                  # either order
    assert m.env.tolist() == list(range(16)) and len(m) == len(a) + len(b) and m.env_id0 == 0
    np.testing.assert_array_equal(m.state, np.concatenate([sa, sb]))
    assert m.counts() == {k: a.counts()[k] + b.counts()[k] for k in a.counts()}
    with pytest.raises(ValueError, match="share env ids"):
        a.merge(a)
    with pytest.raises(ValueError, match="not adjacent"):
        a.merge(_synthetic(12, 4, 3, 3)[0])
    assert "record word" in sr.same_search(a, sr.SearchResult.from_raw(sa + (np.arange(16) == 2), ra, a.scenario))
    # join by (env, episode) with anything that has those columns
    from types import SimpleNamespace
    other = SimpleNamespace(env=m.trial_env[::2], episode=m.episode[::2])
    j = m.join(other)
    assert j[::2].tolist() == list(range(len(other.env))) and (j[1::2] == -1).all()
    # summaries
    s = m.summary()
    assert s["envs"] == int((m.scenario != 0).sum()) and s["trials"] == int(m.trials.sum()) and 0 < s["fail_share"] < 1
    by = m.by_scenario()
    assert sorted(by) == [1, 2, 3] and by[1]["done_share"] == 1.0 and by[2]["done"] == 0 and by[2]["threshold"]["n"] > 0
    pol = m.by_policy(np.arange(16) % 2)
    assert sorted(pol) == ["0", "1"] and pol["0"]["envs"] + pol["1"]["envs"] == s["envs"]
    sv = m.survival(4)
    assert 2 in sv and set(sv) <= {1, 2, 3} and all(int(v["trials"].sum()) == int((m.counted & (m.scenario[m.trial_env] == r)).sum()) for r, v in sv.items())
    assert all(((v["pass_share"][v["trials"] > 0] >= 0) & (v["pass_share"][v["trials"] > 0] <= 1)).all() for v in sv.values())
    nr = sr.SearchResult.from_raw(sa, None, a.scenario)            # without the rings
    assert len(nr) == 0 and nr.summary()["trials"] == a.summary()["trials"]


def test_kernel_resource_tables_keep_every_existing_kernel():
    """profiles/search_kres_parent.txt / search_kres_this.txt (tools/kres.py before and after): every kernel of the parent shows the
    identical line afterwards, scenario_step_kernel among them, and the four new kernels use no LDS."""
    def table(name):
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return [ln.rstrip("\n") for ln in f if ln.strip()]
    old, new = table("search_kres_parent.txt"), table("search_kres_this.txt")
    assert any(ln.startswith("scenario_step_kernel") for ln in old)
    added = [ln for ln in new if ln not in old]
    assert [ln for ln in old if ln not in new] == [] and [ln for ln in new if ln in old] == old
    assert sorted(ln.split("(")[0] for ln in added) == ["scenario_search_step_kernel", "search_begin_kernel", "search_init_kernel", "search_step_kernel"]
    assert all(ln.split()[-1] == "0" for ln in added)               # LDS bytes
