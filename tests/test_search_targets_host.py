"""What the limit search gained over its first form, on the host (no GPU): marked parameter windows, observation faults and action
faults scaled by the level, ``harder`` up / down, a check verdict as a failure criterion and the long table form.  The shared headers
(csrc/cosim_search.h, cosim_fault.h, cosim_scnparams.h, cosim_obsfault.h, cosim_actfault.h, cosim_tables.h) are compiled as a plain C++ program with its own main (tests/search_targets_lanes.cpp, once more
with address and undefined-behaviour sanitizers) and driven lane by lane against the numpy twins, bit for bit; then packing, the
round trips and every refusal."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CD = 4
i32, f32 = np.int32, np.float32
SEED = 0x1234_5678_9ABC
ACT = ["hip_l", "knee_l", "wheel_l", "hip_r", "knee_r", "wheel_r"]
NU = len(ACT)
PUSH = [[2, 5, 0.0, 1.0, 0.0]]
CHECKS = [[0, 10, "info", 3, "always", "<", 1.0, "bounded"], [5, 20, "tracking_error", 0, "settle", "<", 0.2, "recovers"],
          [0, 20, "info", 1, "mean", ">", 0.1]]
# every markable op, a hold in between, two items on one actuator (composition), "*" (one ordinal, NU elements), clock 0 inside
FAULTS = [[0, 6, "hip_l", "scale", 1.5],          # 0
          [0, 6, "hip_l", "bias", 0.25],          # 1: composes with 0
          [1, 9, "knee_l", "set", -0.75],         # 2
          [0, 9, "*", "noise", 0.125],            # 3
          [2, 9, "wheel_l", "hold", 0.0],         # 4: never marked
          [0, 12, "*", "drop", 0.2],              # 5: the probability is scaled
          [0, 12, "knee_r", "clip", 0.4],         # 6
          [0, 12, "wheel_r", "bias", -0.5]]       # 7


def item(**kw):
    base = {"lo": 0.0, "hi": 4.0, "rule": "bisect", "trials": 3, "targets": ["pushes"], "fail_on": ["terminated"]}
    base.update(kw)
    return base


KP = {"kp": ACT, "kd": ACT, "geom_friction": ["floor", "g1", "g2"], "dof_frictionloss": ["d0", "d1"]}
OBS = {"stacked": [("gyro", 3), ("enc", 4)], "non_stacked": [("clock", 2)], "stack_size": 3}


def table(rows):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(rows, CD, names={"action_faults": ACT, "faults": OBS, **KP})


def table5():
    """Row 0: no item.  1: every markable listed item marked, harder up.  2: ordinals 1, 5 and 7 marked (0, 2, 3, 6 stay as written in
    the same row), harder down.  3: the old form (pushes, no new key).  4: fails on checks only, harder down, staircase."""
    return table([
        {"pushes": PUSH, "action_faults": FAULTS},
        {"pushes": PUSH, "action_faults": FAULTS[:4] + FAULTS[5:],
         "search": item(lo=0.25, hi=2.0, targets=["action_faults"], trials=1000)},
        {"pushes": PUSH, "action_faults": FAULTS, "checks": CHECKS,
         "search": item(lo=0.5, hi=3.0, start=1.0, step=1.0, min_step=0.25, rule="staircase", trials=1000, harder="down",
                        targets=["pushes", "action_faults:7,1,5"], fail_on=["terminated", "check:recovers"], rev_skip=1)},
        {"pushes": PUSH, "search": item(trials=6, fail_on=["tilt"])},
        {"pushes": PUSH, "checks": CHECKS, "search": item(lo=0.05, hi=1.0, rule="staircase", trials=1000, harder="down", fail_on=["checks"])},
    ])


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    """tests/search_targets_lanes.cpp + the shared headers as a plain C++ program (no HIP, no GPU), stand-alone, run as a child."""
    out = str(tmp_path_factory.mktemp("search_targets") / ("lanes_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "search_targets_lanes.cpp")])
    return out


def _run(exe, words):
    p = subprocess.run([exe], input=" ".join(str(int(w)) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.strip().splitlines()


def _ints(a):
    return np.ascontiguousarray(a).astype(np.int64).reshape(-1).tolist()


def _s32(a):
    """uint32 / uint64 words as the int32 the driver reads."""
    return (np.asarray(a).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(i32).reshape(-1).tolist()


def _table_words(T, slots):
    w = T.pack_search(slots)
    S = len(T)
    cols = (len(w) - 2) // S
    assert len(w) == 2 + cols * S and cols in (11, 14)
    return [S, slots, cols] + w[2:].tolist()


# ------------------------------------------------------------------------------------------------------------ packing, both lengths
def test_pack_is_short_for_old_items_and_long_for_the_new_keys():
    from cosim_amd.scenario import ScenarioTable
    old = ScenarioTable([{"pushes": PUSH}, {"pushes": PUSH, "search": item()}], CD)
    assert len(old.pack_search(3)) == 2 + 11 * 2
    marked_only = table([{"pushes": PUSH}, {"action_faults": FAULTS[:2], "search": item(targets=["action_faults:1"])}])
    w = marked_only.pack_search(3)
    assert len(w) == 2 + 11 * 2 and w[2 + 8 * 2 + 1] == 16            # a mark alone needs no long form: the targets word says it
    T = table5()
    w = T.pack_search(4)
    assert len(w) == 2 + 14 * 5
    cols = w[2:].reshape(14, 5)
    assert cols[8].tolist() == [0, 16, 1 | 16, 1, 1]                  # targets
    assert cols[9].tolist() == [0, 1, 1, 32, 0]                       # fail_mask: the ledger's bits alone
    assert cols[11].tolist() == [0, 0, 1, 0, 1]                       # harder
    assert cols[12].tolist() == [0, 0, 2, 0, 7] and cols[13].tolist() == [0] * 5
    assert T.search_marks("action_faults", 1) == list(range(7)) and T.search_marks("action_faults", 2) == [1, 5, 7]
    assert T.search_marks("action_faults", 0) == [] and T.has_search_marks("action_faults")
    # the marks travel in the item table: bit 15 of the element of exactly the marked ordinals, nothing else moves
    from cosim_amd.scenario import _ACTION_FAULTS, FAULT_MARK
    plain = T.pack_action_faults()                                    # stays unmarked
    assert not (plain[2] & FAULT_MARK).any()
    adr, t, elem, op, ordinal, value = T._pack_fault_items(_ACTION_FAULTS, marks=True)
    want = np.zeros(len(elem), dtype=bool)
    want[adr[1]:adr[2]] = True
    want[adr[2]:adr[3]] = np.isin(ordinal[adr[2]:adr[3]], [1, 5, 7])
    np.testing.assert_array_equal((elem & FAULT_MARK) != 0, want)
    np.testing.assert_array_equal(elem & ~FAULT_MARK, plain[2])
    for a, b in zip((adr, t, op, ordinal, value), (plain[0], plain[1], plain[3], plain[4], plain[5])):
        np.testing.assert_array_equal(a, b)


def test_round_trips_emit_the_new_keys_only_when_not_default():
    import yaml
    from cosim_amd.scenario import ScenarioTable, sweep
    T = table5()
    lst = T.to_list()
    assert "harder" not in lst[1]["search"] and "harder" not in lst[3]["search"] and lst[2]["search"]["harder"] == "down"
    assert lst[2]["search"]["targets"] == ["pushes", "action_faults:7,1,5"] and lst[2]["search"]["fail_on"] == ["terminated", "check:recovers"]
    assert set(lst[3]["search"]) == {"lo", "hi", "start", "step", "min_step", "rule", "trials", "targets", "fail_on", "rev_skip"}
    back = ScenarioTable(yaml.safe_load(yaml.safe_dump(lst)), CD, names={"action_faults": ACT})
    for slots in (1, 7):
        np.testing.assert_array_equal(back.pack_search(slots), T.pack_search(slots))
    assert [back.search_marks("action_faults", s) for s in range(5)] == [T.search_marks("action_faults", s) for s in range(5)]
    # words -> items -> words, both lengths
    again = T.search_from_words(T.pack_search(5))
    np.testing.assert_array_equal(again.pack_search(5), T.pack_search(5))
    assert again.search[2]["harder"] == "down" and again.search[2]["fail_on"] == ["terminated", "check:1"] and again.search[4]["fail_on"] == ["checks"]
    assert again.search_marks("action_faults", 2) == [1, 5, 7]
    old = ScenarioTable([{"pushes": PUSH}, {"pushes": PUSH, "search": item()}], CD)
    np.testing.assert_array_equal(old.search_from_words(old.pack_search(2)).pack_search(2), old.pack_search(2))
    with pytest.raises(ValueError, match="search table"):
        T.search_from_words(T.pack_search(5)[:-1])
    # the sweep axis carries the new keys
    full = list(sweep([[0.5, 0, 0, 0]], [0.3], (0.0,), [(5, 8)], action_faults=[FAULTS[:2]], checks=[CHECKS],
                      search=[item(targets=["action_faults:0"], harder="down", fail_on=["check:bounded"])]))
    S = ScenarioTable(full, CD, names={"action_faults": ACT})
    assert S.search[0]["harder"] == "down" and S.search_marks("action_faults", 0) == [0] and S.search[0]["check_mask"] == 1


# ------------------------------------------------------------------------------------------------------------ the rule, lane by lane
def _scripted(rng, N, K, p_end):
    """K events for N lanes: steps with random done flags, verdict masks with failed, incomplete and passed items, and host cuts."""
    events, meta4 = [], np.zeros(N, dtype=np.int64)
    for k in range(K):
        if k in (17, 41, 90):
            mask = None if k == 90 else rng.random(N) < 0.4
            events.append(("begin", mask, 8 if k == 41 else 0, meta4.copy()))
        te, tr = rng.random(N) < p_end, rng.random(N) < p_end / 3
        meta4 = meta4 + ((rng.random(N) < 0.05) & (te | tr))
        fail = rng.choice(np.array([0, 0, 0, 1, 2, 4, 3, 1 << 40], dtype=np.uint64), size=N)
        inc = rng.choice(np.array([0, 0, 0, 0, 2, 4, 1 << 63], dtype=np.uint64), size=N)
        events.append(("step", te, tr, meta4.copy(), rng.choice([0, 0, 1, 2, 4, 5], size=N), fail, inc))
    return events


def _lanes_rule(exe, T, slots, rows, events, fall, flag, meta4):
    N = len(rows)
    words = [0] + _table_words(T, slots) + [int(fall), flag, N] + _ints(rows) + _ints(meta4)
    for ev in events:
        if ev[0] == "step":
            fail, inc = np.asarray(ev[5], dtype=np.uint64), np.asarray(ev[6], dtype=np.uint64)
            words += [1] + _ints(ev[1]) + _ints(ev[2]) + _ints(ev[3]) + _ints(ev[4]) + _s32(fail) + _s32(fail >> np.uint64(32)) + _s32(inc) + _s32(inc >> np.uint64(32))
        else:
            words += [2, ev[2]] + _ints(np.ones(N) if ev[1] is None else ev[1]) + _ints(ev[3])
    lines = _run(exe, words + [-1])
    rec = np.array([[int(x) for x in ln.split()[1:]] for ln in lines[:N]], dtype=i32)
    ring = np.array([[int(x) for x in ln.split()[1:]] for ln in lines[N:2 * N]], dtype=i32).reshape(N, slots, 4)
    return rec, ring, int(lines[2 * N].split()[1])


@pytest.mark.parametrize("fall,flag", [(True, 0), (False, 8)])
def test_rule_with_harder_and_checks_equals_the_twin(exe, fall, flag):
    from cosim_amd import search as sr
    T = table5()
    rng = np.random.default_rng(5)
    N, K, slots = 31, 150, 6
    rows = np.arange(N) % 5
    meta4 = np.zeros(N, dtype=np.int64)
    events = _scripted(rng, N, K, 0.35)
    rec, ring, rem = _lanes_rule(exe, T, slots, rows, events, fall, flag, meta4)
    state, tring, trem = sr.reference_search(T, slots, rows, events, fall=fall, flag=flag, meta4=meta4)
    np.testing.assert_array_equal(rec, state)
    np.testing.assert_array_equal(ring, tring)
    assert rem == trem
    res = sr.SearchResult.from_raw(state, tring, rows, table=T)
    assert res.harder.tolist() == [int(r in (2, 4)) for r in rows]
    loc = res.trial_env
    by_check = (res.flags & sr.BY_CHECK) != 0
    # a check fails a trial only on the rows that select one, only a counted one, and the selected bits alone matter: row 2 selects
    # bit 1 (of the values 2 and 3), row 4 bits 0..2; bit 40 and bit 63 are selected by nobody
    assert by_check.any() and set(np.unique(rows[loc][by_check])) == {2, 4}
    assert (res.counted & res.failed)[by_check].all()
    only_check = by_check & ((res.flags & 1) == 0)
    assert only_check.any()                                           # trials the ledger's flags would have passed
    assert not by_check[rows[loc] == 3].any() and not by_check[rows[loc] == 1].any()
    # harder down: a failure moves the level up, a pass down (or not at all: clamped at an end); harder up the other way
    seen = set()
    for k in range(len(res) - 1):
        if loc[k] != loc[k + 1] or not (res.counted[k] and res.counted[k + 1]) or rows[loc[k]] not in (1, 2, 4):
            continue
        down, d = rows[loc[k]] in (2, 4), float(res.trial_level[k + 1]) - float(res.trial_level[k])
        assert d == 0 or (d > 0) == (bool(res.failed[k]) == down)
        seen.add((int(rows[loc[k]]), bool(res.failed[k]), d != 0))
    assert {(1, True, True), (1, False, True), (2, True, True), (2, False, True), (4, True, True), (4, False, True)} <= seen
    by = res.by_scenario()
    assert by[2]["harder"] == "down" and by[2]["targets"] == ["pushes", "action_faults:7,1,5"] and by[1]["harder"] == "up"
    assert res.survival(4)[2]["harder"] == "down" and res.survival(4)[1]["harder"] == "up"


def test_harder_down_clamps_brackets_and_threshold(exe, tmp_path):
    """Outcomes that only fail, then only pass, under harder="down": failures run the level into hi, passes into lo; the bracket
    holds the lowest pass and the highest failure; a check that is incomplete fails the trial as a failed one does."""
    from cosim_amd import search as sr
    T = table([{"pushes": PUSH, "checks": CHECKS[:1],
                "search": item(lo=0.05, hi=1.0, start=0.5, step=0.25, min_step=0.0625, rule="staircase", trials=30, harder="down", fail_on=["check:0"])}])
    z, one = np.zeros(3, dtype=np.int64), np.ones(3, dtype=bool)
    u = lambda *a: np.array(a, dtype=np.uint64)                       # noqa: E731
    # env 0: the check fails every episode; env 1: incomplete every episode; env 2: passes every episode (another check's bit is set)
    end = ("step", ~one, one, z, z, u(1, 0, 2), u(0, 1, 4))
    events = [end] * 6
    rec, ring, rem = _lanes_rule(exe, T, 8, [0, 0, 0], events, False, 0, z)
    state, tring, trem = sr.reference_search(T, 8, [0, 0, 0], events, meta4=z)
    np.testing.assert_array_equal(rec, state)
    np.testing.assert_array_equal(ring, tring)
    res = sr.SearchResult.from_raw(state, tring, [0, 0, 0], table=T)
    lv = res.trial_level.reshape(3, -1)
    assert lv[0].tolist() == lv[1].tolist() == [0.5, 0.75, 1.0, 1.0, 1.0, 1.0]          # failures: up, into hi
    assert lv[2].tolist() == [0.5, 0.25, f32(0.05), f32(0.05), f32(0.05), f32(0.05)]   # passes: down, into lo
    assert res.level.tolist() == [1.0, 1.0, f32(0.05)]
    fl = res.flags.reshape(3, -1)
    assert ((fl[:2] & (sr.FAILED | sr.BY_CHECK)) == (sr.FAILED | sr.BY_CHECK)).all() and ((fl[2] & (sr.FAILED | sr.BY_CHECK)) == 0).all()
    assert np.isnan(res.bracket[0, 0]) and res.bracket[0, 1] == 1.0                     # the HIGHEST failure
    assert res.bracket[2, 0] == f32(0.05) and np.isnan(res.bracket[2, 1])               # the LOWEST pass
    # then the other outcome: a reversal each; the bracket closes round the threshold
    swap = ("step", ~one, one, z, z, u(0, 0, 1), u(0, 0, 0))
    events2 = events + [swap] * 2
    rec, ring, _ = _lanes_rule(exe, T, 8, [0, 0, 0], events2, False, 0, z)
    state, tring, _ = sr.reference_search(T, 8, [0, 0, 0], events2, meta4=z)
    np.testing.assert_array_equal(rec, state)
    np.testing.assert_array_equal(ring, tring)
    res = sr.SearchResult.from_raw(state, tring, [0, 0, 0], table=T)
    assert res.reversals.tolist() == [1, 1, 1]
    assert res.bracket[0].tolist() == [0.875, 1.0] and res.bracket[2].tolist() == [f32(0.05), f32(0.175)]
    assert (res.bracket[[0, 2], 0] <= res.threshold[[0, 2]]).all() and (res.threshold[[0, 2]] <= res.bracket[[0, 2], 1]).all()
    path = str(tmp_path / "s.npz")
    res.save(path)
    back = sr.SearchResult.load(path)
    assert sr.same_search(res, back) is None and back.harder.tolist() == [1, 1, 1] and back.items == res.items
    # the same outcomes with harder="up" move the other way (the old rule)
    up = table([{"pushes": PUSH, "checks": CHECKS[:1],
                 "search": item(lo=0.05, hi=1.0, start=0.5, step=0.25, min_step=0.0625, rule="staircase", trials=30, fail_on=["check:0"])}])
    state_up, ring_up, _ = sr.reference_search(up, 8, [0, 0, 0], events, meta4=z)
    rec_up, rring_up, _ = _lanes_rule(exe, up, 8, [0, 0, 0], events, False, 0, z)
    np.testing.assert_array_equal(rec_up, state_up)
    assert sr.SearchResult.from_raw(state_up, ring_up, [0, 0, 0]).level.tolist() == [f32(0.05), f32(0.05), 1.0]


def test_old_items_give_the_old_words_through_the_new_driver(exe):
    """A table of old items: the short form, and records equal to the twin's with the verdict words ignored."""
    from cosim_amd import search as sr
    from cosim_amd.scenario import ScenarioTable
    T = ScenarioTable([{"pushes": PUSH}, {"pushes": PUSH, "search": item(trials=9)}], CD)
    assert _table_words(T, 2)[2] == 11
    rng = np.random.default_rng(3)
    rows = np.arange(7) % 2
    events = _scripted(rng, 7, 60, 0.4)
    rec, ring, rem = _lanes_rule(exe, T, 2, rows, events, True, 0, np.zeros(7, dtype=np.int64))
    plain = [ev[:5] if ev[0] == "step" else ev for ev in events]      # the old twin call: no masks
    state, tring, trem = sr.reference_search(T, 2, rows, plain, fall=True)
    np.testing.assert_array_equal(rec, state)
    np.testing.assert_array_equal(ring, tring)
    assert rem == trem and not (tring[:, :, 2] & sr.BY_CHECK).any()


# ------------------------------------------------------------------------------------------------------------ marked action faults
def _item_words(T):
    from cosim_amd.scenario import _ACTION_FAULTS
    adr, t, elem, op, ordinal, value = T._pack_fault_items(_ACTION_FAULTS, marks=True)
    key = elem.astype(np.uint32) | (op.astype(np.uint32) << 16) | (ordinal.astype(np.uint32) << 24)
    return adr, np.stack([t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32), key, value.view(np.uint32)], axis=1)


def test_marked_action_faults_as_host_cpp_equal_the_twin(exe):
    """Random envs over all rows at clocks from 0 on: the walk a search's kernel runs equals ``reference_action_faults(level=...)``
    bit for bit, the unmarked items of a marked row are what they are without a search, and a level of exactly 1 changes nothing."""
    from cosim_amd.scenario import MODES, reference_action_faults
    T = table5()
    adr, items = _item_words(T)
    rng = np.random.default_rng(9)
    N, env_id0 = 160, 3
    env = np.arange(N)
    gid = env + env_id0
    t = rng.integers(0, 13, size=N)
    t[:20] = 0                                                       # clock 0: hold / drop are the identity, set / bias / noise are not
    ep = np.zeros(N, dtype=np.int64)
    sc = rng.integers(1, 1000, size=N)
    raw = rng.uniform(-1, 1, size=(N, NU)).astype(f32)
    last = rng.uniform(-1, 1, size=(N, NU)).astype(f32)
    level = rng.uniform(0.25, 2.0, size=N).astype(f32)
    level[::7] = 1.0
    words = [1, len(T), MODES["env"], env_id0, len(items)] + adr.tolist() + _s32(items)
    words += [NU] + _s32([SEED & 0xFFFFFFFF, SEED >> 32]) + [N]
    bits = lambda a: np.ascontiguousarray(a, dtype=f32).view(i32).reshape(-1).tolist()   # noqa: E731
    for i in range(N):
        words += [int(env[i]), int(ep[i]), int(t[i]), int(sc[i])] + bits(level[i]) + bits(raw[i]) + bits(last[i])
    out = np.array([[int(x) for x in ln.split()] for ln in _run(exe, words)], dtype=np.int64)
    assert out.shape == (N, 1 + 2 * NU)
    eff = out[:, 1:1 + NU].astype(i32).view(f32)
    plain = out[:, 1 + NU:].astype(i32).view(f32)
    want = reference_action_faults(T, "env", gid, t, ep, sc, SEED, raw, last, level=level)
    unscaled = reference_action_faults(T, "env", gid, t, ep, sc, SEED, raw, last)
    np.testing.assert_array_equal(out[:, 0], gid % len(T))
    np.testing.assert_array_equal(eff.view(i32), want.view(i32))
    row = gid % len(T)
    np.testing.assert_array_equal(eff[row == 0].view(i32), unscaled[row == 0].view(i32))          # a row without an item
    np.testing.assert_array_equal(eff[level == 1.0].view(i32), unscaled[level == 1.0].view(i32))  # x * 1 is x
    assert (eff[(row == 1) & (level != 1.0)] != unscaled[(row == 1) & (level != 1.0)]).any()
    # row 2: ordinals 1, 5, 7 marked; actuator 4 (knee_r) is under the unmarked clip (6) and the marked drop (5) and noise stays unmarked:
    # with the drop not firing it equals the unscaled word.  Actuator 5 (wheel_r) is under the marked bias 7: -0.5 * level.
    m2 = (row == 2) & (t < 9) & (level != 1.0)
    assert (eff[m2, 5] != unscaled[m2, 5]).any()
    # the walk without a search never sees a marked element match: those items are inert there, the rest is as written
    T_unmarked_rows = reference_action_faults(table([{"pushes": PUSH, "action_faults": FAULTS}] + [{"pushes": PUSH}] * 4), "env", gid, t, ep, sc, SEED, raw, last)
    np.testing.assert_array_equal(plain[row == 0].view(i32), T_unmarked_rows[row == 0].view(i32))
    # a drop whose probability is scaled: over many draws the share follows p * level
    Td = table([{"action_faults": [[0, 100, "*", "drop", 0.25]], "pushes": PUSH, "search": item(lo=0.0, hi=4.0, targets=["action_faults"])}])
    M = 4000
    g = np.arange(M)
    r0, l0 = np.ones((M, NU), dtype=f32), np.zeros((M, NU), dtype=f32)
    for lv, share in ((0.0, 0.0), (1.0, 0.25), (2.0, 0.5), (4.0, 1.0)):
        got = reference_action_faults(Td, "env", g, np.full(M, 3), np.zeros(M), np.full(M, 7), SEED, r0, l0, level=np.full(M, lv, dtype=f32))
        lost = (got[:, 0] == 0).mean()
        assert (got == got[:, :1]).all() and abs(lost - share) < 0.03, (lv, lost)


def test_twin_level_none_is_todays_result():
    from cosim_amd.scenario import reference_action_faults
    T = table5()
    rng = np.random.default_rng(1)
    N = 40
    raw, last = rng.uniform(-1, 1, (N, NU)).astype(f32), rng.uniform(-1, 1, (N, NU)).astype(f32)
    a = reference_action_faults(T, "env", np.arange(N), np.arange(N) % 12, np.zeros(N), np.arange(N) + 5, SEED, raw, last)
    b = reference_action_faults(T, "env", np.arange(N), np.arange(N) % 12, np.zeros(N), np.arange(N) + 5, SEED, raw, last, level=np.ones(N, dtype=f32))
    np.testing.assert_array_equal(a.view(i32), b.view(i32))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_python_refusals_name_the_scenario_and_search():
    def bad(match, faults=FAULTS, checks=CHECKS, **kw):
        with pytest.raises(ValueError, match=match) as e:
            table([{"pushes": PUSH}, {"pushes": PUSH, "action_faults": faults, "checks": checks, "search": item(**kw)}])
        assert "scenario 1, search" in str(e.value)

    bad("lists no action-fault item", faults=[], targets=["action_faults"])
    bad("ordinal 8 outside", targets=["action_faults:8"])
    bad("ordinal -1 outside", targets=["action_faults:-1"])
    bad("followed by ordinals", targets=["action_faults:x"])
    bad("a hold", targets=["action_faults:4"])
    bad("a hold", targets=["action_faults"])                                      # the whole kind would mark the hold too
    bad("named twice", targets=["action_faults:0", "action_faults:1"])
    bad("drop probability must stay in", targets=["action_faults:5"], lo=0.0, hi=6.0)      # 0.2 * 6 > 1
    bad("noise value must stay >= 0", targets=["action_faults:3"], lo=-1.0, hi=1.0)
    bad("clip value must stay >= 0", targets=["action_faults:6"], lo=-1.0, hi=1.0)
    bad("not finite", faults=[[0, 5, 0, "bias", 3e38]], targets=["action_faults:0"], lo=0.0, hi=4.0)
    bad("lists no parameter window", targets=["params"])
    bad("lists no fault item", targets=["faults"])
    bad("non-empty list of different names", targets=["windows"])
    bad("harder 'sideways'", harder="sideways")
    bad("has no check", checks=[], fail_on=["checks"])
    bad("no check of that name or ordinal", fail_on=["check:nope"])
    bad("no check of that name or ordinal", fail_on=["check:3"])
    bad("non-empty list of different names", fail_on=["check"])
    # what stays accepted
    T = table([{"pushes": PUSH, "action_faults": FAULTS, "checks": CHECKS,
                "search": item(targets=["action_faults:0,1,2,3,5,6,7"], fail_on=["check:2", "check:bounded"], lo=0.0, hi=4.0)}])
    assert T.search[0]["check_mask"] == 5 and T.search_marks("action_faults", 0) == [0, 1, 2, 3, 5, 6, 7]


def _validate(exe, T, words, mode=0, auto_reset=1, chk=True, kinds=True):
    key_adr, _, _, push_adr, _, _ = T.pack()
    head = [2, len(T), mode, auto_reset] + key_adr.tolist() + push_adr.tolist()
    head += [1] + T.pack_checks()[0].tolist() if chk and T.has_checks else [0]
    head += ([1] + T.pack_params()[0].tolist() if kinds and T.has_params else [0])
    head += [0]                                                       # (no observation faults in these tables)
    head += ([1] + T.pack_action_faults()[0].tolist() if kinds and T.has_action_faults else [0])
    S = int(words[0])
    cols = (len(words) - 2) // S
    return _run(exe, head + [S, int(words[1]), cols] + list(words[2:]))


def test_validator_takes_both_lengths_and_refuses_by_name(exe):
    T = table5()
    T.resolve_checks(None)
    w = T.pack_search(3)
    out = _validate(exe, T, w)
    assert out[0] == "OK 4"
    cols = w[2:].reshape(14, 5)
    for k, ln in enumerate(out[1:]):
        f = [int(x) for x in ln.split()[1:]]
        assert f[0] == 5 * k and f[1:] == cols[k].tolist()
    assert len(out) == 15
    short = np.concatenate([w[:2], w[2:2 + 55]])
    short[2 + 9 * 5 + 4] = 1                                          # (row 4 fails on checks alone: give it a ledger bit)
    out = _validate(exe, T, short)
    assert out[0] == "OK 4" and len(out) == 12                        # the short form: eleven arrays, three null pointers
    who = 'cosim_set_param "search": '

    def err(words, **kw):
        out = _validate(exe, T, words, **kw)
        assert len(out) == 1 and out[0].startswith("ERR " + who), out
        return out[0][4 + len(who):]

    def changed(col, s, value):
        c = w.copy()
        c[2 + col * 5 + s] = value
        return c

    assert err(changed(11, 2, 2)) == "scenario 2: harder 2 is neither 0 (up) nor 1 (down)"
    assert err(w, chk=False).startswith("scenario 2: the item fails on a check and no checks are armed")
    assert err(changed(12, 2, 8)) == "scenario 2: the item fails on a check the scenario does not have: it has 3 check items"
    assert err(changed(13, 4, 1)) == "scenario 4: the item fails on a check the scenario does not have: it has 3 check items"
    assert err(changed(12, 4, 0)).startswith("scenario 4: fail_mask 0 must be a non-empty set")       # no ledger bit and no check
    kinds5 = "(1 pushes | 2 commands | 4 parameter windows | 8 observation faults | 16 action faults)"
    assert err(changed(8, 1, 32)) == "scenario 1: targets 32 names nothing " + kinds5
    assert err(changed(8, 1, 4)) == "scenario 1: targets 4 names nothing (1 pushes | 2 commands)"      # no parameter windows are set at all
    assert err(changed(8, 1, 8)) == "scenario 1: targets 8 names nothing (1 pushes | 2 commands)"      # no observation faults are set
    assert err(w, kinds=False) == "scenario 1: targets 16 names nothing (1 pushes | 2 commands)"       # no action faults are set
    assert err(changed(8, 3, 1 | 16)) == "scenario 3: the target is the action faults and the scenario has no action-fault item"
    P = table([{"pushes": PUSH, "params": [[0, 5, "kp", 0, "scale", 0.5]]}, {"pushes": PUSH, "search": item(targets=["pushes"])}])
    pw = P.pack_search(2)
    pw[2 + 8 * 2 + 1] = 1 | 4
    out = _validate(exe, P, pw)
    assert out == ['ERR cosim_set_param "search": scenario 1: the target is the parameter windows and the scenario has no parameter item']


def _marks(exe, T, armed=True, elem_or=None, lo=None, hi=None, targets=None):
    from cosim_amd.scenario import _ACTION_FAULTS
    adr, t, elem, op, ordinal, value = T._pack_fault_items(_ACTION_FAULTS, marks=True)
    if elem_or is not None:
        elem = elem | np.asarray(elem_or, dtype=i32)
    S, n = len(T), len(elem)
    w = T.pack_search(2)[2:].reshape(-1, S)
    words = [3, 16, NU, S, n] + adr.tolist() + t.reshape(-1).tolist() + elem.tolist() + op.tolist() + ordinal.tolist() + value.view(i32).tolist()
    words += [int(armed)] + w[0].tolist() + (w[8].tolist() if targets is None else targets)
    words += (w[1] if lo is None else np.asarray(lo, dtype=f32).view(i32)).tolist() + (w[2] if hi is None else np.asarray(hi, dtype=f32).view(i32)).tolist()
    return _run(exe, words), (adr, t, elem, op, ordinal, value)


def test_marked_item_table_rules(exe):
    from cosim_amd.scenario import FAULT_MARK
    T = table5()
    out, (adr, t, elem, op, ordinal, value) = _marks(exe, T)
    n = len(elem)
    assert out[0] == f"OK {n} {int(((elem & FAULT_MARK) != 0).sum())}" and len(out) == 1 + n
    got = np.array([[int(x) for x in ln.split()[1:]] for ln in out[1:]], dtype=np.int64).astype(i32)
    key = elem.astype(np.uint32) | (op.astype(np.uint32) << 16) | (ordinal.astype(np.uint32) << 24)
    np.testing.assert_array_equal(got, np.stack([t[:, 0], t[:, 1], key.view(i32), value.view(i32)], axis=1))   # the mark rides in the el field
    who = 'cosim_set_param "action_faults": '

    def err(**kw):
        out, _ = _marks(exe, T, **kw)
        assert len(out) == 1 and out[0].startswith("ERR " + who), out
        return out[0][4 + len(who):]

    no_search = "the item is marked for a limit search and no search whose targets name these items is armed on the scenario"
    assert no_search in err(armed=False)                              # no search at all
    assert no_search in err(targets=[0, 1, 1, 1, 1])                  # a search on the pushes alone
    first0 = np.zeros(n, dtype=i32)
    first0[0] = FAULT_MARK
    assert err(elem_or=first0).startswith("scenario 0, action-fault item 0: " + no_search)   # a row without an item
    hold = np.zeros(n, dtype=i32)
    k = int(adr[2]) + int(np.nonzero(op[adr[2]:adr[3]] == 4)[0][0])
    hold[k] = FAULT_MARK
    assert err(elem_or=hold).endswith("a hold has no value and cannot be marked for a limit search")
    S = len(T)
    assert "a drop probability must lie in [0, 1] at both ends" in err(hi=[0, 2.0, 6.0, 4.0, 1.0])
    assert "a noise amplitude must be >= 0 at both ends" in err(lo=[0, -1.0, 0.5, 0.0, 0.05])
    assert "value * level is not finite" in err(hi=[0, 3e38, 3.0, 4.0, 1.0])
    assert S == 5
    # an unmarked table passes with no search, as it always did
    out, _ = _marks(exe, table([{"action_faults": FAULTS}] + [{"pushes": PUSH}] * 4), armed=False, targets=[0] * 5, lo=[0] * 5, hi=[0] * 5)
    assert out[0] == f"OK {len(FAULTS) - 2 + 2 * NU} 0"


# ------------------------------------------------------------------------------------------------------------ marked parameter windows
PARAMS = [[0, 8, "geom_friction", "floor", "scale", 1.0],            # 0: marked in row 1: the friction scale is the level itself
          [2, 6, "kp", "*", "scale", 0.8],                           # 1: one ordinal, NU items
          [0, 12, "kd", 1, "set", 3.0],                              # 2
          [4, 9, "kp", 0, "set", 40.0],                              # 3: listed behind 1: the last listed item wins on kp[0]
          [0, 12, "dof_frictionloss", "*", "scale", 2.0]]            # 4


def _param_table():
    """Row 0: windows, no item.  1: all marked, harder down.  2: ordinals 1 and 2 marked, 0, 3, 4 as written in the same row."""
    return table([{"pushes": PUSH, "params": PARAMS},
                  {"pushes": PUSH, "params": PARAMS, "search": item(lo=0.05, hi=1.0, targets=["params"], harder="down")},
                  {"pushes": PUSH, "params": PARAMS, "search": item(lo=0.5, hi=2.0, targets=["params:2,1", "pushes"])}])


def test_marked_params_as_host_cpp_equal_the_twin(exe):
    from cosim_amd.scenario import MODES, PARAM_MARK, reference_params
    T = _param_table()
    assert T.pack_search(2)[2 + 8 * 3:2 + 9 * 3].tolist() == [0, 4, 1 | 4] and len(T.pack_search(2)) == 2 + 14 * 3   # harder down: the long form
    lay = {"kp": 0, "kd": NU, "geom_friction": 2 * NU, "dof_frictionloss": 2 * NU + 3, "stride": 2 * NU + 5 + 60}      # more than one pass of 64 lanes
    adr, t, field, index, op, value = T.pack_params(marks=True)
    plain = T.pack_params()
    assert not (plain[4] & PARAM_MARK).any() and np.array_equal(op & ~PARAM_MARK, plain[4])
    want_mark = np.zeros(len(op), dtype=bool)
    want_mark[adr[1]:adr[2]] = True
    want_mark[adr[2]:adr[3]] = np.isin(np.asarray(T.param_ords[2]), [1, 2])
    np.testing.assert_array_equal((op & PARAM_MARK) != 0, want_mark)
    word = np.array([lay[{0: "kp", 1: "kd", 2: "geom_friction", 3: "dof_frictionloss"}[int(f)]] + int(i) for f, i in zip(field, index)], dtype=i32)
    rng = np.random.default_rng(4)
    N, env_id0 = 90, 2
    gid = np.arange(N) + env_id0
    tt = rng.integers(0, 13, size=N)
    tt[:12] = 0                                                       # clock 0
    base = rng.uniform(0.5, 2.0, size=(N, lay["stride"])).astype(f32)
    level = rng.uniform(0.05, 2.0, size=N).astype(f32)
    level[::5] = 1.0
    bits = lambda a: np.ascontiguousarray(a, dtype=f32).view(i32).reshape(-1).tolist()   # noqa: E731
    words = [4, len(T), MODES["env"], env_id0, len(op)] + adr.tolist() + t.reshape(-1).tolist() + word.tolist() + op.tolist() + bits(value) + [lay["stride"], N]
    for i in range(N):
        words += [i, 0, int(tt[i])] + bits(level[i]) + bits(base[i])
    out = np.array([[int(x) for x in ln.split()] for ln in _run(exe, words)], dtype=np.int64)
    P = lay["stride"]
    eff, plain_eff = out[:, 1:1 + P].astype(i32).view(f32), out[:, 1 + P:].astype(i32).view(f32)
    want = reference_params(T, "env", gid, tt, np.zeros(N), base, lay, level=level)
    unscaled = reference_params(T, "env", gid, tt, np.zeros(N), base, lay)
    np.testing.assert_array_equal(eff.view(i32), want.view(i32))
    np.testing.assert_array_equal(plain_eff.view(i32), unscaled.view(i32))
    row = gid % 3
    np.testing.assert_array_equal(eff[row == 0].view(i32), unscaled[row == 0].view(i32))
    np.testing.assert_array_equal(eff[level == 1.0].view(i32), unscaled[level == 1.0].view(i32))
    m1 = (row == 1) & (tt < 8) & (level != 1.0)
    np.testing.assert_array_equal(eff[m1, 2 * NU].view(i32), (base[m1, 2 * NU] * level[m1]).astype(f32).view(i32))   # friction = base * (1.0 * level)
    m2 = (row == 2) & (level != 1.0) & (tt < 12)
    np.testing.assert_array_equal(eff[m2, NU + 1].view(i32), (f32(3.0) * level[m2]).astype(f32).view(i32))            # a marked set is v
    hold3 = (row == 2) & (tt >= 4) & (tt < 9)
    assert (eff[hold3, 0] == f32(40.0)).all()                          # the unmarked set listed last wins, unscaled
    assert (eff[m2][:, 2 * NU + 3:2 * NU + 5] == (base[m2][:, 2 * NU + 3:2 * NU + 5] * f32(2.0))).all()   # unmarked in a marked row
    a = reference_params(T, "env", gid, tt, np.zeros(N), base, lay, level=np.ones(N, dtype=f32))
    np.testing.assert_array_equal(a.view(i32), unscaled.view(i32))


def test_marked_param_table_rules(exe):
    from cosim_amd.scenario import PARAM_MARK
    T = _param_table()
    adr, t, field, index, op, value = T.pack_params(marks=True)
    S, n = len(T), len(op)
    w = T.pack_search(2)[2:].reshape(-1, S)

    def run(op=op, armed=True, targets=None, hi=None, value=value):
        words = [5, NU, S, n] + adr.tolist() + t.reshape(-1).tolist() + field.tolist() + index.tolist() + list(op) + np.asarray(value, dtype=f32).view(i32).tolist()
        words += [int(armed)] + w[0].tolist() + (w[8].tolist() if targets is None else targets) + w[1].tolist()
        words += (w[2] if hi is None else np.asarray(hi, dtype=f32).view(i32)).tolist()
        return _run(exe, words)

    assert run() == [f"OK {n} {int(((op & PARAM_MARK) != 0).sum())}"]
    who = 'ERR cosim_scenario_params_set: '
    no_search = "the item is marked for a limit search and no search whose targets name the parameter windows is armed on the scenario"
    assert no_search in run(armed=False)[0] and run(armed=False)[0].startswith(who + "scenario 1, parameter item 0")
    assert no_search in run(targets=[0, 1, 1])[0]
    first0 = op.copy()
    first0[0] |= PARAM_MARK
    assert run(op=first0)[0].startswith(who + "scenario 0, parameter item 0: " + no_search)
    assert "value * level is not finite" in run(hi=[0, 3e38, 2.0], value=np.where(np.arange(n) == adr[1], 3e38, value))[0]
    bad = op.copy()
    bad[adr[1]] = PARAM_MARK | 2
    assert "unknown op" in run(op=bad)[0]
    assert run(op=op & ~PARAM_MARK, armed=False) == [f"OK {n} 0"]


# ------------------------------------------------------------------------------------------------------------ marked observation faults
OBS_FAULTS = [[0, 6, "gyro", "*", "bias", 0.1],                     # 0: touches clock 0
              [0, 9, "enc", 1, "scale", 1.5],                        # 1
              [1, 9, "enc", 1, "noise", 0.05],                       # 2: composes with 1
              [0, 12, "clock", 0, "set", 2.0],                       # 3: a non-stacked element
              [2, 9, "gyro", 0, "hold", 0.0],                        # 4: never marked
              [0, 12, "enc", "*", "drop", 0.2]]                      # 5


def _obs_table():
    return table([{"pushes": PUSH, "faults": OBS_FAULTS},
                  {"pushes": PUSH, "faults": OBS_FAULTS[:4] + OBS_FAULTS[5:], "search": item(lo=0.25, hi=2.0, targets=["faults"])},
                  {"pushes": PUSH, "faults": OBS_FAULTS, "search": item(lo=0.5, hi=3.0, targets=["faults:0,3,5"], harder="down")}])


def test_marked_obs_faults_as_host_cpp_equal_the_twin(exe):
    """One observation per env at clocks from 0 on, the stack as a run of the twin leaves it: the walk a search's kernel runs
    equals ``reference_obs_faults(level=...)`` bit for bit; rows without an item and a level of exactly 1 give today's words."""
    from cosim_amd.scenario import _OBS_FAULTS, FAULT_MARK, MODES, reference_obs_faults
    T = _obs_table()
    adr, t, elem, op, ordinal, value = T._pack_fault_items(_OBS_FAULTS, marks=True)
    assert not (T.pack_faults()[2] & FAULT_MARK).any()
    want_mark = np.zeros(len(elem), dtype=bool)
    want_mark[adr[1]:adr[2]] = True
    want_mark[adr[2]:adr[3]] = np.isin(ordinal[adr[2]:adr[3]], [0, 3, 5])
    np.testing.assert_array_equal((elem & FAULT_MARK) != 0, want_mark)
    key = elem.astype(np.uint32) | (op.astype(np.uint32) << 16) | (ordinal.astype(np.uint32) << 24)
    items = np.stack([t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32), key, value.view(np.uint32)], axis=1)
    sd, fd, S = 7, 9, 3
    lay = {"stacked_dim": sd, "frame_dim": fd, "stack_size": S, "command": []}
    rng = np.random.default_rng(2)
    N, K, env_id0 = 60, 11, 1
    gid = np.arange(N) + env_id0
    t_obs = np.stack([np.zeros(N, dtype=np.int64)] + [np.full(N, k) for k in range(1, K)])
    ep, sc = np.zeros((K, N), dtype=np.int64), np.stack([np.full(N, 5 + k) for k in range(K)])
    frames = rng.uniform(-1, 1, size=(K, N, fd)).astype(f32)
    level = np.repeat(rng.uniform(0.25, 3.0, size=(1, N)).astype(f32), K, axis=0)
    level[:, ::6] = 1.0
    want = reference_obs_faults(T, "env", gid, t_obs, ep, sc, SEED, frames, lay, level=level)
    unscaled = reference_obs_faults(T, "env", gid, t_obs, ep, sc, SEED, frames, lay)
    row = gid % 3
    np.testing.assert_array_equal(want[:, row == 0].view(i32), unscaled[:, row == 0].view(i32))
    np.testing.assert_array_equal(want[:, level[0] == 1.0].view(i32), unscaled[:, level[0] == 1.0].view(i32))
    assert (want[:, (row == 1) & (level[0] != 1.0)] != unscaled[:, (row == 1) & (level[0] != 1.0)]).any()
    # the device rule, observation by observation: the stack the previous observation left, rolled, with the clean newest frame in row 0
    bits = lambda a: np.ascontiguousarray(a, dtype=f32).view(i32).reshape(-1).tolist()   # noqa: E731
    stack = np.zeros((N, S, sd), dtype=f32)
    for k in range(K):
        if k == 0:
            stack[:] = frames[0, :, None, :sd]
        else:
            stack[:, 1:] = stack[:, :-1].copy()
            stack[:, 0] = frames[k, :, :sd]
        out_in = np.concatenate([stack.reshape(N, S * sd), frames[k, :, sd:]], axis=1)
        words = [6, len(T), MODES["env"], env_id0, len(items)] + adr.tolist() + _s32(items) + [sd, S, fd] + _s32([SEED & 0xFFFFFFFF, SEED >> 32]) + [N]
        for i in range(N):
            words += [i, 0, int(t_obs[k, i]), int(sc[k, i])] + bits(level[k, i]) + bits(stack[i]) + bits(out_in[i])
        got = np.array([[int(x) for x in ln.split()] for ln in _run(exe, words)], dtype=np.int64)[:, 1:].astype(i32).view(f32)
        stack = got[:, :S * sd].reshape(N, S, sd).copy()
        np.testing.assert_array_equal(got[:, S * sd:].view(i32), want[k].view(i32), err_msg=f"observation {k}")   # (the driver prints the stack, then state_out)


def test_marked_obs_fault_table_rules(exe):
    from cosim_amd.scenario import _OBS_FAULTS, FAULT_MARK
    T = _obs_table()
    adr, t, elem, op, ordinal, value = T._pack_fault_items(_OBS_FAULTS, marks=True)
    S, n = len(T), len(elem)
    w = T.pack_search(2)[2:].reshape(-1, S)

    def run(elem=elem, armed=True, targets=None, hi=None):
        words = [3, 8, 9, S, n] + adr.tolist() + t.reshape(-1).tolist() + list(elem) + op.tolist() + ordinal.tolist() + value.view(i32).tolist()
        words += [int(armed)] + w[0].tolist() + (w[8].tolist() if targets is None else targets) + w[1].tolist()
        words += (w[2] if hi is None else np.asarray(hi, dtype=f32).view(i32)).tolist()
        return _run(exe, words)

    out = run()
    assert out[0] == f"OK {n} {int(((elem & FAULT_MARK) != 0).sum())}"
    no_search = "the item is marked for a limit search and no search whose targets name these items is armed on the scenario"
    assert no_search in run(armed=False)[0] and no_search in run(targets=[0, 16, 16])[0]       # a search on the action faults is not one on these
    hold = elem.copy()
    hold[int(adr[2]) + int(np.nonzero(op[adr[2]:adr[3]] == 4)[0][0])] |= FAULT_MARK
    assert run(elem=hold)[0].endswith("a hold has no value and cannot be marked for a limit search")
    assert "a drop probability must lie in [0, 1] at both ends" in run(hi=[0, 2.0, 6.0])[0]


def test_python_refusals_for_params_and_obs_faults():
    def bad(match, **kw):
        row = {"pushes": PUSH, "params": PARAMS, "faults": OBS_FAULTS}
        row.update({k: kw.pop(k) for k in ("params", "faults") if k in kw})
        with pytest.raises(ValueError, match=match) as e:
            table([{"pushes": PUSH}, {**row, "search": item(**kw)}])
        assert "scenario 1, search" in str(e.value)

    bad("lists no parameter window", params=[], targets=["params"])
    bad("ordinal 5 outside", targets=["params:5"])
    bad("not finite", params=[[0, 5, "kp", 0, "scale", 3e38]], targets=["params:0"])
    bad("lists no fault item", faults=[], targets=["faults"])
    bad("a hold", targets=["faults"])
    bad("ordinal 6 outside", targets=["faults:6"])
    bad("drop probability must stay in", targets=["faults:5"], hi=6.0)
    bad("noise value must stay >= 0", targets=["faults:2"], lo=-1.0, hi=1.0)
    bad("named twice", targets=["params", "params:1"])
    T = table([{"pushes": PUSH, "params": PARAMS, "faults": OBS_FAULTS, "action_faults": FAULTS,
                "search": item(targets=["params:0", "faults:0,1", "action_faults:7"], harder="down")}])
    assert T.pack_search(2)[2 + 8] == 4 | 8 | 16 and T.search_marks("params", 0) == [0] and T.search_marks("faults", 0) == [0, 1]
    again = T.search_from_words(T.pack_search(2))
    assert again.search[0]["targets"] == ["params:0", "faults:0,1", "action_faults:7"]
    # a words-only round trip on a table whose own item does not name the kind marks the whole kind -- and is refused where that marks a hold
    bare = table([{"pushes": PUSH, "faults": OBS_FAULTS, "search": item(targets=["pushes"])}])
    w = bare.pack_search(2)
    w[2 + 8] = 1 | 8
    with pytest.raises(ValueError, match="a hold"):
        bare.search_from_words(w)
