"""Observation faults of a scenario table on the host (no GPU): the numpy twin (cosim_amd/scenario.py reference_obs_faults) against
expectations written out by hand, CSR packing and its round trip, the sweep generator's new axis, the validation messages, the Philox
draws against cosim_amd/rng.py, the kernel's per-env body (csrc/cosim_obsfault.h) compiled as plain C++ and driven lane by lane
against the twin -- once more under AddressSanitizer and UBSan, as a stand-alone child process --, and the kernel-resource and
code-size tables recorded before and after the change."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CD = 2
f32 = np.float32
SEED = 0x1234_5678_9ABC

# a small made-up frame: stacked ang_vel 0..2 | dof_pos 3..4 | command 5..6, non-stacked height_map 7..10; three stack rows
OBS_DIM = {"ang_vel": 3, "dof_pos": 2, "command": 2, "height_map": 4}
SD, FD, S, STATE = 7, 11, 3, 25
TABLE2 = [
    {"faults": [[2, 5, "ang_vel", 0, "bias", 0.5],                  # 0
                [3, 4, "ang_vel", 0, "scale", 2.0],                 # 1: listed behind the bias: (x + 0.5) * 2 at t = 3
                [3, 6, "dof_pos", 1, "hold", 0.0],                  # 2: frozen at its value of t = 2
                [0, 2, "height_map", "*", "set", 9.0],              # 3: a blind height map over the reset's observation and the next
                [1, 3, "ang_vel", 2, "scale", -1.0],                # 4
                [0, 1, "ang_vel", 1, "set", 7.0, "stuck at reset"],  # 5: a fill: every stack row
                {"t0": 0, "t1": 2, "obs": "dof_pos", "index": 0, "op": "hold"}]},   # 6: the identity at t = 0
    {"faults": [[0, 100, "dof_pos", "*", "bias", 1.0]]},
]


def _names(stack_size=S):
    from cosim_amd.scenario import fault_names
    return fault_names(["ang_vel", "dof_pos", "command"], ["height_map"], OBS_DIM, stack_size)


def _table(rows=TABLE2, names=None):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(rows, CD, names={"faults": names or _names()})


def _clean(K, N=1):
    """Distinct words, exact in float32: observation k, env i, element e -> 16 k + e + 1 + 1024 i."""
    return (16.0 * np.arange(K)[:, None, None] + 1024.0 * np.arange(N)[None, :, None] + np.arange(FD)[None, None, :] + 1.0).astype(f32)


def _twin(T, mode, gid, t_obs, ep, frames, step_count=None, names=None, active=None):
    from cosim_amd.scenario import fault_layout, reference_obs_faults
    t_obs = np.asarray(t_obs)
    step_count = np.arange(1, len(t_obs) + 1)[:, None] + np.zeros_like(t_obs) if step_count is None else step_count
    return reference_obs_faults(T, mode, gid, t_obs, ep, step_count, SEED, frames, fault_layout(names or _names()), active=active)


def _row(out, e):
    """The stack rows (newest first) of stacked element e, or the one word of a non-stacked element."""
    return [float(out[k * SD + e]) for k in range(S)] if e < SD else float(out[S * SD + e - SD])


# ------------------------------------------------------------------------------------------------------------ the twin, by hand
def test_twin_against_hand_written_table():
    from cosim_amd.scenario import fault_layout
    T = _table()
    assert len(T) == 2 and T.has_faults and [len(f) for f in T.faults] == [10, 2] and T.n_fault_items == 12
    assert fault_layout(_names()) == {"stacked_dim": SD, "frame_dim": FD, "stack_size": S, "state_dim": STATE, "command": [5, 6]}
    K = 7
    fr = _clean(K)
    t = np.arange(K)[:, None]                                       # one episode: a reset's observation, then six steps
    out = _twin(T, "env", [0], t, np.zeros_like(t), fr)[:, 0]
    assert out.shape == (K, STATE)
    c = lambda k, e: 16.0 * k + e + 1.0                             # noqa: E731  the clean word
    # ang_vel[0]: bias over [2, 5), scale listed behind it over [3, 4): composition in listed order; the roll carries the faulted frames
    assert [_row(out[k], 0)[0] for k in range(K)] == [1.0, 17.0, 33.5, 99.0, 65.5, 81.0, 97.0]
    assert _row(out[3], 0) == [99.0, 33.5, 17.0] and _row(out[4], 0) == [65.5, 99.0, 33.5] and _row(out[6], 0) == [97.0, 81.0, 65.5]
    # dof_pos[1]: held over [3, 6) at what the policy saw at t = 2, across the window's edges
    assert [_row(out[k], 4)[0] for k in range(K)] == [5.0, 21.0, 37.0, 37.0, 37.0, 37.0, 101.0]
    assert _row(out[2], 4) == [37.0, 21.0, 5.0] and _row(out[5], 4) == [37.0, 37.0, 37.0] and _row(out[6], 4) == [101.0, 37.0, 37.0]
    # the non-stacked height map: blind at the reset's observation and the next one
    for e in range(7, 11):
        assert [_row(out[k], e) for k in range(4)] == [9.0, 9.0, c(2, e), c(3, e)]
    # ang_vel[2]: a sign flip over [1, 3)
    assert _row(out[3], 2) == [51.0, -35.0, -19.0] and _row(out[0], 2) == [3.0, 3.0, 3.0]
    # the fill at t_obs = 0: the faulted value in EVERY row; one step on, the roll has moved it down
    assert _row(out[0], 1) == [7.0, 7.0, 7.0] and _row(out[1], 1) == [18.0, 7.0, 7.0] and _row(out[2], 1) == [34.0, 18.0, 7.0]
    # hold at a fill is the identity; at t = 1 it is the reset's value
    assert _row(out[0], 3) == [4.0, 4.0, 4.0] and _row(out[1], 3) == [4.0, 4.0, 4.0] and _row(out[2], 3) == [36.0, 4.0, 4.0]
    # command elements: every row of state_out holds the applied command, untouched
    for k in range(K):
        assert _row(out[k], 5) == [c(k, 5)] * 3 and _row(out[k], 6) == [c(k, 6)] * 3
    # an element under no holding item keeps its bits: the last observation's newest frame but ang_vel[0]... is clean everywhere
    assert np.array_equal(out[6, :SD].view(np.uint32), fr[6, 0, :SD].view(np.uint32))


def test_twin_gated_element_is_faulted_again_from_the_clean_cache():
    """An element that is not refreshed comes back clean from the frequency cache (the clean frame repeats it) and is faulted again at
    its own clock: a bias does not accumulate."""
    T = _table()
    K = 5
    fr = _clean(K, 2)
    fr[1:, 1, 3] = 5.0                                              # env 1 (scenario 1): dof_pos[0] refreshed at k = 1 only
    t = np.repeat(np.arange(K)[:, None], 2, axis=1)
    out = _twin(T, "env", [0, 1], t, np.zeros_like(t), fr)[:, 1]
    assert [_row(out[k], 3)[0] for k in range(1, K)] == [6.0] * 4 and _row(out[4], 3) == [6.0, 6.0, 6.0]
    assert _row(out[4], 4)[0] == float(fr[4, 1, 4]) + 1.0 and _row(out[4], 0)[0] == float(fr[4, 1, 0])


def test_twin_cycle_changes_the_row_at_an_episode_end():
    T = _table()
    K = 6
    fr = _clean(K)
    t = np.array([0, 1, 2, 3, 0, 1])[:, None]                       # the fourth step ends the episode: its observation is the new one's fill
    ep = np.array([0, 0, 0, 0, 1, 1])[:, None]
    out = _twin(T, "cycle", [0], t, ep, fr)[:, 0]
    assert _row(out[3], 0)[0] == 99.0                               # scenario 0 up to the end
    assert _row(out[4], 3) == [16.0 * 4 + 4 + 1] * 3 and _row(out[4], 4) == [16.0 * 4 + 5 + 1] * 3   # scenario 1's bias, every row
    assert _row(out[4], 0) == [65.0] * 3 and _row(out[4], 7) == 16.0 * 4 + 8                                # and none of scenario 0's items
    assert _row(out[5], 3) == [16.0 * 5 + 4 + 1, 16.0 * 4 + 4 + 1, 16.0 * 4 + 4 + 1]
    env = _twin(T, "env", [0], t, ep, fr)[:, 0]                     # mode env ignores the episode count
    assert _row(env[4], 1) == [7.0] * 3 and _row(env[4], 3) == [16.0 * 4 + 4] * 3


def test_twin_masked_observation_leaves_the_other_envs_alone():
    T = _table()
    fr = _clean(3, 2)
    t = np.array([[0, 0], [1, 1], [0, 1]])                          # observation 2: a reset of env 0 alone
    active = np.array([[True, True], [True, True], [True, False]])
    out = _twin(T, "env", [0, 1], t, np.zeros_like(t), fr, active=active)
    assert np.array_equal(out[2, 1].view(np.uint32), out[1, 1].view(np.uint32))
    assert _row(out[2, 0], 1) == [7.0] * 3


# ------------------------------------------------------------------------------------------------------------ the draws
def test_noise_and_drop_draws_are_those_of_rng():
    from cosim_amd import rng
    T = _table([{"faults": [[0, 50, "ang_vel", "*", "set", 0.0], [0, 50, "ang_vel", "*", "noise", 1.0], [1, 50, "dof_pos", "*", "drop", 0.25]]}])
    K, N = 40, 64
    gid = np.arange(100, 100 + N)
    fr = np.broadcast_to(_clean(K)[:, :1], (K, N, FD)).copy()
    t = np.repeat(np.arange(K)[:, None], N, axis=1)
    sc = t + 7
    out = _twin(T, "env", gid, t, np.zeros_like(t), fr, step_count=sc)
    for e in range(3):                                              # x = 0, amplitude 1: the word is u itself, index = the frame element
        w = rng.first_word(SEED, gid[None, :].astype(np.uint64), sc.astype(np.uint32), rng.PURPOSE_OBS_FAULT, e)
        u = rng.fault_noise_u(w)
        assert np.array_equal(out[:, :, e].view(np.uint32), u.view(np.uint32))
        assert u.min() >= -1.0 and u.max() < 1.0 and abs(float(u.mean())) < 0.05
        assert np.array_equal(rng.u01(w), rng.uniform(SEED, gid[None, :].astype(np.uint64), sc.astype(np.uint32), rng.PURPOSE_OBS_FAULT, e))
    assert rng.PURPOSE_OBS_FAULT == 7 and rng.PURPOSE_OBS_FAULT not in (rng.PURPOSE_DELAY, rng.PURPOSE_SENSOR, rng.PURPOSE_INIT, rng.PURPOSE_MASS,
                                                                      rng.PURPOSE_GAIN, rng.PURPOSE_SPAWN, rng.PURPOSE_SPAWN_POSE)
    # the extremes of the two maps
    assert rng.fault_noise_u(np.uint32(0)) == -1.0 and rng.fault_noise_u(np.uint32(0xFFFFFFFF)) == f32(1.0 - 2.0 ** -23)
    assert rng.fault_drop_u(np.uint32(0)) == 0.0 and rng.fault_drop_u(np.uint32(0xFFFFFFFF)) == f32(1.0 - 2.0 ** -24)
    # drop: one draw per (env, step, listed item) -- ordinal 2 here, index 0x10000 + 2 --, both elements lost together
    lost = rng.fault_drop_u(rng.first_word(SEED, gid[None, :].astype(np.uint64), sc.astype(np.uint32), rng.PURPOSE_OBS_FAULT, 0x10000 + 2)) < f32(0.25)
    lost[0] = False                                                 # the fill
    for e in (3, 4):
        same_as_before = out[1:, :, e] == out[:-1, :, e]
        assert np.array_equal(same_as_before, lost[1:])
    assert 0.18 < lost[1:].mean() < 0.32
    never = _table([{"faults": [[0, 50, "dof_pos", "*", "drop", 0.0]]}])
    always = _table([{"faults": [[0, 50, "dof_pos", "*", "drop", 1.0]]}])
    assert np.array_equal(_twin(never, "env", gid, t, np.zeros_like(t), fr)[:, :, 3], fr[:, :, 3])
    assert (_twin(always, "env", gid, t, np.zeros_like(t), fr)[:, :, 3] == fr[0, :, 3]).all()


# ------------------------------------------------------------------------------------------------------------ packing, sweep
def test_packing_and_the_csr_round_trip():
    from cosim_amd.scenario import FAULT_OPS, ScenarioTable
    T = _table()
    adr, t, elem, op, ordinal, value = T.pack_faults()
    assert adr.tolist() == [0, 10, 12] and adr.dtype == np.int32 and t.shape == (12, 2) and value.dtype == np.float32
    assert elem.tolist() == [0, 0, 4, 7, 8, 9, 10, 2, 1, 3, 3, 4]
    assert op.tolist() == [FAULT_OPS[o] for o in ["bias", "scale", "hold"] + ["set"] * 4 + ["scale", "set", "hold", "bias", "bias"]]
    assert ordinal.tolist() == [0, 1, 2, 3, 3, 3, 3, 4, 5, 6, 0, 0]
    assert t[:4].tolist() == [[2, 5], [3, 4], [3, 6], [0, 2]] and value[:4].tolist() == [0.5, 2.0, 0.0, 9.0]
    back = T.faults_from_csr(adr, t, elem, op, ordinal, value, _names())
    for a, b in zip(T.pack_faults(), back.pack_faults()):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    assert back.to_list()[0]["faults"][3] == [0, 2, "height_map", "*", "set", 9.0] and back.to_list()[1]["faults"] == [[0, 100, "dof_pos", "*", "bias", 1.0]]
    # to_list keeps the rows as written, names included, and builds the same table again (dict and YAML form alike)
    again = ScenarioTable(T.to_list(), CD, names={"faults": _names()})
    assert again.to_list() == T.to_list() and T.to_list()[0]["faults"][5][-1] == "stuck at reset"
    import yaml
    from_yaml = ScenarioTable.build(yaml.safe_load(yaml.safe_dump({"scenarios": T.to_list()})), CD)
    assert from_yaml.faults is None and from_yaml.has_faults       # no names yet: kept as written
    assert from_yaml.resolve_faults(_names()).faults == T.faults
    with pytest.raises(ValueError, match="not resolved yet"):
        ScenarioTable(TABLE2, CD).pack_faults()
    assert ScenarioTable([{}], CD).faults == [[]] and not ScenarioTable([{}], CD).has_faults


def test_sweep_has_a_faults_axis_innermost():
    from cosim_amd.scenario import sweep
    F = [[], [[10, 20, "ang_vel", "*", "bias", 0.05]], [{"t0": 0, "t1": 5, "obs": "dof_pos", "op": "hold"}]]
    C = [[[0, 5, 0, "info", 1, 0.0, 1.0, 0]], []]
    base = list(sweep([[0.5, 0.0], [1.0, 0.0]], [0.5], [0.0], [(5, 8)]))
    out = list(sweep([[0.5, 0.0], [1.0, 0.0]], [0.5], [0.0], [(5, 8)], curves=C, faults=F))
    assert len(out) == len(base) * len(C) * len(F)
    assert [("curves" in sc, sc.get("faults")) for sc in out[:6]] == [(True, None), (True, F[1]), (True, F[2]), (False, None), (False, F[1]), (False, F[2])]
    assert list(sweep([[0.5, 0.0]], [0.5], [0.0], [(5, 8)], (), (), ())) == base[:1]   # the positional calls of before
    assert _table(list(sweep([[0.5, 0.0]], faults=F))).n_fault_items == 3 + 2


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("row, message", [
    ([0, 1, "ang_vel", 0, "bias"], r"scenario 0, fault item 0: expected \[t0, t1, obs, index, op, value\] and an optional name"),
    ({"t0": 0, "t1": 1, "obs": "ang_vel", "op": "bias", "amount": 1}, r"fault item 0: a mapping with the keys t0, t1, obs, index, op, value"),
    ([0, 1, "ang_vel", 0, "bias", "much"], r"fault item 0: times and value must be numbers"),
    ([0, 1, "ang_vel", 0, "bias", float("nan")], r"fault item 0: non-finite value"),
    ([0, 1, "ang_vel", 0, "set", 1e39], r"fault item 0: non-finite value"),
    ([0.5, 1, "ang_vel", 0, "bias", 1.0], r"fault item 0: times must be control steps in \[0, 2\^30\)"),
    ([-1, 1, "ang_vel", 0, "bias", 1.0], r"fault item 0: times must be control steps in \[0, 2\^30\)"),
    ([5, 5, "ang_vel", 0, "bias", 1.0], r"fault item 0: t1 5 is not after t0 5"),
    ([0, 1, "command", 0, "bias", 1.0], r"fault item 0: observation 'command' is refused: the command words are the scenario's keyframes"),
    ([0, 1, "ang_vel", 0, "halve", 1.0], r"fault item 0: unknown op 'halve' \(one of scale, bias, set, noise, hold, drop\)"),
    ([0, 1, "ang_vel", 0, "noise", -0.1], r"fault item 0: a noise amplitude must be >= 0"),
    ([0, 1, "ang_vel", 0, "drop", 1.5], r"fault item 0: a drop probability must lie in \[0, 1\]"),
    ([0, 1, "ang_vel", 1.0, "bias", 1.0], r"fault item 0: index must be an int or '\*'"),
    ([0, 1, "ang_vel", "x", "bias", 1.0], r"fault item 0: index must be an int or '\*'"),
    ([0, 1, "ang_vel", 0, "bias", 1.0, 7], r"fault item 0: the name must be a string"),
    ([0, 1, "gyro", 0, "bias", 1.0], r"fault item 0: unknown observation 'gyro' \(the env observes ang_vel, dof_pos, command, height_map\)"),
    ([0, 1, "ang_vel", 3, "bias", 1.0], r"fault item 0: index 3 out of range: 'ang_vel' has 3 entries"),
    ([0, 1, "ang_vel", -1, "bias", 1.0], r"fault item 0: index -1 out of range"),
    ([0, 1, "height_map", 0, "hold", 0.0], r"fault item 0: op 'hold' on 'height_map' needs a stacked observation and stack_size >= 2: there is no previous frame in the record"),
    ([0, 1, "height_map", "*", "drop", 0.5], r"fault item 0: op 'drop' on 'height_map' needs a stacked observation"),
])
def test_refusals_name_scenario_and_item(row, message):
    with pytest.raises(ValueError, match=message):
        _table([{"faults": [row]}])


def test_refusals_that_depend_on_the_table():
    from cosim_amd.scenario import ScenarioTable
    with pytest.raises(ValueError, match=r"scenario 1, fault item 2: t1 3 is not after t0 4"):
        _table([{}, {"faults": [[0, 1, "ang_vel", 0, "bias", 1.0], [0, 1, "ang_vel", 0, "bias", 1.0], [4, 3, "ang_vel", 0, "bias", 1.0]]}])
    with pytest.raises(ValueError, match=r"scenario 0, fault item 0: op 'hold' on 'dof_pos' needs a stacked observation and stack_size >= 2"):
        _table([{"faults": [[0, 1, "dof_pos", 0, "hold", 0.0]]}], names=_names(stack_size=1))
    many = [[0, 1, "height_map", "*", "bias", 1.0]] * 65            # 260 items after expansion
    with pytest.raises(ValueError, match=r"scenario 0: 260 fault items after expansion, at most 256"):
        _table([{"faults": many}])
    assert _table([{"faults": many[:64]}]).n_fault_items == 256
    with pytest.raises(ValueError, match=r"scenario 0: 'faults' must be a list of items"):
        ScenarioTable([{"faults": 3}], CD)
    with pytest.raises(ValueError, match=r"scenario 0: a mapping with the keys 'commands' and 'pushes' is expected"):
        ScenarioTable([{"fault": []}], CD)                          # an unknown scenario key is still refused


# ------------------------------------------------------------------------------------------------------------ the kernel's body, as host C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "obsfault_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/obsfault_lanes.cpp + csrc/cosim_obsfault.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("obsfault")
    return _build(tmp, "obsfault_lanes", []), _build(tmp, "obsfault_lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                                 "-fno-omit-frame-pointer"])


def _item_words(table):
    adr, t, elem, op, ordinal, value = table.pack_faults()
    key = elem.astype(np.uint32) | (op.astype(np.uint32) << 16) | (ordinal.astype(np.uint32) << 24)
    words = np.stack([t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32), key, value.view(np.uint32)], axis=1)
    return adr, words


def _run_lanes(exe, table, mode, env_id0, lay, lanes, env, ep, t, sc, stack, out):
    from cosim_amd.scenario import MODES
    adr, item = _item_words(table)
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    sd, S_, fd = lay["stacked_dim"], lay["stack_size"], lay["frame_dim"]
    words = [len(table), MODES[mode], env_id0, len(item)] + adr.tolist() + item.reshape(-1).tolist()
    words += [sd, S_, fd, lanes, SEED & 0xFFFFFFFF, SEED >> 32, len(env)]
    for i in range(len(env)):
        words += [int(env[i]), int(ep[i]), int(t[i]), int(sc[i])] + u(stack[i]) + u(out[i])
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = np.array([[int(x) for x in line.split()] for line in p.stdout.strip().splitlines()], dtype=np.int64)
    assert rows.shape == (len(env), 1 + S_ * sd + lay["state_dim"])
    return rows[:, 0].astype(np.int32), rows[:, 1:1 + S_ * sd].astype(np.uint32).view(f32), rows[:, 1 + S_ * sd:].astype(np.uint32).view(f32)


# flamingo_light_v1's frame (16 stacked elements, three rows) and one with a non-stacked 15 x 9 height map behind it (151: three passes)
FRAMES = {16: (["dof_pos", "dof_vel", "ang_vel", "projected_gravity", "command"], [], {"dof_pos": 2, "dof_vel": 4, "ang_vel": 3, "projected_gravity": 3, "command": 4}),
          151: (["dof_pos", "dof_vel", "ang_vel", "projected_gravity", "command"], ["height_map"],
                {"dof_pos": 2, "dof_vel": 4, "ang_vel": 3, "projected_gravity": 3, "command": 4, "height_map": 135})}
EVERY_OP = [
    {"faults": [[2, 6, "ang_vel", "*", "bias", 0.05], [3, 5, "ang_vel", 1, "scale", -2.0], [1, 4, "dof_vel", "*", "noise", 0.3],
                [4, 9, "dof_pos", "*", "hold", 0.0], [0, 3, "projected_gravity", 2, "set", -1.0], [1, 9, "dof_vel", "*", "drop", 0.5],
                [5, 7, "dof_vel", 3, "bias", 1.0]]},
    {},
    {"faults": [[0, 9, "projected_gravity", "*", "drop", 0.3], [0, 2, "dof_pos", 0, "hold", 0.0], [0, 1, "dof_vel", "*", "noise", 1.0]]},
]
HM = [[0, 4, "height_map", "*", "set", 0.0], [2, 8, "height_map", 134, "bias", 0.25], [3, 5, "height_map", 64, "noise", 0.1]]


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("lanes", [64, 5, 1])
@pytest.mark.parametrize("frame", [16, 151])
def test_kernel_body_as_host_cpp_equals_the_twin(lanes_exes, frame, lanes, sanitized):
    """A run of nine observations (two episodes) of twelve envs through the functions the kernel calls, with 64 lanes (the wave), 5 and
    1: the test plays the step kernel (roll, clean newest frame, fill at an episode's first observation), the program faults the
    record's stack and the state_out row, and both equal the twin's rows as uint32 at every observation."""
    from cosim_amd.scenario import ScenarioTable, fault_layout, fault_names, scenario_rows
    stacked, non_stacked, dims = FRAMES[frame]
    names = fault_names(stacked, non_stacked, dims, 3)
    lay = fault_layout(names)
    sd, S_, fd = lay["stacked_dim"], lay["stack_size"], lay["frame_dim"]
    assert fd == frame and sd == 16
    rows = [dict(sc) for sc in EVERY_OP]
    if frame == 151:
        rows[1] = {"faults": HM}
        rows[0] = {"faults": rows[0]["faults"] + HM[1:2]}
    T = ScenarioTable(rows, CD, names={"faults": names})
    exe = lanes_exes[1 if sanitized else 0]
    rng = np.random.default_rng(frame + lanes)
    N, env_id0 = 12, 7
    env = np.arange(N)
    t_run = np.array([0, 1, 2, 3, 4, 5, 0, 1, 2])
    for mode in ("env", "cycle"):
        K = len(t_run)
        t = np.repeat(t_run[:, None], N, axis=1)
        ep = np.repeat((np.arange(K) >= 6).astype(np.int64)[:, None], N, axis=1) + 3
        sc = np.arange(K)[:, None] * 3 + 11 + env[None, :]
        frames = rng.uniform(-2.0, 2.0, size=(K, N, fd)).astype(f32)
        from cosim_amd.scenario import reference_obs_faults
        want = reference_obs_faults(T, mode, env + env_id0, t, ep, sc, SEED, frames, lay)
        cmd = np.array(lay["command"])
        stack = np.zeros((N, S_, sd), dtype=f32)
        touched = 0
        for k in range(K):                                          # the step kernel's part: the roll or the fill, commands in every row of state_out
            rec_frame = frames[k, :, :sd].copy()
            rec_frame[:, cmd] = 0.0                                 # the record's stack holds 0 in the command words
            if t_run[k] == 0:
                stack[:] = rec_frame[:, None, :]
            else:
                stack[:, 1:] = stack[:, :-1].copy()
                stack[:, 0] = rec_frame
            so = stack.copy()
            so[:, :, cmd] = frames[k, :, None, :sd][:, :, cmd]
            out = np.concatenate([so.reshape(N, -1), frames[k, :, sd:]], axis=1)
            clean_stack, clean_out = stack.copy(), out.copy()
            row, stack_new, out_new = _run_lanes(exe, T, mode, env_id0, lay, lanes, env, ep[k], t[k], sc[k], stack.reshape(N, -1), out)
            assert np.array_equal(row, scenario_rows(3, mode, env + env_id0, ep[k]))
            assert np.array_equal(out_new.view(np.uint32), want[k].view(np.uint32)), (mode, k, np.nonzero(out_new.view(np.uint32) != want[k].view(np.uint32)))
            stack = stack_new.reshape(N, S_, sd).copy()
            rec_want = want[k, :, :S_ * sd].reshape(N, S_, sd).copy()
            rec_want[:, :, cmd] = 0.0
            assert np.array_equal(stack.view(np.uint32), rec_want.view(np.uint32))   # the record's stack: the same rows, commands left at 0
            touched += int((out_new.view(np.uint32) != clean_out.view(np.uint32)).sum())
            assert np.array_equal(stack[:, :, cmd], clean_stack[:, :, cmd])
        assert touched > 50


# ------------------------------------------------------------------------------------------------------------ kernel resources, code size
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip() for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/obsfault_kres_parent.txt) and after (obsfault_kres_this.txt): every existing kernel's line is
    identical, in the same order; the one added line is obsfault_step_kernel's, which uses no LDS, no scratch and spills nothing."""
    head_a, a = _table_file("obsfault_kres_parent.txt")
    head_b, b = _table_file("obsfault_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["obsfault_step_kernel"], sorted(added)
    vgpr, agpr, sspill, vspill, scratch, occ, lds = added["obsfault_step_kernel"]
    assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 64 and occ == 8


def test_code_size_of_existing_kernels_is_unchanged():
    """tools/ksize.py --lib before and after: the same kernels with the same bytes, plus the new one."""
    head_a, a = _table_file("obsfault_ksize_parent.txt")
    head_b, b = _table_file("obsfault_ksize_this.txt")
    assert head_a == head_b and len(a) >= 40
    new = [ln for ln in b if "obsfault_step_kernel" in ln]
    assert len(new) == 1 and [ln for ln in b if ln not in new] == a
