"""Action faults of a scenario table on the host (no GPU): the numpy twin (cosim_amd/scenario.py reference_action_faults) against
expectations written out by hand, composition order, hold / drop at episode step 0, the Philox draws against cosim_amd/rng.py, CSR
packing and its round trip, the sweep generator's new axis, the validation messages, the kernels' per-env body
(csrc/cosim_actfault.h) compiled as plain C++ and driven lane by lane against the twin -- once more under AddressSanitizer and UBSan,
as a stand-alone child process --, and the kernel-resource and code-size tables recorded before and after the change."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CD = 2
f32 = np.float32
SEED = 0x1234_5678_9ABC
ACT = ["hip_l", "knee_l", "wheel_l", "hip_r", "knee_r", "wheel_r"]
NU = len(ACT)

TABLE2 = [
    {"action_faults": [[2, 5, 0, "bias", 0.5],                      # 0
                       [3, 4, "hip_l", "scale", 2.0],               # 1: listed behind the bias: (x + 0.5) * 2 at t = 3
                       [3, 6, "knee_l", "hold", 0.0],               # 2: frozen at the effective action of t = 2
                       [0, 2, "*", "clip", 0.25],                   # 3: a saturating output over the first two steps
                       [1, 3, 2, "scale", -1.0],                    # 4
                       [4, 6, 3, "set", 7.0, "stuck"],              # 5
                       {"t0": 0, "t1": 2, "index": "knee_r", "op": "hold"}]},   # 6: the identity at t = 0, the reset's zeros at t = 1
    {"action_faults": [[0, 100, "*", "bias", 1.0]]},
]


def _table(rows=TABLE2, act=ACT):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(rows, CD, names={"action_faults": act})


def _run(T, mode, gid, t_run, ep_run, raw, step0=1):
    """K steps of N envs through the twin, prev_eff tracked as the record does: the step's effective action, zeros where the NEXT
    step's clock is 0 (the step ended the episode)."""
    from cosim_amd.scenario import reference_action_faults
    K, N = raw.shape[:2]
    prev = np.zeros((N, raw.shape[2]), dtype=f32)
    out = np.zeros_like(raw)
    for k in range(K):
        if k > 0:
            prev[np.asarray(t_run[k]) == 0] = 0.0
        sc = np.full(N, step0 + k)
        out[k] = reference_action_faults(T, mode, gid, t_run[k], ep_run[k], sc, SEED, raw[k], prev)
        prev = out[k].copy()
    return out


# ------------------------------------------------------------------------------------------------------------ the twin, by hand
def test_twin_against_hand_written_table():
    T = _table()
    assert len(T) == 2 and T.has_action_faults and [len(f) for f in T.action_faults] == [12, 6] and T.n_action_fault_items == 18
    K = 7
    raw = (0.125 * (np.arange(K)[:, None, None] + 1) + np.arange(NU)[None, None, :]).astype(f32)   # step k, actuator j -> (k + 1) / 8 + j
    t = np.arange(K)[:, None]
    out = _run(T, "env", [0], t, np.zeros_like(t), raw)[:, 0]
    x = lambda k, j: (k + 1) / 8 + j                                # noqa: E731  the caller's word
    # hip_l: clip over [0, 2), bias over [2, 5), scale listed behind it over [3, 4): composition in listed order
    assert out[:, 0].tolist() == [0.125, 0.25, x(2, 0) + 0.5, (x(3, 0) + 0.5) * 2.0, x(4, 0) + 0.5, x(5, 0), x(6, 0)]
    # knee_l: clipped, then held over [3, 6) at the effective action of t = 2, across the window's edges
    assert out[:, 1].tolist() == [0.25, 0.25, x(2, 1), x(2, 1), x(2, 1), x(2, 1), x(6, 1)]
    # wheel_l: clip at t = 0; at t = 1 the clip (listed first) and then the sign flip; the flip alone at t = 2
    assert out[:, 2].tolist() == [0.25, -0.25, -x(2, 2), x(3, 2), x(4, 2), x(5, 2), x(6, 2)]
    # hip_r: set over [4, 6)
    assert out[:, 3].tolist() == [0.25, 0.25, x(2, 3), x(3, 3), 7.0, 7.0, x(6, 3)]
    # knee_r: clip, then hold listed behind it: the identity at t = 0, the previous EFFECTIVE action (the clipped one) at t = 1
    assert out[:, 4].tolist() == [0.25, 0.25, x(2, 4), x(3, 4), x(4, 4), x(5, 4), x(6, 4)]
    # an actuator under no holding item keeps the caller's bits
    assert np.array_equal(out[2:, 5].view(np.uint32), raw[2:, 0, 5].view(np.uint32))


def test_every_op_by_hand_and_clip_keeps_nan():
    from cosim_amd.scenario import reference_action_faults
    ops = [("scale", 3.0, 1.5), ("bias", 0.25, 0.75), ("set", -2.0, -2.0), ("hold", 0.0, 9.0), ("drop", 1.0, 9.0), ("drop", 0.0, 0.5),
           ("clip", 0.25, 0.25)]
    for op, value, want in ops:
        T = _table([{"action_faults": [[0, 10, 1, op, value]]}])
        got = reference_action_faults(T, "env", [5], [3], [0], [17], SEED, np.full((1, NU), 0.5, f32), np.full((1, NU), 9.0, f32))
        assert got[0, 1] == f32(want) and got.dtype == np.float32, op
        assert np.array_equal(np.delete(got[0], 1), np.full(NU - 1, 0.5, f32))
    T = _table([{"action_faults": [[0, 10, "*", "clip", 0.25]]}])
    x = np.array([[np.nan, -3.0, 3.0, -0.25, 0.1, -0.0]], dtype=f32)
    got = reference_action_faults(T, "env", [0], [0], [0], [1], SEED, x, np.zeros((1, NU), f32))
    assert np.isnan(got[0, 0]) and got[0, 1:].tolist() == [-0.25, 0.25, -0.25, f32(0.1), -0.0] and np.signbit(got[0, 5])
    # noise: x + value * u with the word of purpose 8, index = the actuator
    from cosim_amd import rng
    T = _table([{"action_faults": [[0, 10, 2, "noise", 0.5]]}])
    got = reference_action_faults(T, "env", [5], [3], [0], [17], SEED, np.full((1, NU), 0.5, f32), np.zeros((1, NU), f32))
    u = rng.fault_noise_u(rng.first_word(SEED, np.uint64(5), np.uint32(17), rng.PURPOSE_ACTION_FAULT, 2))
    assert got[0, 2] == f32(0.5) + f32(0.5) * u


def test_composition_order_matters():
    a = _table([{"action_faults": [[0, 9, 0, "bias", 1.0], [0, 9, 0, "scale", 2.0], [0, 9, 0, "clip", 2.5]]}])
    b = _table([{"action_faults": [[0, 9, 0, "clip", 2.5], [0, 9, 0, "scale", 2.0], [0, 9, 0, "bias", 1.0]]}])
    raw = np.full((1, 1, NU), 1.0, f32)
    z = np.zeros((1, 1), dtype=int)
    assert _run(a, "env", [0], z, z, raw)[0, 0, 0] == 2.5 and _run(b, "env", [0], z, z, raw)[0, 0, 0] == 3.0
    # set behind hold: the set wins; hold behind set: the previous effective action wins
    c = _table([{"action_faults": [[0, 9, 0, "hold", 0.0], [0, 9, 0, "set", 4.0]]}, {"action_faults": [[0, 9, 0, "set", 4.0], [0, 9, 0, "hold", 0.0]]}])
    raw = np.arange(1, 4, dtype=f32)[:, None, None] * np.ones((3, 2, NU), f32)
    t = np.repeat(np.arange(3)[:, None], 2, axis=1)
    out = _run(c, "env", [0, 1], t, np.zeros_like(t), raw)
    assert out[:, 0, 0].tolist() == [4.0, 4.0, 4.0] and out[:, 1, 0].tolist() == [4.0, 4.0, 4.0]
    d = _table([{"action_faults": [[1, 9, 0, "set", 4.0], [0, 9, 0, "hold", 0.0]]}])
    assert _run(d, "env", [0], t[:, :1], np.zeros_like(t[:, :1]), raw[:, :1])[:, 0, 0].tolist() == [1.0, 1.0, 1.0]   # frozen at the first action


def test_hold_and_drop_are_the_identity_at_episode_step_0_and_cycle_changes_the_row():
    T = _table([{"action_faults": [[0, 9, "*", "hold", 0.0]]}, {"action_faults": [[0, 9, "*", "drop", 1.0]]}, {}])
    K = 6
    raw = (np.arange(K)[:, None, None] + 1.0 + 0.0 * np.arange(NU)[None, None, :]).astype(f32)
    t = np.array([0, 1, 2, 0, 1, 2])[:, None]                       # the third step ends the episode
    ep = np.array([0, 0, 0, 1, 1, 1])[:, None]
    for gid in ([0], [1]):
        out = _run(T, "env", gid, t, ep, raw)[:, 0, 0]
        assert out.tolist() == [1.0, 1.0, 1.0, 4.0, 4.0, 4.0]       # frozen at each episode's first action
    out = _run(T, "cycle", [1], t, ep, raw)[:, 0, 0]                # the second episode runs row 2: no items
    assert out.tolist() == [1.0, 1.0, 1.0, 4.0, 5.0, 6.0]


# ------------------------------------------------------------------------------------------------------------ the draws
def test_noise_and_drop_draws_are_those_of_rng():
    from cosim_amd import rng
    from cosim_amd.scenario import reference_action_faults
    assert rng.PURPOSE_ACTION_FAULT == 8 and rng.PURPOSE_ACTION_FAULT not in (rng.PURPOSE_DELAY, rng.PURPOSE_SENSOR, rng.PURPOSE_INIT, rng.PURPOSE_MASS,
                                                                            rng.PURPOSE_GAIN, rng.PURPOSE_SPAWN, rng.PURPOSE_SPAWN_POSE, rng.PURPOSE_OBS_FAULT)
    T = _table([{"action_faults": [[0, 50, "*", "set", 0.0], [0, 50, "*", "noise", 1.0]]}, {"action_faults": [[0, 9, 0, "bias", 1.0], [0, 50, "*", "drop", 0.25]]}])
    N = 64
    gid = np.arange(100, 100 + N)
    sc = np.arange(N) * 3 + 7
    t = np.full(N, 5)
    raw = np.full((N, NU), 0.5, f32)
    prev = np.full((N, NU), -1.0, f32)
    out = reference_action_faults(T, "env", gid, t, np.zeros(N, int), sc, SEED, raw, prev)
    even, odd = gid % 2 == 0, gid % 2 == 1
    for j in range(NU):                                             # x = 0, amplitude 1: the word is u itself, index = the actuator
        u = rng.fault_noise_u(rng.first_word(SEED, gid[even].astype(np.uint64), sc[even].astype(np.uint32), 8, j))
        assert np.array_equal(out[even, j].view(np.uint32), u.view(np.uint32))
        assert u.min() >= -1.0 and u.max() < 1.0
    # drop: one draw per (env, step, listed item) -- ordinal 1 here, index 0x10000 + 1 --, all actuators lost together
    lost = rng.fault_drop_u(rng.first_word(SEED, gid[odd].astype(np.uint64), sc[odd].astype(np.uint32), rng.PURPOSE_ACTION_FAULT, 0x10000 + 1)) < f32(0.25)
    assert 0 < lost.sum() < lost.size
    for j in range(NU):
        assert np.array_equal(out[odd, j] == -1.0, lost)
    assert np.array_equal(out[odd, 0][~lost], np.full(int((~lost).sum()), 1.5, f32))
    at0 = reference_action_faults(T, "env", gid, np.zeros(N, int), np.zeros(N, int), sc, SEED, raw, prev)
    assert (at0[odd, 1:] == 0.5).all() and (at0[odd, 0] == 1.5).all()   # the identity at episode step 0


# ------------------------------------------------------------------------------------------------------------ packing, sweep
def test_packing_and_the_csr_round_trip():
    from cosim_amd.scenario import ACTION_FAULT_OPS, ScenarioTable
    T = _table()
    adr, t, elem, op, ordinal, value = T.pack_action_faults()
    assert adr.tolist() == [0, 12, 18] and adr.dtype == np.int32 and t.shape == (18, 2) and value.dtype == np.float32
    assert elem.tolist() == [0, 0, 1, 0, 1, 2, 3, 4, 5, 2, 3, 4, 0, 1, 2, 3, 4, 5]
    assert op.tolist() == [ACTION_FAULT_OPS[o] for o in ["bias", "scale", "hold"] + ["clip"] * 6 + ["scale", "set", "hold"] + ["bias"] * 6]
    assert ordinal.tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3, 4, 5, 6, 0, 0, 0, 0, 0, 0]
    assert t[:4].tolist() == [[2, 5], [3, 4], [3, 6], [0, 2]] and value[:4].tolist() == [0.5, 2.0, 0.0, 0.25]
    back = T.action_faults_from_csr(adr, t, elem, op, ordinal, value, ACT)
    for a, b in zip(T.pack_action_faults(), back.pack_action_faults()):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    assert back.to_list()[0]["action_faults"][3] == [0, 2, "*", "clip", 0.25] and back.to_list()[1]["action_faults"] == [[0, 100, "*", "bias", 1.0]]
    again = ScenarioTable(T.to_list(), CD, names={"action_faults": ACT})
    assert again.to_list() == T.to_list() and T.to_list()[0]["action_faults"][5][-1] == "stuck"
    import yaml
    from_yaml = ScenarioTable.build(yaml.safe_load(yaml.safe_dump({"scenarios": T.to_list()})), CD)
    assert from_yaml.action_faults is None and from_yaml.has_action_faults   # no names yet: kept as written
    assert from_yaml.resolve_action_faults(ACT).action_faults == T.action_faults
    with pytest.raises(ValueError, match="not resolved yet"):
        ScenarioTable(TABLE2, CD).pack_action_faults()
    assert ScenarioTable([{}], CD).action_faults == [[]] and not ScenarioTable([{}], CD).has_action_faults
    # the other keys of a scenario ride along untouched
    both = ScenarioTable([{"commands": [[0, 1.0, 0.0]], "action_faults": [[0, 1, 0, "set", 1.0]]}], CD, names={"action_faults": ACT})
    assert both.to_list()[0]["commands"] == [[0, 1.0, 0.0]] and not both.has_faults


def test_sweep_has_an_action_faults_axis_innermost():
    from cosim_amd.scenario import sweep
    A = [[], [[10, 20, "*", "drop", 0.2]], [{"t0": 0, "t1": 5, "index": 1, "op": "hold"}]]
    F = [[[0, 5, "ang_vel", "*", "bias", 0.05]], []]
    base = list(sweep([[0.5, 0.0], [1.0, 0.0]], [0.5], [0.0], [(5, 8)]))
    out = list(sweep([[0.5, 0.0], [1.0, 0.0]], [0.5], [0.0], [(5, 8)], faults=F, action_faults=A))
    assert len(out) == len(base) * len(F) * len(A)
    assert [("faults" in sc, sc.get("action_faults")) for sc in out[:6]] == [(True, None), (True, A[1]), (True, A[2]), (False, None), (False, A[1]), (False, A[2])]
    assert list(sweep([[0.5, 0.0]], [0.5], [0.0], [(5, 8)], (), (), (), ())) == base[:1]   # the positional calls of before
    assert _table(list(sweep([[0.5, 0.0]], action_faults=A))).n_action_fault_items == NU + 1


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("row, message", [
    ([0, 1, 0, "bias"], r"scenario 0, action-fault item 0: expected \[t0, t1, index, op, value\] and an optional name"),
    ({"t0": 0, "t1": 1, "op": "bias", "amount": 1}, r"action-fault item 0: a mapping with the keys t0, t1, index, op, value"),
    ([0, 1, 0, "bias", "much"], r"action-fault item 0: times and value must be numbers"),
    ([0, 1, 0, "bias", float("nan")], r"action-fault item 0: non-finite value"),
    ([0, 1, 0, "set", float("inf")], r"action-fault item 0: non-finite value"),
    ([0, 1, 0, "set", 1e39], r"action-fault item 0: non-finite value"),
    ([0.5, 1, 0, "bias", 1.0], r"action-fault item 0: times must be control steps in \[0, 2\^30\)"),
    ([-1, 1, 0, "bias", 1.0], r"action-fault item 0: times must be control steps in \[0, 2\^30\)"),
    ([5, 5, 0, "bias", 1.0], r"action-fault item 0: t1 5 is not after t0 5"),
    ([0, 1, 0, "halve", 1.0], r"action-fault item 0: unknown op 'halve' \(one of scale, bias, set, noise, hold, drop, clip\)"),
    ([0, 1, 0, 3, 1.0], r"action-fault item 0: unknown op 3"),
    ([0, 1, 0, "noise", -0.1], r"action-fault item 0: a noise amplitude must be >= 0"),
    ([0, 1, 0, "clip", -0.1], r"action-fault item 0: a clip bound must be >= 0"),
    ([0, 1, 0, "drop", 1.5], r"action-fault item 0: a drop probability must lie in \[0, 1\]"),
    ([0, 1, 0, "drop", -0.5], r"action-fault item 0: a drop probability must lie in \[0, 1\]"),
    ([0, 1, 1.0, "bias", 1.0], r"action-fault item 0: index must be an int, an actuator name or '\*'"),
    ([0, 1, True, "bias", 1.0], r"action-fault item 0: index must be an int, an actuator name or '\*'"),
    ([0, 1, 0, "bias", 1.0, 7], r"action-fault item 0: the name must be a string"),
    ([0, 1, "elbow", "bias", 1.0], r"action-fault item 0: unknown actuator 'elbow' \(the model has hip_l, knee_l, wheel_l, hip_r, knee_r, wheel_r\)"),
    ([0, 1, 6, "bias", 1.0], r"action-fault item 0: index 6 out of range: the model has 6 actuators"),
    ([0, 1, -1, "bias", 1.0], r"action-fault item 0: index -1 out of range"),
])
def test_refusals_name_scenario_and_item(row, message):
    with pytest.raises(ValueError, match=message):
        _table([{"action_faults": [row]}])


def test_refusals_that_depend_on_the_table():
    from cosim_amd.scenario import ScenarioTable
    with pytest.raises(ValueError, match=r"scenario 1, action-fault item 2: t1 3 is not after t0 4"):
        _table([{}, {"action_faults": [[0, 1, 0, "bias", 1.0], [0, 1, 0, "bias", 1.0], [4, 3, 0, "bias", 1.0]]}])
    many = [[0, 1, "*", "bias", 1.0]] * 43                          # 258 items after expansion
    with pytest.raises(ValueError, match=r"scenario 0: 258 action-fault items after expansion, at most 256"):
        _table([{"action_faults": many}])
    assert _table([{"action_faults": many[:42] + [[0, 1, 0, "bias", 1.0]] * 4}]).n_action_fault_items == 256
    with pytest.raises(ValueError, match=r"scenario 0: 'action_faults' must be a list of items"):
        ScenarioTable([{"action_faults": 3}], CD)
    with pytest.raises(ValueError, match=r"scenario 0: a mapping with the keys 'commands' and 'pushes' is expected"):
        ScenarioTable([{"action_fault": []}], CD)                   # an unknown scenario key is still refused


def test_engine_wrapper_refuses_short_and_long_arrays_before_the_engine_reads_them():
    """Engine.scenario_action_faults_set builds the word table from the arrays' own sizes: arrays that do not match their row
    addresses never reach cosim_set_param (no library is loaded here: the check comes first)."""
    from cosim_amd.engine import Engine
    e = Engine.__new__(Engine)
    adr, t, elem, op, ordinal, value = _table().pack_action_faults()
    with pytest.raises(ValueError, match=r"scenario_action_faults_set: the item arrays are shorter than their row addresses \(18 items\)"):
        e.scenario_action_faults_set((adr, t, elem[:-1], op, ordinal, value))
    with pytest.raises(ValueError, match=r"scenario_action_faults_set: the item arrays are longer than their row addresses \(18 items\)"):
        e.scenario_action_faults_set((adr, t, elem, op, ordinal, np.concatenate([value, value])))
    with pytest.raises(ValueError, match=r"scenario_action_faults_set: adr must be \[S \+ 1\]"):
        e.scenario_action_faults_set((adr.reshape(1, -1), t, elem, op, ordinal, value))


# ------------------------------------------------------------------------------------------------------------ the validator, as host C++
VALIDATE_CPP = r"""
#include <stdio.h>
#include "cosim_tables.h"
// in: nu S | adr[S+1] | n x (t0 t1 elem op ord value_bits); out: the refusal (empty line: none) and the packed words
int main() {
  long long v; std::vector<long long> w;
  while (scanf("%lld", &v) == 1) w.push_back(v);
  size_t k = 0;
  const int nu = (int)w[k++], S = (int)w[k++];
  std::vector<int32_t> adr(S + 1);
  for (auto& x : adr) x = (int32_t)w[k++];
  const size_t n = (w.size() - k) / 6;
  std::vector<int32_t> t(2 * n + 1), elem(n + 1), op(n + 1), ord(n + 1); std::vector<float> value(n + 1);
  for (size_t i = 0; i < n; i++) {
    t[2 * i] = (int32_t)w[k++]; t[2 * i + 1] = (int32_t)w[k++]; elem[i] = (int32_t)w[k++]; op[i] = (int32_t)w[k++]; ord[i] = (int32_t)w[k++];
    const unsigned u = (unsigned)w[k++]; memcpy(&value[i], &u, 4);
  }
  const cosim::FltRaw raw = {S, adr.data(), t.data(), elem.data(), op.data(), ord.data(), value.data()};
  const cosim::FltShape s = cosim::validate_action_faults(nu, raw);
  printf("%s\n", s.err.c_str());
  if (s.err.empty()) { printf("%d", s.n); for (int32_t x : s.item) printf(" %u", (unsigned)x); printf("\n"); }
  return 0;
}
"""


@pytest.fixture(scope="module")
def validate_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("actfault_validate")
    src, exe = str(tmp / "validate.cpp"), str(tmp / "validate")
    with open(src, "w") as f:
        f.write(VALIDATE_CPP)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe, src])
    return exe


def _validate(exe, nu, adr, items):
    words = [nu, len(adr) - 1] + list(adr)
    for t0, t1, e, op, o, v in items:
        words += [t0, t1, e, op, o, int(np.array(v, dtype=f32).view(np.uint32))]
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.split("\n")
    return lines[0], ([int(x) for x in lines[1].split()] if not lines[0] else None)


def test_engine_validator_messages_and_packed_records(validate_exe):
    """validate_action_faults of csrc/cosim_tables.h, the code cosim_set_param "action_faults" runs before anything changes, as a
    stand-alone sanitized host program: every refusal by message, and the 16-byte records with their padding."""
    ok = (0, 5, 1, 1, 0, 0.5)
    err, words = _validate(validate_exe, NU, [0, 1, 2], [ok, (3, 4, 5, 6, 7, 0.25)])
    bits = lambda v: int(np.array(v, dtype=f32).view(np.uint32))    # noqa: E731
    assert err == "" and words == [2, 0, 5, 1 | 1 << 16, bits(0.5), 3, 4, 5 | 6 << 16 | 7 << 24, bits(0.25)] + [0] * 12
    pre = 'cosim_set_param "action_faults": scenario 1, action-fault item 0: '
    for item, message in [((0, 5, 6, 1, 0, 0.5), pre + "actuator 6 out of range: the model has 6 actuators"),
                          ((0, 5, -1, 1, 0, 0.5), pre + "actuator -1 out of range: the model has 6 actuators"),
                          ((5, 5, 0, 1, 0, 0.5), pre + "t1 5 is not after t0 5"),
                          ((-1, 5, 0, 1, 0, 0.5), pre + "times outside [0, 2^30)"),
                          ((0, 5, 0, 7, 0, 0.5), pre + "unknown op 7 (0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop, 6 clip)"),
                          ((0, 5, 0, -1, 0, 0.5), pre + "unknown op -1 (0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop, 6 clip)"),
                          ((0, 5, 0, 1, 0, np.inf), pre + "value is not finite"),
                          ((0, 5, 0, 2, 0, np.nan), pre + "value is not finite"),
                          ((0, 5, 0, 3, 0, -0.5), pre + "a noise amplitude must be >= 0"),
                          ((0, 5, 0, 6, 0, -0.5), pre + "a clip bound must be >= 0"),
                          ((0, 5, 0, 5, 0, 1.5), pre + "a drop probability must lie in [0, 1]"),
                          ((0, 5, 0, 1, 256, 0.5), pre + "ordinal 256 outside 0..255")]:
        assert _validate(validate_exe, NU, [0, 1, 2], [ok, item])[0] == message
    assert _validate(validate_exe, NU, [0, 257], [ok] * 257)[0] == 'cosim_set_param "action_faults": scenario 0: 257 action-fault items, at most 256'
    assert _validate(validate_exe, NU, [0, 256], [ok] * 256)[0] == ""
    assert _validate(validate_exe, NU, [0, 2, 1], [ok, ok])[0] == 'cosim_set_param "action_faults": scenario 1: row addresses must not decrease'
    assert _validate(validate_exe, NU, [1, 2], [ok, ok])[0] == 'cosim_set_param "action_faults": adr[0] must be 0'
    assert _validate(validate_exe, NU, [0, 0, 0], [])[0] == 'cosim_set_param "action_faults": the table holds no action-fault item (n_scn = 0 clears the faults)'


# ------------------------------------------------------------------------------------------------------------ the kernels' body, as host C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "actfault_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/actfault_lanes.cpp + csrc/cosim_actfault.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("actfault")
    return _build(tmp, "actfault_lanes", []), _build(tmp, "actfault_lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                                 "-fno-omit-frame-pointer"])


def _item_words(table):
    adr, t, elem, op, ordinal, value = table.pack_action_faults()
    key = elem.astype(np.uint32) | (op.astype(np.uint32) << 16) | (ordinal.astype(np.uint32) << 24)
    words = np.stack([t[:, 0].astype(np.uint32), t[:, 1].astype(np.uint32), key, value.view(np.uint32)], axis=1)
    return adr, words


def _run_lanes(exe, table, mode, env_id0, nu, obs, env, ep, t, sc, raw, lastact):
    from cosim_amd.scenario import MODES
    adr, item = _item_words(table)
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    sd, S_, fd, e0, scale = obs
    words = [len(table), MODES[mode], env_id0, len(item)] + adr.tolist() + item.reshape(-1).tolist()
    words += [nu, SEED & 0xFFFFFFFF, SEED >> 32, sd, S_, fd, e0] + u(scale) + [len(env)]
    for i in range(len(env)):
        words += [int(env[i]), int(ep[i]), int(t[i]), int(sc[i])] + u(raw[i]) + u(lastact[i])
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = np.array([[int(x) for x in line.split()] for line in p.stdout.strip().splitlines()], dtype=np.int64)
    so = S_ * sd + fd - sd
    assert rows.shape == (len(env), 1 + nu + fd + sd + so)
    w = rows[:, 1:].astype(np.uint32).view(f32)
    return rows[:, 0].astype(np.int32), w[:, :nu], w[:, nu:nu + fd], w[:, nu + fd:nu + fd + sd], w[:, nu + fd + sd:]


RANDOM_TABLES = {
    6: [{"action_faults": [[2, 6, "*", "bias", 0.05], [3, 5, 1, "scale", -2.0], [1, 4, "*", "noise", 0.3], [4, 9, 0, "hold", 0.0],
                           [0, 3, 2, "set", -1.0], [1, 9, "*", "drop", 0.5], [5, 7, 3, "bias", 1.0], [0, 9, "*", "clip", 0.6]]},
        {},
        {"action_faults": [[0, 9, "*", "drop", 0.3], [0, 2, 0, "hold", 0.0], [0, 1, "*", "noise", 1.0], [2, 3, 5, "clip", 0.0]]}],
    # the widest model a wave serves and a one-actuator one; five items per scenario 0: a chunk and a part of the next
    64: [{"action_faults": [[0, 9, "*", "noise", 0.5], [1, 9, 63, "hold", 0.0], [2, 4, "*", "drop", 0.5], [0, 9, 17, "clip", 0.1]]}, {}, {}],
    1: [{"action_faults": [[0, 3, 0, "bias", 1.0], [1, 9, 0, "drop", 0.5], [2, 9, 0, "scale", 0.5], [3, 9, 0, "clip", 1.0], [4, 9, 0, "noise", 0.1]]},
        {"action_faults": [[1, 2, 0, "hold", 0.0]]}, {}],
}


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("nu", [6, 64, 1])
def test_kernel_body_as_host_cpp_equals_the_twin(lanes_exes, nu, sanitized):
    """A run of nine steps (two episodes) of twelve envs through the functions the kernels call, lane = actuator: the test plays the
    step kernel (s_lastact = the effective action it was handed, zeros after an episode's end), the program computes the effective
    action and the restored last_action words, and both equal the twin's as uint32 at every step."""
    from cosim_amd.scenario import ScenarioTable, reference_action_faults, scenario_rows
    act = [f"a{j}" for j in range(nu)]
    T = ScenarioTable(RANDOM_TABLES[nu], CD, names={"action_faults": act})
    exe = lanes_exes[1 if sanitized else 0]
    rng = np.random.default_rng(nu)
    N, env_id0 = 12, 7
    env = np.arange(N)
    t_run = np.array([0, 1, 2, 3, 4, 5, 0, 1, 2])
    # last_action as the frame elements [e0, e0 + nu): stacked (sd covers it) for nu 6 and 1, non-stacked for nu 64
    obs = {6: (16, 3, 20, 8, f32(0.25)), 64: (5, 2, 70, 6, f32(1.0)), 1: (3, 1, 3, 2, f32(-2.0))}[nu]
    sd, S_, fd, e0, scale = obs
    for mode in ("env", "cycle"):
        K = len(t_run)
        ep = (np.arange(K) >= 6).astype(np.int64) + 3
        lastact = np.zeros((N, nu), dtype=f32)
        touched = 0
        for k in range(K):
            sc = k * 3 + 11 + env
            raw = rng.uniform(-1.0, 1.0, size=(N, nu)).astype(f32)
            if k == 4:
                raw[2, min(4, nu - 1)] = np.nan                     # a NaN from the policy stays a NaN through bias, drop and clip
            t = np.full(N, t_run[k])
            if t_run[k] == 0:
                lastact[:] = 0.0                                    # the step that ended the episode left zeros
            want = reference_action_faults(T, mode, env + env_id0, t, np.full(N, ep[k]), sc, SEED, raw, lastact)
            row, eff, cache, stack, out = _run_lanes(exe, T, mode, env_id0, nu, obs, env, np.full(N, ep[k]), t, sc, raw, lastact)
            assert np.array_equal(row, scenario_rows(3, mode, env + env_id0, np.full(N, ep[k])))
            assert np.array_equal(eff.view(np.uint32), want.view(np.uint32)), (mode, k, np.nonzero(eff.view(np.uint32) != want.view(np.uint32)))
            touched += int((eff.view(np.uint32) != raw.view(np.uint32)).sum())
            # the restore: raw * scale in the cache, stack row 0 and the newest frame of state_out, nothing else
            v = (raw * scale).astype(f32)
            want_cache = np.zeros((N, fd), dtype=f32)
            want_cache[:, e0:e0 + nu] = v
            assert np.array_equal(cache.view(np.uint32), want_cache.view(np.uint32))
            want_stack, want_out = np.zeros((N, sd), dtype=f32), np.zeros((N, S_ * sd + fd - sd), dtype=f32)
            for j in range(nu):
                e = e0 + j
                if e < sd:
                    want_stack[:, e] = v[:, j]
                    want_out[:, e] = v[:, j]
                else:
                    want_out[:, S_ * sd + e - sd] = v[:, j]
            assert np.array_equal(stack.view(np.uint32), want_stack.view(np.uint32)) and np.array_equal(out.view(np.uint32), want_out.view(np.uint32))
            lastact = eff.copy()
        assert touched > 20


# ------------------------------------------------------------------------------------------------------------ kernel resources, code size
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip() for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/obsfault_kres_this.txt, the parent's table) and after (actfault_kres_this.txt): every existing
    kernel's line is identical, in the same order; the two added lines are the action-fault kernels', which use no LDS, no scratch
    and spill nothing."""
    head_a, a = _table_file("obsfault_kres_this.txt")
    head_b, b = _table_file("actfault_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["actfault_obs_kernel", "actfault_step_kernel"], sorted(added)
    for name in added:
        vgpr, agpr, sspill, vspill, scratch, occ, lds = added[name]
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 64 and occ == 8, name


def test_code_size_of_existing_kernels_is_unchanged():
    """tools/ksize.py --lib before and after: the same kernels with the same bytes, plus the two new ones."""
    head_a, a = _table_file("obsfault_ksize_this.txt")
    head_b, b = _table_file("actfault_ksize_this.txt")
    assert head_a == head_b and len(a) >= 40
    new = [ln for ln in b if "actfault_" in ln]
    assert len(new) == 2 and [ln for ln in b if ln not in new] == a


# ------------------------------------------------------------------------------------------------------------ one core under both kinds
BOTH_CPP = r"""
#include <stdio.h>
#include "cosim_tables.h"
// in: kind (0 observation, 1 action) width S | adr[S+1] | n x (t0 t1 elem op ord value_bits); out: the refusal (empty line: none).
// width: nu, or the elements of a frame that is all stacked, two rows deep, and holds no command word
int main() {
  long long v; std::vector<long long> w;
  while (scanf("%lld", &v) == 1) w.push_back(v);
  size_t k = 0;
  const int kind = (int)w[k++], width = (int)w[k++], S = (int)w[k++];
  std::vector<int32_t> adr(S + 1);
  for (auto& x : adr) x = (int32_t)w[k++];
  const size_t n = (w.size() - k) / 6;
  std::vector<int32_t> t(2 * n + 1), elem(n + 1), op(n + 1), ord(n + 1); std::vector<float> value(n + 1);
  for (size_t i = 0; i < n; i++) {
    t[2 * i] = (int32_t)w[k++]; t[2 * i + 1] = (int32_t)w[k++]; elem[i] = (int32_t)w[k++]; op[i] = (int32_t)w[k++]; ord[i] = (int32_t)w[k++];
    const unsigned u = (unsigned)w[k++]; memcpy(&value[i], &u, 4);
  }
  const cosim::FltRaw raw = {S, adr.data(), t.data(), elem.data(), op.data(), ord.data(), value.data()};
  const std::vector<unsigned char> field(width, 0);
  const cosim::ObsDims dims = {width, width, 2, field.data(), 1};
  const cosim::FltShape s = kind == 0 ? cosim::validate_faults(dims, raw) : cosim::validate_action_faults(width, raw);
  printf("%s\n", s.err.c_str());
  return 0;
}
"""


@pytest.fixture(scope="module")
def both_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fault_validate_both")
    src, exe = str(tmp / "both.cpp"), str(tmp / "both")
    with open(src, "w") as f:
        f.write(BOTH_CPP)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe, src])
    return exe


def _both(exe, kind, adr, items):
    words = [kind, NU, len(adr) - 1] + list(adr)
    for t0, t1, e, op, o, v in items:
        words += [t0, t1, e, op, o, int(np.array(v, dtype=f32).view(np.uint32))]
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout.split("\n")[0]


_OK = (0, 5, 1, 1, 0, 0.5)
MALFORMED_TABLES = {
    "bad window": ([0, 1, 2], [_OK, (5, 5, 0, 1, 0, 0.5)]),
    "negative time": ([0, 1, 2], [_OK, (-1, 5, 0, 1, 0, 0.5)]),
    "non-finite value": ([0, 1, 2], [_OK, (0, 5, 0, 2, 0, np.nan)]),
    "negative noise": ([0, 1, 2], [_OK, (0, 5, 0, 3, 0, -0.5)]),
    "drop above 1": ([0, 1, 2], [_OK, (0, 5, 0, 5, 0, 1.5)]),
    "drop below 0": ([0, 1, 2], [_OK, (0, 5, 0, 5, 0, -0.5)]),
    "ordinal 256": ([0, 1, 2], [_OK, (0, 5, 0, 1, 256, 0.5)]),
    "257 items": ([0, 257], [_OK] * 257),
    "decreasing addresses": ([0, 2, 1], [_OK, _OK]),
    "adr[0] not 0": ([1, 2], [_OK, _OK]),
    "empty table": ([0, 0, 0], []),
}


@pytest.mark.parametrize("case", sorted(MALFORMED_TABLES))
def test_both_validators_refuse_the_same_rows_in_the_same_words(both_exe, case):
    """validate_faults and validate_action_faults (csrc/cosim_tables.h) are entry points of one core: a table that is malformed in a
    way that is no kind's own is refused by both, in the same words but for the setter's name and the noun."""
    adr, items = MALFORMED_TABLES[case]
    obs, act = _both(both_exe, 0, adr, items), _both(both_exe, 1, adr, items)
    assert obs.startswith('cosim_set_param "obs_faults": ') and act.startswith('cosim_set_param "action_faults": ')
    assert "action" not in obs
    assert act.replace('cosim_set_param "action_faults"', 'cosim_set_param "obs_faults"').replace("action-fault item", "fault item") == obs
    assert _both(both_exe, 0, [0, 1], [_OK]) == "" and _both(both_exe, 1, [0, 1], [_OK]) == ""


MALFORMED_ROWS = {
    "value no number": [0, 1, 0, "bias", "much"],
    "nan": [0, 1, 0, "bias", float("nan")],
    "inf as float32": [0, 1, 0, "set", 1e39],
    "fractional time": [0.5, 1, 0, "bias", 1.0],
    "negative time": [-1, 1, 0, "bias", 1.0],
    "bad window": [5, 5, 0, "bias", 1.0],
    "negative noise": [0, 1, 0, "noise", -0.1],
    "drop above 1": [0, 1, 0, "drop", 1.5],
    "drop below 0": [0, 1, 0, "drop", -0.5],
    "float index": [0, 1, 1.0, "bias", 1.0],
    "bool index": [0, 1, True, "bias", 1.0],
    "name no string": [0, 1, 0, "bias", 1.0, 7],
    "op no string": [0, 1, 0, 3, 1.0],
}


@pytest.mark.parametrize("case", sorted(MALFORMED_ROWS))
def test_both_kinds_of_row_are_refused_in_the_same_words(case):
    """The one row checker of cosim_amd/scenario.py under "faults" and "action_faults": the same malformed row, with and without the
    obs column, is refused in the same words but for the noun, what an index may be, the op list and the echo of the row."""
    from cosim_amd.scenario import ScenarioTable
    row = MALFORMED_ROWS[case]
    msg = {}
    for key, r in (("action_faults", row), ("faults", row[:2] + ["ang_vel"] + row[2:])):
        with pytest.raises(ValueError) as err:
            ScenarioTable([{}, {key: [r]}], CD)
        msg[key] = str(err.value).split(", got ")[0].split(" (one of ")[0]
    assert msg["action_faults"].startswith("ScenarioTable: scenario 1, action-fault item 0: ")
    assert msg["action_faults"].replace("action-fault item", "fault item").replace("an int, an actuator name or '*'", "an int or '*'") == msg["faults"]


def test_clip_stays_an_action_op(both_exe):
    """Op 6 is the actions' alone: the observation validator and the "faults" rows refuse it in the words they had."""
    from cosim_amd.scenario import ACTION_FAULT_OPS, FAULT_OPS, ScenarioTable
    assert "clip" not in FAULT_OPS and ACTION_FAULT_OPS["clip"] == 6 and {k: ACTION_FAULT_OPS[k] for k in FAULT_OPS} == FAULT_OPS
    assert _both(both_exe, 0, [0, 1], [(0, 5, 0, 6, 0, 0.25)]) == ('cosim_set_param "obs_faults": scenario 0, fault item 0: unknown op 6 '
                                                                  "(0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop)")
    assert _both(both_exe, 1, [0, 1], [(0, 5, 0, 6, 0, 0.25)]) == ""
    with pytest.raises(ValueError, match=r"scenario 0, fault item 0: unknown op 'clip' \(one of scale, bias, set, noise, hold, drop\)"):
        ScenarioTable([{"faults": [[0, 1, "ang_vel", 0, "clip", 0.25]]}], CD)
    with pytest.raises(ValueError, match=r"scenario 0, fault item 0: unknown op 6 \(one of scale, bias, set, noise, hold, drop\)"):
        ScenarioTable([{"faults": [[0, 1, "ang_vel", 0, 6, 0.25]]}], CD)


# ------------------------------------------------------------------------------------------------------------ the shared walk: resources, code size
FAULT_KERNELS = ("obsfault_step_kernel", "actfault_step_kernel", "actfault_obs_kernel")


def test_shared_walk_keeps_the_fault_kernels_resources_and_changes_no_other_kernel():
    """tools/kres.py of the parent (profiles/actfault_kres_this.txt) and with the walk shared (fault_core_kres_this.txt): every other
    kernel's line is identical, in the same order; the three fault kernels keep 0 AGPRs, spills, scratch and LDS and occupancy 8, with
    no more VGPRs than the parent's build."""
    head_a, a = _table_file("actfault_kres_this.txt")
    head_b, b = _table_file("fault_core_kres_this.txt")
    other = lambda lines: [ln for ln in lines if ln.split("(")[0] not in FAULT_KERNELS]   # noqa: E731
    assert head_a == head_b and len(a) >= 40 and other(a) == other(b)
    assert [ln.split("(")[0] for ln in a] == [ln.split("(")[0] for ln in b]
    res = lambda lines: {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in lines if ln.split("(")[0] in FAULT_KERNELS}   # noqa: E731
    before, after = res(a), res(b)
    assert sorted(before) == sorted(after) == sorted(FAULT_KERNELS)
    for name in FAULT_KERNELS:
        vgpr, agpr, sspill, vspill, scratch, occ, lds = after[name]
        print(name, "VGPRs", before[name][0], "->", vgpr)
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and occ == 8 and vgpr <= before[name][0], name


def test_shared_walk_adds_no_code_bytes():
    """tools/ksize.py --lib of the parent (profiles/actfault_ksize_this.txt) and with the walk shared (fault_core_ksize_this.txt): every
    other kernel has the bytes it had, in the same order; no fault kernel has more code bytes than in the parent's build."""
    head_a, a = _table_file("actfault_ksize_this.txt")
    head_b, b = _table_file("fault_core_ksize_this.txt")
    is_fault = lambda ln: any(k + "(" in ln for k in FAULT_KERNELS)   # noqa: E731
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in a if not is_fault(ln)] == [ln for ln in b if not is_fault(ln)]
    size = lambda lines: {ln.split()[1].split("(")[0]: int(ln.split()[0]) for ln in lines if is_fault(ln)}   # noqa: E731
    before, after = size(a), size(b)
    assert sorted(before) == sorted(after) == sorted(FAULT_KERNELS)
    for name in FAULT_KERNELS:
        print(name, "bytes", before[name], "->", after[name])
        assert after[name] <= before[name], name
