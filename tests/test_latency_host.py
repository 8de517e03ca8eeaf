"""Latency lines of a scenario table on the host (no GPU): the numpy twin (cosim_amd/scenario.py LatencyTwin) against expectations
written out by hand, the jitter draws against cosim_amd/rng.py, the word table and its round trip, the sweep generator's new axis, the
refusals by message -- the engine validator's (csrc/cosim_tables.h) from a stand-alone sanitized C++ program --, the kernels' per-env
body (csrc/cosim_latency.h) compiled as plain C++ and driven lane by lane against the twin, once more under AddressSanitizer and
UBSan as a stand-alone child process, and the kernel-resource and code-size tables recorded before and after the change."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CD = 2
f32 = np.float32
SEED = 0x1234_5678_9ABC
ACT = ["hip_l", "knee_l", "wheel_l", "hip_r"]
NU = len(ACT)
NAMES = {"stacked": [("dof_pos", 2), ("ang_vel", 3), ("command", 2)], "non_stacked": [("height", 1)], "stack_size": 3}
FD = 8


def _table(rows, act=ACT, names=NAMES):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(rows, CD, names={"latency": (names, act)})


def _u(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


HAND = [
    {"latency": [[0, 100, "action", 0, 1],                          # 0: one step late throughout
                 [0, 100, "action", "knee_l", 3],                   # 1: three steps late
                 [0, 100, "action", 2, 0],                          # 2: delay 0 keeps the element's own bits
                 [4, 6, "action", "hip_r", 2, "late_hip"],          # 3: a window that opens in mid-episode delivers the history before it
                 [0, 100, "ang_vel", "*", 1],                       # 4: all three words one step late
                 [5, 100, "ang_vel", 1, 2],                         # 5: listed later: wins on element 3 from clock 5 on
                 {"t0": 0, "t1": 100, "channel": "height", "steps": 20}]},   # 6: at least the episode: never delivered
    {},
]


def test_twin_against_hand_written_table():
    from cosim_amd.scenario import LATENCY_ACTION, LATENCY_OBS, LatencyTwin
    T = _table(HAND)
    assert T.has_latency and T.n_latency_items == 4 + 3 + 1 + 1 and T.latency_depth == 21 and T.latency[1] == []
    assert T.latency[0][3] == (4, 6, LATENCY_ACTION, 3, 3, 2, 0) and T.latency[0][4:7] == [(0, 100, LATENCY_OBS, 2 + i, 4, 1, 0) for i in range(3)]
    K = 8
    tw = LatencyTwin(T, "env", [0, 1], SEED, NU, FD)
    raw = (np.arange(K)[:, None, None] * 10 + np.arange(NU)[None, None, :] + 1).astype(f32) * np.ones((1, 2, 1), dtype=f32)   # step k, actuator j -> 10 k + j + 1
    frames = (np.arange(K + 1)[:, None, None] * 10 + np.arange(FD)[None, None, :] + 0.5).astype(f32) * np.ones((1, 2, 1), dtype=f32)
    zero = np.zeros(2, dtype=np.int64)
    first = tw.step_obs(frames[0], zero, zero, zero + 7)
    assert np.array_equal(_u(first), _u(frames[0]))                 # a reset's observation is its own
    for k in range(K):
        eff = tw.step_actions(raw[k], zero + k, zero, zero + 7 + k)
        assert np.array_equal(_u(eff[1]), _u(raw[k, 1]))            # scenario 1 lists nothing: the caller's bits
        want = raw[k, 0].copy()
        want[0] = raw[k - 1, 0, 0] if k >= 1 else 0.0               # nothing has arrived yet after a reset
        want[1] = raw[k - 3, 0, 1] if k >= 3 else 0.0
        if 4 <= k < 6:
            want[3] = raw[k - 2, 0, 3]                              # clocks 2 and 3: written to the line before the window opened
        assert np.array_equal(_u(eff[0]), _u(want)), k
        obs = tw.step_obs(frames[k + 1], zero + k + 1, zero, zero + 8 + k)
        t = k + 1
        want = frames[t, 0].copy()
        want[2:5] = frames[t - 1, 0, 2:5]
        if t >= 5:
            want[3] = frames[t - 2, 0, 3]                           # the last listed item that holds wins; delays do not compose
        want[7] = frames[0, 0, 7]                                   # the channel is full of its first reading
        assert np.array_equal(_u(obs[0]), _u(want)), t
        assert np.array_equal(_u(obs[1]), _u(frames[t, 1]))


def test_cycle_changes_the_row_and_a_cut_restarts_the_line():
    from cosim_amd.scenario import LatencyTwin
    T = _table([{"latency": [[0, 100, "action", "*", 2], [0, 100, "dof_pos", 0, 2]]}, {}])
    tw = LatencyTwin(T, "cycle", [0], SEED, NU, FD)
    one = np.ones(1, dtype=np.int64)
    raw = lambda k: np.full((1, NU), k + 1, dtype=f32)              # noqa: E731
    fr = lambda k: np.full((1, FD), k + 0.5, dtype=f32)             # noqa: E731
    # episode 0 (row 0), clocks 0..3
    got = [tw.step_actions(raw(k), one * k, one * 0, one * k)[0, 0] for k in range(4)]
    assert got == [0.0, 0.0, 1.0, 2.0]
    # episode 1 runs row 1: nothing listed, the caller's bits; episode 2 is row 0 again and starts from an empty channel
    assert tw.step_actions(raw(10), one * 0, one * 1, one * 4)[0, 0] == 11.0
    got = [tw.step_actions(raw(20 + k), one * k, one * 2, one * (5 + k))[0, 0] for k in range(3)]
    assert got == [0.0, 0.0, 21.0]
    # a cut in mid-episode: the line restarts at the cut; the drives get the first word after it until the delayed one is there
    tw.cut()
    got = [tw.step_actions(raw(30 + k), one * (3 + k), one * 2, one * (8 + k))[0, 0] for k in range(4)]
    assert got == [31.0, 31.0, 31.0, 32.0]
    # observations: the first reading fills the channel, at a reset and after a cut alike
    got = [tw.step_obs(fr(k), one * k, one * 2, one * k)[0, 0] for k in range(4)]
    assert got == [0.5, 0.5, 0.5, 1.5]
    tw.cut(np.array([True]))
    got = [tw.step_obs(fr(10 + k), one * (4 + k), one * 2, one * k)[0, 0] for k in range(4)]
    assert got == [10.5, 10.5, 10.5, 11.5]
    assert tw.step_obs(fr(50), one * 8, one * 2, one * 9, active=np.array([False]))[0, 0] == 50.5   # not under the reset's mask: untouched


def test_jitter_draws_are_those_of_rng_and_reach_every_value():
    from cosim_amd import rng
    from cosim_amd.scenario import LatencyTwin
    T = _table([{"latency": [[0, 1000, "action", "*", 1, 2], [0, 1000, "dof_pos", "*", 0, 3]]}])
    N, K = 16, 24
    gid = 5 + np.arange(N)
    tw = LatencyTwin(T, "env", gid, SEED, NU, FD)
    raw = np.arange(K * N * NU, dtype=f32).reshape(K, N, NU) + 1
    fr = np.arange((K + 1) * N * FD, dtype=f32).reshape(K + 1, N, FD) + 0.5
    ep = np.zeros(N, dtype=np.int64)
    seen_a, seen_o = set(), set()
    tw.step_obs(fr[0], ep, ep, ep + 3)
    for k in range(K):
        sc = 3 + k + np.arange(N)
        j = rng.latency_jitter(rng.first_word(SEED, gid.astype(np.uint64), sc.astype(np.uint32), rng.PURPOSE_LATENCY, 0), 2)
        assert rng.PURPOSE_LATENCY == 9 and ((0 <= j) & (j <= 2)).all()
        eff = tw.step_actions(raw[k], ep + k, ep, sc)
        for i in range(N):
            d = 1 + int(j[i])
            want = raw[k - d, i] if k - d >= 0 else np.zeros(NU, dtype=f32)
            assert np.array_equal(eff[i], want), (k, i)             # all actuators of the listed item share the draw
        seen_a |= set(j.tolist())
        jo = rng.latency_jitter(rng.first_word(SEED, gid.astype(np.uint64), (sc + 1).astype(np.uint32), rng.PURPOSE_LATENCY, 1), 3)
        obs = tw.step_obs(fr[k + 1], ep + k + 1, ep, sc + 1)
        for i in range(N):
            assert np.array_equal(obs[i, :2], fr[max(k + 1 - int(jo[i]), 0), i, :2]) and np.array_equal(obs[i, 2:], fr[k + 1, i, 2:])
        seen_o |= set(jo.tolist())
    assert seen_a == {0, 1, 2} and seen_o == {0, 1, 2, 3}
    assert rng.latency_jitter(np.uint32(0), 63) == 0 and rng.latency_jitter(np.uint32(0xFFFFFFFF), 63) == 63


def test_word_table_round_trip_and_sweep_axis():
    from cosim_amd.scenario import ScenarioTable, sweep
    T = _table(HAND)
    w = T.pack_latency()
    assert w.dtype == np.int32 and w[0] == 2 and w[1:4].tolist() == [0, 4, 4] and w[4:7].tolist() == [0, 5, 5] and len(w) == 7 + 6 * 9
    assert w[7:13].tolist() == [0, 100, 0, 0, 1, 0] and w[7 + 6 * 4:7 + 6 * 5].tolist() == [0, 100, 2, 4, 1, 0] and w[-6:].tolist() == [0, 100, 7, 6, 20, 0]
    back = T.latency_from_words(w, NAMES, ACT)
    assert back.latency == T.latency and back.pack_latency().tolist() == w.tolist()
    assert back.to_list()[0]["latency"][4] == [0, 100, "ang_vel", "*", 1, 0] and "latency" not in back.to_list()[1]
    lst = T.to_list()
    assert lst[0]["latency"][3] == [4, 6, "action", "hip_r", 2, 0, "late_hip"] and lst[0]["latency"][6] == [0, 100, "height", "*", 20, 0]
    again = ScenarioTable(lst, CD, names={"latency": (NAMES, ACT)})
    assert again.latency == T.latency
    assert ScenarioTable(lst, CD).latency is None                   # kept as written until resolve_latency
    for other in (T.params_from_csr(*T.pack_params()), T.action_faults_from_csr(*T.pack_action_faults(), ACT), T.faults_from_csr(*T.pack_faults(), NAMES)):
        assert other.latency == T.latency and other.pack_latency().tolist() == w.tolist()   # the other ways back carry the expansion along
    with pytest.raises(ValueError, match="latency items are not resolved yet"):
        ScenarioTable(lst, CD).pack_latency()
    two, four = [[0, 1000, "action", "*", 2]], [[0, 1000, "action", "*", 4, 1, "jittery"]]
    sw = list(sweep([[0.5, 0.0], [1.0, 0.0]], search=[None, {"lo": 0.0, "hi": 1.0}], latency=[[], two, four]))
    assert len(sw) == 2 * 2 * 3
    assert ["latency" in s for s in sw[:3]] == [False, True, True] and sw[1]["latency"] == two and sw[2]["latency"] == four   # innermost
    assert "search" not in sw[0] and "search" in sw[3] and sw[6]["commands"] == [[0, 1.0, 0.0]]
    assert len(list(sweep([[0.5, 0.0]], latency=[]))) == 1


def test_refusals_name_the_scenario_and_the_item():
    cases = [
        ([0, 5, "command", 0, 1], r"scenario 1, latency item 0: channel 'command' is refused"),
        ([0, 5, "gyro", 0, 1], r"scenario 1, latency item 0: unknown channel 'gyro' \('action' or an observation: the env observes dof_pos, ang_vel, command, height\)"),
        ([0, 5, "action", 0, 60, 4], r"scenario 1, latency item 0: steps 60 \+ jitter 4 is more than 63"),
        ([0, 5, "action", 0, -1], r"scenario 1, latency item 0: steps -1 is negative"),
        ([0, 5, "action", 0, 1, -2], r"scenario 1, latency item 0: jitter -2 is negative"),
        ([0, 5, "action", 0, 1.5], r"scenario 1, latency item 0: steps must be an int, got 1.5"),
        ([0, 5, "action", 0, 1, 0.5], r"scenario 1, latency item 0: jitter must be an int, got 0.5"),
        ([0, 5, "action", 4, 1], r"scenario 1, latency item 0: index 4 out of range: the model has 4 actuators"),
        ([0, 5, "ang_vel", 3, 1], r"scenario 1, latency item 0: index 3 out of range: 'ang_vel' has 3 entries"),
        ([0, 5, "action", "elbow", 1], r"scenario 1, latency item 0: unknown actuator 'elbow'"),
        ([0, 5, "ang_vel", "x", 1], r"scenario 1, latency item 0: index must be an int or '\*'"),
        ([5, 5, "action", 0, 1], r"scenario 1, latency item 0: t1 5 is not after t0 5"),
        ([0, 5, "action", 0], r"scenario 1, latency item 0: expected \[t0, t1, channel, index, steps\]"),
    ]
    for item, msg in cases:
        with pytest.raises(ValueError, match=msg):
            _table([{}, {"latency": [item]}])
    with pytest.raises(ValueError, match=r"scenario 0: 260 action latency items after expansion, at most 256"):
        _table([{"latency": [[0, 5, "action", "*", 1]] * 65}])
    with pytest.raises(ValueError, match=r"scenario 0: 258 observation latency items after expansion, at most 256"):
        _table([{"latency": [[0, 5, "ang_vel", "*", 1]] * 86}])
    _table([{"latency": [[0, 5, "action", "*", 1]] * 64 + [[0, 5, "ang_vel", "*", 1]] * 85}])   # 256 + 255: the cap is per channel kind
    _table([{"latency": [[0, 5, "action", 0, 60, 3]]}], names=dict(NAMES, stack_size=1))        # 63 is allowed; no stack is needed


# ------------------------------------------------------------------------------------------------------------ the engine's validator
VALIDATE_CPP = r"""
#include <stdio.h>
#include "cosim_tables.h"
// in: nu frame_dim command_element S | act_adr[S+1] | obs_adr[S+1] | (na + no) x (t0 t1 el ord steps jitter); out: the refusal (empty
// line: none), max_delay and the packed records of both kinds
int main() {
  int nu, fd, cmd, S;
  if (scanf("%d %d %d %d", &nu, &fd, &cmd, &S) != 4 || S < 1 || fd < 1) return 2;
  std::vector<int32_t> act_adr(S + 1), obs_adr(S + 1);
  for (auto& x : act_adr) if (scanf("%d", &x) != 1) return 2;
  for (auto& x : obs_adr) if (scanf("%d", &x) != 1) return 2;
  const long long na = act_adr[S] > 0 ? act_adr[S] : 0, no = obs_adr[S] > 0 ? obs_adr[S] : 0;
  std::vector<int32_t> act(6 * na), obs(6 * no);
  for (auto& x : act) if (scanf("%d", &x) != 1) return 2;
  for (auto& x : obs) if (scanf("%d", &x) != 1) return 2;
  std::vector<unsigned char> field(fd, 0);
  if (cmd >= 0 && cmd < fd) field[cmd] = 9;
  const cosim::LatRaw raw = {S, act_adr.data(), obs_adr.data(), act.data(), obs.data()};
  const cosim::LatShape v = cosim::validate_latency(nu, {fd, fd, 1, field.data(), 9}, raw);
  printf("%s\n%d", v.err.c_str(), v.max_delay);
  if (v.err.empty()) {
    for (int32_t w : v.act_item) printf(" %u", (unsigned)w);
    for (int32_t w : v.obs_item) printf(" %u", (unsigned)w);
  }
  printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def validate_exe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("latency_validate")
    src, exe = str(tmp / "validate.cpp"), str(tmp / "validate")
    with open(src, "w") as f:
        f.write(VALIDATE_CPP)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe, src])
    return exe


def _validate(exe, act_adr, obs_adr, act, obs, nu=NU, fd=FD, cmd=5):
    words = [nu, fd, cmd, len(act_adr) - 1] + list(act_adr) + list(obs_adr) + [w for it in list(act) + list(obs) for w in it]
    p = subprocess.run([exe], input=" ".join(str(int(w)) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    err, rest = p.stdout.split("\n")[:2]
    rest = [int(x) for x in rest.split()]
    return err, rest[0], rest[1:]


def test_engine_validator_messages_equal_the_python_refusals(validate_exe):
    """validate_latency of csrc/cosim_tables.h, the code cosim_set_param "latency" runs before anything changes, as a stand-alone
    sanitized host program: the packed 16-byte records, and every refusal by message.  Where Python refuses the same malformed item
    (it names the listed item, the engine the expanded one of the channel kind) the words behind the item's name are equal."""
    ok = (0, 5, 1, 0, 2, 1)
    err, md, words = _validate(validate_exe, [0, 1, 2], [0, 0, 1], [ok, (3, 4, 3, 7, 60, 3)], [(1, 9, 7, 2, 0, 5)])
    assert err == "" and md == 63
    assert words == [0, 5, 1, 2 | 1 << 8, 3, 4, 3 | 7 << 16, 60 | 3 << 8, 1, 9, 7 | 2 << 16, 5 << 8]
    pre_a = 'cosim_set_param "latency": scenario 1, action latency item 0: '
    pre_o = 'cosim_set_param "latency": scenario 1, observation latency item 0: '

    def python_tail(item):
        with pytest.raises(ValueError) as ei:
            _table([{}, {"latency": [item]}])
        return str(ei.value).split("latency item 0: ", 1)[1]
    shared = [((0, 5, 0, 0, 60, 4), [0, 5, "action", 0, 60, 4], "steps 60 + jitter 4 is more than 63"),
              ((0, 5, 0, 0, -1, 0), [0, 5, "action", 0, -1], "steps -1 is negative"),
              ((0, 5, 0, 0, 1, -2), [0, 5, "action", 0, 1, -2], "jitter -2 is negative"),
              ((5, 5, 0, 0, 1, 0), [5, 5, "action", 0, 1], "t1 5 is not after t0 5")]
    for rec, item, tail in shared:
        assert _validate(validate_exe, [0, 0, 1], [0, 0, 0], [rec], [])[0] == pre_a + tail
        assert _validate(validate_exe, [0, 0, 0], [0, 0, 1], [], [rec])[0] == pre_o + tail
        assert python_tail(item) == tail
    for rec, message in [((0, 5, 4, 0, 1, 0), pre_a + "actuator 4 out of range: the model has 4 actuators"),
                         ((0, 5, -1, 0, 1, 0), pre_a + "actuator -1 out of range: the model has 4 actuators"),
                         ((-1, 5, 0, 0, 1, 0), pre_a + "times outside [0, 2^30)"),
                         ((0, 5, 0, 65536, 1, 0), pre_a + "ordinal 65536 outside 0..65535")]:
        assert _validate(validate_exe, [0, 0, 1], [0, 0, 0], [rec], [])[0] == message
    for rec, message in [((0, 5, 8, 0, 1, 0), pre_o + "element 8 out of range: the frame has 8 elements"),
                         ((0, 5, 5, 0, 1, 0), pre_o + "element 5 is a command word and is refused: the command words are the scenario's keyframes")]:
        assert _validate(validate_exe, [0, 0, 0], [0, 0, 1], [], [rec])[0] == message
    head = 'cosim_set_param "latency": '
    assert _validate(validate_exe, [0, 257], [0, 0], [ok] * 257, [])[0] == head + "scenario 0: 257 action latency items, at most 256"
    assert _validate(validate_exe, [0, 0], [0, 257], [], [ok] * 257)[0] == head + "scenario 0: 257 observation latency items, at most 256"
    assert _validate(validate_exe, [0, 256], [0, 256], [ok] * 256, [ok] * 256)[0] == ""
    assert _validate(validate_exe, [0, 2, 1], [0, 0, 0], [ok, ok], [])[0] == head + "scenario 1: row addresses must not decrease"
    assert _validate(validate_exe, [1, 2], [0, 0], [ok, ok], [])[0] == head + "act_adr[0] and obs_adr[0] must be 0"
    assert _validate(validate_exe, [0, 0, 0], [0, 0, 0], [], [])[0] == head + "the table holds no latency item (n_scn = 0 clears the latency)"


# ------------------------------------------------------------------------------------------------------------ the kernels' body, as host C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "latency_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/latency_lanes.cpp + csrc/cosim_latency.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("latency")
    return _build(tmp, "latency_lanes", []), _build(tmp, "latency_lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                               "-fno-omit-frame-pointer"])


def _records(table):
    """The 16-byte records of both kinds and their row addresses, from the word table."""
    w = table.pack_latency().astype(np.int64)
    S = int(w[0])
    act_adr, obs_adr = w[1:S + 2], w[S + 2:2 * S + 3]
    recs = w[2 * S + 3:].reshape(-1, 6)
    packed = np.stack([recs[:, 0], recs[:, 1], recs[:, 2] | recs[:, 3] << 16, recs[:, 4] | recs[:, 5] << 8], axis=1)
    return act_adr.tolist(), obs_adr.tolist(), packed[:int(act_adr[-1])].reshape(-1).tolist(), packed[int(act_adr[-1]):].reshape(-1).tolist()


def _lane_tables(nu, fd, big):
    act = [f"a{j}" for j in range(nu)]
    names = {"stacked": [("dof_pos", 3), ("ang_vel", 3)] if fd > 8 else [("dof_pos", 2)], "non_stacked": [("height", fd - 6 if fd > 8 else fd - 2)], "stack_size": 2}
    rows = [{"latency": [[0, 100, "action", "*", 1], [2, 9, "action", nu - 1, big, "wide"], [3, 7, "action", 0, 0, min(2, big)],
                         [0, 100, "dof_pos", "*", 1, min(1, big - 1)], [4, 100, "height", "*", big], [6, 100, "height", fd - 7 if fd > 8 else 0, 2 if big > 2 else 1]]},
            {},
            {"latency": [[0, 5, "action", 0, big], [1, 100, "dof_pos", 1, 1]]}]
    return _table(rows, act, names), names


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("nu, fd, D", [(1, 8, 2), (6, 65, 4), (64, 8, 64)])
def test_kernel_body_as_host_cpp_equals_the_twin(lanes_exes, nu, fd, D, sanitized):
    """40 steps of 7 envs (episodes of 12 steps, a cut in mid-episode) through the functions the kernels call: the program keeps the
    lines as the engine does, and its delivered actions and frames equal the twin's as uint32 at every step.  Widths 1, 6 and 64
    actuators; a frame of 65 elements takes two passes of 64 lanes; depths 2, 4 and 64."""
    from cosim_amd.scenario import MODES, LatencyTwin, scenario_rows
    T, names = _lane_tables(nu, fd, D - 1)
    assert T.latency_depth == D
    exe = lanes_exes[1 if sanitized else 0]
    sd = sum(d for _, d in names["stacked"])
    assert sd + sum(d for _, d in names["non_stacked"]) == fd
    N, K, env_id0, LIMIT = 7, 40, 5, 12
    rng = np.random.default_rng(nu + fd)
    raw = rng.uniform(-1, 1, size=(K, N, nu)).astype(f32)
    frames = rng.uniform(-1, 1, size=(K, N, fd)).astype(f32)
    act_adr, obs_adr, act_item, obs_item = _records(T)
    for mode in ("env", "cycle"):
        tw = LatencyTwin(T, mode, env_id0 + np.arange(N), SEED, nu, fd)
        words = [len(T), MODES[mode], env_id0, D, len(act_item) // 4, len(obs_item) // 4] + act_adr + obs_adr + act_item + obs_item
        words += [nu, fd, sd, 2, SEED & 0xFFFFFFFF, SEED >> 32, N, K]
        want, rows = [], []
        for k in range(K):
            t_pre, ep_pre = np.full(N, k % LIMIT), np.full(N, k // LIMIT)
            t_post, ep_post = np.full(N, (k + 1) % LIMIT), np.full(N, (k + 1) // LIMIT)
            sc = 100 + 3 * k + np.arange(N)
            cut = np.zeros(N, dtype=bool)
            if k == 17:
                cut[[0, 2, 3]] = True                               # clock 5 of the second episode
                tw.cut(cut)
            eff = tw.step_actions(raw[k], t_pre, ep_pre, sc)
            obs = tw.step_obs(frames[k], t_post, ep_post, sc + 1)
            want.append(np.concatenate([eff, obs], axis=1))
            rows.append((scenario_rows(3, mode, env_id0 + np.arange(N), ep_pre), scenario_rows(3, mode, env_id0 + np.arange(N), ep_post)))
            for i in range(N):
                words += [int(cut[i]), int(ep_pre[i]), int(t_pre[i]), int(sc[i])] + _u(raw[k, i]).tolist()
                words += [int(ep_post[i]), int(t_post[i]), int(sc[i]) + 1] + _u(frames[k, i]).tolist()
        p = subprocess.run([exe], input=" ".join(str(int(w)) for w in words), capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        out = np.array([[int(x) for x in line.split()] for line in p.stdout.strip().splitlines()], dtype=np.int64).reshape(K, N, 2 + nu + fd)
        want = np.stack(want)
        assert np.array_equal(out[:, :, 0], np.stack([r[0] for r in rows])) and np.array_equal(out[:, :, 1 + nu], np.stack([r[1] for r in rows]))
        got = np.concatenate([out[:, :, 1:1 + nu], out[:, :, 2 + nu:]], axis=2).astype(np.uint32)
        bad = np.argwhere(got != _u(want))
        assert len(bad) == 0, (mode, bad[:6])
        assert (_u(want[:, :, :nu]) != _u(raw)).any() and (_u(want[:, :, nu:]) != _u(frames)).any()


# ------------------------------------------------------------------------------------------------------------ kernel resources, code size
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return [ln.rstrip() for ln in f if ln.strip()]


NEW_KERNELS = ["latency_act_kernel", "latency_cut_kernel", "latency_obs_kernel"]


def test_kernel_resources_of_existing_kernels_are_unchanged_and_the_new_kernels_are_lean():
    """tools/kres.py on the parent commit (profiles/latency_kres_parent.txt) and on this one (latency_kres_this.txt): every existing
    kernel's line is identical, in the same order; the three added lines are the latency kernels', which use no LDS, no scratch, no
    AGPRs and spill nothing."""
    a, b = _table_file("latency_kres_parent.txt"), _table_file("latency_kres_this.txt")
    assert a[0] == b[0] and len(a) >= 40
    assert [ln for ln in b if "latency_" not in ln] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in ln.split()[-7:]] for ln in b if "latency_" in ln}
    assert sorted(added) == NEW_KERNELS
    for name, (vgpr, agpr, sspill, vspill, scratch, occ, lds) in added.items():
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 32 and occ == 8, name


def test_code_size_of_existing_kernels_is_unchanged():
    """tools/ksize.py --lib on the parent commit's library and on this one's: the same kernels with the same bytes, plus the three
    new ones, a few KB together."""
    a, b = _table_file("latency_ksize_parent.txt"), _table_file("latency_ksize_this.txt")
    assert a[:2] == b[:2] and len(a) >= 40
    new = [ln for ln in b if "latency_" in ln]
    assert sorted(ln.split()[1].split("(")[0] for ln in new) == NEW_KERNELS and [ln for ln in b if ln not in new] == a
    assert sum(int(ln.split()[0]) for ln in new) < 8192
