"""Scenario checks on the host (no GPU): the numpy twin of the check kernels (cosim_amd/checks.py reference_checks) against a
hand-written case in which every verdict class occurs; the kernels' per-item bodies (csrc/cosim_checks.h) compiled as plain C++ and
driven lane by lane against the twin, a second time under AddressSanitizer / UBSan as a stand-alone child process; validation
messages; the .npz round trip, summary, by_scenario, join and sweep(checks=...); and the kernel-resource tables recorded before and
after the change.  Every comparison is exact: float32 as bits, ints as ints."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
K, N, NU, CD, NQ, NV = 12, 4, 1, 1, 7, 6
NI = 4 + 2 * NU + 1
VX0 = [0.1, 0.2, 0.1, 0.9, 0.2, 0.45, 0.5, 0.4]                         # env 0, first episode: lin_vel_x at t = 0 .. 7

ROW0 = [[0, 8, "info", "lin_vel_x", "always", "<", 1.0, "vx_ok"],        # 0 passes
        [0, 8, "abs_info", 1, "always", "<", 0.5, "vx_small"],           # 1 fails, first at t = 3
        [2, 8, "tracking_error", 0, "settle", "<", 0.2, "track"],        # 2 settles after t = 4: settle time 3
        [2, 5, "tracking_error", 0, "settle", "<", 0.2, "track_short"],  # 3 bad at its last sample: fails
        [0, 8, "info", 1, "mean", "<", 0.45, "vx_mean"],                 # 4 mean 0.35625
        [4, 12, "up", 0, "always", ">", 0.9, "upright"],                 # 5 the episode ends inside the window: incomplete
        {"t0": 6, "t1": 8, "signal": "qvel", "index": "hip", "mode": "always", "op": "<", "bound": 10.0, "name": "qv"},   # 6 loses its done row
        [0, 8, "info", 2, "always", "<", 5.0, "nan"]]                    # 7 a NaN sample at t = 5 is not ok
ROW1 = [[0, 3, "torque_max", 0, "always", "<", 2.0, "torque"], [0, 4, "abs_qvel", 1, "mean", ">", 0.1], [0, 2, "qpos", 2, "settle", ">", 0.3, "height"]]
NAMES = {"info": {"action_diff_RMSE": (0, 1), "lin_vel_x": (1, 1), "lin_vel_y": (2, 1), "ang_vel_yaw": (3, 1), "torque": (4, NU), "set_points": (4 + NU, NU),
                  "state": (4 + 2 * NU, 1)}, "info_dim": NI, "command_dim": CD, "nq": NQ, "nv": NV, "qpos": {"root": 0}, "qvel": {"root": 0, "hip": 0}}


def _table(rows=(ROW0, ROW1)):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable([{"commands": [[0, 0.5]], "checks": list(r)} for r in rows], CD, names={"checks": NAMES})


def _hand_case():
    """12 steps of four envs under two scenarios (mode env: envs 0, 2 run row 0, envs 1, 3 row 1).
      env 0: truncated in step 7 (clock 7); the steps 8 .. 11 are an open episode at clocks 0 .. 3
      env 1: terminated in steps 3 and 9: two records (a ring of one slot loses the first)
      env 2: cut by a masked host reset before step 5 (no record); restored before step 9 with meta word 0 = 3 (flag 8, the clock
             starts from 3); terminated in step 11 at clock 5
      env 3: never ends"""
    rng = np.random.default_rng(7)
    c = {"info": rng.uniform(-1.0, 1.0, size=(K, N, NI)).astype(f32), "cmd": np.full((K, N, CD), 0.5, dtype=f32),
         "qpos": rng.uniform(-0.2, 0.2, size=(K, N, NQ)).astype(f32), "qvel": rng.uniform(-1.0, 1.0, size=(K, N, NV)).astype(f32)}
    c["qpos"][:, :, 2] += f32(0.6)
    c["info"][:8, 0, 1] = np.asarray(VX0, dtype=f32)
    c["info"][5, 0, 2] = np.nan
    te, tr = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    tr[7, 0] = 1
    te[[3, 9], 1] = 1
    te[11, 2] = 1
    c["term"], c["trunc"] = te, tr
    clock = np.zeros((K + 1, N), dtype=np.int32)                         # meta word 0 before step k; row K: after the last step
    clock[:, 0] = [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4]
    clock[:, 1] = [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 0, 1, 2]
    clock[:, 2] = [0, 1, 2, 3, 4, 0, 1, 2, 3, 3, 4, 5, 0]
    clock[:, 3] = np.arange(K + 1)
    c["clock"] = clock
    c["rows"] = np.tile(np.array([0, 1, 0, 1]), (K, 1))
    c["begins"] = [(5, np.array([0, 0, 1, 0], dtype=np.uint8), 0), (9, np.array([0, 0, 1, 0], dtype=np.uint8), 8)]
    c["ep"] = np.array([1, 2, 1, 0])                                     # meta word 11 at the end (mode env: the rows do not move)
    return c


def _twin(c, table, slots=2, **kw):
    from cosim_amd.checks import reference_checks
    return reference_checks(table, c["info"], c["term"], c["trunc"], c["cmd"], c["qpos"], c["qvel"], c["clock"], c["rows"], slots, NU,
                            begins=c.get("begins", ()), open_scenario_rows=c["rows"][-1], **kw)


# ------------------------------------------------------------------------------------------------------------ 1: the twin, by hand
def test_twin_against_hand_written_case():
    from cosim_amd.checks import NONE_BITS
    c, T = _hand_case(), _table()
    v = _twin(c, T)
    assert len(v) == 4 and v.env.tolist() == [0, 1, 1, 2] and v.episode.tolist() == [0, 0, 1, 0] and v.lost.tolist() == [0, 0, 0, 0]
    assert v.length.tolist() == [8, 4, 6, 3] and v.flags.tolist() == [2, 1, 1, 1 | 8] and v.scenario.tolist() == [0, 1, 1, 0]
    assert v.words.shape[1] == 8 + 2 * 8
    # env 0, its truncated episode: every class of verdict
    e = 0
    assert v.valid[e].all()
    assert v.failed[e].tolist() == [False, True, False, True, False, False, False, True] and v.words[e, 4] == 0x8A and v.words[e, 5] == 0
    assert v.incomplete[e].tolist() == [False] * 5 + [True, True, False] and v.words[e, 6] == 0x60
    assert v.passed[e].tolist() == [True, False, True, False, True, False, False, False]
    vx = np.asarray(VX0, dtype=f32)
    assert v.value[e, 0] == f32(0.9) and v.aux[e, 0] == -1                                   # always, passed
    assert v.value[e, 1] == f32(0.9) and v.aux[e, 1] == 3, "the first violation is at step 3"
    err = np.abs(f32(0.5) - vx)
    assert v.aux[e, 2] == 4 and v.settle_time[e, 2] == 3 and v.value[e, 2] == err[2:8].max()  # settle, non-zero settle time
    assert v.aux[e, 3] == 4 and v.settle_time[e, 3] == 3 and v.failed[e, 3], "bad at the last sample of [2, 5)"
    m = np.float64(0.0)
    for x in vx:
        m = m + np.float64(x)
    assert v.value[e, 4].view(np.int32) == f32(m / np.float64(8)).view(np.int32) and v.aux[e, 4] == 8   # mean, aux = n
    from cosim_amd.fall import up_component
    assert v.value[e, 5] == up_component(c["qpos"][4:7, 0]).min() and v.aux[e, 5] == -1     # three samples: steps 4, 5, 6
    assert v.value[e, 6] == c["qvel"][6, 0, 0], "the state signal took its sample at step 6 and none on the done row"
    assert v.aux[e, 7] == 5 and np.isfinite(v.value[e, 7]), "the NaN sample is a violation and never the extreme"
    assert v.value[e, 7] == np.nanmax(c["info"][:8, 0, 2])
    assert (v.settle_time[e, [0, 1, 4, 5, 6, 7]] == -1).all()
    # env 1: two episodes of row 1; items past the row's three are not valid and their words are zero
    assert v.valid[1].tolist() == [True] * 3 + [False] * 5 and (v.words[1, 8 + 6:] == 0).all()
    tq = np.abs(c["info"][:3, 1, 4])
    assert v.value[1, 0] == tq.max() and not v.failed[1, 0] and not v.incomplete[1, 0]
    assert v.aux[1, 1] == 3 and v.incomplete[1, 1], "abs_qvel mean over [0, 4): the done row at clock 3 is not sampled"
    # env 2: the cut episode left no record; the restart's clock began at meta word 0 = 3, so [2, 5) saw t = 3, 4 only
    e = 3
    assert v.incomplete[e, 3] and v.aux[e, 4] == 3 and v.incomplete[e, 4]                    # mean over [0, 8): t = 3, 4, 5
    assert v.aux[e, 6] == -1 and v.value[e, 6].view(np.int32) == NONE_BITS, "[6, 8) was never reached: no sample"
    assert np.isnan(v.value[e, 6]) and v.incomplete[e, 6]

    opn = _twin(c, T, include_open=True)
    o = (opn.flags & 16) != 0
    assert len(opn) == 8 and opn.env[o].tolist() == [0, 1, 2, 3] and opn.episode[o].tolist() == [1, 2, 1, 0]
    assert opn.length[o].tolist() == [4, 2, 0, 12] and opn.flags[o].tolist() == [16] * 4
    np.testing.assert_array_equal(opn.words[~o], v.words)
    assert opn.incomplete[o][0, :5].all() and opn.aux[o][0, 4] == 4                          # env 0 again at clocks 0 .. 3

    one = _twin(c, T, slots=1)                                                               # a ring of one slot loses env 1's first record
    assert one.lost.tolist() == [0, 1, 0, 0] and one.env.tolist() == [0, 1, 2] and one.episode.tolist() == [0, 1, 0]
    np.testing.assert_array_equal(one.words, v.words[[0, 2, 3]])
    first = _twin(c, T, initial_flags=8)                                                     # armed on a stepped fleet
    assert first.flags.tolist() == [2 | 8, 1 | 8, 1, 1 | 8]


# ------------------------------------------------------------------------------------------------------------ 2: container
def test_npz_summary_by_scenario_and_join(tmp_path):
    from cosim_amd.checks import Verdicts, same_verdicts
    from cosim_amd.ledger import reference_ledger
    c, T = _hand_case(), _table()
    v = _twin(c, T, include_open=True)
    path = str(tmp_path / "verdicts.npz")
    v.save(path)
    w = Verdicts.load(path)
    assert same_verdicts(v, w) is None and w.names == v.names and w.slots == 2
    for name in ("failed", "incomplete", "passed", "valid", "settle_time", "aux", "scenario"):
        np.testing.assert_array_equal(getattr(v, name), getattr(w, name))
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"words", "env", "lost", "names", "item_mode", "item_t", "header"}
    s = v.summary()
    assert s["episodes"] == 4 and s["episodes_failed"] >= 1 and s["lost"] == 0
    assert s["episodes_failed"] + s["episodes_incomplete"] + s["episodes_passed"] == 4
    assert s["items"] == 8 + 3 + 3 + 8 and s["items_passed"] + s["items_failed"] + s["items_incomplete"] == s["items"]
    assert s["checks"]["vx_small"]["failed"] >= 1 and s["checks"]["track"]["settle_time"]["max"] == 3
    assert s["checks"]["torque"]["items"] == 2 and abs(s["items_failed_share"] - s["items_failed"] / s["items"]) < 1e-12
    b = v.by_scenario()
    assert sorted(b) == [0, 1] and b[0]["episodes"] == 2 and b[1]["episodes"] == 2 and "height" in b[1]["checks"] and "track" in b[0]["checks"]
    assert b[0]["checks"]["track"]["settle_time"]["min"] >= 0
    led = reference_ledger(c["info"], c["term"], c["trunc"], c["cmd"], None, None, 4, NU, CD, begins=[(k, m, f) for k, m, f in c["begins"]],
                           scenario_rows=c["rows"])
    j = _twin(c, T).join(led)
    assert (j >= 0).all() and np.array_equal(led.env[j], _twin(c, T).env) and np.array_equal(led.episode[j], _twin(c, T).episode)
    assert np.array_equal(led.length[j], _twin(c, T).length) and np.array_equal(led.scenario[j], _twin(c, T).scenario)
    assert same_verdicts(v, _twin(c, T)) is not None


def test_sweep_checks_axis_and_packing():
    from cosim_amd.scenario import ScenarioTable, sweep
    ck = [[], [[155, 255, "tracking_error", 0, "settle", "<", 0.2, "recovers"], [0, 300, "up", 0, "always", ">", 0.8]]]
    scn = list(sweep([[0.5, 0.0, 0.0], [1.0, 0.0, 0.0]], [1.0], [0.0], [(150, 155)], checks=ck))
    assert len(scn) == 4 and "checks" not in scn[0] and scn[1]["checks"][0][7] == "recovers" and scn[3]["commands"] == [[0, 1.0, 0.0, 0.0]]
    T = ScenarioTable(scn, 3)
    adr, t, sig, idx, mode, cmp, bound = T.pack_checks()
    assert adr.tolist() == [0, 0, 2, 2, 4] and t.tolist() == [[155, 255], [0, 300]] * 2 and sig.tolist() == [2, 4, 2, 4]
    assert mode.tolist() == [1, 0, 1, 0] and cmp.tolist() == [0, 1, 0, 1] and bound.dtype == np.float32 and idx.tolist() == [0] * 4
    assert T.check_item_names()[1][0] == "recovers" and T.check_item_names()[1][1].startswith("up[0] always >")
    assert ScenarioTable(T.to_list(), 3).pack_checks()[1].tolist() == t.tolist()
    both = list(sweep([[0.5, 0.0, 0.0]], params=[[], [[0, 5, "kp", "*", "scale", 0.5]]], checks=ck))
    assert len(both) == 4 and "params" in both[2] and "checks" in both[3] and "checks" not in both[2]


def test_yaml_loading(tmp_path):
    yaml = pytest.importorskip("yaml")
    from cosim_amd.scenario import ScenarioTable
    p = tmp_path / "scn.yaml"
    p.write_text(yaml.safe_dump({"scenarios": [{"commands": [[0, 0.5]], "checks": [list(r) if not isinstance(r, dict) else r for r in ROW1]}]}))
    T = ScenarioTable.build(str(p), CD)
    assert T.has_checks and T.pack_checks()[2].tolist() == [3, 7, 5]


def test_validation_messages_name_the_scenario_and_the_item():
    from cosim_amd.scenario import ScenarioTable
    ok = [0, 5, "info", 1, "always", "<", 1.0]

    def bad(row, match, names=NAMES):
        with pytest.raises(ValueError, match=match):
            ScenarioTable([{}, {"checks": [ok, row]}], CD, names={"checks": names})
    bad([0, 5, "info", 1, "always", "<", float("nan")], r"scenario 1, check item 1: non-finite bound")
    bad([5, 5, "info", 1, "always", "<", 1.0], r"scenario 1, check item 1: t1 5 is not after t0 5")
    bad([-1, 5, "info", 1, "always", "<", 1.0], r"scenario 1, check item 1: times must be control steps")
    bad([0, 5, "speed", 1, "always", "<", 1.0], r"scenario 1, check item 1: unknown signal 'speed'")
    bad([0, 5, "info", 1, "often", "<", 1.0], r"scenario 1, check item 1: unknown mode 'often'")
    bad([0, 5, "info", 1, "always", "<=", 1.0], r"scenario 1, check item 1: unknown op '<='")
    bad([0, 5, "info", NI, "always", "<", 1.0], r"scenario 1, check item 1: index %d out of range: 'info' has %d entries" % (NI, NI))
    bad([0, 5, "tracking_error", 1, "always", "<", 1.0], r"check item 1: index 1 out of range: 'tracking_error' has 1 entries")
    bad([0, 5, "info", "speed", "always", "<", 1.0], r"scenario 1, check item 1: unknown info column 'speed'")
    bad([0, 5, "info", "torque[1]", "always", "<", 1.0], r"check item 1: 'torque\[1\]' out of range: 'torque' has 1 entries")
    bad([0, 5, "qpos", "knee", "always", "<", 1.0], r"scenario 1, check item 1: unknown joint 'knee'")
    bad([0, 5, "info", 1, "always", "<"], r"scenario 1, check item 1: expected \[t0, t1, signal, index, mode, op, bound\]")
    with pytest.raises(ValueError, match=r"scenario 0: 65 check items, at most 64"):
        ScenarioTable([{"checks": [ok] * 65}], CD)
    T = ScenarioTable([{"checks": [[0, 5, "qvel", "hip", "always", "<", 1.0]]}], CD)       # a name and no model yet: resolved later
    with pytest.raises(ValueError, match="not resolved yet"):
        T.pack_checks()
    assert T.resolve_checks(NAMES).pack_checks()[3].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------ 3: the header as C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "checks_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/checks_lanes.cpp + csrc/cosim_checks.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("checks")
    return _build(tmp, "checks_lanes", []), _build(tmp, "checks_lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                             "-fno-omit-frame-pointer"])


def _run_lanes(exe, c, table, slots, lanes, reverse, dims, initial_flags=0):
    from cosim_amd.checks import items_per_record
    n_envs, ni, nu, cd, nq, nv = dims
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    adr, t, sig, idx, mode, cmp, bound = table.pack_checks()
    I = items_per_record(table)
    words = [len(table), 0, 0, len(sig)] + adr.tolist() + t.reshape(-1).tolist() + sig.tolist() + idx.tolist() + mode.tolist() + cmp.tolist() + u(bound)
    words += [I, slots, lanes, n_envs, ni, nu, cd, nq, nv, int(reverse)]
    steps = c["info"].shape[0]
    words += [1, initial_flags] + [1] * n_envs + c["clock"][0].tolist()
    for k in range(steps):
        for kb, mask, flag in c.get("begins", ()):
            if kb == k:
                words += [1, flag] + np.asarray(mask).astype(int).tolist() + c["clock"][k].tolist()
        words.append(2)
        for i in range(n_envs):
            words += [int(c["term"][k, i]), int(c["trunc"][k, i]), int(c["rows"][k, i]), int(c["clock"][k + 1, i])]
            words += u(c["info"][k, i]) + u(c["cmd"][k, i]) + u(c["qpos"][k, i]) + u(c["qvel"][k, i])
    words += [3] + np.asarray(c["ep"]).astype(int).tolist()
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    ring, cnt, opn = (np.array(line.split(), dtype=np.int64).astype(np.int32) for line in p.stdout.strip().splitlines())
    W = 8 + 2 * I
    return ring.reshape(n_envs, slots, W), cnt, opn.reshape(n_envs, W)


def _random_case(seed=3):
    """8 envs, 30 steps, three scenarios -- 64 items, one item, 5 items -- in mode env; episodes end at random."""
    rng = np.random.default_rng(seed)
    n_envs, steps, nu, cd, nq, nv = 8, 30, 3, 2, 9, 8
    ni = 4 + 2 * nu + 2
    sigs = ["info", "abs_info", "tracking_error", "torque_max", "up", "qpos", "qvel", "abs_qvel"]

    def item():
        s = sigs[rng.integers(len(sigs))]
        width = {"info": ni, "abs_info": ni, "tracking_error": cd, "torque_max": 1, "up": 1, "qpos": nq, "qvel": nv, "abs_qvel": nv}[s]
        t0 = int(rng.integers(0, 8))
        return [t0, t0 + int(rng.integers(1, 8)), s, int(rng.integers(width)), ["always", "settle", "mean"][rng.integers(3)], "<>"[rng.integers(2)],
                float(f32(rng.uniform(-0.5, 0.8)))]
    from cosim_amd.scenario import ScenarioTable
    T = ScenarioTable([{"checks": [item() for _ in range(n)]} for n in (64, 1, 5)], cd)
    c = {"info": rng.uniform(-1.0, 1.0, size=(steps, n_envs, ni)).astype(f32), "cmd": rng.uniform(-1.0, 1.0, size=(steps, n_envs, cd)).astype(f32),
         "qpos": rng.uniform(-0.6, 0.6, size=(steps, n_envs, nq)).astype(f32), "qvel": rng.uniform(-1.0, 1.0, size=(steps, n_envs, nv)).astype(f32)}
    c["info"][rng.integers(steps, size=6), rng.integers(n_envs, size=6), rng.integers(ni, size=6)] = np.nan
    done = rng.uniform(size=(steps, n_envs)) < 0.12
    c["term"], c["trunc"] = (done & (rng.uniform(size=done.shape) < 0.5)).astype(np.uint8), done.astype(np.uint8)
    c["trunc"] = (c["trunc"] & ~c["term"]).astype(np.uint8)
    clock = np.zeros((steps + 1, n_envs), dtype=np.int32)
    for k in range(steps):
        clock[k + 1] = np.where(done[k], 0, clock[k] + 1)
    c["clock"], c["rows"] = clock, np.tile(np.arange(n_envs) % 3, (steps, 1))
    c["begins"], c["ep"] = [], done.sum(axis=0)
    return c, T, (n_envs, ni, nu, cd, nq, nv)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("lanes", [64, 5, 1])
def test_kernel_bodies_as_host_cpp_equal_the_twin(lanes_exes, lanes, sanitized):
    """The hand-written case and a random one with a 64-item scenario through the functions the kernels call, with 64 lanes (the
    wave), 5 and 1, the two ranges of a step in either order: rings, counts and open rows equal the twin's word for word."""
    from cosim_amd.checks import reference_checks
    exe = lanes_exes[1 if sanitized else 0]
    c, T = _hand_case(), _table()
    for slots, reverse, iflag in ((2, False, 0), (1, True, 8)):
        ring, cnt, opn = _run_lanes(exe, c, T, slots, lanes, reverse, (N, NI, NU, CD, NQ, NV), iflag)
        want = _twin(c, T, slots=slots, include_open=True, initial_flags=iflag)
        o = (want.flags & 16) != 0
        np.testing.assert_array_equal(opn, want.words[o])
        assert cnt.tolist() == [1, 2, 1, 0]
        from cosim_amd.checks import Verdicts
        got = Verdicts.from_raw(ring, cnt, opn, T)
        np.testing.assert_array_equal(got.words, want.words)
        np.testing.assert_array_equal(got.lost, want.lost)
    c, T, dims = _random_case()
    for reverse in (False, True):
        ring, cnt, opn = _run_lanes(exe, c, T, 3, lanes, reverse, dims)
        want = reference_checks(T, c["info"], c["term"], c["trunc"], c["cmd"], c["qpos"], c["qvel"], c["clock"], c["rows"], 3, dims[2],
                                include_open=True, open_scenario_rows=c["rows"][-1])
        from cosim_amd.checks import Verdicts
        got = Verdicts.from_raw(ring, cnt, opn, T)
        np.testing.assert_array_equal(got.words, want.words)
        np.testing.assert_array_equal(got.lost, want.lost)
        e = want.ended()
        assert want.failed[e].any() and want.passed[e].any() and want.incomplete[e].any() and want.lost.sum() > 0


# ------------------------------------------------------------------------------------------------------------ 4: resources
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/checks_kres_parent.txt) and after (checks_kres_this.txt): every existing kernel's line is
    identical, in the same order; the three added lines are the check kernels', which use no LDS, no scratch and spill nothing."""
    head_a, a = _table_file("checks_kres_parent.txt")
    head_b, b = _table_file("checks_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["checks_begin_kernel", "checks_open_kernel", "checks_step_kernel"]
    for name, (vgpr, agpr, sspill, vspill, scratch, occ, lds) in added.items():
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0), name
