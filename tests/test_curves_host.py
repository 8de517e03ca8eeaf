"""Response curves on the host (no GPU): the numpy twin of the curve kernels (cosim_amd/curves.py reference_curves) against a
hand-written case whose cells are written out by hand; the kernels' per-lane bodies (csrc/cosim_curves.h) compiled as plain C++ and
driven lane by lane against the twin, a second time under AddressSanitizer / UBSan as a stand-alone child process; quantiles, merge
and the .npz round trip; sweep(curves=...), YAML and validation messages; and the kernel-resource tables recorded before and after
the change.  Every comparison of cells is exact: words as words."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
K, N, NU, CD, NQ, NV = 12, 4, 1, 1, 7, 6
NI = 4 + 2 * NU + 1
Q = 1 << 20                                                             # one unit of the fixed-point sum

ROW0 = [[0, 8, 1, "info", "lin_vel_x", 0.0, 1.0, 4, "vx"],             # A: every step, T = 8, four bins of 0.25
        {"t0": 1, "t1": 8, "every": 3, "signal": "up", "lo": 0.5, "hi": 1.0, "bins": 2, "name": "up"},   # B: t = 1, 4, 7: T = ceil(7 / 3) = 3
        [0, 4, 1, "abs_info", 2, 0.0, 1.0, 0, "nobins"]]                # C: no histogram
ROW1 = [[0, 6, 2, "qpos", 2, 0.0, 1.0, 2, "height"]]                    # D: t = 0, 2, 4
NAMES = {"info": {"action_diff_RMSE": (0, 1), "lin_vel_x": (1, 1), "lin_vel_y": (2, 1), "ang_vel_yaw": (3, 1), "torque": (4, NU), "set_points": (4 + NU, NU),
                  "state": (4 + 2 * NU, 1)}, "info_dim": NI, "command_dim": CD, "nq": NQ, "nv": NV, "qpos": {"root": 0}, "qvel": {"root": 0, "hip": 0}}


def _table(rows=(ROW0, ROW1)):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable([{"commands": [[0, 0.5]], "curves": list(r)} for r in rows], CD, names={"checks": NAMES})


def _hand_case():
    """12 steps of four envs under two scenarios (mode env: envs 0, 2 run row 0, envs 1, 3 row 1).
      env 0: truncated in step 7 (clock 7): class 0 of row 0; the steps 8 .. 11 are an open episode (in no cell)
      env 1: terminated in step 3 (clock 3) and in step 9 (clock 5): two episodes in class 1 of row 1
      env 2: cut by a masked host reset before step 5 (nothing), cut again by a restore before step 9 that sets meta word 0 = 5
             (nothing); that restart is terminated in step 10 at clock 6: class 1 of row 0 gets the bins t = 5, 6 alone
      env 3: terminated in step 4 at clock 4, a sample time of the state signal D: the done row takes no sample"""
    rng = np.random.default_rng(11)
    c = {"info": rng.uniform(-1.0, 1.0, size=(K, N, NI)).astype(f32), "cmd": np.full((K, N, CD), 0.5, dtype=f32),
         "qpos": rng.uniform(-0.2, 0.2, size=(K, N, NQ)).astype(f32), "qvel": rng.uniform(-1.0, 1.0, size=(K, N, NV)).astype(f32)}
    # env 0, item A at t = 0 .. 7: inside, below lo, at hi, on a bin edge, NaN, inf, clamped at 2^20, on a bin edge (the done row)
    c["info"][:8, 0, 1] = np.array([0.125, -0.5, 1.0, 0.5, np.nan, np.inf, 3.0e6, 0.25], dtype=f32)
    # env 0, item C at t = 0 .. 3: halves of a unit round to even (0.5 -> 0, 1.5 -> 2)
    c["info"][:4, 0, 2] = np.array([2.0 ** -21, -3.0 * 2.0 ** -21, 0.5, 1.0], dtype=f32)
    # env 0, item B at t = 1 (up = 1 - 2 * 0.25 = 0.5 = lo) and t = 4 (up = 1 = hi); t = 7 is the done row
    c["qpos"][1, 0, 4:6] = [0.5, 0.0]
    c["qpos"][4, 0, 4:6] = [0.0, 0.0]
    # env 2 after the restore: item A at t = 5, 6
    c["info"][9:11, 2, 1] = np.array([0.75, 0.9375], dtype=f32)
    # item D: env 1 at t = 0, 2 | 0, 2, 4 and env 3 at t = 0, 2
    c["qpos"][[0, 2, 4, 6, 8], 1, 2] = np.array([0.0, 0.5, 0.25, 0.75, 2.0e6], dtype=f32)
    c["qpos"][[0, 2], 3, 2] = np.array([-0.0, -3.0e6], dtype=f32)
    te, tr = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    tr[7, 0] = 1
    te[[3, 9], 1] = 1
    te[10, 2] = 1
    te[4, 3] = 1
    c["term"], c["trunc"] = te, tr
    clock = np.zeros((K + 1, N), dtype=np.int32)                         # meta word 0 before step k; row K: after the last step
    clock[:, 0] = [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4]
    clock[:, 1] = [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 0, 1, 2]
    clock[:, 2] = [0, 1, 2, 3, 4, 0, 1, 2, 3, 5, 6, 0, 1]
    clock[:, 3] = [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6, 7]
    c["clock"] = clock
    c["rows"] = np.tile(np.array([0, 1, 0, 1]), (K, 1))
    c["begins"] = [(5, np.array([0, 0, 1, 0], dtype=np.uint8), 0), (9, np.array([0, 0, 1, 0], dtype=np.uint8), 8)]
    return c


def _twin(c, table, envs=slice(None), **kw):
    from cosim_amd.curves import reference_curves
    begins = [(k, None if m is None else np.asarray(m)[envs], f) for k, m, f in c.get("begins", ())]
    return reference_curves(table, c["info"][:, envs], c["term"][:, envs], c["trunc"][:, envs], c["cmd"][:, envs], c["qpos"][:, envs],
                            c["qvel"][:, envs], c["clock"][:, envs], c["rows"][:, envs], NU if "nu" not in c else c["nu"], begins=begins, **kw)


def _bits(x):
    return np.asarray(x, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ 1: the twin, by hand
def test_twin_against_hand_written_case():
    c, T = _hand_case(), _table()
    cv = _twin(c, T)
    assert cv.items() == [(0, 0), (0, 1), (0, 2), (1, 0)] and cv.names == [["vx", "up", "nobins"], ["height"]]
    # 2 classes x ((4 + 8) * 8 + (2 + 8) * 3 + 8 * 4 + (2 + 8) * 3)
    assert cv.cells.size == 2 * (96 + 30 + 32 + 30)
    nan = np.nan
    # ---- A, class 0: env 0's truncated episode
    a = cv[0, "vx"]
    assert a.t.tolist() == list(range(8)) and a.bins == 4
    assert a.count("truncated").tolist() == [1, 1, 1, 1, 0, 0, 1, 1] and a.nan("truncated").tolist() == [0, 0, 0, 0, 1, 1, 0, 0]
    assert a._sum[0].tolist() == [Q // 8, -Q // 2, Q, Q // 2, 0, 0, Q * Q, Q // 4], "3e6 is clamped at 2^20: 2^40 units"
    want = np.array([0.125, -0.5, 1.0, 0.5, nan, nan, 3.0e6, 0.25], dtype=f32)
    np.testing.assert_array_equal(a.min("truncated"), want)
    np.testing.assert_array_equal(a.max("truncated"), want)
    #                                   t:   0  1  2  3  4  5  6  7
    assert a.hist("truncated").tolist() == [[0, 1, 0, 0, 0, 0, 0, 0],     # below lo
                                            [1, 0, 0, 0, 0, 0, 0, 0],     # [0, 0.25)
                                            [0, 0, 0, 0, 0, 0, 0, 1],     # [0.25, 0.5): 0.25 is on the edge and belongs to the bin above it
                                            [0, 0, 0, 1, 0, 0, 0, 0],     # [0.5, 0.75): 0.5 likewise
                                            [0, 0, 0, 0, 0, 0, 0, 0],
                                            [0, 0, 1, 0, 0, 0, 1, 0]]     # at or above hi: 1.0 and 3e6
    # ---- A, class 1: env 2's restart at clock 5 sampled t = 5, 6 alone; its two cut episodes are nowhere
    assert a.count("terminated").tolist() == [0, 0, 0, 0, 0, 1, 1, 0] and a.nan("terminated").sum() == 0
    assert a._sum[1].tolist() == [0, 0, 0, 0, 0, 3 * Q // 4, 15 * Q // 16, 0]
    assert a.hist("terminated")[4].tolist() == [0, 0, 0, 0, 0, 1, 1, 0] and a.hist("terminated").sum() == 2
    assert a.count().tolist() == [1, 1, 1, 1, 0, 1, 2, 1] and a.nan().tolist() == [0, 0, 0, 0, 1, 1, 0, 0]
    np.testing.assert_array_equal(a.min(), np.array([0.125, -0.5, 1.0, 0.5, nan, 0.75, 0.9375, 0.25], dtype=f32))
    np.testing.assert_array_equal(a.max(), np.array([0.125, -0.5, 1.0, 0.5, nan, 0.75, 3.0e6, 0.25], dtype=f32))
    np.testing.assert_array_equal(a.mean("terminated"), [nan, nan, nan, nan, nan, 0.75, 0.9375, nan])
    assert a.mean()[6] == (2.0 ** 20 + 0.9375) / 2
    # ---- B: a state signal; t = 7 was env 0's done row: no sample there.  A window of 7 steps sampled every 3: three bins.
    b = cv[0, 1]
    assert b.name == "up" and b.t.tolist() == [1, 4, 7]
    assert b.count("truncated").tolist() == [1, 1, 0] and b._sum[0].tolist() == [Q // 2, Q, 0] and b.count("terminated").sum() == 0
    assert b.hist("truncated").tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0]], "0.5 = lo is inside, 1.0 = hi is above"
    # ---- C: bins = 0 keeps no histogram; halves round to even
    cc = cv[0, "nobins"]
    assert cc.hist().shape == (2, 4) and cc.hist().sum() == 0 and cc.count("truncated").tolist() == [1, 1, 1, 1]
    assert cc._sum[0].tolist() == [0, 2, Q // 2, Q]
    np.testing.assert_array_equal(cc.max(), np.array([2.0 ** -21, 3.0 * 2.0 ** -21, 0.5, 1.0], dtype=f32))
    with pytest.raises(ValueError, match="bins = 0 keeps no histogram"):
        cc.quantile(0.5)
    # ---- D, class 1: env 1's two episodes and env 3's; t = 4 was env 3's done row, and env 1's first episode ended before it
    d = cv[1, 0]
    assert d.t.tolist() == [0, 2, 4] and d.count("truncated").sum() == 0 and d.nan().sum() == 0
    assert d.count("terminated").tolist() == [3, 3, 1], "a bin with fewer samples than episodes"
    assert d._sum[1].tolist() == [Q // 4, Q // 2 + 3 * Q // 4 - Q * Q, Q * Q]
    assert d.hist("terminated").tolist() == [[0, 1, 0], [3, 0, 0], [0, 2, 0], [0, 0, 1]]
    np.testing.assert_array_equal(_bits(d.min("terminated")), _bits([-0.0, -3.0e6, 2.0e6]))    # -0 sorts below +0
    np.testing.assert_array_equal(_bits(d.max("terminated")), _bits([0.25, 0.75, 2.0e6]))
    assert d._min[1, 0] == 0x7FFFFFFF and d._min[0].tolist() == [0xFFFFFFFF] * 3 and d._max[0].tolist() == [0] * 3
    np.testing.assert_array_equal(d.mean("truncated"), [nan] * 3)
    assert d.both("count").tolist() == [[0, 0, 0], [3, 3, 1]] and d.both("hist").shape == (2, 4, 3) and d.both("mean").shape == (2, 3)
    # ---- quantiles off the histogram: linear inside a bin, the outer rows clamp to lo / hi, NaN with no sample
    np.testing.assert_array_equal(d.quantile(0.5), [0.25, 0.625, 1.0])
    np.testing.assert_allclose(d.quantile(0.05, "terminated"), [0.025, 0.0, 1.0], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(d.quantile(0.5, "truncated"), [nan] * 3)
    lo, mid, hi = d.band(0.05, 0.95)
    assert (lo <= mid).all() and (mid <= hi).all() and abs(hi[1] - 0.9625) < 1e-15
    s = cv.summary()
    assert s["items"] == 4 and s["episodes"] == 5 and s["episodes_truncated"] == 1 and s["episodes_terminated"] == 4 and s["nonfinite"] == 2
    assert cv.episodes().tolist() == [[1, 1], [0, 3]]
    # a clear ahead of step 8 leaves what ended from step 8 on: env 1's second episode has lost its t = 0, 2 samples, env 2's restart
    late = _twin(c, T, clears=(8,))
    assert late[0, 0].count("truncated").sum() == 0 and late[0, 0].count("terminated").tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    assert late[1, 0].count("terminated").tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------------------------------------ 2: container
def test_npz_merge_and_half_fleets(tmp_path):
    from cosim_amd.curves import Curves, same_curves
    c, T = _hand_case(), _table()
    whole = _twin(c, T)
    path = str(tmp_path / "curves.npz")
    whole.save(path)
    w = Curves.load(path)
    assert same_curves(whole, w) is None and w.names == whole.names
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"cells", "adr", "spec", "lohi", "bins", "names"}
    a, b = _twin(c, T, envs=slice(0, 2)), _twin(c, T, envs=slice(2, 4))
    assert same_curves(a, whole) is not None and "words differ" in same_curves(a, whole)
    assert same_curves(a.merge(b), whole) is None and same_curves(b.merge(a), whole) is None
    assert same_curves(whole.merge(Curves.empty(T)), whole) is None
    twice = whole.merge(whole)
    assert twice[1, 0].count("terminated").tolist() == [6, 6, 2] and twice[1, 0]._sum[1, 2] == 2 * Q * Q
    np.testing.assert_array_equal(_bits(twice[1, 0].min()), _bits(whole[1, 0].min()))
    with pytest.raises(ValueError, match="different items"):
        whole.merge(_twin(c, _table((ROW0, [[0, 6, 2, "qpos", 2, 0.0, 2.0, 2, "height"]]))))
    with pytest.raises(KeyError, match="no item 'nope'"):
        whole[0, "nope"]


def test_sweep_curves_axis_packing_and_layout():
    from cosim_amd.curves import layout
    from cosim_amd.scenario import ScenarioTable, sweep
    cu = [[], [[150, 260, 2, "tracking_error", 0, 0.0, 1.0, 32, "recovery"], [0, 300, 1, "up", 0, 0.0, 1.0, 0]]]
    scn = list(sweep([[0.5, 0.0, 0.0], [1.0, 0.0, 0.0]], [1.0], [0.0], [(150, 155)], curves=cu))
    assert len(scn) == 4 and "curves" not in scn[0] and scn[1]["curves"][0][8] == "recovery" and scn[3]["commands"] == [[0, 1.0, 0.0, 0.0]]
    T = ScenarioTable(scn, 3)
    adr, t, sig, idx, lo, hi, bins = T.pack_curves()
    assert adr.tolist() == [0, 0, 2, 2, 4] and t.tolist() == [[150, 260, 2], [0, 300, 1]] * 2 and sig.tolist() == [2, 4, 2, 4]
    assert bins.tolist() == [32, 0, 32, 0] and lo.dtype == np.float32 and hi.tolist() == [1.0] * 4 and idx.tolist() == [0] * 4
    assert T.curve_item_names()[1] == ["recovery", "up[0] @0:300:1"] and T.n_curve_items == 4 and T.has_curves
    assert ScenarioTable(T.to_list(), 3).pack_curves()[1].tolist() == t.tolist()
    L = layout(T.pack_curves())
    assert L["T"].tolist() == [55, 300, 55, 300] and L["soff"].tolist() == [0, 55, 0, 55] and L["stage_words"] == 355
    assert L["cw"].tolist() == [40 * 55, 8 * 300] * 2 and L["coff"].tolist() == [0, 4400, 9200, 13600] and L["words"] == 18400
    both = list(sweep([[0.5, 0.0, 0.0]], checks=[[], [[0, 5, "up", 0, "always", ">", 0.5]]], curves=cu))
    assert len(both) == 4 and "checks" in both[2] and "curves" in both[3] and "curves" not in both[2]


def test_yaml_loading(tmp_path):
    yaml = pytest.importorskip("yaml")
    from cosim_amd.scenario import ScenarioTable
    p = tmp_path / "scn.yaml"
    p.write_text(yaml.safe_dump({"scenarios": [{"commands": [[0, 0.5]], "curves": [list(r) if not isinstance(r, dict) else r for r in ROW0]}]}))
    T = ScenarioTable.build(str(p), CD)
    assert T.has_curves and not T.has_checks
    with pytest.raises(ValueError, match="not resolved yet"):          # 'lin_vel_x' needs the model
        T.pack_curves()
    assert T.resolve_curves(NAMES).pack_curves()[2].tolist() == [0, 4, 1] and T.pack_curves()[3].tolist() == [1, 0, 2]


def test_validation_messages_name_the_scenario_and_the_item():
    from cosim_amd.scenario import ScenarioTable
    ok = [0, 5, 1, "info", 1, 0.0, 1.0, 4]

    def bad(row, match, names=NAMES):
        with pytest.raises(ValueError, match=match):
            ScenarioTable([{}, {"curves": [ok, row]}], CD, names={"checks": names})
    bad([0, 5, 1, "info", 1, float("nan"), 1.0, 4], r"scenario 1, curve item 1: non-finite lo / hi")
    bad([0, 5, 1, "info", 1, 0.0, float("inf"), 0], r"scenario 1, curve item 1: non-finite lo / hi")
    bad([0, 5, 1, "info", 1, 1.0, 1.0, 4], r"scenario 1, curve item 1: hi 1.0 is not above lo 1.0")
    bad([5, 5, 1, "info", 1, 0.0, 1.0, 4], r"scenario 1, curve item 1: t1 5 is not after t0 5")
    bad([-1, 5, 1, "info", 1, 0.0, 1.0, 4], r"scenario 1, curve item 1: times must be control steps")
    bad([0, 5, 0, "info", 1, 0.0, 1.0, 4], r"scenario 1, curve item 1: every must be a whole number of control steps >= 1")
    bad([0, 1025, 1, "info", 1, 0.0, 1.0, 4], r"scenario 1, curve item 1: 1025 time bins, at most 1024")
    bad([0, 5, 1, "info", 1, 0.0, 1.0, 65], r"scenario 1, curve item 1: bins must be 0..64")
    bad([0, 5, 1, "speed", 1, 0.0, 1.0, 4], r"scenario 1, curve item 1: unknown signal 'speed'")
    bad([0, 5, 1, "info", NI, 0.0, 1.0, 4], r"scenario 1, curve item 1: index %d out of range: 'info' has %d entries" % (NI, NI))
    bad([0, 5, 1, "info", "torque[1]", 0.0, 1.0, 4], r"curve item 1: 'torque\[1\]' out of range: 'torque' has 1 entries")
    bad([0, 5, 1, "qpos", "knee", 0.0, 1.0, 4], r"scenario 1, curve item 1: unknown joint 'knee'")
    bad([0, 5, 1, "info", 1, 0.0, 1.0], r"scenario 1, curve item 1: expected \[t0, t1, every, signal, index, lo, hi, bins\]")
    ScenarioTable([{"curves": [[0, 2048, 2, "info", 1, 1.0, 1.0, 0]]}], CD)     # T = 1024 and, with no histogram, any finite lo / hi
    with pytest.raises(ValueError, match=r"scenario 0: 9 curve items, at most 8"):
        ScenarioTable([{"curves": [ok] * 9}], CD)


# ------------------------------------------------------------------------------------------------------------ 3: the header as C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "curves_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/curves_lanes.cpp + csrc/cosim_curves.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("curves")
    return _build(tmp, "curves_lanes", []), _build(tmp, "curves_lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                             "-fno-omit-frame-pointer"])


def _run_lanes(exe, c, table, lanes, reverse, dims, clears=()):
    from cosim_amd.curves import Curves, layout
    n_envs, ni, nu, cd, nq, nv = dims
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    csr = table.pack_curves()
    adr, t, sig, idx, lo, hi, bins = csr
    L = layout(csr)
    inv_w = [f32(np.float64(b) / (np.float64(h) - np.float64(l))) if b > 0 else f32(0) for l, h, b in zip(lo, hi, bins)]
    words = [len(adr) - 1, len(sig)] + adr.tolist() + t.reshape(-1).tolist() + sig.tolist() + idx.tolist() + bins.tolist()
    words += L["T"].tolist() + L["soff"].tolist() + L["coff"].tolist() + L["cw"].tolist() + u(lo) + u(hi) + u(inv_w)
    words += [L["stage_words"], L["words"], lanes, n_envs, ni, nu, cd, nq, nv, int(reverse)]
    steps = c["info"].shape[0]
    words += [1] + [1] * n_envs + c["clock"][0].tolist()
    for k in range(steps):
        if k in clears:
            words += [4] + c["clock"][k].tolist()
        for kb, mask, _ in c.get("begins", ()):
            if kb == k:
                words += [1] + np.asarray(mask).astype(int).tolist() + c["clock"][k].tolist()
        words.append(2)
        for i in range(n_envs):
            words += [int(c["term"][k, i]), int(c["trunc"][k, i]), int(c["rows"][k, i]), int(c["clock"][k + 1, i])]
            words += u(c["info"][k, i]) + u(c["cmd"][k, i]) + u(c["qpos"][k, i]) + u(c["qvel"][k, i])
    words.append(3)
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return Curves.from_raw(np.array(p.stdout.split(), dtype=np.uint64).astype(np.uint32), table)


def _random_case(seed=5):
    """8 envs, 40 steps, three scenarios -- 8 items (one with T = 1024 and 64 bins), one item, 5 items -- in mode env; the curves are
    armed on a stepped fleet (the clocks start anywhere in the windows) and episodes end at random."""
    rng = np.random.default_rng(seed)
    n_envs, steps, nu, cd, nq, nv = 8, 40, 3, 2, 9, 8
    ni = 4 + 2 * nu + 2
    sigs = ["info", "abs_info", "tracking_error", "torque_max", "up", "qpos", "qvel", "abs_qvel"]

    def item(big=False):
        s = sigs[rng.integers(len(sigs))]
        width = {"info": ni, "abs_info": ni, "tracking_error": cd, "torque_max": 1, "up": 1, "qpos": nq, "qvel": nv, "abs_qvel": nv}[s]
        t0, every = (0, 1) if big else (int(rng.integers(0, 30)), int(rng.integers(1, 5)))
        lo = float(f32(rng.uniform(-0.8, 0.2)))
        return [t0, 1024 if big else t0 + int(rng.integers(1, 60)), every, s, int(rng.integers(width)), lo, float(f32(lo + rng.uniform(0.05, 1.0))),
                64 if big else int(rng.integers(0, 65))]
    from cosim_amd.scenario import ScenarioTable
    T = ScenarioTable([{"curves": [item(big=(n == 8 and j == 3)) for j in range(n)]} for n in (8, 1, 5)], cd)
    c = {"info": rng.uniform(-1.0, 1.0, size=(steps, n_envs, ni)).astype(f32), "cmd": rng.uniform(-1.0, 1.0, size=(steps, n_envs, cd)).astype(f32),
         "qpos": rng.uniform(-0.6, 0.6, size=(steps, n_envs, nq)).astype(f32), "qvel": rng.uniform(-1.0, 1.0, size=(steps, n_envs, nv)).astype(f32)}
    c["info"][rng.integers(steps, size=12), rng.integers(n_envs, size=12)] = np.nan          # whole info rows
    c["info"][rng.integers(steps, size=6), rng.integers(n_envs, size=6)] = -np.inf
    done = rng.uniform(size=(steps, n_envs)) < 0.1
    c["term"] = (done & (rng.uniform(size=done.shape) < 0.5)).astype(np.uint8)
    c["trunc"] = (done & (c["term"] == 0)).astype(np.uint8)
    clock = np.zeros((steps + 1, n_envs), dtype=np.int32)
    clock[0] = rng.integers(0, 1000, size=n_envs)
    for k in range(steps):
        clock[k + 1] = np.where(done[k], 0, clock[k] + 1)
    c["clock"], c["rows"] = clock, np.tile(np.arange(n_envs) % 3, (steps, 1))
    c["begins"], c["nu"] = [], nu
    return c, T, (n_envs, ni, nu, cd, nq, nv)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("lanes", [64, 5, 1])
def test_kernel_bodies_as_host_cpp_equal_the_twin(lanes_exes, lanes, sanitized):
    """The hand-written case and a random one with 8 items, T = 1024 and B = 64 through the functions the kernels call, with 64
    lanes (the wave), 5 and 1, the two ranges of a step in either order: the cells equal the twin's word for word."""
    from cosim_amd.curves import same_curves
    exe = lanes_exes[1 if sanitized else 0]
    c, T = _hand_case(), _table()
    for reverse, clears in ((False, ()), (True, (8,))):
        got = _run_lanes(exe, c, T, lanes, reverse, (N, NI, NU, CD, NQ, NV), clears)
        assert same_curves(got, _twin(c, T, clears=clears)) is None, same_curves(got, _twin(c, T, clears=clears))
    c, T, dims = _random_case()
    want = _twin(c, T)
    for reverse in (False, True):
        got = _run_lanes(exe, c, T, lanes, reverse, dims)
        assert same_curves(got, want) is None, same_curves(got, want)
    s = want.summary()
    big = want[0, 3]
    assert s["episodes_truncated"] > 0 and s["episodes_terminated"] > 0 and s["nonfinite"] > 0 and big.t.size == 1024 and big.bins == 64
    assert big.count().sum() > 0 and big.hist().shape == (66, 1024)


def test_merge_of_two_half_fleets_equals_the_whole_fleet():
    from cosim_amd.curves import same_curves
    c, T, _ = _random_case(seed=9)
    whole = _twin(c, T)
    a, b = _twin(c, T, envs=slice(0, 3)), _twin(c, T, envs=slice(3, 8))
    assert same_curves(a.merge(b), whole) is None, same_curves(a.merge(b), whole)


def test_word_kinds_reduce_like_merge():
    """What FleetReporter all-reduces under torchrun: SUM over the add words and the int64 sums, MIN / MAX over the keys."""
    c, T, _ = _random_case(seed=9)
    a, b = _twin(c, T, envs=slice(0, 3)), _twin(c, T, envs=slice(3, 8))
    kind, cells = a.word_kinds(), a.cells.copy()
    assert set(np.unique(kind).tolist()) == {0, 1, 2, 3} and int((kind == 3).sum()) == 2 * int((kind == 1).sum())
    cells[kind == 0] = a.cells[kind == 0] + b.cells[kind == 0]
    cells[kind == 3] = (a.cells[kind == 3].view(np.int64) + b.cells[kind == 3].view(np.int64)).view(np.uint32)
    cells[kind == 1] = np.minimum(a.cells[kind == 1], b.cells[kind == 1])
    cells[kind == 2] = np.maximum(a.cells[kind == 2], b.cells[kind == 2])
    np.testing.assert_array_equal(cells, a.merge(b).cells)


# ------------------------------------------------------------------------------------------------------------ 4: resources
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/curves_kres_parent.txt) and after (curves_kres_this.txt): every existing kernel's line is
    identical, in the same order; the three added lines are the curve kernels', which use no LDS, no scratch and spill nothing."""
    head_a, a = _table_file("curves_kres_parent.txt")
    head_b, b = _table_file("curves_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["curves_begin_kernel", "curves_clear_kernel", "curves_step_kernel"]
    for name, (vgpr, agpr, sspill, vspill, scratch, occ, lds) in added.items():
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0), name
