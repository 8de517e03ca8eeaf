"""The host side of the scenario family's setters (csrc/cosim_tables.h) without a GPU: tests/tables_host.cpp, built plain and with
AddressSanitizer / UBSan as a stand-alone child process, is handed raw tables the way the C ABI is and answers with the refusal, or
with the packed image and the derived values.  Every refusal of the four validators once, word for word as cosim_last_error returns
it (the patterns the GPU suites match are held against the same strings); where a table's arrays lie in the image and where its
pointers point; the derived values against cosim_amd.curves.layout; and the in-place test."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
i32, f32 = np.int32, np.float32
# a robot of the size of flamingo_light_v1 with four motors and a four-value command; parameter record: floss at 46, gmu 64, kp 77, kd 81
NQ, NV, NU, NGEOM, CD = 19, 18, 4, 13, 4
INFO = 4 + 2 * NU + 3
P_KP, P_KD, P_GMU, P_FLOSS = 77, 81, 64, 46
DIMS = (NQ, NV, NU, NGEOM, INFO, CD, P_KP, P_KD, P_GMU, P_FLOSS)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tables") / ("tables_host_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "tables_host.cpp")])
    return out


def _words(a):
    if a is None:
        return ["-1"]
    a = np.ascontiguousarray(a)
    assert a.dtype in (i32, f32), a.dtype
    w = a.view(i32).ravel()
    return [str(w.size)] + [str(int(x)) for x in w]


def run(exe, kind, tables, n_envs=4, slots=2, dims=DIMS):
    """tables: one (n_scn, array, ...) tuple per table.  ("ERR", message) or ("OK", {name: ints}, {name: (offset, words)}, total)."""
    tok = [kind] + [str(d) for d in dims] + [str(n_envs), str(slots)]
    for tab in tables:
        tok.append(str(tab[0]))
        for a in tab[1:]:
            tok += _words(a)
    p = subprocess.run([exe], input=" ".join(tok), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    if lines[0].startswith("ERR "):
        return "ERR", lines[0][4:]
    if lines[0].startswith("same "):
        return "same", int(lines[0][5:])
    assert lines[0] == "OK"
    val, arr, total = {}, {}, None
    for ln in lines[1:]:
        f = ln.split()
        if f[0] == "val":
            val[f[1]] = [int(x) for x in f[2:]]
        elif f[0] == "arr":
            assert int(f[3]) == len(f) - 4
            arr[f[1]] = (int(f[2]), np.array(f[4:], dtype=np.int64).astype(i32))
        else:
            total = int(f[1])
    return "OK", val, arr, total


def refused(exe, kind, table, want, gpu_match=None, **kw):
    got = run(exe, kind, [table], **kw)
    assert got == ("ERR", want)
    if gpu_match is not None:                                     # the pattern the GPU suite holds against cosim_last_error
        assert re.search(gpu_match, want), gpu_match


def csr(rows, widths):
    """rows: per scenario a list of item tuples; widths: per column (words per item, dtype).  (n_scn, adr, columns ...)."""
    flat = [it for r in rows for it in r]
    adr = np.cumsum([0] + [len(r) for r in rows]).astype(i32)
    cols, k = [], 0
    for w, dt in widths:
        cols.append(np.array([it[k:k + w] for it in flat], dtype=dt).reshape(len(flat), w) if w > 1 else np.array([it[k] for it in flat], dtype=dt))
        k += w
    return (len(rows), adr, *cols)


CHK_COLS = [(2, i32), (1, i32), (1, i32), (1, i32), (1, i32), (1, f32)]            # t | signal | index | mode | cmp | bound
CUR_COLS = [(3, i32), (1, i32), (1, i32), (1, f32), (1, f32), (1, i32)]            # t | signal | index | lo | hi | bins
PAR_COLS = [(2, i32), (1, i32), (1, i32), (1, i32), (1, f32)]                      # t | field | index | op | value
CHK_OK = (0, 5, 0, 1, 0, 0, 1.0)
CUR_OK = (0, 5, 1, 0, 1, 0.0, 1.0, 4)
PAR_OK = (0, 5, 0, 0, 0, 0.5)
SIGNALS = [("info", INFO), ("abs_info", INFO), ("tracking_error", 3), ("torque_max", 1), ("up", 1), ("qpos", NQ), ("qvel", NV), ("abs_qvel", NV)]
SIGNAL_LIST = "(0 info, 1 abs_info, 2 tracking_error, 3 torque_max, 4 up, 5 qpos, 6 qvel, 7 abs_qvel)"


def _with(base, k, value):
    it = list(base)
    it[k] = value
    return tuple(it)


def scenario(keys, pushes, cd=CD):
    """keys: per scenario [(t, c0 .. c(cd-1))]; pushes: per scenario [(t0, t1, vx, vy, vz)]."""
    _, kadr, kt, kc = csr(keys, [(1, i32), (cd, f32)])
    _, padr, pt, pv = csr(pushes, [(2, i32), (3, f32)])
    return (len(keys), kadr, kt, kc.reshape(-1, cd), padr, pt, pv)


# ------------------------------------------------------------------------------------------------------------------ 1: the refusals
def test_row_address_refusals_of_every_setter(exe):
    for kind, fn, cols, ok, noun, cap in (("params", "cosim_scenario_params_set", PAR_COLS, PAR_OK, "parameter items", 256),
                                          ("checks", "cosim_scenario_checks_set", CHK_COLS, CHK_OK, "check items", 64),
                                          ("curves", "cosim_scenario_curves_set", CUR_COLS, CUR_OK, "curve items", 8)):
        good = csr([[ok], [], [ok, ok]], cols)
        refused(exe, kind, (3, None) + good[2:], fn + ": null argument")
        refused(exe, kind, (3, np.array([1, 1, 1, 3], i32)) + good[2:], fn + ": adr[0] must be 0")
        refused(exe, kind, (3, np.array([0, 2, 1, 3], i32)) + good[2:], fn + ": scenario 1: row addresses must not decrease")
        refused(exe, kind, (3, good[1]) + (None,) + good[3:], fn + ": scenario 0: null table array")
        many = csr([[], [ok] * (cap + 1), []], cols)
        refused(exe, kind, many, "%s: scenario 1: %d %s, at most %d" % (fn, cap + 1, noun, cap), gpu_match=r"scenario 1: %d %s, at most %d" % (cap + 1, noun, cap))
        refused(exe, kind, csr([[], [], []], cols), "%s: the table holds no %s (n_scn = 0 clears the %s)" %
                (fn, noun[:-1], {"params": "windows", "checks": "checks", "curves": "curves"}[kind]))
        # both window messages, with the item named
        what = noun[:-1]
        for t, msg in (((-1, 7), "times outside [0, 2^30)"), ((1 << 30, (1 << 30) + 0), "times outside [0, 2^30)"), ((0, (1 << 30) + 1), "times outside [0, 2^30)"),
                       ((7, 7), "t1 7 is not after t0 7"), ((9, 3), "t1 3 is not after t0 9")):
            bad = tuple(t) + tuple(ok[2:])
            refused(exe, kind, csr([[ok], [], [ok, bad]], cols), "%s: scenario 2, %s 1: %s" % (fn, what, msg))
    # the scenario table: two address arrays, judged together row by row
    fn = "cosim_scenario_set"
    good = scenario([[(0, 1, 0, 0, 0)], [], []], [[], [(0, 5, 1, 0, 0)], []])
    refused(exe, "scenario", (3, None) + good[2:], fn + ": null argument")
    refused(exe, "scenario", good[:4] + (None,) + good[5:], fn + ": null argument")
    refused(exe, "scenario", good[:4] + (np.array([1, 1, 2, 2], i32),) + good[5:], fn + ": key_adr[0] and push_adr[0] must be 0")
    refused(exe, "scenario", (3, np.array([0, 1, 0, 1], i32)) + good[2:], fn + ": scenario 1: row addresses must not decrease")
    refused(exe, "scenario", good[:4] + (np.array([0, 1, 0, 1], i32),) + good[5:], fn + ": scenario 1: row addresses must not decrease")
    refused(exe, "scenario", good[:3] + (None,) + good[4:], fn + ": scenario 0: null table array")
    refused(exe, "scenario", good[:6] + (None,), fn + ": scenario 1: null table array")
    refused(exe, "scenario", scenario([[], [(k, 0, 0, 0, 0) for k in range(65)]], [[], []]), fn + ": scenario 1: 65 keyframes, at most 64",
            gpu_match=r"scenario 1: 65 keyframes, at most 64")
    refused(exe, "scenario", scenario([[]], [[(k, k + 1, 0, 0, 0) for k in range(65)]]), fn + ": scenario 0: 65 push windows, at most 64",
            gpu_match=r"scenario 0: 65 push windows, at most 64")
    # a row with too many keyframes whose push addresses decrease: the addresses are judged first
    refused(exe, "scenario", (2, np.array([0, 65, 65], i32), np.arange(65, dtype=i32), np.zeros((65, CD), f32), np.array([0, 1, 0], i32),
                              np.array([[0, 1]], i32), np.zeros((1, 3), f32)), fn + ": scenario 0: 65 keyframes, at most 64")
    refused(exe, "scenario", (2, np.array([0, 65, 65], i32), np.arange(65, dtype=i32), np.zeros((65, CD), f32), np.array([0, -1, 0], i32),
                              np.array([[0, 1]], i32), np.zeros((1, 3), f32)), fn + ": scenario 0: row addresses must not decrease")


def test_scenario_item_refusals(exe):
    fn = "cosim_scenario_set"
    refused(exe, "scenario", scenario([[], [(0, 0, 0, 0, 0), (-1, 0, 0, 0, 0)]], [[], []]), fn + ": scenario 1, keyframe 1: time -1 outside [0, 2^30)")
    refused(exe, "scenario", scenario([[(1 << 30, 0, 0, 0, 0)]], [[]]), fn + ": scenario 0, keyframe 0: time 1073741824 outside [0, 2^30)")
    refused(exe, "scenario", scenario([[], [(7, 0, 0, 0, 0), (4, 0, 0, 0, 0)]], [[], []]), fn + ": scenario 1, keyframe 1: time 4 does not increase (previous 7)",
            gpu_match=r"scenario 1, keyframe 1: time 4 does not increase \(previous 7\)")
    refused(exe, "scenario", scenario([[(0, 0, 0, NAN, 0)]], [[]]), fn + ": scenario 0, keyframe 0: command 2 is not finite",
            gpu_match=r"scenario 0, keyframe 0: command 2 is not finite")
    refused(exe, "scenario", scenario([[], [], []], [[], [], [(3, 3, 1, 0, 0)]]), fn + ": scenario 2, push window 0: t1 3 is not after t0 3",
            gpu_match=r"scenario 2, push window 0: t1 3 is not after t0 3")
    refused(exe, "scenario", scenario([[]], [[(-2, 3, 1, 0, 0)]]), fn + ": scenario 0, push window 0: times outside [0, 2^30)")
    refused(exe, "scenario", scenario([[]], [[(0, 1, 1, 0, 0), (1, 2, 0, INF, 0)]]), fn + ": scenario 0, push window 1: velocity 1 is not finite",
            gpu_match=r"scenario 0, push window 1: velocity 1 is not finite")
    # a keyframe fault of a row is reported ahead of a push fault of the same row, and a fault of row 0 ahead of row 1's addresses
    refused(exe, "scenario", scenario([[(0, INF, 0, 0, 0)]], [[(3, 3, 0, 0, 0)]]), fn + ": scenario 0, keyframe 0: command 0 is not finite")
    t = scenario([[(0, INF, 0, 0, 0)], []], [[], []])
    refused(exe, "scenario", (2, np.array([0, 1, 0], i32)) + t[2:], fn + ": scenario 0, keyframe 0: command 0 is not finite")


def test_parameter_item_refusals(exe):
    fn, one = "cosim_scenario_params_set", lambda it: csr([[], [PAR_OK, it], []], PAR_COLS)   # noqa: E731
    for field in (4, 5, 6, 7):
        refused(exe, "params", one(_with(PAR_OK, 2, field)), fn + ": scenario 1, parameter item 1: field %d (body_mass, body_invweight0, dof_invweight0, "
                "meaninertia) is refused: the mass fields are consistent only as a set computed on the host in fp64; a payload change in mid-episode "
                "is out of scope" % field, gpu_match=r"scenario 1, parameter item 1: field %d .* is refused: .* fp64" % field)
    for field in (8, 9, -1):
        refused(exe, "params", one(_with(PAR_OK, 2, field)), fn + ": scenario 1, parameter item 1: unknown field %d (0 kp, 1 kd, 2 geom_friction, "
                "3 dof_frictionloss)" % field, gpu_match=r"parameter item 1: unknown field")
    for field, (name, width) in enumerate([("kp", NU), ("kd", NU), ("geom_friction", NGEOM), ("dof_frictionloss", NV)]):
        for index in (width, -1):
            refused(exe, "params", one(_with(_with(PAR_OK, 2, field), 3, index)), "%s: scenario 1, parameter item 1: index %d out of range: %s has %d entries" %
                    (fn, index, name, width), gpu_match=r"parameter item 1: index %d out of range" % index)
    refused(exe, "params", one(_with(PAR_OK, 4, 2)), fn + ": scenario 1, parameter item 1: unknown op 2 (0 scale, 1 set)", gpu_match=r"parameter item 1: unknown op 2")
    for value in (INF, -INF, NAN):
        refused(exe, "params", one(_with(PAR_OK, 5, value)), fn + ": scenario 1, parameter item 1: value is not finite", gpu_match=r"parameter item 1: value is not finite")
    # the order within an item: window, field, index, op, value
    refused(exe, "params", one((5, 5, 9, -1, 2, NAN)), fn + ": scenario 1, parameter item 1: t1 5 is not after t0 5")
    refused(exe, "params", one((0, 5, 9, -1, 2, NAN)), fn + ": scenario 1, parameter item 1: unknown field 9 (0 kp, 1 kd, 2 geom_friction, 3 dof_frictionloss)")
    refused(exe, "params", one((0, 5, 1, -1, 2, NAN)), fn + ": scenario 1, parameter item 1: index -1 out of range: kd has 4 entries")
    refused(exe, "params", one((0, 5, 1, 0, 2, NAN)), fn + ": scenario 1, parameter item 1: unknown op 2 (0 scale, 1 set)")


def test_check_item_refusals(exe):
    fn, one = "cosim_scenario_checks_set", lambda it: csr([[], [it], []], CHK_COLS)   # noqa: E731
    for slots in (0, 65, -3):
        refused(exe, "checks", one(CHK_OK), "%s: slots %d outside 1..64" % (fn, slots), slots=slots, gpu_match=r"slots -?\d+ outside 1\.\.64")
    refused(exe, "checks", (3, None) + one(CHK_OK)[2:], fn + ": slots 0 outside 1..64", slots=0)      # the slots ahead of the table
    for signal in (8, 9, -1):
        refused(exe, "checks", one(_with(CHK_OK, 2, signal)), "%s: scenario 1, check item 0: unknown signal %d %s" % (fn, signal, SIGNAL_LIST),
                gpu_match=r"scenario 1, check item 0: unknown signal")
    for signal, (name, width) in enumerate(SIGNALS):
        for index in (width, -1):
            refused(exe, "checks", one(_with(_with(CHK_OK, 2, signal), 3, index)), "%s: scenario 1, check item 0: index %d out of range: %s has %d entries" %
                    (fn, index, name, width))
        assert run(exe, "checks", [one(_with(_with(CHK_OK, 2, signal), 3, width - 1))])[0] == "OK"
    assert re.search(r"scenario 1, check item 0: index 3 out of range: tracking_error has 3 entries", fn + ": scenario 1, check item 0: index 3 out of range: "
                     "tracking_error has 3 entries")
    # a command of two values tracks two; a robot without a free joint's quaternion has no "up"
    refused(exe, "checks", one(_with(_with(CHK_OK, 2, 2), 3, 2)), fn + ": scenario 1, check item 0: index 2 out of range: tracking_error has 2 entries",
            dims=DIMS[:5] + (2,) + DIMS[6:])
    refused(exe, "checks", one(_with(_with(CHK_OK, 2, 4), 3, 0)), fn + ": scenario 1, check item 0: index 0 out of range: up has 0 entries", dims=(6,) + DIMS[1:])
    for mode in (3, -1):
        refused(exe, "checks", one(_with(CHK_OK, 4, mode)), "%s: scenario 1, check item 0: unknown mode %d (0 always, 1 settle, 2 mean)" % (fn, mode),
                gpu_match=r"scenario 1, check item 0: unknown mode")
    for cmp in (2, -1):
        refused(exe, "checks", one(_with(CHK_OK, 5, cmp)), "%s: scenario 1, check item 0: unknown cmp %d (0 <, 1 >)" % (fn, cmp),
                gpu_match=r"scenario 1, check item 0: unknown cmp")
    for bound in (INF, NAN):
        refused(exe, "checks", one(_with(CHK_OK, 6, bound)), fn + ": scenario 1, check item 0: bound is not finite", gpu_match=r"scenario 1, check item 0: bound is not finite")
    # items of a row are judged before the next row's addresses
    t = csr([[_with(CHK_OK, 6, NAN)], [], []], CHK_COLS)
    refused(exe, "checks", (3, np.array([0, 1, 0, 1], i32)) + t[2:], fn + ": scenario 0, check item 0: bound is not finite")


def test_curve_item_refusals(exe):
    fn, one = "cosim_scenario_curves_set", lambda it: csr([[], [it], []], CUR_COLS)   # noqa: E731
    at = fn + ": scenario 1, curve item 0: "
    for every in (0, -2):
        refused(exe, "curves", one(_with(CUR_OK, 2, every)), at + "every %d is below 1" % every, gpu_match=r"scenario 1, curve item 0: every -?\d is below 1")
    refused(exe, "curves", one((0, 1025, 1) + CUR_OK[3:]), at + "1025 time bins, at most 1024", gpu_match=r"scenario 1, curve item 0: 1025 time bins, at most 1024")
    refused(exe, "curves", one((3, 2052, 2) + CUR_OK[3:]), at + "1025 time bins, at most 1024")
    assert run(exe, "curves", [one((3, 2051, 2) + CUR_OK[3:])])[0] == "OK"
    for bins in (65, -1):
        refused(exe, "curves", one(_with(CUR_OK, 7, bins)), at + "bins %d outside 0..64" % bins, gpu_match=r"scenario 1, curve item 0: bins -?\d+ outside 0\.\.64")
    for k, value in ((5, NAN), (6, INF), (5, -INF)):
        refused(exe, "curves", one(_with(CUR_OK, k, value)), at + "lo / hi is not finite", gpu_match=r"scenario 1, curve item 0: lo / hi is not finite")
    for hi in (0.0, -1.0):
        refused(exe, "curves", one(_with(CUR_OK, 6, hi)), at + "hi is not above lo", gpu_match=r"scenario 1, curve item 0: hi is not above lo")
    assert run(exe, "curves", [one(_with(_with(CUR_OK, 6, 0.0), 7, 0))])[0] == "OK"               # no histogram: lo and hi are not used
    for signal in (8, -1):
        refused(exe, "curves", one(_with(CUR_OK, 3, signal)), at + "unknown signal %d %s" % (signal, SIGNAL_LIST), gpu_match=r"scenario 1, curve item 0: unknown signal")
    for signal, (name, width) in enumerate(SIGNALS):
        for index in (width, -1):
            refused(exe, "curves", one(_with(_with(CUR_OK, 3, signal), 4, index)), at + "index %d out of range: %s has %d entries" % (index, name, width))
    # every row's addresses are judged before any item is read
    t = csr([[_with(CUR_OK, 2, 0)], [], []], CUR_COLS)
    refused(exe, "curves", (3, np.array([0, 1, 0, 1], i32)) + t[2:], fn + ": scenario 1: row addresses must not decrease")
    # the order within an item: window, every, T, bins, lo / hi, signal, index
    refused(exe, "curves", one((0, 5, 0, 9, -1, NAN, 0.0, 65)), at + "every 0 is below 1")
    refused(exe, "curves", one((0, 5, 1, 9, -1, NAN, 0.0, 65)), at + "bins 65 outside 0..64")
    refused(exe, "curves", one((0, 5, 1, 9, -1, NAN, 0.0, 4)), at + "lo / hi is not finite")
    refused(exe, "curves", one((0, 5, 1, 9, -1, 0.0, 0.0, 4)), at + "hi is not above lo")
    refused(exe, "curves", one((0, 5, 1, 9, -1, 0.0, 1.0, 4)), at + "unknown signal 9 " + SIGNAL_LIST)


def test_curve_design_limits(exe):
    fn = "cosim_scenario_curves_set"
    # 64 scenarios of 8 items x 2 classes x 72 x 1024 words are 288 MiB of cells; item 455 = scenario 56, item 7 crosses 256 MiB
    n = 64 * 8
    big = (64, np.arange(0, n + 1, 8, dtype=i32), np.tile(np.array([0, 1024, 1], i32), (n, 1)), np.zeros(n, i32), np.zeros(n, i32), np.zeros(n, f32),
           np.ones(n, f32), np.full(n, 64, i32))
    refused(exe, "curves", big, fn + ": scenario 56, curve item 7: the cells would exceed 256 MiB (a design limit)",
            gpu_match=r"scenario 56, curve item \d: the cells would exceed 256 MiB")
    adr = big[1][:58].copy()
    adr[57] = 455                                                                               # the same table up to the item before that one
    ok = run(exe, "curves", [(57, adr) + tuple(a[:455] for a in big[2:])])
    assert ok[0] == "OK" and ok[1]["cells"] == [455 * 2 * 72 * 1024] and ok[1]["cells"][0] * 4 <= 256 << 20
    # the stage: 8192 words per env; 8192 envs are 256 MiB exactly, one more is refused
    row = csr([[(0, 1024, 1, 0, 0, 0.0, 1.0, 0)] * 8], CUR_COLS)
    assert run(exe, "curves", [row], n_envs=8192)[1]["SW"] == [8192]
    refused(exe, "curves", row, fn + ": the stage, 8192 words for each of 8193 envs, would exceed 256 MiB (a design limit)", n_envs=8193)


# ------------------------------------------------------------------------------------------------------------------- 2: the packing
def _placed(got, order, total=None):
    """Each array sits where the documented order puts it, and is read back whole through its patched pointer."""
    status, val, arr, words = got
    assert status == "OK" and list(arr) == [name for name, _ in order]
    off = 0
    for name, want in order:
        w = np.ascontiguousarray(want).view(i32).ravel()
        assert arr[name][0] == off, name
        np.testing.assert_array_equal(arr[name][1], w, err_msg=name)
        off += w.size
    assert words == off
    return val


def test_scenario_image(exe):
    rng = np.random.default_rng(3)
    keys = [[], [(4,) + tuple(rng.uniform(-1, 1, CD))], [(2 * k + 1,) + tuple(rng.uniform(-1, 1, CD)) for k in range(64)]]
    pushes = [[(k, k + 3) + tuple(rng.uniform(-1, 1, 3)) for k in range(64)], [], [(0, 1 << 30, 0.5, 0.0, -0.5)]]
    n_scn, kadr, kt, kc, padr, pt, pv = tab = scenario(keys, pushes)
    val = _placed(run(exe, "scenario", [tab]), [("key_adr", kadr), ("push_adr", padr), ("key_t", kt), ("push_t", pt), ("key_cmd", kc), ("push_v", pv)])
    assert val["nkey"] == [65] and val["npush"] == [65] and val["n_scn"] == [3] and val["cd"] == [CD]
    # no command: keyframes carry times only, and key_cmd may be null
    tab0 = (2, np.array([0, 1, 2], i32), np.array([0, 5], i32), None, np.array([0, 0, 0], i32), None, None)
    val = _placed(run(exe, "scenario", [tab0], dims=DIMS[:5] + (0,) + DIMS[6:]),
                  [("key_adr", tab0[1]), ("push_adr", tab0[4]), ("key_t", tab0[2]), ("push_t", np.zeros(0, i32)), ("key_cmd", np.zeros(0, f32)), ("push_v", np.zeros(0, f32))])
    assert val["nkey"] == [2] and val["npush"] == [0] and val["cd"] == [0]


def test_params_image_and_words(exe):
    rng = np.random.default_rng(4)
    fields = [(0, NU, P_KP), (1, NU, P_KD), (2, NGEOM, P_GMU), (3, NV, P_FLOSS)]
    items = []
    for k in range(257):
        f, width, _ = fields[k % 4]
        items.append((k, k + 1 + k % 7, f, int(rng.integers(width)) if k >= 8 else (0 if k < 4 else width - 1), k % 2, float(rng.uniform(0.5, 2.0))))
    n_scn, adr, t, field, index, op, value = tab = csr([[], items[:1], items[1:]], PAR_COLS)
    word = np.array([fields[f][2] + i for f, i in zip(field, index)], dtype=i32)                 # offset + index
    val = _placed(run(exe, "params", [tab]), [("adr", adr), ("t", t), ("word", word), ("op", op), ("value", value)])
    assert val["n"] == val["n_items"] == [257] and val["word"] == word.tolist() and val["n_scn"] == [3]
    assert {P_KP, P_KP + NU - 1, P_KD, P_KD + NU - 1, P_GMU, P_GMU + NGEOM - 1, P_FLOSS, P_FLOSS + NV - 1} <= set(val["word"])


def test_checks_image_and_items_per_env(exe):
    rng = np.random.default_rng(5)

    def item(k):
        s = k % 8
        return (k, k + 1 + k % 5, s, int(rng.integers(SIGNALS[s][1])), k % 3, k % 2, float(rng.uniform(-1, 1)))
    n_scn, adr, t, sig, idx, mode, cmp, bound = tab = csr([[], [item(0)], [item(k) for k in range(1, 65)]], CHK_COLS)
    val = _placed(run(exe, "checks", [tab]), [("adr", adr), ("t", t), ("signal", sig), ("index", idx), ("mode", mode), ("cmp", cmp), ("bound", bound)])
    assert val["n"] == val["n_items"] == [65] and val["I"] == val["tab_I"] == [64] and val["n_scn"] == [3]
    for most, I in ((1, 2), (2, 2), (3, 4), (63, 64)):                                          # the largest row, rounded up to even
        assert run(exe, "checks", [csr([[item(0)], [item(k) for k in range(most)], []], CHK_COLS)])[1]["I"] == [I]


def test_curves_image_and_layout(exe):
    from cosim_amd.curves import layout
    rng = np.random.default_rng(6)

    def item(k):
        s, every = k % 8, 1 + k % 3
        t0 = int(rng.integers(0, 50))
        return (t0, t0 + int(rng.integers(1, 1024 * every - every + 2)), every, s, int(rng.integers(SIGNALS[s][1])), float(rng.uniform(-2, 0)), float(rng.uniform(0.5, 2)),
                [0, 1, 7, 64][k % 4])
    items = [item(k) for k in range(9)]
    items[3] = (0, 1024, 1) + items[3][3:]                                                        # T = 1024, the most
    n_scn, adr, t, sig, idx, lo, hi, bins = tab = csr([[], items[:1], items[1:]], CUR_COLS)
    L = layout((adr, t, sig, idx, lo, hi, bins))
    inv_w = np.array([f32(float(b) / (float(h) - float(l))) if b > 0 else f32(0) for b, l, h in zip(bins, lo, hi)], dtype=f32)
    derived = {"nt": L["T"].astype(i32), "soff": L["soff"].astype(i32), "coff": L["coff"].astype(i32), "cw": L["cw"].astype(i32), "inv_w": inv_w}
    val = _placed(run(exe, "curves", [tab]), [("adr", adr), ("t", t), ("signal", sig), ("index", idx), ("bins", bins), ("nt", derived["nt"]), ("soff", derived["soff"]),
                                              ("coff", derived["coff"]), ("cw", derived["cw"]), ("lo", lo), ("hi", hi), ("inv_w", inv_w)])
    assert val["n"] == val["n_items"] == [9] and val["n_scn"] == [3]
    assert val["cells"] == [L["words"]] and val["SW"] == val["tab_SW"] == [L["stage_words"]] and L["T"].max() == 1024
    for name, want in derived.items():
        assert val[name] == want.view(i32).tolist(), name


# ------------------------------------------------------------------------------------------------------------ 3: the in-place test
def test_in_place_predicates(exe):
    a = [(0, 20, 1, 0, 1, 0.0, 1.0, 4), (5, 25, 2, 2, 0, -1.0, 1.0, 0)]
    b = [(3, 11, 1, 5, 2, 0.0, 2.0, 8)]
    base = csr([a, [], b], CUR_COLS)
    same = lambda x: run(exe, "same_curves", [base, x])   # noqa: E731
    # other windows of the same length, signals, indices, ranges: in place
    assert same(csr([[(7, 27, 1, 1, 0, -3.0, 3.0, 4), (0, 20, 2, 6, 1, 0.0, 9.0, 0)], [], [(0, 8, 1, 0, 3, 1.0, 2.0, 8)]], CUR_COLS)) == ("same", 1)
    assert same(base) == ("same", 1)
    assert same(csr([a, b[:0], b], CUR_COLS)) == ("same", 1)
    assert same(csr([a[:1], a[1:], b], CUR_COLS)) == ("same", 0), "one row address differs"
    long = [(0, 100, 1, 0, 0, 0.0, 1.0, 0)]                                                     # a row that sets the stage words of both
    assert run(exe, "same_curves", [csr([a, [], b, long], CUR_COLS), csr([a[:1], a[1:], b, long], CUR_COLS)]) == ("same", 0), \
        "one row address differs: the same S, n, stage words and cell words"
    assert run(exe, "same_curves", [csr([a, [], b, long], CUR_COLS), csr([a, [], b, [_with(long[0], 4, 2)]], CUR_COLS)]) == ("same", 1)
    assert same(csr([[_with(a[0], 7, 5), a[1]], [], b], CUR_COLS)) == ("same", 0), "one bins differs"
    assert same(csr([[_with(a[0], 1, 21), a[1]], [], b], CUR_COLS)) == ("same", 0), "one window is a step longer"
    assert same(csr([[a[0], (5, 25, 1) + a[1][3:]], [], b], CUR_COLS)) == ("same", 0), "one window is sampled twice as often"
    assert same(csr([a, [], b, []], CUR_COLS)) == ("same", 0), "one more scenario"
    c = [(0, 9, 0, 0, 0, 0, 1.0), (2, 5, 3, 0, 1, 1, 2.0), (0, 4, 5, 2, 2, 0, 0.5)]
    base = csr([c[:2], [], c[2:]], CHK_COLS)
    same = lambda x: run(exe, "same_checks", [base, x])   # noqa: E731
    assert same(csr([[(1, 3, 1, 1, 1, 1, -1.0), (0, 50, 6, 3, 0, 0, 7.0)], [], [(9, 10, 2, 1, 0, 1, 0.0)]], CHK_COLS)) == ("same", 1)
    assert same(csr([c[:2], c[2:], []], CHK_COLS)) == ("same", 0), "one row address differs (the same S, n and I)"
    assert same(csr([c[:1], [], c[1:]], CHK_COLS)) == ("same", 0)
    assert same(csr([c[:2], [], c[2:] + c[2:]], CHK_COLS)) == ("same", 0), "one more item"


# ------------------------------------------------------------------------------------------------- 4: what the change left alone
def test_device_code_is_what_it_was():
    """profiles/tables_refactor_codeobj.txt: the gfx950 code object of cosim_engine.hip before and after the host code moved."""
    text = open(os.path.join(ROOT, "profiles", "tables_refactor_codeobj.txt")).read()
    h = dict(re.findall(r"^text_sha256_(parent|this)\s+([0-9a-f]{64})$", text, flags=re.M))
    assert set(h) == {"parent", "this"} and h["parent"] == h["this"]
    assert re.search(r"^ksize_tables\s+identical$", text, flags=re.M) and re.search(r"^kres_tables\s+identical$", text, flags=re.M)


def test_device_code_is_what_it_was_before_the_owning_buffers():
    """profiles/devbuf_codeobj.txt: the same comparison across the change that gave every device allocation an owner."""
    text = open(os.path.join(ROOT, "profiles", "devbuf_codeobj.txt")).read()
    h = dict(re.findall(r"^text_sha256_(parent|this)\s+([0-9a-f]{64})$", text, flags=re.M))
    assert set(h) == {"parent", "this"} and h["parent"] == h["this"]
    assert re.search(r"^text_section\s+byte-identical$", text, flags=re.M)
    assert re.search(r"^ksize_tables\s+identical$", text, flags=re.M) and re.search(r"^kres_tables\s+identical$", text, flags=re.M)


def test_each_rule_is_written_once():
    csrc = os.path.join(ROOT, "cosim_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)))
    assert src.count("times outside [0, 2^30)") == 1 and src.count("unknown signal ") == 1 and src.count("row addresses must not decrease") == 1


def test_the_engine_allocates_in_one_place():
    """csrc/cosim_devbuf.h owns every allocation: the four calls occur once each, in the allocator policies, and the
    hand-written cleanup helpers are gone from csrc/."""
    csrc = os.path.join(ROOT, "cosim_amd", "csrc")
    engine = open(os.path.join(csrc, "cosim_engine.hip")).read()
    for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("):
        assert engine.count(call) == 1, call
    policies = engine[engine.index("struct HipDevice"):engine.index("template <class T> using Dev")]
    assert all(call in policies for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree("))
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)))
    for name in ("scnparams_free", "obsfault_free", "actfault_free", "latency_drop", "latency_free", "checks_free", "curves_free", "search_free",
                 "ledger_free", "ftrace_free", "rotate_free", "table_free", "DbgBuf"):
        assert not re.search(r"\b%s\b" % name, src), name
    # the four that must name no buffer: they assign groups and delete, nothing else
    for fn in ("int cosim_destroy", "int cosim_policy_table_destroy", "int cosim_recurrent_table_destroy", "static void scenario_free"):
        body = engine[engine.index("%s(" % fn):]
        body = body[:body.index("\n}\n")]
        assert ".get()" not in body and ".reset()" not in body and "d_" not in body, fn
