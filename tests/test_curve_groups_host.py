"""Response curves split by group, on the host (no GPU): the numpy twin (cosim_amd/curves.py reference_curves(groups=...)) against a
hand-written case whose planes are written out by hand; the grouped rule of csrc/cosim_curves.h (the group fields of CurArgs,
curves_fold_group_lane) compiled as plain C++ (tests/curve_groups_lanes.cpp), driven lane by lane against the twin and a second time
under AddressSanitizer / UBSan as a stand-alone child process; the merge identity (the planes merged are the cells without groups);
the group axis of ``Curves``; validation messages; and the kernel-resource tables recorded before and after the change.  Every
comparison of cells is exact: words as words."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
K, N, G, NU, CD, NQ, NV = 12, 4, 3, 1, 1, 7, 6
NI = 4 + 2 * NU + 1
Q = 1 << 20                                                             # one unit of the fixed-point sum
S16 = Q // 16

ROW0 = [[0, 6, 1, "info", "lin_vel_x", 0.0, 1.0, 2, "vx"]]             # A: every step, T = 6, two bins of 0.5: 10 * 6 words per class
ROW1 = [[0, 4, 2, "qpos", 2, 0.0, 1.0, 0, "height"]]                    # D: a state signal at t = 0, 2; no histogram: 8 * 2 words per class
NAMES = {"info": {"action_diff_RMSE": (0, 1), "lin_vel_x": (1, 1), "lin_vel_y": (2, 1), "ang_vel_yaw": (3, 1), "torque": (4, NU), "set_points": (4 + NU, NU),
                  "state": (4 + 2 * NU, 1)}, "info_dim": NI, "command_dim": CD, "nq": NQ, "nv": NV, "qpos": {"root": 0}, "qvel": {"root": 0, "hip": 0}}
POLICIES = ["ckpt_a", "ckpt_b", "ckpt_c"]


def _table(rows=(ROW0, ROW1)):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable([{"commands": [[0, 0.5]], "curves": list(r)} for r in rows], CD, names={"checks": NAMES})


def _hand_case(env2_late=-1):
    """12 steps of four envs under two scenarios (mode env: envs 0, 2 run row 0, envs 1, 3 row 1), G = 3.  In step k every env's
    lin_vel_x and height are (k + 1) / 16.
      env 0: word 0 while its first episode runs (truncated in step 3, clock 3), word 2 from step 4 on (its second episode is
             terminated in step 9 at clock 5): plane 0 class 0 gets t = 0 .. 3, plane 2 class 1 gets t = 0 .. 5; steps 10, 11 are open
      env 1: word 1; terminated in step 5 at clock 5, past D's window: plane 1 class 1 of row 1 gets t = 0, 2
      env 2: word -1: truncated in step 6 (clock 6), terminated in step 9 (clock 2), truncated in step 11 (clock 1): three episodes in no
             plane.  With ``env2_late = 1`` the word is 1 from step 7 on: the first episode (t = 0 .. 5 staged) is still in no plane, the
             second lands in plane 1 class 1 with t = 0 .. 2 ALONE (the lost episode's stage was emptied), the third in plane 1 class 0
      env 3: word G = 3: terminated in step 2 (clock 2, a done row: D takes no sample there) and truncated in step 11: two episodes in
             no plane"""
    c = {"info": np.zeros((K, N, NI), dtype=f32), "cmd": np.full((K, N, CD), 0.5, dtype=f32),
         "qpos": np.zeros((K, N, NQ), dtype=f32), "qvel": np.zeros((K, N, NV), dtype=f32)}
    v = ((np.arange(K) + 1) / 16.0).astype(f32)
    c["info"][:, :, 1] = v[:, None]
    c["qpos"][:, :, 2] = v[:, None]
    c["qpos"][:, :, 3] = 1.0                                            # an upright quaternion (no item reads it)
    te, tr = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    tr[3, 0] = te[9, 0] = 1
    te[5, 1] = 1
    tr[6, 2] = te[9, 2] = tr[11, 2] = 1
    te[2, 3] = tr[11, 3] = 1
    c["term"], c["trunc"] = te, tr
    clock = np.zeros((K + 1, N), dtype=np.int32)                         # meta word 0 before step k; row K: after the last step
    clock[:, 0] = [0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 0, 1, 2]
    clock[:, 1] = [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 6]
    clock[:, 2] = [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 0, 1, 0]
    clock[:, 3] = [0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0]
    c["clock"] = clock
    c["rows"] = np.tile(np.array([0, 1, 0, 1]), (K, 1))
    grp = np.tile(np.array([0, 1, -1, G], dtype=np.int32), (K, 1))
    grp[4:, 0] = 2
    grp[7:, 2] = env2_late
    c["groups"] = grp
    return c


def _twin(c, table, n_groups=G, envs=slice(None), **kw):
    from cosim_amd.curves import reference_curves
    more = {} if not n_groups else {"groups": c["groups"][:, envs], "n_groups": n_groups}
    return reference_curves(table, c["info"][:, envs], c["term"][:, envs], c["trunc"][:, envs], c["cmd"][:, envs], c["qpos"][:, envs],
                            c["qvel"][:, envs], c["clock"][:, envs], c["rows"][:, envs], c.get("nu", NU), **more, **kw)


# ------------------------------------------------------------------------------------------------------------ 1: the twin, by hand
def test_grouped_twin_against_hand_written_planes():
    from cosim_amd.curves import Curves
    c, T = _hand_case(), _table()
    cv = _twin(c, T, group_names=POLICIES)
    W = 2 * 60 + 2 * 16
    assert cv.groups == G and cv.plane_words == W and cv.cells.size == G * W and cv.group_names == POLICIES and cv.grouped
    assert cv.ungrouped == 5, "three episodes of env 2 (word -1) and two of env 3 (word G)"
    nan = np.nan
    # ---- plane 0: env 0's first episode, truncated: steps 0 .. 3 are t = 0 .. 3 with v = 1/16 .. 4/16, all in [0, 0.5)
    a = cv[0, "vx", 0]
    assert a.count("truncated").tolist() == [1, 1, 1, 1, 0, 0] and a.count("terminated").sum() == 0 and a.nan().sum() == 0
    assert a._sum[0].tolist() == [S16, 2 * S16, 3 * S16, 4 * S16, 0, 0]
    assert a.hist("truncated").tolist() == [[0] * 6, [1, 1, 1, 1, 0, 0], [0] * 6, [0] * 6]
    np.testing.assert_array_equal(a.min(), np.array([1 / 16, 2 / 16, 3 / 16, 4 / 16, nan, nan], dtype=f32))
    assert cv[1, 0, 0].count().sum() == 0 and cv.group(0).episodes().tolist() == [[1, 0], [0, 0]]
    # ---- plane 2: env 0's second episode, terminated: steps 4 .. 9 are t = 0 .. 5 with v = 5/16 .. 10/16; 8/16 = 0.5 is the upper bin's
    b = cv[0, 0, "ckpt_c"]
    assert b.count("terminated").tolist() == [1] * 6 and b.count("truncated").sum() == 0
    assert b._sum[1].tolist() == [k * S16 for k in range(5, 11)]
    assert b.hist("terminated").tolist() == [[0] * 6, [1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1], [0] * 6]
    np.testing.assert_array_equal(b.max(), (np.arange(5, 11) / 16).astype(f32))
    assert cv.group("ckpt_c").episodes().tolist() == [[0, 1], [0, 0]]
    # ---- plane 1: env 1's episode on row 1: t = 0, 2 in steps 0, 2
    d = cv[1, "height", 1]
    assert d.count("terminated").tolist() == [1, 1] and d._sum[1].tolist() == [S16, 3 * S16] and d.count("truncated").sum() == 0
    assert d.hist().shape == (2, 2) and d.hist().sum() == 0
    np.testing.assert_array_equal(d.min(), np.array([1 / 16, 3 / 16], dtype=f32))
    assert cv[0, 0, 1].count().sum() == 0 and cv.group(1).episodes().tolist() == [[0, 0], [0, 1]]
    # ---- nothing else anywhere: every plane but for the words above is the empty image
    want = Curves.empty(T, G).cells.reshape(G, W).copy()
    got = cv.cells.reshape(G, W)
    for g, (base, t_bins, n) in {0: (0, 6, 4), 2: (60, 6, 6), 1: (120 + 16, 2, 2)}.items():
        touched = np.zeros(W, dtype=bool)
        for part in (0, 2, 3, 4, 5) + ((6, 7, 8, 9) if g != 1 else ()):   # count, min, max, sum (two words a bin), hist rows
            touched[base + part * t_bins:base + (part + 1) * t_bins] = True
        assert (got[g][~touched] == want[g][~touched]).all(), f"plane {g}: a word outside the episode's block changed"
        assert (got[g][touched] != want[g][touched]).sum() >= 3 * n
    # ---- two-index access is the curve over ALL groups: the planes merged
    m = cv[0, "vx"]
    assert m.count("truncated").tolist() == [1, 1, 1, 1, 0, 0] and m.count("terminated").tolist() == [1] * 6
    assert m.count().tolist() == [2, 2, 2, 2, 1, 1] and cv.episodes().tolist() == [[1, 1], [0, 1]]
    s = cv.summary()
    assert s["episodes"] == 3 and s["groups"] == G and s["ungrouped"] == 5 and list(s["by_group"]) == POLICIES
    assert [s["by_group"][n]["episodes"] for n in POLICIES] == [1, 1, 1] and s["by_group"]["ckpt_a"]["episodes_truncated"] == 1
    assert s["by_group"]["ckpt_c"]["samples"] == 6 and s["samples"] == 4 + 6 + 2

    # ---- env 2's word becomes 1 behind its first (lost) episode: the later episodes hold their own bins alone
    late = _twin(_hand_case(env2_late=1), T)
    assert late.ungrouped == 3
    e = late[0, 0, 1]
    assert e.count("terminated").tolist() == [1, 1, 1, 0, 0, 0], "bins 3 .. 5 were staged by the lost episode: its stage was not emptied"
    assert e._sum[1].tolist() == [8 * S16, 9 * S16, 10 * S16, 0, 0, 0]                  # steps 7 .. 9
    assert e.count("truncated").tolist() == [1, 1, 0, 0, 0, 0] and e._sum[0].tolist() == [11 * S16, 12 * S16, 0, 0, 0, 0]
    assert late.group(1).episodes().tolist() == [[1, 1], [0, 1]]
    assert (late.cells.reshape(G, W)[[0, 2]] == got[[0, 2]]).all()


def test_twin_argument_checks():
    c, T = _hand_case(), _table()
    from cosim_amd.curves import reference_curves
    args = (T, c["info"], c["term"], c["trunc"], c["cmd"], c["qpos"], c["qvel"], c["clock"], c["rows"], NU)
    with pytest.raises(ValueError, match="groups .* and n_groups .* go together"):
        reference_curves(*args, groups=c["groups"])
    with pytest.raises(ValueError, match="groups .* and n_groups .* go together"):
        reference_curves(*args, n_groups=3)
    with pytest.raises(ValueError, match=r"groups 65: an integer 1\.\.64"):
        reference_curves(*args, groups=c["groups"], n_groups=65)


# ------------------------------------------------------------------------------------------------------------ 2: the header as C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "curve_groups_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/curve_groups_lanes.cpp + csrc/cosim_curves.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("curve_groups")
    return _build(tmp, "lanes", []), _build(tmp, "lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run_lanes(exe, c, table, n_groups, lanes, reverse, dims):
    """``(Curves, stage words that still hold a sample per env)`` of the C++ program."""
    from cosim_amd.curves import Curves, layout
    n_envs, ni, nu, cd, nq, nv = dims
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    csr = table.pack_curves()
    adr, t, sig, idx, lo, hi, bins = csr
    L = layout(csr)
    inv_w = [f32(np.float64(b) / (np.float64(h) - np.float64(l))) if b > 0 else f32(0) for l, h, b in zip(lo, hi, bins)]
    words = [len(adr) - 1, len(sig)] + adr.tolist() + t.reshape(-1).tolist() + sig.tolist() + idx.tolist() + bins.tolist()
    words += L["T"].tolist() + L["soff"].tolist() + L["coff"].tolist() + L["cw"].tolist() + u(lo) + u(hi) + u(inv_w)
    words += [L["stage_words"], L["words"], lanes, n_envs, ni, nu, cd, nq, nv, int(reverse), n_groups] + c["clock"][0].tolist()
    for k in range(c["info"].shape[0]):
        words.append(2)
        for i in range(n_envs):
            words += [int(c["term"][k, i]), int(c["trunc"][k, i]), int(c["rows"][k, i]), int(c["clock"][k + 1, i]), int(c["groups"][k, i])]
            words += u(c["info"][k, i]) + u(c["cmd"][k, i]) + u(c["qpos"][k, i]) + u(c["qvel"][k, i])
    words.append(3)
    p = subprocess.run([exe], input=" ".join(str(w) for w in words).encode(), capture_output=True)
    assert p.returncode == 0, p.stderr[-2000:].decode(errors="replace")
    raw = np.frombuffer(p.stdout, dtype="<u4")
    assert raw.size == n_groups * L["words"] + 1 + n_envs
    held = raw[-n_envs:].astype(np.int64)
    return Curves.from_raw(raw[:n_groups * L["words"]].copy(), table, groups=n_groups, ungrouped=int(raw[n_groups * L["words"]])), held


def _random_case(seed=5, n_groups=64):
    """8 envs, 40 steps, three scenarios -- 8 items (one with T = 1024 and 64 bins), one item, 5 items -- in mode env, the clocks start
    anywhere in the windows and episodes end at random; every env's group word is redrawn from [0, G) behind each of its episodes."""
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
    grp = np.zeros((steps, n_envs), dtype=np.int32)
    now = rng.integers(0, n_groups, size=n_envs)
    for k in range(steps):
        clock[k + 1] = np.where(done[k], 0, clock[k] + 1)
        grp[k] = now
        now = np.where(done[k], rng.integers(0, n_groups, size=n_envs), now)
    c["clock"], c["rows"], c["groups"] = clock, np.tile(np.arange(n_envs) % 3, (steps, 1)), grp
    c["nu"] = nu
    return c, T, (n_envs, ni, nu, cd, nq, nv)


@pytest.fixture(scope="module")
def random_twin():
    c, T, dims = _random_case()
    return c, T, dims, _twin(c, T, 64)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("lanes", [64, 5, 1])
def test_grouped_rule_as_host_cpp_equals_the_twin(lanes_exes, random_twin, lanes, sanitized):
    """The hand-written case (G = 3, words -1 and G among them) and a random one with 8 items, T = 1024, B = 64 and G = 64 through the
    functions curves_step_grouped_kernel calls, with 64 lanes (the wave), 5 and 1, the two ranges of a step in either order: the planes
    and the ``ungrouped`` count equal the twin's word for word, and a lost episode leaves its stage clean."""
    from cosim_amd.curves import same_curves
    exe = lanes_exes[1 if sanitized else 0]
    T = _table()
    for reverse, late in ((False, -1), (True, -1), (False, 1), (True, 1)):
        c = _hand_case(env2_late=late)
        got, held = _run_lanes(exe, c, T, G, lanes, reverse, (N, NI, NU, CD, NQ, NV))
        want = _twin(c, T)
        assert same_curves(got, want) is None, same_curves(got, want)
        assert got.ungrouped == (5 if late < 0 else 3)
        assert held.tolist() == [2, 2, 0, 0], "the open episodes of envs 0 and 1 hold t = 0, 1 and t = 0, 2; envs 2 and 3 ended their last episode in the last step: nothing may be staged"
    c, T, dims, want = random_twin
    for reverse in (False, True):
        got, _ = _run_lanes(exe, c, T, 64, lanes, reverse, dims)
        assert same_curves(got, want) is None, same_curves(got, want)
    assert want.ungrouped == 0 and want.groups == 64 and want.cells.size == 64 * want.plane_words
    used = [g for g in range(64) if want.group(g).summary()["samples"] > 0]
    big = want[0, 3]
    assert len(used) >= 8 and big.t.size == 1024 and big.bins == 64 and big.count().sum() > 0
    s = want.summary()
    assert s["episodes_truncated"] > 0 and s["episodes_terminated"] > 0 and s["nonfinite"] > 0


# ------------------------------------------------------------------------------------------------------------ 3: merge identity
def test_merged_planes_equal_the_ungrouped_twin(random_twin):
    """Each plane is a whole cell image, so the planes merged by ``Curves.merge``'s rule are the cells without groups whenever no
    episode was lost; a plane is the ungrouped twin of the episodes that carried its word."""
    from cosim_amd.curves import same_curves
    c, T, dims, grouped = random_twin
    flat = _twin(c, T, 0)
    assert grouped.ungrouped == 0 and not flat.grouped and flat.groups == 1
    assert same_curves(grouped.merged(), flat) is None, same_curves(grouped.merged(), flat)
    for s, k in flat.items():                                             # two-index access reads the merged planes
        for name in ("count", "nan", "hist"):
            np.testing.assert_array_equal(grouped[s, k].both(name), flat[s, k].both(name))
        np.testing.assert_array_equal(grouped[s, k]._sum, flat[s, k]._sum)
        np.testing.assert_array_equal(grouped[s, k]._min, flat[s, k]._min)
    assert grouped.episodes().tolist() == flat.episodes().tolist()
    # fewer groups over the same records: words taken mod 3
    c3 = dict(c, groups=c["groups"] % 3)
    g3 = _twin(c3, T, 3)
    assert same_curves(g3.merged(), flat) is None and all(p.summary()["samples"] > 0 for p in g3.by_group().values())
    # the hand case lost episodes: its planes merged are NOT the ungrouped cells
    h, HT = _hand_case(), _table()
    assert same_curves(_twin(h, HT).merged(), _twin(h, HT, 0)) is not None


# ------------------------------------------------------------------------------------------------------------ 4: the container
def test_curves_group_axis(tmp_path):
    from cosim_amd.curves import Curves, same_curves
    c, T = _hand_case(env2_late=1), _table()
    cv = _twin(c, T, group_names=POLICIES)
    planes = cv.by_group()
    assert list(planes) == POLICIES and all(p.groups == 1 and not p.grouped and p.cells.size == cv.plane_words for p in planes.values())
    assert same_curves(planes["ckpt_b"], cv.group(1)) is None and same_curves(cv.group("ckpt_b"), cv.group(1)) is None
    np.testing.assert_array_equal(cv.group(2).cells, cv.cells[2 * cv.plane_words:])
    assert cv[0, "vx", "ckpt_b"].count().tolist() == cv[0, 0, 1].count().tolist() == [2, 2, 1, 0, 0, 0]
    for bad in ("nope", 3, -1, 1.5, True):
        with pytest.raises(KeyError, match="no group"):
            cv.group(bad)
    with pytest.raises(KeyError, match="no group 'ckpt_d'"):
        cv[0, 0, "ckpt_d"]
    # merge: plane by plane, the lost counts add; G and the names must agree
    twice = cv.merge(cv)
    assert twice.groups == G and twice.group_names == POLICIES and twice.ungrouped == 6
    assert same_curves(twice.group(1), cv.group(1).merge(cv.group(1))) is None and twice[0, 0, 1].count().tolist() == [4, 4, 2, 0, 0, 0]
    np.testing.assert_array_equal(twice[0, 0, 1]._min, cv[0, 0, 1]._min)
    with pytest.raises(ValueError, match="different groups: 3 .* against 1"):
        cv.merge(_twin(c, T, 0))
    with pytest.raises(ValueError, match="different groups: 3 .* against 2"):
        cv.merge(Curves.empty(T, 2))
    with pytest.raises(ValueError, match="different groups"):
        cv.merge(_twin(c, T))                                             # the same G under other names
    assert "the groups differ" in same_curves(cv, _twin(c, T, 0)) and "ungrouped episodes: 3 against 5" in same_curves(cv, _twin(_hand_case(), T, group_names=POLICIES))
    diff = same_curves(cv, _twin(_hand_case(env2_late=0), T, group_names=POLICIES))
    assert diff is not None and "group 0 ('ckpt_a')" in diff
    # word kinds: one plane's, tiled
    kind = cv.word_kinds()
    assert kind.shape == cv.cells.shape and (kind.reshape(G, -1) == cv.group(0).word_kinds()).all()
    cells = cv.cells.copy()
    cells[kind == 0] += cv.cells[kind == 0]
    cells[kind == 3] = (2 * cv.cells[kind == 3].view(np.int64)).view(np.uint32)
    np.testing.assert_array_equal(cells, twice.cells)
    # cell counts that do not fit
    with pytest.raises(ValueError, match=r"456 cell words, the items need 152 in each of 2 planes"):
        Curves(cv.cells, cv.adr, cv.spec, cv.lohi, cv.bins, cv.names, groups=2)
    with pytest.raises(ValueError, match="group_names must be 3 different strings"):
        Curves(cv.cells, cv.adr, cv.spec, cv.lohi, cv.bins, cv.names, groups=3, group_names=["a", "a", "b"])
    # .npz round trip with the group axis
    path = str(tmp_path / "grouped.npz")
    cv.save(path)
    back = Curves.load(path)
    assert same_curves(back, cv) is None and back.group_names == POLICIES and back.ungrouped == 3 and back.names == cv.names and back.grouped
    s = back.summary()
    assert s["by_group"]["ckpt_b"]["episodes"] == 3 and s["groups"] == 3 and s["ungrouped"] == 3
    assert s["episodes"] == cv.merged().summary()["episodes"] and "by_group" not in cv.group(1).summary()
    # ungrouped curves keep the earlier file, and a file written before there were groups -- plain arrays, no group keys -- still loads
    flat = _twin(c, T, 0)
    flat.save(str(tmp_path / "flat.npz"))
    with np.load(str(tmp_path / "flat.npz"), allow_pickle=False) as z:
        assert set(z.files) == {"cells", "adr", "spec", "lohi", "bins", "names"}
    old = str(tmp_path / "old.npz")
    np.savez(old, cells=flat.cells, adr=flat.adr, spec=flat.spec, lohi=flat.lohi, bins=flat.bins,
             names=np.array([["vx"], ["height"]], dtype=np.str_))
    o = Curves.load(old)
    assert same_curves(o, flat) is None and o.groups == 1 and not o.grouped and o.names == [["vx"], ["height"]] and o.ungrouped == 0
    assert Curves(flat.cells, flat.adr, flat.spec, flat.lohi, flat.bins, flat.names).groups == 1     # the positional call of before


# ------------------------------------------------------------------------------------------------------------ 5: messages
def test_set_curve_groups_and_table_messages(tmp_path):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.policy import PolicyTable, write_random_mlp
    env = types.SimpleNamespace(curves_armed=False, torch=torch, num_envs=4, device=torch.device("cuda:0"), _curve_groups=None)
    words = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"set_curve_groups\(\): no curves are armed"):
        BatchedEnv.set_curve_groups(env, words, 3)
    env.curves_armed = True
    with pytest.raises(ValueError, match="a group tensor needs n_groups"):
        BatchedEnv.set_curve_groups(env, words)
    with pytest.raises(ValueError, match=r"contiguous int32 tensor \[4\] on cuda:0, got torch.int32 \(4,\) on cpu"):
        BatchedEnv.set_curve_groups(env, words, 3)
    with pytest.raises(ValueError, match=r"got torch.int64 \(4,\)"):
        BatchedEnv.set_curve_groups(env, words.long(), 3)
    with pytest.raises(ValueError, match=r"got torch.int32 \(5,\)"):
        BatchedEnv.set_curve_groups(env, torch.zeros(5, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="got list"):
        BatchedEnv.set_curve_groups(env, [0, 1, 2, 0], 3)
    env.device = torch.device("cpu")                                      # (only to get past the tensor test without a GPU)
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match=r"n_groups .*: an integer 1\.\.64"):
            BatchedEnv.set_curve_groups(env, words, bad)
    with pytest.raises(ValueError, match="names must be 3 different strings"):
        BatchedEnv.set_curve_groups(env, words, 3, names=["a", "b"])
    files = []
    for k in range(2):
        files.append(str(tmp_path / f"p{k}.onnx"))
        write_random_mlp(files[-1], 6, 2, hidden=(8,), seed=k)
    for rot in (None, 1):
        tab = PolicyTable(files, 4, device="cpu", fused=False, rotate_every=rot)
        with pytest.raises(ValueError, match=r"PolicyTable.curve_groups: the table is on 'cpu'"):
            tab.curve_groups()
        with pytest.raises(ValueError, match="a policy table brings its own n_groups"):
            BatchedEnv.set_curve_groups(env, tab, 2)
    with pytest.raises(ValueError, match="the table was built for 5 envs, the env has 4"):
        BatchedEnv.set_curve_groups(env, PolicyTable(files, 5, device="cpu", fused=False))


# ------------------------------------------------------------------------------------------------------------ 6: resources
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/curve_groups_kres_parent.txt) and after (curve_groups_kres_this.txt): every existing kernel's line
    is identical, in the same order -- curves_step_kernel and curves_clear_kernel among them; the two added lines are the grouped
    kernels', which use no LDS, no scratch and spill nothing."""
    head_a, a = _table_file("curve_groups_kres_parent.txt")
    head_b, b = _table_file("curve_groups_kres_this.txt")
    assert head_a == head_b and len(a) >= 43
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    assert any(ln.startswith("curves_step_kernel(") for ln in a) and any(ln.startswith("curves_clear_kernel(") for ln in a)
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["curves_clear_grouped_kernel", "curves_step_grouped_kernel"]
    for name, (vgpr, agpr, sspill, vspill, scratch, occ, lds) in added.items():
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and occ >= 1, name
