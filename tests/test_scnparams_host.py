"""Parameter windows of a scenario table on the host (no GPU): the numpy twin (cosim_amd/scenario.py reference_params) against
expectations written out by hand, CSR packing, the sweep generator's new axis, the validation messages, the kernel's per-env body
(csrc/cosim_scnparams.h) compiled as plain C++ and driven lane by lane against the twin -- once more under AddressSanitizer and
UBSan, as a stand-alone child process --, and the kernel-resource and code-size tables recorded before and after the change."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CD = 4
f32 = np.float32

# a small made-up model: 3 bodies, 8 dofs (a free joint and two hinges), 5 geoms, 4 actuators
NAMES = {"kp": ["hip_l", "hip_r", "knee_l", "knee_r"], "kd": ["hip_l", "hip_r", "knee_l", "knee_r"],
         "geom_friction": ["torso", "shin_l", "shin_r", "foot_l", "foot_r"],
         "dof_frictionloss": ["root"] * 6 + ["knee_l", "knee_r"]}
# record: body_mass 0..2 | body_invweight0 3..5 | dof_invweight0 6..13 | dof_frictionloss 14..21 | geom_friction 22..26 | kp 27..30 |
# kd 31..34 | meaninertia 35 | padding to 64
FLOSS, GMU, KP, KD, STRIDE = 14, 22, 27, 31, 64
TABLE3 = [
    # 0: a "*" window under a single-index window; two overlapping windows on kp[1], the last LISTED wins; scale by 0 and set
    {"params": [[5, 12, "kp", "*", "scale", 0.5], [8, 10, "kp", "hip_r", "set", 7.0], [9, 11, "kp", 1, "scale", 0.0]]},
    # 1: a slippery foot by name, a limp knee (kp = kd = 0), a joint that binds: the name "root" is the free joint's six dofs
    {"commands": [[0, 0.3, 0.0, 0.0, 0.0]],
     "params": [[0, 3, "geom_friction", "foot_l", "scale", 0.25], [3, 6, "kp", 2, "scale", 0.0], [3, 6, "kd", "knee_l", "set", 0.0],
                [20, 30, "dof_frictionloss", "root", "set", 0.75], [21, 22, "dof_frictionloss", 7, "scale", 3.0]]},
    # 2: no window
    {"pushes": [[1, 2, 0.1, 0.0, 0.0]]},
]


def _table(names=NAMES):
    from cosim_amd.scenario import ScenarioTable
    return ScenarioTable(TABLE3, CD, names=names)


def _base(n, stride=STRIDE):
    """Distinct words, exact in float32: env i, word w -> 1 + w / 8 + 16 i."""
    return (1.0 + np.arange(stride)[None, :] / 8.0 + 16.0 * np.arange(n)[:, None]).astype(f32)


def _layout():
    from cosim_amd.scenario import param_layout
    lay = param_layout(nbody=3, nv=8, ngeom=5, nu=4)
    assert lay == {"dof_frictionloss": FLOSS, "geom_friction": GMU, "kp": KP, "kd": KD, "stride": STRIDE}
    return lay


def _eff(table, mode, gid, t, ep, base=None, layout=None):
    from cosim_amd.scenario import reference_params
    gid = np.atleast_1d(gid)
    base = _base(len(gid)) if base is None else base
    return reference_params(table, mode, gid, np.broadcast_to(t, gid.shape), np.broadcast_to(ep, gid.shape), base, layout or _layout())


# ------------------------------------------------------------------------------------------------------------ the twin, by hand
def test_twin_against_hand_written_table():
    T = _table()
    assert len(T) == 3 and T.has_params and T.n_param_items == 6 + 10 and [len(p) for p in T.params] == [6, 10, 0]
    b = _base(1)[0]
    kp = b[KP:KP + 4].copy()                                        # 4.375, 4.5, 4.625, 4.75
    assert kp.tolist() == [4.375, 4.5, 4.625, 4.75]

    def row0(t):
        return _eff(T, "env", 0, t, 0)[0]

    def only(e, words):                                             # every word outside `words` is the base word, bit for bit
        rest = np.setdiff1d(np.arange(STRIDE), words)
        return np.array_equal(e[rest].view(np.uint32), b[rest].view(np.uint32))
    # t = t0 - 1, t0, t1 - 1, t1 of the "*" window [5, 12)
    assert np.array_equal(row0(4).view(np.uint32), b.view(np.uint32))
    assert row0(5)[KP:KP + 4].tolist() == [2.1875, 2.25, 2.3125, 2.375] and only(row0(5), np.arange(KP, KP + 4))
    assert row0(11)[KP:KP + 4].tolist() == [2.1875, 2.25, 2.3125, 2.375]
    assert np.array_equal(row0(12).view(np.uint32), b.view(np.uint32))
    # the single-index window [8, 10) over the "*" window: t = 7, 8; from t = 9 the window listed last, [9, 11), scales by 0
    assert row0(7)[KP + 1] == f32(2.25)
    assert row0(8)[KP:KP + 4].tolist() == [2.1875, 7.0, 2.3125, 2.375]
    assert row0(9)[KP:KP + 4].tolist() == [2.1875, 0.0, 2.3125, 2.375]   # set 7 holds too; the last LISTED wins
    assert row0(10)[KP:KP + 4].tolist() == [2.1875, 0.0, 2.3125, 2.375]  # t1 - 1 of [9, 11), t1 of [8, 10)
    assert row0(11)[KP + 1] == f32(2.25) and only(row0(9), np.arange(KP, KP + 4))
    # scenario 1 (env 1; its base is 16 higher): friction by name, the limp knee, the free joint's six dofs
    b1 = _base(2)[1]

    def row1(t):
        return _eff(T, "env", [0, 1], t, 0)[1]
    e = row1(0)
    assert b1[GMU + 3] == f32(20.125) and e[GMU + 3] == f32(5.03125)
    rest = np.setdiff1d(np.arange(STRIDE), [GMU + 3])
    assert np.array_equal(e[rest].view(np.uint32), b1[rest].view(np.uint32))
    assert row1(2)[GMU + 3] == e[GMU + 3] and row1(3)[GMU + 3] == b1[GMU + 3]
    e = row1(3)
    assert e[KP + 2] == 0.0 and e[KD + 2] == 0.0 and e[KP + 1] == b1[KP + 1] and e[KD + 1] == b1[KD + 1]
    assert row1(5)[KP + 2] == 0.0 and row1(6)[KP + 2] == b1[KP + 2] and row1(6)[KD + 2] == b1[KD + 2] and row1(2)[KD + 2] == b1[KD + 2]
    e = row1(21)
    assert e[FLOSS:FLOSS + 6].tolist() == [0.75] * 6 and e[FLOSS + 6] == b1[FLOSS + 6] and e[FLOSS + 7] == f32(b1[FLOSS + 7] * f32(3.0))
    assert row1(19)[FLOSS] == b1[FLOSS] and row1(20)[FLOSS] == f32(0.75) and row1(29)[FLOSS] == f32(0.75) and row1(30)[FLOSS] == b1[FLOSS]
    assert row1(20)[FLOSS + 7] == b1[FLOSS + 7] and row1(22)[FLOSS + 7] == b1[FLOSS + 7]
    # scenario 2 has no window: base at every t
    for t in (0, 1, 5, 9, 21):
        e = _eff(T, "env", [0, 1, 2], t, 0)
        assert np.array_equal(e[2].view(np.uint32), _base(3)[2].view(np.uint32))


def test_twin_cycle_changes_rows_between_episodes():
    T = _table()
    b = _base(3)
    for ep in range(7):
        e = _eff(T, "cycle", [0, 1, 2], 9, ep)                      # t = 9: only scenario 0 changes anything (kp)
        for g in range(3):
            row = (g + ep) % 3
            want = b[g].copy()
            if row == 0:
                want[KP:KP + 4] = b[g, KP:KP + 4] * f32(0.5)
                want[KP + 1] = 0.0
            assert np.array_equal(e[g].view(np.uint32), want.view(np.uint32)), (g, ep)
    e = _eff(T, "env", [0, 1, 2], 9, 5)                             # mode env ignores the episode count
    assert (e[0, KP + 1] == 0.0) and np.array_equal(e[1:].view(np.uint32), b[1:].view(np.uint32))
    e = _eff(T, "env", [3, 301], 4, 0, base=_base(2))               # row = global id mod S: 0 and 1
    assert e[0, KP] == b[0, KP] and e[1, KP + 2] == 0.0


# ------------------------------------------------------------------------------------------------------------ packing, sweep
def test_pack_round_trip(tmp_path):
    import yaml
    from cosim_amd.scenario import ScenarioTable
    T = _table()
    adr, t, field, index, op, value = T.pack_params()
    assert adr.tolist() == [0, 6, 16, 16] and adr.dtype == np.int32 and t.shape == (16, 2) and value.dtype == f32
    assert field[:6].tolist() == [0] * 6 and index[:6].tolist() == [0, 1, 2, 3, 1, 1] and op[:6].tolist() == [0, 0, 0, 0, 1, 0]
    assert field[6:].tolist() == [2, 0, 1] + [3] * 7 and index[6:].tolist() == [3, 2, 2, 0, 1, 2, 3, 4, 5, 7]
    back = T.params_from_csr(adr, t, field, index, op, value, names=NAMES)
    assert back.params == T.params and back.pack()[0].tolist() == T.pack()[0].tolist()
    for x, y in zip(back.pack_params(), T.pack_params()):
        assert np.array_equal(x, y) and x.dtype == y.dtype
    # pack() keeps its 6-tuple and from_csr its signature; to_list emits "params" only where there are some, as written
    assert len(T.pack()) == 6
    plain = ScenarioTable.from_csr(*T.pack(), CD)
    assert not plain.has_params and plain.params == [[], [], []] and all("params" not in s for s in plain.to_list())
    lst = T.to_list()
    assert "params" in lst[0] and "params" in lst[1] and "params" not in lst[2] and lst[0]["params"][0] == [5, 12, "kp", "*", "scale", 0.5]
    p = tmp_path / "t.yaml"
    p.write_text(yaml.safe_dump({"scenarios": lst}))
    again = ScenarioTable.build(str(p), CD)
    assert again.params is None and again.has_params               # names and "*" wait for a model ...
    with pytest.raises(ValueError, match="not resolved yet"):
        again.pack_params()
    assert again.resolve(NAMES).params == T.params                  # ... and resolve against it
    with pytest.raises(ValueError, match=r"parameter windows for 2 scenarios, the table has 3"):   # another S
        T.params_from_csr(adr[:3], t, field, index, op, value)


def test_sweep_counts_with_the_params_axis():
    from cosim_amd.scenario import ScenarioTable, sweep
    C = [[0.5, 0, 0, 0], [1.0, 0, 0, 0]]
    V, D, W = [0.3, 0.6], [0.0, np.pi], [(5, 8)]
    P = [[], [[10, 20, "kp", "*", "scale", 0.0]], [[0, 5, "geom_friction", "*", "scale", 0.3], [5, 9, "kd", 0, "set", 1.0]]]
    got = list(sweep(C, V, D, W, params=P))
    assert len(got) == len(C) * len(V) * len(D) * len(W) * len(P) == 24
    assert len(list(sweep(C, params=P))) == 6 and len(list(sweep(C, V, D, W))) == 8
    # innermost: consecutive scenarios share command and push and walk through P
    for k in range(0, 24, 3):
        assert got[k]["commands"] == got[k + 1]["commands"] == got[k + 2]["commands"] and got[k]["pushes"] == got[k + 2]["pushes"]
        assert "params" not in got[k] and got[k + 1]["params"] == P[1] and got[k + 2]["params"] == P[2]
    T = ScenarioTable(got, CD, names=NAMES)
    assert [len(p) for p in T.params[:3]] == [0, 4, 6] and T.n_param_items == 8 * 10


# ------------------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad, message", [
    ([{}, {"params": [[0, 5, "kp", 0, "scale", float("nan")]]}], r"scenario 1, parameter window 0: non-finite value"),
    ([{"params": [[0, 5, "kp", 0, "set", 1e39]]}], r"scenario 0, parameter window 0: non-finite value"),          # inf as float32
    ([{"params": [[0, 5, "kp", 0, "scale", 1.0], [7, 7, "kp", 0, "set", 1.0]]}], r"scenario 0, parameter window 1: t1 7 is not after t0 7"),
    ([{"params": [[9, 3, "kd", 0, "set", 1.0]]}], r"parameter window 0: t1 3 is not after t0 9"),
    ([{"params": [[-1, 3, "kd", 0, "set", 1.0]]}], r"parameter window 0: times must be control steps in \[0, 2\^30\)"),
    ([{"params": [[0, 2 ** 30 + 1, "kd", 0, "set", 1.0]]}], r"times must be control steps"),
    ([{"params": [[0.5, 3, "kd", 0, "set", 1.0]]}], r"times must be control steps"),
    ([{"params": [[0, 3, "gain", 0, "set", 1.0]]}], r"scenario 0, parameter window 0: unknown field 'gain'"),
    ([{"params": [[0, 3, "kp", 0, "add", 1.0]]}], r"unknown op 'add'"),
    ([{"params": [[0, 3, "kp", "elbow", "set", 1.0]]}], r"scenario 0, parameter window 0: unknown name 'elbow' for field 'kp'"),
    ([{"params": [[0, 3, "geom_friction", "hip_l", "set", 1.0]]}], r"unknown name 'hip_l' for field 'geom_friction'"),
    ([{}, {}, {"params": [[0, 3, "kp", 4, "set", 1.0]]}], r"scenario 2, parameter window 0: index 4 out of range: 'kp' has 4 entries"),
    ([{"params": [[0, 3, "dof_frictionloss", -1, "set", 1.0]]}], r"index -1 out of range: 'dof_frictionloss' has 8 entries"),
    ([{"params": [[0, 3, "kp", 1.0, "set", 1.0]]}], r"index must be an int, a name or '\*'"),
    ([{"params": [[0, 3, "kp", 0, "set"]]}], r"expected \[t0, t1, field, index, op, value\]"),
    ([{"params": [[k, k + 1, "dof_frictionloss", "*", "scale", 0.5] for k in range(33)]}], r"scenario 0: 264 parameter items after expansion, at most 256"),
    ([{"params": [[0, 3, "body_mass", 0, "scale", 1.5]]}], r"field 'body_mass' is refused: .* consistent only as a set .* fp64 .* out of scope"),
    ([{"params": [[0, 3, "body_invweight0", 0, "scale", 1.5]]}], r"'body_invweight0' is refused"),
    ([{"params": [[0, 3, "dof_invweight0", 0, "scale", 1.5]]}], r"'dof_invweight0' is refused"),
    ([{"params": [[0, 3, "meaninertia", 0, "set", 1.5]]}], r"'meaninertia' is refused"),
])
def test_validation_names_scenario_and_row(bad, message):
    """Refused while the table is built: no engine exists here."""
    from cosim_amd.scenario import ScenarioTable
    with pytest.raises(ValueError, match=message):
        ScenarioTable(bad, CD, names=NAMES)


def test_unresolved_windows_are_refused_by_the_twin_and_the_packer():
    from cosim_amd.scenario import ScenarioTable, reference_params
    T = ScenarioTable(TABLE3, CD)                                    # no names: times, fields and ops are checked, the rest waits
    assert T.params is None
    with pytest.raises(ValueError, match="not resolved yet"):
        reference_params(T, "env", [0], [0], [0], _base(1), _layout())
    with pytest.raises(ValueError, match=r"scenario 0, parameter window 0: unknown op 'halve'"):
        ScenarioTable([{"params": [[0, 1, "kp", "*", "halve", 1.0]]}], CD)
    with pytest.raises(ValueError, match=r"field 'kd' needs the model's names"):
        ScenarioTable([{"params": [[0, 1, "kd", "*", "set", 1.0]]}], CD).resolve({"kp": ["a"]})


def test_names_and_layout_of_a_compiled_model():
    """flamingo_light_v1: the names an index may use and the layout the twin is given are the engine's (param_stride 96)."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    from cosim_amd.scenario import ScenarioTable, param_layout, param_names
    cm = compile_model(make_config("flamingo_light_v1"))
    b = cm.blob
    names = param_names(cm)
    assert len(names["kp"]) == len(names["kd"]) == b.nu and len(names["geom_friction"]) == b.ngeom and len(names["dof_frictionloss"]) == b.nv
    lay = param_layout(b.nbody, b.nv, b.ngeom, b.nu)
    assert lay["stride"] == 96 and lay["kd"] + b.nu < 96 and lay["dof_frictionloss"] == 2 * b.nbody + b.nv
    free = names["dof_frictionloss"][0]
    T = ScenarioTable([{"params": [[0, 1, "dof_frictionloss", free, "scale", 2.0], [0, 1, "kp", names["kp"][-1], "set", 0.0]]}], CD, names=names)
    assert [it[3] for it in T.params[0]] == list(range(6)) + [b.nu - 1]


# ------------------------------------------------------------------------------------------------------------ the kernel's body, as host C++
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "scnparams_lanes.cpp")])
    return exe


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/scnparams_lanes.cpp + csrc/cosim_scnparams.h as a plain C++ program (no HIP, no GPU), and the same program built with
    AddressSanitizer and UBSan: a stand-alone executable with its own main, run as a child process."""
    tmp = tmp_path_factory.mktemp("scnpar")
    return _build(tmp, "scnparams_lanes", []), _build(tmp, "scnparams_lanes_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                                                   "-fno-omit-frame-pointer"])


def _run_lanes(exe, table, layout, mode, gid_off, lanes, env, ep, t, base):
    from cosim_amd.scenario import _FIELD_NAMES, MODES
    adr, tt, field, index, op, value = table.pack_params()
    word = [layout[_FIELD_NAMES[int(f)]] + int(i) for f, i in zip(field, index)]
    u = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    stride = base.shape[1]
    words = [len(table), MODES[mode], gid_off, len(word)] + adr.tolist() + tt.reshape(-1).tolist() + word + op.tolist() + u(value)
    words += [stride, lanes, len(env)]
    for i in range(len(env)):
        words += [int(env[i]), int(ep[i]), int(t[i])] + u(base[i])
    p = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = np.array([[int(x) for x in line.split()] for line in p.stdout.strip().splitlines()], dtype=np.int64)
    assert rows.shape == (len(env), 1 + stride)
    return rows[:, 0].astype(np.int32), rows[:, 1:].astype(np.uint32)


# a 200-word record (no multiple of 64: the word loop's last pass is a tail) with windows on its first and last fields
NAMES200 = {"dof_frictionloss": [f"j{k}" for k in range(30)], "geom_friction": [f"g{k}" for k in range(80)],
            "kp": [f"a{k}" for k in range(20)], "kd": [f"a{k}" for k in range(20)]}
LAYOUT200 = {"dof_frictionloss": 40, "geom_friction": 70, "kp": 150, "kd": 170, "stride": 200}
TABLE200 = [
    {"params": [[0, 4, "geom_friction", "*", "scale", 0.3], [2, 6, "geom_friction", "g79", "set", 0.01], [1, 3, "kd", "a19", "scale", 0.0],
                [1, 2, "dof_frictionloss", 0, "set", 0.5]]},
    {},
    {"params": [[3, 5, "kp", "*", "scale", 1.5], [3, 5, "kd", "*", "scale", 1.5], [4, 5, "kp", "a7", "set", 0.0]]},
]


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
@pytest.mark.parametrize("lanes", [64, 5, 1])
@pytest.mark.parametrize("record", [96, 200])
def test_kernel_body_as_host_cpp_equals_the_twin(lanes_exes, record, lanes, sanitized):
    """Every (env, episode, t) of a hand-written table through the functions the kernel calls, with 64 lanes (the wave), 5 and 1: the
    rows and every word of the effective record equal the twin's, compared as uint32; no word is left unwritten."""
    from cosim_amd.scenario import ScenarioTable, param_layout, scenario_rows
    if record == 96:                                                # flamingo_light_v1's sizes: 8 bodies, 12 dofs, 9 geoms... any that give 96
        lay = param_layout(nbody=8, nv=13, ngeom=14, nu=6)
        assert lay["stride"] == 96
        names = {"kp": NAMES["kp"] + ["a", "b"], "kd": NAMES["kd"] + ["a", "b"], "geom_friction": NAMES["geom_friction"] + [None] * 9,
                 "dof_frictionloss": NAMES["dof_frictionloss"] + ["x"] * 5}
        T = ScenarioTable(TABLE3, CD, names=names)
        ts = [0, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 19, 20, 21, 22, 29, 30]
    else:
        lay, T = LAYOUT200, ScenarioTable(TABLE200, CD, names=NAMES200)
        ts = [0, 1, 2, 3, 4, 5, 6]
    exe = lanes_exes[1 if sanitized else 0]
    rng = np.random.default_rng(record + lanes)
    for mode, gid_off in (("env", 0), ("cycle", 2)):
        env, ep, t = (x.reshape(-1) for x in np.meshgrid(np.arange(4), np.array([0, 1, 2, 7]), np.array(ts), indexing="ij"))
        base = rng.uniform(0.01, 40.0, size=(len(env), lay["stride"])).astype(f32)
        row, eff = _run_lanes(exe, T, lay, mode, gid_off, lanes, env, ep, t, base)
        assert np.array_equal(row, scenario_rows(3, mode, env + gid_off, ep))
        want = _eff(T, mode, env + gid_off, t, ep, base=base, layout=lay)
        assert np.array_equal(eff, want.view(np.uint32)), np.nonzero(eff != want.view(np.uint32))
        assert (eff != base.view(np.uint32)).any() and (eff == base.view(np.uint32)).all(axis=1).any()   # windows opened, and closed


# ------------------------------------------------------------------------------------------------------------ kernel resources, code size
def _table_file(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip() for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/scnparams_kres_parent.txt) and after (scnparams_kres_this.txt): every existing kernel's line is
    identical, in the same order; the one added line is scnparams_step_kernel's, which uses no LDS, no scratch and spills nothing."""
    head_a, a = _table_file("scnparams_kres_parent.txt")
    head_b, b = _table_file("scnparams_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["scnparams_step_kernel"], sorted(added)
    vgpr, agpr, sspill, vspill, scratch, occ, lds = added["scnparams_step_kernel"]
    assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 64 and occ == 8


def test_code_size_of_existing_kernels_is_unchanged():
    """tools/ksize.py --lib before and after: the same kernels with the same bytes, plus the new one."""
    head_a, a = _table_file("scnparams_ksize_parent.txt")
    head_b, b = _table_file("scnparams_ksize_this.txt")
    assert head_a == head_b and len(a) >= 40
    new = [ln for ln in b if "scnparams_step_kernel" in ln]
    assert len(new) == 1 and [ln for ln in b if ln not in new] == a
