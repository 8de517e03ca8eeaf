"""Scenario tables on the host (no GPU): the numpy twin of the scenario kernel against hand-written expectations, CSR packing, the
sweep generator, validation messages, the kernel's per-env body compiled as plain C++ and driven lane by lane against the twin, the
ledger twin with per-step commands and scenario rows, and the kernel-resource tables recorded before and after the change."""
import os
import re
import subprocess

import numpy as np
import pytest

from scenario_cases import BASE, CD, NEVER, TABLE5, table5

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _sched(table, mode, gid, t, ep, base=BASE):
    from cosim_amd.scenario import reference_schedule
    gid = np.atleast_1d(gid)
    return reference_schedule(table, mode, gid, np.broadcast_to(t, gid.shape), np.broadcast_to(ep, gid.shape), np.tile(base, (len(gid), 1)))


# ------------------------------------------------------------------------------------------------------------ the twin, by hand
def test_twin_against_hand_written_table():
    T = table5()
    assert len(T) == 5 and T.has_push
    f = np.float32

    def one(gid, t, ep=0, mode="env"):
        row, cmd, mask, v = _sched(T, mode, [gid], t, ep)
        return int(row[0]), cmd[0].tolist(), bool(mask[0]), v[0].tolist()

    # 0: an empty scenario -- the caller's command, never a push
    for t in (0, 7, 24, 1000):
        assert one(0, t) == (0, BASE.tolist(), False, [0.0, 0.0, 0.0])
    # 1: the caller's command passes through before the first keyframe at t = 3
    assert one(1, 0)[1] == BASE.tolist() and one(1, 2)[1] == BASE.tolist()
    assert one(1, 3)[1] == [1.0, 0.0, 0.0, 0.0] and one(1, 9)[1] == [1.0, 0.0, 0.0, 0.0]
    assert one(1, 10)[1] == [f(0.2), 0.0, f(0.3), 0.0] and one(1, 24)[1] == [f(0.2), 0.0, f(0.3), 0.0]
    # 2: keyframes at 24 and 25: under the time limit the pre-step clock stops at 24
    assert one(2, 0)[1] == [f(0.4), 0.0, 0.0, 0.0] and one(2, 23)[1] == [f(0.4), 0.0, 0.0, 0.0]
    assert one(2, 24)[1] == [f(0.8), 0.0, 0.0, 0.0]
    assert all(one(2, t)[1] != NEVER for t in range(25)) and one(2, 25)[1] == NEVER
    # 3: overlapping windows -- the last LISTED one that holds wins
    assert one(3, 4)[2] is False and one(3, 12)[2] is False
    for t in (5, 6, 7, 10, 11):
        assert one(3, t)[2:] == (True, [0.5, 0.0, 0.0])
    for t in (8, 9):
        assert one(3, t)[2:] == (True, [0.0, f(0.4), f(0.1)])
    assert one(3, 8)[1] == [f(0.3), f(0.1), 0.0, 0.0]
    # 4: a window across the time limit: held in 22 .. 24, and (t = 0 after the auto-reset) not after it
    assert [one(4, t)[2] for t in (21, 22, 23, 24, 0, 1)] == [False, True, True, True, False, False]
    assert one(4, 22)[3] == [f(-0.3), f(0.2), 0.0] and one(4, 22)[1] == BASE.tolist()
    # rows: gid mod S, negative ids included
    row = _sched(T, "env", np.array([0, 4, 5, 96, -1, -5]), 0, 0)[0]
    assert row.tolist() == [0, 4, 0, 1, 4, 0]


def test_twin_cycle_walks_through_the_scenarios():
    T = table5()
    gid = np.arange(12)
    for ep in range(8):                                            # several episodes: every env has seen every scenario after five
        row = _sched(T, "cycle", gid, 0, ep)[0]
        assert row.tolist() == [(g + ep) % 5 for g in gid]
    assert _sched(T, "env", gid, 0, 3)[0].tolist() == [g % 5 for g in gid]   # mode env ignores the episode count
    # ep is taken as uint32: a meta word that reads negative still lands inside the table, by the same formula
    row = _sched(T, "cycle", np.array([3]), 0, np.array([-1]))[0]
    assert row.tolist() == [(3 + (2 ** 32 - 1) % 5) % 5]
    # the command follows the row of the episode
    assert _sched(T, "cycle", [0], 24, 2)[1][0].tolist() == [np.float32(0.8), 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------------------ packing, building
def test_csr_round_trip(tmp_path):
    import yaml
    from cosim_amd.scenario import ScenarioTable
    T = table5()
    key_adr, key_t, key_cmd, push_adr, push_t, push_v = T.pack()
    assert key_adr.tolist() == [0, 0, 2, 5, 6, 6] and push_adr.tolist() == [0, 0, 0, 0, 2, 3]
    assert key_t.tolist() == [3, 10, 0, 24, 25, 0] and key_cmd.shape == (6, CD) and key_cmd.dtype == np.float32
    assert push_t.tolist() == [[5, 12], [8, 10], [22, 30]] and push_v.shape == (3, 3)
    assert all(a.dtype == np.int32 for a in (key_adr, key_t, push_adr, push_t))
    back = ScenarioTable.from_csr(*T.pack(), CD)
    assert back.to_list() == T.to_list()
    for a, b in zip(back.pack(), T.pack()):
        np.testing.assert_array_equal(a, b)
    # from a mapping, from a YAML file, from itself
    path = tmp_path / "scn.yaml"
    path.write_text(yaml.safe_dump({"scenarios": T.to_list()}))
    for spec in ({"scenarios": TABLE5}, str(path), T, TABLE5):
        assert ScenarioTable.build(spec, CD).to_list() == T.to_list()
    empty = ScenarioTable([{}], 0).pack()                          # no command at all: still a table
    assert [a.shape for a in empty] == [(2,), (0,), (0, 0), (2,), (0, 2), (0, 3)]


def test_sweep_counts():
    from cosim_amd.scenario import ScenarioTable, sweep
    C = [[0.5, 0, 0, 0], [1.0, 0, 0, 0], [0.0, 0, 0.5, 0]]
    V, D, W = [0.3, 0.6], [0.0, np.pi / 2, np.pi, -np.pi / 2], [(5, 8), (15, 18)]
    full = list(sweep(C, V, D, W))
    assert len(full) == len(C) * len(V) * len(D) * len(W) == 48
    assert len(list(sweep(C))) == 3 and len(list(sweep(C, V, D, ()))) == 3 and len(list(sweep(C, (), D, W))) == 3
    T = ScenarioTable(full, CD)
    assert len(T) == 48 and all(len(k) == 1 and len(p) == 1 for k, p in zip(T.keys, T.pushes))
    assert full[0] == {"commands": [[0, 0.5, 0.0, 0.0, 0.0]], "pushes": [[5, 8, 0.3, 0.0, 0.0]]}
    # commands outermost, then speeds, directions, times; a direction of pi / 2 pushes along +y
    s = full[1 * 16 + 1 * 8 + 1 * 2 + 1]
    assert s["commands"] == [[0, 1.0, 0.0, 0.0, 0.0]] and s["pushes"][0][:2] == [15, 18]
    np.testing.assert_allclose(s["pushes"][0][2:], [0.0, 0.6, 0.0], atol=1e-15)


@pytest.mark.parametrize("bad, message", [
    ([{}, {"commands": [[0, 1, 0, 0, 0], [5, 1, 0, float("nan"), 0]]}], r"scenario 1, keyframe 1: non-finite"),
    ([{"pushes": [[0, 4, 1, 0, 0]]}, {}, {"pushes": [[1, 2, 0, 0, 0], [3, 4, 0, float("inf"), 0]]}], r"scenario 2, push window 1: non-finite"),
    ([{"commands": [[4, 1, 0, 0, 0], [4, 2, 0, 0, 0]]}], r"scenario 0, keyframe 1: time 4 does not increase \(previous 4\)"),
    ([{}, {}, {}, {"commands": [[0, 1, 0, 0, 0], [7, 1, 0, 0, 0], [6, 1, 0, 0, 0]]}], r"scenario 3, keyframe 2: time 6 does not increase"),
    ([{"pushes": [[5, 5, 1, 0, 0]]}], r"scenario 0, push window 0: t1 5 is not after t0 5"),
    ([{}, {"pushes": [[1, 2, 1, 0, 0], [9, 3, 1, 0, 0]]}], r"scenario 1, push window 1: t1 3 is not after t0 9"),
    ([{"commands": [[k, 1, 0, 0, 0] for k in range(65)]}], r"scenario 0: 65 keyframes, at most 64"),
    ([{}, {"pushes": [[k, k + 1, 1, 0, 0] for k in range(65)]}], r"scenario 1: 65 push windows, at most 64"),
    ([{"commands": [[0, 1, 0, 0]]}], r"scenario 0, keyframe 0: 4 values"),
    ([{"commands": [[-1, 1, 0, 0, 0]]}], r"scenario 0, keyframe 0: time -1.0 must be a control step"),
    ([{"commands": [[2 ** 30, 1, 0, 0, 0]]}], r"scenario 0, keyframe 0: time"),
    ([{"pushes": [[0.5, 2, 1, 0, 0]]}], r"scenario 0, push window 0: times"),
    ([], r"0 scenarios: must be 1\.\.65536"),
    ([{}] * 65537, r"65537 scenarios: must be 1\.\.65536"),
])
def test_validation_names_scenario_and_row(bad, message):
    from cosim_amd.scenario import ScenarioTable
    with pytest.raises(ValueError, match=message):
        ScenarioTable(bad, CD)


# ------------------------------------------------------------------------------------------------------------ the kernel's body, as host C++
@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    """tests/scenario_lanes.cpp + csrc/cosim_scenario.h as a plain C++ program (no HIP, no GPU)."""
    exe = str(tmp_path_factory.mktemp("scn") / "scenario_lanes")
    cxx = os.environ.get("CXX", "c++")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "scenario_lanes.cpp")])
    return exe


def _run_lanes(exe, table, mode, gid_off, env, ep, t, cmd_in, quat):
    from cosim_amd.scenario import MODES
    key_adr, key_t, key_cmd, push_adr, push_t, push_v = table.pack()
    u = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    words = [len(table), MODES[mode], table.command_dim, gid_off, len(key_t), len(push_t)]
    words += key_adr.tolist() + key_t.tolist() + u(key_cmd) + push_adr.tolist() + push_t.reshape(-1).tolist() + u(push_v) + [len(env)]
    for i in range(len(env)):
        words += [int(env[i]), int(ep[i]), int(t[i])] + u(cmd_in[i]) + u(quat[i])
    out = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True, check=True).stdout
    rows = np.array([[int(x) for x in line.split()] for line in out.strip().splitlines()], dtype=np.int64)
    assert rows.shape == (len(env), 2 + table.command_dim + 3)
    cd = table.command_dim
    return (rows[:, 0].astype(np.int32), rows[:, 1].astype(bool), rows[:, 2:2 + cd].astype(np.uint32).view(np.float32),
            rows[:, 2 + cd:].astype(np.uint32).view(np.float32))


@pytest.mark.parametrize("mode", ["env", "cycle"])
def test_kernel_body_as_host_cpp_equals_the_twin(lanes_exe, mode):
    """Every (env, episode, t) of the hand-written table through the function the kernel calls: rows and commands equal the twin's
    exactly; the push equals push_reference to 1e-6 relative (the host compiler's contraction is not the GPU's: the device bits are
    pinned by tests/test_gpu_scenario.py)."""
    from cosim_amd.scenario import push_reference, reference_schedule
    T = table5()
    rng = np.random.default_rng(5)
    env_id0 = 37                                                   # a shard's first global id: gid_off = 37 mod 5
    env, ep, t = (x.reshape(-1) for x in np.meshgrid(np.arange(11), np.array([0, 1, 2, 3, 7, -1]), np.arange(0, 32), indexing="ij"))
    n = len(env)
    cmd_in = rng.uniform(-1, 1, size=(n, CD)).astype(np.float32)
    quat = rng.normal(size=(n, 4)).astype(np.float32)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True).astype(np.float32)
    row, pushed, cmd, qvel = _run_lanes(lanes_exe, T, mode, env_id0 % 5, env, ep, t, cmd_in, quat)
    r_row, r_cmd, r_mask, r_v = reference_schedule(T, mode, env_id0 + env, t, ep, cmd_in)
    np.testing.assert_array_equal(row, r_row)
    np.testing.assert_array_equal(cmd.view(np.uint32), r_cmd.view(np.uint32))
    np.testing.assert_array_equal(pushed, r_mask)
    assert r_mask.sum() > 50 and (~r_mask).sum() > 50 and len(set(row.tolist())) == 5
    want = push_reference(quat[r_mask], r_v[r_mask])
    got = qvel[r_mask].astype(np.float64)
    scale = np.linalg.norm(r_v[r_mask].astype(np.float64), axis=1, keepdims=True)
    assert (np.abs(got - want) <= 1e-6 * scale).all(), float(np.abs((got - want) / scale).max())
    assert (qvel[~r_mask] == 0).all()                              # no window due: qvel untouched


def test_kernel_body_without_commands(lanes_exe):
    """command_dim 0: only pushes."""
    from cosim_amd.scenario import ScenarioTable
    T = ScenarioTable([{"pushes": [[1, 3, 0.0, 0.0, 0.25]]}, {}], 0)
    quat = np.tile(np.array([1, 0, 0, 0], dtype=np.float32), (4, 1))
    row, pushed, cmd, qvel = _run_lanes(lanes_exe, T, "env", 0, [0, 0, 1, 2], [0] * 4, [0, 1, 1, 2], np.zeros((4, 0), dtype=np.float32), quat)
    assert row.tolist() == [0, 0, 1, 0] and pushed.tolist() == [False, True, False, True] and cmd.shape == (4, 0)
    assert qvel[1].tolist() == [0.0, 0.0, 0.25] and qvel[3].tolist() == [0.0, 0.0, 0.25]


# ------------------------------------------------------------------------------------------------------------ ledger twin
def test_reference_ledger_with_per_step_commands_and_scenario_rows():
    from cosim_amd.ledger import reference_ledger
    K, N, nu, cd = 9, 3, 2, CD
    rng = np.random.default_rng(2)
    info = rng.uniform(-1, 1, size=(K, N, 4 + 2 * nu)).astype(np.float32)
    cmds = rng.uniform(-1, 1, size=(K, N, cd)).astype(np.float32)
    te, tr = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    tr[2, 0] = tr[5, 0] = tr[8, 0] = 1                             # env 0: three episodes of 3 steps
    te[3, 1] = 1                                                   # env 1: one of 4 steps, then open
    rows = np.zeros((K, N), dtype=np.int32)
    rows[:, 0] = np.repeat([0, 1, 2], 3)                           # env 0 cycles 0, 1, 2
    rows[:, 1] = np.where(np.arange(K) <= 3, 4, 0)
    rows[:, 2] = 3
    led = reference_ledger(info, te, tr, cmds, None, None, 4, nu, cd, scenario_rows=rows, include_open=True,
                           open_scenario_rows=np.array([0, 0, 3]))
    ended = led.ended()
    assert led.env.tolist() == [0, 0, 0, 0, 1, 1, 2] and ended.tolist() == [True, True, True, False, True, False, False]
    assert led.scenario.tolist() == [0, 1, 2, 0, 4, 0, 3] and led.words[:, 13].tolist() == [1, 2, 3, 1, 5, 1, 4]
    # tracking means are against the per-step command: env 0, episode 1 = steps 3 .. 5
    want = np.float32(sum(np.float64(np.abs(cmds[k, 0, 0] - info[k, 0, 1])) for k in (3, 4, 5)) / 3.0)
    assert led.mean_tracking_err_0[1] == want
    assert led.peak_tracking_err_0[1] == max(np.abs(cmds[k, 0, 0] - info[k, 0, 1]) for k in (3, 4, 5))
    # the old 2-D call: word 13 stays 0, scenario -1
    old = reference_ledger(info, te, tr, cmds[0], None, None, 4, nu, cd)
    assert (old.words[:, 13] == 0).all() and (old.scenario == -1).all() and len(old) == 4
    # by_scenario: counts, shares, lengths, means
    by = led.by_scenario()
    assert sorted(by) == [0, 1, 2, 4] and sum(v["episodes"] for v in by.values()) == int(ended.sum()) == 4
    assert by[4] == {"episodes": 1, "terminated": 1, "terminated_share": 1.0, "length": {"mean": 4.0, "min": 4, "p50": 4.0, "max": 4},
                     "means": {name: float(getattr(led, name)[4]) for name in by[4]["means"]}}
    assert by[1]["terminated_share"] == 0.0 and by[1]["length"]["mean"] == 3.0
    assert by[1]["means"]["mean_tracking_err_0"] == float(want)
    assert old.by_scenario()[-1]["episodes"] == 4


# ------------------------------------------------------------------------------------------------------------ kernel resources
def _kres(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip() for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/scenario_kres_parent.txt) and after (scenario_kres_this.txt): every existing kernel's line is
    identical, in the same order; the only added lines are the new kernels' -- the scenario kernel and the ledger's two table
    variants (the no-table ledger kernels are the code they were) -- which use no LDS, no scratch and spill nothing."""
    head_a, a = _kres("scenario_kres_parent.txt")
    head_b, b = _kres("scenario_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["ledger_open_scn_kernel", "ledger_step_scn_kernel", "scenario_step_kernel"], sorted(added)
    for name, (vgpr, agpr, sspill, vspill, scratch, occ, lds) in added.items():
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 96 and occ >= 5, (name, vgpr, occ)
    assert added["scenario_step_kernel"][0] <= 64 and added["scenario_step_kernel"][5] == 8
