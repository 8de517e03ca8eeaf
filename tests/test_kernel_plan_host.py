"""Which kernel runs when, on the host (no GPU): csrc/cosim_plan.h compiled as plain C++ with int ids for launchers
(tests/kernel_plan.cpp) and driven over five synthetic kernel sets -- every switch alone, every ordered pair, the refusals and the
sequences the GPU test (test_gpu_kernel_plan.py) runs -- against the rules of ``cosim_set_param`` written out here."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MEMBERS = ("fleet", "fleet_step", "fleet_prof", "epw2", "epw2_prof", "ct", "ct_prof", "fix", "roll", "roll_step", "roll_fix", "hfix", "stepfix",
           "dbg_hfix", "narrow0", "narrow1", "narrow2", "narrow3", "solver")
ID = {m: i + 1 for i, m in enumerate(MEMBERS)}                 # launcher ids; 0: the set has no such kernel


def _caps(m):
    """(lds_bytes, contact_slots, pair_slots, geom_stage) of member m: every number names its member and field."""
    return 1000 + ID[m], 100 + ID[m], 200 + ID[m], 300 + ID[m]


SETS = {
    # dense plane with everything (like flamingo_light_v1)
    "dense_all": ("fleet", "fleet_step", "fleet_prof", "epw2", "epw2_prof", "ct", "ct_prof", "fix", "roll", "roll_step", "roll_fix"),
    # dense plane without a two-per-wave or step-only kernel (like flamingo_p_v3)
    "dense_p": ("fleet", "fleet_prof", "ct", "ct_prof", "fix", "roll", "roll_fix"),
    # bare (like w4_p_v2 on the plane)
    "bare": ("fleet",),
    # fused heightfield kernel with a fix-up (like flamingo_light_v1 on a heightfield)
    "fused_hf": ("fleet", "hfix", "dbg_hfix"),
    # split heightfield pipeline with both fix-ups (like humanoid_p_v0 on a heightfield)
    "split_hf": ("fleet", "fleet_prof", "narrow0", "narrow1", "narrow2", "narrow3", "solver", "hfix", "stepfix"),
}
ACTIONS = [("contact_twist", 0), ("contact_twist", 1), ("fixup", 0), ("fixup", 1), ("hfield_fixup", 0), ("hfield_fixup", 1), ("hfield_fixup", 2),
           ("split", 0), ("split", 1), ("step_kernel", 0), ("step_kernel", 1), ("step_kernel", 2), ("envs_per_wave", 1), ("envs_per_wave", 2),
           ("envs_per_wave", 3), ("narrow_occupancy", 0), ("narrow_occupancy", 1), ("narrow_occupancy", 2), ("narrow_occupancy", 3),
           ("narrow_occupancy", 4), ("narrow_occupancy", 5)]
MSG = {
    "ct": "cosim_set_param: no contact-twist variant for this model / terrain",
    "hfix01": "cosim_set_param: hfield_fixup must be 0 or 1",
    "hfix": "cosim_set_param: no heightfield fix-up for this model / terrain / kernel variant",
    "split": "cosim_set_param: no split pipeline for this model / terrain",
    "sk01": "cosim_set_param: step_kernel must be 0 or 1",
    "epw": "cosim_set_param: envs_per_wave not available for this model / env count",
}


class Rules:
    """The rules of the kernel switches, as the issue and DESIGN 4.17 state them, over one set (`have`: its members)."""

    def __init__(self, have, n_envs):
        self.have, self.n = set(have), n_envs
        self.twist = self.nofix = self.hfield = False              # "contact_twist" 1 and "fixup" 0 are one-way
        self.split = "solver" in self.have                         # the split pipeline is the default where there is one
        self.step_kernel, self.epw, self.occ = True, 1, 2

    def call(self, which, v):
        """-> the refusal message, or None."""
        h = self.have
        if which == "contact_twist":
            if v == 0:
                return None                                        # 0 is a no-op, even after 1
            if "ct" not in h:
                return MSG["ct"]
            self.twist, self.epw = True, 1                         # epw is forced to 1
        elif which == "fixup":
            if v == 0:                                             # non-zero is a no-op
                self.nofix, self.hfield = True, False
        elif which == "hfield_fixup":
            if v not in (0, 1):
                return MSG["hfix01"]
            if "hfix" not in h or self.nofix or self.epw != 1:     # after "fixup" 0 either value is refused
                return MSG["hfix"]
            self.hfield = bool(v)
        elif which == "split":
            if v and "solver" not in h:
                return MSG["split"]
            self.split = bool(v)
        elif which == "step_kernel":
            if v not in (0, 1):
                return MSG["sk01"]
            self.step_kernel = bool(v)
        elif which == "envs_per_wave":
            if v != 1 and not (v == 2 and "epw2" in h and not self.twist and self.n % 2 == 0):
                return MSG["epw"]
            self.epw = v
        elif which == "narrow_occupancy":
            self.occ = v
        return None

    def row(self, refused):
        h = self.have

        def k(m):
            return ID[m] if m in h else 0

        fleet = "ct" if self.twist else "fleet"
        general = fleet if self.epw == 1 else "epw2"
        split = self.split and "solver" in h
        step_kernel = self.step_kernel and self.epw == 1 and not self.twist and "fleet_step" in h
        reset = "solver" if split else general                     # reset always runs a general instantiation
        step = "solver" if split else ("fleet_step" if step_kernel else general)
        narrow = ("narrow3" if self.occ >= 4 else "narrow2" if self.occ == 3 else "narrow1" if self.occ == 2 else "narrow0") if split else None
        if split:
            fix = "stepfix" if self.hfield else None
        elif self.hfield:
            fix = "hfix"
        else:
            fix = None if (self.twist or self.nofix) else "fix"
        fix = fix if fix in h else None
        launched_fix = fix if self.epw == 1 else None              # under two envs per wave no fix-up is launched ...
        rollout = self.epw == 1 and not self.twist and "roll" in h and not (self.nofix and "roll_fix" in h)
        roll = ("roll_step" if self.step_kernel and "roll_step" in h else "roll") if rollout else None
        prof = "ct_prof" if self.twist else ("fleet_prof" if self.epw == 1 else "epw2_prof")
        debug = "solver" if split else ("dbg_hfix" if self.hfield and "dbg_hfix" in h else general)
        lds, slots, pairs, _ = _caps(fleet)                        # ... and the capacities stay the one-per-wave kernel's
        ids = [k(reset), k(narrow) if narrow else 0, k(step), k(launched_fix) if launched_fix else 0, k(roll) if roll else 0,
               k("roll_fix") if rollout else 0, k(prof), k(debug)]
        answers = [int(split and self.occ == 0), lds, slots, pairs, _caps(fix)[1] if fix else 0, int(step_kernel), int(split)]
        return [int(refused is not None), self.epw], ids, answers, refused or ""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kernel_plan") / "kernel_plan")
    cxx = os.environ.get("CXX", "c++")
    p = subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "kernel_plan.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _drive(exe, runs):
    """runs: [(set name, n_envs, [(switch, value), ...])] -> per run, the parsed rows of tests/kernel_plan.cpp."""
    lines = []
    for name, have in SETS.items():
        words = []
        for m in MEMBERS:
            words += [ID[m] if m in have else 0, *(_caps(m) if m in have else (0, 0, 0, 64))]
        lines.append(f"SET {name} " + " ".join(map(str, words)))
    for name, n, calls in runs:
        lines.append(f"RUN {name} {n} " + " ".join(f"{w} {v}" for w, v in calls))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = iter(p.stdout.splitlines())
    res = []
    for _, _, calls in runs:
        rows = []
        for _ in range(len(calls) + 1):
            a, b, c, msg = next(out).split(" | ")
            rows.append(([int(x) for x in a.split()], [int(x) for x in b.split()], [int(x) for x in c.split()], msg.strip()))
        res.append(rows)
    assert next(out, None) is None
    return res


def _expected(name, n, calls):
    r = Rules(SETS[name], n)
    rows = [r.row(None)]
    for which, v in calls:
        rows.append(r.row(r.call(which, v)))
    return [(a, b, c, m) for a, b, c, m in rows]


def _check(exe, runs):
    for (name, n, calls), got in zip(runs, _drive(exe, runs)):
        want = _expected(name, n, calls)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == tuple(w), f"{name}, {n} envs, after {calls[:i]}: got {g}, want {tuple(w)}"


def test_every_switch_alone_and_every_ordered_pair(plan_exe):
    runs = []
    for name in SETS:
        runs += [(name, 4, [a]) for a in ACTIONS]
        runs += [(name, 4, [a, b]) for a, b in itertools.product(ACTIONS, ACTIONS)]
    _check(plan_exe, runs)


def test_sequences_of_the_gpu_test_and_the_odd_env_count(plan_exe):
    seqs = [[("contact_twist", 1), ("contact_twist", 0), ("envs_per_wave", 2)],
            [("fixup", 0), ("fixup", 1), ("hfield_fixup", 1)],
            [("fixup", 0), ("hfield_fixup", 0)],
            [("hfield_fixup", 1), ("hfield_fixup", 0)],
            [("envs_per_wave", 2), ("envs_per_wave", 1)],
            [("hfield_fixup", 1), ("split", 0), ("split", 1)],
            [("step_kernel", 0), ("step_kernel", 1)],
            [("envs_per_wave", 2), ("contact_twist", 1), ("envs_per_wave", 2), ("step_kernel", 1)],
            [("envs_per_wave", 2), ("hfield_fixup", 1), ("fixup", 0), ("envs_per_wave", 1)],
            [("hfield_fixup", 1), ("fixup", 0), ("split", 0), ("hfield_fixup", 1)]]
    _check(plan_exe, [(name, n, s) for name in SETS for n in (4, 3) for s in seqs])


def test_rows_written_out_by_hand(plan_exe):
    """A few rows as literals, so that the rules above are not the only statement of them."""
    I = ID
    runs = [("dense_all", 4, [("envs_per_wave", 2), ("contact_twist", 1), ("fixup", 0)]),
            ("dense_all", 3, [("envs_per_wave", 2)]),
            ("dense_p", 4, [("fixup", 0), ("envs_per_wave", 2)]),
            ("bare", 4, [("split", 1), ("contact_twist", 1), ("hfield_fixup", 1)]),
            ("fused_hf", 4, [("hfield_fixup", 1), ("fixup", 0), ("hfield_fixup", 0)]),
            ("split_hf", 4, [("hfield_fixup", 1), ("narrow_occupancy", 0), ("split", 0)])]
    got = _drive(plan_exe, runs)
    f, c = I["fleet"], I["ct"]
    assert got[0] == [
        # fresh: the step-only kernels step and roll, the plane fix-up stands behind them
        ([0, 1], [f, 0, I["fleet_step"], I["fix"], I["roll_step"], I["roll_fix"], I["fleet_prof"], f], [0, 1000 + f, 100 + f, 200 + f, 100 + I["fix"], 1, 0], ""),
        # two envs per wave: no fix-up launched, no rollout, no step kernel; the answers stay the one-per-wave kernel's
        ([0, 2], [I["epw2"], 0, I["epw2"], 0, 0, 0, I["epw2_prof"], I["epw2"]], [0, 1000 + f, 100 + f, 200 + f, 100 + I["fix"], 0, 0], ""),
        # contact twist: one env per wave again, everything is the contact-twist kernel, nothing behind it
        ([0, 1], [c, 0, c, 0, 0, 0, I["ct_prof"], c], [0, 1000 + c, 100 + c, 200 + c, 0, 0, 0], ""),
        ([0, 1], [c, 0, c, 0, 0, 0, I["ct_prof"], c], [0, 1000 + c, 100 + c, 200 + c, 0, 0, 0], "")]
    assert got[1][1] == ([1, 1], got[1][0][1], got[1][0][2], MSG["epw"])
    assert got[2][1] == ([0, 1], [f, 0, f, 0, 0, 0, I["fleet_prof"], f], [0, 1000 + f, 100 + f, 200 + f, 0, 0, 0], "")
    assert got[2][2] == ([1, 1], got[2][1][1], got[2][1][2], MSG["epw"])
    bare = ([f, 0, f, 0, 0, 0, 0, f], [0, 1000 + f, 100 + f, 200 + f, 0, 0, 0])
    assert got[3] == [([0, 1], *bare, ""), ([1, 1], *bare, MSG["split"]), ([1, 1], *bare, MSG["ct"]), ([1, 1], *bare, MSG["hfix"])]
    assert got[4] == [([0, 1], [f, 0, f, 0, 0, 0, 0, f], [0, 1000 + f, 100 + f, 200 + f, 0, 0, 0], ""),
                      ([0, 1], [f, 0, f, I["hfix"], 0, 0, 0, I["dbg_hfix"]], [0, 1000 + f, 100 + f, 200 + f, 100 + I["hfix"], 0, 0], ""),
                      ([0, 1], [f, 0, f, 0, 0, 0, 0, f], [0, 1000 + f, 100 + f, 200 + f, 0, 0, 0], ""),
                      ([1, 1], [f, 0, f, 0, 0, 0, 0, f], [0, 1000 + f, 100 + f, 200 + f, 0, 0, 0], MSG["hfix"])]
    s, p = I["solver"], I["fleet_prof"]
    assert got[5] == [([0, 1], [s, I["narrow1"], s, 0, 0, 0, p, s], [0, 1000 + f, 100 + f, 200 + f, 0, 0, 1], ""),
                      ([0, 1], [s, I["narrow1"], s, I["stepfix"], 0, 0, p, s], [0, 1000 + f, 100 + f, 200 + f, 100 + I["stepfix"], 0, 1], ""),
                      ([0, 1], [s, I["narrow0"], s, I["stepfix"], 0, 0, p, s], [1, 1000 + f, 100 + f, 200 + f, 100 + I["stepfix"], 0, 1], ""),
                      ([0, 1], [f, 0, f, I["hfix"], 0, 0, p, f], [0, 1000 + f, 100 + f, 200 + f, 100 + I["hfix"], 0, 0], "")]


def test_more_rows_written_out_by_hand(plan_exe):
    """The one-way "fixup" 0 on the split set, "step_kernel" 0 on the dense plane and its rollout, the plane without step-only kernels,
    and the four narrowphase builds, as literals."""
    I = ID
    f, s, p = I["fleet"], I["solver"], I["fleet_prof"]
    runs = [("split_hf", 4, [("fixup", 0), ("hfield_fixup", 1), ("hfield_fixup", 0), ("fixup", 1), ("split", 0), ("hfield_fixup", 1)]),
            ("dense_all", 4, [("step_kernel", 0), ("fixup", 0), ("step_kernel", 1), ("step_kernel", 2)]),
            ("dense_p", 4, [("step_kernel", 0), ("contact_twist", 0)]),
            ("split_hf", 4, [("narrow_occupancy", 3), ("narrow_occupancy", 7), ("narrow_occupancy", 1), ("narrow_occupancy", -1)])]
    got = _drive(plan_exe, runs)
    caps = [1000 + f, 100 + f, 200 + f]
    split = ([s, I["narrow1"], s, 0, 0, 0, p, s], [0, *caps, 0, 0, 1])
    fused = ([f, 0, f, 0, 0, 0, p, f], [0, *caps, 0, 0, 0])
    # after "fixup" 0 the heightfield fix-up is refused, either value, split or fused; "fixup" 1 brings nothing back
    assert got[0] == [([0, 1], *split, ""), ([0, 1], *split, ""), ([1, 1], *split, MSG["hfix"]), ([1, 1], *split, MSG["hfix"]),
                      ([0, 1], *split, ""), ([0, 1], *fused, ""), ([1, 1], *fused, MSG["hfix"])]
    # "step_kernel" 0: steps and rollouts on the general kernels, the fix-ups stay; "fixup" 0 takes the plane fix-up and the whole rollout
    # (it needs roll_fix) but not the step-only kernel, which "step_kernel" 1 brings back; 2 is refused
    fix, rfix, fp = I["fix"], I["roll_fix"], I["fleet_prof"]
    assert got[1] == [([0, 1], [f, 0, I["fleet_step"], fix, I["roll_step"], rfix, fp, f], [0, *caps, 100 + fix, 1, 0], ""),
                      ([0, 1], [f, 0, f, fix, I["roll"], rfix, fp, f], [0, *caps, 100 + fix, 0, 0], ""),
                      ([0, 1], [f, 0, f, 0, 0, 0, fp, f], [0, *caps, 0, 0, 0], ""),
                      ([0, 1], [f, 0, I["fleet_step"], 0, 0, 0, fp, f], [0, *caps, 0, 1, 0], ""),
                      ([1, 1], [f, 0, I["fleet_step"], 0, 0, 0, fp, f], [0, *caps, 0, 1, 0], MSG["sk01"])]
    # no step-only kernels: "step_kernel" changes nothing and answers 0; "contact_twist" 0 is a no-op
    plain = ([f, 0, f, fix, I["roll"], rfix, fp, f], [0, *caps, 100 + fix, 0, 0])
    assert got[2] == [([0, 1], *plain, ""), ([0, 1], *plain, ""), ([0, 1], *plain, "")]
    # narrowphase builds: 3 -> narrow2, 4 and more -> narrow3, anything else the diagnostic build, which counts only at 0
    def nar(n, diag=0):
        return ([0, 1], [s, I[n], s, 0, 0, 0, p, s], [diag, *caps, 0, 0, 1], "")
    assert got[3] == [nar("narrow1"), nar("narrow2"), nar("narrow3"), nar("narrow0"), nar("narrow0")]
