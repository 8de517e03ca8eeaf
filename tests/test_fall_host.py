"""Fall rules, host side (cosim_amd/fall.py, cosim_amd/ledger.py): the numpy twin of the kernel's posture rules on hand-written
quaternions and a hand-built heightfield, FallRule's validation, the ledger twin with a cause array and the arithmetic of the
``fell`` counts, and the kernel resources before / after the rule went into ``env_body``.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from cosim_amd.fall import (CONTACT, HEIGHT, TILT, FallRule, Terrain, base_height, min_up, reference_fall, terrain_height,
                            up_component)
from cosim_amd.ledger import (FELL, FELL_CONTACT, FELL_HEIGHT, FELL_TILT, INT_FIELDS, NO_RESET, OPEN, TERMINATED, TRUNCATED,
                              EpisodeLedger, reference_ledger, same_records)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * a])


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _rot(axis, angle):
    """Rodrigues' formula: a rotation matrix built without any quaternion."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _qpos(quats, z=0.5, xy=(0.0, 0.0), nq=12):
    q = np.zeros((len(quats), nq), dtype=np.float32)
    q[:, 0], q[:, 1], q[:, 2] = xy[0], xy[1], z
    q[:, 3:7] = np.asarray(quats, dtype=np.float32)
    return q


# ------------------------------------------------------------------------------------------------------------ tilt
def test_up_component_on_hand_written_quaternions():
    s = math.sqrt(0.5)
    quats = [[1, 0, 0, 0],                       # upright
             _quat([0, 0, 1], 0.7), _quat([0, 0, 1], -2.9), [0, 0, 0, 1],   # any yaw
             [s, s, 0, 0], [s, 0, s, 0],         # 90 degrees about x, about y
             [0, 1, 0, 0], [0, 0, 1, 0]]         # inverted: half a turn about x, about y
    up = up_component(_qpos(quats))
    assert up.dtype == np.float32
    assert up[0] == 1.0 and (up[1:4] == 1.0).all()
    assert abs(up[4]) < 1e-7 and abs(up[5]) < 1e-7
    assert up[6] == -1.0 and up[7] == -1.0


def test_up_component_mixed_roll_pitch_yaw_against_a_rotation_matrix():
    rng = np.random.default_rng(5)
    for roll, pitch, yaw in [(0.3, -0.5, 1.1), (1.2, 0.9, -2.0), (-2.5, 0.4, 0.3)] + [tuple(rng.uniform(-3, 3, 3)) for _ in range(20)]:
        q = _qmul(_quat([0, 0, 1], yaw), _qmul(_quat([0, 1, 0], pitch), _quat([1, 0, 0], roll)))
        R = _rot([0, 0, 1], yaw) @ _rot([0, 1, 0], pitch) @ _rot([1, 0, 0], roll)
        want = R[2, 2]                           # world-z component of the body's z axis
        assert abs(float(up_component(_qpos([q]))[0]) - want) < 5e-7, (roll, pitch, yaw)
        assert abs(want - math.cos(roll) * math.cos(pitch)) < 1e-12
    # a tilt by t about any horizontal axis, whatever the yaw in front of it: up = cos t
    for t in (0.0, 0.3, 0.7, 0.9, 1.5, 3.0):
        for ax in ([1, 0, 0], [0, 1, 0], [0.6, -0.8, 0]):
            q = _qmul(_quat([0, 0, 1], 0.9), _quat(ax, t))
            assert abs(float(up_component(_qpos([q]))[0]) - math.cos(t)) < 5e-7


def test_min_up_round_trip_grace_and_off_values():
    for t in (0.1, 0.8, math.pi / 2, 2.5):
        m = min_up(t)
        assert m == float(np.float32(math.cos(t))) and abs(math.acos(m) - t) < 1e-6
        assert FallRule(tilt=t).min_up == m
    assert min_up(None) == -1.0 and FallRule().min_up == -1.0 and FallRule().min_height == 0.0
    assert FallRule().is_off() and not FallRule(bodies=[]).is_off() and FallRule(tilt=0.8).posture_mask() == TILT
    assert FallRule(tilt=0.8, height=0.1).posture_mask() == TILT | HEIGHT and FallRule(height=0.1).min_height == float(np.float32(0.1))
    # the rule on a pose on either side of the threshold; the threshold itself does not fire (strict <)
    rule = FallRule(tilt=0.8)
    q = _qpos([_quat([1, 0, 0], 0.79), _quat([1, 0, 0], 0.81), _quat([0, 1, 0], 3.0), [1, 0, 0, 0]])
    assert reference_fall(q, 1, rule).tolist() == [0, TILT, TILT, 0]
    exact = _qpos([[1, 0, 0, 0]])
    exact[0, 4] = np.sqrt(np.float32(0.25))      # up = 1 - 2 * 0.25 = 0.5 exactly
    assert up_component(exact)[0] == 0.5 and min_up(math.pi / 3) == 0.5
    assert reference_fall(exact, 1, {"tilt": math.pi / 3}).tolist() == [0] and reference_fall(exact, 1, {"tilt": 1.0}).tolist() == [TILT]
    # grace: the episode clock is 1 on the first step after a reset; the rules hold from step grace + 1 on
    g = FallRule(tilt=0.8, height=0.2, grace=3)
    fallen = _qpos([_quat([1, 0, 0], 1.5)], z=0.1)
    assert [int(reference_fall(fallen, k, g)[0]) for k in (1, 2, 3, 4, 5)] == [0, 0, 0, TILT | HEIGHT, TILT | HEIGHT]
    assert reference_fall(np.repeat(fallen, 3, 0), np.array([3, 4, 100]), g).tolist() == [0, 3, 3]
    # off values: no rule, a rule with nothing set, NaN compares false
    assert reference_fall(fallen, 9, None).tolist() == [0] and reference_fall(fallen, 9, FallRule()).tolist() == [0]
    assert reference_fall(fallen, 9, FallRule(height=0.2)).tolist() == [HEIGHT]
    nan = fallen.copy()
    nan[0, 2:7] = np.nan
    assert reference_fall(nan, 9, FallRule(tilt=0.8, height=0.2)).tolist() == [0]
    # the plane's own height
    assert reference_fall(_qpos([[1, 0, 0, 0]], z=1.1), 1, FallRule(height=0.2), Terrain([0, 0, 1.0])).tolist() == [HEIGHT]
    assert reference_fall(_qpos([[1, 0, 0, 0]], z=1.3), 1, FallRule(height=0.2), Terrain([0, 0, 1.0])).tolist() == [0]


# ------------------------------------------------------------------------------------------------------------ terrain twin
def test_terrain_twin_on_a_hand_built_field():
    """The convention of test_host_logic.test_hfield_png_conventions_known_answer: column c sits at x = -size_x + c * 2 size_x /
    (ncol - 1), row r at y = -size_y + r * 2 size_y / (nrow - 1), the surface height is ground_z + size_z * elevation; every cell is
    split along (r, c)-(r + 1, c + 1) (the ray's triangulation)."""
    data = np.array([[0.0, 0.25, 0.5, 1.0],
                     [0.25, 0.5, 0.0, 0.75],
                     [1.0, 0.0, 0.25, 0.5],
                     [0.5, 0.75, 1.0, 0.0]], dtype=np.float32)
    T = Terrain(pos=[10.0, -20.0, 0.5], size=[3.0, 1.5, 2.0, 0.1], data=data)     # cells of 2 m x 1 m

    def at(x, y):
        h, inside = terrain_height(T, np.float32([x]), np.float32([y]))
        return float(h[0]), bool(inside[0])
    # the vertices
    for r in range(4):
        for c in range(4):
            assert at(10.0 - 3.0 + 2.0 * c, -20.0 - 1.5 + 1.0 * r) == (0.5 + 2.0 * float(data[r, c]), True)
    # cell (r, c) = (0, 0): corners h00 = 0, h01 = 0.25, h10 = 0.25, h11 = 0.5 -> planar; cell (1, 1): h00 = 0.5, h01 = 0, h10 = 0, h11 = 0.25
    x0, y0 = 10.0 - 3.0 + 2.0, -20.0 - 1.5 + 1.0          # origin of cell (1, 1)
    # lower triangle (u >= v): h00 + u (h01 - h00) + v (h11 - h01)
    u, v = 0.75, 0.25
    assert at(x0 + 2.0 * u, y0 + 1.0 * v)[0] == pytest.approx(0.5 + 2.0 * (0.5 + u * (0.0 - 0.5) + v * (0.25 - 0.0)), abs=1e-6)
    # upper triangle (u < v): h00 + v (h10 - h00) + u (h11 - h10)
    u, v = 0.25, 0.75
    assert at(x0 + 2.0 * u, y0 + 1.0 * v)[0] == pytest.approx(0.5 + 2.0 * (0.5 + v * (0.0 - 0.5) + u * (0.25 - 0.0)), abs=1e-6)
    # the two triangles differ: the other split would give the mirrored value at both points
    assert abs(at(x0 + 1.5, y0 + 0.25)[0] - at(x0 + 0.5, y0 + 0.75)[0]) < 1e-6      # symmetric corners of this cell
    assert at(x0 + 1.0, y0 + 0.5)[0] == pytest.approx(0.5 + 2.0 * 0.375, abs=1e-6)  # on the diagonal: between h00 and h11
    # edges are inside, beyond them is not; off the field the height rule does not fire
    assert at(13.0, -18.5) == (0.5 + 2.0 * 0.0, True) and at(7.0, -21.5) == (0.5, True)
    assert at(13.01, -20.0) == (0.0, False) and at(10.0, -18.49)[1] is False and at(6.9, -20.0)[1] is False
    q = _qpos([[1, 0, 0, 0]] * 3, z=1.0)
    q[:, 0], q[:, 1] = [7.0, 13.0 - 1e-3, 20.0], [-21.5, -21.5 + 1e-3, -20.0]      # over height 0.5, ~2.5, off the field
    hgt, inside = base_height(q, T)
    assert inside.tolist() == [True, True, False] and hgt[0] == 0.5 and hgt[1] < -1.4
    assert reference_fall(q, 1, FallRule(height=0.6), T).tolist() == [HEIGHT, HEIGHT, 0]
    assert reference_fall(q, 1, FallRule(height=0.4), T).tolist() == [0, HEIGHT, 0]
    with pytest.raises(ValueError, match="both size and data"):
        Terrain(size=[1, 1, 1, 1])


def test_terrain_of_a_compiled_model():
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    flat = Terrain.of(compile_model(make_config("flamingo_light_v1", random=PARITY_RANDOM)))
    assert flat.data is None and terrain_height(flat, np.float32([3.0]), np.float32([4.0]))[0][0] == flat.pos[2]
    cm = compile_model(make_config("flamingo_light_v1", terrain="rocky_easy", random=PARITY_RANDOM))
    T = Terrain.of(cm)
    assert T.data.shape == cm.hfield.shape and T.size[2] == np.float32(cm.blob.hfield_size[2])
    h, inside = terrain_height(T, np.float32([0.0, 1e6]), np.float32([0.0, 0.0]))
    assert inside.tolist() == [True, False] and T.pos[2] <= h[0] <= T.pos[2] + T.size[2]


# ------------------------------------------------------------------------------------------------------------ validation
def test_validation_messages():
    names = ["world", "base_link", "left_leg_link", "right_leg_link"]
    with pytest.raises(ValueError, match=r"bodies: the model has no body 'left_arm'"):
        FallRule(bodies=["base_link", "left_arm"]).body_ids(names)
    with pytest.raises(ValueError, match=r"'world' is the world body"):
        FallRule(bodies=["world"]).body_ids(names)
    assert FallRule(bodies=["right_leg_link", "base_link"]).body_ids(names).tolist() == [3, 1]
    assert FallRule(tilt=0.5).body_ids(names) is None and FallRule(bodies=[]).body_ids(names).tolist() == []
    with pytest.raises(ValueError, match=r"grace must be >= 0"):
        FallRule(tilt=0.5, grace=-1)
    with pytest.raises(ValueError, match=r"grace must be a whole number"):
        FallRule(grace=1.5)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"tilt must be a finite angle"):
            FallRule(tilt=bad)
    with pytest.raises(ValueError, match=r"tilt must lie in \(0, pi\)"):
        FallRule(tilt=3.5)
    with pytest.raises(ValueError, match=r"height must be > 0"):
        FallRule(height=0.0)
    with pytest.raises(ValueError, match=r"height must be a finite"):
        FallRule(height=float("nan"))
    with pytest.raises(ValueError, match=r"bodies must be a list"):
        FallRule(bodies="base_link")
    with pytest.raises(ValueError, match=r"unknown keys \['tilt_deg'\]"):
        FallRule.build({"tilt_deg": 40})
    r = FallRule.build({"tilt": 0.8, "grace": 2})
    assert (r.tilt, r.height, r.grace, r.bodies) == (0.8, None, 2, None) and FallRule.build(None) is None and FallRule.build(r) is r
    assert FallRule.build(r.as_dict()).as_dict() == r.as_dict()


def test_abi_names():
    from cosim_amd.engine import EXPORTS
    assert "cosim_fall_set" in EXPORTS
    with open(os.path.join(ROOT, "include", "cosim.h")) as f:
        assert "int cosim_fall_set(cosim_engine_t* e, float min_up, float min_height, int grace_steps, const int32_t* body_ids, int n_bodies);" in f.read()


# ------------------------------------------------------------------------------------------------------------ ledger twin
NU, CD = 2, 4


def _rows(K, N):
    info = np.zeros((K, N, 4 + 2 * NU + 1), dtype=np.float32)
    for k in range(K):
        for n in range(N):
            info[k, n, :4] = [k + 1, n, 0.5, -0.25]
            info[k, n, 4:6] = [k + n, -(k + 2)]
    return info


def test_ledger_twin_with_a_cause_array():
    K, N = 6, 4
    info = _rows(K, N)
    term, trunc = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    cause = np.zeros((K, N), dtype=np.int32)
    term[1, 0], cause[1:, 0] = 1, TILT                    # env 0 falls by tilt in step 1; the word stays until the next end
    term[4, 0], cause[4:, 0] = 1, TILT | HEIGHT           # ... and by both in step 4
    term[2, 1], cause[2:, 1] = 1, CONTACT                 # env 1: body contact
    trunc[3, 2] = 1                                       # env 2: the time limit, cause 0
    term[5, 3], trunc[5, 3], cause[5, 3] = 1, 1, HEIGHT   # env 3: height, on the step of the time limit
    cmd = np.zeros((N, CD), dtype=np.float32)
    led = reference_ledger(info, term, trunc, cmd, None, None, slots=4, nu=NU, command_dim=CD, causes=cause)
    assert led.env.tolist() == [0, 0, 1, 2, 3] and led.length.tolist() == [2, 3, 3, 4, 6]
    assert led.flags.tolist() == [TERMINATED | FELL_TILT, TERMINATED | FELL_TILT | FELL_HEIGHT, TERMINATED | FELL_CONTACT, TRUNCATED,
                                  TERMINATED | TRUNCATED | FELL_HEIGHT]
    assert (FELL_TILT, FELL_HEIGHT, FELL_CONTACT) == (32, 64, 128) and FELL == 224
    # only bits 0..2 of the word reach the flags
    wide = cause.copy()
    wide[1, 0] |= 8 | 1024
    assert same_records(reference_ledger(info, term, trunc, cmd, None, None, slots=4, nu=NU, command_dim=CD, causes=wide), led) is None
    # no cause array: today's records, bit for bit -- and the same as a cause array of zeros
    old = reference_ledger(info, term, trunc, cmd, None, None, slots=4, nu=NU, command_dim=CD)
    zero = reference_ledger(info, term, trunc, cmd, None, None, slots=4, nu=NU, command_dim=CD, causes=np.zeros_like(cause))
    assert same_records(old, zero) is None and (old.flags & FELL == 0).all()
    stripped = led.words.copy()
    stripped[:, INT_FIELDS["flags"]] &= ~FELL
    assert np.array_equal(stripped, old.words)
    # open rows carry no cause
    opn = reference_ledger(info, term, trunc, cmd, None, None, slots=4, nu=NU, command_dim=CD, causes=cause, include_open=True)
    assert ((opn.flags[opn.flags & OPEN != 0] & FELL) == 0).all()


def _ledger(flags, spawn, scenario, length):
    n = len(flags)
    words = np.zeros((n, 16), dtype=np.int32)
    words[:, INT_FIELDS["episode"]] = np.arange(n)
    words[:, INT_FIELDS["length"]] = length
    words[:, INT_FIELDS["flags"]] = flags
    words[:, INT_FIELDS["spawn_row"]] = spawn
    words[:, 13] = np.asarray(scenario) + 1
    return EpisodeLedger(words, np.zeros(n), [0], slots=16)


def test_fell_counts_and_shares_on_hand_written_records():
    T = TERMINATED
    led = _ledger([T | FELL_TILT, T | FELL_TILT | FELL_HEIGHT, TRUNCATED, T | FELL_CONTACT, T, TRUNCATED | NO_RESET, OPEN | 0, T | FELL_HEIGHT],
                  spawn=[0, 0, 0, 1, 1, 1, 1, 2], scenario=[0, 1, 0, 1, 0, 1, 0, 0], length=[10, 20, 30, 40, 50, 60, 5, 70])
    c = led.counts()
    assert (c["episodes"], c["terminated"], c["truncated"]) == (7, 5, 2)
    assert (c["fell"], c["fell_tilt"], c["fell_height"], c["fell_contact"]) == (4, 2, 2, 1)
    s = led.summary()
    assert s["fell"] == 4 and s["fell_share"] == 4 / 7 and s["terminated_share"] == 5 / 7
    by = led.by_spawn_row()
    assert by[0] == {"episodes": 3, "terminated": 2, "terminated_share": 2 / 3, "fell": 2, "fell_share": 2 / 3}
    assert by[1] == {"episodes": 3, "terminated": 2, "terminated_share": 2 / 3, "fell": 1, "fell_share": 1 / 3}
    assert by[2] == {"episodes": 1, "terminated": 1, "terminated_share": 1.0, "fell": 1, "fell_share": 1.0}
    sc = led.by_scenario()
    assert (sc[0]["episodes"], sc[0]["terminated"], sc[0]["fell"], sc[0]["fell_share"]) == (4, 3, 2, 0.5)
    assert (sc[1]["episodes"], sc[1]["terminated"], sc[1]["fell"], sc[1]["fell_share"]) == (3, 2, 2, 2 / 3)
    assert sc[1]["length"]["mean"] == 40.0
    # a ledger without a fall flag keeps the tables it had; asked for, the columns are there with zeros
    plain = _ledger([T, TRUNCATED], spawn=[0, 0], scenario=[0, 0], length=[1, 2])
    assert plain.by_spawn_row() == {0: {"episodes": 2, "terminated": 1, "terminated_share": 0.5}}
    assert plain.by_spawn_row(fell=True) == {0: {"episodes": 2, "terminated": 1, "terminated_share": 0.5, "fell": 0, "fell_share": 0.0}}
    assert "fell" not in plain.by_scenario()[0] and plain.by_scenario(fell=True)[0]["fell"] == 0 and "fell" not in led.by_scenario(fell=False)[0]
    assert plain.counts()["fell"] == 0 and plain.summary()["fell_share"] == 0.0
    empty = EpisodeLedger(np.zeros((0, 16), dtype=np.int32), [], [0], slots=2)
    assert empty.counts()["fell"] == 0 and empty.summary()["fell_share"] is None and empty.by_spawn_row(fell=True) == {}


# ------------------------------------------------------------------------------------------------------------ kernel resources
def _kres(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip() for ln in f if ln.strip()]
    rows = []
    for ln in lines[1:]:
        cols = re.split(r"\s+", ln.strip())
        rows.append((" ".join(cols[:-7]), [int(x) for x in cols[-7:]]))
    return lines[0], rows


def test_kernel_resources_with_the_rule_compiled_in():
    """tools/kres.py before (profiles/fall_kres_parent.txt) and after (fall_kres_this.txt): the rule adds no kernel, and every
    kernel keeps its VGPRs, AGPRs, LDS bytes and waves per SIMD.  Scalar-register spills and the scratch of a few instantiations
    moved by a few words in either direction: DESIGN.md section 4.15 lists them, they are not asserted."""
    head_a, a = _kres("fall_kres_parent.txt")
    head_b, b = _kres("fall_kres_this.txt")
    assert head_a == head_b and head_a.split() == ["kernel", "VGPR", "AGPR", "sSpill", "vSpill", "scratch", "occ", "LDS"]
    assert len(a) >= 50 and [n for n, _ in a] == [n for n, _ in b], "the set or the order of the kernels changed"
    for (name, (vgpr0, agpr0, _s0, _v0, _sc0, occ0, lds0)), (_, (vgpr1, agpr1, _s1, _v1, _sc1, occ1, lds1)) in zip(a, b):
        assert (vgpr0, agpr0, occ0, lds0) == (vgpr1, agpr1, occ1, lds1), name
    # the step-only headline kernel still spills no vector register and uses no scratch
    head = [r for n, r in b if n.startswith("void env_kernel<18, 14, 1, false, 11, false, false, 1, 0, 0>")]
    assert len(head) == 1 and head[0][3] == 0 and head[0][4] == 0
