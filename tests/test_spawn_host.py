"""Spawn tables, host side (cosim_amd/spawn.py): the footprint table, the pose generators and the float64 placement rule, the
latter against the fp64 oracle's own collision detection.  No GPU: the device kernel is held to place_reference in
test_gpu_spawn.py."""
import numpy as np
import pytest

from cosim_amd import rng as crng
from cosim_amd import spawn as sp
from cosim_amd.compile import compile_model
from cosim_amd.config import PARITY_RANDOM, make_config
from cosim_amd.model import get_field

ROBOT_TERRAIN = [("flamingo_light_v1", "stairs_up_easy"), ("w4_p_v2", "rocky_hard"), ("humanoid_p_v0", "stairs_up_hard"),
                 ("flamingo_p_v3", "slope_hard")]

_CM = {}


def _cm(robot, terrain):
    if (robot, terrain) not in _CM:
        _CM[(robot, terrain)] = compile_model(make_config(robot, terrain=terrain, random=PARITY_RANDOM))
    return _CM[(robot, terrain)]


def _footprints_inside(cm, xyyaw):
    lx, ly, _ = sp.windows(cm, xyyaw)
    r = sp.footprint(cm).astype(np.float64)[None, :, 2]
    return bool(np.all(np.abs(lx) + r <= cm.blob.hfield_size[0]) and np.all(np.abs(ly) + r <= cm.blob.hfield_size[1]))


@pytest.mark.parametrize("robot,terrain", ROBOT_TERRAIN)
def test_footprint_has_one_sphere_per_ground_geom(robot, terrain):
    """One entry per geom with geom_ground != 0, free >= 0, radius = geom_rbound; on the three wheeled robots the wheels rest on
    z = 0 at init_qpos, so a geom of a wheel body has free == 0.  humanoid_p_v0 has no wheels and its init_qpos holds it off the
    ground (the oracle finds no contact there): its lowest sphere, a foot's, is 3.7 cm up."""
    cm = _cm(robot, terrain)
    b = cm.blob
    fp = sp.footprint(cm)
    ground = np.array(get_field(b, "geom_ground")[:b.ngeom]) != 0
    assert fp.dtype == np.float32 and fp.shape == (int(ground.sum()), 4) and len(fp) > 0
    assert np.all(np.isfinite(fp)) and np.all(fp[:, 3] >= 0) and np.all(fp[:, 2] > 0)
    np.testing.assert_array_equal(fp[:, 2], np.array(get_field(b, "geom_rbound")[:b.ngeom], dtype=np.float32)[ground])
    body = np.array(get_field(b, "geom_bodyid")[:b.ngeom])[ground]
    wheel = np.array(["wheel" in cm.body_names[i] for i in body])
    if robot == "humanoid_p_v0":
        assert not wheel.any() and 0.0 < fp[:, 3].min() < 0.05
    else:
        assert wheel.any() and np.any(fp[wheel, 3] == 0.0), fp[wheel]
    # the horizontal offsets are those of the nominal pose: all within the robot's size of the base
    assert np.hypot(fp[:, 0], fp[:, 1]).max() < 1.0 and sp.footprint_radius(cm) < 1.2


@pytest.mark.parametrize("robot,terrain", ROBOT_TERRAIN)
def test_pose_generators_are_deterministic_and_stay_on_the_field(robot, terrain):
    cm = _cm(robot, terrain)
    a = sp.uniform_poses(cm, 200, seed=7)
    assert a.shape == (200, 3) and a.dtype == np.float32
    np.testing.assert_array_equal(a, sp.uniform_poses(cm, 200, seed=7))
    np.testing.assert_array_equal(a[:50], sp.uniform_poses(cm, 50, seed=7))        # row i depends on (seed, i) only
    np.testing.assert_array_equal(a[120:], sp.uniform_poses(cm, 200, seed=7)[120:])
    assert not np.array_equal(a, sp.uniform_poses(cm, 200, seed=8))
    u = crng.uniform(7, np.arange(200), 0, crng.PURPOSE_SPAWN_POSE, 0).astype(np.float64)
    np.testing.assert_array_equal(a[:, 0], ((2 * u - 1) * sp.default_extent(cm)).astype(np.float32))
    assert np.all(np.abs(a[:, 2]) <= np.pi) and np.unique(np.sign(a[:, 0]) * 2 + np.sign(a[:, 1])).size == 4
    assert _footprints_inside(cm, a)
    sp.check_rows(cm, a)
    for count in (1, 2, 5, 16, 17, 64):
        g = sp.grid_poses(cm, count)
        assert g.shape == (count, 3) and len(np.unique(g[:, :2], axis=0)) == count and np.all(g[:, 2] == 0)
        assert _footprints_inside(cm, g)
        np.testing.assert_array_equal(g, sp.grid_poses(cm, count))
    g = sp.grid_poses(cm, 9, spacing=1.0, yaw=0.5)
    np.testing.assert_allclose(np.unique(g[:, 0]), [-1.0, 0.0, 1.0])
    assert np.all(g[:, 2] == np.float32(0.5))
    gr = sp.grid_poses(cm, 9, extent=2.0, yaw="random")
    assert np.abs(gr[:, :2]).max() == 2.0 and np.unique(gr[:, 2]).size == 9
    with pytest.raises(ValueError):
        sp.grid_poses(cm, 9, extent=1.0, spacing=2.0)
    # the corner of the widest allowed square, turned so that the footprint reaches furthest, is still on the field; one
    # footprint radius further out is not
    e = sp.default_extent(cm)
    for yaw in np.linspace(-np.pi, np.pi, 17):
        sp.check_rows(cm, np.array([[e, -e, yaw]]))
    with pytest.raises(ValueError, match="row 1"):
        sp.check_rows(cm, np.array([[0.0, 0.0, 0.0], [cm.blob.hfield_size[0], 0.0, 0.0]]))
    with pytest.raises(ValueError, match="row 2"):
        sp.check_rows(cm, np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, np.nan, 0.0]]))


def test_resolve_accepts_arrays_and_dicts_and_rejects_other_orientations():
    cm = _cm("w4_p_v2", "rocky_hard")
    xy, clr, per = sp.resolve(cm, np.array([[1.0, 2.0, 0.3], [-4.0, 5.0, -2.0]]))
    assert xy.shape == (2, 3) and xy.dtype == np.float32 and clr == 0.0 and per is False
    xy, clr, per = sp.resolve(cm, {"pattern": "uniform", "count": 32, "extent": 50.0, "per_episode": True, "clearance": 0.02}, seed=11)
    np.testing.assert_array_equal(xy, sp.uniform_poses(cm, 32, 11, 50.0))
    assert clr == 0.02 and per is True
    xy, _, _ = sp.resolve(cm, {"pattern": "grid", "count": 10, "yaw": 1.0})
    np.testing.assert_array_equal(xy, sp.grid_poses(cm, 10, yaw=1.0))
    yaw = 0.7
    xy, _, _ = sp.resolve(cm, {"poses": [[1.0, 2.0, 9.0, np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]]})
    np.testing.assert_allclose(xy, [[1.0, 2.0, yaw]], rtol=1e-6)
    with pytest.raises(ValueError, match="yaw"):
        sp.resolve(cm, {"poses": [[1.0, 2.0, 9.0, np.cos(0.2), np.sin(0.2), 0.0, 0.0]]})      # roll
    with pytest.raises(ValueError):
        sp.resolve(cm, {"pattern": "spiral", "count": 4})
    with pytest.raises(ValueError):
        sp.resolve(cm, {"pattern": "grid"})
    with pytest.raises(ValueError):
        sp.resolve(cm, {"pattern": "grid", "count": 4, "rows": 2})
    with pytest.raises(ValueError):
        sp.resolve(cm, np.zeros((3, 4)))
    with pytest.raises(ValueError, match="row 0"):
        sp.resolve(cm, np.array([[139.99, 0.0, 0.0]]))


def test_episode_row_is_the_documented_draw():
    gids = np.arange(5, 37)
    r = sp.episode_row(9, gids, 3, 64)
    u = crng.uniform(9, gids, 3, crng.PURPOSE_SPAWN, 0)
    np.testing.assert_array_equal(r, np.minimum(63, np.floor(u.astype(np.float64) * 64).astype(np.int64)))
    assert r.min() >= 0 and r.max() <= 63 and np.unique(r).size > 8
    assert np.all(sp.episode_row(9, gids, 3, 1) == 0)
    assert crng.PURPOSE_SPAWN == 5 and crng.PURPOSE_SPAWN_POSE == 6


def _min_contact_distance(o, q):
    o.reset(q)
    o.forward()
    return (o.contacts()[:, 0].min() if o.ncon else None), o.ncon


@pytest.mark.parametrize("robot,terrain,extent", [("flamingo_light_v1", "stairs_up_easy", 3.5), ("w4_p_v2", "rocky_hard", 100.0),
                                                  ("humanoid_p_v0", "stairs_up_hard", 3.5), ("flamingo_p_v3", "slope_hard", 100.0)])
def test_placement_never_penetrates_deeper_than_the_nominal_pose(robot, terrain, extent):
    """64 random spawns per case, default_rng(5), placed by place_reference and handed to the fp64 oracle: the smallest contact
    distance after reset(q); forward() is not below the nominal one -- init_qpos at the origin of the same terrain -- by more
    than 1e-5 m, ten times the 1e-6 convergence tolerance of the oracle's convex collision; where nothing touches at the nominal
    pose nothing touches after placement."""
    from oracle.oracle import Oracle
    cm = _cm(robot, terrain)
    b = cm.blob
    o = Oracle(cm)
    q0 = np.array(get_field(b, "init_qpos")[:b.nq])
    nominal, ncon0 = _min_contact_distance(o, q0)
    rng = np.random.default_rng(5)
    xyyaw = np.column_stack([rng.uniform(-extent, extent, size=(64, 2)), rng.uniform(-np.pi, np.pi, size=64)])
    poses = sp.place_reference(cm, xyyaw, 0.0)
    assert poses.shape == (64, 7) and np.all(poses[:, 2] >= q0[2])
    np.testing.assert_array_equal(poses[:, :2], xyyaw[:, :2].astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(np.linalg.norm(poses[:, 3:], axis=1), 1.0, atol=1e-12)
    worst, touching = np.inf, 0
    for p in poses:
        q = q0.copy()
        q[:7] = p
        d, ncon = _min_contact_distance(o, q)
        touching += ncon > 0
        if d is not None:
            worst = min(worst, d)
    print(f"[{robot} / {terrain}] nominal min contact distance {nominal}, worst after placement {worst if touching else None}, "
          f"spawns with a contact {touching} of 64, lift mean {np.mean(poses[:, 2] - q0[2]):.4f} max {np.max(poses[:, 2] - q0[2]):.4f}")
    if ncon0 == 0:
        assert touching == 0
    else:
        assert worst >= nominal - 1e-5, (worst, nominal)


@pytest.mark.parametrize("robot", ["flamingo_light_v1", "flamingo_p_v3", "w4_p_v2", "humanoid_p_v0"])
def test_flat_terrain_lifts_by_the_clearance_exactly(robot):
    """On `flat` terrain (and wherever the field is 0) dz == clearance exactly: clearance 0 reproduces init_qpos[2] bit for bit."""
    cm = compile_model(make_config(robot, terrain="flat", random=PARITY_RANDOM))
    z0 = get_field(cm.blob, "init_qpos")[2]
    xyyaw = sp.uniform_poses(cm, 16, seed=3)
    p = sp.place_reference(cm, xyyaw, 0.0)
    assert np.all(p[:, 2] == z0)
    np.testing.assert_array_equal(p[:, :2], xyyaw[:, :2].astype(np.float64))
    np.testing.assert_array_equal(sp.place_reference(cm, xyyaw, 0.03)[:, 2], np.full(16, z0 + 0.03))
