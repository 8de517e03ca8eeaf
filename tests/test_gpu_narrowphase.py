"""The device's convex narrowphase on geometry whose answer is known: mpr_probe / mpr_penetration on primitive pairs and on
(prism, primitive) pairs (csrc/cosim_mpr.h) and box_box_lane (csrc/cosim_boxbox.h), reached through the test hooks
cosim_debug_mpr_prims / cosim_debug_mpr_prism / cosim_debug_box_box, against the fp64 oracle.

The cases, the oracle's answers and every bound come from tests/narrowphase_cases.py and are fixed on the CPU
(tests/test_narrowphase_host.py says how): each case is held to its own FLOOR + K * spread; the only cases skipped are those whose
hit / miss (box-box: count) is not stable under the reference's own perturbations.  The exact cases (concentric centres, touching
spheres, every closed-form box pair: dyadic inputs on a tie of the algorithm, where the spread says nothing) are held to the
UNPERTURBED oracle at the floors alone, stable or not, box contacts in order.  Nothing here is calibrated on device output.
Each test is one launch of one to two thousand pairs.

Largest device iteration count (n_iter: the discoverPortal, refinePortal and findPenetr loops of one call together) measured on
MI355X with the committed seeds: 31 on both sets (primitives: a sphere-cyl pair at depth 2e-2; prisms: a sphere on a prism corner at
1e-4), median 10 - 11, against MPR_MAXIT = 50 per loop.  test_no_oracle_hit_is_lost_to_the_iteration_cap prints it.
"""
import numpy as np
import pytest

import narrowphase_cases as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    """Any robot's engine: the hooks use the handle for its device only."""
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    env = BatchedEnv(make_config("flamingo_light_v1", num_envs=2, seed=1), num_envs=2, seed=1)
    yield env.engine
    env.close()


def _mpr_device(engine, cs, coop=0):
    """(Answer, probe [n], n_iter [n]) of the device on an mpr / prism case set."""
    n = cs.n
    irec, frec = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 7), dtype=np.float32)
    if cs.what == "mpr":
        kinds = np.ascontiguousarray(cs.kinds, dtype=np.int32)
        geo = np.ascontiguousarray(np.stack([cs.a, cs.b], 1), dtype=np.float32)
        assert np.array_equal(geo.astype(np.float64), np.stack([cs.a, cs.b], 1))      # the inputs are fp32 values: both sides see the same geometry
        engine._check(engine.L.cosim_debug_mpr_prims(engine.h, kinds.ctypes.data, geo.ctypes.data, n, coop, irec.ctypes.data, frec.ctypes.data))
    else:
        kinds = np.ascontiguousarray(cs.kinds[:, 1], dtype=np.int32)
        prism, geo = np.ascontiguousarray(cs.a, dtype=np.float32), np.ascontiguousarray(cs.b, dtype=np.float32)
        assert np.array_equal(prism.astype(np.float64), cs.a) and np.array_equal(geo.astype(np.float64), cs.b)
        engine._check(engine.L.cosim_debug_mpr_prism(engine.h, prism.ctypes.data, kinds.ctypes.data, geo.ctypes.data, n, irec.ctypes.data, frec.ctypes.data))
    A = N.Answer()
    A.hit = irec[:, 1] != 0
    A.depth, A.normal, A.pos = frec[:, 0].astype(np.float64), frec[:, 1:4].astype(np.float64), frec[:, 4:7].astype(np.float64)
    A.raw = (irec.copy(), frec.copy())
    return A, irec[:, 0] != 0, irec[:, 2]


@pytest.fixture(scope="module")
def device_mpr(engine):
    out = {}
    for what, fn in (("mpr", N.mpr_cases), ("prism", N.prism_cases)):
        cs = fn()
        out[what] = (cs, N.reference(cs)) + _mpr_device(engine, cs)
    return out


@pytest.mark.parametrize("what", ["mpr", "prism"])
def test_device_mpr_lies_within_every_case_bound(device_mpr, what, capsys):
    """Depth, normal and position against the fp64 oracle under the per-case bounds fixed on the CPU; hit / miss equal on every stable
    case deeper than the grazing allowance 1e-5; closed forms, separated, concentric, ratio-100 and frame-shifted cases included."""
    cs, R, A, _, _ = device_mpr[what]
    fails, fig = N.compare(cs, R, A)
    with capsys.disabled():
        print(f"\n[{what}] {cs.n} cases, {int(R.stable.sum())} stable, largest device error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])


@pytest.mark.parametrize("what", ["mpr", "prism"])
def test_device_meets_the_closed_forms(device_mpr, what):
    """The device against the formulas themselves, at the formula's tolerance widened by the case's own bound against the oracle
    (measured bounds of the sphere-sphere cases at depths >= 1e-3: normal 3e-3 at the median, 6e-3 at most, where the fp32 supports
    leave the oracle's origin-on-segment exit for the portal loops; the shallower ones, down to 1e-6, go up to 1.7)."""
    cs, R, A, _, _ = device_mpr[what]
    for i in cs.sel("cf:"):
        if not R.stable[i] or cs.x_hit[i] < 0:
            continue
        tag = f"{what}[{i}] {cs.family[i]}"
        assert bool(A.hit[i]) == bool(cs.x_hit[i]), tag
        if np.isfinite(cs.x_depth[i]):
            assert abs(A.depth[i] - cs.x_depth[i]) <= cs.x_tol[i, 0] + R.b_depth[i], (tag, A.depth[i], cs.x_depth[i])
        if np.isfinite(cs.x_normal[i]).all():
            assert np.linalg.norm(A.normal[i] - cs.x_normal[i]) <= np.sqrt(3) * cs.x_tol[i, 1] + R.b_normal[i], (tag, A.normal[i], cs.x_normal[i])


@pytest.mark.parametrize("what", ["mpr", "prism"])
def test_hits_have_finite_outputs_and_unit_normals(device_mpr, what):
    cs, R, A, _, _ = device_mpr[what]
    h = A.hit
    assert h.sum() > 0.8 * cs.n
    assert np.isfinite(A.depth[h]).all() and np.isfinite(A.normal[h]).all() and np.isfinite(A.pos[h]).all()
    assert np.abs(np.linalg.norm(A.normal[h], axis=1) - 1).max() <= 1e-6


@pytest.mark.parametrize("what", ["mpr", "prism"])
def test_probe_false_implies_no_penetration(device_mpr, what):
    """mpr_probe == false means that mpr_penetration returns false at exactly these points: on every case, stable or not."""
    cs, R, A, probe, _ = device_mpr[what]
    assert not (A.hit & ~probe).any(), np.flatnonzero(A.hit & ~probe)[:10]
    assert (~probe).any() and probe.any()      # both answers occur (the separated and beside cases are decided by the probe)


def test_cooperative_route_returns_the_same_bits(engine, device_mpr):
    """MprPair<.., true>, one pair per wave, against MprPair<.., false>, one pair per lane: same code, same values, same bits."""
    cs, _, A, probe, nit = device_mpr["mpr"]
    B, probe_c, nit_c = _mpr_device(engine, cs, coop=1)
    assert np.array_equal(A.raw[0], B.raw[0])
    assert np.array_equal(A.raw[1].view(np.uint32), B.raw[1].view(np.uint32))


@pytest.mark.parametrize("what", ["mpr", "prism"])
def test_no_oracle_hit_is_lost_to_the_iteration_cap(device_mpr, what, capsys):
    """The device bounds discoverPortal and refinePortal by MPR_MAXIT where the oracle runs them to the end: no case that the oracle hits
    (stable, deeper than grazing) may come back as a miss.  n_iter counts the iterations of the three loops together."""
    cs, R, A, _, nit = device_mpr[what]
    lost = R.stable & R.hit & (R.depth > N.GRAZE) & ~A.hit
    assert not lost.any(), [(int(i), cs.family[i], int(nit[i])) for i in np.flatnonzero(lost)[:10]]
    with capsys.disabled():
        print(f"\n[{what}] largest n_iter {int(nit.max())} (case {int(nit.argmax())}, {cs.family[nit.argmax()]}), median {int(np.median(nit))}")


def test_device_box_box_matches_the_oracle_in_order(engine, capsys):
    """box_box_lane, compacted as the step kernel does: the count on every stable case, the contacts in order (the kernel keeps the first
    eight), position / distance / normal under the per-case bounds; the margin case keeps its positive-distance contacts, the separated
    case none."""
    cs = N.box_cases()
    R = N.reference(cs)
    n = cs.n
    geo = np.ascontiguousarray(np.stack([cs.a, cs.b], 1), dtype=np.float32)
    margin = np.ascontiguousarray(cs.margin, dtype=np.float32)
    assert np.array_equal(geo.astype(np.float64), np.stack([cs.a, cs.b], 1))
    cnt, out = np.full(n, -1, dtype=np.int32), np.zeros((n, 35), dtype=np.float32)
    engine._check(engine.L.cosim_debug_box_box(engine.h, geo.ctypes.data, margin.ctypes.data, n, cnt.ctypes.data, out.ctypes.data))
    A = N.Answer()
    A.count, A.normal, A.pts = cnt.astype(int), out[:, :3].astype(np.float64), out[:, 3:].reshape(n, 8, 4).astype(np.float64)
    fails, fig = N.compare(cs, R, A)
    with capsys.disabled():
        print(f"\n[box] {n} cases, {int(R.stable.sum())} stable, counts {np.bincount(np.minimum(A.count, 8), minlength=9).tolist()}, "
              "largest device error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:30])
    i = cs.sel("cf:margin")[0]
    assert A.count[i] == 4 and (A.pts[i, :4, 3] > 0).all() and np.allclose(A.pts[i, :4, 3], 0.001, atol=2e-6)
    assert A.count[cs.sel("cf:separated")[0]] == 0
    # the closed-form cases sit on ties (parallel faces; edge axes along the face axis) that no perturbation keeps: compare() holds
    # them to the unperturbed oracle at the floors, count and order included; the eight-vertex manifold is the octagon's
    i = cs.sel("cf:octagon")[0]
    assert cs.exact[cs.sel("cf:")].all() and A.count[i] == 8
    live = np.arange(8)[None] < A.count[:, None]
    assert np.isfinite(A.pts[live]).all() and np.abs(np.linalg.norm(A.normal[A.count > 0], axis=1) - 1).max() <= 1e-6


def test_hooks_reject_what_they_cannot_run(engine):
    """A kind without an O(1) support in the probe kernels is an error, not a zero-size geom."""
    kinds = np.array([[N.SPH, 7]], dtype=np.int32)      # 7 = mesh
    geo = np.zeros((1, 2, 10), dtype=np.float32)
    irec, frec = np.zeros((1, 3), dtype=np.int32), np.zeros((1, 7), dtype=np.float32)
    assert engine.L.cosim_debug_mpr_prims(engine.h, kinds.ctypes.data, geo.ctypes.data, 1, 0, irec.ctypes.data, frec.ctypes.data) < 0
    assert engine.L.cosim_debug_mpr_prims(engine.h, kinds.ctypes.data, geo.ctypes.data, 0, 0, irec.ctypes.data, frec.ctypes.data) < 0
