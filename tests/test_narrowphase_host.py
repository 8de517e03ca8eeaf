"""The reference side of the narrowphase tests, on the CPU: closed forms, conditioning, and the bounds the device is held to.

tests/narrowphase_cases.py builds three case sets (MPR on primitive pairs, MPR prism - primitive, box-box) and, per case, the fp64
oracle's answer and its SPREAD: the largest deviation from that answer over M perturbed evaluations of the reference.  Every case is
then held to its own bound FLOOR + K * spread, here for the CPU stand-in of the device (the oracle with fp32 support points, box-box
with fp32 rotation matrices) and in tests/test_gpu_narrowphase.py for the device.  Nothing below is calibrated on device output.

What a perturbed evaluation is (narrowphase_cases._samples): every pose / size component moved by +-EPS = 1e-6 (a few fp32 ulp at
unit scale); odd samples run with the fp32-supports switch on; every fourth sample uses 1e-9 instead of EPS (breaks exact ties of
the closed-form inputs without moving an answer).  The fp32-support samples are needed, measured: with fp64 perturbations alone
(M = 8 or 64, EPS 1e-6 or 4e-6) the stand-in misses FLOOR + K * spread on 100 - 200 of 1924 MPR cases (the set before the deep sphere-sphere cases) unless K >= 1.5e4, because
rounding each support point separately is a different disturbance from moving the inputs: spheres on a common axis stay exactly
collinear under every input perturbation (the origin-on-segment exit; spread 5e-6) while fp32 supports send them through the portal
loops (normal off by up to 2.7e-2, position by 1.6e-2), and a box's support jumps between corners when sign(0) is decided by
rounding.  With them, the smallest K for which (a) holds:

    measured on seeds 20250, 20251 and then on the held-out seed 77003 (all committed), M = 512, EPS = 1e-6
      MPR primitives  depth 0.97   normal 1.00   position 1.00      (M = 128: 0.97 / 1.27 / 1.00;  M = 64: 0.98 / 2.59 / 20.5;
      MPR prisms      depth 1.00   normal 1.00   position 0.96       M = 8: 26 / 190 / 192)
      box-box         dist 0.006   normal 0.024  position 0.006     (the stand-in errs by <= 3.6e-8 / 1.8e-6 / 3.8e-5)
    K = 2 is the smallest integer above them.  A ratio of 1.00 means that the stand-in's error equals the spread: for those cases the
    fp32-support samples are what the spread consists of, and the floor is what separates the bound from the error.
    M = 512 and not less, because a branch that fp32 rounding flips with probability p per sample is missed by M / 2 fp32 samples with
    probability (1 - p)^(M/2): at M = 128 the device missed one prism case (prism-sphere-corner/0.02, MI355X: normal error 1.97e-2
    against a bound of 6.2e-4) whose 1.99e-2 deviation 1.9 % of that case's fp32-support samples reproduce on the CPU (4096 samples)
    and of which M = 128 had drawn none (chance 29 %; at M = 512: 0.7 %).  Conditioning the estimate missed, handled by raising M.

Floors (derived, not measured): depth 2e-6 = MPR's tolerance 1e-6 plus the fp32 rounding of two support points at |x| <= 4 (ulp
4.8e-7); normal 2e-5 = an fp32 ulp of a support point (2.4e-7) over the smallest geom (0.02), rounded up; position 2e-6 = four ulp at
|x| <= 4.  Box-box: position 2e-6, distance 1e-6, normal 1e-6.

(b) Ill-posed share = cases whose normal bound exceeds 1e-2 (the normal assertion says little there), per family, measured with the
constants above on the committed seeds (450 cases per family, 120 per prism family):
      sphere-box 0.9 %, cyl-cyl 0.7 % (cap 2 %);  sphere-cyl 15.6 %, cyl-box 20.4 % (cap 1/3);  prism-box-* 1.7 - 3.3 % (cap 7 %, twice the measured);
      prism-sphere-* and prism-cyl-* 13.3 - 18.3 % (cap 1/3).
    The well-posed families are built for it: a sphere over a box-face interior, cylinders crossing side against side.  With generic
    random poses 20 - 30 % of sphere-box and cyl-cyl pairs touch on a box edge or a cylinder rim, where MPR's normal differs from the
    closest-point normal by up to 0.5 in fp64 already and moves by 0.3 under the perturbations (90th percentile 3e-2 .. 5e-2).
    With half of the samples the stand-in itself, (a) is a consistency check of the spread estimate (does a fresh fp32 evaluation stay
    inside K times what M / 2 others showed), not a validation that fp64 conditioning predicts fp32 effects: it does not, see above.
    Cases flagged exact (concentric, touching, the closed-form box pairs) are held to the unperturbed oracle at the floors alone.
(c) Hit / miss (box-box: the count) is the same in all M evaluations for 100 % of the random MPR and prism cases and 99.6 % of the
    random box-box cases; the closed-form cases that sit on exact ties (touching spheres, aligned stacks) are unstable by construction.
    Unstable cases are the only ones a comparison skips.
"""
import numpy as np
import pytest

import narrowphase_cases as N

SETS = {"mpr": N.mpr_cases, "prism": N.prism_cases, "box": N.box_cases}
CAPS = {"sphere-box": 0.02, "cyl-cyl": 0.02, "sphere-cyl": 1 / 3, "cyl-box": 1 / 3,
        # a box on a prism rests on its flat faces and straight edges: measured 1.7 - 3.3 %, cap at twice that so that a loss of
        # conditioning shows; spheres and cylinders on a prism smaller than they are touch ridges and corners (measured 13 - 18 %)
        "prism-box-face": 0.07, "prism-box-ridge": 0.07, "prism-box-corner": 0.07}


def _family_of(name):
    return name.split("/")[0]


@pytest.mark.parametrize("what", ["mpr", "prism"])
def test_oracle_reaches_the_closed_forms(what):
    """The fp64 oracle against the formulas, at the accuracy it reaches on them (sphere-sphere: depth and position 1e-11, normal
    1e-9 -- measured 2e-10 at depth 1e-5, where the normal is a normalised difference of that size; flat faces: depth 8e-7, normal 8e-6,
    position not asserted; cylinder side: depth 1e-6, normal 4e-3; crossed cylinders 1e-5 / 1e-3; aligned boxes 1e-9)."""
    cs = SETS[what]()
    R = N.reference(cs)
    cf = cs.sel("cf:")
    assert len(cf) >= 15
    for i in cf:
        tag = f"{what}[{i}] {cs.family[i]}"
        if cs.x_hit[i] >= 0:
            assert bool(R.hit[i]) == bool(cs.x_hit[i]), tag
        if np.isfinite(cs.x_depth[i]):
            assert abs(R.depth[i] - cs.x_depth[i]) <= cs.x_tol[i, 0], (tag, R.depth[i], cs.x_depth[i])
        if np.isfinite(cs.x_normal[i]).all():
            assert np.abs(R.normal[i] - cs.x_normal[i]).max() <= cs.x_tol[i, 1], (tag, R.normal[i], cs.x_normal[i])
        m = np.isfinite(cs.x_pos[i])
        if m.any():
            assert np.abs(R.pos[i] - cs.x_pos[i])[m].max() <= cs.x_tol[i, 2], (tag, R.pos[i], cs.x_pos[i])
    # the reference values of the exits without a closed form
    if what == "mpr":
        i = cs.sel("cf:concentric")[0]     # box / sphere, same centre: the epsilon-shift branch answers 0.5 + 0.25 along -x
        assert R.depth[i] == pytest.approx(0.75, abs=1e-9) and np.allclose(R.normal[i], [-1, 0, 0], atol=1e-9)
        assert not R.hit[cs.sel("cf:touching")].any()


def test_box_box_closed_forms():
    """The cases of test_oracle_kat.test_box_box_manifolds_have_closed_form_vertices from fp32 inputs, the swapped pair, the stack."""
    cs = N.box_cases()
    R = N.reference(cs)
    for i in cs.sel("cf:"):
        f, n = cs.family[i], R.count[i]
        assert n == cs.x_count[i], (f, n)
        if n == 0:
            continue
        assert np.allclose(R.normal[i], cs.x_normal[i], atol=1e-6), f
        if np.isfinite(cs.x_depth[i]):
            assert np.allclose(R.pts[i, :n, 3], -cs.x_depth[i], atol=1e-7), (f, R.pts[i, :n, 3])
    p = R.pts[cs.sel("cf:corner")[0], :4]
    assert {(round(x, 6), round(y, 6)) for x, y in p[:, :2]} == {(0.0, -0.05), (0.2, -0.05), (0.2, 0.15), (0.0, 0.15)} and np.allclose(p[:, 2], 0.0995, atol=1e-7)
    p = R.pts[cs.sel("cf:octagon")[0]]
    a = np.abs(p[:, :2])
    assert np.allclose(a.max(axis=1), 0.1, atol=1e-7) and np.allclose(a.sum(axis=1), np.sqrt(2) * 0.1, atol=1e-7) and np.allclose(p[:, 2], 0.099, atol=1e-7)
    assert len({(round(x, 5), round(y, 5)) for x, y in p[:, :2]}) == 8
    assert np.allclose(R.pts[cs.sel("cf:crossed-edge")[0], 0, :3], [0, 0, 0.1 * np.sqrt(2) - 0.001], atol=1e-7)
    i = cs.sel("cf:margin")[0]
    assert (R.pts[i, :4, 3] > 0).all()           # separated faces admitted by the margin
    i = cs.sel("cf:tilt")[0]
    t = 0.02
    assert np.allclose(R.pts[i, :2, 3], 0.2 - 0.1 * np.cos(t) - 0.1 * np.sin(t) - 0.1, atol=1e-7)
    p = R.pts[cs.sel("cf:stack")[0], :4]
    assert {(round(x, 6), round(y, 6)) for x, y in p[:, :2]} == {(-0.25, -0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, 0.25)}


@pytest.mark.parametrize("what", ["mpr", "prism", "box"])
def test_standin_lies_within_every_case_bound(what, capsys):
    """(a): the fp32 stand-in against the fp64 oracle, each stable case under its own FLOOR + K * spread, no failures."""
    cs = SETS[what]()
    R = N.reference(cs)
    fails, fig = N.compare(cs, R, N.standin(cs))
    with capsys.disabled():
        print(f"\n[{what}] {cs.n} cases, stable {R.stable.mean():.4f}, largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("what", ["mpr", "prism", "box"])
def test_held_out_seed(what):
    """(a) again on cases from a seed that took no part in choosing M and K."""
    cs = SETS[what](seeds=(N.HELD_OUT_SEED,))
    R = N.reference(cs)
    fails, _ = N.compare(cs, R, N.standin(cs))
    assert not fails, "\n".join(fails[:20])
    rnd = ~np.char.startswith(cs.family, "cf:")
    assert R.stable[rnd].mean() >= 0.99


def test_illposed_share_per_family():
    """(b): the share of cases whose normal bound exceeds 1e-2 stays under the family's cap (1/3 for every prism family: a terrain
    prism is smaller than the geoms on it, so ridge and corner contacts are the rule there)."""
    for what in ("mpr", "prism"):
        cs = SETS[what]()
        R = N.reference(cs)
        fam = np.array([_family_of(f) for f in cs.family])
        for f in dict.fromkeys(fam[~np.char.startswith(fam, "cf:")].tolist()):
            share = float(np.mean(R.b_normal[fam == f] > 1e-2))
            assert share <= CAPS.get(f, 1 / 3), (f, share)


@pytest.mark.parametrize("what", ["mpr", "prism", "box"])
def test_hit_and_count_are_stable_under_perturbation(what):
    """(c): >= 99 % of the random cases; the rest (and the closed-form cases on exact ties) are what a comparison may skip."""
    cs = SETS[what]()
    R = N.reference(cs)
    rnd = ~np.char.startswith(cs.family, "cf:")
    assert R.stable[rnd].mean() >= 0.99, R.stable[rnd].mean()
    if what == "box":   # the near-parallel family reaches multi-point manifolds
        assert set(np.unique(R.count[cs.sel("box-parallel")])) >= {1, 2, 4}
        assert R.stable[cs.sel("cf:crossed-edge")].all() and R.stable[cs.sel("cf:separated")].all()


def test_random_families_sit_at_their_depths():
    """After the rounding to fp32 the oracle's depth is the family's target to 2e-6, or to 20 % where a rim contact amplifies the rounding."""
    for what in ("mpr", "prism"):
        cs = SETS[what]()
        R = N.reference(cs)
        for f in cs.families():
            if not f.startswith("cf:"):
                i = cs.sel(f)
                target = float(f.split("/")[1])
                assert R.hit[i].all() and np.allclose(R.depth[i], target, rtol=0.2, atol=2e-6), f
                assert np.median(np.abs(R.depth[i] - target)) < 2e-6, f


def test_fp32_supports_switch_and_prism_hook():
    """The switch is off by default and restored by the context; it changes answers only in the low digits; oracle_mpr_prism (the
    twin of oracle_mpr_prims) agrees with the batched form."""
    from oracle import oracle as O
    L = O.lib()
    assert L.oracle_get_fp32_supports() == 0
    cs = N.prism_cases()
    R = N.reference(cs)
    with O.fp32_supports():
        assert L.oracle_get_fp32_supports() == 1
    assert L.oracle_get_fp32_supports() == 0
    A = N.standin(cs)
    assert (A.depth != R.depth).any() and np.abs(A.depth - R.depth)[R.hit & A.hit].max() < 1e-2
    for i in list(cs.sel("cf:")) + list(cs.sel("prism-box-ridge"))[:5]:
        pose = np.concatenate([cs.b[i, :3], N.quat_mat(cs.b[i, 3:7]).ravel()])
        size, pr, out = cs.b[i, 7:].copy(), cs.a[i].copy(), np.zeros(7)
        kind = {N.SPH: 0, N.CYL: 1, N.BOX: 2}[int(cs.kinds[i, 1])]
        rc = L.oracle_mpr_prism(pr.ctypes.data, kind, pose.ctypes.data, size.ctypes.data, out.ctypes.data)
        assert (rc == 0) == bool(R.hit[i])
        if rc == 0:
            assert out[0] == R.depth[i] and (out[1:4] == R.normal[i]).all() and (out[4:7] == R.pos[i]).all()
