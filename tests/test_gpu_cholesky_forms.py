"""The two forms of the step kernels' in-register Cholesky and its solve, side by side on matrices chosen to hurt
(cosim_debug_forward "cholesky", csrc/cosim_kernels.hip: chol_probe_kernel):

  form 0  chol_lower / chol_park / chol_solve_lds: scalar trailing updates, both substitutions from LDS;
  form 1  chol_lower_pk / chol_park_fwd / chol_bwd_lds: packed trailing updates (v_pk_fma_f32 fed from a scalar register pair), pivot
          look-ahead, forward substitution from the factor's registers (KTraits::CHOLP).

Form 1 reorders and packs independent operations only, so every assertion on the device's output is BIT equality between the two
forms (factor, dinv and solution compared as uint32 words).  numpy's float64 Cholesky of the same inputs is a sanity bound only:
8 NV eps32 max|L| on the factor, 100 NV eps32 max|x| on the solution -- NV roundings of half an ulp on terms no larger than the
largest entry, with a factor 16 (factor) and the condition number of the well-conditioned cases, < 10, times 20 (solution) to spare.

Inputs: 64 matrices per case and order, NV = 18 (the order of the kernels built with form 1), 10 (a smaller even order) and 7 (an odd
one: both parities of every trailing count, the chunk sizes 4, 3, 2 and 1, the pad column).  Generator: numpy.random.default_rng(SEED +
100 * case + NV) with SEED = 20250611, cases numbered a = 0, b = 1, b2 = 2, c = 3; standard_normal draws in the order written in
_cases().  Every matrix is rounded to float32 before either side sees it.
  (a)  A A^T + NV I, A standard normal [NV][NV];
  (b)  the headline's structure: a dense base block, two leg blocks coupled to the base only, exact zeros between the legs; values
       standard normal, the diagonal set to the row's absolute sum + 1 (strictly diagonally dominant: positive definite);
  (b2) as (b) with the legs decoupled from the base as well (block diagonal): every multiplier outside a column's own block is an
       exact zero and goes through the packed path as one;
  (c)  pivot clamp: (a)'s leading block, a last row of +-2^-60 and a last diagonal of 2^-110 = 7.7e-34: positive definite (float64
       factorises it) with a last pivot below the 1e-30 clamp, so dinv's last entry must be rsqrt(1e-30) in both forms;
  (d)  (a) with NaN and +-inf in the slots the routines document as garbage (k > i of every row, all of the lanes >= NV, the
       right-hand side of those lanes): no returned word may differ from (a)'s.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20250611
ORDERS = (18, 10, 7)
N = 64
EPS32 = float(np.finfo(np.float32).eps)


def _blocks(nv):
    """(base, leg 1, leg 2) index ranges: 6 + 6 + 6 of 18, 3 + 3 + 4 of 10, 2 + 2 + 3 of 7."""
    nb = nv // 3
    l1 = (nv - nb) // 2
    return np.arange(nb), np.arange(nb, nb + l1), np.arange(nb + l1, nv)


def _structured(rng, nv, couple_base):
    M = rng.standard_normal((N, nv, nv))
    M = 0.5 * (M + M.transpose(0, 2, 1))
    base, l1, l2 = _blocks(nv)
    M[:, l1[:, None], l2[None, :]] = 0.0
    M[:, l2[:, None], l1[None, :]] = 0.0
    if not couple_base:
        for leg in (l1, l2):
            M[:, base[:, None], leg[None, :]] = 0.0
            M[:, leg[:, None], base[None, :]] = 0.0
    i = np.arange(nv)
    M[:, i, i] = 0.0
    M[:, i, i] = np.abs(M).sum(axis=2) + 1.0
    return M


def _cases(nv):
    """name -> (matrices [N][nv][nv] as float32 values in float64, right-hand sides [N][nv])."""
    out = {}
    rng = np.random.default_rng(SEED + nv)
    A = rng.standard_normal((N, nv, nv))
    Ma = A @ A.transpose(0, 2, 1) + nv * np.eye(nv)
    out["a"] = (0.5 * (Ma + Ma.transpose(0, 2, 1)), rng.standard_normal((N, nv)))
    rng = np.random.default_rng(SEED + 100 + nv)
    out["b"] = (_structured(rng, nv, True), rng.standard_normal((N, nv)))
    rng = np.random.default_rng(SEED + 200 + nv)
    out["b2"] = (_structured(rng, nv, False), rng.standard_normal((N, nv)))
    rng = np.random.default_rng(SEED + 300 + nv)
    Mc = out["a"][0].copy()
    sign = np.where(rng.standard_normal((N, nv - 1)) < 0, -1.0, 1.0)
    Mc[:, nv - 1, :nv - 1] = sign * 2.0 ** -60
    Mc[:, :nv - 1, nv - 1] = sign * 2.0 ** -60
    Mc[:, nv - 1, nv - 1] = 2.0 ** -110
    out["c"] = (Mc, rng.standard_normal((N, nv)))
    return {k: (M.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)) for k, (M, b) in out.items()}


def _lanes(M, b, poison=False):
    """What the wave's 64 lanes hold: rows [N][64][nv], rhs [N][64].  Lanes >= nv: a copy of row 0, as in the step kernels."""
    nv = M.shape[1]
    rows = np.empty((N, 64, nv), dtype=np.float32)
    rows[:, :nv] = M
    rows[:, nv:] = M[:, :1]
    rhs = np.zeros((N, 64), dtype=np.float32)
    rhs[:, :nv] = b
    if poison:
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        k, i = np.meshgrid(np.arange(nv), np.arange(nv))
        up = k > i
        rows[:, :nv][:, up] = bad[(np.arange(int(up.sum())) % 3)]
        rows[:, nv:] = bad[np.arange((64 - nv) * nv).reshape(64 - nv, nv) % 3]
        rhs[:, nv:] = bad[np.arange(64 - nv) % 3]
    return rows, rhs


def _device(engine, rows, rhs):
    """One block, read and written (include/cosim.h): rows, then rhs; back come fac [N][2][nv][nv], dinv and sol [N][2][nv]."""
    nv = rows.shape[2]
    io = np.concatenate([rows.ravel(), rhs.ravel()]).astype(np.float32)
    assert io.size == N * 64 * (nv + 1)
    engine._check(engine.L.cosim_debug_forward(engine.h, nv, b"cholesky", io.ctypes.data, io.size))
    nf, nd = N * 2 * nv * nv, N * 2 * nv
    return io[:nf].reshape(N, 2, nv, nv).copy(), io[nf:nf + nd].reshape(N, 2, nv).copy(), io[nf + nd:nf + 2 * nd].reshape(N, 2, nv).copy()


@pytest.fixture(scope="module")
def engine():
    """Any robot's engine: the hook uses the handle for its device only."""
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    env = BatchedEnv(make_config("flamingo_light_v1", num_envs=2, seed=1), num_envs=2, seed=1)
    yield env.engine
    env.close()


@pytest.fixture(scope="module")
def runs(engine):
    """(order, case) -> (M, b, fac, dinv, sol); case "d" is (a) poisoned.  One launch each."""
    out = {}
    for nv in ORDERS:
        cs = _cases(nv)
        for name, (M, b) in cs.items():
            out[nv, name] = (M, b) + _device(engine, *_lanes(M, b))
        M, b = cs["a"]
        out[nv, "d"] = (M, b) + _device(engine, *_lanes(M, b, poison=True))
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same_forms(fac, dinv, sol):
    bad = [name for name, x in (("factor", fac), ("dinv", dinv), ("solution", sol)) if not np.array_equal(_bits(x[:, 0]), _bits(x[:, 1]))]
    return bad


@pytest.mark.parametrize("nv", ORDERS)
@pytest.mark.parametrize("case", ["a", "b", "b2", "c", "d"])
def test_packed_form_equals_scalar_form_bit_for_bit(runs, nv, case):
    M, b, fac, dinv, sol = runs[nv, case]
    assert not np.array_equal(_bits(fac[:, 0]), np.zeros_like(_bits(fac[:, 0]))), "the probe wrote nothing"
    bad = _same_forms(fac, dinv, sol)
    if bad:
        w = np.argwhere(_bits(fac[:, 0]) != _bits(fac[:, 1]))
        print(f"NV {nv} case {case}: {bad} differ; factor words that differ: {len(w)}, first (matrix, row, column) {w[:5].tolist()}")
    assert not bad, f"forms differ in {bad}"


@pytest.mark.parametrize("nv", ORDERS)
@pytest.mark.parametrize("case", ["a", "b", "b2"])
def test_both_forms_lie_within_the_float64_sanity_bound(runs, nv, case):
    M, b, fac, dinv, sol = runs[nv, case]
    L = np.linalg.cholesky(M)            # raises outside its domain
    x = np.linalg.solve(M, b[..., None])[..., 0]
    assert np.isfinite(L).all() and (np.diagonal(L, axis1=1, axis2=2) > 0).all()
    for form in (0, 1):
        eL = np.abs(fac[:, form].astype(np.float64) - L).max(axis=(1, 2)) / np.abs(L).max(axis=(1, 2))
        ex = np.abs(sol[:, form].astype(np.float64) - x).max(axis=1) / np.abs(x).max(axis=1)
        ed = np.abs(dinv[:, form].astype(np.float64) * np.diagonal(L, axis1=1, axis2=2) - 1.0).max()
        print(f"NV {nv} case {case} form {form}: factor {eL.max():.2e} (bound {8 * nv * EPS32:.2e}), solution {ex.max():.2e} (bound {100 * nv * EPS32:.2e}), dinv {ed:.2e}")
        assert eL.max() <= 8 * nv * EPS32 and ex.max() <= 100 * nv * EPS32 and ed <= 8 * nv * EPS32


@pytest.mark.parametrize("nv", ORDERS)
def test_clamped_last_pivot_survives_the_reordering(runs, nv):
    M, b, fac, dinv, sol = runs[nv, "c"]
    L = np.linalg.cholesky(M)            # positive definite in float64: the reference is inside its domain
    assert (np.diagonal(L, axis1=1, axis2=2) > 0).all()
    clamp = np.float32(1.0) / np.sqrt(np.float32(1e-30))
    for form in (0, 1):
        assert np.isfinite(fac[:, form]).all() and np.isfinite(dinv[:, form]).all() and np.isfinite(sol[:, form]).all()
        assert np.allclose(dinv[:, form, nv - 1], clamp, rtol=4 * EPS32, atol=0), "the last pivot was not clamped to 1e-30"
        lead = np.abs(fac[:, form, :nv - 1, :nv - 1].astype(np.float64) - L[:, :nv - 1, :nv - 1]).max() / np.abs(L).max()
        assert lead <= 8 * nv * EPS32
    assert np.array_equal(_bits(dinv[:, 0]), _bits(dinv[:, 1]))


@pytest.mark.parametrize("nv", ORDERS)
def test_poison_in_the_garbage_slots_reaches_no_returned_word(runs, nv):
    clean, dirty = runs[nv, "a"], runs[nv, "d"]
    for name, c, d in zip(("factor", "dinv", "solution"), clean[2:], dirty[2:]):
        assert np.isfinite(d).all(), f"non-finite {name}"
        assert np.array_equal(_bits(c), _bits(d)), f"{name} changed under poison"
