"""The solver primitives that KTraits::LDSB rewrites, both forms side by side in one launch on operands given directly
(cosim_debug_forward "ldsbatch", csrc/cosim_kernels.hip: ldsbatch_probe_kernel), one problem per wave:

  form 0  one read at a time: the dot product as dot_term's chain straight from LDS, chol_fwd_lds / chol_bwd_lds;
  form 1  lds_row_dot (row and vector behind one wait), chol_fwd_lds_b / chol_bwd_lds_b (the multipliers ahead of the chain).

Form 1 moves reads, never an arithmetic operation, so every assertion between the forms is BIT equality (uint32 words).  One test
holds form 0 to numpy float32 arithmetic in the stated order, a fused multiply-add being one rounding of the exact a b + c: the pinned
sequence is then written down twice, in the kernel source and here.  Form 0 of the dot product is that sequence read one term at a
time, not the `s += a[k] * b[k]` loop of mulM / rowdot: this file proves that moving the reads changes nothing and that the sequence is
what it says.  That the sequence is the rounding the compiler gives that loop in the step kernels is held by
tests/test_gpu_ldsbatch_steps.py (whole steps against the rollout kernel, which still runs the loop).

Orders 18 (the kernels built with form 1), 10 and 7 (an odd order: a last pair that reads one float twice); 64 problems each.
Generator: numpy.random.default_rng(SEED + NV), draws in the order written in _problems().
  A [64][NV]   standard normal, one entry in ten an exact zero; rows < NV play M, all 64 rows play J (lane l: row l . v);
  v [NV]       standard normal, entry 1 an exact zero, entry (problem mod NV) a -0.0;
  factor       chol_lower's factor and dinv (form 0 of the "cholesky" hook) of the Cholesky test's matrices (a) for even problems and
               (b) for odd ones, parked as chol_park does (row i scaled by dinv_i, zeros on and above the diagonal); rhs as there.
The batched tail of J^T f measured slower than the rows it replaced and is not in the kernels, and the mask helper was never built, so
neither has a case here: J^T f runs the code tests/test_gpu_row_loops.py covers."""
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_cholesky_forms import _cases, _device as _chol_device, _lanes, engine  # noqa: F401  (engine: the fixture)

pytestmark = pytest.mark.gpu

SEED = 20251021
ORDERS = (18, 10, 7)
N = 64


def _problems(engine, nv):
    rng = np.random.default_rng(SEED + nv)
    A = rng.standard_normal((N, 64, nv)).astype(np.float32)
    A[rng.random((N, 64, nv)) < 0.1] = 0.0
    v = rng.standard_normal((N, nv)).astype(np.float32)
    v[:, 1] = 0.0
    v[np.arange(N), np.arange(N) % nv] = -0.0
    cs = _cases(nv)
    M = np.where((np.arange(N) % 2 == 0)[:, None, None], cs["a"][0], cs["b"][0])
    rhs = np.where((np.arange(N) % 2 == 0)[:, None], cs["a"][1], cs["b"][1]).astype(np.float32)
    fac, dinv, _ = _chol_device(engine, *_lanes(M, rhs))
    fac, dinv = fac[:, 0], dinv[:, 0]                                   # form 0: chol_lower
    Lp = np.tril((fac * dinv[:, :, None]).astype(np.float32), -1)         # chol_park: a[k] * dinv for k < lane, one float32 product
    return dict(A=A, v=v, Lp=Lp, dinv=dinv.astype(np.float32), rhs=rhs)


def _device(engine, P, nv):
    per = 64 * nv + nv * nv + 3 * nv
    io = np.concatenate([P["A"].reshape(N, -1), P["v"], P["Lp"].reshape(N, -1), P["dinv"], P["rhs"]], axis=1)
    io = np.ascontiguousarray(io, dtype=np.float32)
    assert io.shape == (N, per)
    io = io.ravel()
    engine._check(engine.L.cosim_debug_forward(engine.h, nv, b"ldsbatch", io.ctypes.data, io.size))
    o = io[:N * 2 * (64 + 2 * nv)].reshape(N, 2, 64 + 2 * nv)
    return dict(Av=o[:, :, :64].copy(), fwd=o[:, :, 64:64 + nv].copy(), bwd=o[:, :, 64 + nv:].copy())


@pytest.fixture(scope="module")
def runs(engine):
    """order -> (problems, device output).  One launch per order."""
    out = {}
    for nv in ORDERS:
        P = _problems(engine, nv)
        out[nv] = (P, _device(engine, P, nv))
    return out


def _words(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("what", ["Av", "fwd", "bwd"])
@pytest.mark.parametrize("nv", ORDERS)
def test_batched_form_is_the_one_read_at_a_time_form_bit_for_bit(runs, nv, what):
    P, D = runs[nv]
    a, b = _words(D[what][:, 0]), _words(D[what][:, 1])
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"order {nv}, {what}: {len(bad)} words differ, first at problem {bad[0][0]}, lane {bad[0][1]}"
    assert np.isfinite(D[what]).all()


def _fma32(a, b, c):
    """float32 fma(a, b, c), elementwise: a b is exact in float64 and the sum is rounded once there; rounding that to float32 is the
    single rounding of the exact value unless the float64 sum sits exactly on the midpoint of two float32 neighbours, and those
    elements are decided in exact arithmetic."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in np.broadcast_arrays(a, b, c))
    s = a * b + c
    r = s.astype(np.float32)
    tie = (s.view(np.int64) & ((1 << 29) - 1)) == (1 << 28)
    for i in np.argwhere(tie):
        i = tuple(i)
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(r[i], np.float32(-np.inf)), np.nextafter(r[i], np.float32(np.inf))
        cand = sorted((abs(Fraction(float(y)) - exact), int(np.float32(y).view(np.uint32)) & 1, k) for k, y in enumerate((lo, r[i], hi)))
        r[i] = (lo, r[i], hi)[cand[0][2]]                                # nearest; on a tie the even mantissa
    return r


@pytest.mark.parametrize("nv", ORDERS)
def test_one_read_at_a_time_form_is_numpy_float32_in_the_stated_order(runs, nv):
    P, D = runs[nv]
    A, v = P["A"], P["v"]
    # dot: terms 0 .. 5 fused from +0, later terms a rounded product and a rounded add
    s = np.zeros((N, 64), dtype=np.float32)
    for k in range(nv):
        s = _fma32(A[:, :, k], v[:, None, k], s) if k < 6 else (s + (A[:, :, k] * v[:, None, k]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(_words(s), _words(D["Av"][:, 0]))
    # forward: b = rhs dinv, then b = fma(-l_ij, b_j, b) for j = 0 .. nv - 2; backward: the same with column j, j = nv - 1 .. 1, then b dinv
    Lp, dinv = P["Lp"], P["dinv"]
    b = (P["rhs"] * dinv).astype(np.float32)
    for j in range(nv - 1):
        b = _fma32(-Lp[:, :, j], b[:, j:j + 1], b)
    assert np.array_equal(_words(b), _words(D["fwd"][:, 0]))
    for j in range(nv - 1, 0, -1):
        b = _fma32(-Lp[:, j, :], b[:, j:j + 1], b)
    b = (b * dinv).astype(np.float32)
    assert np.array_equal(_words(b), _words(D["bwd"][:, 0]))
    # the signed zeros went through: a row of zeros times v gives the same zero word in numpy and on the device (checked above), and
    # v holds a -0.0 in every problem
    assert (_words(v) == 0x80000000).sum() == N
