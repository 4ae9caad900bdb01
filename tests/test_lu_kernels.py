"""smg_log_determinant_fwd / _rev (the blocked LU with partial pivoting of
csrc/lu.hip) through the C ABI: the defining properties of partial pivoting on
the device's own LU and piv, the value against numpy, the gradient against
adj A^{-T}.

Shapes cross the 64-column panel (63, 64, 65, 130) and the panel kernel's
1024-thread row stride (1100: 18 panels, the last of 12 columns).  A and Aadj
sit in padded buffers (lda, ldaa > n; NaN / sentinel padding); LU (n x n,
ld n) is followed by a sentinel column.

Bounds: |P A - L U| <= 4 gamma_n |L| |U| elementwise (the a-priori bound of
Gaussian elimination, gamma_n = n u / (1 - n u), with room for the float64
product that checks it above n = 130); out[0] against sum log|u_ii| of the
device's own U at gamma_{n + 4} sum |log|u_ii|| (n - 1 additions, the log's
1 ulp = 2 u, fabs exact: c = 4 with one in hand).
"""
import functools

import numpy as np
import pytest

from _ref_tangent import LD, Mat, apply_swaps, gamma, same_bits, sentinel
from _util import near_rel

RTOL = 1e-10
SHAPES = [1, 2, 63, 64, 65, 130, 1100]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from math_amd import hip
    c = hip.Context(0, 1 << 30)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _rewind(request):
    if "ctx" not in request.fixturenames:
        yield
        return
    c = request.getfixturevalue("ctx")
    m = c.mark()
    yield
    assert c.status() == 0
    c.rewind(m)


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    rng = np.random.default_rng(10 * n + len(kind))
    if kind == "uniform":        # generic pivoting
        return rng.uniform(-1.0, 1.0, (n, n))
    if kind == "permuted":       # R / sqrt(n) + 2 Pi: condition number about 2.3, n - O(1) real swaps
        Pi = np.eye(n)[rng.permutation(n)]
        return rng.uniform(-1.0, 1.0, (n, n)) / np.sqrt(n) + 2.0 * Pi
    if kind == "ties":           # every candidate of the first column ties
        return np.where(rng.uniform(size=(n, n)) < 0.5, -1.0, 1.0)
    assert kind.startswith("zerocol")
    A = rng.uniform(-1.0, 1.0, (n, n))
    A[:, int(kind[7:])] = 0.0
    return A


def factor(ctx, A, shift=0):
    """(LU, piv, out[0], the device pointers of LU and piv) of A in a padded buffer."""
    n = A.shape[0]
    mA = Mat(A, n + 1 + shift, np.nan)
    mA.put(ctx)
    lu0 = np.concatenate([np.full(n * n, np.nan), sentinel(n + 8)])
    dLU = ctx.put(lu0)
    dpiv = ctx.put(np.full(n + 4, -7, np.int32))
    ws = ctx.put(np.full(64 * 64 + 8, np.nan))
    dout = ctx.put(np.array([np.nan, 123.25]))
    ctx.call("smg_log_determinant_fwd", mA.dev, mA.ld, n, dLU, dpiv, ws, dout)
    lu = ctx.get(dLU, lu0.size)
    assert same_bits(lu[n * n:], lu0[n * n:]), "LU overstepped"
    piv = ctx.get(dpiv, n + 4, dtype=np.int32)
    assert np.all(piv[n:] == -7), "piv overstepped"
    out = ctx.get(dout, 2)
    assert out[1] == 123.25
    return lu[:n * n].reshape(n, n).T.copy(), piv[:n].copy(), out[0], dLU, dpiv


def check_factorisation(A, LU, piv):
    n = A.shape[0]
    k = np.arange(n)
    assert np.all((k <= piv) & (piv < n)), "piv out of range"
    L = np.tril(LU, -1) + np.eye(n)
    Um = np.triu(LU)
    assert np.abs(np.tril(LU, -1)).max(initial=0.0) <= 1.0, "a multiplier above 1: not the largest pivot"
    dt = LD if n <= 130 else np.float64
    res = np.abs(apply_swaps(A, piv).astype(dt) - L.astype(dt) @ Um.astype(dt))
    bound = 4.0 * gamma(n) * (np.abs(L) @ np.abs(Um))
    print(f"n={n}: max residual / bound {float((res / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.all(res <= bound), float((res / np.maximum(bound, 1e-300)).max())


def check_value(LU, out0):
    n = LU.shape[0]
    logs = np.log(np.abs(np.diag(LU).astype(LD)))
    assert abs(out0 - logs.sum()) <= gamma(n + 4) * float(np.abs(logs).sum()), (out0, float(logs.sum()))


@pytest.mark.parametrize("kind", ["uniform", "permuted"])
@pytest.mark.parametrize("n", SHAPES)
def test_lu_forward(ctx, n, kind):
    A = matrix(kind, n)
    LU, piv, out0, _, _ = factor(ctx, A, shift=n % 2)
    assert np.isfinite(LU).all()
    check_factorisation(A, LU, piv)
    check_value(LU, out0)
    if kind == "permuted":
        near_rel(out0, np.linalg.slogdet(A)[1], 1e-12, what="log|det| against numpy")
        if n > 2:
            assert (piv != np.arange(n)).sum() >= n // 2  # real swaps
    LU2, piv2, out2, _, _ = factor(ctx, A, shift=1 + n % 2)      # the other parity of lda: the same bits
    assert same_bits(LU2, LU) and np.array_equal(piv2, piv) and out2 == out0


def test_lu_ties_take_the_first_row(ctx):
    A = matrix("ties", 65)
    LU, piv, out0, _, _ = factor(ctx, A)
    assert piv[0] == 0
    check_factorisation(A, LU, piv)


@pytest.mark.parametrize("col", [5, 70, 129])
def test_lu_zero_column(ctx, col):
    """An exactly zero column: the factorisation completes (LAPACK getf2
    semantics), out[0] == -inf, no NaN in LU."""
    A = matrix(f"zerocol{col}", 130)
    LU, piv, out0, _, _ = factor(ctx, A)
    assert not np.isnan(LU).any()
    assert out0 == -np.inf
    assert np.all((np.arange(130) <= piv) & (piv < 130))


def test_lu_empty(ctx):
    """n == 0: log|det| of the empty matrix is 0; the reverse is a no-op."""
    dout = ctx.put(np.array([np.nan, 5.0]))
    ctx.call("smg_log_determinant_fwd", None, 0, 0, None, None, None, dout)
    assert np.array_equal(ctx.get(dout, 2), [0.0, 5.0])
    ctx.call("smg_log_determinant_rev", None, None, 0, 1.0, None, 0, None, None)


@pytest.mark.parametrize("n", SHAPES)
def test_lu_reverse(ctx, n):
    A = matrix("permuted", n)
    LU, piv, out0, dLU, dpiv = factor(ctx, A)
    rng = np.random.default_rng(n)
    Aadj0 = rng.uniform(-1.0, 1.0, (n, n))
    adj = -0.75
    ws = ctx.put(np.full(3 * n * n + 8, np.nan))
    iws = ctx.put(np.full(n + 4, -7, np.int32))
    ref = Aadj0 + adj * np.linalg.inv(A).T
    for shift in (0, 1):
        mAa = Mat(Aadj0, n + 2 + shift)
        mAa.put(ctx)
        ctx.call("smg_log_determinant_rev", dLU, dpiv, n, adj, mAa.dev, mAa.ld, ws, iws)
        near_rel(mAa.get(ctx), ref, RTOL, atol=RTOL * float(np.abs(ref).max()), what="Aadj")
    assert np.all(ctx.get(iws, n + 4, dtype=np.int32)[n:] == -7)
    mAa = Mat(Aadj0, n + 3)
    mAa.put(ctx)
    ctx.call("smg_log_determinant_rev", dLU, dpiv, n, 0.0, mAa.dev, mAa.ld, ws, iws)   # adj == 0
    assert same_bits(mAa.get(ctx), Aadj0)
