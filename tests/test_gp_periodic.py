"""gp_periodic_cov and gp_dot_prod_cov, square and cross: the entries
smg_gp_periodic_cov_fwd / _rev and smg_gp_dot_prod_cov_fwd / _rev through
ctypes, and the stan::math overloads through the tape
(tests/cpp/test_gp_periodic.cpp).

The reference of every test is float64 numpy written from the formulas.  With
d = |x1_i - x2_j| (D == 1) or the square root of the squared distance summed in
coordinate order, s2 = sigma^2 and a = pi d / p, every position alike:

    periodic  K = s2 exp(-2 sin^2(a) / l^2)       dK/dsigma = 2 K / sigma
              dK/dl = K 4 sin^2(a) / l^3          dK/dp = K (2 pi d / (l^2 p^2)) sin(2a)
    dot prod  K = s2 + sum_d x1_id x2_jd           dK/dsigma = 2 sigma

Tolerances.  Periodic K at 1e-13 relative where max(a) 2 / l^2 < 60: that
quantity bounds K's relative sensitivity to the rounding of the argument of the
sine (|dK/K| = (2 / l^2) |sin(2a)| a |da/a|), so a few 2^-53 of it stay below
1e-14; every reference that backs a K tolerance asserts it.  The points are
drawn from (-h, h) with h = 4.4 / sqrt(D): d <= 8.8 and the quantity is at most
pi 8.8 / 1.7 * 2 / 0.81 = 40.2.  The hyperparameter adjoints are sums that
cancel (dK/dp changes sign across the matrix), so they are bounded by 1e-11 of
the sum of their terms' absolute values; the dot product's K, which cancels
too, by 1e-13 (sigma^2 + sum_d |x1_id x2_jd|) (its rounding bound is (D + 1)
2^-53 of that sum, 8e-15 at D = 70).  Through the tape: fx at 1e-12, gradient
entries at 1e-10, with an absolute part of 1e-10 of the sum of the absolute
terms where the entry cancels.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import gen
from _util import ROOT, near_rel, prebuilt

gpu = pytest.mark.gpu

SIG, ELL, PER = 1.3, 0.9, 1.7
SMG_ERR_ARG = 16
COND_MAX = 60.0


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


def F(a):  # column-major flat
    return np.asfortranarray(a).ravel(order="F")


# ------------------------------------------------------------ numpy reference
def dist(x1, x2):
    """d_ij for x1 (n1, D), x2 (n2, D): |x1_i - x2_j| for D == 1, else the square
    root of the squared distance summed in coordinate order."""
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    if x1.shape[1] == 1:
        return np.abs(x1[:, 0][:, None] - x2[:, 0][None, :])
    d2 = np.zeros((x1.shape[0], x2.shape[0]))
    for c in range(x1.shape[1]):
        t = x1[:, c][:, None] - x2[:, c][None, :]
        d2 += t * t
    return np.sqrt(d2)


def per_ref(d, sigma, l, p):
    """(K, dK/dsigma, dK/dl, dK/dp, max(a) 2 / l^2), every position alike."""
    a = np.pi * d / p
    s = np.sin(a)
    K = sigma * sigma * np.exp(-2 * s * s / (l * l))
    Kp = K * (2 * np.pi * d / (l * l * p * p)) * np.sin(2 * a)
    return K, 2 * K / sigma, K * 4 * s * s / (l * l * l), Kp, float(a.max()) * 2 / (l * l) if a.size else 0.0


def dot_ref(x1, x2, sigma):
    """(K, sigma^2 + sum_d |x1_id x2_jd|), summed in coordinate order."""
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    K = np.zeros((x1.shape[0], x2.shape[0]))
    A = np.zeros_like(K)
    for c in range(x1.shape[1]):
        t = x1[:, c][:, None] * x2[:, c][None, :]
        K += t
        A += np.abs(t)
    return sigma * sigma + K, sigma * sigma + A


@functools.lru_cache(maxsize=None)
def inputs(n1, n2, D):
    """x1 (n1, D), x2 (n2, D) in (-h, h), h = 4.4 / sqrt(D), and the full weights W (n1, n2) in (-1, 1)."""
    half = 4.4 / np.sqrt(D)
    x1 = gen.unif(gen.SEED + 7 * n1 + D, n1 * D, -half, half).reshape(n1, D)
    x2 = gen.unif(gen.SEED + 13 * n2 + 3 * D + 1, n2 * D, -half, half).reshape(n2, D)
    W = gen.unif(gen.SEED + 11 * n1 + n2 + D, n1 * n2, -1.0, 1.0).reshape(n1, n2)
    for a in (x1, x2, W):
        a.setflags(write=False)
    return x1, x2, W


@functools.lru_cache(maxsize=16)
def per_reference(n1, n2, D):
    x1, x2, _ = inputs(n1, n2, D)
    ref = per_ref(dist(x1, x2), SIG, ELL, PER)
    assert ref[4] < COND_MAX, ref[4]  # the condition under which 1e-13 on K holds
    return ref


# ------------------------------------------------------------ device helpers
PRE3 = np.array([0.25, -0.5, 0.75])  # out3 / out1 are accumulated into


def kfill(ctx, ldk, n2):
    return ctx.put(np.full(ldk * n2, np.nan))


def kget(ctx, dK, ldk, n2):
    return ctx.get(dK, ldk * n2).reshape(n2, ldk).T  # (ldk, n2): column j of K at [:, j]


def per_fwd(ctx, x1, x2, ldk, sigma=SIG, l=ELL, p=PER):
    n1, D = x1.shape
    n2 = x2.shape[0]
    dK = kfill(ctx, ldk, n2)
    rc = ctx.lib.smg_gp_periodic_cov_fwd(ctx.ptr, ctx.put(x1.ravel()), n1, ctx.put(x2.ravel()), n2, D, sigma, l, p, dK,
                                         ldk)
    assert rc == 0
    return kget(ctx, dK, ldk, n2)


def dot_fwd(ctx, x1, x2, ldk, sigma=SIG):
    n1, D = x1.shape
    n2 = x2.shape[0]
    dK = kfill(ctx, ldk, n2)
    rc = ctx.lib.smg_gp_dot_prod_cov_fwd(ctx.ptr, ctx.put(x1.ravel()), n1, ctx.put(x2.ravel()), n2, D, sigma, dK, ldk)
    assert rc == 0
    return kget(ctx, dK, ldk, n2)


def padded(W, ld):
    """W in a leading dimension ld, the padding rows NaN: a read of them shows in the sums."""
    A = np.full((ld, W.shape[1]), np.nan)
    A[:W.shape[0]] = W
    return F(A)


def per_rev(ctx, x1, x2, W, ldka, sigma=SIG, l=ELL, p=PER):
    """out3 after the call, pre-filled with PRE3."""
    n1, D = x1.shape
    n2 = x2.shape[0]
    out = ctx.put(PRE3)
    rc = ctx.lib.smg_gp_periodic_cov_rev(ctx.ptr, ctx.put(x1.ravel()), n1, ctx.put(x2.ravel()), n2, D, sigma, l, p,
                                         ctx.put(padded(W, ldka)), ldka, out)
    assert rc == 0
    return ctx.get(out, 3)


def dot_rev(ctx, W, ldka, sigma=SIG):
    n1, n2 = W.shape
    out = ctx.put(PRE3[:1])
    rc = ctx.lib.smg_gp_dot_prod_cov_rev(ctx.ptr, n1, n2, sigma, ctx.put(padded(W, ldka)), ldka, out)
    assert rc == 0
    return ctx.get(out, 1)


# (n1, n2, ldk), D = 1: odd sizes; the 16-byte form; the generic form by an odd
# ld and by an odd n1; rows split over blockIdx.y; more columns than GP_BLOCKS
SCALAR = [(33, 20, 33), (300, 257, 300), (300, 257, 301), (299, 20, 299), (5000, 3, 5000), (3, 2100, 3)]
POINTS = [(33, 20, 3), (300, 257, 5)]


# ---------------------------------------------------------- 1. periodic forward
def check_per_fwd(ctx, n1, n2, D, ldk):
    x1, x2, _ = inputs(n1, n2, D)
    K, _, _, _, cond = per_reference(n1, n2, D)
    out = per_fwd(ctx, x1, x2, ldk)
    rel = near_rel(out[:n1], K, 1e-13, atol=1e-300, what="K")
    print(f"periodic n1={n1} n2={n2} D={D} ldk={ldk}: condition {cond:.1f}, K rel {rel:.2e}")
    assert np.all(np.isnan(out[n1:]))  # the padding rows are not written


@gpu
@pytest.mark.parametrize("n1,n2,ldk", SCALAR)
def test_periodic_forward_scalar_points(ctx, n1, n2, ldk):
    """K at 1e-13 relative into a NaN-filled buffer."""
    check_per_fwd(ctx, n1, n2, 1, ldk)


@gpu
@pytest.mark.parametrize("n1,n2,D", POINTS)
def test_periodic_forward_points(ctx, n1, n2, D):
    """x2_j staged in LDS; (33, 20, 3) also with ldk = n1 + 3."""
    check_per_fwd(ctx, n1, n2, D, n1)
    if (n1, n2, D) == (33, 20, 3):
        check_per_fwd(ctx, n1, n2, D, n1 + 3)


# ---------------------------------------------------------- 2. periodic reverse
def check_per_rev(ctx, n1, n2, D, lds):
    x1, x2, W = inputs(n1, n2, D)
    _, Ks, Kl, Kp, _ = per_reference(n1, n2, D)
    ref = np.array([np.sum(W * M) for M in (Ks, Kl, Kp)])
    terms = np.array([np.sum(np.abs(W * M)) for M in (Ks, Kl, Kp)])
    for ld in lds:
        a = per_rev(ctx, x1, x2, W, ld)
        b = per_rev(ctx, x1, x2, W, ld)
        assert np.array_equal(a, b), (a, b)  # ordered sums: the same bits
        got = a - PRE3
        print(f"periodic reverse n1={n1} n2={n2} D={D} ldka={ld}: {got} (ref {ref}, term sums {terms}) "
              f"error / terms {np.abs(got - ref) / terms}")
        assert np.all(np.isfinite(a))  # (a padding row read would be NaN)
        assert np.all(np.abs(got - ref) <= 1e-11 * terms), (got, ref, terms)


@gpu
@pytest.mark.parametrize("n1,n2,ldk", SCALAR)
def test_periodic_reverse_scalar_points(ctx, n1, n2, ldk):
    """out3 += [d/dsigma, d/dl, d/dp] with a full adjoint, ldka = n1 and above
    (NaN padding), each entry within 1e-11 of the sum of its terms' absolute
    values; two runs give the same bits."""
    check_per_rev(ctx, n1, n2, 1, sorted({n1, ldk, n1 + 3}))


@gpu
@pytest.mark.parametrize("n1,n2,D", POINTS)
def test_periodic_reverse_points(ctx, n1, n2, D):
    check_per_rev(ctx, n1, n2, D, [n1, n1 + 3])


# ------------------------------------------------------------------ 3. x1 == x2
@gpu
@pytest.mark.parametrize("n,D", [(33, 1), (300, 1), (33, 5), (300, 5)])
def test_periodic_same_points(ctx, n, D):
    """K(x, x) equals its transpose bitwise and its diagonal is sigma * sigma bitwise."""
    x, _, _ = inputs(n, n, D)
    got = per_fwd(ctx, x, x, n)
    near_rel(got, per_ref(dist(x, x), SIG, ELL, PER)[0], 1e-13, atol=1e-300, what="K")
    assert np.array_equal(got, got.T)
    assert np.array_equal(np.diag(got), np.full(n, SIG * SIG))


@gpu
@pytest.mark.parametrize("D", [1, 3])
def test_periodic_whole_periods_apart(ctx, D):
    """x2 = x1 + 3 p in the first coordinate with p = 0.5, x1 on a 2^-20 grid so
    that the sum and the difference are exact: the pairs (i, i) are within
    1e-15 of sigma * sigma."""
    n = 33
    x1 = np.round(inputs(n, n, D)[0] * 2.0 ** 20) / 2.0 ** 20
    x2 = x1.copy()
    x2[:, 0] += 1.5
    assert np.array_equal(x2[:, 0] - x1[:, 0], np.full(n, 1.5))
    got = per_fwd(ctx, x1, x2, n, p=0.5)
    print(f"D={D}: max |K_ii - sigma^2| {np.abs(np.diag(got) - SIG * SIG).max():.2e}")
    assert np.all(np.abs(np.diag(got) - SIG * SIG) <= 1e-15)


# ------------------------------------------------------- 4. dot-product forward
DOT_SHAPES = [(n1, n2, 1, ldk) for n1, n2, ldk in SCALAR] + [(33, 20, 3, 33), (33, 20, 3, 36), (300, 257, 70, 300)]


@gpu
@pytest.mark.parametrize("n1,n2,D,ldk", DOT_SHAPES)
def test_dot_prod_forward(ctx, n1, n2, D, ldk):
    """|K - ref| <= 1e-13 (sigma^2 + sum_d |x1_id x2_jd|), the padding rows
    left NaN; sigma = 0 gives the plain dot products."""
    x1, x2, _ = inputs(n1, n2, D)
    for sigma in (SIG, 0.0):
        K, A = dot_ref(x1, x2, sigma)
        out = dot_fwd(ctx, x1, x2, ldk, sigma=sigma)
        err = np.abs(out[:n1] - K) / A
        print(f"dot product n1={n1} n2={n2} D={D} ldk={ldk} sigma={sigma}: max error / sum of terms {err.max():.2e}")
        assert np.all(np.abs(out[:n1] - K) <= 1e-13 * A)
        assert np.all(np.isnan(out[n1:]))
        if sigma == 0.0 and D == 1:
            assert np.array_equal(out[:n1], x1[:, 0][:, None] * x2[:, 0][None, :])


@gpu
def test_dot_prod_same_points(ctx):
    """x1 == x2 at (300, D = 5): bitwise symmetric."""
    x, _, _ = inputs(300, 300, 5)
    K, A = dot_ref(x, x, SIG)
    got = dot_fwd(ctx, x, x, 300)
    assert np.all(np.abs(got - K) <= 1e-13 * A)
    assert np.array_equal(got, got.T)


# ------------------------------------------------------- 5. dot-product reverse
@gpu
@pytest.mark.parametrize("n1,n2,ldk", SCALAR)
def test_dot_prod_reverse(ctx, n1, n2, ldk):
    """out1 += 2 sigma sum(Kadj) within 1e-12 2 sigma sum |Kadj|, the padding
    (NaN) not read, two runs the same bits; sigma = 0 adds exactly 0."""
    W = inputs(n1, n2, 1)[2]
    for ld in sorted({n1, ldk, n1 + 3}):
        a = dot_rev(ctx, W, ld)
        b = dot_rev(ctx, W, ld)
        assert np.array_equal(a, b), (a, b)
        got, ref, bound = a[0] - PRE3[0], 2 * SIG * np.sum(W), 1e-12 * 2 * SIG * np.sum(np.abs(W))
        print(f"dot product reverse n1={n1} n2={n2} ldka={ld}: {got!r} (ref {ref!r}), error {abs(got - ref):.2e} "
              f"bound {bound:.2e}")
        assert np.isfinite(a[0])
        assert abs(got - ref) <= bound
        assert np.array_equal(dot_rev(ctx, W, ld, sigma=0.0), PRE3[:1])


# ------------------------------------------------------------- 6. errors (ctypes)
@gpu
def test_entries_argument_errors(ctx):
    """Null ctx / points / matrix / output, D < 1, D > 8192, a negative size,
    ld < n1: SMG_ERR_ARG, the context's status untouched; a zero size is a
    no-op that leaves K and `out` alone."""
    n1, n2 = 8, 5
    x1, x2, _ = inputs(33, 20, 1)
    d1, d2 = ctx.put(x1[:n1].ravel()), ctx.put(x2[:n2].ravel())
    dK, o = ctx.zeros(n1 * n2), ctx.put(np.array([3.0, -4.0, 5.0]))
    L = ctx.lib
    pf, pr = L.smg_gp_periodic_cov_fwd, L.smg_gp_periodic_cov_rev
    df, dr = L.smg_gp_dot_prod_cov_fwd, L.smg_gp_dot_prod_cov_rev
    E = SMG_ERR_ARG
    assert pf(None, d1, n1, d2, n2, 1, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, None, n1, d2, n2, 1, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, d1, n1, None, n2, 1, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, d1, n1, d2, n2, 1, SIG, ELL, PER, None, n1) == E
    assert pf(ctx.ptr, d1, n1, d2, n2, 0, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, d1, n1, d2, n2, 8193, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, d1, -1, d2, n2, 1, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, d1, n1, d2, -1, 1, SIG, ELL, PER, dK, n1) == E
    assert pf(ctx.ptr, d1, n1, d2, n2, 1, SIG, ELL, PER, dK, n1 - 1) == E
    assert pr(None, d1, n1, d2, n2, 1, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, None, n1, d2, n2, 1, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, d1, n1, None, n2, 1, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, d1, n1, d2, n2, 1, SIG, ELL, PER, None, n1, o) == E
    assert pr(ctx.ptr, d1, n1, d2, n2, 1, SIG, ELL, PER, dK, n1, None) == E
    assert pr(ctx.ptr, d1, n1, d2, n2, 0, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, d1, n1, d2, n2, 8193, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, d1, -1, d2, n2, 1, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, d1, n1, d2, -1, 1, SIG, ELL, PER, dK, n1, o) == E
    assert pr(ctx.ptr, d1, n1, d2, n2, 1, SIG, ELL, PER, dK, n1 - 1, o) == E
    assert df(None, d1, n1, d2, n2, 1, SIG, dK, n1) == E
    assert df(ctx.ptr, None, n1, d2, n2, 1, SIG, dK, n1) == E
    assert df(ctx.ptr, d1, n1, None, n2, 1, SIG, dK, n1) == E
    assert df(ctx.ptr, d1, n1, d2, n2, 1, SIG, None, n1) == E
    assert df(ctx.ptr, d1, n1, d2, n2, 0, SIG, dK, n1) == E
    assert df(ctx.ptr, d1, n1, d2, n2, 8193, SIG, dK, n1) == E
    assert df(ctx.ptr, d1, -1, d2, n2, 1, SIG, dK, n1) == E
    assert df(ctx.ptr, d1, n1, d2, -1, 1, SIG, dK, n1) == E
    assert df(ctx.ptr, d1, n1, d2, n2, 1, SIG, dK, n1 - 1) == E
    assert dr(None, n1, n2, SIG, dK, n1, o) == E
    assert dr(ctx.ptr, n1, n2, SIG, None, n1, o) == E
    assert dr(ctx.ptr, n1, n2, SIG, dK, n1, None) == E
    assert dr(ctx.ptr, -1, n2, SIG, dK, n1, o) == E
    assert dr(ctx.ptr, n1, -1, SIG, dK, n1, o) == E
    assert dr(ctx.ptr, n1, n2, SIG, dK, n1 - 1, o) == E
    for a, b in ((0, n2), (n1, 0), (0, 0)):
        assert pf(ctx.ptr, d1, a, d2, b, 1, SIG, ELL, PER, dK, n1) == 0
        assert pr(ctx.ptr, d1, a, d2, b, 1, SIG, ELL, PER, dK, n1, o) == 0
        assert df(ctx.ptr, d1, a, d2, b, 1, SIG, dK, n1) == 0
        assert dr(ctx.ptr, a, b, SIG, dK, n1, o) == 0
    assert pf(ctx.ptr, None, 0, None, 0, 1, SIG, ELL, PER, None, 0) == 0
    assert pr(ctx.ptr, None, 0, None, 0, 1, SIG, ELL, PER, None, 0, None) == 0
    assert df(ctx.ptr, None, 0, None, 0, 1, SIG, None, 0) == 0
    assert dr(ctx.ptr, 0, 0, SIG, None, 0, None) == 0
    assert ctx.status() == 0
    assert np.array_equal(ctx.get(o, 3), [3.0, -4.0, 5.0])
    assert np.array_equal(ctx.get(dK, n1 * n2), np.zeros(n1 * n2))


# ---------------------------------------------------- end to end through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_periodic")


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def nums(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def rows_of(out, count=2):
    lines = out.strip().splitlines()
    assert lines[-1] == "stack 0 0", lines[-1]
    rows = [np.array([float(v) for v in l.split()]) for l in lines[:-1]]
    assert len(rows) == count
    return rows


# ---------------------------------------------------------------- 7. bilinear form
@functools.lru_cache(maxsize=None)
def bilinear_inputs(n1, n2):
    """U (3, n1) and V (n2, 2) with entries in (0.25, 1): u and v are positive,
    and so are K, dK/dsigma and dK/dl of the periodic kernel."""
    U = gen.unif(gen.SEED + 17 * n1 + 1, 3 * n1, 0.25, 1.0).reshape(3, n1)
    V = gen.unif(gen.SEED + 19 * n2 + 2, n2 * 2, 0.25, 1.0).reshape(n2, 2)
    U.setflags(write=False)
    V.setflags(write=False)
    return U, V


def bilinear(fn, n1, n2, D, kinds, form):
    """f = sum(U K V) = u^T K v with u = U^T 1, v = V 1, twice.  form 0: K(x1, x2)
    over host points; 2: device-resident scalar points; 3: the single-x overload."""
    x1, x2, _ = inputs(n1, n2, D)
    if form == 3:
        x2 = x1
    U, V = bilinear_inputs(n1, n2)
    u, v = U.sum(axis=0), V.sum(axis=1)
    if fn == "per":
        K, Ks, Kl, Kp, cond = per_ref(dist(x1, x2), SIG, ELL, PER)
        assert cond < COND_MAX, cond
        full = np.array([u @ M @ v for M in (Ks, Kl, Kp)])
        # sigma and l have no cancellation (u, v, K, dK/dl >= 0); p is bounded by its terms
        atol = np.array([0.0, 0.0, 1e-10 * (u @ np.abs(Kp) @ v)])
        keep = [i for i in range(3) if kinds[i] == "v"]
    else:
        K = dot_ref(x1, x2, SIG)[0]
        full, atol, keep = np.array([2 * SIG * u.sum() * v.sum()]), np.array([0.0]), [0]
    fx = u @ K @ v
    xs = f"{nums(x1)}\n" if form == 3 else f"{nums(x1)}\n{nums(x2)}\n"
    out = _run(f"bilinear {fn} {kinds} {form} {D} {n1} {n2} {SIG!r} {ELL!r} {PER!r}\n{xs}{nums(F(U))}\n{nums(F(V))}\n")
    for row in rows_of(out):  # the gradient taken twice
        print(f"{fn} {n1}x{n2} D={D} {kinds} form {form}: {row} (ref {fx!r} {full[keep]})")
        assert row.size == 1 + len(keep), row
        near_rel(row[0], fx, 1e-12, what="fx")
        for k, i in enumerate(keep):
            near_rel(row[1 + k], full[i], 1e-10, atol=atol[i], what=f"grad[{i}]")


KINDS = ["vvv", "vvd", "vdv", "dvv", "vdd", "dvd", "ddv"]


@gpu
@pytest.mark.parametrize("kinds", KINDS)
def test_periodic_bilinear_every_kind(kinds):
    """Every var / double combination of (sigma, l, p) at (33, 20, 1): the
    gradient has entries for the var arguments alone."""
    bilinear("per", 33, 20, 1, kinds, 0)


@gpu
@pytest.mark.parametrize("n1,n2,D,form", [(300, 257, 1, 0), (33, 20, 3, 0), (33, 20, 1, 2), (33, 33, 1, 3),
                                          (33, 33, 3, 3)])
@pytest.mark.parametrize("fn,kinds", [("per", "vvv"), ("dot", "v")])
def test_bilinear_form_through_tape(fn, kinds, n1, n2, D, form):
    """A larger K, Eigen points, device-resident points and the single-x
    overloads of both functions."""
    bilinear(fn, n1, n2, D, kinds, form)


@gpu
def test_dot_prod_bilinear_small():
    bilinear("dot", 33, 20, 1, "v", 0)


# ------------------------------------------------------ 8. GP marginal likelihood
THETA = (1.3, 0.7, 1.7, 0.5)  # sigma, l, p, noise
SIG_DOT = 0.8


@functools.lru_cache(maxsize=None)
def marginal_inputs(N):
    rng = np.random.default_rng(4000 + N)
    x = rng.uniform(-10, 10, N)
    y = rng.standard_normal(N)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def marginal_parts(kernel, N, th):
    """(Kd, [dKd/dtheta_i]) for theta = (sigma, l, p, noise[, sigma_dot])."""
    x, _ = marginal_inputs(N)
    K, Ks, Kl, Kp, _ = per_ref(dist(x[:, None], x[:, None]), th[0], th[1], th[2])
    Kd = K + th[3] * th[3] * np.eye(N)
    dK = [Ks, Kl, Kp, 2 * th[3] * np.eye(N)]
    if kernel == "sum":
        Kd = Kd + dot_ref(x[:, None], x[:, None], th[4])[0]
        dK.append(np.full((N, N), 2 * th[4]))
    return Kd, dK


def marginal_value(kernel, N, th):
    _, y = marginal_inputs(N)
    Kd, _ = marginal_parts(kernel, N, th)
    Lc = np.linalg.cholesky(Kd)
    return -0.5 * y @ np.linalg.solve(Kd, y) - np.log(np.diag(Lc)).sum() - 0.5 * N * np.log(2 * np.pi)


def theta_of(kernel):
    return np.array(THETA + ((SIG_DOT,) if kernel == "sum" else ()))


@functools.lru_cache(maxsize=None)
def marginal_ref(kernel, N):
    """(f, grad, the gradient entries' scales): f = -y^T alpha / 2 - log det Kd
    / 2 - N log(2 pi) / 2, df/dtheta = sum_ij (alpha alpha^T - Kd^-1)_ij
    dKd_ij/dtheta / 2; the scales are the sums of the absolute terms, what the
    tolerances' absolute parts are multiples of."""
    _, y = marginal_inputs(N)
    Kd, dK = marginal_parts(kernel, N, theta_of(kernel))
    alpha = np.linalg.solve(Kd, y)
    G = np.outer(alpha, alpha) - np.linalg.inv(Kd)
    g = np.array([0.5 * np.sum(G * M) for M in dK])
    gs = np.array([0.5 * np.sum(np.abs(G * M)) for M in dK])
    return marginal_value(kernel, N, theta_of(kernel)), g, gs


MARGINAL = [("per", 64), ("per", 301), ("sum", 64)]


@pytest.mark.parametrize("kernel,N", MARGINAL)
def test_marginal_reference_against_differences(kernel, N):
    """No GPU: the numpy reference of the marginal-likelihood test against
    central differences (h = 1e-5) of its own value at 1e-6 -- the yardstick
    verified before the device is compared with it."""
    f, g, gs = marginal_ref(kernel, N)
    th = theta_of(kernel)
    h = 1e-5
    for i in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[i] += h
        tm[i] -= h
        fd = (marginal_value(kernel, N, tp) - marginal_value(kernel, N, tm)) / (2 * h)
        print(f"{kernel} N={N} theta[{i}]: closed form {g[i]!r} differences {fd!r} scale {gs[i]:.3e}")
        near_rel(g[i], fd, 1e-6, atol=1e-6 * gs[i], what=f"grad[{i}]")


@gpu
@pytest.mark.parametrize("kernel,N", MARGINAL)
def test_marginal_likelihood_through_tape(kernel, N):
    """f = multi_normal_cholesky_lpdf(y | 0, cholesky_decompose(add_diag(K,
    noise^2))) with K = gp_periodic_cov(x, sigma, l, p), and with the sum kernel
    K + gp_dot_prod_cov(x, sigma_dot): plain nodes, so the factorisation reads
    K's stored values and writes its dense adjoint.  fx at 1e-12, the gradient
    at 1e-10 with an absolute part of 1e-10 of the sum of its absolute terms."""
    x, y = marginal_inputs(N)
    f, g, gs = marginal_ref(kernel, N)
    out = _run(f"marginal {kernel} {N} {nums(theta_of(kernel))}\n{nums(x)}\n{nums(y)}\n")
    for row in rows_of(out):  # the gradient taken twice
        print(f"{kernel} N={N}: fx {row[0]!r} (ref {f!r}) grad {row[1:]} (ref {g}, scales {gs})")
        assert row.size == 1 + g.size
        near_rel(row[0], f, 1e-12, what="fx")
        for i in range(g.size):
            near_rel(row[1 + i], g[i], 1e-10, atol=1e-10 * gs[i], what=f"grad[{i}]")


# ------------------------------------------------------- 9. degenerate shapes
@gpu
@pytest.mark.parametrize("fn", ["per", "dot"])
def test_degenerate_shapes_through_tape(fn):
    """Points without coordinates are all coincident: K = sigma^2 everywhere,
    d/dsigma sum(K) = 2 n1 n2 sigma and zero l- and p-derivatives, over two
    sets (3 x 2) and over one (3 x 3); an empty set gives a matrix without
    entries: sum 0, gradient 0."""
    m = 3 if fn == "per" else 1
    rows = rows_of(_run(f"degenerate {fn}\n"), 4)
    zeros = [0.0] * (m - 1)
    near_rel(rows[0], [6 * SIG * SIG, 12 * SIG] + zeros, 1e-12, atol=0.0, what="no coordinates, two sets")
    near_rel(rows[1], [9 * SIG * SIG, 18 * SIG] + zeros, 1e-12, atol=0.0, what="no coordinates, one set")
    assert np.array_equal(rows[2], np.zeros(1 + m))
    assert np.array_equal(rows[3], np.zeros(1 + m))


@gpu
def test_cpp_argument_errors():
    """Exception types and messages: gp_periodic_cov checks sigma, l, p (> 0, a
    NaN fails, infinity passes) before the points (not NaN), gp_dot_prod_cov
    sigma (not NaN, >= 0, finite) before the points (not NaN, finite); two
    sets are checked as x1 then x2; the point sizes come last."""
    lines = _run("errors\n").strip().splitlines()
    assert lines[-1] == "stack 0 0"
    got = {}
    for line in lines[:-1]:
        fn, case, typ, msg = line.split("|", 3)
        assert (fn, case) not in got
        got[(fn, case)] = (typ, msg)
    none = ("none", "")
    sizes = ("invalid_argument", "squared_distance: size of v1 (2) and size of v2 (3) must match in size")
    P, Dt = "gp_periodic_cov", "gp_dot_prod_cov"
    pos = lambda name, v: ("domain_error", f"{P}: {name} is {v}, but must be > 0!")  # noqa: E731
    pnan = lambda name: ("domain_error", f"{P}: element of {name} is nan, but must not be nan!")  # noqa: E731
    sd, ls, pe = "signal standard deviation", "length-scale", "period"
    dom = lambda name, v, must: ("domain_error", f"{Dt}: {name} is {v}, but must {must}!")  # noqa: E731
    nn, ge, fi = "not be nan", "be >= 0", "be finite"
    want = {
        (P, "ok"): none,
        (P, "x1 empty"): none,
        (P, "x2 empty"): none,
        (P, "sigma=0"): pos(sd, 0),
        (P, "sigma=-1"): pos(sd, -1),
        (P, "sigma=nan"): pos(sd, "nan"),
        (P, "sigma=inf"): none,
        (P, "l=0"): pos(ls, 0),
        (P, "l=-1"): pos(ls, -1),
        (P, "l=nan"): pos(ls, "nan"),
        (P, "l=inf"): none,
        (P, "p=0"): pos(pe, 0),
        (P, "p=-1"): pos(pe, -1),
        (P, "p=nan"): pos(pe, "nan"),
        (P, "p=inf"): none,
        (P, "sigma=0, l=0, p=0"): pos(sd, 0),
        (P, "l=0, p=0"): pos(ls, 0),
        (P, "x1 nan"): pnan("x1"),
        (P, "x2 nan"): pnan("x2"),
        (P, "x1 nan, x2 nan"): pnan("x1"),
        (P, "x1 nan, p=0"): pos(pe, 0),
        (P, "x2 nan, sigma=0"): pos(sd, 0),
        (P, "dvv l=0"): pos(ls, 0),
        (P, "vdd sigma=0"): pos(sd, 0),
        (P, "ddv sigma=0"): pos(sd, 0),
        (P, "ddv p=0"): pos(pe, 0),
        (P, "single ok"): none,
        (P, "single empty"): none,
        (P, "single x nan"): pnan("x"),
        (P, "single x nan, l=0"): pos(ls, 0),
        (P, "single p=inf"): none,
        (P, "points ok"): none,
        (P, "points x1 nan"): pnan("x1"),
        (P, "points x2 nan"): pnan("x2"),
        (P, "points x1 nan, x2 nan"): pnan("x1"),
        (P, "points sigma=0"): pos(sd, 0),
        (P, "points x2 nan, p=0"): pos(pe, 0),
        (P, "points sizes across"): sizes,
        (P, "points sizes within x1"): sizes,
        (P, "points sizes across, l=0"): pos(ls, 0),
        (P, "points sizes across, x1 nan"): pnan("x1"),
        (P, "single points ok"): none,
        (P, "single points x nan"): pnan("x"),
        (P, "single points sizes"): sizes,
        (Dt, "ok"): none,
        (Dt, "x1 empty"): none,
        (Dt, "x2 empty"): none,
        (Dt, "sigma=0"): none,
        (Dt, "sigma=-1"): dom("sigma", -1, ge),
        (Dt, "sigma=nan"): dom("sigma", "nan", nn),
        (Dt, "sigma=inf"): dom("sigma", "inf", fi),
        (Dt, "sigma=-inf"): dom("sigma", "-inf", ge),
        (Dt, "x1 nan"): dom("x1", "nan", nn),
        (Dt, "x2 nan"): dom("x2", "nan", nn),
        (Dt, "x1 inf"): dom("x1", "inf", fi),
        (Dt, "x2 inf"): dom("x2", "-inf", fi),
        (Dt, "x1 inf then nan"): dom("x1", "inf", fi),
        (Dt, "x1 inf, x2 nan"): dom("x1", "inf", fi),
        (Dt, "x1 nan, sigma=-1"): dom("sigma", -1, ge),
        (Dt, "x2 inf, sigma=inf"): dom("sigma", "inf", fi),
        (Dt, "single ok"): none,
        (Dt, "single empty"): none,
        (Dt, "single sigma=0"): none,
        (Dt, "single x nan"): dom("x", "nan", nn),
        (Dt, "single x inf"): dom("x", "inf", fi),
        (Dt, "single x nan, sigma=nan"): dom("sigma", "nan", nn),
        (Dt, "points ok"): none,
        (Dt, "points x1 nan"): dom("x1", "nan", nn),
        (Dt, "points x2 nan"): dom("x2", "nan", nn),
        (Dt, "points x1 inf"): dom("x1", "inf", fi),
        (Dt, "points x1 inf, x2 nan"): dom("x1", "inf", fi),
        (Dt, "points sigma=-1"): dom("sigma", -1, ge),
        (Dt, "points sizes across"): sizes,
        (Dt, "points sizes within x1"): sizes,
        (Dt, "points sizes across, sigma=-1"): dom("sigma", -1, ge),
        (Dt, "single points ok"): none,
        (Dt, "single points x inf"): dom("x", "inf", fi),
        (Dt, "single points sizes"): sizes,
    }
    for key, w in want.items():
        assert got[key] == w, (key, got[key], w)
    assert len(got) == len(want)
