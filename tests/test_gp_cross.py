"""The GP cross-covariance K(x1, x2) of the four covariance families:
smg_gp_cross_cov_fwd / smg_gp_cross_cov_rev / smg_gp_ard_cross_cov_rev through
ctypes, and the (x1, x2, sigma, length_scale) overloads of gp_exp_quad_cov /
gp_exponential_cov / gp_matern32_cov / gp_matern52_cov through the tape
(tests/cpp/test_gp_cross.cpp).

The reference of every test is float64 numpy written from gp_family.h's table.
With d = |x1_i - x2_j| (D == 1) or the square root of the squared distance
summed in coordinate order, every position alike (a rectangle has no diagonal):

    exp_quad     K = s2 exp(-d^2 / (2 l^2))                          dK/dl = K d^2 / l^3
    exponential  K = s2 exp(-d / l)                                  dK/dl = K d / l^2
    matern32     K = s2 (1 + a) exp(-a),           a = sqrt(3) d / l  dK/dl = s2 a^2 exp(-a) / l
    matern52     K = s2 (1 + a + a^2 / 3) exp(-a), a = sqrt(5) d / l  dK/dl = s2 a^2 (1 + a) exp(-a) / (3 l)

and dK/dsigma = 2 K / sigma.  ARD: z = x / l first, t_d = z1_id - z2_jd, r^2 =
sum_d t_d^2, a = c r, dK_ij/dl_d = s2 h t_d^2 / l_d with h = exp(-r^2 / 2) |
exp(-a) / a (0 at a = 0) | 3 exp(-a) | (5/3)(1 + a) exp(-a).

Tolerances (tests/test_gp_families.py's and test_gp_ard.py's): K at 1e-13
relative where the exponent's argument (a, or d^2 / (2 l^2) for exp_quad) stays
below 60 -- the points are drawn from (-h, h) with h = 4.4 / sqrt(D), which
bounds it by 4 * 4.4^2 / (2 * 0.9^2) = 47.8 for every family, shape and the ARD
scales used, and every reference asserts the bound -- hyperparameter adjoints
at 1e-11, x1 == x2 against the symmetric entries' reverse at 1e-12, the tape's
fx at 1e-12 and gradient at 1e-10.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gen
from _util import ROOT, near_rel, prebuilt

gpu = pytest.mark.gpu

FAMILIES = {"exp_quad": 0, "exponential": 1, "matern32": 2, "matern52": 3}
COEF = {"exp_quad": 1.0, "exponential": 1.0, "matern32": np.sqrt(3.0), "matern52": np.sqrt(5.0)}
NAMES = sorted(FAMILIES)
SIG, ELL = 1.3, 0.9
SMG_ERR_ARG = 16
ARG_MAX = 60.0


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


def hp(a):  # a host array's pointer (the caller keeps `a` alive)
    return ctypes.c_void_p(a.ctypes.data)


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


def cov_ref(family, d, sigma, l):
    """(K, dK/dsigma, dK/dl, the largest exponent argument) from the table, every position alike."""
    s2 = sigma * sigma
    if family == "exp_quad":
        a = d * d / (2 * l * l)
        K = s2 * np.exp(-a)
        Kl = K * d * d / (l * l * l)
    elif family == "exponential":
        a = d / l
        e = np.exp(-a)
        K, Kl = s2 * e, s2 * e * d / (l * l)
    elif family == "matern32":
        a = np.sqrt(3.0) * d / l
        e = np.exp(-a)
        K, Kl = s2 * (1 + a) * e, s2 * a * a * e / l
    else:
        a = np.sqrt(5.0) * d / l
        e = np.exp(-a)
        K, Kl = s2 * (1 + a + a * a / 3) * e, s2 * a * a * (1 + a) * e / (3 * l)
    return K, 2 * K / sigma, Kl, float(a.max()) if a.size else 0.0


def ard_ref(family, x1, x2, l, sigma):
    """(K, dK/dsigma, [dK/dl_d], the largest exponent argument) for x1 (n1, D), x2 (n2, D), l (D,)."""
    l = np.asarray(l, dtype=np.float64)
    z1, z2 = np.asarray(x1, dtype=np.float64) / l, np.asarray(x2, dtype=np.float64) / l
    D = z1.shape[1]
    r2 = np.zeros((z1.shape[0], z2.shape[0]))
    T2 = []
    for d in range(D):
        t = z1[:, d][:, None] - z2[:, d][None, :]
        T2.append(t * t)
        r2 += t * t
    r = np.abs(z1[:, 0][:, None] - z2[:, 0][None, :]) if D == 1 else np.sqrt(r2)
    a = COEF[family] * r
    s2 = sigma * sigma
    with np.errstate(divide="ignore", invalid="ignore"):
        if family == "exp_quad":
            e = np.exp(-0.5 * r2)
            K, h, arg = s2 * e, e, 0.5 * r2
        elif family == "exponential":
            e = np.exp(-a)
            K, h, arg = s2 * e, np.where(a > 0, e / a, 0.0), a
        elif family == "matern32":
            e = np.exp(-a)
            K, h, arg = s2 * (1 + a) * e, 3.0 * e, a
        else:
            e = np.exp(-a)
            K, h, arg = s2 * (1 + a + a * a / 3) * e, (5.0 / 3.0) * (1 + a) * e, a
    Kl = [s2 * h * T2[d] / l[d] for d in range(D)]
    return K, 2 * K / sigma, Kl, float(arg.max())


def scales(D):
    return np.linspace(0.9, 2.0, D)


@functools.lru_cache(maxsize=None)
def inputs(n1, n2, D):
    """x1 (n1, D), x2 (n2, D) and the full weights W (n1, n2), shared by the families."""
    half = 4.4 / np.sqrt(D)
    x1 = gen.unif(gen.SEED + 7 * n1 + D, n1 * D, -half, half).reshape(n1, D)
    x2 = gen.unif(gen.SEED + 13 * n2 + 3 * D + 1, n2 * D, -half, half).reshape(n2, D)
    W = gen.unif(gen.SEED + 11 * n1 + n2 + D, n1 * n2, -1.0, 1.0).reshape(n1, n2)
    for a in (x1, x2, W):
        a.setflags(write=False)
    return x1, x2, W


@functools.lru_cache(maxsize=16)
def reference(family, n1, n2, D):
    x1, x2, _ = inputs(n1, n2, D)
    ref = cov_ref(family, dist(x1, x2), SIG, ELL)
    assert ref[3] < ARG_MAX, ref[3]  # the condition under which 1e-13 on K holds
    return ref


@functools.lru_cache(maxsize=8)
def ard_reference(family, n1, n2, D):
    x1, x2, _ = inputs(n1, n2, D)
    ref = ard_ref(family, x1, x2, scales(D), SIG)
    assert ref[3] < ARG_MAX, ref[3]
    return ref


# ------------------------------------------------------------ device helpers
PRE2 = np.array([0.25, -0.5])  # out2 is accumulated into


def cross_fwd(ctx, fam, x1, x2, ldk, sigma=SIG, l=ELL, fill=np.nan):
    n1, D = x1.shape
    n2 = x2.shape[0]
    dK = ctx.put(np.full(ldk * n2, fill))
    rc = ctx.lib.smg_gp_cross_cov_fwd(ctx.ptr, fam, ctx.put(x1.ravel()), n1, ctx.put(x2.ravel()), n2, D, sigma, l, dK,
                                      ldk)
    assert rc == 0
    return ctx.get(dK, ldk * n2).reshape(n2, ldk).T  # (ldk, n2): column j of K at [:, j]


def padded(W, ld):
    A = np.zeros((ld, W.shape[1]))
    A[:W.shape[0]] = W
    return F(A)


def cross_rev(ctx, fam, x1, x2, W, ldka, sigma=SIG, l=ELL, raw=False):
    n1, D = x1.shape
    n2 = x2.shape[0]
    out = ctx.put(PRE2)
    rc = ctx.lib.smg_gp_cross_cov_rev(ctx.ptr, fam, ctx.put(x1.ravel()), n1, ctx.put(x2.ravel()), n2, D, sigma, l,
                                      ctx.put(padded(W, ldka)), ldka, out)
    assert rc == 0
    got = ctx.get(out, 2)
    return got if raw else got - PRE2


def scale(ctx, x, l):
    """(device z point-major, device zt coordinate-major) of smg_gp_ard_scale."""
    n, D = x.shape
    dz, dzt = ctx.put(np.full(n * D, np.nan)), ctx.put(np.full(n * D, np.nan))
    l = np.ascontiguousarray(l, dtype=np.float64)
    assert ctx.lib.smg_gp_ard_scale(ctx.ptr, ctx.put(x.ravel()), D, n, hp(l), dz, dzt) == 0
    return dz, dzt


def ard_pre(D):
    return 0.25 * (1 + np.arange(1 + D)) * (-1.0) ** np.arange(1 + D)


def ard_cross_rev(ctx, fam, x1, x2, l, W, ldka, sigma=SIG, raw=False):
    """smg_gp_ard_cross_cov_rev's increment of an `out` pre-filled with non-zeros."""
    n1, D = x1.shape
    n2 = x2.shape[0]
    l = np.ascontiguousarray(l, dtype=np.float64)
    _, z1t = scale(ctx, x1, l)
    _, z2t = scale(ctx, x2, l)
    pre = ard_pre(D)
    out = ctx.put(pre)
    rc = ctx.lib.smg_gp_ard_cross_cov_rev(ctx.ptr, fam, z1t, n1, z2t, n2, D, sigma, hp(l), ctx.put(padded(W, ldka)),
                                          ldka, out)
    assert rc == 0
    got = ctx.get(out, 1 + D)
    return got if raw else got - pre


def check_fwd_rev(ctx, family, n1, n2, D, ldk):
    x1, x2, W = inputs(n1, n2, D)
    K, Ks, Kl, amax = reference(family, n1, n2, D)
    out = cross_fwd(ctx, FAMILIES[family], x1, x2, ldk, fill=-7.0)
    got = out[:n1]
    rel = near_rel(got, K, 1e-13, atol=1e-300, what="K")
    print(f"{family} n1={n1} n2={n2} D={D} ldk={ldk}: max arg {amax:.1f}, K rel {rel:.2e}")
    assert np.all(out[n1:] == -7.0)  # the padding rows are not written
    g = cross_rev(ctx, FAMILIES[family], x1, x2, W, ldk)
    ref = np.array([np.sum(W * Ks), np.sum(W * Kl)])
    print(f"  [dsigma, dl] {g} (ref {ref}) rel {near_rel(g, ref, 1e-11, what='[dsigma, dl]'):.2e}")


# ------------------------------------------------ 1. forward / reverse, scalar points
SCALAR = [(1, 1, 1), (1, 7, 1), (7, 1, 7), (33, 20, 33), (33, 20, 36), (300, 257, 300), (300, 257, 303),
          (5, 2050, 5), (2050, 5, 2050), (2050, 5, 2053)]


@gpu
@pytest.mark.parametrize("n1,n2,ldk", SCALAR)
@pytest.mark.parametrize("family", NAMES)
def test_cross_scalar_points(ctx, family, n1, n2, ldk):
    """Odd n1 and odd leading dimensions take the generic form, even ones the
    16-byte column form; ldk > n1 leaves the padding at its fill value; n2 =
    2050 > 2048 workgroups wraps the column loop, n1 = 2050 takes more than one
    pass of a workgroup's rows.  A full random adjoint, out2 pre-loaded."""
    check_fwd_rev(ctx, family, n1, n2, 1, ldk)


# ------------------------------------------------------ 2. D-dimensional points
POINTS = [(1, 3, 3), (33, 20, 3), (300, 7, 5), (7, 2051, 3), (64, 9, 200)]


@gpu
@pytest.mark.parametrize("n1,n2,D", POINTS)
@pytest.mark.parametrize("family", NAMES)
def test_cross_points(ctx, family, n1, n2, D):
    """x2_j staged in LDS; (33, 20, 3) also with ldk = n1 + 3."""
    check_fwd_rev(ctx, family, n1, n2, D, n1)
    if (n1, n2, D) == (33, 20, 3):
        check_fwd_rev(ctx, family, n1, n2, D, n1 + 3)


# ------------------------------------------------------------------ 3. x1 == x2
@gpu
@pytest.mark.parametrize("n,D", [(33, 1), (300, 1), (300, 5)])
@pytest.mark.parametrize("family", NAMES)
def test_same_points_is_the_symmetric_entry(ctx, family, n, D):
    """K(x, x) has the bits of smg_gp_cov_fwd, its diagonal included (every
    family gives exactly s2 at distance 0); the reverse with a full adjoint
    agrees with smg_gp_cov_rev at 1e-12 (the sums differ in order)."""
    fam = FAMILIES[family]
    x, _, _ = inputs(n, n, D)
    W = inputs(n, n, D)[2]
    dx = ctx.put(x.ravel())
    dK = ctx.put(np.full(n * n, np.nan))
    ctx.call("smg_gp_cov_fwd", fam, dx, D, n, SIG, ELL, dK, n)
    sym = ctx.get(dK, n * n).reshape(n, n).T
    got = cross_fwd(ctx, fam, x, x, n)
    assert np.array_equal(got, sym)
    assert np.array_equal(got, got.T)
    assert np.array_equal(np.diag(got), np.full(n, SIG * SIG))
    o = ctx.zeros(2)
    ctx.call("smg_gp_cov_rev", fam, dx, D, n, SIG, ELL, ctx.put(F(W)), n, o)
    g = cross_rev(ctx, fam, x, x, W, n)
    print(f"{family} n={n} D={D}: cross {g} symmetric {ctx.get(o, 2)}")
    near_rel(g, ctx.get(o, 2), 1e-12, what="[dsigma, dl] vs smg_gp_cov_rev")


# ------------------------------------------------------------ 4. coincident pair
@gpu
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("family", NAMES)
def test_coincident_pair(ctx, family, D):
    """x1[3] == x2[7]: that entry is exactly sigma^2; with all the weight on it
    dl is exactly zero and dsigma = 2 sigma; everything finite, the ARD reverse
    (exponential's h = exp(-a) / a) included."""
    fam = FAMILIES[family]
    n1, n2 = 33, 20
    x1, x2, W = inputs(n1, n2, D)
    x1 = x1.copy()
    x1[3] = x2[7]
    out = cross_fwd(ctx, fam, x1, x2, n1)
    assert out[3, 7] == SIG * SIG
    assert np.all(np.isfinite(out))
    K, Ks, Kl, amax = cov_ref(family, dist(x1, x2), SIG, ELL)
    assert amax < ARG_MAX
    near_rel(out, K, 1e-13, atol=1e-300, what="K")
    E = np.zeros((n1, n2))
    E[3, 7] = 1.0
    g = cross_rev(ctx, fam, x1, x2, E, n1)
    assert g[1] == 0.0 and np.isfinite(g[0])
    near_rel(g[0], 2 * SIG, 1e-13, what="dsigma of the pair")
    g = cross_rev(ctx, fam, x1, x2, W, n1)
    assert np.all(np.isfinite(g))
    near_rel(g, [np.sum(W * Ks), np.sum(W * Kl)], 1e-11, what="[dsigma, dl]")
    # ARD on the same points
    l = scales(D)
    g = ard_cross_rev(ctx, fam, x1, x2, l, E, n1)
    assert np.all(np.isfinite(g)) and np.all(g[1:] == 0.0)
    near_rel(g[0], 2 * SIG, 1e-13, what="ARD dsigma of the pair")
    Ka, Ksa, Kla, amax = ard_ref(family, x1, x2, l, SIG)
    assert amax < ARG_MAX
    g = ard_cross_rev(ctx, fam, x1, x2, l, W, n1)
    assert np.all(np.isfinite(g))
    near_rel(g, [np.sum(W * Ksa)] + [np.sum(W * k) for k in Kla], 1e-11, what="ARD [dsigma, dl_d]")


# ---------------------------------------------------------------- 5. determinism
@gpu
@pytest.mark.parametrize("family", NAMES)
def test_reverse_is_deterministic(ctx, family):
    """Two reverse calls on the same input give the same bits (ordered sums, no
    floating-point atomics): the dense entry in both forms, and ARD."""
    fam = FAMILIES[family]
    for n1, n2, ld in ((300, 257, 300), (300, 257, 303)):
        x1, x2, W = inputs(n1, n2, 1)
        a = cross_rev(ctx, fam, x1, x2, W, ld, raw=True)
        b = cross_rev(ctx, fam, x1, x2, W, ld, raw=True)
        assert np.array_equal(a, b), (a, b)
    x1, x2, W = inputs(300, 257, 7)
    a = cross_rev(ctx, fam, x1, x2, W, 300, raw=True)
    b = cross_rev(ctx, fam, x1, x2, W, 300, raw=True)
    assert np.array_equal(a, b), (a, b)
    a = ard_cross_rev(ctx, fam, x1, x2, scales(7), W, 300, raw=True)
    b = ard_cross_rev(ctx, fam, x1, x2, scales(7), W, 300, raw=True)
    assert np.array_equal(a, b), (a, b)


# ---------------------------------------------------------------- 6. ARD reverse
ARD_SHAPES = [(33, 20, 2), (33, 20, 4), (300, 257, 7), (64, 9, 16), (40, 33, 17), (20, 12, 64)]


@gpu
@pytest.mark.parametrize("n1,n2,D", ARD_SHAPES)
@pytest.mark.parametrize("family", NAMES)
def test_ard_cross_reverse(ctx, family, n1, n2, D):
    """Every padded-D register form (4, 8, 16), a second 16-coordinate pass
    (D = 17) and SMG_GP_ARD_MAX_D, against numpy's [dsigma, dl_1 .. dl_D]; the
    forward on the scaled points with l = 1 is the ARD K; with every l_d equal
    the l-sums add up to the scalar entry's dl."""
    fam = FAMILIES[family]
    x1, x2, W = inputs(n1, n2, D)
    l = scales(D)
    K, Ks, Kl, amax = ard_reference(family, n1, n2, D)
    z1, _ = scale(ctx, x1, l)
    z2, _ = scale(ctx, x2, l)
    dK = ctx.put(np.full(n1 * n2, np.nan))
    assert ctx.lib.smg_gp_cross_cov_fwd(ctx.ptr, fam, z1, n1, z2, n2, D, SIG, 1.0, dK, n1) == 0
    got = ctx.get(dK, n1 * n2).reshape(n2, n1).T
    print(f"{family} {n1}x{n2} D={D}: max arg {amax:.1f}, K rel {near_rel(got, K, 1e-13, atol=1e-300, what='K'):.2e}")
    g = ard_cross_rev(ctx, fam, x1, x2, l, W, n1)
    ref = np.array([np.sum(W * Ks)] + [np.sum(W * k) for k in Kl])
    print(f"  [dsigma, dl_d] rel {near_rel(g, ref, 1e-11, what='[dsigma, dl_d]'):.2e}")
    g = ard_cross_rev(ctx, fam, x1, x2, l, W, n1 + 3)  # a padded adjoint
    near_rel(g, ref, 1e-11, what="[dsigma, dl_d], ldka = n1 + 3")
    same = np.full(D, ELL)
    ga = ard_cross_rev(ctx, fam, x1, x2, same, W, n1)
    gs = cross_rev(ctx, fam, x1, x2, W, n1)
    near_rel(ga[0], gs[0], 1e-11, what="dsigma, equal length scales")
    near_rel(ga[1:].sum(), gs[1], 1e-11, what="sum_d dl_d against the scalar dl")


# ------------------------------------------------------------- 7. errors (ctypes)
@gpu
def test_cross_entries_argument_errors(ctx):
    """Unknown family, null ctx / points / matrix / output, D < 1, ld < n1:
    SMG_ERR_ARG, the context's status untouched; a zero size is a no-op that
    leaves `out` alone."""
    n1, n2 = 8, 5
    x1, x2, W = inputs(33, 20, 1)
    d1, d2 = ctx.put(x1[:n1].ravel()), ctx.put(x2[:n2].ravel())
    dK, o = ctx.zeros(n1 * n2), ctx.put(np.array([3.0, -4.0, 5.0]))
    l = np.array([ELL])
    L = ctx.lib
    fw, rv, ar = L.smg_gp_cross_cov_fwd, L.smg_gp_cross_cov_rev, L.smg_gp_ard_cross_cov_rev
    for fam in (-1, 4, 17):
        assert fw(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, hp(l), dK, n1, o) == SMG_ERR_ARG
    for fam in (0, 1, 2, 3):
        assert fw(None, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1) == SMG_ERR_ARG
        assert fw(ctx.ptr, fam, None, n1, d2, n2, 1, SIG, ELL, dK, n1) == SMG_ERR_ARG
        assert fw(ctx.ptr, fam, d1, n1, None, n2, 1, SIG, ELL, dK, n1) == SMG_ERR_ARG
        assert fw(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, None, n1) == SMG_ERR_ARG
        assert fw(ctx.ptr, fam, d1, n1, d2, n2, 0, SIG, ELL, dK, n1) == SMG_ERR_ARG
        assert fw(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1 - 1) == SMG_ERR_ARG
        assert rv(None, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, None, n1, d2, n2, 1, SIG, ELL, dK, n1, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, d1, n1, None, n2, 1, SIG, ELL, dK, n1, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, None, n1, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1, None) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, d1, n1, d2, n2, 0, SIG, ELL, dK, n1, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, ELL, dK, n1 - 1, o) == SMG_ERR_ARG
        assert ar(None, fam, d1, n1, d2, n2, 1, SIG, hp(l), dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, None, n1, d2, n2, 1, SIG, hp(l), dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, None, n2, 1, SIG, hp(l), dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, None, dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, hp(l), None, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, hp(l), dK, n1, None) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 0, SIG, hp(l), dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 65, SIG, hp(l), dK, n1, o) == SMG_ERR_ARG
        assert ar(ctx.ptr, fam, d1, n1, d2, n2, 1, SIG, hp(l), dK, n1 - 1, o) == SMG_ERR_ARG
        for a, b in ((0, n2), (n1, 0), (0, 0)):
            assert fw(ctx.ptr, fam, d1, a, d2, b, 1, SIG, ELL, dK, n1) == 0
            assert rv(ctx.ptr, fam, d1, a, d2, b, 1, SIG, ELL, dK, n1, o) == 0
            assert ar(ctx.ptr, fam, d1, a, d2, b, 1, SIG, hp(l), dK, n1, o) == 0
        assert fw(ctx.ptr, fam, None, 0, None, 0, 1, SIG, ELL, None, 0) == 0
        assert rv(ctx.ptr, fam, None, 0, None, 0, 1, SIG, ELL, None, 0, None) == 0
    assert ctx.status() == 0
    assert np.array_equal(ctx.get(o, 3), [3.0, -4.0, 5.0])
    assert np.array_equal(ctx.get(dK, n1 * n2), np.zeros(n1 * n2))


# ---------------------------------------------------- end to end through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_cross")
THETA = (1.3, 0.7, 0.5)


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def nums(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def rows_of(out):
    lines = out.strip().splitlines()
    assert lines[-1] == "stack 0 0", lines[-1]
    rows = [np.array([float(v) for v in l.split()]) for l in lines[:-1]]
    assert len(rows) == 2
    return rows


# ---------------------------------------------------------------- 8. bilinear form
@functools.lru_cache(maxsize=None)
def bilinear_inputs(n1, n2):
    """U (3, n1) and V (n2, 2) with entries in (0.25, 1): u, v, K and every
    derivative of K are positive, so no sum of the form u^T M v cancels and the
    plain relative bounds apply."""
    U = gen.unif(gen.SEED + 17 * n1 + 1, 3 * n1, 0.25, 1.0).reshape(3, n1)
    V = gen.unif(gen.SEED + 19 * n2 + 2, n2 * 2, 0.25, 1.0).reshape(n2, 2)
    U.setflags(write=False)
    V.setflags(write=False)
    return U, V


def check_bilinear(what, out, fx, full, keep):
    for row in rows_of(out):
        print(f"{what}: {row} (ref {fx!r} {full[keep]})")
        assert row.size == 1 + len(keep), row
        near_rel(row[0], fx, 1e-12, what="fx")
        near_rel(row[1:], full[keep], 1e-10, what="grad")


def bilinear_scalar_l(family, n1, n2, D, kinds, form):
    """form 0: host points (std::vector<double> for D == 1, Eigen vectors
    otherwise); form 2: device-resident scalar points (dev_data<double>)."""
    x1, x2, _ = inputs(n1, n2, D)
    U, V = bilinear_inputs(n1, n2)
    K, Ks, Kl, _ = reference(family, n1, n2, D)
    u, v = U.sum(axis=0), V.sum(axis=1)
    full = np.array([u @ Ks @ v, u @ Kl @ v])
    keep = {"vv": [0, 1], "dv": [1], "vd": [0]}[kinds]
    out = _run(f"bilinear {family} {kinds} {form} {D} {n1} {n2} {SIG!r} {ELL!r}\n{nums(x1)}\n{nums(x2)}\n"
               f"{nums(F(U))}\n{nums(F(V))}\n")
    check_bilinear(f"{family} {n1}x{n2} D={D} {kinds} form {form}", out, u @ K @ v, full, keep)


@gpu
@pytest.mark.parametrize("kinds", ["vv", "dv", "vd"])
@pytest.mark.parametrize("n1,n2,D", [(33, 20, 1), (300, 257, 1), (33, 20, 3)])
@pytest.mark.parametrize("family", NAMES)
def test_bilinear_form_through_tape(family, n1, n2, D, kinds):
    """f = sum(U K(x1, x2) V) = u^T K v with u = U^T 1, v = V 1: fx at 1e-12
    and the gradient at 1e-10, which has entries for the var arguments alone,
    twice."""
    bilinear_scalar_l(family, n1, n2, D, kinds, 0)


@gpu
@pytest.mark.parametrize("kinds", ["vv", "dv", "vd"])
@pytest.mark.parametrize("family", NAMES)
def test_bilinear_form_device_resident_points(family, kinds):
    """The same through the dev_data<double> overloads at (33, 20, 1)."""
    bilinear_scalar_l(family, 33, 20, 1, kinds, 2)


@gpu
@pytest.mark.parametrize("kinds", ["vv", "dv", "vd"])
@pytest.mark.parametrize("family", NAMES)
def test_bilinear_form_ard_through_tape(family, kinds):
    """The same with one length scale per dimension at (33, 20, 4)."""
    n1, n2, D = 33, 20, 4
    x1, x2, _ = inputs(n1, n2, D)
    U, V = bilinear_inputs(n1, n2)
    l = scales(D)
    K, Ks, Kl, _ = ard_reference(family, n1, n2, D)
    u, v = U.sum(axis=0), V.sum(axis=1)
    full = np.array([u @ M @ v for M in [Ks] + list(Kl)])
    keep = {"vv": list(range(1 + D)), "dv": list(range(1, 1 + D)), "vd": [0]}[kinds]
    out = _run(f"bilinear {family} {kinds} 1 {D} {n1} {n2} {SIG!r} {nums(l)}\n{nums(x1)}\n{nums(x2)}\n{nums(F(U))}\n"
               f"{nums(F(V))}\n")
    check_bilinear(f"{family} ARD {kinds}", out, u @ K @ v, full, keep)


# ----------------------------------------------------------- 9. GP posterior mean
@functools.lru_cache(maxsize=None)
def mean_inputs(N, m):
    rng = np.random.default_rng(1000 * m + N)
    x = rng.uniform(-10, 10, N)
    xs = rng.uniform(-10, 10, m)
    y = rng.standard_normal(N)
    w = rng.uniform(-1, 1, m)
    for a in (x, xs, y, w):
        a.setflags(write=False)
    return x, xs, y, w


def mean_value(family, N, m, th):
    x, xs, y, w = mean_inputs(N, m)
    K = cov_ref(family, dist(x[:, None], x[:, None]), th[0], th[1])[0]
    Ks = cov_ref(family, dist(xs[:, None], x[:, None]), th[0], th[1])[0]
    return w @ Ks @ np.linalg.solve(K + th[2] * th[2] * np.eye(N), y)


@functools.lru_cache(maxsize=None)
def mean_ref(family, N, m):
    """(f, grad, f's scale, the gradient entries' scales) of f = w^T Ks alpha,
    alpha = Kd^{-1} y:  df = w^T dKs alpha - w^T Ks Kd^{-1} dKd alpha.  The
    scales are the sums of the absolute values of the terms the results are
    sums of (f and its derivatives can cancel): what the tolerances' absolute
    parts are multiples of."""
    x, xs, y, w = mean_inputs(N, m)
    sigma, l, noise = THETA
    K, Kdsig, Kdl, _ = cov_ref(family, dist(x[:, None], x[:, None]), sigma, l)
    Ks, Ksdsig, Ksdl, _ = cov_ref(family, dist(xs[:, None], x[:, None]), sigma, l)
    Kd = K + noise * noise * np.eye(N)
    alpha = np.linalg.solve(Kd, y)
    mean = Ks @ alpha
    f = w @ mean
    g, gs = [], []
    for dKs, dKd in ((Ksdsig, Kdsig), (Ksdl, Kdl), (np.zeros_like(Ks), 2 * noise * np.eye(N))):
        a = dKs @ alpha
        b = Ks @ np.linalg.solve(Kd, dKd @ alpha)
        g.append(w @ (a - b))
        gs.append(np.abs(w) @ (np.abs(a) + np.abs(b)))
    return f, np.array(g), np.abs(w) @ np.abs(mean), np.array(gs)


MEAN_SIZES = [(64, 20), (301, 33)]


@pytest.mark.parametrize("N,m", MEAN_SIZES)
@pytest.mark.parametrize("family", NAMES)
def test_posterior_mean_reference_against_differences(family, N, m):
    """No GPU: the numpy reference of the posterior-mean test against central
    differences (h = 1e-5) of its own value at 1e-6 -- the yardstick verified."""
    f, g, fs, gs = mean_ref(family, N, m)
    near_rel(f, mean_value(family, N, m, np.array(THETA)), 1e-12, atol=1e-12 * fs, what="f")
    h = 1e-5
    for i in range(3):
        tp, tm = np.array(THETA), np.array(THETA)
        tp[i] += h
        tm[i] -= h
        fd = (mean_value(family, N, m, tp) - mean_value(family, N, m, tm)) / (2 * h)
        print(f"{family} N={N} m={m} theta[{i}]: closed form {g[i]!r} differences {fd!r}")
        near_rel(g[i], fd, 1e-6, atol=1e-6 * gs[i], what=f"grad[{i}]")


@gpu
@pytest.mark.parametrize("N,m", MEAN_SIZES)
@pytest.mark.parametrize("family", NAMES)
def test_posterior_mean_through_tape(family, N, m):
    """f = sum(w (K(xs, x) alpha)) with alpha = L^-T L^-1 y, L the factor of
    K(x, x) + noise^2 I: fx at 1e-12 and the gradient in (sigma, l, noise) at
    1e-10, each with an absolute part scaled by the sum of its terms' sizes."""
    x, xs, y, w = mean_inputs(N, m)
    f, g, fs, gs = mean_ref(family, N, m)
    out = _run(f"mean {family} {N} {m} {nums(THETA)}\n{nums(x)}\n{nums(xs)}\n{nums(y)}\n{nums(w)}\n")
    for row in rows_of(out):
        print(f"{family} N={N} m={m}: fx {row[0]!r} (ref {f!r}) grad {row[1:]} (ref {g})")
        assert row.size == 4
        near_rel(row[0], f, 1e-12, atol=1e-12 * fs, what="fx")
        for i in range(3):
            near_rel(row[1 + i], g[i], 1e-10, atol=1e-10 * gs[i], what=f"grad[{i}]")


# ------------------------------------------------------- degenerate shapes
@gpu
@pytest.mark.parametrize("family", NAMES)
def test_degenerate_shapes_through_tape(family):
    """Points without coordinates are all at distance 0: K = sigma^2
    everywhere, d/dsigma sum(K) = 2 n1 n2 sigma and a zero l-derivative, in the
    one-length-scale and the ARD form; an empty x1 gives a matrix without
    entries: sum 0, gradient 0."""
    lines = _run(f"degenerate {family}\n").strip().splitlines()
    assert lines[-1] == "stack 0 0", lines[-1]
    rows = [np.array([float(v) for v in l.split()]) for l in lines[:-1]]
    assert len(rows) == 3
    near_rel(rows[0], [6 * SIG * SIG, 12 * SIG, 0.0], 1e-12, atol=0.0, what="no coordinates")
    near_rel(rows[1], [6 * SIG * SIG, 12 * SIG], 1e-12, atol=0.0, what="no coordinates, ARD")
    assert np.array_equal(rows[2], [0.0, 0.0, 0.0])


# ---------------------------------------------------------------- 10. exceptions
@gpu
def test_cpp_argument_errors():
    """Exception types and messages of the four functions' (x1, x2) overloads:
    each function's single-x checks in their order, the points as x1 then x2."""
    lines = _run("errors\n").strip().splitlines()
    assert lines[-1] == "stack 0 0"
    got = {}
    for line in lines[:-1]:
        fn, case, typ, msg = line.split("|", 3)
        got[(fn, case)] = (typ, msg)
    none = ("none", "")
    sizes = ("invalid_argument", "squared_distance: size of v1 (2) and size of v2 (3) must match in size")
    for fn in ("gp_exp_quad_cov", "gp_exponential_cov", "gp_matern32_cov", "gp_matern52_cov"):
        eq = fn == "gp_exp_quad_cov"
        dom = lambda m: ("domain_error", f"{fn}: {m}")  # noqa: E731
        pos = lambda name, v: dom(f"{name} is {v}, but must be > 0!")  # noqa: E731
        fin = lambda name: none if eq else dom(f"{name} is inf, but must be finite!")  # noqa: E731
        nan = lambda name: dom(f"{name} is nan, but must not be nan!")  # noqa: E731
        sig_vv, l_vv = ("sigma", "length_scale") if eq else ("magnitude", "length scale")
        sig_dv, l_dv = ("marginal variance", "length-scale") if eq else ("magnitude", "length scale")
        inv = lambda m: ("invalid_argument", f"{fn}: {m}")  # noqa: E731
        want = {
            "ok": none,
            "x1 empty": none,
            "x2 empty": none,
            "x1 nan": nan("x1"),
            "x2 nan": nan("x2"),
            "x1 nan, x2 nan": nan("x1"),
            "x2 nan, sigma=0, l=0": nan("x2"),
            "sigma=0": pos(sig_vv, 0),
            "sigma=-1": pos(sig_vv, -1),
            "sigma=inf": fin(sig_vv),
            "l=0": pos(l_vv, 0),
            "l=-1": pos(l_vv, -1),
            "l=inf": fin(l_vv),
            "sigma=0, l=0": pos(sig_vv, 0),
            "dv sigma=0": pos(sig_dv, 0),
            "dv l=0": pos(l_dv, 0),
            "vd sigma=0": pos("magnitude", 0),
            "vd l=0": pos("length scale", 0),
            "points ok": none,
            "points x1 nan": nan("x1[3]" if eq else "x1"),
            "points x2 nan": nan("x2[2]" if eq else "x2"),
            "points x1 nan, x2 nan": nan("x1[3]" if eq else "x1"),
            "points sigma=0": pos(sig_vv, 0),
            "points l=inf": fin(l_vv),
            "points l=-1": pos(l_vv, -1),
            "points sizes across": sizes,
            "points sizes within x1": sizes,
            "points sizes across, l=0": pos(l_vv, 0),
            "points x2 nan, sigma=0": pos(sig_vv, 0) if eq else nan("x2"),
            "ard ok": none,
            "ard x1 empty": none,
            "ard x1 nan": nan("x1"),
            "ard x2 nan": nan("x2"),
            "ard x1 nan, x2 nan, sigma=0": nan("x1"),
            "ard sigma=0": pos("magnitude", 0),
            "ard sigma=inf": dom("magnitude is inf, but must be finite!"),
            "ard l2=0": pos("length scale[2]", 0),
            "ard l3=inf": dom("length scale[3] is inf, but must be finite!"),
            "ard l1=-1, l2=0": pos("length scale[1]", -1),
            "ard count": inv("x dimension (3) and number of length scales (2) must match in size"),
            "ard count 65": inv("x dimension (3) and number of length scales (65) must match in size"),
            "ard sizes across": sizes,
            "ard sizes across, count": inv("x dimension (3) and number of length scales (2) must match in size"),
        }
        for case, w in want.items():
            assert got[(fn, case)] == w, (fn, case, got[(fn, case)], w)
    assert len(got) == 4 * len(want)
