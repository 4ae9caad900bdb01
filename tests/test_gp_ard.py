"""One length scale per input dimension (ARD) for the GP covariances:
smg_gp_ard_scale (z and its coordinate-major copy zt) / smg_gp_ard_cov_rev /
smg_gp_ard_cov_inverse_adjoint through ctypes, and the std::vector length-scale overloads of gp_exp_quad_cov /
gp_exponential_cov / gp_matern32_cov / gp_matern52_cov through the tape
(tests/cpp/test_gp_ard.cpp).

The reference of every test is float64 numpy written from the table, z = x / l
first and then the differences of z (the device's order).  With t_d = z_id -
z_jd, r^2 = sum_d t_d^2 in coordinate order, a = c r, K_ii = sigma^2,
dK/dsigma = 2 K / sigma and, for i != j, dK_ij/dl_d = sigma^2 h t_d^2 / l_d:

    exp_quad     c = 1        K = s2 exp(-r^2 / 2)             h = exp(-r^2 / 2)
    exponential  c = 1        K = s2 exp(-a)                   h = exp(-a) / a   (0 at a = 0)
    matern32     c = sqrt 3   K = s2 (1 + a) exp(-a)           h = 3 exp(-a)
    matern52     c = sqrt 5   K = s2 (1 + a + a^2 / 3) exp(-a) h = (5/3)(1 + a) exp(-a)

Tolerances (tests/test_gp_families.py's): K at 1e-13 relative where max a < 60,
hyperparameter adjoints against numpy at 1e-11, the fused reducer against the
composition at 1e-12, the tape's fx at 1e-12 and gradient at 1e-10; equal
length scales against the scalar entries at 1e-12 (the two formulations round
differently: numpy alone shows up to 5.7e-14 on exp_quad's K).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import gen
from _util import ROOT, near_rel, prebuilt

pytestmark = pytest.mark.gpu

FAMILIES = {"exp_quad": 0, "exponential": 1, "matern32": 2, "matern52": 3}
COEF = {"exp_quad": 1.0, "exponential": 1.0, "matern32": np.sqrt(3.0), "matern52": np.sqrt(5.0)}
NAMES = sorted(FAMILIES)
SIG = 1.3
SMG_ERR_ARG = 16
MAX_D = 64


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
def ard_ref(family, x, l, sigma):
    """(K, dK/dsigma, [dK/dl_d], max a) from the table for x (n, D), l (D,)."""
    z = np.asarray(x, dtype=np.float64) / np.asarray(l, dtype=np.float64)
    n, D = z.shape
    r2 = np.zeros((n, n))
    T2 = []
    for d in range(D):
        t = z[:, d][:, None] - z[:, d][None, :]
        T2.append(t * t)
        r2 += t * t
    r = np.abs(z[:, 0][:, None] - z[:, 0][None, :]) if D == 1 else np.sqrt(r2)
    a = COEF[family] * r
    s2 = sigma * sigma
    with np.errstate(divide="ignore", invalid="ignore"):
        if family == "exp_quad":
            e = np.exp(-0.5 * r2)
            K, h = s2 * e, e
        elif family == "exponential":
            e = np.exp(-a)
            K, h = s2 * e, np.where(a > 0, e / a, 0.0)
        elif family == "matern32":
            e = np.exp(-a)
            K, h = s2 * (1 + a) * e, 3.0 * e
        else:
            e = np.exp(-a)
            K, h = s2 * (1 + a + a * a / 3) * e, (5.0 / 3.0) * (1 + a) * e
    K = K.copy()
    np.fill_diagonal(K, s2)
    Kl = []
    for d in range(D):
        g = s2 * h * T2[d] / l[d]
        np.fill_diagonal(g, 0.0)
        Kl.append(g)
    return K, 2 * K / sigma, Kl, float(a.max())


def ard_sums(G, Ks, Kl):
    return np.array([np.sum(G * Ks)] + [np.sum(G * g) for g in Kl])


def scales(D):
    return np.linspace(0.9, 2.0, D)


@functools.lru_cache(maxsize=None)
def inputs(n, D):
    """x (n, D) and the upper-triangle weights W, shared by the families."""
    half = 0.5 if D >= 40 else 5.0
    x = gen.unif(gen.SEED + 7 * n + D, n * D, -half, half).reshape(n, D)
    W = np.triu(gen.unif(gen.SEED + 11 * n + D, n * n, -1.0, 1.0).reshape(n, n))
    for a in (x, W):
        a.setflags(write=False)
    return x, W


@functools.lru_cache(maxsize=8)
def reference(family, n, D):
    x, _ = inputs(n, D)
    ref = ard_ref(family, x, scales(D), SIG)
    assert ref[3] < 60, ref[3]  # the condition under which 1e-13 on K holds
    return ref


# ------------------------------------------------------------ device helpers
def scale(ctx, x, l):
    """(device z, device zt, host z) of smg_gp_ard_scale, both pre-filled with
    NaN: z point-major (the forward's input), zt its coordinate-major copy
    (the reducers' input), which must hold the same bits."""
    n, D = x.shape
    dz, dzt = ctx.put(np.full(n * D, np.nan)), ctx.put(np.full(n * D, np.nan))
    l = np.ascontiguousarray(l, dtype=np.float64)
    assert ctx.lib.smg_gp_ard_scale(ctx.ptr, ctx.put(x.ravel()), D, n, hp(l), dz, dzt) == 0
    z = ctx.get(dz, n * D).reshape(n, D)
    assert np.array_equal(ctx.get(dzt, n * D).reshape(D, n), z.T)
    return dz, dzt, z


def fwd(ctx, fam, dz, n, D, ldk, sigma=SIG, l=1.0, fill=np.nan):
    dK = ctx.put(np.full(ldk * n, fill))
    assert ctx.lib.smg_gp_cov_fwd(ctx.ptr, fam, dz, D, n, sigma, l, dK, ldk) == 0
    return ctx.get(dK, ldk * n).reshape(n, ldk).T  # (ldk, n): column j of K at [:, j]


def ard_rev(ctx, fam, dzt, n, D, l, W, ldka, sigma=SIG):
    """smg_gp_ard_cov_rev's increment of an `out` pre-filled with non-zeros."""
    A = np.zeros((ldka, n))
    A[:n] = W
    pre = 0.25 * (1 + np.arange(1 + D)) * (-1.0) ** np.arange(1 + D)
    out = ctx.put(pre)
    l = np.ascontiguousarray(l, dtype=np.float64)
    rc = ctx.lib.smg_gp_ard_cov_rev(ctx.ptr, fam, dzt, D, n, sigma, hp(l), ctx.put(F(A)), ldka, out)
    assert rc == 0
    return ctx.get(out, 1 + D) - pre, ctx.get(out, 1 + D)


# (n, D, ld): 256 rows per pass, the 2048-workgroup cap, odd n (the unpaired
# middle column), D = 1, the 16-coordinate pass boundary, the D cap; one padded
# ld each for n = 300 and n = 2051
SHAPES = [(1, 3, 1), (2, 2, 2), (33, 3, 33), (257, 1, 257), (300, 5, 300), (300, 5, 303), (300, 16, 300),
          (300, 17, 300), (64, 40, 64), (64, 64, 64), (2051, 3, 2051), (2051, 3, 2053)]
NDS = sorted({(n, D) for n, D, _ in SHAPES})


# --------------------------------------------------------------- 1. scale, forward
@pytest.mark.parametrize("n,D,ld", SHAPES)
@pytest.mark.parametrize("family", NAMES)
def test_scale_and_forward(ctx, family, n, D, ld):
    """z is numpy's x / l bit for bit; the existing forward on z with l = 1 is
    the ARD covariance: the reference at 1e-13, symmetric, an exact diagonal."""
    x, _ = inputs(n, D)
    l = scales(D)
    K = reference(family, n, D)[0]
    dz, _, z = scale(ctx, x, l)
    assert np.array_equal(z, x / l)
    only = ctx.put(np.full(n * D, np.nan))  # zt is optional
    assert ctx.lib.smg_gp_ard_scale(ctx.ptr, ctx.put(x.ravel()), D, n, hp(l), only, None) == 0
    assert np.array_equal(ctx.get(only, n * D).reshape(n, D), z)
    out = fwd(ctx, FAMILIES[family], dz, n, D, ld, fill=-7.0)
    got = out[:n]
    print(f"{family} n={n} D={D} ld={ld}: K rel {near_rel(got, K, 1e-13, atol=1e-300, what='K'):.2e}")
    assert np.array_equal(got, got.T)
    assert np.array_equal(np.diag(got), np.full(n, SIG * SIG))
    assert np.all(out[n:] == -7.0)


# ----------------------------------------------------------------- 2. dense reverse
@pytest.mark.parametrize("n,D,ld", SHAPES)
@pytest.mark.parametrize("family", NAMES)
def test_dense_reverse(ctx, family, n, D, ld):
    """smg_gp_ard_cov_rev with an upper-triangular Kadj against numpy's 1 + D
    sums at 1e-11; `out` is accumulated into."""
    x, W = inputs(n, D)
    l = scales(D)
    _, Ks, Kl, _ = reference(family, n, D)
    _, dzt, _ = scale(ctx, x, l)
    g, _ = ard_rev(ctx, FAMILIES[family], dzt, n, D, l, W, ld)
    ref = ard_sums(W, Ks, Kl)
    print(f"{family} n={n} D={D} ld={ld}: [dsigma, dl] rel {near_rel(g, ref, 1e-11, what='[dsigma, dl..]'):.2e}")
    if n == 1:
        assert np.all(g[1:] == 0.0)


# ------------------------------------------- 3. fused reducer against composition
def _inverse_adjoint_inputs(N, D, k):  # tests/test_gp_families.py's recipe
    rng = np.random.default_rng(N * 7 + D + k)
    M = rng.uniform(-1, 1, (N, N))
    C = M @ M.T / N + np.eye(N)
    s = rng.uniform(-1, 1, (k, 2 * N))  # observation o's s at o * 2N (s_stride 2N)
    x = rng.uniform(-3, 3, (N, D))
    return C, s, x


def fused(ctx, fam, dC, N, ds, k, adj, dzt, D, sig, l, want_out=True):
    """[d', sigma', l'..] of smg_gp_ard_cov_inverse_adjoint, outputs pre-filled with NaN."""
    dd, o = ctx.put(np.array([np.nan])), ctx.put(np.full(1 + D, np.nan))
    if want_out:
        ctx.call("smg_gp_ard_cov_inverse_adjoint", fam, dC, N, N, ds, k, 2 * N, adj, dzt, D, sig, hp(l), dd, o)
        return np.concatenate([ctx.get(dd, 1), ctx.get(o, 1 + D)])
    ctx.call("smg_gp_ard_cov_inverse_adjoint", fam, dC, N, N, ds, k, 2 * N, adj, None, D, sig, None, dd, None)
    return ctx.get(dd, 1)


@pytest.mark.parametrize("N,D", NDS)
@pytest.mark.parametrize("family", NAMES)
def test_inverse_adjoint_vs_composition(ctx, family, N, D):
    """For k = 1, 2, 3: the fused entry against smg_cholesky_inverse_adjoint ->
    smg_add_diag_rev -> smg_gp_ard_cov_rev on the device at 1e-12 (d' alone
    with z, l and out NULL too), and against numpy from
    G = adj Phi(sum_o s_o s_o^T - k C) at 1e-11; outputs are written."""
    fam = FAMILIES[family]
    l = scales(D)
    sig, adj = 1.3, 0.8
    for k in (1, 2, 3):
        C, s, x = _inverse_adjoint_inputs(N, D, k)
        m = ctx.mark()
        dC, ds = ctx.put(F(C)), ctx.put(s.ravel())
        _, dzt, _ = scale(ctx, x, l)
        dKd, dKa, dd0, o0 = ctx.zeros(N * N), ctx.zeros(N * N), ctx.zeros(1), ctx.zeros(1 + D)
        ctx.call("smg_cholesky_inverse_adjoint", dC, N, N, ds, k, 2 * N, adj, dKd, N)
        ctx.call("smg_add_diag_rev", dKd, N, N, dKa, N, dd0, 0)
        ctx.call("smg_gp_ard_cov_rev", fam, dzt, D, N, sig, hp(l), dKa, N, o0)
        r0 = np.concatenate([ctx.get(dd0, 1), ctx.get(o0, 1 + D)])
        r1 = fused(ctx, fam, dC, N, ds, k, adj, dzt, D, sig, l)
        d2 = fused(ctx, fam, dC, N, ds, k, adj, dzt, D, sig, l, want_out=False)
        ctx.rewind(m)
        print(f"{family} N={N} D={D} k={k}: fused {r1[:4]} composition {r0[:4]}")
        near_rel(r1, r0, 1e-12, what="[d', sigma', l'..]")
        near_rel(d2, r0[:1], 1e-12, what="d' alone")
        S = sum(np.outer(s[o, :N], s[o, :N]) for o in range(k))
        G = adj * (S - k * C)
        G = np.tril(G, -1) + 0.5 * np.diag(np.diag(G))
        _, Ks, Kl, _ = ard_ref(family, x, l, sig)
        near_rel(r1[1:], ard_sums(G, Ks, Kl), 1e-11, what="[sigma', l'..] vs numpy")
        near_rel(r1[0], np.trace(G), 1e-11, what="d' vs numpy")


# ------------------------------------- 4. equal length scales: the scalar entries
@pytest.mark.parametrize("n,D", [(33, 3), (257, 1), (300, 5), (300, 17)])
@pytest.mark.parametrize("family", NAMES)
def test_equal_length_scales_match_scalar_entries(ctx, family, n, D):
    """l_d = 0.9 for every d: K is smg_gp_cov_fwd(x, l = 0.9)'s at 1e-12, the
    sum of the l_d' is smg_gp_cov_rev's l' and sigma' its sigma' at 1e-11."""
    fam = FAMILIES[family]
    x, W = inputs(n, D)
    l = np.full(D, 0.9)
    dz, dzt, _ = scale(ctx, x, l)
    K1 = fwd(ctx, fam, dz, n, D, n)
    K0 = fwd(ctx, fam, ctx.put(x.ravel()), n, D, n, l=0.9)
    print(f"{family} n={n} D={D}: K rel {near_rel(K1, K0, 1e-12, atol=1e-300, what='K'):.2e}")
    g, _ = ard_rev(ctx, fam, dzt, n, D, l, W, n)
    o = ctx.zeros(2)
    ctx.call("smg_gp_cov_rev", fam, ctx.put(x.ravel()), D, n, SIG, 0.9, ctx.put(F(W)), n, o)
    o = ctx.get(o, 2)
    near_rel(g[0], o[0], 1e-11, what="sigma'")
    near_rel(np.sum(g[1:]), o[1], 1e-11, what="sum of l_d' against l'")


# --------------------------------------------------- 5. coincident and far points
@pytest.mark.parametrize("n,D", [(33, 3), (257, 1), (300, 5)])
@pytest.mark.parametrize("family", NAMES)
def test_coincident_and_far_points(ctx, family, n, D):
    """Rows 3 and 7 equal (the exponential family's a = 0 guard), row 11 about
    1e3 length scales away from every other: K is exactly sigma^2 / exactly 0
    there, every output finite and the reference's."""
    fam = FAMILIES[family]
    l = scales(D)
    x = inputs(n, D)[0].copy()
    x[7] = x[3]
    x[11] = 1e3 * l + 20.0
    W = inputs(n, D)[1]
    K, Ks, Kl, _ = ard_ref(family, x, l, SIG)
    dz, dzt, z = scale(ctx, x, l)
    assert np.array_equal(z, x / l)
    out = fwd(ctx, fam, dz, n, D, n)
    assert out[7, 3] == SIG * SIG and out[3, 7] == SIG * SIG
    far = np.delete(np.arange(n), 11)
    assert np.all(out[11, far] == 0.0) and np.all(out[far, 11] == 0.0)
    assert np.all(np.isfinite(out)) and np.array_equal(out, out.T)
    near_rel(out, K, 1e-13, atol=1e-300, what="K")
    # all the weight on the coincident pair and on a far pair: every l_d' is exactly zero
    E = np.zeros((n, n))
    E[3, 7] = E[7, 3] = E[11, 2] = E[2, 11] = 1.0
    g, _ = ard_rev(ctx, fam, dzt, n, D, l, E, n)
    assert np.all(g[1:] == 0.0) and np.isfinite(g[0])
    near_rel(g[0], 4 * SIG, 1e-13, what="dsigma of the pairs")
    g, raw = ard_rev(ctx, fam, dzt, n, D, l, W, n)
    assert np.all(np.isfinite(raw))
    near_rel(g, ard_sums(W, Ks, Kl), 1e-11, what="[dsigma, dl..]")
    # the fused reducer over the same points
    C, s, _ = _inverse_adjoint_inputs(n, D, 2)
    r = fused(ctx, fam, ctx.put(F(C)), n, ctx.put(s.ravel()), 2, 0.8, dzt, D, SIG, l)
    assert np.all(np.isfinite(r))
    S = sum(np.outer(s[o, :n], s[o, :n]) for o in range(2))
    G = 0.8 * (S - 2 * C)
    G = np.tril(G, -1) + 0.5 * np.diag(np.diag(G))
    near_rel(r[1:], ard_sums(G, Ks, Kl), 1e-11, what="fused [sigma', l'..]")
    near_rel(r[0], np.trace(G), 1e-11, what="fused d'")


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("n,D", [(300, 5), (300, 17), (2051, 3)])
@pytest.mark.parametrize("family", NAMES)
def test_reducers_repeat_bitwise(ctx, family, n, D):
    """Two calls of each reducer give the same bits (ordered sums, no atomics)."""
    fam = FAMILIES[family]
    x, W = inputs(n, D)
    l = scales(D)
    _, dzt, _ = scale(ctx, x, l)
    a = ard_rev(ctx, fam, dzt, n, D, l, W, n)[1]
    b = ard_rev(ctx, fam, dzt, n, D, l, W, n)[1]
    assert np.array_equal(a, b)
    C, s, _ = _inverse_adjoint_inputs(n, D, 2)
    dC, ds = ctx.put(F(C)), ctx.put(s.ravel())
    a = fused(ctx, fam, dC, n, ds, 2, 0.8, dzt, D, SIG, l)
    b = fused(ctx, fam, dC, n, ds, 2, 0.8, dzt, D, SIG, l)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


# ------------------------------------------------------------ 7. errors (ctypes)
def test_ard_entries_argument_errors(ctx):
    """Null ctx or required pointer, n < 0, D < 1, D > 64, an unknown family,
    ld < n: SMG_ERR_ARG, the context's status untouched; n = 0 is a no-op."""
    n, D = 8, 3
    x, _ = inputs(33, 3)
    l = scales(D)
    big = np.full(MAX_D + 1, 1.0)
    dx, dz, dzt = ctx.put(x[:n].ravel()), ctx.zeros(n * D), ctx.zeros(n * D)
    dK, o, dd = ctx.zeros(n * n), ctx.zeros(2 + MAX_D), ctx.zeros(1)
    L = ctx.lib
    sc, rv, ia = L.smg_gp_ard_scale, L.smg_gp_ard_cov_rev, L.smg_gp_ard_cov_inverse_adjoint
    assert sc(None, dx, D, n, hp(l), dz, dzt) == SMG_ERR_ARG
    assert sc(ctx.ptr, None, D, n, hp(l), dz, dzt) == SMG_ERR_ARG
    assert sc(ctx.ptr, dx, D, n, None, dz, dzt) == SMG_ERR_ARG
    assert sc(ctx.ptr, dx, D, n, hp(l), None, None) == SMG_ERR_ARG
    assert sc(ctx.ptr, dx, D, -1, hp(l), dz, dzt) == SMG_ERR_ARG
    assert sc(ctx.ptr, dx, 0, n, hp(l), dz, dzt) == SMG_ERR_ARG
    assert sc(ctx.ptr, dx, MAX_D + 1, n, hp(big), dz, dzt) == SMG_ERR_ARG
    assert sc(ctx.ptr, None, D, 0, None, None, None) == 0
    for fam in (-1, 4, 17):
        assert rv(ctx.ptr, fam, dz, D, n, SIG, hp(l), dK, n, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dz, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
    for fam in (0, 1, 2, 3):
        assert rv(None, fam, dz, D, n, SIG, hp(l), dK, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, None, D, n, SIG, hp(l), dK, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, D, n, SIG, None, dK, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, D, n, SIG, hp(l), None, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, D, n, SIG, hp(l), dK, n, None) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, D, n, SIG, hp(l), dK, n - 1, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, D, -1, SIG, hp(l), dK, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, 0, n, SIG, hp(l), dK, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, dz, MAX_D + 1, n, SIG, hp(big), dK, n, o) == SMG_ERR_ARG
        assert rv(ctx.ptr, fam, None, D, 0, SIG, None, None, 0, None) == 0
        assert ia(None, fam, dK, n, n, dx, 1, n, 1.0, dz, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, None, n, n, dx, 1, n, 1.0, dz, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, None, 1, n, 1.0, dz, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, None, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dz, D, SIG, None, dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n - 1, n, dx, 1, n, 1.0, dz, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, -1, dx, 1, n, 1.0, dz, D, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dz, 0, SIG, hp(l), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dz, MAX_D + 1, SIG, hp(big), dd, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, None, 0, 0, None, 1, 0, 1.0, None, D, SIG, None, None, None) == 0
    assert ctx.status() == 0
    assert np.all(ctx.get(dz, n * D) == 0.0) and np.all(ctx.get(dzt, n * D) == 0.0)
    assert np.all(ctx.get(o, 2 + MAX_D) == 0.0) and ctx.get(dd, 1)[0] == 0.0  # nothing was written


# ---------------------------------------------------- 8. end to end through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_ard")
TSIG, NOISE = 1.3, 0.5


def tape_scales(D):
    return np.linspace(0.7, 2.1, D)


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _nums(a):
    return " ".join(repr(float(v)) for v in np.asarray(a).ravel())


@functools.lru_cache(maxsize=None)
def tape_inputs(N, D):
    rng = np.random.default_rng(1000 * D + N)
    x = rng.uniform(-10, 10, (N, D))
    y = rng.standard_normal(N)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def tape_run(family, N, D, mixed, kinds, deferred=True):
    """(the rows [fx, gradient...] of the program's two evaluations, materialisation count)."""
    x, y = tape_inputs(N, D)
    head = f"grad {family} {int(mixed)} {kinds} {int(deferred)} {D} {N} {TSIG!r} {_nums(tape_scales(D))} {NOISE!r}"
    out = _run(head + "\n" + _nums(x) + "\n" + _nums(y) + "\n")
    lines = out.strip().splitlines()
    assert lines[-1] == "stack 0 0", lines[-1]
    assert lines[-2].startswith("materialised "), lines[-2]
    rows = [np.array([float(v) for v in l.split()]) for l in lines[:-2]]
    assert len(rows) == 2
    return rows, int(lines[-2].split()[1])


@functools.lru_cache(maxsize=None)
def marginal_ref(family, N, D):
    """(fx, [dsigma, dl_1..dl_D, dnoise], sum(L)) of the GP marginal in numpy:
    G = (alpha alpha^T - Kd^{-1}) / 2 against the table's derivatives."""
    x, y = tape_inputs(N, D)
    K, Ks, Kl, _ = ard_ref(family, x, tape_scales(D), TSIG)
    Kd = K + NOISE * NOISE * np.eye(N)
    L = np.linalg.cholesky(Kd)
    Kinv = np.linalg.inv(Kd)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    fx = -0.5 * y @ alpha - np.sum(np.log(np.diag(L))) - 0.5 * N * np.log(2 * np.pi)
    G = 0.5 * (np.outer(alpha, alpha) - Kinv)
    return fx, np.concatenate([ard_sums(G, Ks, Kl), [2 * NOISE * np.trace(G)]]), L.sum()


def _sum_chol(family, N, D, th):
    x, _ = tape_inputs(N, D)
    K = ard_ref(family, x, th[1:1 + D], th[0])[0]
    return np.linalg.cholesky(K + th[-1] * th[-1] * np.eye(N)).sum()


@pytest.mark.parametrize("N,D", [(64, 3), (301, 2), (1024, 4)])
@pytest.mark.parametrize("family", NAMES)
def test_gp_marginal_gradient_through_tape(family, N, D):
    """stan::math::gradient of the GP marginal with theta = (sigma, l_1..l_D,
    noise), twice (arena re-use; N = 1024 takes the closed-form schedule on
    the second evaluation).  K is never formed: no deferred matrix is
    materialised, and the gradient with deferred values off agrees at 1e-12."""
    fx, g, _ = marginal_ref(family, N, D)
    rows, formed = tape_run(family, N, D, False, "vv")
    for row in rows:
        print(f"{family} N={N} D={D}: fx {row[0]!r} (ref {fx!r}) grad {row[1:]} (ref {g})")
        assert row.size == 3 + D
        near_rel(row[0], fx, 1e-12, what="fx")
        near_rel(row[1:], g, 1e-10, what="grad")
    assert formed == 0
    eager, formed = tape_run(family, N, D, False, "vv", False)
    assert formed == 0  # (nothing is deferred then)
    for row, e in zip(rows, eager):
        near_rel(e, row, 1e-12, what="deferred values off")


@pytest.mark.parametrize("family", NAMES)
def test_gp_marginal_mixed_consumers(family):
    """+ 1e-3 sum(L): the factor has a second consumer, the dense fallback
    through smg_gp_ard_cov_rev.  The gradient is the unmixed one plus the
    increment d/dtheta 1e-3 sum(L), whose reference is a central difference
    (h = 1e-5) of numpy's Cholesky: the total at 1e-10 and the increment at
    1e-6 of its own size."""
    N, D = 301, 2
    fx, g, sl = marginal_ref(family, N, D)
    th0 = np.concatenate([[TSIG], tape_scales(D), [NOISE]])
    h = 1e-5
    inc = np.zeros(th0.size)
    for i in range(th0.size):
        tp, tm = th0.copy(), th0.copy()
        tp[i] += h
        tm[i] -= h
        inc[i] = 1e-3 * (_sum_chol(family, N, D, tp) - _sum_chol(family, N, D, tm)) / (2 * h)
    plain = tape_run(family, N, D, False, "vv")[0]
    for row, base in zip(tape_run(family, N, D, True, "vv")[0], plain):
        print(f"{family}: mixed fx {row[0]!r} grad {row[1:]} increment {row[1:] - base[1:]} (ref {inc})")
        near_rel(row[0], fx + 1e-3 * sl, 1e-12, what="fx")
        near_rel(row[1:], g + inc, 1e-10, atol=1e-6 * np.abs(inc).min(), what="grad")
        near_rel(row[1:] - base[1:], inc, 1e-6, atol=0.0, what="increment")


@pytest.mark.parametrize("kinds", ["dv", "vd"])
@pytest.mark.parametrize("family", NAMES)
def test_gp_marginal_data_arguments(family, kinds):
    """(double sigma, vector<var> l) and (var sigma, vector<double> l): the
    gradient has the entries of the var arguments alone."""
    N, D = 64, 3
    fx, g, _ = marginal_ref(family, N, D)
    keep = list(range(1, 2 + D)) if kinds == "dv" else [0, 1 + D]
    for row in tape_run(family, N, D, False, kinds)[0]:
        assert row.size == 1 + len(keep), row  # none for the data argument
        near_rel(row[0], fx, 1e-12, what="fx")
        near_rel(row[1:], g[keep], 1e-10, what="grad")


def test_cpp_argument_errors():
    """Exception types and messages of the four functions, checks in the order
    x, magnitude, every length scale, their count, the cap, the point sizes."""
    lines = _run("errors\n").strip().splitlines()
    assert lines[-1] == "stack 0 0"
    got = {}
    for l in lines[:-1]:
        fn, case, typ, msg = l.split("|", 3)
        got[(fn, case)] = (typ, msg)
    for fn in ("gp_exp_quad_cov", "gp_exponential_cov", "gp_matern32_cov", "gp_matern52_cov"):
        dom = lambda m: ("domain_error", f"{fn}: {m}")  # noqa: E731
        inv = lambda m: ("invalid_argument", f"{fn}: {m}")  # noqa: E731
        nan = dom("x is nan, but must not be nan!")
        count = inv("x dimension (3) and number of length scales (2) must match in size")
        want = {
            "ok": ("none", ""),
            "empty": ("none", ""),
            "sigma=0": dom("magnitude is 0, but must be > 0!"),
            "sigma=inf": dom("magnitude is inf, but must be finite!"),
            "l2=0": dom("length scale[2] is 0, but must be > 0!"),
            "l3=inf": dom("length scale[3] is inf, but must be finite!"),
            "l1=-1, l2=0": dom("length scale[1] is -1, but must be > 0!"),
            "x nan": nan,
            "x nan, sigma=0, l1=0": nan,
            "sigma=0, l1=0": dom("magnitude is 0, but must be > 0!"),
            "count": count,
            "count, l2=0": dom("length scale[2] is 0, but must be > 0!"),
            "count 65": inv("x dimension (3) and number of length scales (65) must match in size"),
            "65": inv("number of length scales (65) exceeds the supported 64"),
            "points size": ("invalid_argument",
                            "squared_distance: size of v1 (2) and size of v2 (3) must match in size"),
            "points size, count": count,
        }
        for case, w in want.items():
            assert got[(fn, case)] == w, (fn, case, got[(fn, case)], w)
    assert len(got) == 4 * 16
