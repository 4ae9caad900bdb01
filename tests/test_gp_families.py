"""The Matern-family GP covariances (exponential, 3/2, 5/2) on the device:
smg_gp_cov_fwd / _rev / _inverse_adjoint through ctypes, and
gp_exponential_cov / gp_matern32_cov / gp_matern52_cov through the tape
(tests/cpp/test_gp_families.cpp).

The reference of every test is float64 numpy written from the closed forms
(d = |x_i - x_j|, K_ii = sigma^2, dK/dsigma = 2 K / sigma everywhere):

    exponential  K = s2 exp(-d / l)                              dK/dl = K d / l^2
    matern32     K = s2 (1 + a) exp(-a),           a = sqrt(3) d / l   dK/dl = s2 a^2 exp(-a) / l
    matern52     K = s2 (1 + a + a^2 / 3) exp(-a), a = sqrt(5) d / l   dK/dl = s2 a^2 (1 + a) exp(-a) / (3 l)

Tolerances: K at 1e-13 relative (the ranges keep a below about 60, where the
a eps growth of exp(-a)'s relative error leaves the float64 reference an order
of magnitude of room), hyperparameter adjoints at 1e-11, the fused reducer
against the composition at 1e-12, the tape's fx at 1e-12 and gradient at 1e-10.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import gen
from _util import ROOT, near_rel, prebuilt

pytestmark = pytest.mark.gpu

FAMILIES = {"exponential": 1, "matern32": 2, "matern52": 3}
NAMES = sorted(FAMILIES)
SIG, ELL = 1.3, 0.9
SMG_ERR_ARG = 16


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
def dist(x):
    """d_ij for x (n, D): |x_i - x_j| for D == 1, else the square root of the
    squared distance summed in coordinate order."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[1] == 1:
        return np.abs(x[:, 0][:, None] - x[:, 0][None, :])
    d2 = np.zeros((x.shape[0], x.shape[0]))
    for c in range(x.shape[1]):
        t = x[:, c][:, None] - x[:, c][None, :]
        d2 += t * t
    return np.sqrt(d2)


def cov_ref(family, d, sigma, l):
    """(K, dK/dsigma, dK/dl) from the table; the diagonal is sigma^2 with a zero l-derivative."""
    s2 = sigma * sigma
    if family == "exponential":
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
    K, Kl = K.copy(), Kl.copy()
    np.fill_diagonal(K, s2)
    np.fill_diagonal(Kl, 0.0)
    return K, 2 * K / sigma, Kl


@functools.lru_cache(maxsize=None)
def inputs(n, D):
    """x (n, D), the upper-triangle weights W and the references' distances,
    shared by the families."""
    half = 0.5 if (n, D) == (64, 200) else 5.0
    x = gen.unif(gen.SEED + 7 * n + D, n * D, -half, half).reshape(n, D)
    W = np.triu(gen.unif(gen.SEED + 11 * n + D, n * n, -1.0, 1.0).reshape(n, n))
    d = dist(x)
    for a in (x, W, d):
        a.setflags(write=False)
    return x, W, d


def fwd(ctx, fam, x, ldk, sigma=SIG, l=ELL, fill=None):
    n, D = x.shape
    buf = np.full(ldk * n, np.nan if fill is None else fill)
    dK = ctx.put(buf)
    rc = ctx.lib.smg_gp_cov_fwd(ctx.ptr, fam, ctx.put(x.ravel()) if n else None, D, n, sigma, l, dK, ldk)
    assert rc == 0
    return ctx.get(dK, ldk * n).reshape(n, ldk).T  # (ldk, n): column j of K at [:, j]


def rev(ctx, fam, x, W, ldka, sigma=SIG, l=ELL):
    n, D = x.shape
    A = np.zeros((ldka, n))
    A[:n] = W
    out = ctx.put(np.array([0.25, -0.5]))  # accumulated into
    rc = ctx.lib.smg_gp_cov_rev(ctx.ptr, fam, ctx.put(x.ravel()), D, n, sigma, l, ctx.put(F(A)), ldka, out)
    assert rc == 0
    return ctx.get(out, 2) - np.array([0.25, -0.5])


SCALAR = [(1, 1), (2, 2), (33, 33), (300, 300), (300, 303), (2050, 2050), (2050, 2053)]
POINTS = [(1, 3), (2, 2), (33, 3), (300, 5), (2051, 3), (64, 200)]


def check_fwd_rev(ctx, family, n, D, ldk):
    x, W, d = inputs(n, D)
    K, Ks, Kl = cov_ref(family, d, SIG, ELL)
    out = fwd(ctx, FAMILIES[family], x, ldk, fill=-7.0)
    got = out[:n]
    print(f"{family} n={n} D={D} ldk={ldk}: K rel {near_rel(got, K, 1e-13, atol=1e-300, what='K'):.2e}")
    assert np.array_equal(got, got.T)
    assert np.array_equal(np.diag(got), np.full(n, SIG * SIG))
    assert np.all(out[n:] == -7.0)  # the padding rows are not written
    g = rev(ctx, FAMILIES[family], x, W, ldk)
    ref = np.array([np.sum(W * Ks), np.sum(W * Kl)])
    if n == 1:
        assert g[1] == 0.0
    print(f"  [dsigma, dl] {g} rel {near_rel(g, ref, 1e-11, what='[dsigma, dl]'):.2e}")


# ------------------------------------------------ 1. forward / reverse per family
@pytest.mark.parametrize("n,ldk", SCALAR)
@pytest.mark.parametrize("family", NAMES)
def test_cov_scalar_x(ctx, family, n, ldk):
    """Scalar x: 33 and odd leading dimensions take the generic form, 300 and
    2050 aligned the 16-byte column form (2050 > 2048 workgroups: the column
    loop wraps); ldk = n + 3 leaves the padding untouched."""
    check_fwd_rev(ctx, family, n, 1, ldk)


@pytest.mark.parametrize("n,D", POINTS)
@pytest.mark.parametrize("family", NAMES)
def test_cov_points(ctx, family, n, D):
    """D-dimensional points (x_j staged in LDS), also with ldk = n + 3."""
    check_fwd_rev(ctx, family, n, D, n)
    if n == 33:
        check_fwd_rev(ctx, family, n, D, n + 3)


@pytest.mark.parametrize("n,D", [(33, 1), (300, 1), (33, 3)])
@pytest.mark.parametrize("family", NAMES)
def test_cov_coincident_points(ctx, family, n, D):
    """x sorted descending with x[7] = x[3]: the off-diagonal entry is exactly
    sigma^2 (no 0 / 0 in any derivative), everything finite."""
    x = inputs(n, D)[0].copy()
    x = x[np.argsort(-x[:, 0])]
    x[7] = x[3]
    W = inputs(n, D)[1]
    out = fwd(ctx, FAMILIES[family], x, n)
    assert out[7, 3] == SIG * SIG and out[3, 7] == SIG * SIG
    assert np.all(np.isfinite(out)) and np.array_equal(out, out.T)
    K, Ks, Kl = cov_ref(family, dist(x), SIG, ELL)
    near_rel(out, K, 1e-13, atol=1e-300, what="K")
    # all the weight on the coincident pair: dl is exactly zero
    E = np.zeros((n, n))
    E[3, 7] = E[7, 3] = 1.0
    g = rev(ctx, FAMILIES[family], x, E, n)
    assert g[1] == 0.0 and np.isfinite(g[0])
    near_rel(g[0], 4 * SIG, 1e-13, what="dsigma of the pair")
    g = rev(ctx, FAMILIES[family], x, W, n)
    assert np.all(np.isfinite(g))
    near_rel(g, [np.sum(W * Ks), np.sum(W * Kl)], 1e-11, what="[dsigma, dl]")


# ------------------------------------------------------ 2. family 0 is the old code
def _inverse_adjoint_inputs(N, D, k):
    rng = np.random.default_rng(N * 7 + D + k)
    M = rng.uniform(-1, 1, (N, N))
    C = M @ M.T / N + np.eye(N)
    s = rng.uniform(-1, 1, (k, 2 * N))  # observation o's s at o * 2N (s_stride 2N)
    x = rng.uniform(-3, 3, (N, D))
    return C, s, x


@pytest.mark.parametrize("n,D", [(33, 1), (300, 1), (300, 5)])
def test_family_zero_is_exp_quad(ctx, n, D):
    """SMG_GP_EXP_QUAD through the family entries gives the bits of the
    smg_gp_exp_quad_cov_nd_* / smg_gp_inverse_adjoint entries."""
    x, W, _ = inputs(n, D)
    dx = ctx.put(x.ravel())
    K0, K1 = ctx.put(np.full(n * n, np.nan)), ctx.put(np.full(n * n, np.nan))
    ctx.call("smg_gp_exp_quad_cov_nd_fwd", dx, D, n, SIG, ELL, K0, n)
    ctx.call("smg_gp_cov_fwd", 0, dx, D, n, SIG, ELL, K1, n)
    assert np.array_equal(ctx.get(K0, n * n), ctx.get(K1, n * n))
    dW, o0, o1 = ctx.put(F(W)), ctx.zeros(2), ctx.zeros(2)
    ctx.call("smg_gp_exp_quad_cov_nd_rev", dx, D, n, SIG, ELL, dW, n, o0)
    ctx.call("smg_gp_cov_rev", 0, dx, D, n, SIG, ELL, dW, n, o1)
    assert np.array_equal(ctx.get(o0, 2), ctx.get(o1, 2))
    C, s, _ = _inverse_adjoint_inputs(n, D, 2)
    dC, ds = ctx.put(F(C)), ctx.put(s.ravel())
    r = []
    for name, fam in (("smg_gp_inverse_adjoint", ()), ("smg_gp_cov_inverse_adjoint", (0,))):
        dd, o = ctx.zeros(1), ctx.zeros(2)
        ctx.call(name, *fam, dC, n, n, ds, 2, 2 * n, 0.8, K0, n, dx, D, SIG, ELL, dd, o)
        r.append(np.concatenate([ctx.get(dd, 1), ctx.get(o, 2)]))
    assert np.array_equal(r[0], r[1])


# ------------------------------------------- 3. fused reducer against composition
@pytest.mark.parametrize("N,D,k", [(64, 1, 1), (301, 1, 1), (512, 3, 1), (1024, 1, 2), (257, 2, 3)])
@pytest.mark.parametrize("family", NAMES)
def test_cov_inverse_adjoint_vs_composition(ctx, family, N, D, k):
    """smg_gp_cov_inverse_adjoint against smg_cholesky_inverse_adjoint ->
    smg_add_diag_rev -> smg_gp_cov_rev on the device ([d', sigma', l'] at
    1e-12; d' alone with out2 = NULL), and sigma', l' against numpy from
    G = adj Phi(sum_o s_o s_o^T - k C) at 1e-11."""
    fam = FAMILIES[family]
    C, s, x = _inverse_adjoint_inputs(N, D, k)
    sig, ell, adj = 1.3, 0.7, 0.8
    dC, ds, dx = ctx.put(F(C)), ctx.put(s.ravel()), ctx.put(x.ravel())
    dK = ctx.zeros(N * N)
    ctx.call("smg_gp_cov_fwd", fam, dx, D, N, sig, ell, dK, N)
    dKd, dKa, dd0, o0 = ctx.zeros(N * N), ctx.zeros(N * N), ctx.zeros(1), ctx.zeros(2)
    ctx.call("smg_cholesky_inverse_adjoint", dC, N, N, ds, k, 2 * N, adj, dKd, N)
    ctx.call("smg_add_diag_rev", dKd, N, N, dKa, N, dd0, 0)
    ctx.call("smg_gp_cov_rev", fam, dx, D, N, sig, ell, dKa, N, o0)
    dd1, o1 = ctx.put(np.array([np.nan])), ctx.put(np.array([np.nan, np.nan]))  # written, not accumulated
    ctx.call("smg_gp_cov_inverse_adjoint", fam, dC, N, N, ds, k, 2 * N, adj, dK, N, dx, D, sig, ell, dd1, o1)
    dd2 = ctx.zeros(1)  # the diagonal sum alone (K0, x unused)
    ctx.call("smg_gp_cov_inverse_adjoint", fam, dC, N, N, ds, k, 2 * N, adj, None, N, None, 1, 1.0, 1.0, dd2, None)
    r0 = np.concatenate([ctx.get(dd0, 1), ctx.get(o0, 2)])
    r1 = np.concatenate([ctx.get(dd1, 1), ctx.get(o1, 2)])
    print(f"{family} N={N} D={D} k={k}: fused {r1} composition {r0}")
    near_rel(r1, r0, 1e-12, what="[d', sigma', l']")
    near_rel(ctx.get(dd2, 1), r0[:1], 1e-12, what="d' alone")
    S = sum(np.outer(s[o, :N], s[o, :N]) for o in range(k))
    G = adj * (S - k * C)
    G = np.tril(G, -1) + 0.5 * np.diag(np.diag(G))
    K, Ks, Kl = cov_ref(family, dist(x), sig, ell)
    near_rel(r1[1:], [np.sum(G * Ks), np.sum(G * Kl)], 1e-11, what="[sigma', l'] vs numpy")
    near_rel(r1[0], np.trace(G), 1e-11, what="d' vs numpy")


# ------------------------------------------------------------- 5. errors (ctypes)
def test_cov_entries_argument_errors(ctx):
    """Unknown family, ldk < n and null pointers: SMG_ERR_ARG, the context's
    status untouched; n = 0 is a no-op."""
    n = 8
    x, W, _ = inputs(33, 1)
    dx, dK, o = ctx.put(x[:n].ravel()), ctx.zeros(n * n), ctx.zeros(2)
    L = ctx.lib
    for fam in (-1, 4, 17):
        assert L.smg_gp_cov_fwd(ctx.ptr, fam, dx, 1, n, SIG, ELL, dK, n) == SMG_ERR_ARG
        assert L.smg_gp_cov_rev(ctx.ptr, fam, dx, 1, n, SIG, ELL, dK, n, o) == SMG_ERR_ARG
        assert L.smg_gp_cov_inverse_adjoint(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dK, n, dx, 1, SIG, ELL, o,
                                            o) == SMG_ERR_ARG
    for fam in (1, 2, 3):
        assert L.smg_gp_cov_fwd(ctx.ptr, fam, dx, 1, n, SIG, ELL, dK, n - 1) == SMG_ERR_ARG
        assert L.smg_gp_cov_fwd(ctx.ptr, fam, None, 1, n, SIG, ELL, dK, n) == SMG_ERR_ARG
        assert L.smg_gp_cov_fwd(ctx.ptr, fam, dx, 1, n, SIG, ELL, None, n) == SMG_ERR_ARG
        assert L.smg_gp_cov_fwd(ctx.ptr, fam, dx, 0, n, SIG, ELL, dK, n) == SMG_ERR_ARG
        assert L.smg_gp_cov_fwd(None, fam, dx, 1, n, SIG, ELL, dK, n) == SMG_ERR_ARG
        assert L.smg_gp_cov_rev(ctx.ptr, fam, dx, 1, n, SIG, ELL, dK, n - 1, o) == SMG_ERR_ARG
        assert L.smg_gp_cov_rev(ctx.ptr, fam, None, 1, n, SIG, ELL, dK, n, o) == SMG_ERR_ARG
        assert L.smg_gp_cov_rev(ctx.ptr, fam, dx, 1, n, SIG, ELL, None, n, o) == SMG_ERR_ARG
        assert L.smg_gp_cov_rev(ctx.ptr, fam, dx, 1, n, SIG, ELL, dK, n, None) == SMG_ERR_ARG
        ia = L.smg_gp_cov_inverse_adjoint
        assert ia(ctx.ptr, fam, dK, n - 1, n, dx, 1, n, 1.0, dK, n, dx, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dK, n - 1, dx, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, None, n, n, dx, 1, n, 1.0, dK, n, dx, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, None, 1, n, 1.0, dK, n, dx, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, None, n, dx, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 1, n, 1.0, dK, n, None, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert ia(ctx.ptr, fam, dK, n, n, dx, 0, n, 1.0, dK, n, dx, 1, SIG, ELL, o, o) == SMG_ERR_ARG
        assert L.smg_gp_cov_fwd(ctx.ptr, fam, None, 1, 0, SIG, ELL, None, 0) == 0
        assert L.smg_gp_cov_rev(ctx.ptr, fam, None, 1, 0, SIG, ELL, None, 0, None) == 0
    assert ctx.status() == 0


# ---------------------------------------------------- 4. end to end through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_families")
THETA = (1.3, 0.7, 0.5)


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@functools.lru_cache(maxsize=None)
def tape_inputs(N, D):
    rng = np.random.default_rng(1000 * D + N)
    x = rng.uniform(-10, 10, (N, D))
    y = rng.standard_normal(N)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def tape_run(family, N, D, mixed, kinds):
    """The rows [fx, gradient...] of the program's two evaluations."""
    x, y = tape_inputs(N, D)
    head = f"grad {family} {int(mixed)} {kinds} {D} {N} " + " ".join(repr(float(v)) for v in THETA)
    out = _run(head + "\n" + " ".join(repr(float(v)) for v in x.ravel()) + "\n" +
               " ".join(repr(float(v)) for v in y) + "\n")
    lines = out.strip().splitlines()
    assert lines[-1] == "stack 0 0", lines[-1]
    rows = [np.array([float(v) for v in l.split()]) for l in lines[:-1]]
    assert len(rows) == 2
    return rows


@functools.lru_cache(maxsize=None)
def marginal_ref(family, N, D):
    """(fx, [dsigma, dl, dnoise], sum(L)) of the GP marginal in numpy:
    G = (alpha alpha^T - Kd^{-1}) / 2 against the table's derivatives."""
    x, y = tape_inputs(N, D)
    sigma, l, noise = THETA
    K, Ks, Kl = cov_ref(family, dist(x), sigma, l)
    Kd = K + noise * noise * np.eye(N)
    L = np.linalg.cholesky(Kd)
    Kinv = np.linalg.inv(Kd)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    fx = -0.5 * y @ alpha - np.sum(np.log(np.diag(L))) - 0.5 * N * np.log(2 * np.pi)
    G = 0.5 * (np.outer(alpha, alpha) - Kinv)
    return fx, np.array([np.sum(G * Ks), np.sum(G * Kl), 2 * noise * np.trace(G)]), L.sum()


def _sum_chol(family, N, D, th):
    x, _ = tape_inputs(N, D)
    K = cov_ref(family, dist(x), th[0], th[1])[0]
    return np.linalg.cholesky(K + th[2] * th[2] * np.eye(N)).sum()


@pytest.mark.parametrize("N,D", [(64, 1), (301, 1), (1024, 1), (64, 3)])
@pytest.mark.parametrize("family", NAMES)
def test_gp_marginal_gradient_through_tape(family, N, D):
    """stan::math::gradient of the GP marginal written with the family's
    function, twice (arena re-use; N = 1024 takes the closed-form schedule on
    the second evaluation), D = 3: std::vector<Eigen::VectorXd> x."""
    fx, g, _ = marginal_ref(family, N, D)
    for row in tape_run(family, N, D, False, "vv"):
        print(f"{family} N={N} D={D}: fx {row[0]!r} (ref {fx!r}) grad {row[1:]} (ref {g})")
        assert row.size == 4
        near_rel(row[0], fx, 1e-12, what="fx")
        near_rel(row[1:], g, 1e-10, what="grad")


@pytest.mark.parametrize("family", NAMES)
def test_gp_marginal_mixed_consumers(family):
    """+ 1e-3 sum(L): the factor has a second consumer, the dense fallback.
    The gradient is the unmixed one plus the increment d/dtheta 1e-3 sum(L),
    whose reference is a central difference (h = 1e-5) of numpy's Cholesky:
    the total at 1e-10 and the increment at 1e-6 of its own size."""
    N = 301
    fx, g, sl = marginal_ref(family, N, 1)
    h = 1e-5
    inc = np.zeros(3)
    for i in range(3):
        tp, tm = np.array(THETA), np.array(THETA)
        tp[i] += h
        tm[i] -= h
        inc[i] = 1e-3 * (_sum_chol(family, N, 1, tp) - _sum_chol(family, N, 1, tm)) / (2 * h)
    plain = tape_run(family, N, 1, False, "vv")
    for row, base in zip(tape_run(family, N, 1, True, "vv"), plain):
        print(f"{family}: mixed fx {row[0]!r} grad {row[1:]} increment {row[1:] - base[1:]} (ref {inc})")
        near_rel(row[0], fx + 1e-3 * sl, 1e-12, what="fx")
        near_rel(row[1:], g + inc, 1e-10, atol=1e-6 * np.abs(inc).min(), what="grad")
        near_rel(row[1:] - base[1:], inc, 1e-6, atol=0.0, what="increment")


@pytest.mark.parametrize("kinds", ["dv", "vd"])
@pytest.mark.parametrize("family", NAMES)
def test_gp_marginal_data_hyperparameter(family, kinds):
    """(double sigma, var l) and (var sigma, double l): the gradient has the
    entries of the var arguments alone (theta = (l, noise) / (sigma, noise))."""
    fx, g, _ = marginal_ref(family, 64, 1)
    keep = [1, 2] if kinds == "dv" else [0, 2]
    for row in tape_run(family, 64, 1, False, kinds):
        assert row.size == 3, row  # fx and two entries: none for the data argument
        near_rel(row[0], fx, 1e-12, what="fx")
        near_rel(row[1:], g[keep], 1e-10, what="grad")


def test_cpp_argument_errors():
    """Exception types and messages of the three functions, checks in the
    order x, magnitude, length scale, then the point sizes."""
    lines = _run("errors\n").strip().splitlines()
    assert lines[-1] == "stack 0 0"
    got = {}
    for l in lines[:-1]:
        fn, case, typ, msg = l.split("|", 3)
        got[(fn, case)] = (typ, msg)
    for fn in ("gp_exponential_cov", "gp_matern32_cov", "gp_matern52_cov"):
        dom = lambda m: ("domain_error", f"{fn}: {m}")  # noqa: E731
        nan = dom("x is nan, but must not be nan!")
        want = {
            "ok": ("none", ""),
            "sigma=0": dom("magnitude is 0, but must be > 0!"),
            "sigma=-1": dom("magnitude is -1, but must be > 0!"),
            "sigma=inf": dom("magnitude is inf, but must be finite!"),
            "l=0": dom("length scale is 0, but must be > 0!"),
            "l=inf": dom("length scale is inf, but must be finite!"),
            "x nan": nan,
            "x nan, sigma=0, l=0": nan,
            "sigma=0, l=0": dom("magnitude is 0, but must be > 0!"),
            "points ok": ("none", ""),
            "points size": ("invalid_argument",
                            "squared_distance: size of v1 (2) and size of v2 (3) must match in size"),
            "points nan": nan,
            "points sigma=0": dom("magnitude is 0, but must be > 0!"),
            "points l=inf": dom("length scale is inf, but must be finite!"),
            "points size, l=0": dom("length scale is 0, but must be > 0!"),
        }
        for case, w in want.items():
            assert got[(fn, case)] == w, (fn, case, got[(fn, case)], w)
    assert len(got) == 3 * 15
