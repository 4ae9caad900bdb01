"""Kernel-level tests of the tangent (fvar<var>) nodes against the plain
references of _ref_tangent.py: the Cholesky tangent node, the tangent of
gp_exp_quad_cov, lse_tangent, glm_tangent and mdivide_left_tri with a factor's
block inverses.

Layout: every matrix sits in a buffer with ld > rows and one spare column
(_ref_tangent.Mat); inputs carry NaN in their padding, outputs a sentinel that
must keep its bits; accumulated outputs start from random values, written ones
from NaN.

Matrix outputs are compared at the project's near_rel(1e-10, atol = 1e-10
max|ref|).  Scalar reductions are held to
    |s - s_ref| <= gamma_{N + c} sum |term|,   gamma_k = k u / (1 - k u), u = 2^-53
with N the number of summed terms, the terms from the longdouble reference and
c the roundings that form one term (a libm exp counted as 2: 1 ulp = 2 u), and
per-element updates a0 + inc to u (c |inc| + 2 (|a0| + |inc|)).  The constants:

  GP tangent, x in [-2, 2], l = 1.3, so z = d^2 / (2 l^2) <= 16 / 3.38 < 4.8:
    z carries 5 roundings (d, d^2, l l, 0.5 / (l l), the product): e = exp(-z)
    is off by 5 z u + 2 u <= 26 u.  Kd_ij = a e + b d^2 e: a (2), b = sigma^2
    l' / l^3 (5), d^2 (2), two products and the sum (3): C_GP_FWD = 26 + 12 =
    38.  out4's terms A e d^4: 26 + the products by A, d^2, d^2 (3) + d^2's own
    roundings twice (4) = 33, and each out4 formula adds at most 10 roundings
    (powers of l, the coefficient products, the division, the sums):
    C_GP_REV = 43.
  lse_tangent, x in [-8, 8]: x - max in [-16, 0] (1 rounding: 16 u absolute)
    + exp (2): e within 18 u; times xd, the division by s, the sum into it:
    C_LSE = 22.  rev: x - lse in [-25, 0] (lse <= 8 + log 4099 < 17): p within
    27 u, (xd - t), the two products: C_LSE_REV = 30.
  glm_tangent: theta = eta + alpha is formed exactly by the inputs below, so
    exp(-s theta) carries 2 u; q = 1 / (1 + e) 2, s e q 2, (etad + alphad) 1,
    the product 1: C_GLM = 8; dd = -e q q and the products by adj and
    (etad + alphad): C_GLM_REV = 10.
"""
import functools

import numpy as np
import pytest

from _ref_tangent import (LD, SMG_ERR_ARG, U, Mat, chol_tangent_case, chol_tangent_fwd_ref, chol_tangent_rev_ref,
                          elem_bound, gamma, glm_theta_derivative_ref, gp_tangent_fwd_ref, gp_tangent_rev_ref, lds,
                          lse_tangent_ref, same_bits, vec)
from _util import near_rel

RTOL = 1e-10  # the project's standing value (test_gpu_kernels.RTOL)
C_GP_FWD, C_GP_REV, C_LSE, C_LSE_REV, C_GLM, C_GLM_REV = 38, 43, 22, 30, 8, 10


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


def near_mat(got, ref, what, rtol=RTOL):
    near_rel(got, ref, rtol, atol=rtol * float(np.abs(ref).max()), what=what)


# ====================================================================== CPU
def test_reference_finite_differences():
    """The reference formulas themselves (not the kernel): central differences
    of <L'bar, L'(L, A')> in longdouble at n = 7 against dLadj and dA'adj, and
    the defining equation L' L^T + L L'^T = A'."""
    n = 7
    A, L, Ad, Ldbar, _ = chol_tangent_case(n, "ld")
    L, Ad, Ldbar = L.astype(LD), Ad.astype(LD), Ldbar.astype(LD)
    W, Y, P, Ld = chol_tangent_fwd_ref(L, Ad)
    dL, dA = chol_tangent_rev_ref(L, W, Y, P, Ldbar)
    assert np.abs(Ld @ L.T + L @ Ld.T - Ad).max() <= 1e-17 * np.abs(Ad).max()

    def f(L_, Ad_):
        return (Ldbar * chol_tangent_fwd_ref(L_, Ad_)[3]).sum()

    def slope(g, h=LD(1e-4)):
        """g'(0) by central differences at h and h / 2, Richardson-combined:
        truncation O(h^4), rounding about 2^-63 |g| / h ~ 1e-14 here."""
        d = lambda t: (g(t) - g(-t)) / (2 * t)  # noqa: E731
        return (4 * d(h / 2) - d(h)) / 3

    rng = np.random.default_rng(5)
    for _ in range(3):
        E = np.tril(rng.uniform(-1, 1, (n, n))).astype(LD)
        err = abs(slope(lambda t: f(L + t * E, Ad)) - (dL * E).sum())
        print(f"dLadj: finite difference off by {float(err):.2e}")
        assert err <= 1e-13 * np.abs(dL).sum()
        R = rng.uniform(-1, 1, (n, n))
        E = (R + R.T).astype(LD)
        err = abs(slope(lambda t: f(L, Ad + t * E)) - (dA * E).sum())
        print(f"dA'adj: finite difference off by {float(err):.2e}")
        assert err <= 1e-13 * np.abs(dA).sum()
    assert np.array_equal(dA, dA.T) or np.abs(dA - dA.T).max() <= 1e-18 * np.abs(dA).max()


def test_reference_float64_margin():
    """The float64 reference used for n >= 512 stays within 1e-12 (relative to
    max-abs) of the longdouble one at n = 200: two digits under RTOL."""
    ld = chol_tangent_case(200, "ld")[4]
    f64 = chol_tangent_case(200, "f64")[4]
    for k in ld:
        assert np.abs(ld[k] - f64[k]).max() <= 1e-12 * np.abs(ld[k]).max(), k


def test_reference_gp_tangent_finite_differences():
    """out4 of the GP tangent's reverse against central differences of
    <Kdadj, Kd(sigma, l, sigma', l')> at n = 6."""
    rng = np.random.default_rng(6)
    n = 6
    x = rng.uniform(-2, 2, n)
    x[4] = x[1]
    Ka = rng.uniform(-1, 1, (n, n))
    th = np.array([1.7, 1.3, 0.7, -0.3], dtype=LD)
    ref, _ = gp_tangent_rev_ref(x, *th, Ka)
    h = LD(1e-6)
    for k in range(4):
        e = np.zeros(4, dtype=LD)
        e[k] = h
        fd = ((Ka * gp_tangent_fwd_ref(x, *(th + e))).sum() - (Ka * gp_tangent_fwd_ref(x, *(th - e))).sum()) / (2 * h)
        assert abs(fd - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), (k, fd, ref[k])


# ====================================================================== the Cholesky tangent node
NODE_CASES = [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (130, 0), (130, 1), (200, 0), (200, 1), (512, 1),
              (1024, 0), (1024, 1), (1536, 1)]
_NODE = {}


def node(ctx, n, with_aux):
    """One forward and the reverses of the node on the device (once per case);
    host copies of every output.  The forward and the reverse test of a case
    share them through _NODE: what fails in here (a write outside a matrix,
    say) is reported by both with the same message, and the reverse test checks
    the reverse of the forward it shares.  P's strict upper outside the
    diagonal 64 x 64 blocks starts as NaN and is checked neither way: the
    header leaves it undefined."""
    key = (n, with_aux)
    if key in _NODE:
        return _NODE[key]
    A, L, Ad, Ldbar, ref = chol_tangent_case(n)
    lib = ctx.lib
    aux = None
    if with_aux:  # the factor and its block inverses from the device's own factorisation
        dA, dL = ctx.put(A.ravel(order="F")), ctx.zeros(n * n)
        aux = ctx.zeros(lib.smg_cholesky_aux_doubles(n))
        ctx.call("smg_cholesky_fwd", dA, n, n, dL, n, aux)
        L = np.tril(ctx.get(dL, n * n).reshape(n, n).T)
    ldl, ldad, ld, ldla, ldladj, ldaa = lds(n, 6, shift=n % 3)
    rng = np.random.default_rng(77 + n)
    mL = Mat(L, ldl, np.nan)
    mAd = Mat(Ad, ldad, np.nan)
    outs = {k: Mat(np.full((n, n), np.nan), ld, seed=i, name=k) for i, k in enumerate(("W", "Wt", "Y", "P", "Ld"))}
    for m in (mL, mAd, *outs.values()):
        m.put(ctx)
    ctx.call("smg_chol_tangent_fwd", mL.dev, ldl, aux, mAd.dev, ldad, n, outs["W"].dev, outs["Wt"].dev,
             outs["Y"].dev, outs["P"].dev, outs["Ld"].dev, ld)
    r = {k: m.get(ctx) for k, m in outs.items()}
    # the same from the W just formed
    outs2 = {k: Mat(np.full((n, n), np.nan), ld, seed=10 + i, name=k + " (fwd_w)")
             for i, k in enumerate(("Wt", "Y", "P", "Ld"))}
    for m in outs2.values():
        m.put(ctx)
    ctx.call("smg_chol_tangent_fwd_w", mL.dev, ldl, outs["W"].dev, mAd.dev, ldad, n, outs2["Wt"].dev, outs2["Y"].dev,
             outs2["P"].dev, outs2["Ld"].dev, ld)
    r.update({k + "_w": m.get(ctx) for k, m in outs2.items()})
    # reverse: L'bar lower (its strict upper NaN: not read), accumulated outputs from random values
    i, j = np.indices((n, n))
    mT = Mat(np.where(i >= j, Ldbar, np.nan), ldla, np.nan)
    mT.put(ctx)
    R = rng.uniform(-1, 1, (n, n))
    Ladj0, Aadj0 = rng.uniform(-1, 1, (n, n)), R + R.T
    ws = ctx.put(np.full(2 * n * n + 8, np.nan))
    for tag, with_l, with_a in (("", 1, 1), ("_noL", 0, 1), ("_noA", 1, 0)):
        mLa, mAa = Mat(Ladj0, ldladj, seed=3, name="Ladj"), Mat(Aadj0, ldaa, seed=4, name="A'adj")
        mLa.put(ctx), mAa.put(ctx)
        ctx.call("smg_chol_tangent_rev", mL.dev, ldl, outs["W"].dev, outs["Wt"].dev, outs["Y"].dev, outs["P"].dev, ld,
                 mT.dev, ldla, n, mLa.dev if with_l else None, ldladj, mAa.dev if with_a else None, ldaa, ws)
        r["Ladj" + tag], r["Aadj" + tag] = mLa.get(ctx), mAa.get(ctx)
    r.update(L=L, Ladj0=Ladj0, Aadj0=Aadj0)
    _NODE[key] = r
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("n,with_aux", NODE_CASES)
def test_chol_tangent_forward(ctx, n, with_aux):
    A, _, Ad, Ldbar, ref = chol_tangent_case(n)
    r = node(ctx, n, with_aux)
    i, j = np.indices((n, n))
    lo, up = i >= j, i < j
    W, Wt, Y, P, Ld, L = (r[k] for k in ("W", "Wt", "Y", "P", "Ld", "L"))
    near_mat(W[lo], ref["W"][lo], "W")
    assert np.all(W[up] == 0.0), "W's strict upper"
    assert same_bits(Wt, W.T), "Wt is not W^T bit for bit"
    near_mat(Y, ref["Y"], "Y")
    assert same_bits(Y, Y.T), "Y is not bit-symmetric"
    near_mat(P[lo], ref["P"][lo], "P")
    tile_up = up & (i // 64 == j // 64)
    assert np.all(P[tile_up] == 0.0), "P's strict upper inside a diagonal tile"
    near_mat(Ld[lo], ref["Ld"][lo], "Ld")
    assert np.all(Ld[up] == 0.0), "Ld's strict upper"
    # the defining equation on the device's own L and L', however W was formed
    dt = LD if n <= 200 else np.float64
    Lh, Ldh = L.astype(dt), np.tril(Ld).astype(dt)
    res = float(np.abs(Ldh @ Lh.T + Lh @ Ldh.T - Ad.astype(dt)).max())
    bound = 4.0 * gamma(n) * float((np.abs(Ldh) @ np.abs(Lh).T).max())
    print(f"n={n} aux={with_aux}: residual {res:.3e} bound {bound:.3e}")
    assert res <= bound, (res, bound)
    # smg_chol_tangent_fwd_w on that W: the same bits
    assert same_bits(r["Wt_w"], Wt)
    assert same_bits(r["Y_w"], Y)
    assert same_bits(r["P_w"][lo | tile_up], P[lo | tile_up])
    assert same_bits(r["Ld_w"], Ld)


@pytest.mark.gpu
@pytest.mark.parametrize("n,with_aux", NODE_CASES)
def test_chol_tangent_reverse(ctx, n, with_aux):
    A, _, Ad, Ldbar, ref = chol_tangent_case(n)
    r = node(ctx, n, with_aux)
    i, j = np.indices((n, n))
    lo, up = i >= j, i < j
    Ladj, Aadj, Ladj0, Aadj0 = r["Ladj"], r["Aadj"], r["Ladj0"], r["Aadj0"]
    near_mat((Ladj - Ladj0)[lo], ref["dLadj"][lo], "Ladj increment")
    assert same_bits(Ladj[up], Ladj0[up]), "Ladj's strict upper written"
    near_mat(Aadj - Aadj0, ref["dAadj"], "A'adj increment")
    # (an i <= j / i < j slip in the symmetric add doubles or drops the diagonal)
    near_mat(np.diag(Aadj - Aadj0), np.diag(ref["dAadj"]), "A'adj diagonal")
    assert same_bits(Aadj, Aadj.T), "A'adj from a symmetric start is not bit-symmetric"
    # L' is linear in A' for a fixed L: <L'bar, L'> = <dA'adj, A'> on the device's outputs
    Ldev = np.tril(r["Ld"]).astype(LD)
    lhs = (Ldbar.astype(LD) * Ldev).sum()
    rhs = ((Aadj.astype(LD) - Aadj0.astype(LD)) * Ad.astype(LD)).sum()
    bound = 4.0 * gamma(n) * float((np.abs(Ldbar) * np.abs(Ldev)).sum())
    print(f"n={n} aux={with_aux}: linear identity off by {float(abs(lhs - rhs)):.3e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound, (float(lhs), float(rhs), bound)
    # NULL Ladj / NULL Adadj (no fork): the other output as in the full call, the skipped one untouched
    near_mat(r["Aadj_noL"] - Aadj0, ref["dAadj"], "A'adj increment, Ladj NULL")
    near_mat((r["Ladj_noA"] - Ladj0)[lo], ref["dLadj"][lo], "Ladj increment, Adadj NULL")
    near_mat(r["Aadj_noL"], Aadj, "A'adj, Ladj NULL against the full call")
    near_mat(r["Ladj_noA"][lo], Ladj[lo], "Ladj, Adadj NULL against the full call")
    assert same_bits(r["Ladj_noA"][up], Ladj0[up])
    assert same_bits(r["Ladj_noL"], Ladj0) and same_bits(r["Aadj_noA"], Aadj0)


@pytest.mark.gpu
def test_chol_tangent_empty(ctx):
    """n == 0 returns SMG_OK without touching anything."""
    m = Mat(np.zeros((3, 3)), 5)
    p = m.put(ctx)
    ctx.call("smg_chol_tangent_fwd", p, 5, None, p, 5, 0, p, p, p, p, p, 5)
    ctx.call("smg_chol_tangent_fwd_w", p, 5, p, p, 5, 0, p, p, p, p, 5)
    ctx.call("smg_chol_tangent_rev", p, 5, p, p, p, p, 5, p, 5, 0, p, 5, p, 5, p)
    assert same_bits(ctx.get(p, m.host.size), m.host)


# ====================================================================== gp_exp_quad_cov tangent
GP_SIGMA, GP_L = 1.7, 1.3


@functools.lru_cache(maxsize=None)
def gp_case(n):
    rng = np.random.default_rng(900 + n)
    x = rng.uniform(-2.0, 2.0, n)
    if n >= 2:
        x[n // 2] = x[0]          # exact duplicates: d = 0 off the diagonal
    if n >= 63:
        x[n - 1] = x[5] = x[17]
    return x, rng.uniform(-1.0, 1.0, (n, n))


@pytest.mark.gpu
@pytest.mark.parametrize("ds,dl", [(0.7, -0.3), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("n", [1, 2, 63, 257, 300])
def test_gp_tangent_forward(ctx, n, ds, dl):
    x, _ = gp_case(n)
    dx, _r = vec(ctx, x)
    K = Mat(np.full((n, n), np.nan), n + 1 + (n + int(10 * ds)) % 2)   # (both parities of ldk for each n)
    K.put(ctx)
    ctx.call("smg_gp_exp_quad_cov_tangent_fwd", dx, n, GP_SIGMA, GP_L, ds, dl, K.dev, K.ld)
    Kd = K.get(ctx)
    assert same_bits(Kd, Kd.T), "Kd is not bit-symmetric"
    xl = x.astype(LD)
    d2 = (xl[:, None] - xl[None, :]) ** 2
    e = np.exp(-d2 / (2 * LD(GP_L) ** 2))
    terms = np.abs(2 * LD(GP_SIGMA) * LD(ds)) * e + np.abs(LD(GP_SIGMA) ** 2 * LD(dl) / LD(GP_L) ** 3) * d2 * e
    err = np.abs(Kd - gp_tangent_fwd_ref(x, GP_SIGMA, GP_L, ds, dl))
    assert np.all(err <= C_GP_FWD * U * terms), float((err / np.maximum(terms, 1e-300)).max() / U)
    assert np.all(np.diag(Kd) == 2 * GP_SIGMA * ds)


@pytest.mark.gpu
@pytest.mark.parametrize("ds,dl", [(0.7, -0.3), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("n", [1, 2, 63, 257, 300])
def test_gp_tangent_reverse(ctx, n, ds, dl):
    x, Ka = gp_case(n)
    dx, _r = vec(ctx, x)
    mK = Mat(Ka, n + 1 + (n + int(10 * ds)) % 2, np.nan)   # (both parities of ldka for each n)
    mK.put(ctx)
    out0 = np.array([0.3, -1.1, 2.5, -0.7])
    ref, absterms = gp_tangent_rev_ref(x, GP_SIGMA, GP_L, ds, dl, Ka)
    got = []
    for _ in range(2):
        dout, read = vec(ctx, out0)
        ctx.call("smg_gp_exp_quad_cov_tangent_rev", dx, n, GP_SIGMA, GP_L, ds, dl, mK.dev, mK.ld, dout)
        got.append(read())
    assert same_bits(got[0], got[1]), "not deterministic"
    err = np.abs(got[0].astype(LD) - (out0 + ref))
    bound = gamma(n * n + C_GP_REV) * (absterms + np.abs(out0))
    print(f"n={n}: out4 error / bound {np.asarray(err / bound, dtype=np.float64)}")
    assert np.all(err <= bound), (got[0], np.asarray(out0 + ref, dtype=np.float64))


@pytest.mark.gpu
def test_gp_tangent_empty(ctx):
    dout, read = vec(ctx, [1.0, 2.0, 3.0, 4.0])
    ctx.call("smg_gp_exp_quad_cov_tangent_fwd", None, 0, 1.0, 1.0, 1.0, 1.0, None, 0)
    ctx.call("smg_gp_exp_quad_cov_tangent_rev", None, 0, 1.0, 1.0, 1.0, 1.0, None, 0, dout)
    assert np.array_equal(read(), [1.0, 2.0, 3.0, 4.0])


# ====================================================================== lse_tangent
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4099]


@functools.lru_cache(maxsize=None)
def lse_case(n):
    rng = np.random.default_rng(300 + n)
    return rng.uniform(-8.0, 8.0, n), rng.uniform(-1.0, 1.0, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_lse_tangent_forward(ctx, n):
    x, xd = lse_case(n)
    lse, t, p = lse_tangent_ref(x, xd)
    dx, _ = vec(ctx, x)
    dxd, _ = vec(ctx, xd)
    dout, read = vec(ctx, [np.nan, np.nan])
    ctx.call("smg_lse_tangent_fwd", dx, dxd, n, dout)
    out = read()
    g = gamma(n + C_LSE)
    assert abs(out[0] - lse) <= g * (1.0 + abs(x.max()) + abs(float(lse) - x.max())), (out[0], float(lse))
    assert abs(out[1] - t) <= g * float((p * np.abs(xd)).sum() + abs(t)), (out[1], float(t))
    d1, read1 = vec(ctx, [np.nan])
    ctx.call("smg_log_sum_exp_fwd", dx, n, d1)
    near_rel(out[0], read1()[0], 1e-14, what="lse against smg_log_sum_exp_fwd")


@pytest.mark.gpu
def test_lse_tangent_edges(ctx):
    """out[0] as smg_log_sum_exp_fwd gives it: -inf for n == 0 and for all
    -inf, +inf with an entry at +inf -- where out[1] is the mean of xd over the
    entries at +inf (the softmax's limit)."""
    def run(x, xd):
        dout, read = vec(ctx, [np.nan, np.nan])
        ctx.call("smg_lse_tangent_fwd", ctx.put(np.array(x + [0.0])), ctx.put(np.array(xd + [0.0])), len(x), dout)
        d1, read1 = vec(ctx, [np.nan])
        ctx.call("smg_log_sum_exp_fwd", ctx.put(np.array(x + [0.0])), len(x), d1)
        out = read()
        assert out[0] == read1()[0] or (np.isnan(out[0]) and np.isnan(read1()[0])), (out, read1())
        return out

    assert run([], [])[0] == -np.inf
    assert run([-np.inf] * 3, [1.0, 2.0, 3.0])[0] == -np.inf
    out = run([1.0, np.inf, 3.0], [0.25, -0.5, 4.0])
    assert out[0] == np.inf and out[1] == -0.5, out
    out = run([np.inf, -2.0, np.inf, -np.inf], [1.0, 7.0, 2.0, 9.0])
    assert out[0] == np.inf and out[1] == 1.5, out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_lse_tangent_reverse(ctx, n):
    x, xd = lse_case(n)
    lse, t, _ = lse_tangent_ref(x, xd)
    lse, t = float(lse), float(t)
    adj = -0.75
    rng = np.random.default_rng(n)
    a0, b0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    p = np.exp(x.astype(LD) - LD(lse))
    inc_a, inc_b = adj * p * (xd.astype(LD) - LD(t)), adj * p
    dx, _ = vec(ctx, x)
    dxd, _ = vec(ctx, xd)
    for with_a, with_b in ((1, 1), (0, 1), (1, 0)):
        da, ra = vec(ctx, a0, seed=1)
        db, rb = vec(ctx, b0, seed=2)
        ctx.call("smg_lse_tangent_rev", dx, dxd, n, lse, t, adj, da if with_a else None, db if with_b else None)
        ga, gb = ra(), rb()
        if with_a:
            assert np.all(np.abs(ga - (a0 + inc_a)) <= elem_bound(a0, inc_a, C_LSE_REV))
        else:
            assert same_bits(ga, a0)
        if with_b:
            assert np.all(np.abs(gb - (b0 + inc_b)) <= elem_bound(b0, inc_b, C_LSE_REV))
        else:
            assert same_bits(gb, b0)
    da, ra = vec(ctx, a0)
    ctx.call("smg_lse_tangent_rev", dx, dxd, n, lse, t, 0.0, da, da)     # adj == 0
    ctx.call("smg_lse_tangent_rev", dx, dxd, 0, lse, t, adj, da, da)     # n == 0
    assert same_bits(ra(), a0)


# ====================================================================== glm_tangent
GLM_ALPHA, GLM_ALPHAD = 0.5, -0.25


@functools.lru_cache(maxsize=None)
def glm_case(n):
    """theta = eta + alpha with s theta at +-19.999, exactly +-20 (the middle
    branch), +-20.001 and out to +-40 for both y; eta + alpha is exact in
    float64 for the edge values (eta = theta - 0.5 within one binade)."""
    rng = np.random.default_rng(500 + n)
    theta = rng.uniform(-40.0, 40.0, n)
    y = rng.integers(0, 2, n).astype(np.int32)
    edges = [s * v for v in (19.999, 20.0, 20.001, 40.0) for s in (1.0, -1.0)]
    k = 0
    for yy in (0, 1):
        for th in edges:
            if k < n:
                theta[k], y[k] = th, yy
                k += 1
    eta = theta - GLM_ALPHA
    return eta, rng.uniform(-1.0, 1.0, n), y, eta + GLM_ALPHA


def test_glm_edge_thetas_exact():
    eta, _, y, theta = glm_case(64)
    assert set(np.abs(theta[:16])) == {19.999, 20.0, 20.001, 40.0}


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_glm_tangent_forward(ctx, n):
    eta, etad, y, theta = glm_case(n)
    d, _ = glm_theta_derivative_ref(y, theta)
    terms = d * (etad.astype(LD) + LD(GLM_ALPHAD))
    de, _ = vec(ctx, eta)
    ded, _ = vec(ctx, etad)
    dy = ctx.put(np.concatenate([y, np.full(4, 7, np.int32)]))
    got = []
    for _ in range(2):
        dout, read = vec(ctx, [np.nan])
        ctx.call("smg_glm_tangent_fwd", de, GLM_ALPHA, ded, GLM_ALPHAD, dy, n, dout)
        got.append(read()[0])
    assert got[0] == got[1]
    assert abs(got[0] - terms.sum()) <= gamma(n + C_GLM) * float(np.abs(terms).sum()), (got[0], float(terms.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_glm_tangent_reverse(ctx, n):
    eta, etad, y, theta = glm_case(n)
    d, dd = glm_theta_derivative_ref(y, theta)
    adj = 1.25
    inc_a, inc_d = adj * dd * (etad.astype(LD) + LD(GLM_ALPHAD)), adj * d
    rng = np.random.default_rng(n)
    a0, d0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    de, _ = vec(ctx, eta)
    ded, _ = vec(ctx, etad)
    dy = ctx.put(np.concatenate([y, np.full(4, 7, np.int32)]))
    for with_a, with_d in ((1, 1), (0, 1), (1, 0)):
        da, ra = vec(ctx, a0, seed=1)
        dd_, rd = vec(ctx, d0, seed=2)
        dout, read = vec(ctx, [np.nan, np.nan])
        ctx.call("smg_glm_tangent_rev", de, GLM_ALPHA, ded, GLM_ALPHAD, dy, n, adj, da if with_a else None,
                 dd_ if with_d else None, dout)
        ga, gd, out = ra(), rd(), read()
        if with_a:
            assert np.all(np.abs(ga - (a0 + inc_a)) <= elem_bound(a0, inc_a, C_GLM_REV))
        else:
            assert same_bits(ga, a0)
        if with_d:
            assert np.all(np.abs(gd - (d0 + inc_d)) <= elem_bound(d0, inc_d, C_GLM_REV))
        else:
            assert same_bits(gd, d0)
        g = gamma(n + C_GLM_REV)
        assert abs(out[0] - inc_a.sum()) <= g * float(np.abs(inc_a).sum())
        assert abs(out[1] - inc_d.sum()) <= g * float(np.abs(inc_d).sum())


# ====================================================================== mdivide_left_tri with aux
@functools.lru_cache(maxsize=None)
def tri_inputs(m, n):
    rng = np.random.default_rng(7000 + m + n)
    B0 = rng.uniform(-1.0, 1.0, (m, m))
    A = B0 @ B0.T / m + np.eye(m)
    return (0.5 * (A + A.T), rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, (m, m)),
            rng.uniform(-1, 1, (m, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(600, 64), (1024, 1), (1024, 96), (200, 7)])
def test_mdivide_left_tri_aux(ctx, m, n):
    from scipy.linalg import solve_triangular
    A, B, Cadj, Aadj0, Badj0 = tri_inputs(m, n)
    dA, dL = ctx.put(A.ravel(order="F")), ctx.zeros(m * m)
    aux = ctx.zeros(ctx.lib.smg_cholesky_aux_doubles(m))
    ctx.call("smg_cholesky_fwd", dA, m, m, dL, m, aux)
    L = np.tril(ctx.get(dL, m * m).reshape(m, m).T)
    lda, ldb, ldc, ldca, ldaa, ldba = lds(m, 6, shift=n % 2)
    mL, mB, mCa = Mat(L, lda, np.nan), Mat(B, ldb, np.nan), Mat(Cadj, ldca, np.nan)
    for x in (mL, mB, mCa):
        x.put(ctx)
    C = {}
    for tag, a in (("aux", aux), ("none", None)):
        mC = Mat(np.full((m, n), np.nan), ldc)
        mC.put(ctx)
        ctx.call("smg_mdivide_left_tri_aux_fwd", 1, mL.dev, lda, a, mB.dev, ldb, m, n, mC.dev, ldc)
        C[tag] = mC.get(ctx)
        dC = mC.dev
    Cref = solve_triangular(L, B, lower=True)
    near_mat(C["aux"], Cref, "C")
    near_mat(C["aux"], C["none"], "C with aux against without", rtol=1e-12)
    # reverse (dC holds the aux == NULL forward's C in its padded buffer)
    X = solve_triangular(L, Cadj, lower=True, trans="T")
    i, j = np.indices((m, m))
    lo, up = i >= j, i < j
    ws = ctx.put(np.full(m * n + 8, np.nan))
    for with_a, with_b in ((1, 1), (0, 1), (1, 0)):
        mAa, mBa = Mat(Aadj0, ldaa, seed=5), Mat(Badj0, ldba, seed=6)
        mAa.put(ctx), mBa.put(ctx)
        ctx.call("smg_mdivide_left_tri_aux_rev", 1, mL.dev, lda, aux, dC, ldc, mCa.dev, ldca, m, n,
                 mAa.dev if with_a else None, ldaa, mBa.dev if with_b else None, ldba, ws)
        Aa, Ba = mAa.get(ctx), mBa.get(ctx)
        if with_b:
            near_mat(Ba - Badj0, X, "Badj increment")
        else:
            assert same_bits(Ba, Badj0)
        if with_a:
            near_mat((Aa - Aadj0)[lo], (-(X @ C["none"].T))[lo], "Aadj increment")
            assert same_bits(Aa[up], Aadj0[up]), "Aadj's strict upper written"
        else:
            assert same_bits(Aa, Aadj0)


@pytest.mark.gpu
def test_mdivide_left_tri_aux_zero_extents(ctx):
    """m == 0 or n == 0: SMG_OK, C, Aadj and Badj untouched (host-side returns)."""
    mO = Mat(np.zeros((4, 4)), 6)
    p = mO.put(ctx)
    for m, n in ((0, 3), (3, 0), (0, 0)):
        ctx.call("smg_mdivide_left_tri_aux_fwd", 1, p, 6, None, p, 6, m, n, p, 6)
        ctx.call("smg_mdivide_left_tri_aux_rev", 1, p, 6, None, p, 6, p, 6, m, n, p, 6, p, 6, p)
    assert same_bits(ctx.get(p, mO.host.size), mO.host)


@pytest.mark.gpu
def test_mdivide_left_tri_aux_leading_dimensions(ctx):
    """A leading dimension below m is SMG_ERR_ARG on both entries (host-side
    returns: nothing is launched)."""
    m, n = 8, 3
    p = ctx.put(np.zeros(16 * 16))
    lib = ctx.lib
    ok = dict(lda=m, ldb=m, ldc=m, ldca=m, ldaa=m, ldba=m)

    def fwd(**kw):
        a = {**ok, **kw}
        return lib.smg_mdivide_left_tri_aux_fwd(ctx.ptr, 1, p, a["lda"], None, p, a["ldb"], m, n, p, a["ldc"])

    def rev(aadj=p, badj=p, **kw):
        a = {**ok, **kw}
        return lib.smg_mdivide_left_tri_aux_rev(ctx.ptr, 1, p, a["lda"], None, p, a["ldc"], p, a["ldca"], m, n, aadj,
                                                a["ldaa"], badj, a["ldba"], p)

    for k in ("lda", "ldb", "ldc"):
        assert fwd(**{k: m - 1}) == SMG_ERR_ARG, k
    for k in ("lda", "ldc", "ldca", "ldaa", "ldba"):
        assert rev(**{k: m - 1}) == SMG_ERR_ARG, k
