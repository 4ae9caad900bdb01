"""neg_binomial_2_log_glm_lpmf: the fused device pass smg_neg_binomial_2_log_glm
through ctypes, and the stan::math overloads through the tape
(tests/cpp/test_glm_neg_binomial.cpp).

The reference of every device test is `nb_ref` below, a float64 numpy / scipy
restatement of the formulas.  With theta = x beta + alpha, d = theta - log phi,
e = exp(-|d|):

    lse   = max(theta, log phi) + log1p(e)            (= log(exp theta + phi))
    s     = 1 / (1 + e) if d >= 0 else e / (1 + e)    (= exp theta / (exp theta + phi))
    1 - s = the same with the sign of d flipped
    A = sum (y + phi) lse        B = sum y theta
    C = sum lgamma(y + 1)        D = sum lgamma(y + phi)
    theta' = y - (y + phi) s     alpha' = sum theta'     beta' = x^T theta'
    phi' = sum (1 - (y + phi)(1 - s) / phi) + (log phi - lse) + (digamma(y + phi) - digamma(phi))
    logp = -C + N (phi log phi - lgamma phi) - A + B + D

`nb_ref` itself is checked against 50-digit mpmath without a GPU
(test_reference_against_mpmath).

Bounds.  Every sum is compared on the scale of the sum of its terms' absolute
values (`abs`): A, B, C, D, alpha', beta' within 1e-12 of it (alpha' and beta'
also pass within 1e-10 of their own value where that is looser), phi' within
1e-11 of sum_rows sum_three-groups |group|.  phi' cancels (at phi = 1e4 its
groups are each ~1e-4 in size while digamma and log phi are ~9), so no bound is
ever taken relative to phi' itself.  The yardstick test holds nb_ref to 5e-14
of the same scales (7e-13 for phi'): numpy's pairwise sum of R <= 1000 terms
rounds within ~10 x 2^-53 of the absolute sum, the terms themselves within a
few 2^-53 of their size, and the three groups of phi' within 2^-53 of
log phi / digamma(phi) ~ 9, i.e. 1e-15 / 3e-4 ~ 3e-12 per row at phi = 1e4,
random in sign, so ~3e-12 / sqrt(R) ~ 1e-13 of the absolute sum.

Inputs: x uniform in (-1, 1), beta = scale u / sum |u| with u uniform in (-1, 1),
alpha = 0.1 (|theta| < scale + 0.1), y = floor(exp(theta) (-log(1 - u))): an
exponentially mixed count, over-dispersed like the model.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
from scipy.special import digamma, gammaln

import gen
from _util import ROOT, check_sums, near_rel, prebuilt

gpu = pytest.mark.gpu

SMG_ERR_ARG = 16
ALPHA = 0.1
PHIS = [0.7, 30.0, 1e4]
FN = "neg_binomial_2_log_glm_lpmf"


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


# ------------------------------------------------------------ inputs and references
@functools.lru_cache(maxsize=None)
def inputs(R, M, scale=1.0):
    """x (R, M), y (R, int32), beta (M); read-only."""
    x = gen.unif(gen.SEED + 101 + 7 * R + M, R * M, -1.0, 1.0).reshape(M, R).T.copy()
    u = gen.unif(gen.SEED + 102 + M, M, -1.0, 1.0)
    beta = scale * u / max(np.abs(u).sum(), 1e-300)
    theta = x @ beta + ALPHA
    u = gen.u01(gen.SEED + 103 + R, R)
    y = np.floor(np.exp(theta) * -np.log1p(-u)).astype(np.int32)
    for a in (x, y, beta):
        a.setflags(write=False)
    return x, y, beta


def nb_ref(y, x, alpha, beta, phi):
    """The float64 restatement: {name: (value, sum of the terms' absolute values)}."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    theta = x @ np.asarray(beta, dtype=np.float64) + alpha if x.shape[1] else np.full(len(y), float(alpha))
    lphi = np.log(phi)
    d = theta - lphi
    e = np.exp(-np.abs(d))
    lse = np.maximum(theta, lphi) + np.log1p(e)
    inv = 1.0 / (1.0 + e)
    s = np.where(d >= 0, inv, e * inv)
    s1 = np.where(d >= 0, e * inv, inv)
    yp = y + phi
    tA, tB, tC, tD = yp * lse, y * theta, gammaln(y + 1.0), gammaln(yp)
    th = y - yp * s
    g1, g2, g3 = 1.0 - yp * s1 / phi, lphi - lse, digamma(yp) - digamma(phi)
    tb = x * th[:, None]
    return {
        "A": (tA.sum(), np.abs(tA).sum()), "B": (tB.sum(), np.abs(tB).sum()),
        "C": (tC.sum(), np.abs(tC).sum()), "D": (tD.sum(), np.abs(tD).sum()),
        "alpha'": (th.sum(), np.abs(th).sum()),
        "beta'": (tb.sum(axis=0), np.abs(tb).sum(axis=0)),
        "phi'": ((g1 + g2 + g3).sum(), (np.abs(g1) + np.abs(g2) + np.abs(g3)).sum()),
    }


def nb_mp(y, x, alpha, beta, phi):
    """The same sums from the defining expressions in 50-digit mpmath
    (exp(theta) formed directly: no overflow there)."""
    import mpmath as mp
    with mp.workdps(50):
        phi_ = mp.mpf(phi)
        R, M = x.shape
        z = mp.mpf(0)
        out = {k: [z, z] for k in ("A", "B", "C", "D", "alpha'", "phi'")}
        bsum, babs = [z] * M, [z] * M
        dg_phi = mp.digamma(phi_)

        def add(k, t):
            out[k][0] += t
            out[k][1] += abs(t)

        for i in range(R):
            yi = mp.mpf(int(y[i]))
            theta = mp.mpf(float(alpha))
            for j in range(M):
                theta += mp.mpf(float(x[i, j])) * mp.mpf(float(beta[j]))
            et = mp.exp(theta)
            lse = mp.log(et + phi_)
            s = et / (et + phi_)
            yp = yi + phi_
            add("A", yp * lse)
            add("B", yi * theta)
            add("C", mp.loggamma(yi + 1))
            add("D", mp.loggamma(yp))
            th = yi - yp * s
            add("alpha'", th)
            for j in range(M):
                t = mp.mpf(float(x[i, j])) * th
                bsum[j] += t
                babs[j] += abs(t)
            g = (1 - yp * (1 - s) / phi_, mp.log(phi_) - lse, mp.digamma(yp) - dg_phi)
            out["phi'"][0] += g[0] + g[1] + g[2]
            out["phi'"][1] += abs(g[0]) + abs(g[1]) + abs(g[2])
        res = {k: (float(v[0]), float(v[1])) for k, v in out.items()}
        res["beta'"] = (np.array([float(v) for v in bsum]), np.array([float(v) for v in babs]))
        return res


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("R,M,phi,scale", [(1000, 8, 0.7, 1.0), (1000, 8, 30.0, 1.0), (1000, 8, 1e4, 1.0),
                                           (257, 3, 2.5, 8.0)])  # theta within +-8, y up to ~1000
def test_reference_against_mpmath(R, M, phi, scale):
    """No GPU: nb_ref against 50-digit mpmath: every sum within 5e-14 of the sum
    of its terms' absolute values, phi' within 7e-13 of its own."""
    x, y, beta = inputs(R, M, scale)
    if scale > 1:
        assert 300 < y.max() < 10000 and 6 < np.abs(x @ beta + ALPHA).max() < 8.1
    ref = nb_ref(y, x, ALPHA, beta, phi)
    check_sums({k: v[0] for k, v in ref.items()}, nb_mp(y, x, ALPHA, beta, phi), f"ref vs mpmath {R}x{M} phi={phi}",
               b_sum=5e-14, b_phi=7e-13, b_rel=None)


# ------------------------------------------------------------ 2. the C entry
def nb_dev(ctx, y, x, alpha, beta, phi, ldx=None, twice=True):
    """smg_neg_binomial_2_log_glm -> {name: value}; x is stored with leading
    dimension ldx, the padding rows NaN; two calls must agree bitwise."""
    R, M = x.shape
    ldx = R if ldx is None else ldx
    xf = np.full((ldx, M), np.nan)
    xf[:R] = x
    abp = np.concatenate([[alpha], beta, [phi]])
    ws = ctx.zeros(int(ctx.lib.smg_neg_binomial_2_log_glm_ws_doubles(R, M)))
    dy = ctx.put(np.ascontiguousarray(y, dtype=np.int32)) if R else None
    dx = ctx.put(F(xf)) if R * M else None
    dab = ctx.put(abp)
    outs = []
    for _ in range(2 if twice else 1):
        out = ctx.put(np.full(M + 6, np.nan))
        ctx.call("smg_neg_binomial_2_log_glm", dy, dx, R, M, ldx, dab, ws, out)
        outs.append(ctx.get(out, M + 6))
    if twice:
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), "two calls differ bitwise"
    o = outs[0]
    return {"A": o[0], "alpha'": o[1], "beta'": o[2:M + 2], "B": o[M + 2], "C": o[M + 3], "D": o[M + 4],
            "phi'": o[M + 5]}


SHAPES = [(1, 8, None), (31, 8, None), (32, 8, None), (33, 8, None),
          (97, 0, None), (97, 1, None), (97, 17, None), (97, 255, None), (97, 256, None),
          (33, 8, 38),          # ldx = R + 5, NaN padding
          (40003, 8, None)]     # 1251 tiles over 512 workgroups: both register buffers and the wrap


@gpu
@pytest.mark.parametrize("phi", PHIS)
@pytest.mark.parametrize("R,M,ldx", SHAPES)
def test_entry_against_reference(ctx, R, M, ldx, phi):
    x, y, beta = inputs(R, M)
    got = nb_dev(ctx, y, x, ALPHA, beta, phi, ldx)
    check_sums(got, nb_ref(y, x, ALPHA, beta, phi), f"entry {R}x{M} ldx={ldx} phi={phi}")


@gpu
def test_entry_wide_predictor(ctx):
    """The 257 x 3 case of the yardstick test (|theta| up to ~8, y up to
    ~1000) on the device."""
    x, y, beta = inputs(257, 3, 8.0)
    check_sums(nb_dev(ctx, y, x, ALPHA, beta, 2.5), nb_ref(y, x, ALPHA, beta, 2.5), "entry 257x3 scale 8")


@gpu
def test_entry_argument_errors_and_empty(ctx):
    """M = 257, ldx < R, null abp: SMG_ERR_ARG (16), the context's status
    untouched; R = 0 writes M + 6 zeros."""
    R, M = 33, 8
    x, y, beta = inputs(R, M)
    lib = ctx.lib
    ws = ctx.zeros(int(lib.smg_neg_binomial_2_log_glm_ws_doubles(R, 257)))
    dy, dx = ctx.put(y), ctx.put(F(x))
    dab = ctx.put(np.concatenate([[ALPHA], beta, [2.5], np.zeros(257)]))
    out = ctx.put(np.full(M + 6, np.nan))
    assert lib.smg_neg_binomial_2_log_glm(ctx.ptr, dy, dx, R, 257, R, dab, ws, out) == SMG_ERR_ARG
    assert lib.smg_neg_binomial_2_log_glm(ctx.ptr, dy, dx, R, M, R - 1, dab, ws, out) == SMG_ERR_ARG
    assert lib.smg_neg_binomial_2_log_glm(ctx.ptr, dy, dx, R, M, R, None, ws, out) == SMG_ERR_ARG
    assert np.all(np.isnan(ctx.get(out, M + 6)))  # nothing was written
    assert ctx.status() == 0
    ctx.call("smg_neg_binomial_2_log_glm", None, None, 0, M, 0, dab, ws, out)
    assert np.array_equal(ctx.get(out, M + 6), np.zeros(M + 6))


# ------------------------------------------------------------ 3. extremes
@gpu
@pytest.mark.parametrize("alpha", [800.0, 0.0, -800.0])
def test_entry_extreme_predictors(ctx, alpha):
    """One column, beta = 1, x in {-20, 20, 0, -40, 40}, so theta is near +-800,
    +-40 and 0 over the three intercepts; y in {0, 1, 1000, 2^31 - 1}; phi =
    2.5.  Every output is finite and within the bounds of the mpmath reference
    (the reference implementation is NaN beyond theta = 709: a deliberate,
    documented difference)."""
    R = 64
    x = np.array([-20.0, 20.0, 0.0, -40.0, 40.0])[np.arange(R) % 5].reshape(R, 1)
    y = np.array([0, 1, 1000, 2**31 - 1], dtype=np.int64)[np.arange(R) % 4].astype(np.int32)
    beta = np.array([1.0])
    got = nb_dev(ctx, y, x, alpha, beta, 2.5)
    for k, v in got.items():
        assert np.all(np.isfinite(v)), (k, v)
    check_sums(got, nb_mp(y, x, alpha, beta, 2.5), f"extremes alpha={alpha}")


# ------------------------------------------------------------ 4. through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_glm_neg_binomial")
TAPE = (1000, 8, 0.7)
KINDS = ["vvv", "vvd", "vdv", "dvv", "vdd", "dvd", "ddv"]


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@functools.lru_cache(maxsize=None)
def tape():
    """One run of the binary's "tape" mode at TAPE, shared by the tests below:
    ({tag: values}, the reference sums)."""
    R, M, phi = TAPE
    x, y, beta = inputs(R, M)
    nums = np.concatenate([y.astype(np.float64), F(x), [ALPHA], beta, [phi]])
    out = _run(f"tape {R} {M}\n" + " ".join(repr(float(v)) for v in nums) + "\n")
    res = {}
    for line in out.strip().splitlines():
        tag, *vals = line.split()
        res[tag] = np.array([float(v) for v in vals])
    return res, nb_ref(y, x, ALPHA, beta, phi)


def logp_terms(ref, N, phi):
    """(-C, N (phi log phi - lgamma phi) + D, B, -A) and the absolute-term sum of logp."""
    norm = N * (phi * np.log(phi) - gammaln(phi))
    t = (-ref["C"][0], norm + ref["D"][0], ref["B"][0], -ref["A"][0])
    return t, ref["C"][1] + abs(norm) + ref["D"][1] + ref["B"][1] + ref["A"][1]


def check_grad(g, kinds, ref, what):
    """The gradient over the var arguments of `kinds` within the entry's bounds."""
    M = len(ref["beta'"][0])
    at, got = 0, {}
    if kinds[0] == "v":
        got["alpha'"] = g[0]
        at = 1
    if kinds[1] == "v":
        got["beta'"] = g[at:at + M]
        at += M
    if kinds[2] == "v":
        got["phi'"] = g[at]
        at += 1
    assert at == len(g), (kinds, len(g))
    check_sums(got, ref, what)


@gpu
@pytest.mark.parametrize("kinds", KINDS)
def test_tape_every_kind_and_propto(kinds):
    """Full density and gradient for each var / double combination of (alpha,
    beta, phi), and the propto variant: -C dropped, N (phi log phi - lgamma
    phi) + D kept when phi is a var, B when alpha or beta is; the partials are
    complete either way."""
    r, ref = tape()
    R, M, phi = TAPE
    (mC, nD, B, mA), scale = logp_terms(ref, R, phi)
    fx = r["fx_" + kinds][0]
    print(f"tape {kinds}: |fx - ref| / abs-term sum = {abs(fx - (mC + nD + B + mA)) / scale:.3e}")
    assert abs(fx - (mC + nD + B + mA)) <= 1e-12 * scale
    check_grad(r["grad_" + kinds], kinds, ref, f"tape {kinds}")
    want = mA + (nD if kinds[2] == "v" else 0.0) + (B if "v" in kinds[:2] else 0.0)
    assert abs(r["fxp_" + kinds][0] - want) <= 1e-12 * scale, (kinds, r["fxp_" + kinds][0], want)
    assert np.array_equal(r["gradp_" + kinds], r["grad_" + kinds])


@gpu
def test_tape_all_double_and_stack():
    r, ref = tape()
    R, M, phi = TAPE
    (mC, nD, B, mA), scale = logp_terms(ref, R, phi)
    assert abs(r["fx_ddd"][0] - (mC + nD + B + mA)) <= 1e-12 * scale
    assert r["fx_ddd"][0] == r["fx_vvv"][0]
    assert r["fxp_ddd"][0] == 0.0
    assert r["fx_eigen_ddd"][0] == r["fx_ddd"][0]
    assert list(r["stack"]) == [0.0, 0.0]


@gpu
def test_tape_shards_distributed_eigen_host_leaf():
    """Seven row shards summed on one tape (each its own N) equal the single
    call: fx within 1e-12 of the absolute-term sum, the gradient within the
    entry's bounds; one distributed shard under a one-rank host collective, the
    Eigen signature and host vectors give the plain call's bits; beta as the
    device leaf of gradient() gives beta'."""
    r, ref = tape()
    R, M, phi = TAPE
    (mC, nD, B, mA), scale = logp_terms(ref, R, phi)
    assert abs(r["fx_shards7"][0] - (mC + nD + B + mA)) <= 1e-12 * scale
    assert abs(r["fx_shards7"][0] - r["fx_vvv"][0]) <= 1e-12 * scale
    check_grad(r["grad_shards7"], "vvv", ref, "tape shards7")
    for tag in ("dist", "eigen", "host"):
        assert r["fx_" + tag][0] == r["fx_vvv"][0], tag
        assert np.array_equal(r["grad_" + tag], r["grad_vvv"]), tag
    assert r["fx_leaf"][0] == r["fx_vvv"][0]
    assert np.array_equal(r["grad_leaf"], r["grad_vvv"][1:M + 1])


@gpu
def test_tape_gradient_against_central_differences():
    """Central differences of the all-double form with h = 1e-5 max(1,
    |theta_i|) at 1e-6 (relative, absolute below 1 in magnitude: _util.near_rel).
    The difference quotient is good to ~1e-7 absolute: truncation h^2 f''' / 6
    with f''' of order R = 1000, round-off 1e-15 of logp's absolute-term sum
    (~1e4) over 2 h."""
    r, _ = tape()
    near_rel(r["grad_vvv"], r["grad_fd"], 1e-6, what="gradient vs central differences")


# ------------------------------------------------------------ 5. errors
@functools.lru_cache(maxsize=None)
def errors():
    got = {}
    for line in _run("errors\n").strip().splitlines():
        case, kind, msg = line.split("|", 2)
        got[case] = (kind, msg)
    return got


SIZES = ("; a function was called with arguments of different scalar, array, vector, or matrix types, and they "
         "were not consistently sized;  all arguments must be scalars or multidimensional values of the same shape.")


@gpu
def test_cpp_argument_errors():
    """The checks in the reference's order, message for message (as recalled
    from Stan Math 3.0.0), thrown with the tape left empty."""
    e = errors()
    assert e["ok"][0] == "value" and np.isfinite(float(e["ok"][1]))
    assert e["negative_y"] == ("domain_error", f"{FN}: Failures variables[3] is -2, but must be >= 0!")
    assert e["negative_y_and_phi"] == e["negative_y"]  # y is checked before phi
    assert e["phi_zero"] == ("domain_error", f"{FN}: Precision parameter is 0, but must be > 0!")
    assert e["phi_negative"] == ("domain_error", f"{FN}: Precision parameter is -1, but must be > 0!")
    assert e["phi_negative_double"] == e["phi_negative"]
    assert e["phi_inf"] == ("domain_error", f"{FN}: Precision parameter is inf, but must be finite!")
    assert e["phi_nan"] == ("domain_error", f"{FN}: Precision parameter is nan, but must be > 0!")
    assert e["beta_size"] == ("invalid_argument",
                              f"{FN}: Weight vector has dimension = 3, expecting dimension = 2" + SIZES)
    assert e["y_size"] == ("invalid_argument",
                           f"{FN}: Vector of dependent variables has dimension = 3, expecting dimension = 4" + SIZES)
    assert e["y_size_eigen"] == e["y_size"]
    assert e["nonfinite_beta"] == ("domain_error", f"{FN}: Weight vector[1] is inf, but must be finite!")
    assert e["nonfinite_alpha"] == ("domain_error", f"{FN}: Intercept is -inf, but must be finite!")
    assert e["nonfinite_x"] == ("domain_error",
                                f"{FN}: Matrix of independent variables is not finite, but must be finite!")
    assert e["empty_y"] == ("value", "0")
    assert e["all_data_propto"] == ("value", "0")
    assert e["stack"] == ("0", "0")
