"""One intercept per row in the fused GLM reducers: the device entry
smg_glm_vec_intercept through ctypes (kinds 0 bernoulli_logit, 1 normal_id, 2
poisson_log, 3 neg_binomial_2_log), and the stan::math overloads through the
tape (tests/cpp/test_glm_vec_intercept.cpp).

The reference of every device test is `_glm_vec_intercept.vec_ref`, the float64
restatement with theta_i = x_i beta + alpha_i; it is itself held to 50-digit
mpmath without a GPU (test_reference_against_mpmath).

Bounds (the project's, _util.check_sums): every reduced sum within 1e-12 of the
sum of its terms' absolute values (alpha' and beta' also within 1e-10 of their
own value where that is looser), phi' within 1e-11 of its own.  The per-row
theta' that the entry stores is one term of the sum alpha', so it is held to
the same 1e-12 of the row's own terms' absolute values (the scales are listed
in _glm_vec_intercept).  The yardstick holds the reference to 5e-14 of the
same scales, 7e-13 for phi'.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from _glm_vec_intercept import (F, KINDS, NAMES, SENTINEL, ab_of, extra_of, inputs, out_width, scalar_dev,
                                split_out, vec_dev, vec_mp, vec_ref, ws_doubles)
from _reducers import same_bits
from _util import ROOT, check_sums, prebuilt, worst

gpu = pytest.mark.gpu

SMG_ERR_ARG = 16
B_ROW = 1e-12


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


def check_rows(th, ref_th, scale, what):
    r = worst(th, ref_th, scale)
    print(f"{what} theta' per row: worst |diff| / row abs-term sum = {r:.3e}")
    assert r <= B_ROW, (what, r)


def check_entry(kind, out, th, ref, M, what):
    sums, rth, rsc = ref
    got = split_out(kind, out, M)
    check_sums(got, sums, what)
    if kind == 0:
        assert got["bad y"] == 0.0
    if th is not None:
        check_rows(th, rth, rsc, what)


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,M", [(200, 0), (200, 5)])
def test_reference_against_mpmath(kind, R, M):
    """No GPU: vec_ref against 50-digit mpmath, every sum within 5e-14 of the sum
    of its terms' absolute values, phi' within 7e-13, theta' per row within
    5e-14 of the row's scale."""
    x, y, beta, av = inputs(kind, R, M)
    sums, th, tsc = vec_ref(kind, y, x, av, beta, extra_of(kind))
    mp_sums, mp_th = vec_mp(kind, y, x, av, beta, extra_of(kind))
    check_sums({k: v[0] for k, v in sums.items()}, mp_sums, f"ref vs mpmath {NAMES[kind]} {R}x{M}",
               b_sum=5e-14, b_phi=7e-13, b_rel=None)
    r = worst(th, mp_th, tsc)
    print(f"ref vs mpmath {NAMES[kind]} {R}x{M} theta' per row = {r:.3e}")
    assert r <= 5e-14


# ------------------------------------------------------------ 2. the C entry
SHAPES = [(1, 0, None), (1, 1, None), (31, 3, None), (32, 16, None), (33, 17, None), (1000, 8, None),
          (1000, 256, None),
          (40003, 5, None),     # 1251 tiles over 512 workgroups: both register buffers, the wrap, a partial tile
          (33, 17, 38)]         # ldx = R + 5, NaN in the padding rows


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,M,ldx", SHAPES)
def test_entry_against_reference(ctx, kind, R, M, ldx):
    x, y, beta, av = inputs(kind, R, M)
    ex = extra_of(kind)
    out, th = vec_dev(ctx, kind, y, x, av, beta, ex, ldx)
    check_entry(kind, out, th, vec_ref(kind, y, x, av, beta, ex), M, f"entry {NAMES[kind]} {R}x{M} ldx={ldx}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,M", [(1000, 8), (40003, 5)])
def test_constant_vector_equals_scalar_entry(ctx, kind, R, M):
    """alpha_vec == 0.1 gives the bits of the kind's scalar entry at alpha = 0.1
    (kind 0: _checked): the same arithmetic in the same reduction order; the
    stored theta' sum to out[1] within 1e-12 of sum |theta'|."""
    x, y, beta, _ = inputs(kind, R, M)
    ex = extra_of(kind)
    out, th = vec_dev(ctx, kind, y, x, np.full(R, 0.1), beta, ex, calls=1)
    assert same_bits(out, scalar_dev(ctx, kind, y, x, 0.1, beta, ex))
    r = abs(th.sum() - out[1]) / np.abs(th).sum()
    print(f"constant vector {NAMES[kind]} {R}x{M}: |sum theta_adj - out[1]| / sum |theta'| = {r:.3e}")
    assert r <= 1e-12


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_null_theta_adj_same_bits(ctx, kind):
    R, M = 40003, 5
    x, y, beta, av = inputs(kind, R, M)
    ex = extra_of(kind)
    a, _ = vec_dev(ctx, kind, y, x, av, beta, ex, calls=1)
    b, th = vec_dev(ctx, kind, y, x, av, beta, ex, want_theta=False, calls=1)
    assert th is None and same_bits(a, b)


@gpu
@pytest.mark.parametrize("phi", [0.7, 1e4])
def test_kind3_large_intercepts(ctx, phi):
    """alpha_vec rows at +-800 (and at the ordinary values between): every
    output is finite and within the bounds of the mpmath sums."""
    R, M = 64, 3
    x, y, beta, av = inputs(3, R, M)
    av = av.copy()
    av[0::4], av[1::4] = 800.0, -800.0
    y = y.copy()
    y[0::8] = 1000
    out, th = vec_dev(ctx, 3, y, x, av, beta, phi)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(th))
    mp_sums, mp_th = vec_mp(3, y, x, av, beta, phi)
    check_sums(split_out(3, out, M), mp_sums, f"kind 3 alpha +-800 phi={phi}")
    check_rows(th, mp_th, vec_ref(3, y, x, av, beta, phi)[2], f"kind 3 alpha +-800 phi={phi}")


@gpu
def test_kind0_off_support_y_is_counted(ctx):
    R, M = 1000, 8
    x, y, beta, av = inputs(0, R, M)
    y = y.copy()
    y[[3, 500, 999]] = [2, -1, 7]
    out, _ = vec_dev(ctx, 0, y, x, av, beta)
    assert out[M + 2] == 3.0


@gpu
def test_kind0_generic_path_m257(ctx):
    """Bernoulli at M = 257: GEMM, the row pass with a vector intercept, GEMM."""
    R, M = 1000, 257
    x, y, beta, av = inputs(0, R, M)
    out, th = vec_dev(ctx, 0, y, x, av, beta)
    check_entry(0, out, th, vec_ref(0, y, x, av, beta), M, "entry bernoulli_logit 1000x257 (generic)")
    y2 = y.copy()
    y2[17] = 5
    assert vec_dev(ctx, 0, y2, x, av, beta, calls=1)[0][M + 2] == 1.0


@gpu
def test_entry_argument_errors_and_empty(ctx):
    """A bad kind, a null alpha_vec with R > 0, M = 257 for kinds 1-3 and the
    scalar entries' argument errors: SMG_ERR_ARG, nothing written, the
    context's status untouched; R = 0 writes zeros."""
    R, M = 33, 8
    lib = ctx.lib
    f = lib.smg_glm_vec_intercept
    for kind in KINDS:
        x, y, beta, av = inputs(kind, R, M)
        W = out_width(kind, M)
        ws = ctx.zeros(max(ws_doubles(lib, kind, R, 257), ws_doubles(lib, kind, R, M)))
        dy = ctx.put(np.ascontiguousarray(y, dtype=np.float64 if kind == 1 else np.int32))
        dx, dav = ctx.put(F(x)), ctx.put(av)
        dab = ctx.put(np.concatenate([ab_of(kind, beta, extra_of(kind)), np.zeros(300)]))
        out = ctx.put(np.full(W, np.nan))
        dth = ctx.put(np.full(R, SENTINEL))
        for bad in (-1, 4):
            assert f(ctx.ptr, bad, dy, dx, R, M, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, R, M, R, None, dab, ws, out, dth) == SMG_ERR_ARG
        if kind:
            assert f(ctx.ptr, kind, dy, dx, R, 257, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, R, M, R - 1, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, -1, M, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, R, -1, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, None, dx, R, M, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, None, R, M, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, R, M, R, dav, None, ws, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, R, M, R, dav, dab, None, out, dth) == SMG_ERR_ARG
        assert f(ctx.ptr, kind, dy, dx, R, M, R, dav, dab, ws, None, dth) == SMG_ERR_ARG
        assert f(None, kind, dy, dx, R, M, R, dav, dab, ws, out, dth) == SMG_ERR_ARG
        assert np.all(np.isnan(ctx.get(out, W)))  # nothing was written
        assert np.all(ctx.get(dth, R) == SENTINEL)
        assert ctx.status() == 0
        ctx.call("smg_glm_vec_intercept", kind, None, None, 0, M, 0, None, dab, ws, out, None)
        assert np.array_equal(ctx.get(out, W), np.zeros(W))
        assert ctx.status() == 0


# ------------------------------------------------------------ 3. through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_glm_vec_intercept")
TAPE = (1000, 8)
GP_N = 64
FNS = {0: "bernoulli_logit_glm_lpmf", 1: "normal_id_glm_lpdf", 2: "poisson_log_glm_lpmf",
       3: "neg_binomial_2_log_glm_lpmf"}
NEG_LOG_SQRT_TWO_PI = -0.91893853320467274178


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@functools.lru_cache(maxsize=None)
def gp_inputs():
    """The latent GP's inputs: x (N) evenly spaced over (-3, 3) with a jitter,
    sigma = 1.1, l = 0.6, eta uniform in (-1, 1), and y drawn at f = L eta (a
    count at exp(f), a Bernoulli at logistic(f))."""
    import gen
    N = GP_N
    x = np.linspace(-3.0, 3.0, N) + gen.unif(gen.SEED + 301, N, -0.02, 0.02)
    sigma, l = 1.1, 0.6
    eta = gen.unif(gen.SEED + 302, N, -1.0, 1.0)
    K = sigma**2 * np.exp(-0.5 * (x[:, None] - x[None, :])**2 / l**2) + 1e-6 * np.eye(N)
    f = np.linalg.cholesky(K) @ eta
    u = gen.u01(gen.SEED + 303, N)
    yc = np.floor(np.exp(f) * -np.log1p(-u))
    yb = (gen.u01(gen.SEED + 304, N) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64)
    return x, sigma, l, eta, yc, yb


@functools.lru_cache(maxsize=None)
def tape():
    """One run of the binary's "tape" mode at TAPE, shared by the tests below:
    ({tag: values}, {kind: vec_ref's result})."""
    R, M = TAPE
    ins = {k: inputs(k, R, M) for k in KINDS}
    x, _, beta, av = ins[0]
    x_, sigma, l, eta, yc, yb = gp_inputs()
    nums = np.concatenate([F(x), beta, av, [extra_of(1), extra_of(3)]] + [np.asarray(ins[k][1], dtype=np.float64)
                                                                          for k in KINDS])
    gp = np.concatenate([x_, [sigma, l], eta, yc, yb])
    out = _run(f"tape {R} {M}\n" + " ".join(repr(float(v)) for v in nums) + f"\ngp {GP_N}\n" +
               " ".join(repr(float(v)) for v in gp) + "\n")
    res = {}
    for line in out.strip().splitlines():
        tag, *vals = line.split()
        res[tag] = np.array([float(v) for v in vals])
    return res, {k: vec_ref(k, ins[k][1], x, av, beta, extra_of(k)) for k in KINDS}


def value_terms(kind, sums, N, propto=False, extra_var=True, any_var=True):
    """(logp, the sum of its terms' absolute values) as the kind composes it,
    and what propto keeps: kind 0 everything; kind 1 -N log sigma with a var
    sigma and the quadratic term; kind 2 nothing (the reference's
    include_summand<propto, double>: the value is 0, the partials stay); kind
    3 N (phi log phi - lgamma phi) + D with a var phi, B with a var alpha or
    beta, and -A."""
    from scipy.special import gammaln
    if kind == 0:
        return sums["value"]
    if kind == 1:
        sq, sq_abs = sums["value"]
        t = [] if propto else [NEG_LOG_SQRT_TWO_PI * N]
        if not propto or extra_var:
            t.append(-N * np.log(extra_of(1)))
        t.append(-0.5 * sq)
        return sum(t), sum(abs(v) for v in t[:-1]) + 0.5 * sq_abs
    if kind == 2:
        if propto:
            return 0.0, 0.0
        return sums["value"][0] - sums["lgamma"][0], sums["value"][1] + sums["lgamma"][1]
    phi = extra_of(3)
    norm = N * (phi * np.log(phi) - gammaln(phi))
    v, sc = -sums["A"][0], sums["A"][1]
    if not propto:
        v, sc = v - sums["C"][0], sc + sums["C"][1]
    if not propto or extra_var:
        v, sc = v + norm + sums["D"][0], sc + abs(norm) + sums["D"][1]
    if not propto or any_var:
        v, sc = v + sums["B"][0], sc + sums["B"][1]
    return v, sc


def check_value(fx, want, scale, what):
    r = 0.0 if fx == want else abs(fx - want) / max(scale, 1e-300)
    print(f"{what}: |fx - ref| / abs-term sum = {r:.3e}")
    assert r <= 1e-12, (what, fx, want)


def check_grad(kind, g, ref, alpha_var, beta_var, what):
    """[alpha'(R)][beta'(M)][sigma' | phi'] within the entry's bounds; sigma' =
    (sum y_scaled^2 - N) / sigma within 1e-12 of (sum y_scaled^2 + N) / sigma."""
    sums, th, tsc = ref
    R, M = TAPE
    at = 0
    if alpha_var:
        check_rows(g[:R], th, tsc, what)
        at = R
    if beta_var:
        got = {"beta'": g[at:at + M]}
        at += M
        if kind == 3:
            got["phi'"] = g[at]
            at += 1
        check_sums(got, sums, what)
        if kind == 1:
            sq, sq_abs = sums["value"]
            s = extra_of(1)
            r = worst(g[at], (sq - R) / s, (sq_abs + R) / s)
            print(f"{what} sigma': |diff| / abs-term sum = {r:.3e}")
            assert r <= 1e-12
            at += 1
    assert at == len(g), (what, at, len(g))


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b", ["v", "d"])
def test_tape_every_alpha_form(kind, b):
    """alpha as std::vector<var> (hv), dev_var_matrix (dv), std::vector<double>
    (hd), dev_data<double> (dd), with beta (and sigma / phi) var or data: value
    and gradient against the reference; the four forms' values are bit-equal,
    dv's gradient agrees with hv's within the bounds.  propto keeps the
    gradient's bits for every kind.  Its value keeps the bits only where the
    kind drops nothing, which is bernoulli_logit alone, with any var operand:
    normal_id always drops N log sqrt(2 pi), poisson_log's value is 0 under
    propto (the reference's include_summand<propto, double>), neg_binomial
    always drops sum lgamma(y + 1) -- each kind's rule from before this
    change -- so for kinds 1-3 the propto value is held to the summands that
    stay (value_terms) at 1e-12, and poisson's to exactly 0.  Every operand
    data: a double equal to the var forms' value, and 0 with propto."""
    r, refs = tape()
    ref = refs[kind]
    R, M = TAPE
    bv = b == "v"
    want, scale = value_terms(kind, ref[0], R)
    for a in ("hv", "dv"):
        tag = f"{kind}_{a}_{b}"
        check_value(r["fx_" + tag][0], want, scale, f"tape {NAMES[kind]} {a} {b}")
        check_grad(kind, r["grad_" + tag], ref, True, bv, f"tape {NAMES[kind]} {a} {b}")
        assert np.array_equal(r["gradp_" + tag], r["grad_" + tag])
        wp, sp = value_terms(kind, ref[0], R, propto=True, extra_var=bv)
        if kind == 0:
            assert r["fxp_" + tag][0] == r["fx_" + tag][0]
        elif kind == 2:
            assert r["fxp_" + tag][0] == 0.0
        else:
            check_value(r["fxp_" + tag][0], wp, sp, f"tape propto {NAMES[kind]} {a} {b}")
    assert r[f"fx_{kind}_dv_{b}"][0] == r[f"fx_{kind}_hv_{b}"][0]
    check_rows(r[f"grad_{kind}_dv_{b}"][:R], r[f"grad_{kind}_hv_{b}"][:R], ref[2], f"dv vs hv {NAMES[kind]} {b}")
    if bv:
        assert np.array_equal(r[f"grad_{kind}_dv_v"][R:], r[f"grad_{kind}_hv_v"][R:])
        for a in ("hd", "dd"):
            tag = f"{kind}_{a}_v"
            assert r["fx_" + tag][0] == r[f"fx_{kind}_hv_v"][0]
            check_grad(kind, r["grad_" + tag], ref, False, True, f"tape {NAMES[kind]} {a} v")
            assert np.array_equal(r["gradp_" + tag], r["grad_" + tag])
            assert np.array_equal(r["grad_" + tag], r[f"grad_{kind}_hv_v"][R:])
    else:
        for a in ("hd", "dd"):
            assert r[f"fx_{kind}_{a}_d"][0] == r[f"fx_{kind}_hv_v"][0]
            assert r[f"fxp_{kind}_{a}_d"][0] == 0.0


@gpu
def test_tape_one_device_alpha_two_calls():
    """One dev_var_matrix alpha feeds a poisson and a neg_binomial call on one
    tape: its adjoint is the sum of the two theta' (the second axpy adds to
    the first write of the lazily cleared device adjoint)."""
    r, refs = tape()
    check_rows(r["grad_two"], refs[2][1] + refs[3][1], refs[2][2] + refs[3][2], "two calls on one device alpha")
    assert r["fx_two"][0] == r["fx_2_dv_d"][0] + r["fx_3_dv_d"][0]


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_tape_shards_distributed_eigen_host(kind):
    """Seven row shards, each with its slice of alpha (as host vars and as a
    device vector in turn), summed on one tape: the single call within the
    entry's bounds, alpha' in row order; one distributed shard under a
    one-rank host collective, the Eigen signatures and host vectors give the
    dev_data call's bits."""
    r, refs = tape()
    ref = refs[kind]
    R, M = TAPE
    want, scale = value_terms(kind, ref[0], R)
    check_value(r[f"fx_{kind}_shards7"][0], want, scale, f"shards7 {NAMES[kind]}")
    check_value(r[f"fx_{kind}_shards7"][0], r[f"fx_{kind}_hv_v"][0], scale, f"shards7 vs single {NAMES[kind]}")
    check_grad(kind, r[f"grad_{kind}_shards7"], ref, True, True, f"shards7 {NAMES[kind]}")
    for tag in ("dist", "eigen", "host"):
        assert r[f"fx_{kind}_{tag}"][0] == r[f"fx_{kind}_hv_v"][0], tag
        assert np.array_equal(r[f"grad_{kind}_{tag}"], r[f"grad_{kind}_hv_v"]), tag
    assert r[f"fx_{kind}_eigenrow"][0] == r[f"fx_{kind}_hd_d"][0]


@gpu
@pytest.mark.parametrize("which", ["p", "b"])
def test_tape_latent_gp(which):
    """f = multiply(cholesky_decompose(K + 1e-6 I), to_dev(eta)) as the
    intercepts of a GLM without columns (poisson_log, bernoulli_logit) plus
    normal_lpdf(eta | 0, 1): the gradient over (sigma, l, eta) against the same
    model with f brought to the host, within 1e-12 of max(|entry|, 1e-3
    |gradient|_inf); the stacks are empty afterwards."""
    r, _ = tape()
    gd, gh = r[f"grad_gp_{which}_dev"], r[f"grad_gp_{which}_host"]
    assert len(gd) == GP_N + 2 and np.all(np.isfinite(gd))
    scale = np.maximum(np.abs(gh), 1e-3 * np.abs(gh).max())
    ratio = np.abs(gd - gh) / scale
    print(f"latent GP {which}: worst |dev - host| / scale = {ratio.max():.3e}")
    assert ratio.max() <= 1e-12
    fd, fh = r[f"fx_gp_{which}_dev"][0], r[f"fx_gp_{which}_host"][0]
    assert abs(fd - fh) <= 1e-12 * abs(fh)
    assert list(r["stack"]) == [0.0, 0.0]


# ------------------------------------------------------------ 4. errors
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
@pytest.mark.parametrize("kind", KINDS)
def test_cpp_argument_errors(kind):
    """The vector intercept's checks in their order, with the tape left empty:
    its size after the weight vector's (a device matrix that is neither a
    column nor a row, and a default-constructed one, are refused there); in
    the non-finite path beta, then
    alpha's first offender (1-based), a device alpha downloaded for it; the y
    domain still first; an empty y returns 0."""
    e = errors()
    fn = FNS[kind]
    k = f"{kind}_"
    for case in ("ok", "ok_dev"):
        assert e[k + case][0] == "value" and np.isfinite(float(e[k + case][1]))
    assert e[k + "ok_dev"] == e[k + "ok"]
    size = ("invalid_argument", f"{fn}: Vector of intercepts has dimension = 3, expecting dimension = 4" + SIZES)
    assert e[k + "alpha_size"] == size
    assert e[k + "alpha_size_dev"] == size
    assert e[k + "alpha_size_eigen"] == size
    assert e[k + "alpha_matrix_dev"] == (
        "invalid_argument", f"{fn}: Vector of intercepts must be a column or a row vector, but is 2 x 2")
    assert e[k + "alpha_null_dev"] == (
        "invalid_argument", f"{fn}: Vector of intercepts has dimension = 0, expecting dimension = 4" + SIZES)
    assert e[k + "alpha_and_beta_size"] == ("invalid_argument",
                                            f"{fn}: Weight vector has dimension = 3, expecting dimension = 2" + SIZES)
    nonfinite = ("domain_error", f"{fn}: Intercept[2] is inf, but must be finite!")
    assert e[k + "alpha_inf"] == nonfinite
    assert e[k + "alpha_inf_dev"] == nonfinite
    assert e[k + "alpha_inf_data"] == nonfinite
    assert e[k + "beta_and_alpha_inf"] == ("domain_error", f"{fn}: Weight vector[1] is inf, but must be finite!")
    if kind == 0:
        assert e[k + "y_domain_and_alpha_inf"] == (
            "domain_error", f"{fn}: Vector of dependent variables[3] is 2, but must be in the interval [0, 1]")
    elif kind == 2:
        assert e[k + "y_domain_and_alpha_inf"] == (
            "domain_error", f"{fn}: Vector of dependent variables[3] is -2, but must be >= 0!")
    elif kind == 3:
        assert e[k + "y_domain_and_alpha_inf"] == ("domain_error", f"{fn}: Failures variables[3] is -2, but must be >= 0!")
    assert e[k + "empty_y"] == ("value", "0")
    assert e["stack"] == ("0", "0")
