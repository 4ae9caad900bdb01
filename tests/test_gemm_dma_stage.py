"""The 64 x 64 GEMM tile's two staging paths (smg_set_gemm_stage_mode: 1 =
through registers, 2 = LDS-DMA wherever the product is eligible) against numpy
and against each other.

Bound of the numpy comparisons, elementwise:
    |C - C_ref| <= 2 gamma_K (|alpha| |op A| |op B| + |beta| |C0|),
    gamma_K = K u / (1 - K u), u = 2^-53
-- the a-priori bound of a K-term inner product in any summation order,
doubled because the float64 reference carries the same error
(test_reference_inside_gamma confirms that against np.longdouble on the very
inputs used).
"""
import functools

import numpy as np
import pytest

from _util import golden, near_rel

U = 2.0 ** -53
KINDS = {"NT-lower": (0, 1, 1), "TN-lower": (1, 0, 1), "NN-full": (0, 0, 0)}
SHAPES = [(64, 64, 64), (128, 128, 64), (192, 128, 128), (256, 256, 512), (320, 64, 192)]
COEFFS = [(-1.0, 1.0), (1.5, -0.5)]


def gamma(k):
    return k * U / (1.0 - k * U)


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
    c.call("smg_set_gemm_stage_mode", 0)
    assert c.status() == 0
    c.rewind(m)


class View:
    """A rows x cols block at (r0, c0) of a column-major backing matrix."""

    def __init__(self, back, r0, c0, rows, cols):
        self.back, self.r0, self.c0, self.rows, self.cols = back, r0, c0, rows, cols
        self.ld = back.shape[0]

    @property
    def a(self):
        return self.back[self.r0:self.r0 + self.rows, self.c0:self.c0 + self.cols]

    def dev(self, base):
        return base + 8 * (self.r0 + self.c0 * self.ld)


def backing(rng, rows, cols):
    return np.asfortranarray(rng.uniform(-1.0, 1.0, (rows, cols)))


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k):
    """Operands as views at 64-multiple offsets of backing matrices with
    leading dimensions larger than their rows; a lower trapezoid (m > n) takes
    A and B from ONE matrix, B being A's first n rows (NT) / columns (TN), as
    the Cholesky's look-ahead update passes them.  Returns the views, op(A),
    op(B) and |op A| |op B|."""
    ta, tb, uplo = KINDS[kind]
    rng = np.random.default_rng(1000 * m + 10 * n + k + 7 * ta + 3 * tb)
    ar, ac = (k, m) if ta else (m, k)
    br, bc = (n, k) if tb else (k, n)
    MA = backing(rng, ar + 128, ac + 64)
    A = View(MA, 64, 64, ar, ac)
    if uplo and m > n:
        B = View(MA, 64, 64, br, bc)
    else:
        B = View(backing(rng, br + 64, bc + 64), 64, 0, br, bc)
    C = View(backing(rng, m + 128, n + 64), 64, 64, m, n)
    opA = A.a.T if ta else A.a
    opB = B.a.T if tb else B.a
    return A, B, C, opA, opB, np.abs(opA) @ np.abs(opB)


def reference(opA, opB, C0, alpha, beta, uplo, dtype=np.float64):
    full = alpha * (opA.astype(dtype) @ opB.astype(dtype)) + beta * C0.astype(dtype)
    if not uplo:
        return full
    i, j = np.indices(C0.shape)
    return np.where(i >= j, full, C0.astype(dtype))


def run(ctx, mode, ta, tb, uplo, tri, m, n, k, alpha, A, B, beta, C, bz=None, put=None):
    """One product on the device in staging mode `mode`; returns C's backing
    matrix afterwards.  `put`: the device copies of the backing matrices."""
    ctx.call("smg_set_gemm_stage_mode", mode)
    bases = {}
    for v in (A, B, C):
        if id(v.back) not in bases:
            bases[id(v.back)] = ctx.put(v.back.ravel(order="F"))
            assert bases[id(v.back)] % 16 == 0
    dA, dB, dC = (v.dev(bases[id(v.back)]) for v in (A, B, C))
    if bz is None:
        ctx.call("smg_gemm_tri", ta, tb, uplo, tri, m, n, k, alpha, dA, A.ld, dB, B.ld, beta, dC, C.ld)
    else:
        ctx.call("smg_gemm_bz", ta, tb, uplo, tri, m, n, k, alpha, dA, A.ld, dB, B.ld, beta, dC, C.ld, bz)
    out = ctx.get(bases[id(C.back)], C.back.size).reshape(C.back.shape[::-1]).T
    ctx.call("smg_set_gemm_stage_mode", 0)
    return out


def inside(out, ref, k, alpha, beta, absprod, C0):
    bound = 2.0 * gamma(k) * (abs(alpha) * absprod + abs(beta) * np.abs(C0))
    err = np.abs(out - ref)
    assert np.all(err <= bound), (float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))


def outside_untouched(out_back, C):
    """Everything of the backing matrix outside the C block keeps its bytes."""
    mask = np.ones(C.back.shape, bool)
    mask[C.r0:C.r0 + C.rows, C.c0:C.c0 + C.cols] = False
    assert np.array_equal(out_back[mask], C.back[mask])


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_reference_inside_gamma(kind, m, n, k):
    """numpy float64 against np.longdouble stays inside gamma_K on the inputs
    of test_agrees_with_numpy (what its doubled bound assumes)."""
    uplo = KINDS[kind][2]
    A, B, C, opA, opB, absprod = case(kind, m, n, k)
    for alpha, beta in COEFFS:
        ref = reference(opA, opB, C.a, alpha, beta, uplo)
        ref_ld = reference(opA, opB, C.a, alpha, beta, uplo, np.longdouble)
        bound = gamma(k) * (abs(alpha) * absprod + abs(beta) * np.abs(C.a))
        assert np.all(np.abs(ref - ref_ld) <= bound)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_agrees_with_numpy(ctx, mode, kind, m, n, k):
    ta, tb, uplo = KINDS[kind]
    A, B, C, opA, opB, absprod = case(kind, m, n, k)
    for alpha, beta in COEFFS:
        out = run(ctx, mode, ta, tb, uplo, 0, m, n, k, alpha, A, B, beta, C)
        ref = reference(opA, opB, C.a, alpha, beta, uplo)
        got = out[C.r0:C.r0 + m, C.c0:C.c0 + n]
        inside(got, ref, k, alpha, beta, absprod, C.a)
        if uplo:
            i, j = np.indices((m, n))
            assert np.array_equal(got[i < j], C.a[i < j])
        outside_untouched(out, C)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("bz", [128, -128])
@pytest.mark.parametrize("kind", ["TN-lower", "NN-full"])
def test_beta_zero_region(ctx, mode, bz, kind):
    """bz: C's rows from 128 on (bz > 0) / columns from 128 on (bz < 0) take
    beta = 0 and are not read (NaN there must not come through); the other
    region accumulates."""
    ta, tb, uplo = KINDS[kind]
    m = n = 256
    k = 64
    A, B, C, opA, opB, absprod = case(kind, m, n, k)
    i, j = np.indices((m, n))
    zero = (i >= bz) if bz > 0 else (j >= -bz)
    C0 = C.a.copy()
    back = C.back.copy()
    back[C.r0:C.r0 + m, C.c0:C.c0 + n][zero] = np.nan
    Cn = View(back, C.r0, C.c0, m, n)
    out = run(ctx, mode, ta, tb, uplo, 0, m, n, k, 1.0, A, B, 1.0, Cn, bz=bz)
    got = out[C.r0:C.r0 + m, C.c0:C.c0 + n]
    written = (i >= j) if uplo else np.ones((m, n), bool)
    assert not np.isnan(got[written]).any()
    assert np.isnan(got[~written & zero]).all()  # (lower: the upper triangle is not touched)
    Cz = np.where(zero, 0.0, C0)
    ref = opA @ opB + Cz
    bound = 2.0 * gamma(k) * (absprod + np.abs(Cz))
    assert np.all(np.abs(got - ref)[written] <= bound[written])
    assert np.array_equal(got[~written & ~zero], C0[~written & ~zero])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["NT-lower", "TN-lower"])
@pytest.mark.parametrize("m,n,k", [(256, 256, 64), (320, 64, 192), (192, 128, 128)])
def test_lower_writes_same_elements(ctx, kind, m, n, k):
    ta, tb, uplo = KINDS[kind]
    A, B, C, opA, opB, absprod = case(kind, m, n, k)
    sentinel = 12345.6789
    Cs = View(np.full_like(C.back, sentinel), C.r0, C.c0, m, n)
    changed = [run(ctx, mode, ta, tb, 1, 0, m, n, k, 1.0, A, B, 1.0, Cs) != sentinel for mode in (1, 2)]
    assert np.array_equal(changed[0], changed[1])
    i, j = np.indices((m, n))
    assert not changed[1][C.r0:C.r0 + m, C.c0:C.c0 + n][i < j].any()
    assert changed[1].sum() == (i >= j).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("tri", [1, 4, 5, 8])
@pytest.mark.parametrize("kind", list(KINDS))
def test_triangular_operands(ctx, mode, tri, kind):
    """K ranges cut to the operands' triangles (zeros stored)."""
    ta, tb, uplo = KINDS[kind]
    n = k = 256
    A, B, C, opA, opB, _ = case(kind, n, n, k)
    i, j = np.indices((n, n))
    fa = np.where(i >= j, 1.0, 0.0) if tri & 1 else np.ones((n, n))    # op(A)(i, k) = 0 for k > i
    fb = np.ones((n, n))
    if tri & 4:
        fb = np.where(i >= j, 1.0, 0.0)                                # op(B)(k, j) = 0 for k < j
    if tri & 8:
        fb = np.where(i <= j, 1.0, 0.0)                                # op(B)(k, j) = 0 for k > j
    tA, tB = opA * fa, opB * fb
    backA, backB = A.back.copy(), B.back.copy()
    At, Bt = View(backA, A.r0, A.c0, A.rows, A.cols), View(backB, B.r0, B.c0, B.rows, B.cols)
    At.a[...] = tA.T if ta else tA
    Bt.a[...] = tB.T if tb else tB
    for alpha, beta in COEFFS:
        out = run(ctx, mode, ta, tb, uplo, tri, n, n, k, alpha, At, Bt, beta, C)
        got = out[C.r0:C.r0 + n, C.c0:C.c0 + n]
        inside(got, reference(tA, tB, C.a, alpha, beta, uplo), k, alpha, beta, np.abs(tA) @ np.abs(tB), C.a)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["m96", "k40", "odd_ld", "offset_pointer", "c_aliases_a"])
def test_ineligible_products_untouched(ctx, what):
    """A product the DMA path cannot take runs the same kernel in mode 2 as in
    mode 1: bitwise equal results."""
    rng = np.random.default_rng(11)
    m, n, k = (96, 128, 64) if what == "m96" else (128, 128, 40) if what == "k40" else (128, 128, 128)
    lda = 257 if what == "odd_ld" else 256
    off = 1 if what == "offset_pointer" else 0
    MA, MB, MC = backing(rng, lda, 256), backing(rng, 256, 256), backing(rng, 256, 256)
    A, B = View(MA, off, 0, m, k), View(MB, 0, 0, k, n)
    C = View(MA, off, 0, m, n) if what == "c_aliases_a" else View(MC, 0, 0, m, n)
    for uplo in (0, 1):
        outs = [run(ctx, mode, 0, 0, uplo, 0, m, n, k, 1.5, A, B, -0.5, C) for mode in (1, 2)]
        assert np.array_equal(outs[0], outs[1])
        # (the computed triangle only: an aliased lower product leaves the other one unspecified)
        i, j = np.indices((m, n))
        w = i >= j if uplo else i >= 0
        ref = reference(A.a, B.a, C.a, 1.5, -0.5, 0)
        inside(outs[1][C.r0:C.r0 + m, :n][w], ref[w], k, 1.5, -0.5, (np.abs(A.a) @ np.abs(B.a))[w], C.a[w])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_deterministic(ctx, kind):
    ta, tb, uplo = KINDS[kind]
    m, n, k = 256, 256, 512
    A, B, C, *_ = case(kind, m, n, k)
    outs = [run(ctx, 2, ta, tb, uplo, 0, m, n, k, -1.0, A, B, 1.0, C) for _ in range(2)]
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_gp_closed_form_dma_staged(ctx):
    """The GP gradient on the closed-form schedule at N = 1024 with every
    eligible product DMA-staged, at test_gp_marginal_golden_closed_form's
    tolerances."""
    from test_gpu_kernels import RTOL, gp_gradient_abi_closed_form
    d = golden("gp_N1024")
    ctx.call("smg_set_gemm_stage_mode", 2)
    fx, g = gp_gradient_abi_closed_form(ctx, d["x"], d["y"], d["theta"])
    assert ctx.status() == 0
    near_rel(fx, d["fx"], 1e-12, what="fx")
    near_rel(g, d["grad"], RTOL, what="grad")
