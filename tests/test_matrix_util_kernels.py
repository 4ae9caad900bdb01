"""The matrix helpers and small reducers behind the host layer (matrix_util.hip,
smg_add_tril of tangent.hip, smg_copy_matrix of tri.hip, smg_axpy / _dev /
smg_sum of elementwise.hip) against numpy.

Pure data movement is bit-exact.  An entry that adds one product or one
sum to a stored value is held to |diff| <= 2 u (|a| + |b|) (one rounding with
an FMA, two without), smg_diag_ratio_rev's two updates included.  The reductions (smg_dot,
smg_sum, smg_diag_ratio_fwd) are held to gamma_{N + 2} sum |term|: N - 1
additions in any order, one rounding forming a term (the product or the
quotient; none for smg_sum) and the addition into out.

Every matrix sits in a padded buffer (_ref_tangent.Mat): NaN padding for
inputs, a sentinel that must keep its bits for outputs; parts of an input the
header says are not read hold NaN as well.  `par` runs each matrix test with
the leading dimensions' parities swapped, so every operand meets an odd and an
even one.
"""
import functools

import numpy as np
import pytest

from _ref_tangent import LD, SMG_ERR_ARG, Mat, elem_bound, gamma, same_bits, sentinel, vec

RECT = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 257), (300, 1)]
SQUARE = [1, 2, 63, 64, 65, 130, 257]
LONG = [1, 255, 256, 257, 100003]

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
def rand(m, n, seed=0):
    a = np.random.default_rng(100000 * seed + 1000 * m + n).uniform(-1.0, 1.0, (m, n))
    a.setflags(write=False)
    return a


def tri_masks(m, n):
    i, j = np.indices((m, n))
    return i >= j, i < j


def within(got, a0, inc, c=0):
    """got = fl(a0 + inc) entry by entry (inc in longdouble)."""
    err = np.abs(got.astype(LD) - (a0.astype(LD) + inc))
    bound = elem_bound(a0, inc, c)
    assert np.all(err <= bound), f"max error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}"


def ldp(rows, par):
    """The smallest leading dimension above `rows` of parity `par`."""
    return rows + 1 + (rows + 1 + par) % 2


def packed(n):
    """(row, column) of each entry of the packed lower triangle, in order."""
    j, i = np.triu_indices(n)  # column-major lower == row-major upper, transposed
    return i, j


# ====================================================================== data movement
@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("m,n", RECT)
def test_transpose(ctx, m, n, par):
    A, B0 = rand(m, n), rand(n, m, 1)
    mA = Mat(A, ldp(m, par), np.nan)
    mA.put(ctx)
    mB = Mat(np.full((n, m), np.nan), ldp(n, 1 - par))
    mB.put(ctx)
    ctx.call("smg_transpose", m, n, mA.dev, mA.ld, mB.dev, mB.ld, 0.0)
    assert same_bits(mB.get(ctx), A.T)
    mB = Mat(B0, ldp(n, par))
    mB.put(ctx)
    ctx.call("smg_transpose", m, n, mA.dev, mA.ld, mB.dev, mB.ld, -0.5)
    got = mB.get(ctx)
    within(got, A.T, -0.5 * B0.astype(LD))
    ctx.call("smg_transpose", 0, n, mA.dev, mA.ld, mB.dev, mB.ld, 0.0)
    ctx.call("smg_transpose", m, 0, mA.dev, mA.ld, mB.dev, mB.ld, 0.0)
    assert ctx.lib.smg_transpose(ctx.ptr, m, n, mA.dev, m - 1, mB.dev, mB.ld, 0.0) == SMG_ERR_ARG
    assert ctx.lib.smg_transpose(ctx.ptr, m, n, mA.dev, mA.ld, mB.dev, n - 1, 0.0) == SMG_ERR_ARG
    assert same_bits(mB.get(ctx), got)


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("n", SQUARE)
def test_sym_from_lower(ctx, n, par):
    lo, up = tri_masks(n, n)
    A = np.where(lo, rand(n, n), np.nan)  # the strict upper is written, never read
    mA = Mat(A, ldp(n, par))
    mA.put(ctx)
    ctx.call("smg_sym_from_lower", n, mA.dev, mA.ld)
    got = mA.get(ctx)
    assert same_bits(got[lo], A[lo]), "diagonal / lower triangle changed"
    assert same_bits(got[up], A.T[up])


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("n", SQUARE)
def test_pack_and_unpack_tril(ctx, n, par):
    A = rand(n, n)
    i, j = packed(n)
    T = n * (n + 1) // 2
    mA = Mat(A, ldp(n, 1 - par), np.nan)
    mA.put(ctx)
    got = {}
    for mode, size in ((0, T), (1, T), (2, n)):
        d, read = vec(ctx, np.full(size, np.nan), seed=mode)
        ctx.call("smg_pack_tril", mode, n, mA.dev, mA.ld, d)
        got[mode] = (d, read())
    assert same_bits(got[0][1], A[i, j])
    assert same_bits(got[2][1], np.diag(A))
    within(got[1][1], A[i, j], np.where(i != j, A[j, i], 0.0).astype(LD))
    # unpack_tril_add: modes 0 / 1 tril(B) += unpack(src), mode 2 B_ii += src[i]
    lo, up = tri_masks(n, n)
    B0 = rand(n, n, 2)
    for mode in (0, 1, 2):
        src = rand(T if mode < 2 else n, 1, 3 + mode).ravel()
        dsrc, _ = vec(ctx, src)
        mB = Mat(B0, ldp(n, par))
        mB.put(ctx)
        ctx.call("smg_unpack_tril_add", mode, n, dsrc, mB.dev, mB.ld)
        inc = np.zeros((n, n), dtype=LD)
        if mode < 2:
            inc[i, j] = src
        else:
            inc[np.arange(n), np.arange(n)] = src
        gotB = mB.get(ctx)
        within(gotB, B0, inc)
        assert same_bits(gotB[inc == 0], B0[inc == 0])
    # the round trip of mode 0 adds tril(A) once
    mB = Mat(B0, n + 3)
    mB.put(ctx)
    ctx.call("smg_unpack_tril_add", 0, n, got[0][0], mB.dev, mB.ld)
    gotB = mB.get(ctx)
    within(gotB, B0, np.tril(A).astype(LD))
    assert same_bits(gotB[up], B0[up])


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("m,n", RECT)
def test_copy_matrix(ctx, m, n, par):
    A = rand(m, n)
    lo, up = tri_masks(m, n)
    mA = Mat(A, ldp(m, 1 - par), np.nan)
    mA.put(ctx)
    for zero_upper in (0, 1):
        mB = Mat(np.full((m, n), np.nan), ldp(m, par))
        mB.put(ctx)
        ctx.call("smg_copy_matrix", m, n, mA.dev, mA.ld, mB.dev, mB.ld, 0, zero_upper)
        assert same_bits(mB.get(ctx), np.where(up, 0.0, A) if zero_upper else A)
    assert ctx.lib.smg_copy_matrix(ctx.ptr, m, n, mA.dev, mA.ld, mB.dev, mB.ld, 1, 0) == SMG_ERR_ARG


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("n", SQUARE)
def test_phi(ctx, n, par):
    lo, up = tri_masks(n, n)
    X = np.where(lo, rand(n, n), np.nan)  # Phi reads the lower triangle only
    ref = np.tril(rand(n, n), -1) + 0.5 * np.diag(np.diag(rand(n, n)))
    mX = Mat(X, ldp(n, par), np.nan)
    mX.put(ctx)
    mY = Mat(np.full((n, n), np.nan), ldp(n, 1 - par))
    mY.put(ctx)
    ctx.call("smg_phi", n, mX.dev, mX.ld, mY.dev, mY.ld, 0)
    assert same_bits(mY.get(ctx), ref), "Phi(X)"      # (halving is exact)
    Y0 = rand(n, n, 1)
    mY = Mat(Y0, n + 3)
    mY.put(ctx)
    ctx.call("smg_phi", n, mX.dev, mX.ld, mY.dev, mY.ld, 1)
    got = mY.get(ctx)
    within(got, Y0, ref.astype(LD))
    assert same_bits(got[up], Y0[up])


def test_zero_extents_touch_nothing(ctx):
    """m == 0 / n == 0 where an entry special-cases it: SMG_OK, and neither
    the output nor the accumulated scalar changes (host-side returns)."""
    mX, mY = Mat(rand(5, 5), 7, np.nan), Mat(rand(5, 5, 1), 8)
    mX.put(ctx), mY.put(ctx)
    dvec, read = vec(ctx, sentinel(15, seed=9))
    X, Y = mX.dev, mY.dev
    ctx.call("smg_add_tril", 0, 5, 2.0, X, 7, Y, 8)
    ctx.call("smg_add_tril", 5, 0, 2.0, X, 7, Y, 8)
    ctx.call("smg_shift", 0, 5, 0.5, Y, 8, 0)
    ctx.call("smg_shift", 5, 0, 0.5, Y, 8, 1)
    for mode in (0, 1, 2):
        ctx.call("smg_pack_tril", mode, 0, Y, 8, dvec)
        ctx.call("smg_unpack_tril_add", mode, 0, dvec, Y, 8)
    ctx.call("smg_phi", 0, Y, 8, Y, 8, 0)
    ctx.call("smg_phi", 0, Y, 8, Y, 8, 1)
    ctx.call("smg_sym_from_lower", 0, Y, 8)
    ctx.call("smg_sym_from_lower", 1, Y, 8)
    ctx.call("smg_diag_ratio_fwd", 0, Y, 8, Y, 8, dvec)
    ctx.call("smg_diag_ratio_rev", 0, Y, 8, Y, 8, 1.5, Y, 8, Y, 8)
    ctx.call("smg_axpy_dev", 0, dvec, dvec, dvec)
    assert same_bits(mY.get(ctx), rand(5, 5, 1))
    assert same_bits(read(), sentinel(15, seed=9))


# ====================================================================== one rounding per entry
@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("m,n", RECT)
def test_add_tril(ctx, m, n, par):
    lo, up = tri_masks(m, n)
    X = np.where(lo, rand(m, n), np.nan)
    Y0 = rand(m, n, 1)
    mX, mY = Mat(X, ldp(m, par), np.nan), Mat(Y0, ldp(m, 1 - par))
    mX.put(ctx), mY.put(ctx)
    ctx.call("smg_add_tril", m, n, -1.5, mX.dev, mX.ld, mY.dev, mY.ld)
    got = mY.get(ctx)
    within(got[lo], Y0[lo], -1.5 * X[lo].astype(LD))
    assert same_bits(got[up], Y0[up])


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("uplo", [0, 1])
@pytest.mark.parametrize("m,n", RECT)
def test_shift(ctx, m, n, uplo, par):
    lo, up = tri_masks(m, n)
    Y0 = rand(m, n)
    mY = Mat(Y0, ldp(m, par))
    mY.put(ctx)
    ctx.call("smg_shift", m, n, 0.0, mY.dev, mY.ld, uplo)       # c == 0: a no-op
    assert same_bits(mY.get(ctx), Y0)
    ctx.call("smg_shift", m, n, 0.3, mY.dev, mY.ld, uplo)
    got = mY.get(ctx)
    where = lo if uplo else np.ones((m, n), bool)
    within(got[where], Y0[where], np.full(where.sum(), LD(0.3)))
    assert same_bits(got[~where], Y0[~where])


@pytest.mark.parametrize("par", [0, 1])
@pytest.mark.parametrize("n", SQUARE)
def test_diag_ratio(ctx, n, par):
    A = rand(n, n)
    B = rand(n, n, 1) + 3.0 * np.eye(n)
    off = ~np.eye(n, dtype=bool)
    An, Bn = np.where(off, np.nan, A), np.where(off, np.nan, B)  # only the diagonals are read
    lda, ldb, ldaa, ldba = (ldp(n, par) + k for k in range(4))
    mA, mB = Mat(An, lda, np.nan), Mat(Bn, ldb, np.nan)
    mA.put(ctx), mB.put(ctx)
    a, b = np.diag(A).astype(LD), np.diag(B).astype(LD)
    got = []
    for _ in range(2):
        dout, read = vec(ctx, [0.625])
        ctx.call("smg_diag_ratio_fwd", n, mA.dev, lda, mB.dev, ldb, dout)
        got.append(read()[0])
    assert got[0] == got[1], "not deterministic"
    assert abs(got[0] - (0.625 + (a / b).sum())) <= gamma(n + 2) * float(0.625 + np.abs(a / b).sum())
    adj = -1.25
    Aa0, Ba0 = rand(n, n, 2), rand(n, n, 3)
    for with_a, with_b in ((1, 1), (0, 1), (1, 0)):
        mAa, mBa = Mat(Aa0, ldaa), Mat(Ba0, ldba)
        mAa.put(ctx), mBa.put(ctx)
        ctx.call("smg_diag_ratio_rev", n, mA.dev, lda, mB.dev, ldb, adj, mAa.dev if with_a else None, ldaa,
                 mBa.dev if with_b else None, ldba)
        Aa, Ba = mAa.get(ctx), mBa.get(ctx)
        assert same_bits(Aa[off], Aa0[off]) and same_bits(Ba[off], Ba0[off])
        if with_a:
            within(np.diag(Aa), np.diag(Aa0), adj / b)
        else:
            assert same_bits(Aa, Aa0)
        if with_b:
            within(np.diag(Ba), np.diag(Ba0), -adj * a / (b * b))
        else:
            assert same_bits(Ba, Ba0)


@pytest.mark.parametrize("incx,incy", [(1, 1), (3, 1), (1, 5), (0, 1)])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_axpy(ctx, n, incx, incy):
    x, y0 = rand(n, 1).ravel(), rand(n, 1, 1).ravel()
    xs = np.full((n - 1) * incx + 1, np.nan)
    xs[::max(incx, 1)] = x if incx else x[:1]
    ys = sentinel((n - 1) * incy + 1, seed=3)
    ys[::incy] = y0
    dx, _ = vec(ctx, xs)
    dy, read = vec(ctx, ys)
    ctx.call("smg_axpy", n, 0.75, dx, incx, dy, incy)
    got = read()
    within(got[::incy], y0, 0.75 * (x if incx else np.full(n, x[0])).astype(LD))
    gaps = np.ones(ys.size, bool)
    gaps[::incy] = False
    assert same_bits(got[gaps], ys[gaps])
    ctx.call("smg_axpy", 0, 0.75, dx, incx, dy, incy)
    assert same_bits(read(), got)


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_axpy_dev(ctx, n):
    x, y0 = rand(n, 1).ravel(), rand(n, 1, 1).ravel()
    dx, _ = vec(ctx, x)
    dy, read = vec(ctx, y0)
    da, _ = vec(ctx, [-0.375])
    ctx.call("smg_axpy_dev", n, da, dx, dy)
    within(read(), y0, -0.375 * x.astype(LD))


# ====================================================================== reductions
@pytest.mark.parametrize("n", LONG)
def test_dot_and_sum(ctx, n):
    x, y = rand(n, 1).ravel(), rand(n, 1, 1).ravel()
    dx, _ = vec(ctx, x)
    dy, _ = vec(ctx, y)
    xl, yl = x.astype(LD), y.astype(LD)
    for name, args, terms in (("smg_dot", (dx, dy, n), xl * yl), ("smg_sum", (dx, n), xl)):
        got = []
        for _ in range(2):
            dout, read = vec(ctx, [-0.875])
            ctx.call(name, *args, dout)
            got.append(read()[0])
        assert got[0] == got[1], name + " is not deterministic"
        ref = -0.875 + terms.sum()
        assert abs(got[0] - ref) <= gamma(n + 2) * float(0.875 + np.abs(terms).sum()), (name, got[0], float(ref))
        dout, read = vec(ctx, [-0.875])
        ctx.call(name, *args[:-1], 0, dout)     # n == 0
        assert read()[0] == -0.875
