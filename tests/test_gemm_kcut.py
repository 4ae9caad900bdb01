"""The GEMM's offset triangular K cuts (smg_gemm_cut) and their use in the
progressive K^{-1} (chol_mvn.hip smg_inv_prog_row).

cut_a >= 0 declares op(A)(i, t) = 0 for t < i - cut_a in the rows i >= cut_a,
cut_b >= 0 declares op(B)(t, j) = 0 for t < j - cut_b in the columns
j >= cut_b -- the shape of a block row [X | T] of a lower triangular matrix
with T its diagonal block.  A tile whose first row (column) lies at or past
the cut skips the K range those zeros cover, floored to its K stage, so the
64-blocks that lie wholly inside the declared region are never read by a
kernel with 32- or 64-wide tiles; the tests fill exactly those with NaN.

Skipped terms are exact zeros added to a chain that is otherwise unchanged, so
the cut product must equal the uncut one under np.array_equal (which takes
-0.0 == 0.0: adding zeros can only change the sign of a zero).  The numpy
comparisons use test_gemm_dma_stage's bound, 2 gamma_K (|alpha| |op A| |op B|
+ |beta| |C0|).

Kernels reached (stage mode 1 = registers, 2 = LDS-DMA where eligible):
  (256, 256, 128) TN lower, (192, 256, 128) NN full: 32 x 32 tiles, 8 waves,
      split over K in two (mode 1); 64 x 64 DMA, 8 waves, K stages of 32 (mode 2)
  (192, 256, 256) NN full: the same, split in four (mode 1)
  (544, 544, 96) NN full: 32 x 32 tiles, 4 waves, unsplit (both modes: 544 is
      no multiple of 64)
  (2112, 2112, 128) TN lower, 561 tiles: 64 x 64, 8 waves, registers (mode 1);
      64 x 64 DMA, 4 waves, K stages of 16 in three buffers (mode 2).  With
      cut_a = 2048 only the last tile row lies past the cut and skips nothing;
      cut_a = 1984 makes that row run the shortest range, 64 of the 128.
  (2560, 2560, 128) NN full, 1600 tiles: 64 x 64, 4 waves, registers (mode 1);
      64 x 64 DMA, 4 waves (mode 2)
"""
import ctypes
import functools

import numpy as np
import pytest

from _util import near_rel
from test_gemm_dma_stage import View, backing, gamma

KINDS = {"TN-lower": (1, 0, 1), "NN-full": (0, 0, 0)}
# (kind, m, n, k, cut): cut_a for TN-lower (the K^{-1} share's form, B = A),
# cut_b for NN-full (the Y parts' form)
CASES = [
    ("TN-lower", 256, 256, 128, 128),
    ("TN-lower", 2112, 2112, 128, 2048),
    ("TN-lower", 2112, 2112, 128, 1984),
    ("NN-full", 192, 256, 128, 128),
    ("NN-full", 192, 256, 256, 128),
    ("NN-full", 544, 544, 96, 320),
    ("NN-full", 2560, 2560, 128, 2432),
]
IDS = [f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-cut{c[4]}" for c in CASES]


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
    c.call("smg_set_gemm_cut_mode", 1)
    assert c.status() == 0
    c.rewind(m)


def declared(rows, k, cut):
    """For an operand in the orientation (row or column index r, K index t):
    the declared zeros t < r - cut (r >= cut), and the 64-blocks wholly inside
    them (rows cut + 64 I .., t < 64 I)."""
    r, t = np.indices((rows, k))
    zero = (r >= cut) & (t < r - cut)
    blocks = (r >= cut) & (t < (r - cut) // 64 * 64)
    return zero, blocks


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k, cut):
    """Operand views at 64-multiple offsets of larger backing matrices, the
    declared zeros stored.  TN lower: B is A (the share C += W_k^T W_k), the
    zeros in op(A)'s rows >= cut_a.  NN full: the zeros in op(B)'s columns
    >= cut_b.  Returns the views, the NaN mask of the operand that carries the
    zeros (in its stored orientation), op(A), op(B), |op A| |op B|."""
    ta, tb, uplo = KINDS[kind]
    rng = np.random.default_rng(100000 * m + 100 * n + k + cut)
    if kind == "TN-lower":
        MA = backing(rng, k + 128, m + 64)
        A = View(MA, 64, 64, k, m)  # stored k x m: op(A) = A^T
        zero, blocks = declared(m, k, cut)
        A.a[zero.T] = 0.0
        B, nanmask = A, blocks.T
    else:
        A = View(backing(rng, m + 128, k + 64), 64, 64, m, k)
        B = View(backing(rng, k + 64, n + 64), 64, 0, k, n)  # stored k x n = op(B)
        zero, blocks = declared(n, k, cut)
        B.a[zero.T] = 0.0
        nanmask = blocks.T
    C = View(backing(rng, m + 128, n + 64), 64, 64, m, n)
    opA = A.a.T if ta else A.a
    opB = B.a.T if tb else B.a
    return A, B, C, nanmask, opA, opB, np.abs(opA) @ np.abs(opB)


def cuts(kind, cut):
    return (cut, -1) if kind == "TN-lower" else (-1, cut)


def with_nan(v, nanmask):
    back = v.back.copy()
    w = View(back, v.r0, v.c0, v.rows, v.cols)
    w.a[nanmask] = np.nan
    return w


def run(ctx, stage, kind, m, n, k, alpha, A, B, beta, C, bz=0, cut_a=-1, cut_b=-1, cut_mode=1):
    """One product; returns C's backing matrix afterwards."""
    ta, tb, uplo = KINDS[kind]
    ctx.call("smg_set_gemm_stage_mode", stage)
    ctx.call("smg_set_gemm_cut_mode", cut_mode)
    mark = ctx.mark()
    bases = {}
    for v in (A, B, C):
        if id(v.back) not in bases:
            bases[id(v.back)] = ctx.put(v.back.ravel(order="F"))
            assert bases[id(v.back)] % 16 == 0
    dA, dB, dC = (v.dev(bases[id(v.back)]) for v in (A, B, C))
    ctx.call("smg_gemm_cut", ta, tb, uplo, 0, m, n, k, alpha, dA, A.ld, dB, B.ld, beta, dC, C.ld, bz, cut_a, cut_b)
    out = ctx.get(bases[id(C.back)], C.back.size).reshape(C.back.shape[::-1]).T
    ctx.rewind(mark)
    ctx.call("smg_set_gemm_stage_mode", 0)
    ctx.call("smg_set_gemm_cut_mode", 1)
    return out


def reference(opA, opB, C0, alpha, beta, uplo):
    full = alpha * (opA @ opB) + beta * C0
    if not uplo:
        return full
    i, j = np.indices(C0.shape)
    return np.where(i >= j, full, C0)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("kind,m,n,k,cut", CASES, ids=IDS)
def test_declared_region(kind, m, n, k, cut):
    """The inputs are what the docstring says: zeros stored in the declared
    region, the NaN blocks inside it, and (all cases but the one whose cut
    lies in the last tile row) at least one whole 64-block to skip."""
    A, B, C, nanmask, opA, opB, _ = case(kind, m, n, k, cut)
    held = A.a if kind == "TN-lower" else B.a
    zero, blocks = declared(m if kind == "TN-lower" else n, k, cut)
    assert not np.any(held[zero.T])
    assert np.array_equal(nanmask, blocks.T) and not np.any(blocks & ~zero)
    assert nanmask.any() == ((m if kind == "TN-lower" else n) - cut > 64)
    assert np.count_nonzero(held) > held.size // 4  # (not all zeros)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("kind,m,n,k,cut", CASES, ids=IDS)
def test_cut_equals_uncut_and_numpy(ctx, stage, kind, m, n, k, cut):
    """smg_gemm_cut with the cut equals the same call with cut_a = cut_b = -1
    bit for bit (alpha, beta general), agrees with numpy inside the gamma_K
    bound, and writes nothing outside C (lower: nothing above the diagonal)."""
    ta, tb, uplo = KINDS[kind]
    A, B, C, _, opA, opB, absprod = case(kind, m, n, k, cut)
    ca, cb = cuts(kind, cut)
    for alpha, beta in ((-1.0, 1.0), (1.5, -0.5)):
        got = run(ctx, stage, kind, m, n, k, alpha, A, B, beta, C, cut_a=ca, cut_b=cb)
        plain = run(ctx, stage, kind, m, n, k, alpha, A, B, beta, C)
        assert np.array_equal(got, plain)
        # (cut mode 2: the same cuts in the uncut product's tile placement)
        assert np.array_equal(got, run(ctx, stage, kind, m, n, k, alpha, A, B, beta, C, cut_a=ca, cut_b=cb, cut_mode=2))
        ref = reference(opA, opB, C.a, alpha, beta, uplo)
        blk = got[C.r0:C.r0 + m, C.c0:C.c0 + n]
        bound = 2.0 * gamma(k) * (abs(alpha) * absprod + abs(beta) * np.abs(C.a))
        err = np.abs(blk - ref)
        assert np.all(err <= bound), (float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
        if uplo:
            i, j = np.indices((m, n))
            assert np.array_equal(blk[i < j], C.a[i < j])
        mask = np.ones(C.back.shape, bool)
        mask[C.r0:C.r0 + m, C.c0:C.c0 + n] = False
        assert np.array_equal(got[mask], C.back[mask])


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("kind,m,n,k,cut", CASES, ids=IDS)
def test_declared_blocks_not_read(ctx, stage, kind, m, n, k, cut):
    """NaN in the declared-zero 64-blocks: with the cuts the result is finite
    and bit-equal to the clean operands' result; with cut mode 0 the same call
    reads them and the NaNs come through (so this test can fail)."""
    ta, tb, uplo = KINDS[kind]
    A, B, C, nanmask, *_ = case(kind, m, n, k, cut)
    ca, cb = cuts(kind, cut)
    if kind == "TN-lower":
        An = Bn = with_nan(A, nanmask)
    else:
        An, Bn = A, with_nan(B, nanmask)
    clean = run(ctx, stage, kind, m, n, k, 1.5, A, B, -0.5, C, cut_a=ca, cut_b=cb)
    got = run(ctx, stage, kind, m, n, k, 1.5, An, Bn, -0.5, C, cut_a=ca, cut_b=cb)
    assert np.isfinite(got).all()
    assert np.array_equal(got, clean)
    if nanmask.any():
        off = run(ctx, stage, kind, m, n, k, 1.5, An, Bn, -0.5, C, cut_a=ca, cut_b=cb, cut_mode=0)
        assert np.isnan(off).any()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("kind,m,n,k,cut", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_with_beta_zero_boundary(ctx, stage, kind, m, n, k, cut):
    """bz at the cut, beta = 1 (the share: rows from cut_a on; the Y parts:
    columns from cut_b on): the region past the boundary ignores a NaN-filled
    C, the rest accumulates, and the cut changes no bit of either."""
    ta, tb, uplo = KINDS[kind]
    A, B, C, _, opA, opB, absprod = case(kind, m, n, k, cut)
    ca, cb = cuts(kind, cut)
    bz = cut if kind == "TN-lower" else -cut
    i, j = np.indices((m, n))
    zero = (i >= bz) if bz > 0 else (j >= -bz)
    Cn = View(C.back.copy(), C.r0, C.c0, m, n)
    Cn.a[zero] = np.nan
    got = run(ctx, stage, kind, m, n, k, 1.0, A, B, 1.0, Cn, bz=bz, cut_a=ca, cut_b=cb)
    plain = run(ctx, stage, kind, m, n, k, 1.0, A, B, 1.0, Cn, bz=bz)
    assert np.array_equal(got, plain, equal_nan=True)
    blk = got[C.r0:C.r0 + m, C.c0:C.c0 + n]
    written = (i >= j) if uplo else np.ones((m, n), bool)
    assert not np.isnan(blk[written]).any()
    assert np.isnan(blk[~written & zero]).all()
    Cz = np.where(zero, 0.0, C.a)
    bound = 2.0 * gamma(k) * (absprod + np.abs(Cz))
    assert np.all(np.abs(blk - (opA @ opB + Cz))[written] <= bound[written])
    assert np.array_equal(blk[~written & ~zero], C.a[~written & ~zero])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,m,n,k,cut", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_deterministic(ctx, kind, m, n, k, cut):
    A, B, C, *_ = case(kind, m, n, k, cut)
    ca, cb = cuts(kind, cut)
    for stage in (1, 2):
        outs = [run(ctx, stage, kind, m, n, k, -1.0, A, B, 1.0, C, cut_a=ca, cut_b=cb) for _ in range(2)]
        assert np.array_equal(outs[0], outs[1])


@functools.lru_cache(maxsize=None)
def spd(n):
    rng = np.random.default_rng(4000 + n)
    Bm = rng.uniform(-1, 1, (n, n))
    A = Bm @ Bm.T / n + 0.2 * np.eye(n)
    return 0.5 * (A + A.T), rng.uniform(-1, 1, n)


def progressive(ctx, n, cut_mode):
    """The factorisation with the progressive W and K^{-1} from a NaN
    workspace, then the MVN's solves on W: tril(W), tril(C), [w, s], lp."""
    A, y = spd(n)
    lib = ctx.lib
    ctx.call("smg_set_gemm_cut_mode", cut_mode)
    dA, dL = ctx.put(A.ravel(order="F")), ctx.zeros(n * n)
    dD = ctx.zeros(lib.smg_cholesky_aux_doubles(n))
    ws = ctx.put(np.full(lib.smg_cholesky_mvn_rev_ws_doubles(n), np.nan))
    started = ctypes.c_int(-1)
    ctx.call("smg_cholesky_fwd_checked_mark_inv", dA, n, n, dL, n, dD, ws, ctypes.byref(started))
    assert started.value == 2
    st = ctypes.c_int(-1)
    ctx.call("smg_status_mark_wait", ctypes.byref(st))
    assert st.value == 0
    ctx.call("smg_cholesky_inverse_wait")
    sol, lp = ctx.zeros(2 * n), ctx.zeros(1)
    ctx.call("smg_mvn_cholesky_fwd_inv", ctx.put(y), None, dL, n, ws, n, n, sol, lp)
    ctx.call("smg_join_async")
    W = np.tril(ctx.get(ws, n * n).reshape(n, n, order="F"))
    C = np.tril(ctx.get(ws + 8 * n * n, n * n).reshape(n, n, order="F"))
    out = W, C, ctx.get(sol, 2 * n), ctx.get(lp, 1)
    ctx.call("smg_set_gemm_cut_mode", 1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 1536])
def test_progressive_inverse_same_bits(ctx, n):
    """smg_cholesky_fwd_checked_mark_inv with the cuts (mode 1) and without
    (mode 0): W, K^{-1} (lower triangles) and the solves' [w, s] and lp are
    equal; twice with the cuts gives the same bits.  n = 1536 is the smallest
    size with a part 4 (Y_{k+2:}); there K^{-1} is also held against numpy's
    inverse at the progressive-inverse tests' tolerance."""
    outs = []
    for mode in (1, 0, 1):
        m0 = ctx.mark()
        outs.append(progressive(ctx, n, mode))
        ctx.rewind(m0)
    for what, a, b, c in zip(("W", "K^-1", "[w, s]", "lp"), *outs):
        assert np.isfinite(a).all(), what
        assert np.array_equal(a, b), f"{what}: cut vs uncut"
        assert np.array_equal(a, c), f"{what}: run to run"
    if n == 1536:
        Kinv = np.linalg.inv(spd(n)[0])
        near_rel(outs[0][1], np.tril(Kinv), 1e-9, atol=1e-10 * np.abs(Kinv).max(), what="K^-1 vs numpy")
