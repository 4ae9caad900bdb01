"""Kernel-level tests of the triangular solves (tri.hip smg_trsm_impl, trsv.hip
smg_trsv_lower_impl) on every dispatch branch and both triangles, through
smg_mdivide_left_tri_aux_fwd / _rev and smg_mvn_cholesky_fwd, against plain
substitution in longdouble (_ref_tri.py).

Inputs: T = chol(S S^T / m + I), S uniform(-1, 1), seeded from (m, n); the
upper case is T^T.  The triangle of A that must not be read, every leading-
dimension pad of an input and the reverse's workspace hold NaN, so a finite
result proves that only the named triangle and the m-row extent were read;
outputs sit in sentinel-padded buffers that must keep their bits; Aadj and
Badj start from random values.  With aux, A is the device factorisation's own
L (strict upper NaN) and aux its block inverses.

Bounds: the project's near_rel(1e-10, atol = 1e-11 max|ref|) for every
quantity, and a tighter per-family bound on max|got - ref| / max|ref| taken
from the measured errors (TIGHT below).  Every case prints the kernel's worst
error, scipy float64's against the same reference, and their ratio.

k_trsv_fwd<256> and k_trsv_bwd<256> (trsv.hip) have no launch site: only the
<64> instantiations are launched, so nothing here can reach them.
"""
import numpy as np
import pytest

from _ref_tangent import Mat, lds, same_bits
from _ref_tri import COLS_512, LD, mdivide_ref, mvn_ref, relerr, rows_512, spd_inputs, tri_of, tri_solve_ld
from _util import near_rel

RTOL = 1e-10  # the project's standing value (test_gpu_kernels.RTOL)

# Worst max|got - ref| / max|ref| of each path family as measured on an MI355X
# (profiles/tri_solve_tests.txt), times 8 for seed-to-seed spread, rounded up
# to a power of ten, never above RTOL.  Measured worst: block 1.30e-14 (the
# Aadj increment at (1, 1): one entry, |increment| << |Aadj0|, so the rounding
# of the accumulated sum shows at this scale; every other block-loop case is
# below 1.2e-15), persistent 6.33e-16, recursion 1.31e-15, step-wise 8.42e-16.
TIGHT = {"block": 1e-13, "persistent": 1e-14, "recursion": 1e-13, "stepwise": 1e-14}


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
    near_rel(got, np.asarray(ref, dtype=np.float64), rtol, atol=0.1 * rtol * float(np.abs(ref).max()), what=what)


def call(ctx, name, *args):
    """The entry returns SMG_OK and latches nothing (the persistent waits latch
    SMG_ERR_SYNC instead of hanging)."""
    ctx.call(name, *args)
    assert ctx.status() == 0, name


def F(a):
    return np.ascontiguousarray(a.T).ravel()


def device_factor(ctx, S):
    """(L, aux) of smg_cholesky_fwd on the clean SPD matrix S."""
    n = S.shape[0]
    dS, dL = ctx.put(F(S)), ctx.zeros(n * n)
    aux = ctx.zeros(ctx.lib.smg_cholesky_aux_doubles(n))
    call(ctx, "smg_cholesky_fwd", dS, n, n, dL, n, aux)
    return np.tril(ctx.get(dL, n * n).reshape(n, n).T), aux


def report(what, family, errs):
    """errs: {name: (kernel error, scipy float64 error)}, both relative to
    max|ref|; the printed line is the record, the family bound the assertion."""
    k = max(v[0] for v in errs.values())
    s = max(v[1] for v in errs.values())
    parts = " ".join(f"{n}={a:.2e}/{b:.2e}" for n, (a, b) in errs.items())
    print(f"tri_solve {what} family={family} kernel={k:.3e} scipy={s:.3e} ratio={k / max(s, 1e-300):.2f} [{parts}]")
    assert k <= RTOL, (what, k)
    if TIGHT[family] is not None:
        assert k <= TIGHT[family], (what, family, k, TIGHT[family])


# ====================================================================== CPU
@pytest.mark.parametrize("m", [65, 577])
def test_reference_float64_margin(m):
    """The longdouble substitution against scipy's float64 solve_triangular for
    the four (lower, trans) forms: within 1e-13 max|X| (measured: 2e-15), with
    NaN in the triangle that must not be read."""
    from scipy.linalg import solve_triangular
    _, T, B, _, _, _ = spd_inputs(m, 3)
    i, j = np.indices((m, m))
    for lower in (1, 0):
        A = T if lower else T.T
        poisoned = np.where(i >= j if lower else i <= j, A, np.nan)
        for trans in (0, 1):
            X = tri_solve_ld(poisoned, B, lower, trans)
            assert np.all(np.isfinite(X))
            Xs = solve_triangular(A, B, lower=bool(lower), trans=trans)
            err = relerr(Xs, X)
            print(f"m={m} lower={lower} trans={trans}: scipy float64 off by {err:.2e} max|X|")
            assert err <= 1e-13
            # the defining equation, in longdouble
            op = tri_of(A, lower).astype(LD)
            op = op.T if trans else op
            assert np.abs(op @ X - B).max() <= 1e-17 * m * np.abs(X).max()


def test_reference_pieces_match_full():
    """The column / row pieces used at n = 512 are the full reference's."""
    m, n = 1030, 512
    _, T, B, Cadj, _, _ = spd_inputs(m, n)
    sub = [c for c in range(n) if c in COLS_512 or c % 97 == 0]  # (a full 512-column longdouble solve is slow)
    for lower in (1, 0):
        A = T if lower else T.T
        Cp, Bp, Ap = mdivide_ref(A, B, Cadj, lower, pieces=True)
        k = [sub.index(c) for c in COLS_512]
        assert relerr(Cp, tri_solve_ld(A, B[:, sub], lower, 0)[:, k]) <= 1e-17
        assert relerr(Bp, tri_solve_ld(A, Cadj[:, sub], lower, 1)[:, k]) <= 1e-17
        # adjA's rows from full-width C and adjB (float64 solves: 1e-13 is their margin)
        from scipy.linalg import solve_triangular
        C = solve_triangular(A, B, lower=bool(lower))
        aB = solve_triangular(A, Cadj, lower=bool(lower), trans=1)
        full = -tri_of(aB @ C.T, lower)
        assert relerr(full[list(rows_512(m))], Ap) <= 1e-13


# ====================================================================== mdivide_left_tri
# (m, n, triangles, aux modes, family, the branch conditions the case satisfies)
BOTH, LOWER, UPPER = (1, 0), (1,), (0,)
TRI_TABLE = [
    # ---- 64-row block loop in place (m < 512 or n < 64), block edges; upper: k_trtri_blocks(upper = 1), the
    # reverse (trans = 1, lower = 0) runs the loop forward with wt = 0
    (1, 1, BOTH, ("none",), "block", "one block, b = 1"),
    (2, 3, BOTH, ("none",), "block", "one block, b = 2"),
    (63, 3, BOTH, ("none",), "block", "one ragged block"),
    (64, 1, BOTH, ("none",), "block", "one full block, N = 1"),
    (65, 3, BOTH, ("none",), "block", "two blocks, tail b = 1: k_trtri_blocks(upper = 1) on a ragged tail"),
    (128, 65, BOTH, ("none",), "block", "two full blocks, n past one GEMM tile"),
    (129, 1, BOTH, ("none",), "block", "three blocks, tail b = 1, N = 1"),
    (200, 65, BOTH, ("none",), "block", "four blocks, tail b = 8: upper reverse beyond one diagonal block"),
    # ---- one right-hand side that misses the persistent path: m >= 512 but m % 256 != 0, or upper
    (600, 1, BOTH, ("none",), "block", "n == 1, m % 256 = 88: GEMM block loop with N = 1"),
    (1000, 1, BOTH, ("none",), "block", "n == 1, m % 256 = 232: GEMM block loop with N = 1"),
    (768, 1, UPPER, ("none",), "block", "n == 1, m % 256 == 0 but lower = 0: GEMM block loop"),
    # ---- persistent, 256-row level (n == 1, lower, m >= 512, m % 256 == 0): forward k_trsv_persist<false, 256>
    # (m < 1024 or m % 512 != 0), reverse k_trsv_persist<true, 256>
    (512, 1, LOWER, ("none", "aux"), "persistent", "m = 512: W512 given but m < 1024, two 256-row blocks"),
    (768, 1, LOWER, ("none", "aux"), "persistent", "m % 512 = 256: W512 == nullptr, three blocks, both directions"),
    (1280, 1, LOWER, ("none", "aux"), "persistent", "m % 512 = 256: W512 == nullptr, five blocks, both directions"),
    # ---- persistent, 512-row forward (m % 512 == 0, m >= 1024) next to the 256-row backward
    (1536, 1, LOWER, ("aux",), "persistent", "k_trsv_persist<false, 512> forward, <true, 256> reverse, aux given"),
    # ---- out of place (m >= 512 and n >= 64, X != NULL), 64-row blocks; upper: the out-of-place upper block loop
    (512, 64, BOTH, ("none",), "block", "8 full blocks out of place"),
    (577, 65, BOTH, ("none",), "block", "10 blocks, tail b = 1, out of place"),
    # ---- recursion (lower, m >= 2048, m % 512 == 0, n >= 512): rec_t::solve on 5 blocks splits 2 + 3, the 3 into
    # 1 + 2, forward and (reverse) transposed; (1536, 512) has m < 2048 and stays on 64-row blocks
    (2560, 512, LOWER, ("none", "aux"), "recursion", "5 and 3 blocks of 512 rows, both directions"),
    (1536, 512, LOWER, ("none",), "block", "m < 2048: 24 blocks of 64 rows out of place (contrast)"),
    # ---- upper at the recursion's shape: big needs lower, so 40 blocks of 64 rows out of place
    (2560, 512, UPPER, ("none",), "block", "lower = 0 at (2560, 512): the block loop, not the recursion"),
]
TRI_CASES = [pytest.param(m, n, lo, modes, fam, id=f"{fam}-{m}x{n}-{'lower' if lo else 'upper'}")
             for m, n, tris, modes, fam, _why in TRI_TABLE for lo in tris]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,lower,modes,family", TRI_CASES)
def test_mdivide_left_tri(ctx, m, n, lower, modes, family):
    from scipy.linalg import solve_triangular
    S, T, B, Cadj, Aadj0, Badj0 = spd_inputs(m, n)
    aux = None
    if "aux" in modes:
        T, aux = device_factor(ctx, S)
    A = T if lower else T.T
    i, j = np.indices((m, m))
    tri = (i >= j) if lower else (i <= j)
    lda, ldb, ldc, ldca, ldaa, ldba = lds(m, 6, shift=n % 2)
    mA, mB, mCa = Mat(np.where(tri, A, np.nan), lda, np.nan), Mat(B, ldb, np.nan), Mat(Cadj, ldca, np.nan)
    for x in (mA, mB, mCa):
        x.put(ctx)
    pieces = n == 512
    rC, rB, rA = mdivide_ref(A, B, Cadj, lower, pieces)
    sC = solve_triangular(A, B, lower=bool(lower))
    sB = solve_triangular(A, Cadj, lower=bool(lower), trans=1)
    sA = -tri_of(sB @ sC.T, lower)
    cols, rows = list(COLS_512), list(rows_512(m))

    def errs_of(C, dB, dA):
        """(kernel, scipy) errors of C, the Badj and the Aadj increment."""
        if pieces:
            return {"C": (relerr(C[:, cols], rC), relerr(sC[:, cols], rC)),
                    "adjB": (relerr(dB[:, cols], rB), relerr(sB[:, cols], rB)),
                    "adjA": (relerr(dA[rows], rA), relerr(sA[rows], rA))}
        return {"C": (relerr(C, rC), relerr(sC, rC)), "adjB": (relerr(dB, rB), relerr(sB, rB)),
                "adjA": (relerr(dA, rA), relerr(sA, rA))}

    def check(C, dB, dA, what):
        for got in (C, dB, dA):
            assert np.all(np.isfinite(got)), f"{what}: NaN leaked from a poisoned region"
        if pieces:  # the pieces in longdouble, the full matrices against float64
            near_mat(C[:, cols], rC, what + " C columns")
            near_mat(dB[:, cols], rB, what + " Badj columns")
            near_mat(dA[rows], rA, what + " Aadj rows")
            near_mat(C, sC, what + " C"), near_mat(dB, sB, what + " Badj"), near_mat(dA, sA, what + " Aadj")
        else:
            near_mat(C, rC, what + " C"), near_mat(dB, rB, what + " Badj"), near_mat(dA, rA, what + " Aadj")

    out = {}
    for mode in modes:
        a = aux if mode == "aux" else None
        what = f"{m}x{n} lower={lower} aux={mode}"
        Cs = []
        for rep in range(2):  # the same forward twice: the same bits
            mC = Mat(np.full((m, n), np.nan), ldc, seed=rep, name="C")
            mC.put(ctx)
            call(ctx, "smg_mdivide_left_tri_aux_fwd", lower, mA.dev, lda, a, mB.dev, ldb, m, n, mC.dev, ldc)
            Cs.append(mC.get(ctx))
        assert same_bits(Cs[0], Cs[1]), f"{what}: forward not repeatable"
        C = Cs[0]
        mCi = Mat(C, ldc, np.nan)  # the reverse's C: an input, NaN in its pad
        mCi.put(ctx)
        ws = ctx.put(np.full(m * n + 8, np.nan))
        mark = ctx.mark()
        res = {}
        for tag, with_a, with_b in (("AB", 1, 1), ("AB2", 1, 1), ("B", 0, 1), ("A", 1, 0)):
            mAa, mBa = Mat(Aadj0, ldaa, seed=5, name="Aadj"), Mat(Badj0, ldba, seed=6, name="Badj")
            mAa.put(ctx), mBa.put(ctx)
            call(ctx, "smg_mdivide_left_tri_aux_rev", lower, mA.dev, lda, a, mCi.dev, ldc, mCa.dev, ldca, m, n,
                 mAa.dev if with_a else None, ldaa, mBa.dev if with_b else None, ldba, ws)
            res[tag] = (mAa.get(ctx), mBa.get(ctx))  # (asserts the pads' bits)
            ctx.rewind(mark)
        Aa, Ba = res["AB"]
        assert same_bits(Aa, res["AB2"][0]) and same_bits(Ba, res["AB2"][1]), f"{what}: reverse not repeatable"
        assert same_bits(Aa[~tri], Aadj0[~tri]), f"{what}: Aadj's other triangle written"
        dA, dB = np.where(tri, Aa.astype(LD) - Aadj0, 0), Ba.astype(LD) - Badj0
        check(C, dB, dA, what)
        # NULL Aadj / NULL Badj: the other as in the full call, the skipped one untouched
        assert same_bits(res["B"][0], Aadj0) and same_bits(res["B"][1], Ba), f"{what}: Aadj = NULL"
        assert same_bits(res["A"][1], Badj0) and same_bits(res["A"][0], Aa), f"{what}: Badj = NULL"
        # the inputs keep their bits
        for x in (mA, mB, mCa, mCi):
            assert same_bits(x.get(ctx), x.a), f"{what}: an input was written"
        report(what, family, errs_of(C, dB, dA))
        out[mode] = (C, dB.astype(np.float64), dA.astype(np.float64))
    if len(modes) == 2:
        for k, name in enumerate(("C", "Badj increment", "Aadj increment")):
            near_rel(out["aux"][k], out["none"][k], 1e-12, atol=1e-12 * float(np.abs(out["none"][k]).max()),
                     what=name + " with aux against without")


# ====================================================================== multi_normal_cholesky_lpdf forward
# Without aux W256 == NULL: the step-wise 64-row kernels, k_trsv_fwd<64> with ceil((N - 64) / 256) workgroups in
# the first step -- 3 at N = 600, 4 at N = 1000 (blockIdx.x >= 1 in i = k + blockIdx.x * ROWS + row), up to 6 at
# 1536.  With aux: N % 256 != 0 takes 256-row steps (k_trsv_diag256 / k_trsv_upd_*) and a 64-row tail; N = 512, 768
# and 1280 take k_trsv_persist<false, 256> (N < 1024 or N % 512 != 0) and <true, 256>; N = 1536 <false, 512> and
# <true, 256>.
MVN_N = [1, 63, 64, 65, 257, 321, 512, 600, 768, 1000, 1280, 1536]


def mvn_family(N, mode):
    return "persistent" if mode == "aux" and N >= 512 and N % 256 == 0 else "stepwise"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["none", "aux"])
@pytest.mark.parametrize("N", MVN_N)
def test_mvn_cholesky_fwd(ctx, N, mode):
    from scipy.linalg import solve_triangular
    S, L, yv, muv, _, _ = spd_inputs(N, 1)
    aux = None
    if mode == "aux":
        L, aux = device_factor(ctx, S)
    y, mu = yv[:, 0], muv[:, 0]
    i, j = np.indices((N, N))
    Lp = np.where(i >= j, L, np.nan)
    dy, dmu = ctx.put(np.concatenate([y, [np.nan] * 4])), ctx.put(np.concatenate([mu, [np.nan] * 4]))
    for with_mu in (1, 0):
        w, sd, lp = mvn_ref(L, y, mu if with_mu else None)
        res = y - mu if with_mu else y
        sw = solve_triangular(L, res, lower=True)
        ssd = solve_triangular(L, sw, lower=True, trans=1)
        slp = -0.5 * (sw @ sw) - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi)
        for ldl in (N, N + 3):
            what = f"mvn N={N} aux={mode} mu={with_mu} ldl={ldl}"
            buf = np.full((N + 1, ldl), np.nan)  # column-major, one spare NaN column
            buf[:N, :N] = Lp.T
            dL = ctx.put(buf.ravel())
            got = []
            for rep in range(2):
                ws_h = np.concatenate([np.full(2 * N, np.nan), 1.0e3 + np.arange(8.0)])
                ws, dlp = ctx.put(ws_h), ctx.put(np.array([np.nan, 77.0]))
                call(ctx, "smg_mvn_cholesky_fwd", dy, dmu if with_mu else None, dL, ldl, aux, N, ws, dlp)
                o, l2 = ctx.get(ws, ws_h.size), ctx.get(dlp, 2)
                assert same_bits(o[2 * N:], ws_h[2 * N:]) and l2[1] == 77.0, f"{what}: written past ws or lp"
                got.append(np.concatenate([o[:2 * N], l2[:1]]))
            assert same_bits(got[0], got[1]), f"{what}: not repeatable"
            assert same_bits(ctx.get(dL, buf.size), buf.ravel()), f"{what}: L written"
            gw, gsd, glp = got[0][:N], got[0][N:2 * N], got[0][2 * N]
            assert np.all(np.isfinite(got[0])), f"{what}: NaN leaked from a poisoned region"
            near_mat(gw, w, what + " w"), near_mat(gsd, sd, what + " sd")
            near_rel(glp, float(lp), RTOL, what=what + " lp")
            report(what, mvn_family(N, mode),
                   {"w": (relerr(gw, w), relerr(sw, w)), "sd": (relerr(gsd, sd), relerr(ssd, sd)),
                    "lp": (relerr([glp], [lp]), relerr([slp], [lp]))})
