"""ordered_logistic_glm_lpmf: the fused device pass smg_ordered_logistic_glm
through ctypes, and the stan::math overloads through the tape
(tests/cpp/test_glm_ordered.cpp).

The reference of every device test is `_ordered.ol_ref`, a float64 numpy
restatement of the formulas (tests/_ordered.py) with every sum by math.fsum.
`ol_ref` itself is checked against multi-precision mpmath without a GPU
(test_reference_against_mpmath), which evaluates log(logistic(a) -
logistic(b)) and its derivatives directly.

Bounds.  Every output (logp, each beta'_j, each cuts'_j) is compared on the
scale of the sum of its terms' absolute values: the terms of logp are ll(a),
ll(-b) and lm of each row, those of beta'_j are x_ij theta'_i, those of
cuts'_j are the d_hi of the rows in class j and the d_lo of the rows in class
j + 1.  No bound is taken relative to a sum itself (cuts'_j cancels: d_hi > 0,
d_lo < 0, and both hold +-1 / expm1(gap), 1e8 at a gap of 1e-8).

    yardstick (ol_ref against mpmath):   asserted at 5e-14 of that scale;
        measured worst ratio over all cases: logp 0 (exact to the last bit),
        beta' 2.8e-17, cuts' 1.7e-16
    device against ol_ref:               1e-12 of that scale, every output
        (the precedent of the other GLM kinds; it holds because the yardstick
        is under 5e-14)

Inputs (_ordered.inputs): x uniform in (-1, 1), beta = 3 u / sum |u|, so
|eta| < 3; cut-points unevenly spread over [-2, 2]; y uniform in 1..C.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from _ordered import inputs, ol_mp, ol_ref, spread_cuts
from _util import ROOT, check_sums, prebuilt

gpu = pytest.mark.gpu

SMG_OK = 0
SMG_ERR_ARG = 16
CMAX = 16  # the fused path's class cap
FN = "ordered_logistic_glm_lpmf"


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


def with_mp(ref, mp):
    """{name: (mpmath value, ol_ref's absolute-term sum)}."""
    return {k: (mp[k], ref[k][1]) for k in ref}


def extreme_case(R=300):
    """One column, beta = 1, x in {-800, 800, 0, -40, 40}: eta is exactly x;
    y cycles through the three classes, so every class meets every eta (the
    improbable ones included: P ~ exp(-800))."""
    x = np.array([-800.0, 800.0, 0.0, -40.0, 40.0])[np.arange(R) % 5].reshape(R, 1)
    y = (1 + np.arange(R) % 3).astype(np.int32)
    return x, y, np.array([1.0]), np.array([-1.0, 1.5])


def tight_cuts(C):
    """Cut-points with adjacent gaps of 1e-8 (C = 3: one; C = 16: two in a row)."""
    if C == 3:
        return np.array([0.3, 0.3 + 1e-8])
    c = spread_cuts(C).copy()
    c[7] = c[6] + 1e-8
    c[8] = c[7] + 1e-8
    return c


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("case", ["C1", "C2", "C3", "C16", "gap1e-8_C3", "gap1e-8_C16", "eta800"])
def test_reference_against_mpmath(case):
    """No GPU: ol_ref against mpmath (50 digits; 420 for |eta| = 800, where
    1 - logistic(800) needs ~350): every output within 5e-14 of the sum of its
    terms' absolute values."""
    dps = 50
    if case == "eta800":
        x, y, beta, cuts = extreme_case()
        dps = 420
    else:
        R, M, C = {"C1": (300, 5, 1), "C2": (300, 5, 2), "C3": (300, 5, 3), "C16": (300, 8, 16),
                   "gap1e-8_C3": (300, 5, 3), "gap1e-8_C16": (300, 8, 16)}[case]
        x, y, beta, cuts = inputs(R, M, C)
        if case.startswith("gap"):
            cuts = tight_cuts(C)
            assert np.min(np.diff(cuts)) < 1.0001e-8
    ref = ol_ref(y, x, beta, cuts)
    check_sums({k: v[0] for k, v in ref.items()}, with_mp(ref, ol_mp(y, x, beta, cuts, dps)),
               f"ref vs mpmath {case}", b_sum=5e-14, b_rel=None)


# ------------------------------------------------------------ 2. the C entry
def ol_dev(ctx, y, x, beta, cuts, ldx=None, twice=False):
    """smg_ordered_logistic_glm -> {name: value}; x is stored with leading
    dimension ldx, the padding rows NaN, and is a null pointer at M = 0."""
    R, M = x.shape
    C = len(cuts) + 1
    ldx = R if ldx is None else ldx
    xf = np.full((ldx, M), np.nan)
    xf[:R] = x
    ws = ctx.zeros(int(ctx.lib.smg_ordered_logistic_glm_ws_doubles(R, M, C)))
    dy = ctx.put(np.ascontiguousarray(y, dtype=np.int32)) if R else None
    dx = ctx.put(F(xf)) if R * M else None
    dbc = ctx.put(np.concatenate([beta, cuts, [0.0]]))  # (never empty)
    outs = []
    for _ in range(2 if twice else 1):
        out = ctx.put(np.full(M + C, np.nan))
        ctx.call("smg_ordered_logistic_glm", dy, dx, R, M, ldx, C, dbc, ws, out)
        outs.append(ctx.get(out, M + C))
    if twice:
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), "two calls differ bitwise"
    o = outs[0]
    return {"logp": o[0], "beta'": o[1:M + 1], "cuts'": o[M + 1:]}


def check_dev(got, ref, what):
    check_sums(got, ref, what, b_sum=1e-12, b_rel=None)


# R: one row, around one tile, two tiles, 512 workgroups x 32 rows + 1 (a second
# tile on one workgroup: the ping-pong buffers), 1251 tiles (the wrap);
# M: none, one, around one column group, the last column and all 256;
# C: every class count around the binning's edges and the cap.
SHAPES = ([(R, 17, 5, None) for R in (1, 31, 32, 33, 64, 16385, 40003)]
          + [(33, M, 3, None) for M in (0, 1, 15, 16, 17, 255, 256)]
          + [(64, 16, C, None) for C in (1, 2, 3, 5, 16)]
          + [(16385, 255, 2, None), (16385, 15, 1, None), (40003, 1, 16, None), (16385, 0, 16, None),
             (33, 17, 5, 38)])   # ldx = R + 5, NaN padding


@gpu
@pytest.mark.parametrize("R,M,C,ldx", SHAPES)
def test_entry_against_reference(ctx, R, M, C, ldx):
    x, y, beta, cuts = inputs(R, M, C)
    check_dev(ol_dev(ctx, y, x, beta, cuts, ldx), ol_ref(y, x, beta, cuts), f"entry {R}x{M} C={C} ldx={ldx}")


@gpu
def test_entry_null_x_without_columns(ctx):
    """M = 0 with x a null pointer: eta = 0, logp and cuts' as the reference's."""
    x, y, beta, cuts = inputs(31, 0, 5)
    got = ol_dev(ctx, y, x, beta, cuts)
    assert len(got["beta'"]) == 0
    check_dev(got, ol_ref(y, x, beta, cuts), "entry 31x0 C=5, x null")


def class_pattern(name, R, C):
    i = np.arange(R)
    if name == "all_first":
        return np.full(R, 1, dtype=np.int32)
    if name == "all_last":
        return np.full(R, C, dtype=np.int32)
    if name == "all_middle":
        return np.full(R, 3, dtype=np.int32)
    if name == "one_absent":  # class 3 never occurs
        return np.array([1, 2, 4, 5], dtype=np.int32)[i % 4]
    if name == "ends_only":  # classes 2, 3 and 4 never occur
        return np.array([1, 5], dtype=np.int32)[i % 2]
    return (1 + i % C).astype(np.int32)  # alternating within a tile


@gpu
@pytest.mark.parametrize("R", [33, 16385])
@pytest.mark.parametrize("pattern", ["all_first", "all_last", "all_middle", "one_absent", "ends_only", "alternating"])
def test_entry_class_patterns(ctx, pattern, R):
    """C = 5.  A bin that no row feeds is exactly 0.0: with every row in class
    1 only cuts'_1 is fed, with every row in class C only cuts'_{C-1}, with
    every row in class 3 only cuts'_2 and cuts'_3, with classes 1 and 5 alone
    the absent class 3 leaves cuts'_2 and cuts'_3 at 0.0 from both sides; with
    class 3 alone absent every bin is still fed by a neighbour (cuts'_2 from
    class 2 only, cuts'_3 from class 4 only), which the reference's values
    check."""
    C = 5
    x, _, beta, cuts = inputs(R, 17, C)
    y = class_pattern(pattern, R, C)
    got = ol_dev(ctx, y, x, beta, cuts)
    check_dev(got, ol_ref(y, x, beta, cuts), f"pattern {pattern} R={R}")
    fed = {"all_first": [0], "all_last": [3], "all_middle": [1, 2], "ends_only": [0, 3]}.get(pattern, [0, 1, 2, 3])
    for j in range(C - 1):
        if j not in fed:
            assert got["cuts'"][j] == 0.0 and not np.signbit(got["cuts'"][j]), (pattern, j, got["cuts'"][j])
        else:
            assert got["cuts'"][j] != 0.0, (pattern, j)


@gpu
def test_entry_extreme_predictors(ctx):
    """|eta| = 800 with y in the improbable class (P ~ exp(-800)): every output
    is finite and within the bound of the 420-digit mpmath reference."""
    x, y, beta, cuts = extreme_case(64)
    got = ol_dev(ctx, y, x, beta, cuts)
    for k, v in got.items():
        assert np.all(np.isfinite(v)), (k, v)
    ref = ol_ref(y, x, beta, cuts)
    assert ref["logp"][0] < -800.0 * 10
    check_dev(got, with_mp(ref, ol_mp(y, x, beta, cuts, 420)), "extremes |eta| = 800")


@gpu
@pytest.mark.parametrize("C", [3, 16])
def test_entry_adjacent_cut_points(ctx, C):
    """Adjacent cut-points 1e-8 apart (lm ~ -18.4, r ~ 1e8) against mpmath."""
    x, y, beta, _ = inputs(300, 5 if C == 3 else 8, C)
    cuts = tight_cuts(C)
    got = ol_dev(ctx, y, x, beta, cuts)
    for k, v in got.items():
        assert np.all(np.isfinite(v)), (k, v)
    check_dev(got, with_mp(ol_ref(y, x, beta, cuts), ol_mp(y, x, beta, cuts)), f"gap 1e-8 C={C}")


@gpu
def test_entry_two_calls_bitwise_equal(ctx):
    x, y, beta, cuts = inputs(40003, 17, 5)
    ol_dev(ctx, y, x, beta, cuts, twice=True)


@gpu
def test_entry_argument_errors_and_empty(ctx):
    """C = 0, R < 0, ldx < R, M = 257, C = cap + 1, null parameters:
    SMG_ERR_ARG, nothing written, the context's status untouched; R = 0 writes
    M + C zeros."""
    R, M, C = 33, 17, 5
    x, y, beta, cuts = inputs(R, M, C)
    lib = ctx.lib
    ws = ctx.zeros(int(max(lib.smg_ordered_logistic_glm_ws_doubles(R, 257, CMAX + 1), 1)))
    dy, dx = ctx.put(y), ctx.put(F(x))
    dbc = ctx.put(np.concatenate([beta, cuts, np.zeros(300)]))
    out = ctx.put(np.full(M + C, np.nan))
    f = lib.smg_ordered_logistic_glm
    assert f(ctx.ptr, dy, dx, R, M, R, 0, dbc, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, dy, dx, -1, M, R, C, dbc, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, dy, dx, R, M, R - 1, C, dbc, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, dy, dx, R, 257, R, C, dbc, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, dy, dx, R, M, R, CMAX + 1, dbc, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, dy, dx, R, -1, R, C, dbc, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, dy, dx, R, M, R, C, None, ws, out) == SMG_ERR_ARG
    assert f(ctx.ptr, None, dx, R, M, R, C, dbc, ws, out) == SMG_ERR_ARG
    assert np.all(np.isnan(ctx.get(out, M + C)))  # nothing was written
    assert ctx.status() == 0
    assert f(ctx.ptr, dy, dx, R, M, R, CMAX, dbc, ws, out) == SMG_OK  # the cap itself is accepted (y <= 5 < 16)
    ctx.call("smg_ordered_logistic_glm", None, None, 0, M, 0, C, dbc, ws, out)
    assert np.array_equal(ctx.get(out, M + C), np.zeros(M + C))
    assert ctx.status() == 0


@gpu
def test_entry_out_of_range_y_is_clamped(ctx):
    """A row with y = C + 1 and one with y = 0 among valid rows: the lookups
    are clamped into the cut-point arrays, the call returns SMG_OK and the
    context's status stays 0 (a bounds-safety check, not a value check; the
    other bins still hold finite sums)."""
    R, M, C = 33, 17, 5
    x, y, beta, cuts = inputs(R, M, C)
    y = y.copy()
    y[7], y[20] = C + 1, 0
    got = ol_dev(ctx, y, x, beta, cuts)
    assert ctx.status() == 0
    y2 = y.copy()
    y2[3], y2[30] = 2**31 - 1, -2**31
    ol_dev(ctx, y2, x, beta, cuts)
    assert ctx.status() == 0
    assert np.isfinite(got["logp"])


# ------------------------------------------------------------ 3. through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_glm_ordered")
TAPE = (1000, 8, 5)
KINDS = ["vv", "vd", "dv"]


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@functools.lru_cache(maxsize=None)
def tape():
    """One run of the binary's "tape" mode at TAPE, shared by the tests below:
    ({tag: values}, the reference sums)."""
    R, M, C = TAPE
    x, y, beta, cuts = inputs(R, M, C)
    nums = np.concatenate([y.astype(np.float64), F(x), beta, cuts])
    out = _run(f"tape {R} {M} {C}\n" + " ".join(repr(float(v)) for v in nums) + "\n")
    res = {}
    for line in out.strip().splitlines():
        tag, *vals = line.split()
        res[tag] = np.array([float(v) for v in vals])
    return res, ol_ref(y, x, beta, cuts)


def check_grad(g, kinds, ref, what):
    """The gradient over the var arguments of `kinds` within the entry's bounds."""
    M, K = len(ref["beta'"][0]), len(ref["cuts'"][0])
    at, got = 0, {}
    if kinds[0] == "v":
        got["beta'"] = g[:M]
        at = M
    if kinds[1] == "v":
        got["cuts'"] = g[at:at + K]
        at += K
    assert at == len(g), (kinds, len(g))
    check_dev(got, ref, what)


@gpu
@pytest.mark.parametrize("kinds", KINDS)
def test_tape_every_kind_and_propto(kinds):
    """Value and gradient for each var / double combination of (beta, cuts);
    propto with a var operand drops nothing: the same bits."""
    r, ref = tape()
    check_dev({"logp": r["fx_" + kinds][0]}, ref, f"tape {kinds}")
    check_grad(r["grad_" + kinds], kinds, ref, f"tape {kinds}")
    assert r["fxp_" + kinds][0] == r["fx_" + kinds][0]
    assert np.array_equal(r["gradp_" + kinds], r["grad_" + kinds])
    assert r["fx_" + kinds][0] == r["fx_vv"][0]


@gpu
def test_tape_all_double_and_stack():
    r, ref = tape()
    check_dev({"logp": r["fx_dd"][0]}, ref, "tape dd")
    assert r["fx_dd"][0] == r["fx_vv"][0]
    assert r["fxp_dd"][0] == 0.0
    assert r["fx_eigen_dd"][0] == r["fx_dd"][0]
    assert list(r["stack"]) == [0.0, 0.0]


@gpu
def test_tape_shards_distributed_eigen_host_leaf():
    """Seven row shards summed on one tape equal the single call within the
    entry's bounds; one distributed shard under a one-rank host collective,
    the Eigen signature and host vectors give the dev_data call's bits; beta
    as the device leaf of gradient() gives beta'."""
    r, ref = tape()
    R, M, C = TAPE
    check_dev({"logp": r["fx_shards7"][0]}, ref, "tape shards7")
    check_grad(r["grad_shards7"], "vv", ref, "tape shards7")
    for tag in ("dist", "eigen", "host"):
        assert r["fx_" + tag][0] == r["fx_vv"][0], tag
        assert np.array_equal(r["grad_" + tag], r["grad_vv"]), tag
    assert r["fx_leaf"][0] == r["fx_vv"][0]
    assert np.array_equal(r["grad_leaf"], r["grad_vv"][:M])


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
def test_cpp_argument_errors():
    """The checks in their order (wording as recalled from Stan Math), thrown
    with the tape left empty; an input that violates two checks reports the
    earlier one."""
    e = errors()
    assert e["ok"][0] == "value" and np.isfinite(float(e["ok"][1])) and float(e["ok"][1]) < 0
    assert e["y_size"] == ("invalid_argument",
                           f"{FN}: Vector of dependent variables has dimension = 3, expecting dimension = 4" + SIZES)
    assert e["y_size_eigen"] == e["y_size"]
    assert e["beta_size"] == ("invalid_argument",
                              f"{FN}: Weight vector has dimension = 3, expecting dimension = 2" + SIZES)
    assert e["beta_size_and_y"] == e["beta_size"]
    y_high = ("domain_error", f"{FN}: Vector of dependent variables[3] is 4, but must be in the interval [1, 3]")
    assert e["y_high"] == y_high
    assert e["y_high_double"] == y_high
    assert e["y_high_propto_double"] == y_high
    assert e["y_zero"] == ("domain_error",
                           f"{FN}: Vector of dependent variables[2] is 0, but must be in the interval [1, 3]")
    assert e["y_shard_row0"] == ("domain_error",
                                 f"{FN}: Vector of dependent variables[13] is 4, but must be in the interval [1, 3]")
    assert e["y_and_cuts"] == y_high
    unordered = ("domain_error", f"{FN}: Cut-points is not a valid ordered vector. The element at 2 is -0.5, "
                                 "but should be greater than the previous element, 0.7")
    assert e["cuts_unordered"] == unordered
    assert e["cuts_unordered_double"] == unordered
    assert e["cuts_equal"] == ("domain_error", f"{FN}: Cut-points is not a valid ordered vector. The element at 2 "
                                               "is 0.5, but should be greater than the previous element, 0.5")
    assert e["cuts_nan"] == ("domain_error", f"{FN}: Cut-points is not a valid ordered vector. The element at 2 "
                                             "is nan, but should be greater than the previous element, -0.5")
    assert e["cuts_unordered_and_inf"] == ("domain_error",
                                           f"{FN}: Cut-points is not a valid ordered vector. The element at 2 is 0.5, "
                                           "but should be greater than the previous element, inf")
    assert e["cut_last_inf"] == ("domain_error", f"{FN}: Final cut-point is inf, but must be finite!")
    assert e["cut_first_inf"] == ("domain_error", f"{FN}: First cut-point is -inf, but must be finite!")
    assert e["nonfinite_beta"] == ("domain_error", f"{FN}: Weight vector[1] is inf, but must be finite!")
    nonfinite_x = ("domain_error", f"{FN}: Matrix of independent variables is not finite, but must be finite!")
    assert e["nonfinite_x"] == nonfinite_x
    assert e["infinite_x"] == nonfinite_x
    assert e["empty_y"] == ("value", "0")
    assert e["all_data_propto"] == ("value", "0")
    assert e["one_class"] == ("value", "0")
    assert e["one_class_grad"] == ("value", "0")
    assert e["one_class_y2"] == ("domain_error",
                                 f"{FN}: Vector of dependent variables[2] is 2, but must be in the interval [1, 1]")
    assert e["stack"] == ("0", "0")
