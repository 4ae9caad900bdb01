"""Element-wise arithmetic and transforms on device vectors: the C entries
smg_elt_unary_* / smg_elt_binary_* through ctypes, and the stan::math overloads
through the tape (tests/cpp/test_elt_ops.cpp).

The reference of every device test is `_elt.unary_ref` / `binary_ref`, a
float64 numpy restatement of the kernels' formulas, with reduced sums by
math.fsum.  The reference is checked against 60-digit mpmath without a GPU
(test_reference_against_mpmath).

Bounds (tests/_elt.py `worst`): every element of a value or of a vector
adjoint on the scale of its own magnitude; an adjoint added into a non-zero
starting adjoint on the sum of the absolute values of its terms; a reduced
scalar on the sum of its terms' absolute values.  Where the reference is NaN
or +-inf the result must be of the same class and sign.

    yardstick (reference against mpmath): asserted at 5e-14; measured worst
        ratios, main grid (400 points in [-30, 30]) / extreme grid:
        (0: equal to the correctly rounded mpmath value at every point)
        values      exp 2.2e-16 / 1.4e-16, log 0 / 0, sqrt 0 / 0, square 0 / 0, inv 0 / 0,
                    inv_logit 3.5e-16 / 0, log_inv_logit 2.2e-16 / 1.8e-16, log1p_exp 2.2e-16 / 1.8e-16,
                    tanh 1.8e-16 / 0
        partials    exp 2.2e-16 / 1.4e-16, log 0 / 0, sqrt 2.2e-16 / 1.9e-16, square 0 / 0,
                    inv 3.8e-16 / 1.7e-16, inv_logit 4.1e-16 / 1.4e-16, log_inv_logit 2.2e-16 / 0,
                    log1p_exp 3.5e-16 / 0, tanh 3.7e-16 / 1.5e-16
        binary partials: 0 but elt_divide's b partial, 2.2e-16 / 0; their fsum-reduced sums <= 1.5e-16
    device against the reference: 1e-12, every output (the project's bound
        for every device reducer; it holds because the yardstick is under 5e-14)
    forward values of add, subtract, elt_multiply and square: numpy's bits

Launch rule (smg_elt_launch_shape): 256-thread blocks, at most 8192 of them,
one 8-byte element or two adjacent ones (16 bytes) per lane and trip (by
default 16 bytes, the binary reverse 8; smg_elt_set_width forces either); the
second-trip size is computed from it.  The reducing reverse follows
k_normal_fused: one 1024-thread block up to 4096 elements, then
ceil(n / 4096) blocks up to 512, so 4097 is its first two-block launch.
"""
import functools
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import gen
from _elt import (A0, B0, BINARY, POSITIVE, SENTINEL, SMG_ERR_ARG, SMG_OK, UNARY, Buf, binary_fwd, binary_inputs, binary_mp,
                  binary_ref, binary_rev, device_extremes, extreme_grid, launch_shape, main_grid, second_trip_size,
                  unary_fwd, unary_inputs, unary_mp, unary_ref, unary_rev, worst)
from _reducers import same_bits
from _util import ROOT, prebuilt

gpu = pytest.mark.gpu
BOUND = 1e-12
SMALL = [1, 2, 3, 63, 64, 65, 255, 257, 4097]
WIDTHS = [1, 2]
EXACT = ("add", "subtract", "elt_multiply", "square")


@pytest.fixture(scope="module")
def ctx():
    from math_amd import hip
    c = hip.Context(0, 1 << 30)
    prev = c.lib.smg_elt_set_width(c.ptr, -1)
    yield c
    c.lib.smg_elt_set_width(c.ptr, prev)
    c.close()


@pytest.fixture(autouse=True)
def _rewind(request):
    if "ctx" not in request.fixturenames:
        yield
        return
    c = request.getfixturevalue("ctx")
    m = c.mark()
    prev = c.lib.smg_elt_set_width(c.ptr, -1)
    yield
    c.lib.smg_elt_set_width(c.ptr, prev)
    assert c.status() == 0
    c.rewind(m)


def check(got, ref, what, scale=None, bound=BOUND):
    r = worst(got, ref, scale)
    print(f"{what}: worst ratio {r:.3e}")
    assert r <= bound, (what, r)
    return r


def fsum_pair(terms):
    return math.fsum(terms), math.fsum(np.abs(terms))


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("grid", ["main", "extreme"])
def test_reference_against_mpmath(grid):
    """No GPU: the float64 reference against 60-digit mpmath at 5e-14: every
    unary value and partial on each function's grid, and every binary partial
    with its fsum-reduced sums (operands from the main grid / the extreme
    grid's finite non-zero points)."""
    for name in UNARY:
        x = main_grid(name) if grid == "main" else extreme_grid(name)
        y, d = unary_ref(name, x)
        ym, dm = unary_mp(name, x)
        check(y, ym, f"ref vs mpmath {grid} {name}", bound=5e-14)
        check(d, dm, f"ref vs mpmath {grid} {name}'", bound=5e-14)
    if grid == "main":
        a, b, ca = main_grid("exp"), main_grid("log") * np.sign(main_grid("exp")[::-1]), main_grid("tanh")[::-1] / 15.0
    else:
        g = extreme_grid("exp")
        g = g[(g != 0.0) & (np.abs(g) < 700.0) & (np.abs(g) > 1e-200)]
        a, b, ca = g, g[::-1].copy(), np.roll(g, 3)
    for name in BINARY:
        _, da, db = binary_ref(name, a, b, ca)
        dam, dbm, sam, sbm = binary_mp(name, a, b, ca)
        check(da, dam, f"ref vs mpmath {grid} {name} a'", bound=5e-14)
        check(db, dbm, f"ref vs mpmath {grid} {name} b'", bound=5e-14)
        for s, terms, what in ((sam, da, "a"), (sbm, db, "b")):
            v, sc = fsum_pair(terms)
            check(v, s, f"ref vs mpmath {grid} {name} sum {what}'", scale=sc, bound=5e-14)


# ------------------------------------------------------------ 2. the C entries
def check_unary(ctx, name, n, mis_fwd=(False, False), mis_rev=(False,) * 4, what=""):
    """Forward, then reverse added into a non-zero adjoint."""
    x, ya, xa0 = unary_inputs(name, n)
    y_ref, d_ref = unary_ref(name, x)
    y, _ = unary_fwd(ctx, name, x, mis_fwd)
    check(y, y_ref, f"{name} n={n} {what} value")
    if name in EXACT:
        assert same_bits(y, y_ref), name
    xa = unary_rev(ctx, name, x, y, ya, xa0, mis_rev)
    check(xa, xa0 + ya * d_ref, f"{name} n={n} {what} xadj", scale=np.abs(xa0) + np.abs(ya * d_ref))


def check_binary(ctx, name, n, mis_fwd=(False,) * 3, mis_rev=(False,) * 5, what=""):
    """Vector / vector: forward, then reverse added into non-zero adjoints."""
    a, b, ca, aa0, ba0 = binary_inputs(n)
    c_ref, da, db = binary_ref(name, a, b, ca)
    c = binary_fwd(ctx, name, a, b, n, mis_fwd)
    check(c, c_ref, f"{name} n={n} {what} value")
    if name in EXACT:
        assert same_bits(c, c_ref), name
    aa, ba, red = binary_rev(ctx, name, a, b, n, ca, aa0, ba0, 0, mis_rev)
    check(aa, aa0 + da, f"{name} n={n} {what} aadj", scale=np.abs(aa0) + np.abs(da))
    check(ba, ba0 + db, f"{name} n={n} {what} badj", scale=np.abs(ba0) + np.abs(db))
    assert np.all(red == SENTINEL)


@gpu
@pytest.mark.parametrize("n", SMALL + ["second trip"])
@pytest.mark.parametrize("width", [0] + WIDTHS)
def test_sizes(ctx, width, n):
    """inv_logit and elt_divide over every size, with the default widths (0:
    16 bytes but for the binary reverse), in the 8-byte and in the 16-byte
    form; the last size, from the entry's launch constants, puts a lane of
    every kernel on its second grid-stride trip."""
    ctx.lib.smg_elt_set_width(ctx.ptr, width)
    shape = launch_shape(ctx)
    assert width == 0 or shape["width"] == shape["binary_rev_width"] == width
    if n == "second trip":
        n = second_trip_size(shape)
        if (shape["threads"], shape["max_blocks"]) == (256, 8192):
            assert n == (2097153 if width == 1 else 4194307)
    check_unary(ctx, "inv_logit", n, what=f"width {width}")
    check_binary(ctx, "elt_divide", n, what=f"width {width}")


@gpu
@pytest.mark.parametrize("name", [f for f in UNARY + BINARY if f not in ("inv_logit", "elt_divide")])
def test_every_other_operation(ctx, name):
    """n = 65 and 4097, both access widths."""
    for width, n in itertools.product(WIDTHS, (65, 4097)):
        ctx.lib.smg_elt_set_width(ctx.ptr, width)
        (check_unary if name in UNARY else check_binary)(ctx, name, n, what=f"width {width}")


@gpu
@pytest.mark.parametrize("n", [65, 4097])
def test_alignment(ctx, n):
    """Buffers one double past a 16-byte boundary (the call then takes the
    8-byte form): for elt_multiply each of a, b, c and of a, b, cadj, aadj,
    badj on its own; for every other operation all of them together.  The
    sentinels around every output show an overstep."""
    assert launch_shape(ctx)["width"] in WIDTHS
    for k in range(3):
        check_binary(ctx, "elt_multiply", n, mis_fwd=tuple(i == k for i in range(3)), what=f"fwd misaligned {k}")
    for k in range(5):
        check_binary(ctx, "elt_multiply", n, mis_rev=tuple(i == k for i in range(5)), what=f"rev misaligned {k}")
    for name in BINARY:
        check_binary(ctx, name, n, (True,) * 3, (True,) * 5, what="all misaligned")
    for name in UNARY:
        check_unary(ctx, name, n, (True, True), (True,) * 4, what="all misaligned")
    for k in range(4):
        check_unary(ctx, "inv_logit", n, mis_rev=tuple(i == k for i in range(4)), what=f"rev misaligned {k}")


@gpu
@pytest.mark.parametrize("name", BINARY)
def test_binary_forms(ctx, name):
    """n = 4097: vector / vector, vector / scalar and scalar / vector; every
    subset of wanted vector adjoints (one not asked for: a NULL pointer,
    nothing written); want_scalar 0 to 3 (a slot not asked for, or of a vector
    operand, keeps its sentinel); red against the fsum reference; a second
    call overwrites red."""
    n = 4097
    a, b, ca, aa0, ba0 = binary_inputs(n)
    for av, bv in ((a, b), (a, B0), (A0, b)):
        c_ref, da, db = binary_ref(name, av, bv, ca)
        c = binary_fwd(ctx, name, av, bv, n)
        form = f"{name} {'v' if av is a else 's'}/{'v' if bv is b else 's'}"
        check(c, c_ref, f"{form} value")
        if name in EXACT:
            assert same_bits(c, c_ref), form
        for wa, wb, ws in itertools.product((True, False), (True, False), range(4)):
            aa, ba, red = binary_rev(ctx, name, av, bv, n, ca, aa0 if wa else None, ba0 if wb else None, ws)
            what = f"{form} want {int(wa)}{int(wb)} scalar {ws}"
            if wa and av is a:
                check(aa, aa0 + da, what + " aadj", scale=np.abs(aa0) + np.abs(da))
            elif wa:
                assert same_bits(aa, aa0), what  # a scalar operand has no vector adjoint: untouched
            if wb and bv is b:
                check(ba, ba0 + db, what + " badj", scale=np.abs(ba0) + np.abs(db))
            elif wb:
                assert same_bits(ba, ba0), what
            for slot, is_scalar, terms in ((0, av is not a, da), (1, bv is not b, db)):
                if is_scalar and (ws >> slot) & 1:
                    v, sc = fsum_pair(terms)
                    check(red[slot], v, what + f" red[{slot}]", scale=sc)
                else:
                    assert red[slot] == SENTINEL, (what, slot, red)
    # written, not accumulated
    once = binary_rev(ctx, name, a, B0, n, ca, None, None, 2)[2]
    twice = binary_rev(ctx, name, a, B0, n, ca, None, None, 2, calls=2)[2]
    assert same_bits(once, twice)


@gpu
@pytest.mark.parametrize("name", UNARY + BINARY)
def test_reverse_accumulates(ctx, name):
    """Two reverse calls on the same buffers add their term twice into the
    non-zero adjoints that were there."""
    n = 257
    if name in UNARY:
        x, ya, xa0 = unary_inputs(name, n)
        y, d = unary_ref(name, x)
        bufs = [Buf(ctx, v) for v in (x, y, ya, xa0)]
        for _ in range(2):
            ctx.call("smg_elt_unary_rev", UNARY.index(name), bufs[0].ptr, bufs[1].ptr, n, bufs[2].ptr, bufs[3].ptr)
        check(bufs[3].read(), xa0 + 2.0 * (ya * d), f"{name} twice", scale=np.abs(xa0) + 2.0 * np.abs(ya * d))
    else:
        a, b, ca, aa0, ba0 = binary_inputs(n)
        _, da, db = binary_ref(name, a, b, ca)
        aa, ba, _ = binary_rev(ctx, name, a, b, n, ca, aa0, ba0, calls=2)
        check(aa, aa0 + 2.0 * da, f"{name} twice aadj", scale=np.abs(aa0) + 2.0 * np.abs(da))
        check(ba, ba0 + 2.0 * db, f"{name} twice badj", scale=np.abs(ba0) + 2.0 * np.abs(db))


@gpu
@pytest.mark.parametrize("name", BINARY)
def test_aliased_adjoints(ctx, name):
    """The same node as both operands: a == b and aadj == badj.  The adjoint
    receives both contributions (a kernel with __restrict__ adjoints loses
    one), at n = 65 and 4097 in both widths and misaligned."""
    for width, n, mis in itertools.product(WIDTHS, (65, 4097), (False, True)):
        ctx.lib.smg_elt_set_width(ctx.ptr, width)
        a, _, ca, aa0, _ = binary_inputs(n)
        a = np.where(np.abs(a) < 0.05, 0.05, a)  # (a is its own divisor)
        _, da, db = binary_ref(name, a, a, ca)
        aa, ba, _ = binary_rev(ctx, name, a, None, n, ca, aa0, None, 0, mis=(mis,) * 5, alias=True)
        assert same_bits(aa, ba)
        check(aa, aa0 + da + db, f"{name} aliased n={n} width {width} mis {mis}",
              scale=np.abs(aa0) + np.abs(da) + np.abs(db))


@gpu
def test_scalar_reduction_repeatable(ctx):
    """Two calls with a scalar reduction give the same bits in red: n = 4097,
    the smallest size with two blocks of the reduction (from the launch
    constants) and one with many blocks and a ragged tail; both widths and
    both scalar positions."""
    shape = launch_shape(ctx)
    two_blocks = shape["red_per_block"] + 1
    for width, n, name in itertools.product(WIDTHS, sorted({4097, two_blocks, 37 * shape["red_per_block"] + 13}), BINARY):
        ctx.lib.smg_elt_set_width(ctx.ptr, width)
        a, b, ca, aa0, ba0 = binary_inputs(n)
        for av, bv, ws in ((a, B0, 2), (A0, b, 1), (A0, B0, 3)):
            r1 = binary_rev(ctx, name, av, bv, n, ca, aa0, ba0, ws)
            r2 = binary_rev(ctx, name, av, bv, n, ca, aa0, ba0, ws)
            assert same_bits(r1[2], r2[2]), (name, n, width, ws)
            _, da, db = binary_ref(name, av, bv, ca)
            for slot, terms in ((0, da), (1, db)):
                if (ws >> slot) & 1:
                    v, sc = fsum_pair(terms)
                    check(r1[2][slot], v, f"{name} n={n} width {width} red[{slot}]", scale=sc)


@gpu
@pytest.mark.parametrize("name", UNARY)
def test_unary_extremes(ctx, name):
    """0, -0.0, +-1e-300, +-1e-8, +-1, +-36.05, +-40, +-709, +-745, +-1e300,
    NaN and +-inf, forward and reverse (into a zero adjoint, with incoming
    adjoints of both signs): within the bound of the reference where it is
    finite, the same class and sign where it is NaN or +-inf; out-of-domain
    input is no error."""
    x = device_extremes()
    ya = np.where(np.arange(len(x)) % 3 == 0, -1.5, 0.75)
    y_ref, d_ref = unary_ref(name, x)
    for width, mis in itertools.product(WIDTHS, (False, True)):
        ctx.lib.smg_elt_set_width(ctx.ptr, width)
        y, _ = unary_fwd(ctx, name, x, (mis, mis))
        check(y, y_ref, f"{name} extremes width {width} value")
        xa = unary_rev(ctx, name, x, y_ref, ya, np.zeros(len(x)), (mis,) * 4)
        with np.errstate(all="ignore"):
            check(xa, ya * d_ref, f"{name} extremes width {width} xadj")
    assert ctx.status() == 0


@gpu
def test_arguments(ctx):
    """n = 0 is SMG_OK and writes nothing; a null context, n < 0, an unknown
    op or a NULL output is SMG_ERR_ARG; the context's status stays 0."""
    lib, p = ctx.lib, ctx.ptr
    n = 33
    x, ya, xa0 = unary_inputs("exp", n)
    bx, by, bya, bxa, bred = Buf(ctx, x), Buf(ctx, np.full(n, SENTINEL)), Buf(ctx, ya), Buf(ctx, np.full(n, SENTINEL)), \
        Buf(ctx, np.full(2, SENTINEL))
    uf, ur, bf, br = lib.smg_elt_unary_fwd, lib.smg_elt_unary_rev, lib.smg_elt_binary_fwd, lib.smg_elt_binary_rev
    assert uf(p, 0, bx.ptr, 0, by.ptr) == SMG_OK
    assert ur(p, 0, bx.ptr, by.ptr, 0, bya.ptr, bxa.ptr) == SMG_OK
    assert bf(p, 0, bx.ptr, bya.ptr, 0.0, 0.0, 0, by.ptr) == SMG_OK
    assert br(p, 0, bx.ptr, None, 0.0, 1.0, 0, bya.ptr, bxa.ptr, None, 2, bred.ptr) == SMG_OK
    for bad_ctx, bad_n, bad_op in ((None, n, 0), (p, -1, 0), (p, n, -1), (p, n, 9)):
        assert uf(bad_ctx, bad_op, bx.ptr, bad_n, by.ptr) == SMG_ERR_ARG
        assert ur(bad_ctx, bad_op, bx.ptr, by.ptr, bad_n, bya.ptr, bxa.ptr) == SMG_ERR_ARG
    for bad_ctx, bad_n, bad_op in ((None, n, 0), (p, -1, 0), (p, n, -1), (p, n, 4)):
        assert bf(bad_ctx, bad_op, bx.ptr, bya.ptr, 0.0, 0.0, bad_n, by.ptr) == SMG_ERR_ARG
        assert br(bad_ctx, bad_op, bx.ptr, None, 0.0, 1.0, bad_n, bya.ptr, bxa.ptr, None, 2, bred.ptr) == SMG_ERR_ARG
    assert uf(p, 0, bx.ptr, n, None) == SMG_ERR_ARG
    assert ur(p, 0, bx.ptr, by.ptr, n, bya.ptr, None) == SMG_ERR_ARG
    assert bf(p, 0, bx.ptr, bya.ptr, 0.0, 0.0, n, None) == SMG_ERR_ARG
    assert br(p, 0, bx.ptr, None, 0.0, 1.0, n, bya.ptr, bxa.ptr, None, 2, None) == SMG_ERR_ARG
    ctx.sync()
    for b in (by, bxa, bred):
        assert np.all(b.read() == SENTINEL)  # nothing was written
    assert ctx.status() == 0


# ------------------------------------------------------------ 3. through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_elt_ops")
TAPE_N = 64
HS_M = 8
C0 = 1.7


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _nums(*parts):
    return " ".join(repr(float(v)) for part in parts for v in np.atleast_1d(part))


@functools.lru_cache(maxsize=None)
def tape_data():
    """a in (-5, 5), b positive, the weights w in +-(0.2, 2), positive data d."""
    N = TAPE_N
    a = gen.unif(gen.SEED + 930, N, -5.0, 5.0)
    b = np.exp(gen.unif(gen.SEED + 931, N, -1.5, 1.5))
    w = gen.unif(gen.SEED + 932, N, 0.2, 2.0) * np.where(gen.u01(gen.SEED + 933, N) < 0.5, -1.0, 1.0)
    d = np.exp(gen.unif(gen.SEED + 934, N, -1.0, 1.0))
    return a, b, w, d


@functools.lru_cache(maxsize=None)
def model_data():
    from _heavy_tail import T_TABLE
    N, M = TAPE_N, HS_M
    x = np.linspace(-3.0, 3.0, N) + gen.unif(gen.SEED + 940, N, -0.02, 0.02)
    gs, gl, mu = 1.1, 0.6, 0.4
    eta = gen.unif(gen.SEED + 941, N, -1.0, 1.0)
    K = gs**2 * np.exp(-0.5 * (x[:, None] - x[None, :])**2 / gl**2) + 1e-6 * np.eye(N)
    f = mu + np.linalg.cholesky(K) @ eta
    yc = np.floor(np.exp(f) * -np.log1p(-gen.u01(gen.SEED + 942, N)))
    gp = (x, [gs, gl, mu], eta, yc)
    f0, g0 = gen.unif(gen.SEED + 943, N, -1.0, 1.0), gen.unif(gen.SEED + 944, N, -0.7, 0.7)
    yh = f0 + np.exp(g0) * T_TABLE[(gen.u01(gen.SEED + 945, N) * len(T_TABLE)).astype(np.int64)]
    het = (yh, f0, g0, [3.5])
    X = gen.unif(gen.SEED + 946, N * M, -1.0, 1.0)
    z0, l0 = gen.unif(gen.SEED + 947, M, -1.5, 1.5), np.exp(gen.unif(gen.SEED + 948, M, -1.0, 1.0))
    tau, sigma = 0.3, 0.8
    ys = X.reshape(M, N).T @ (tau * z0 * l0) + sigma * gen.unif(gen.SEED + 949, N, -1.0, 1.0)
    hs = (X, ys, z0, l0, [tau, sigma])
    return gp, het, hs


def scalar_grid(fn):
    return extreme_grid("inv" if fn == "inv" else "exp")


@functools.lru_cache(maxsize=None)
def tape():
    """One run of the binary over every mode but the errors: {tag: values}."""
    a, b, w, d = tape_data()
    gp, het, hs = model_data()
    grid = np.concatenate([scalar_grid("tanh"), [1e300]])
    out = _run(f"tape {TAPE_N}\n{_nums(a, b, w, d, C0)}\nscalars {len(grid)}\n{_nums(grid)}\n"
               f"gp {TAPE_N}\n{_nums(*gp)}\nhet {TAPE_N}\n{_nums(*het)}\nhs {TAPE_N} {HS_M}\n{_nums(*hs)}\narena\n")
    res = {}
    for line in out.strip().splitlines():
        tag, _, vals = line.partition(" ")
        res[tag] = np.array(vals.split(), dtype=np.float64)
    res["scalar grid"] = grid
    return res


def check_tape(r, tag, value_terms, grads):
    """fx and the gradient of `tag`, device and host, against the reference:
    value_terms: the terms of the objective (arrays); grads: per var operand
    either ("vec", terms...) -- element-wise, the scale each element's sum of
    absolute terms -- or ("sum", terms) -- one entry, the fsum of the terms."""
    terms = np.concatenate([np.ravel(t) for t in value_terms])
    fx, fsc = fsum_pair(terms)
    ref, scale = [], []
    for kind, *ts in grads:
        if kind == "vec":
            ref.append(np.sum(ts, axis=0))
            scale.append(np.sum(np.abs(ts), axis=0))
        else:
            v, sc = fsum_pair(np.ravel(ts[0]))
            ref.append([v])
            scale.append([sc])
    ref, scale = np.concatenate(ref), np.concatenate(scale)
    for path in ("dev", "host"):
        check(r[f"fx_{tag}_{path}"][0], fx, f"tape {tag} {path} value", scale=fsc)
        check(r[f"grad_{tag}_{path}"], ref, f"tape {tag} {path} gradient", scale=scale)
    check(r[f"grad_{tag}_dev"], r[f"grad_{tag}_host"], f"tape {tag} dev against host", scale=scale)


@gpu
@pytest.mark.parametrize("fn", UNARY)
def test_tape_unary(fn):
    """dot_product(w, fn(x)) at N = 64: value and gradient on the device,
    composed of host scalar vars, and from the numpy reference."""
    a, b, w, _ = tape_data()
    x = b if fn in POSITIVE else a
    y, d = unary_ref(fn, x)
    check_tape(tape(), f"u_{fn}", [w * y], [("vec", w * d)])


BINARY_TAPE = [(fn, k) for fn in ("add", "subtract", "elt_multiply", "elt_divide") for k in ("vv", "vd", "dv")] + \
              [(fn, k) for fn in ("add", "subtract") for k in ("vs", "vc", "sv", "cv")] + \
              [("divide", "vs"), ("divide", "vc"), ("elt_divide", "sv"), ("elt_divide", "cv")]


@gpu
@pytest.mark.parametrize("fn,kinds", BINARY_TAPE)
def test_tape_binary(fn, kinds):
    """Every overload: v a var matrix, d a data matrix, s a scalar var, c a
    double; the gradient over the var operands in order."""
    a, b, w, d = tape_data()
    A = {"v": a, "d": d, "s": C0, "c": C0}[kinds[0]]
    B = {"v": b, "d": d, "s": C0, "c": C0}[kinds[1]]
    c, da, db = binary_ref("elt_divide" if fn == "divide" else fn, A, B, w)
    grads = [("vec" if k == "v" else "sum", t) for k, t in zip(kinds, (da, db)) if k in "vs"]
    check_tape(tape(), f"b_{fn}_{kinds}", [w * c], grads)


@gpu
def test_tape_one_operand_in_two_places():
    """elt_multiply(x, x) and subtract(exp(x), x): a node's adjoint fed by two consumers."""
    a, _, w, _ = tape_data()
    check_tape(tape(), "two_mul", [w * (a * a)], [("vec", w * a, w * a)])
    check_tape(tape(), "two_sub", [w * np.exp(a), -w * a], [("vec", w * np.exp(a), -w)])


@gpu
@pytest.mark.parametrize("fn", ["inv", "inv_logit", "log_inv_logit", "log1p_exp", "tanh"])
def test_tape_new_scalar_overloads(fn):
    """The scalar var overloads on the extreme grid (inv: its positive points
    and 1e300) against the reference."""
    r = tape()
    keep = np.isin(r["scalar grid"], scalar_grid(fn)) if fn != "inv" else r["scalar grid"] > 0.0
    x = r["scalar grid"][keep]
    y, d = unary_ref(fn, x)
    check(r[f"sv_{fn}"][keep], y, f"scalar {fn} value")
    check(r[f"sg_{fn}"][keep], d, f"scalar {fn} derivative")


@gpu
@pytest.mark.parametrize("model", ["gp", "het", "hs"])
def test_tape_composed_models(model):
    """The shifted latent GP (f = add(mu, multiply(L, eta)) as the Poisson
    GLM's per-row intercept), the heteroscedastic robust regression
    (student_t_lpdf(y | nu, f, exp(g))) and the horseshoe (beta = multiply(tau,
    elt_multiply(z, lambda))): the gradient over all parameters against the
    host-composed model within 1e-12 of max(|entry|, 1e-3 |gradient|_inf)."""
    r = tape()
    gd, gh = r[f"grad_{model}_dev"], r[f"grad_{model}_host"]
    assert len(gd) == {"gp": TAPE_N + 3, "het": 2 * TAPE_N + 1, "hs": 2 * HS_M + 2}[model]
    assert np.all(np.isfinite(gd)) and np.any(gd != 0.0)
    check(gd, gh, f"model {model} gradient", scale=np.maximum(np.abs(gh), 1e-3 * np.abs(gh).max()))
    check(r[f"fx_{model}_dev"], r[f"fx_{model}_host"], f"model {model} value")


@gpu
def test_tape_arena_and_stacks():
    """After the nested recovery the device arena's use is back to its mark
    (the nodes leak nothing; inside the block it was above it), and the stacks
    are empty after everything."""
    r = tape()
    before, inside, after = r["arena"]
    assert inside > before and after == before
    assert list(r["stack"]) == [0.0, 0.0]


@functools.lru_cache(maxsize=None)
def errors():
    return {k: tuple(v) for k, *v in (line.split("|") for line in _run("errors\n").strip().splitlines())}


MISMATCH = {
    "subtract_vv": ("subtract", "4 x 1", "3 x 1"), "subtract_vd": ("subtract", "4 x 1", "3 x 1"),
    "subtract_dv": ("subtract", "3 x 1", "4 x 1"), "elt_multiply_vv": ("elt_multiply", "3 x 1", "4 x 1"),
    "elt_multiply_vd": ("elt_multiply", "3 x 1", "4 x 1"), "elt_multiply_dv": ("elt_multiply", "4 x 1", "3 x 1"),
    "elt_divide_vv": ("elt_divide", "4 x 1", "3 x 1"), "elt_divide_vd": ("elt_divide", "4 x 1", "3 x 1"),
    "elt_divide_dv": ("elt_divide", "3 x 1", "4 x 1"), "add_vd": ("add", "4 x 1", "3 x 1"),
    "add_dv": ("add", "3 x 1", "4 x 1"), "subtract_reshaped": ("subtract", "2 x 3", "3 x 2"),
}


@gpu
def test_cpp_errors_and_empty():
    """A shape mismatch throws std::invalid_argument that starts with the
    function's name and states both shapes; matching matrices pass; a
    size-zero operand gives an empty matrix and the tape still sweeps."""
    e = errors()
    for case, (fn, sa, sb) in MISMATCH.items():
        kind, msg = e[case]
        assert kind == "invalid_argument" and msg.startswith(fn + ": ") and sa in msg and sb in msg, (case, e[case])
        assert msg.index(sa) < msg.rindex(sb)
    assert e["ok_matrix"] == ("value", "2x3:6")
    kind, v = e["empty"]
    parts = v.split()
    assert kind == "value" and parts[:10] == ["0x1:0"] * 10, e["empty"]
    assert float(parts[10]) == 8.0 and float(parts[11]) == 4.0  # d/dx4 sum x^2 at 4, d/dc c^2 at 2
    assert e["stack"] == ("0", "0")
