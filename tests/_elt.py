"""References, inputs and ctypes callers of the element-wise device maps
(math_amd/csrc/elt.hip, rev/fun/elt_ops.hpp; tests/test_elt_ops.py).

`unary_ref` and `binary_ref` are float64 numpy restatements of the kernels'
formulas; `unary_mp` and `binary_mp` are the same outputs in 60-digit mpmath
(in forms that need no more digits than that in the tails: log1p(exp(.)), not
log(1 + exp(.))).  With e = exp(-|x|), t = exp(-2|x|):

    inv_logit     = x >= 0 ? 1/(1+e) : e/(1+e)      inv_logit'     = e/(1+e)^2
    log1p_exp     = max(x, 0) + log1p(e)            log1p_exp'     = inv_logit(x)
    log_inv_logit = min(x, 0) - log1p(e)            log_inv_logit' = inv_logit(-x)
    tanh                                            tanh'          = 4t/(1+t)^2
    exp' = y, log' = 1/x, sqrt' = 0.5/y, square' = 2x, inv' = -y^2
    add: (c', c');  subtract: (c', -c');  elt_multiply: (c' b, c' a);
    elt_divide: (c'/b, -(c'/b)(a/b))

Comparisons (`worst`): each element on the scale of its own magnitude (or of a
given scale: the sum of the absolute values of an accumulated adjoint's terms,
of a reduced sum's terms).  Where the reference is NaN or +-inf the result must
be of the same class and sign.  The results at +-745 (exp(-745),
inv_logit(-745), log1p_exp(-745), ...) are the smallest subnormal, the float64
nearest to 4.98e-324: there the bound asks for that very number.
"""
import functools
import math

import numpy as np

import gen

UNARY = ("exp", "log", "sqrt", "square", "inv", "inv_logit", "log_inv_logit", "log1p_exp", "tanh")  # smg_elt_unary
BINARY = ("add", "subtract", "elt_multiply", "elt_divide")  # smg_elt_binary
POSITIVE = ("log", "sqrt", "inv")  # the unary functions whose grids are positive
SMG_OK, SMG_ERR_ARG = 0, 16


# ------------------------------------------------------------ references
def _inv_logit(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def unary_ref(name, x):
    """(f(x), f'(x)), float64 arrays."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if name == "exp":
            y = np.exp(x)
            return y, y.copy()
        if name == "log":
            return np.log(x), 1.0 / x
        if name == "sqrt":
            y = np.sqrt(x)
            return y, 0.5 / y
        if name == "square":
            return x * x, 2.0 * x
        if name == "inv":
            y = 1.0 / x
            return y, -(y * y)
        e = np.exp(-np.abs(x))
        if name == "inv_logit":
            d = 1.0 + e
            return _inv_logit(x), e / (d * d)
        if name == "log_inv_logit":
            return np.minimum(x, 0.0) - np.log1p(e), _inv_logit(-x)
        if name == "log1p_exp":
            return np.maximum(x, 0.0) + np.log1p(e), _inv_logit(x)
        assert name == "tanh", name
        t = np.exp(-2.0 * np.abs(x))
        d = 1.0 + t
        return np.tanh(x), 4.0 * t / (d * d)


def binary_ref(name, a, b, ca=1.0):
    """(c, c' dc/da, c' dc/db) element-wise, a and b broadcast."""
    a, b, ca = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, ca)))
    with np.errstate(all="ignore"):
        if name == "add":
            return a + b, ca.copy(), ca.copy()
        if name == "subtract":
            return a - b, ca.copy(), -ca
        if name == "elt_multiply":
            return a * b, ca * b, ca * a
        assert name == "elt_divide", name
        da = ca / b
        return a / b, da, -(da * (a / b))


def _to_float(v):
    try:
        return float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf


def unary_mp(name, x):
    """(f(x), f'(x)) in 60-digit mpmath, rounded to float64."""
    import mpmath as mp
    ys, ds = [], []
    with mp.workdps(60):
        one = mp.mpf(1)
        for xi in np.asarray(x, dtype=np.float64):
            v = mp.mpf(float(xi))
            il = lambda u: one / (one + mp.exp(-u))  # noqa: E731
            if name == "exp":
                y = d = mp.exp(v)
            elif name == "log":
                y, d = mp.log(v), one / v
            elif name == "sqrt":
                y = mp.sqrt(v)
                d = one / (2 * y)
            elif name == "square":
                y, d = v * v, 2 * v
            elif name == "inv":
                y, d = one / v, -one / (v * v)
            elif name == "inv_logit":
                y = il(v)
                d = mp.exp(-abs(v)) / (one + mp.exp(-abs(v))) ** 2
            elif name == "log_inv_logit":
                y, d = -mp.log1p(mp.exp(-v)), il(-v)
            elif name == "log1p_exp":
                y, d = mp.log1p(mp.exp(v)), il(v)
            else:
                y, d = mp.tanh(v), one / mp.cosh(v) ** 2
            ys.append(_to_float(y))
            ds.append(_to_float(d))
    return np.array(ys), np.array(ds)


def binary_mp(name, a, b, ca):
    """(c' dc/da, c' dc/db, their sums) in 60-digit mpmath, rounded to float64."""
    import mpmath as mp
    a, b, ca = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, ca)))
    das, dbs = [], []
    with mp.workdps(60):
        for ai, bi, ci in zip(a, b, ca):
            ai, bi, ci = mp.mpf(float(ai)), mp.mpf(float(bi)), mp.mpf(float(ci))
            if name == "add":
                da, db = ci, ci
            elif name == "subtract":
                da, db = ci, -ci
            elif name == "elt_multiply":
                da, db = ci * bi, ci * ai
            else:
                da, db = ci / bi, -ci * ai / (bi * bi)
            das.append(da)
            dbs.append(db)
        sa, sb = float(mp.fsum(das)), float(mp.fsum(dbs))
    return np.array([float(v) for v in das]), np.array([float(v) for v in dbs]), sa, sb


def worst(got, ref, scale=None):
    """max |got - ref| / scale over the entries (scale: |ref| unless given;
    0 where they are equal); an entry whose reference is NaN or +-inf must be
    of the same class and sign."""
    got, ref = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, ref))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref) if scale is None else np.broadcast_to(np.atleast_1d(np.asarray(scale, dtype=np.float64)), ref.shape)
    special = ~np.isfinite(ref)
    same = (np.isnan(ref) & np.isnan(got)) | (np.isinf(ref) & (got == ref))
    assert np.all(same[special]), ("class or sign", got[special & ~same][:4], ref[special & ~same][:4])
    fin = ~special
    assert np.all(np.isfinite(got[fin])), ("not finite", got[fin][~np.isfinite(got[fin])][:4])
    if not np.any(fin):
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got[fin] - ref[fin])
        r = np.where(err == 0.0, 0.0, err / scale[fin])
    return float(np.max(r))


# ------------------------------------------------------------ grids and inputs
def main_grid(name):
    """About 400 points in [-30, 30]; positive for log, sqrt and inv."""
    x = gen.unif(gen.SEED + 900, 400, -30.0, 30.0)
    return np.abs(x) + 1e-3 if name in POSITIVE else x


EXTREME = np.array([0.0, -0.0, 1e-300, -1e-300, 1e-8, -1e-8, 1.0, -1.0, 36.05, -36.05, 40.0, -40.0, 709.0, -709.0,
                    745.0, -745.0])


def extreme_grid(name):
    """0, -0.0, +-1e-300, +-1e-8, +-1, +-36.05, +-40, +-709, +-745; for log,
    sqrt and inv the positive ones with 1e300."""
    if name in POSITIVE:
        return np.concatenate([EXTREME[EXTREME > 0.0], [1e300]])
    return EXTREME.copy()


def device_extremes():
    """The extreme grid with 1e300 and NaN, +-inf: every unary kernel gets all of it."""
    return np.concatenate([EXTREME, [1e300, -1e300, np.nan, np.inf, -np.inf]])


@functools.lru_cache(maxsize=None)
def unary_inputs(name, n):
    """(x, yadj, xadj0): x in (-12, 12) (|x| + 0.05 for log, sqrt, inv), the
    incoming adjoint in (-2, 2), the adjoint already there in (-1, 1)."""
    x = gen.unif(gen.SEED + 910, n, -12.0, 12.0)
    if name in POSITIVE:
        x = np.abs(x) + 0.05
    out = (x, gen.unif(gen.SEED + 911, n, -2.0, 2.0), gen.unif(gen.SEED + 912, n, -1.0, 1.0))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def binary_inputs(n):
    """(a, b, cadj, aadj0, badj0): a in (-4, 4), |b| in (0.3, 3) of either sign."""
    a = gen.unif(gen.SEED + 920, n, -4.0, 4.0)
    b = gen.unif(gen.SEED + 921, n, 0.3, 3.0) * np.where(gen.u01(gen.SEED + 922, n) < 0.5, -1.0, 1.0)
    out = (a, b, gen.unif(gen.SEED + 923, n, -2.0, 2.0), gen.unif(gen.SEED + 924, n, -1.0, 1.0),
           gen.unif(gen.SEED + 925, n, -1.0, 1.0))
    for v in out:
        v.setflags(write=False)
    return out


A0, B0 = 1.7, -0.6  # the scalar operands


# ------------------------------------------------------------ the C entries
SENTINEL = -7.25
TAIL = 3  # sentinel doubles after each buffer


class Buf:
    """`a` on the device between sentinels: two doubles before it (it starts
    on a 16-byte boundary) or, misaligned, three (one double past one), and
    TAIL after it."""

    def __init__(self, ctx, a, mis=False):
        a = np.asarray(a, dtype=np.float64)
        self.ctx, self.n, self.pre = ctx, len(a), 3 if mis else 2
        self.base = ctx.put(np.concatenate([np.full(self.pre, SENTINEL), a, np.full(TAIL, SENTINEL)]))
        assert self.base % 16 == 0
        self.ptr = self.base + 8 * self.pre
        assert (self.ptr % 16 == 8) == bool(mis)

    def read(self, what="buffer"):
        g = self.ctx.get(self.base, self.pre + self.n + TAIL)
        assert np.all(g[:self.pre] == SENTINEL), (what, "wrote before it")
        assert np.all(g[self.pre + self.n:] == SENTINEL), (what, "wrote past it")
        return g[self.pre:self.pre + self.n]


def launch_shape(ctx):
    """{threads, max_blocks, width, red_threads, red_per_block, red_max_blocks,
    binary_rev_width} of the entries under the current smg_elt_set_width."""
    import ctypes
    s = (ctypes.c_int * 7)()
    assert ctx.lib.smg_elt_launch_shape(ctx.ptr, s) == SMG_OK
    return dict(zip(("threads", "max_blocks", "width", "red_threads", "red_per_block", "red_max_blocks",
                     "binary_rev_width"), list(s)))


def second_trip_size(shape):
    """The smallest n that puts a lane on its second grid-stride trip (with
    two elements per lane: a whole pair of it, and the odd last element)."""
    w = max(shape["width"], shape["binary_rev_width"])
    return shape["threads"] * shape["max_blocks"] * w + (3 if w == 2 else 1)


def unary_fwd(ctx, name, x, mis=(False, False)):
    bx, by = Buf(ctx, x, mis[0]), Buf(ctx, np.full(len(x), SENTINEL), mis[1])
    ctx.call("smg_elt_unary_fwd", UNARY.index(name), bx.ptr, len(x), by.ptr)
    return by.read(name + " y"), by


def unary_rev(ctx, name, x, y, yadj, xadj0, mis=(False,) * 4):
    bx, by, bya, bxa = (Buf(ctx, v, m) for v, m in zip((x, y, yadj, xadj0), mis))
    ctx.call("smg_elt_unary_rev", UNARY.index(name), bx.ptr, by.ptr, len(x), bya.ptr, bxa.ptr)
    return bxa.read(name + " xadj")


def _operand(ctx, v, mis):
    """(pointer or None, scalar value) of a vector or scalar operand."""
    if np.isscalar(v):
        return None, float(v)
    return Buf(ctx, v, mis).ptr, 0.0


def binary_fwd(ctx, name, a, b, n, mis=(False,) * 3):
    pa, a0 = _operand(ctx, a, mis[0])
    pb, b0 = _operand(ctx, b, mis[1])
    bc = Buf(ctx, np.full(n, SENTINEL), mis[2])
    ctx.call("smg_elt_binary_fwd", BINARY.index(name), pa, pb, a0, b0, n, bc.ptr)
    return bc.read(name + " c")


def binary_rev(ctx, name, a, b, n, cadj, aadj0=None, badj0=None, want_scalar=0, mis=(False,) * 5, alias=False,
               calls=1):
    """smg_elt_binary_rev -> (aadj, badj, red): aadj0 / badj0 None passes a
    NULL adjoint pointer (then None comes back); alias: b is a, badj is aadj;
    red starts as two sentinels; calls > 1 repeats the call on the same
    buffers."""
    pa, a0 = _operand(ctx, a, mis[0])
    pb, b0 = (pa, a0) if alias else _operand(ctx, b, mis[1])
    bc = Buf(ctx, cadj, mis[2])
    ba = None if aadj0 is None else Buf(ctx, aadj0, mis[3])
    bb = ba if alias else (None if badj0 is None else Buf(ctx, badj0, mis[4]))
    red = Buf(ctx, np.full(2, SENTINEL))
    for _ in range(calls):
        ctx.call("smg_elt_binary_rev", BINARY.index(name), pa, pb, a0, b0, n, bc.ptr, ba and ba.ptr, bb and bb.ptr,
                 want_scalar, red.ptr)
    return (None if ba is None else ba.read(name + " aadj"), None if bb is None else bb.read(name + " badj"),
            red.read(name + " red"))
