"""References, grid and bounds for lgamma / digamma / trigamma and log_sum_exp
(tests/test_special_lse_kernels.py).  Nothing here touches the device.

Truth is mpmath at 50 digits: log|Gamma(x)|, psi(x), psi_1(x).  Below 1e-4 the
exact recurrences are used (psi(x) = psi(1 + x) - 1/x, psi_1(x) = psi_1(1 + x)
+ 1/x^2, log Gamma(x) = log Gamma(1 + x) - log x) and below zero the exact
reflections (with mpmath's sinpi / cospi, which reduce the argument exactly),
so that no mpmath call sees a tiny or a negative argument.

`trigamma_spec` is a 50-digit restatement of the algorithm the kernel
implements (stan/math/prim/scal/fun/trigamma.hpp): 1/x^2 for x <= 1e-4, the
recurrence up to z >= 5, the four-term series, the reflection with exact pi.
The algorithm's control flow sees z as the doubles fl(z + 1), so the
restatement steps z in float64 too (a point one ulp under an integer takes as
many steps as the kernel does) and evaluates every term of those z in mpmath.
That algorithm is up to 1.64e-8 relative from the function; the kernel has to
match the restatement to rounding and the function to 2e-8.

`port_digamma` / `port_trigamma` are line-by-line float64 ports of
dev_digamma (special_dev.h) and dev_trigamma (elementwise.hip); their only use
is the no-GPU yardstick, which shows that the bounds asserted on the device
are met by the algorithm itself with margin.
"""
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SEED = 20240611
DIGAMMA_ROOT = 1.4616321449683623
SWITCH = 0.0001          # dev_trigamma_pos: x <= small
TINY = 5e-324            # the smallest denormal: what a result below 2^-1022 is rounded to
NAN, INF = math.nan, math.inf


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


# ------------------------------------------------------------------ the grid
def _snap(x):
    """Move x so that its distance to the nearest integer is >= 2^-10."""
    r = x - np.round(x)
    near = np.abs(r) < 2.0 ** -10
    return np.where(near, np.round(x) + np.where(r < 0, -1.0, 1.0) * 2.0 ** -10, x)


@functools.lru_cache(maxsize=None)
def grid():
    """(x, stratum) of the finite, pole-free points: fixed and seeded."""
    rng = np.random.default_rng(SEED)
    parts = []

    def add(name, v):
        v = np.asarray(v, dtype=np.float64).ravel()
        parts.append((name, v))

    add("tiny", 10.0 ** rng.uniform(-300.0, -4.0, 300))
    add("(1e-4,1)", rng.uniform(1e-4, 1.0, 400))
    add("[1,2]", rng.uniform(1.0, 2.0, 300))
    add("(2,10)", rng.uniform(2.0, 10.0, 400))
    add("[10,1e15]", 10.0 ** rng.uniform(1.0, 15.0, 300))
    k = np.arange(2, 16)
    add("root", np.concatenate([[DIGAMMA_ROOT], DIGAMMA_ROOT + 10.0 ** -k, DIGAMMA_ROOT - 10.0 ** -k,
                                DIGAMMA_ROOT + rng.choice([-1.0, 1.0], 40) * 10.0 ** rng.uniform(-15.0, -2.0, 40)]))
    k = np.arange(1, 13)
    add("switch", np.concatenate([[SWITCH, np.nextafter(SWITCH, 0.0), np.nextafter(SWITCH, 1.0)],
                                  SWITCH * (1.0 + 10.0 ** -k), SWITCH * (1.0 - 10.0 ** -k)]))
    ints = np.arange(1.0, 6.0)
    side = [np.nextafter(ints, 0.0), np.nextafter(ints, 10.0)]
    for d in (1e-12, 1e-6, 1e-3):
        side += [ints * (1.0 - d), ints * (1.0 + d)]
    add("integers", np.concatenate(side + [[5.0, 10.0, np.nextafter(10.0, 0.0), np.nextafter(10.0, 11.0)]]))
    add("(-1,0)", _snap(rng.uniform(-1.0, 0.0, 300)))
    add("(-64,-1)", _snap(rng.uniform(-64.0, -1.0, 500)))
    add("half-integers", -0.5 - np.arange(64.0))
    x = np.concatenate([v for _, v in parts])
    stratum = np.concatenate([np.full(v.size, name) for name, v in parts])
    assert np.all(np.isfinite(x)) and not np.any((x <= 0) & (np.floor(x) == x))
    return x, stratum


def large_negative():
    """Trigamma only: -(10^k) - 0.5 and -(10^k) - 0.25, all representable."""
    k = np.array([3.0, 6.0, 9.0, 12.0, 15.0])
    x = np.concatenate([-(10.0 ** k) - 0.5, -(10.0 ** k) - 0.25])
    assert np.all(x - np.round(x) != 0.0)
    return x


# Exact rows: (x, lgamma, digamma, trigamma) written from the definitions.
# Poles: log|Gamma| -> +inf, psi has no limit (boost's errno_on_error policy:
# NaN), psi_1 -> +inf.  -inf: what the CPU restatement of the reference
# returns (glibc lgamma_r: +inf; boost's reflection forms inf - floor(inf):
# NaN; the reference's trigamma takes -inf for a pole since floor(x) == x:
# +inf).  5e-324: log Gamma = -log x, finite; -1/x and 1/x^2 overflow.
# 1e-160: -1/x is finite, 1/x^2 = 1e320 overflows.  1.7e308: x log x
# overflows, psi = log x, psi_1 = 1/x = 5.88e-309 is a denormal (checked to
# two units of 2^-1074).  None: finite, compared with truth under the bounds.
EXACT_ROWS = [
    (0.0, INF, NAN, INF),
    (-0.0, INF, NAN, INF),
    (-1.0, INF, NAN, INF),
    (-2.0, INF, NAN, INF),
    (-17.0, INF, NAN, INF),
    (INF, INF, INF, 0.0),
    (-INF, INF, NAN, INF),
    (NAN, NAN, NAN, NAN),
    (1.0, 0.0, None, None),
    (2.0, 0.0, None, None),
    (5e-324, None, -INF, INF),
    (1e-160, None, None, INF),
    (1.7e308, INF, None, None),
]


# ------------------------------------------------------------------ truth (mpmath)
def _truth_point(mp, x):
    """(log|Gamma|, psi, psi_1, lgamma scale, digamma scale) at a finite x that is no pole."""
    m = mp.mpf
    xm = m(x)
    if x > 0:
        if x < SWITCH:
            y = 1 + xm
            return mp.loggamma(y) - mp.log(xm), mp.psi(0, y) - 1 / xm, mp.psi(1, y) + 1 / (xm * xm), None, None
        return mp.loggamma(xm), mp.psi(0, xm), mp.psi(1, xm), None, None
    y = 1 - xm
    s, c = mp.sinpi(xm), mp.cospi(xm)
    lg1, cot = mp.loggamma(y), mp.pi * c / s
    lsin = mp.log(abs(s) / mp.pi)
    # Gamma(x) Gamma(1 - x) = pi / sin(pi x); psi(1 - x) - psi(x) = pi cot(pi x);
    # psi_1(x) + psi_1(1 - x) = pi^2 / sin^2(pi x)
    psi_y = mp.psi(0, y)
    return (-lsin - lg1, psi_y - cot, (mp.pi / s) ** 2 - mp.psi(1, y),
            abs(lg1) + abs(lsin) + 1, abs(psi_y) + abs(cot))


def _f(v):
    """An mpmath number rounded to float64 (overflow to inf, underflow to denormals)."""
    try:
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, float(v > 0) - 0.5)


def trigamma_spec_point(mp, x):
    """The reference's trigamma algorithm at 50 digits; z steps in float64."""
    m = mp.mpf
    if x <= 0:
        s = mp.pi / mp.sinpi(m(x))
        return s * s - trigamma_spec_point(mp, -x + 1.0)
    if x <= SWITCH:
        return 1 / (m(x) * m(x))
    z, value = x, m(0)
    while z < 5.0:
        value += 1 / (m(z) * m(z))
        z += 1.0
    y = 1 / (m(z) * m(z))
    b2, b4, b6, b8 = m(1) / 6, m(-1) / 30, m(1) / 42, m(-1) / 30
    return value + y / 2 + (1 + y * (b2 + y * (b4 + y * (b6 + y * b8)))) / m(z)


@functools.lru_cache(maxsize=None)
def reference():
    """Everything the tests compare with, over grid() + large_negative() + the
    finite entries of EXACT_ROWS, as float64 arrays (a 50-digit value rounded
    once: 2^-53 relative, against bounds of 1e-13 and more):
    x, stratum, lg, dg, tg (truth), tg_spec, and the tolerances tol_lg, tol_dg,
    tol_tg_spec, tol_tg_truth, and tol_dg_ref: tol_dg plus the reference
    digamma's own reflection error (for the oracle, which keeps it)."""
    mp = _mp()
    gx, gs = grid()
    ln = large_negative()
    ex = np.array([r[0] for r in EXACT_ROWS if math.isfinite(r[0]) and not (r[0] <= 0 and math.floor(r[0]) == r[0])])
    x = np.concatenate([gx, ln, ex])
    stratum = np.concatenate([gs, np.full(ln.size, "large negative"), np.full(ex.size, "exact rows")])
    n = x.size
    lg, dg, tg, spec = (np.empty(n) for _ in range(4))
    tol_lg, tol_dg, tol_spec, tol_truth, tol_dg_ref = (np.empty(n) for _ in range(5))
    for i, xi in enumerate(x):
        xi = float(xi)
        t = _truth_point(mp, xi)
        sp = trigamma_spec_point(mp, xi)
        lg[i], dg[i], tg[i], spec[i] = _f(t[0]), _f(t[1]), _f(t[2]), _f(sp)
        if xi > 0:
            tol_lg[i] = max(1e-13 * abs(lg[i]), 1e-13 if 0.5 <= xi <= 3.0 else 0.0)
            tol_dg[i] = 1e-13 * abs(dg[i])
            if abs(xi - DIGAMMA_ROOT) <= 1e-2:  # 1e-13 absolute, and 1e-10 relative (boost's split root)
                tol_dg[i] = min(max(tol_dg[i], 1e-13), 1e-10 * abs(dg[i]))
            tol_spec[i] = max(1e-13 * abs(spec[i]), 2 * TINY)
            tol_truth[i] = max(2e-8 * abs(tg[i]), 2 * TINY)
            tol_dg_ref[i] = tol_dg[i]
        else:
            tol_lg[i] = 1e-13 * _f(t[3])
            tol_dg[i] = 1e-13 * _f(t[4])
            # the reflection's argument: pi x as the reference forms it, pi (x -
            # round(x)) where the kernel reduces first (the large negative rows)
            xm = mp.mpf(xi)
            arg = xm - mp.nint(xm) if stratum[i] == "large negative" else xm
            s, c = mp.sinpi(xm), mp.cospi(xm)
            refl = (4 + 2 * abs(mp.pi * arg * c / s)) * U * (mp.pi / s) ** 2
            pos = trigamma_spec_point(mp, -xi + 1.0)
            tol_spec[i] = _f(4 * (refl + mp.mpf(1e-13) * pos))
            tol_truth[i] = _f(4 * (refl + mp.mpf(1e-13) * pos) + mp.mpf(2e-8) * pos)
            # the reference reduces 1 - x after rounding it: |1 - x| 2^-53 in the
            # argument of pi cot, whose slope is pi^2 / sin^2 (first order: the
            # grid keeps 2^-10 from a pole, the shift is under 2^-46)
            tol_dg_ref[i] = tol_dg[i] + (_f(U * abs(1 - xm) * (mp.pi / s) ** 2) if xi <= -1 else 0.0)
    for a in (lg, dg, tg, spec, tol_lg, tol_dg, tol_spec, tol_truth, tol_dg_ref):
        a.setflags(write=False)
    x.setflags(write=False)
    return dict(x=x, stratum=stratum, lg=lg, dg=dg, tg=tg, tg_spec=spec, tol_lg=tol_lg, tol_dg=tol_dg,
                tol_tg_spec=tol_spec, tol_tg_truth=tol_truth, tol_dg_ref=tol_dg_ref)


FUNCS = ("lgamma", "digamma", "trigamma")


@functools.lru_cache(maxsize=None)
def points(f, reference_algorithm=False):
    """(x, [(expected, tolerance), ...], stratum) for function f: every point of
    reference() that f is held to, then the non-finite exact rows with
    tolerance 0 (an exact match, NaN for NaN).  Read-only float64 arrays.
    reference_algorithm: digamma's tolerance with the reference's reflection
    error added."""
    ref = reference()
    keep = np.ones(ref["x"].size, dtype=bool)
    if f != "trigamma":
        keep &= ref["stratum"] != "large negative"
    col = FUNCS.index(f) + 1
    rows = [r for r in EXACT_ROWS if r[col] is not None]
    rx, rv = np.array([r[0] for r in rows]), np.array([r[col] for r in rows])
    # a row given exactly replaces that point's comparison with truth
    for xv in rx[np.isfinite(rx)]:
        keep &= ~((ref["x"] == xv) & (ref["stratum"] == "exact rows"))
    x = np.concatenate([ref["x"][keep], rx])
    zero = np.zeros(rx.size)
    if f == "lgamma":
        pairs = [(ref["lg"][keep], ref["tol_lg"][keep])]
    elif f == "digamma":
        pairs = [(ref["dg"][keep], ref["tol_dg_ref" if reference_algorithm else "tol_dg"][keep])]
    else:
        pairs = [(ref["tg_spec"][keep], ref["tol_tg_spec"][keep]), (ref["tg"][keep], ref["tol_tg_truth"][keep])]
    out = []
    for want, tol in pairs:
        w, t = np.concatenate([want, rv]), np.concatenate([tol, zero])
        w.setflags(write=False)
        t.setflags(write=False)
        out.append((w, t))
    x.setflags(write=False)
    return x, out, np.concatenate([ref["stratum"][keep], np.full(rx.size, "exact rows")])


def ratio(got, want, tol):
    """max |got - want| / tol over the finite expectations, after asserting that
    every non-finite expectation (and every zero tolerance) is met exactly.
    -> (worst ratio, its index)."""
    got, want, tol = (np.asarray(v, dtype=np.float64) for v in (got, want, tol))
    assert got.shape == want.shape == tol.shape
    exact = ~np.isfinite(want) | (tol == 0.0)
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    assert np.all(same[exact]), ("exact rows", np.where(exact & ~same)[0][:8], got[exact & ~same][:8],
                                 want[exact & ~same][:8])
    rest = ~exact
    assert np.all(np.isfinite(got[rest])), ("non-finite result", np.where(rest & ~np.isfinite(got))[0][:8])
    r = np.zeros(got.shape)
    r[rest] = np.abs(got[rest] - want[rest]) / tol[rest]
    i = int(np.argmax(r)) if r.size else 0
    return (float(r[i]) if r.size else 0.0), i


# ------------------------------------------------------------------ float64 ports of the device code
def _c_round(x):
    return math.copysign(math.floor(abs(x) + 0.5), x)  # C round(): halves away from zero


def _div(a, b):
    """a / b as IEEE division: no exception at b == 0 or on overflow."""
    return float(np.divide(np.float64(a), np.float64(b)))


def _digamma_large(x):
    P = (0.083333333333333333333333333333333333333333333333333, -0.0083333333333333333333333333333333333333333333333333,
         0.003968253968253968253968253968253968253968253968254, -0.0041666666666666666666666666666666666666666666666667,
         0.0075757575757575757575757575757575757575757575757576, -0.021092796092796092796092796092796092796092796092796,
         0.083333333333333333333333333333333333333333333333333, -0.44325980392156862745098039215686274509803921568627)
    x -= 1
    result = math.log(x) if x != math.inf else math.inf
    result += _div(1, 2 * x)
    z = _div(1, float(np.float64(x) * np.float64(x)))
    p = P[7]
    for c in P[6::-1]:
        p = c + z * p
    return result - z * p


def _digamma_1_2(x, drop_root3=False):
    Y = float(np.float32(0.99558162689208984))
    root1 = 1569415565.0 / 1073741824.0
    root2 = (381566830.0 / 1073741824.0) / 1073741824.0
    root3 = 0.9016312093258695918615325266959189453125e-19
    g = x - root1
    g -= root2
    if not drop_root3:
        g -= root3
    t = x - 1
    p = 0.25479851061131551 + t * (-0.32555031186804491 + t * (-0.65031853770896507 + t * (
        -0.28919126444774784 + t * (-0.045251321448739056 + t * -0.0020713321167745952))))
    q = 1.0 + t * (2.0767117023730469 + t * (1.4606242909763515 + t * (0.43593529692665969 + t * (
        0.054151797245674225 + t * (0.0021284987017821144 + t * -0.55789841321675513e-6)))))
    return g * Y + g * (p / q)


def port_digamma(x, drop_root3=False, reference_reflection=False):
    """dev_digamma; reference_reflection: the remainder taken from the rounded
    1 - x, as boost does and the kernel did."""
    x = float(x)
    result = 0.0
    with np.errstate(all="ignore"):
        if x <= -1 and reference_reflection:
            x = 1 - x
            rem = x - math.floor(x) if math.isfinite(x) else math.nan
            if rem > 0.5:
                rem -= 1
            if rem == 0:
                return math.nan
            result = _div(math.pi, math.tan(math.pi * rem)) if rem == rem else math.nan
        elif x <= -1:
            r = x - _c_round(x) if math.isfinite(x) else math.nan
            if r == 0:
                return math.nan
            result = -_div(math.pi, math.tan(math.pi * r)) if r == r else math.nan
            x = 1 - x
        if x == 0:
            return math.nan
        if math.isnan(x):
            return x
        if x >= 10:
            result += _digamma_large(x)
        else:
            while x > 2:
                x -= 1
                result += 1 / x
            while x < 1:
                result -= _div(1, x)
                x += 1
            result += _digamma_1_2(x, drop_root3)
    return result


def _trigamma_pos(x, large=5.0, strict_switch=False):
    b2, b4, b6, b8 = 1.0 / 6.0, -1.0 / 30.0, 1.0 / 42.0, -1.0 / 30.0
    with np.errstate(all="ignore"):
        if (x < SWITCH) if strict_switch else (x <= SWITCH):
            return _div(1.0, float(np.float64(x) * np.float64(x)))
        z, value = x, 0.0
        while z < large:
            value += 1.0 / (z * z)
            z += 1.0
        y = _div(1.0, float(np.float64(z) * np.float64(z)))
        return value + (0.5 * y + _div(1.0 + y * (b2 + y * (b4 + y * (b6 + y * b8))), z))


def port_trigamma(x, reduce=True, large=5.0, strict_switch=False):
    """dev_trigamma; reduce=False is the reference's reflection, sin(-pi x),
    at every x <= 0 (the kernel keeps it above -32 only)."""
    x = float(x)
    if math.isnan(x):
        return x
    if x <= 0.0 and (x == -math.inf or math.floor(x) == x):
        return math.inf
    if x <= 0:
        arg = math.pi * (x - _c_round(x)) if reduce and not x > -32.0 else math.pi * -x
        s = math.pi / math.sin(arg)
        return -_trigamma_pos(-x + 1.0, large, strict_switch) + s * s
    return _trigamma_pos(x, large, strict_switch)


# ------------------------------------------------------------------ log_sum_exp
C_LSE = 22  # test_tangent_kernels.C_LSE: the roundings of one term of the sum


def gamma(k):
    return k * U / (1.0 - k * U)


def lse_ref(x):
    """(lse, softmax p) in longdouble for a finite-or--inf x with a finite maximum."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    m = x.max()
    s = np.exp(x - m).sum()
    lse = m + np.log(s)
    return lse, np.exp(x - lse)


def lse_value_bound(n, x, lse):
    m = float(np.max(x))
    return gamma(n + C_LSE) * (1.0 + abs(m) + abs(float(lse - LD(m))))


LSE_KINDS = ("uniform", "plus700", "minus700", "spike", "equal", "neginf")


@functools.lru_cache(maxsize=None)
def lse_case(kind, n):
    """A read-only input of n doubles."""
    rng = np.random.default_rng(SEED + 7 * n + LSE_KINDS.index(kind))
    x = rng.uniform(-8.0, 8.0, n)
    if kind == "plus700":
        x += 700.0
    elif kind == "minus700":
        x -= 700.0
    elif kind == "spike":      # one entry 800 above the rest: every other exp underflows to 0
        x[(5 * n) // 7] += 800.0
    elif kind == "equal":
        x[:] = 3.25
    elif kind == "neginf":     # -inf scattered among finite entries; the first stays finite
        x[1::3] = -np.inf
    x.setflags(write=False)
    return x


def sentinel(size, seed=0):
    """A finite, position-dependent pattern no kernel produces by accident."""
    return 1.0e3 + 0.25 * ((np.arange(size, dtype=np.float64) * 7 + seed) % 4093)


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in (a, b))
    return np.array_equal(a, b)
