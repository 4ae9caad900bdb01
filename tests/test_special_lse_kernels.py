"""lgamma / digamma / trigamma (k_unary, k_unary_rev) and log_sum_exp at their
edges, through the C entries, against references that are not the same
algorithm (tests/_special.py: 50-digit mpmath; longdouble for log_sum_exp).

Special functions: a fixed grid of about 2,900 points (tiny arguments, the
digamma root, the trigamma switch at 1e-4, both sides of the integers where
the recurrence count changes, negative arguments, half-integers, large
negative arguments for trigamma) plus exact rows (poles, +-inf, NaN,
overflow) whose expected results are a table written from the definitions.

Bounds, all derived or the project's own (test_gpu_kernels.test_special's
1e-13), put on a cancellation-safe scale -- none is measured:
  lgamma   x > 0: 1e-13 relative, or 1e-13 absolute on [0.5, 3];
           x < 0: 1e-13 (|lgamma(1 - x)| + |log|sin(pi x) / pi|| + 1).
  digamma  x > 0: 1e-13 relative; within 1e-2 of the root 1e-13 absolute
           and 1e-10 relative (boost's split root keeps it relatively
           accurate there: the port's worst is printed by the yardstick);
           x < 0: 1e-13 (|psi(1 - x)| + |pi cot(pi x)|).
  trigamma x > 0: 1e-13 relative against the 50-digit restatement of the
           algorithm (the kernel is that algorithm, to rounding) and 2e-8
           against the function (the algorithm drops pi^2/6 just below
           x = 1e-4: 1.64e-8 relative there);
           x < 0: 4 ((4 + 2 |pi r cot(pi r)|) 2^-53 (pi / sin(pi x))^2 + 1e-13
           psi_1(1 - x)) with r = x - round(x), plus 2e-8 psi_1(1 - x)
           against the function.
The no-GPU yardsticks run float64 ports of the device code and the CPU oracle
over the same points under the same bounds and require the ports to use at
most a quarter of each bound; they print the worst ratios.  They also show
that each bound tells a wrong kernel from a right one: the ports with root3
dropped, the series started at 4, `<` at the switch and the unreduced
reflection each miss it.

Adjoints accumulate: expected is pre + ya f'(x) in float64 with the bound
|ya| tol(f') + 2^-52 |pre + g| (the device's sum and the test's own, one
rounding each).  Every element is compared, so a pole or NaN at index i that
leaked into a neighbour would show there.

What the grid turned up, and what became of it:
  trigamma, large negative x: the reference forms sin(-pi x) unreduced (10.877
    for pi^2 at x = -1e15 - 0.5).  The kernel and prim/special.hpp now reduce
    the argument from x = -32 down; above -32 they keep the reference's
    expression, because the parity goldens are the reference's own roundings
    (up to 1.09e-13 from the function, at x = -6.0146: a kernel reduced
    everywhere misses test_special's 1e-13 there).  So the rows of (-64, 0) are
    held to the bound with |pi x|, the large negative rows to |pi r|.
  digamma, x <= -1: the reference takes the remainder of the rounded 1 - x;
    at x = -63.9459 that alone is 1.09 times the bound above.  The kernel and
    prim/special.hpp now take it from x (exact) and use 0.027 of the bound.
    The oracle keeps the reference's line and is held to the bound plus that
    error, |1 - x| 2^-53 pi^2 / sin^2(pi x).
  log_sum_exp: a NaN with nothing above -inf beside it (alone at n = 1) gave
    -inf, since fmax skips it and the sum is not used then; it now gives NaN.
  lgamma at x < 0 (ROCm's libm): 3.2e-3 of the bound at worst; nothing to fix.

log_sum_exp: value within gamma(n + 22) (1 + |max| + |lse - max|)
(test_tangent_kernels.test_lse_tangent_forward's bound), gradient within 1e-12
relative or 1e-15 absolute (test_gpu_kernels.test_log_sum_exp's), plus
2^-52 |pre + g| where it lands on a preload.
"""
import math

import numpy as np
import pytest

import _special as S
from _util import oracle

gpu = pytest.mark.gpu

BLOCK = 256
BIG = 8192 * BLOCK + 257      # past the 8192-block cap of k_unary / k_unary_rev / k_lse_rev: a second trip
RED2 = 1024 * BLOCK + 1       # past the RED_BLOCKS cap of k_max_part / k_sumexp_part
TAIL = 64
ULP = 2.0 ** -52


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


def names(f):
    return ("algorithm", "function") if f == "trigamma" else ("function",)


# ------------------------------------------------------------ 1. references and yardsticks (no GPU)
def test_restatement_against_truth():
    """The 50-digit restatement of the trigamma algorithm against the function:
    at most 1.65e-8 relative over the positive grid, the worst at and just below the
    switch (pi^2/6 x^2 at x = 1e-4 is 1.645e-8), about 6e-9 at z = 5; and the
    recurrences that stand in for mpmath below 1e-4 agree with mpmath's own
    psi where it answers quickly."""
    ref = S.reference()
    pos = (ref["x"] > 0) & np.isfinite(ref["tg"]) & (ref["tg_spec"] > 1e-300)
    rel = np.abs(ref["tg_spec"][pos] - ref["tg"][pos]) / ref["tg"][pos]
    i = int(np.argmax(rel))
    x = ref["x"][pos]
    print(f"trigamma algorithm vs function: worst relative {rel[i]:.4e} at x = {x[i]!r}")
    assert rel[i] <= 1.65e-8 and 0.99e-4 <= x[i] <= S.SWITCH
    at5 = rel[(x >= 4.0) & (x <= 6.0)].max()
    print(f"trigamma algorithm vs function on [4, 6]: worst relative {at5:.4e}")
    assert 1e-9 <= at5 <= 1e-8
    mp = S._mp()
    for xv in (9.5e-5, 3e-5):
        t = S._truth_point(mp, xv)
        assert abs(t[1] - mp.psi(0, mp.mpf(xv))) <= mp.mpf(10) ** -40 * abs(t[1])
        assert abs(t[2] - mp.psi(1, mp.mpf(xv))) <= mp.mpf(10) ** -40 * abs(t[2])
        assert abs(t[0] - mp.loggamma(mp.mpf(xv))) <= mp.mpf(10) ** -40 * abs(t[0])


@pytest.mark.parametrize("f", ["digamma", "trigamma"])
def test_port_yardstick(f):
    """No GPU: the float64 port of the device code uses at most a quarter of
    every 1e-13 bound asserted on the device (digamma everywhere, trigamma
    against the algorithm at x > 0), and meets the derived ones: trigamma's
    reflection bound at x < 0, which counts its roundings, and the 2e-8 against
    the function, of which the algorithm's own truncation takes 1.645e-8."""
    x, pairs, stratum = S.points(f)
    with np.errstate(all="ignore"):
        got = np.array([(S.port_digamma if f == "digamma" else S.port_trigamma)(float(v)) for v in x])
    for (want, tol), name in zip(pairs, names(f)):
        derived = (x < 0) if (f, name) == ("trigamma", "algorithm") else np.full(x.size, name == "function"
                                                                                  and f == "trigamma")
        for sel, limit, kind in ((~derived, 0.25, "1e-13 bounds"), (derived, 1.0, "derived bounds")):
            if not sel.any():
                continue
            r, i = S.ratio(got[sel], want[sel], tol[sel])
            print(f"port {f} vs {name}, {kind}: worst |diff| / bound = {r:.3e} at x = {x[sel][i]!r} "
                  f"({stratum[sel][i]})")
            assert r <= limit, (f, name, kind, r, x[sel][i])


def test_bounds_tell_wrong_from_right():
    """No GPU: the ports with one line wrong miss the bounds, where expected."""
    x, (dg,), _ = S.points("digamma")
    got = np.array([S.port_digamma(float(v), drop_root3=True) for v in x])
    fin = np.isfinite(dg[0])
    bad = np.abs(got[fin] - dg[0][fin]) > dg[1][fin]
    assert bad.any() and np.all(np.abs(x[fin][bad] - S.DIGAMMA_ROOT) <= 1e-2), "root3 dropped"
    x, (spec, truth), stratum = S.points("trigamma")
    fin = np.isfinite(spec[0]) & (spec[1] > 0)

    def misses(**kw):
        with np.errstate(all="ignore"):
            g = np.array([S.port_trigamma(float(v), **kw) for v in x])
            return fin & (np.abs(g - spec[0]) > spec[1]), fin & (np.abs(g - truth[0]) > truth[1])

    a, t = misses(large=4.0)
    assert a.any() and t.any(), "series started at z = 4"
    a, t = misses(strict_switch=True)
    assert list(x[a]) == [S.SWITCH], "`<` at the switch shows at x = 1e-4 alone"
    a, t = misses(reduce=False)
    assert a.any() and t.any() and np.all(stratum[t] == "large negative"), "unreduced reflection"
    k = int(np.where(x == -1e15 - 0.5)[0][0])
    print(f"trigamma(-1e15 - 0.5): unreduced {S.port_trigamma(x[k], reduce=False)!r}, reduced "
          f"{S.port_trigamma(x[k])!r}, function {truth[0][k]!r}")


@pytest.mark.parametrize("f", S.FUNCS)
def test_oracle_over_grid(f):
    """No GPU: the CPU restatement of the reference under the device's bounds.
    Its trigamma keeps the reference's own reflection, sin(-pi x) unreduced,
    so the large negative rows are the device's alone; what the oracle returns
    there is printed."""
    o = oracle()
    fn = getattr(o, "oracle_" + f)
    x, pairs, stratum = S.points(f, reference_algorithm=True)
    got = np.array([fn(float(v)) for v in x])
    keep = stratum != "large negative"
    for (want, tol), name in zip(pairs, names(f)):
        r, i = S.ratio(got[keep], want[keep], tol[keep])
        print(f"oracle {f} vs {name}: worst |diff| / bound = {r:.3e} at x = {x[keep][i]!r} ({stratum[keep][i]})")
        assert r <= 1.0, (f, name, r, x[keep][i])
    if f == "trigamma":
        k = int(np.where(x == -1e15 - 0.5)[0][0])
        print(f"oracle trigamma(-1e15 - 0.5) = {got[k]!r} (function: {pairs[1][0][k]!r})")


# ------------------------------------------------------------ 2. special functions on the device
def tiled(a, n):
    return np.resize(a, n)


def run_forward(ctx, f, x):
    n = len(x)
    buf = S.sentinel(n + TAIL, seed=3)
    dy = ctx.put(buf)
    ctx.call(f"smg_{f}_fwd", ctx.put(x), n, dy)
    out = ctx.get(dy, n + TAIL)
    assert S.same_bits(out[n:], buf[n:]), "wrote past n"
    return out[:n]


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, "grid", BIG])
@pytest.mark.parametrize("f", S.FUNCS)
def test_forward(ctx, f, n):
    """The grid, tiled to n, through smg_<f>_fwd into a sentinel-tailed buffer:
    every element under its point's bound, the tail untouched.  "grid" is every
    point once (about 2,900: 12 blocks); n = BIG takes the grid-stride loop
    into its second trip."""
    px, pairs, stratum = S.points(f)
    n = len(px) if n == "grid" else n
    x = tiled(px, n)
    got = run_forward(ctx, f, x)
    for (want, tol), name in zip(pairs, names(f)):
        r, i = S.ratio(got, tiled(want, n), tiled(tol, n))
        print(f"smg_{f}_fwd n={n} vs {name}: worst |diff| / bound = {r:.3e} at x = {x[i]!r} "
              f"({stratum[i % len(px)]})")
        assert r <= 1.0, (f, n, name, r, x[i], got[i])


def adjoint_case(f, n):
    """x, ya, preload, and per reference (expected, bound) for smg_<f>_rev."""
    px, pairs, stratum = S.points("digamma" if f == "lgamma" else "trigamma")
    n = len(px) if n == "grid" else n
    i = np.arange(n)
    x = tiled(px, n)
    ya = ((i % 7) - 3.0) * 0.375                      # signs mixed, a zero every seventh
    pre = (0.5 + 0.125 * (i % 5)) * np.where(i % 3 == 0, -1.0, 1.0)
    out = []
    with np.errstate(all="ignore"):
        for want, tol in pairs:
            tot = pre + ya * tiled(want, n)
            bound = np.abs(ya) * tiled(tol, n) + ULP * np.abs(tot)
            out.append((tot, np.where(np.isfinite(tot), bound, 0.0)))
    return x, ya, pre, out, stratum, len(px)


@gpu
@pytest.mark.parametrize("n", [257, "grid", BIG])
@pytest.mark.parametrize("f", ["lgamma", "digamma"])
def test_adjoint_accumulates(ctx, f, n):
    """smg_<f>_rev with a varied ya onto a nonzero preload: pre + ya f'(x)
    element by element (poles and NaN included: they stay where they are),
    the tail beyond n untouched."""
    x, ya, pre, refs, stratum, m = adjoint_case(f, n)
    n = len(x)
    buf = np.concatenate([pre, S.sentinel(TAIL, seed=5)])
    dxa = ctx.put(buf)
    ctx.call(f"smg_{f}_rev", ctx.put(x), n, ctx.put(ya), dxa)
    out = ctx.get(dxa, n + TAIL)
    assert S.same_bits(out[n:], buf[n:]), "wrote past n"
    for (tot, bound), name in zip(refs, names("trigamma" if f == "digamma" else "digamma")):
        r, i = S.ratio(out[:n], tot, bound)
        print(f"smg_{f}_rev n={n} vs {name}: worst |diff| / bound = {r:.3e} at x = {x[i]!r} ({stratum[i % m]})")
        assert r <= 1.0, (f, n, name, r, x[i], out[i], tot[i])


@gpu
@pytest.mark.parametrize("entry", ["smg_lgamma_rev", "smg_digamma_rev", "smg_lgamma_fwd", "smg_digamma_fwd",
                                   "smg_trigamma_fwd"])
def test_empty_leaves_buffer(ctx, entry):
    buf = S.sentinel(TAIL, seed=9)
    d = ctx.put(buf)
    x = ctx.put(np.full(TAIL, 2.5))
    if entry.endswith("_rev"):
        ctx.call(entry, x, 0, ctx.put(np.ones(TAIL)), d)
    else:
        ctx.call(entry, x, 0, d)
    assert S.same_bits(ctx.get(d, TAIL), buf)


# ------------------------------------------------------------ 3. log_sum_exp on the device
LSE_SIZES = [1, 2, 255, 256, 257, 1024 * BLOCK, RED2]
ADJ = -0.75


def lse_fwd(ctx, x, dx=None):
    """smg_log_sum_exp_fwd into a NaN-prefilled, sentinel-tailed output."""
    buf = np.concatenate([[np.nan], S.sentinel(7, seed=1)])
    dout = ctx.put(buf)
    ctx.call("smg_log_sum_exp_fwd", ctx.put(x) if dx is None else dx, len(x), dout)
    out = ctx.get(dout, 8)
    assert S.same_bits(out[1:], buf[1:])
    return out[0]


@gpu
@pytest.mark.parametrize("n", LSE_SIZES)
@pytest.mark.parametrize("kind", S.LSE_KINDS)
def test_lse_forward(ctx, kind, n):
    x = S.lse_case(kind, n)
    lse, _ = S.lse_ref(x)
    got = lse_fwd(ctx, x)
    bound = S.lse_value_bound(n, x, lse)
    print(f"smg_log_sum_exp_fwd {kind} n={n}: |diff| / bound = {abs(got - float(lse)) / bound:.3e}")
    assert abs(S.LD(got) - lse) <= bound, (got, float(lse))
    if n == 1:
        assert S.same_bits(got, x[0])
    if kind == "spike":  # every other term underflows: the sum is 1, its log 0
        assert got == x.max()


@gpu
@pytest.mark.parametrize("n", LSE_SIZES)
def test_lse_forward_nonfinite(ctx, n):
    """All -inf -> -inf; one +inf -> +inf; one NaN among finite entries ->
    NaN wherever it sits (fmax skips a NaN, so it arrives through the sum)."""
    assert lse_fwd(ctx, np.full(n, -np.inf)) == -np.inf
    x = np.full(n, -np.inf)
    x[n // 2] = np.nan  # a NaN with nothing finite beside it (alone, at n = 1): the reference's maxCoeff is NaN
    assert math.isnan(lse_fwd(ctx, x))
    base = S.lse_case("uniform", n)
    for k in sorted({0, n - 1, n // 2, 256 if n > 256 else 0}):
        x = base.copy()
        x[k] = np.inf
        assert lse_fwd(ctx, x) == np.inf, k
        x[k] = np.nan
        assert math.isnan(lse_fwd(ctx, x)), k


def lse_rev_check(ctx, kind, n):
    x = S.lse_case(kind, n)
    lse, p = S.lse_ref(x)
    i = np.arange(n)
    pre = (0.5 + 0.125 * (i % 5)) * np.where(i % 3 == 0, -1.0, 1.0)
    buf = np.concatenate([pre, S.sentinel(TAIL, seed=11)])
    dxa = ctx.put(buf)
    ctx.call("smg_log_sum_exp_rev", ctx.put(x), n, float(lse), ADJ, dxa)
    out = ctx.get(dxa, n + TAIL)
    assert S.same_bits(out[n:], buf[n:]), "wrote past n"
    g = (S.LD(ADJ) * p).astype(np.float64)
    tot = pre + g
    bound = np.maximum(1e-12 * np.abs(g), 1e-15) + ULP * np.abs(tot)
    r, k = S.ratio(out[:n], tot, bound)
    print(f"smg_log_sum_exp_rev {kind} n={n}: worst |diff| / bound = {r:.3e} at {k}")
    assert r <= 1.0, (kind, n, r, k, out[k], tot[k])
    if n == 1:
        assert out[0] == pre[0] + ADJ
    if kind == "neginf":
        assert S.same_bits(out[:n][np.isneginf(x)], pre[np.isneginf(x)])
    if kind == "spike":
        k = int(np.argmax(x))
        assert out[k] == pre[k] + ADJ
        rest = np.delete(out[:n] - pre, k)
        assert np.all(np.abs(rest) <= 1e-300)
    # sum p = 1.  out - pre is exact (|g| <= 0.75 <= 2 |pre|... where not, one
    # rounding of 2^-53 |out|); the passed lse is the reference rounded to
    # float64, (|lse| + 28) 2^-53 <= 50 2^-53 here, exp and the product 3 more:
    # the whole under 4 n 2^-53 from n = 255 on.  Below that the bound is
    # smaller than the rounding of lse itself; n = 1 is exact (above).
    if kind in ("uniform", "equal", "neginf") and n >= 255:
        s = math.fsum(out[:n] - pre) / ADJ
        print(f"smg_log_sum_exp_rev {kind} n={n}: |sum(grad) / adj - 1| / (4 n 2^-53) = "
              f"{abs(s - 1.0) / (4 * n * S.U):.3e}")
        assert abs(s - 1.0) <= 4 * n * S.U, (kind, n, s)


@gpu
@pytest.mark.parametrize("n", LSE_SIZES)
@pytest.mark.parametrize("kind", S.LSE_KINDS)
def test_lse_reverse(ctx, kind, n):
    """adj = -0.75 onto a nonzero preload, sentinel tail: pre + adj softmax(x)."""
    lse_rev_check(ctx, kind, n)


@gpu
def test_lse_reverse_second_trip(ctx):
    lse_rev_check(ctx, "uniform", BIG)


@gpu
def test_lse_deterministic(ctx):
    """The same bits from three runs at 262,145, and again after other
    reductions have left their partials in the workspace that log_sum_exp
    shares: smg_sum (one partial per block) and smg_normal_lpdf (four per
    block, large ones: they cover every slot log_sum_exp reads, so a partial it
    reads without having written it shows)."""
    n = RED2
    cases = [S.lse_case(k, n) for k in ("uniform", "minus700")]
    dxs = [ctx.put(x) for x in cases]
    first = [lse_fwd(ctx, x, dx) for x, dx in zip(cases, dxs)]
    for x, got in zip(cases, first):
        lse, _ = S.lse_ref(x)
        assert abs(S.LD(got) - lse) <= S.lse_value_bound(n, x, lse)
    for _ in range(2):
        for x, dx, want in zip(cases, dxs, first):
            assert S.same_bits(lse_fwd(ctx, x, dx), want)
    y = np.random.default_rng(S.SEED + 1).uniform(1e3, 2e3, n)
    dy = ctx.put(y)
    dsum = ctx.put(np.zeros(1))  # smg_sum accumulates: out += sum(x)
    ctx.call("smg_sum", dy, n, dsum)
    assert abs(ctx.get(dsum, 1)[0] - math.fsum(y)) <= S.gamma(n) * math.fsum(y)
    for x, dx, want in zip(cases, dxs, first):
        assert S.same_bits(lse_fwd(ctx, x, dx), want)
    out, gmu, gs = ctx.put(np.full(1, np.nan)), ctx.zeros(1), ctx.zeros(1)
    ctx.call("smg_normal_lpdf", dy, 1, ctx.zeros(1), 0, ctx.put(np.ones(1)), 0, n, 7, out, None, gmu, gs)
    assert ctx.get(gmu, 1)[0] > 1e8  # sum of y: partials of about 4e5 a block were left behind
    for x, dx, want in zip(cases, dxs, first):
        assert S.same_bits(lse_fwd(ctx, x, dx), want)
