"""student_t_lpdf and cauchy_lpdf: the fused device reducers
smg_student_t_lpdf_fused / smg_cauchy_lpdf_fused through ctypes, and the
stan::math overloads through the tape (tests/cpp/test_heavy_tail_lpdf.cpp).

The reference of every device test is `_heavy_tail.st_ref` / `cauchy_ref`, a
float64 numpy restatement of the formulas with every sum by math.fsum.  The
references are checked against 60-digit mpmath without a GPU
(test_reference_against_mpmath).

Bounds.  Every output (logp, each reduced partial, each element of a vector
partial) is compared on the scale of the sum of its terms' absolute values
(tests/_heavy_tail.py lists the terms); y' and mu' are single terms, their
scale is |value|.

    yardstick (reference against mpmath):  asserted at 5e-14 of that scale;
        measured worst ratios, main grid (400 elements) / extreme grid
        (z in {0, 1e-8, 1, 1e6, +-1e150} x nu in {1e-3, 1, 4, 1e8}):
        Student-t (scipy gammaln, digamma): logp 1.2e-17 / 0,
            y' 3.9e-16 / 2.0e-16, nu' 1.6e-16 / 1.2e-16, sigma' 3.1e-16 / 1.7e-16,
            reduced sums <= 3.6e-17 / 0
        Cauchy: logp 0 / 0, y' 3.2e-16 / 2.0e-16, sigma' 2.5e-16 / 1.7e-16,
            reduced sums <= 1.7e-17 / 1.7e-16
    device against the reference:          1e-12 of that scale, every output
        (the project's bound for every fused reducer; it holds because the
        yardstick is under 5e-14)

The launch rule is k_normal_fused's: one 1024-thread block up to 4096
elements, then ceil(n / 4096) blocks up to 512; a lane reads one 8-byte
element per trip (the 16-byte form was measured and not kept: DESIGN.md).
4097 is the first two-block launch (the ticket), 2,097,153 the second trip
of the grid stride.
"""
import ctypes
import functools
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import gen
from _heavy_tail import (PARTIALS, cauchy_mp, cauchy_ref, extreme_grid, fused, got_of, inputs, st_mp, st_ref, with_mp,
                         yardstick_grid)
from _reducers import same_bits
from _util import ROOT, check_sums, prebuilt

gpu = pytest.mark.gpu

SMG_OK = 0
SMG_ERR_ARG = 16
KINDS = (0, 1)
NAME = {0: "student_t", 1: "cauchy"}
SCALARS = (0.7, 4.5, 0.2, 1.3)  # y, nu, mu, sigma as scalar operands


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


def ref_of(kind, ops, include=None, n=None):
    """The reference of `kind` over ops = (y, nu, mu, sigma); Cauchy ignores nu."""
    if kind == 0:
        return st_ref(*ops, include=15 if include is None else include, n=n)
    return cauchy_ref(ops[0], ops[2], ops[3], include=7 if include is None else include, n=n)


def entry_ops(kind, ops):
    return tuple(ops) if kind == 0 else (ops[0], ops[2], ops[3])


def form_ops(n, vec):
    """ops with operand i a vector of n (vec[i]) or the scalar SCALARS[i];
    y = mu + sigma t keeps its table where y is a vector."""
    y, nu, mu, sigma = inputs(n)
    return tuple(v if isvec else s for v, isvec, s in zip((y, nu, mu, sigma), vec, SCALARS))


@functools.lru_cache(maxsize=None)
def problem(kind, n, vec=(True,) * 4, include=None):
    ops = form_ops(n, vec)
    return ops, ref_of(kind, ops, include, n)


def check_dev(got, ref, what):
    check_sums(got, ref, what, b_sum=1e-12, b_rel=None)


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("grid", ["main", "extreme"])
@pytest.mark.parametrize("kind", KINDS)
def test_reference_against_mpmath(kind, grid):
    """No GPU: the float64 reference against 60-digit mpmath, every output
    within 5e-14 of the sum of its terms' absolute values."""
    ops = yardstick_grid() if grid == "main" else extreme_grid()
    ref = ref_of(kind, ops)
    mp = st_mp(*ops) if kind == 0 else cauchy_mp(ops[0], ops[2], ops[3])
    for k, (v, _) in ref.items():
        assert np.all(np.isfinite(v)), k
    check_sums({k: v[0] for k, v in ref.items()}, with_mp(ref, mp), f"ref vs mpmath {NAME[kind]} {grid}",
               b_sum=5e-14, b_rel=None)


# ------------------------------------------------------------ 2. the C entries
SIZES = [1, 63, 64, 65, 1023, 1025, 4096, 4097, 8193, 2097153]


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_entry_sizes(ctx, kind, n):
    """Every operand a vector, every partial asked for."""
    ops, ref = problem(kind, n)
    res, gs = fused(ctx, kind, entry_ops(kind, ops), n)
    check_dev(got_of(kind, res, gs, entry_ops(kind, ops)), ref, f"{NAME[kind]} n={n}")


FORMS = {0: list(itertools.product((True, False), repeat=4)),
         1: [(a, True, b, c) for a, b, c in itertools.product((True, False), repeat=3)]}


@gpu
@pytest.mark.parametrize("kind,vec", [(k, f) for k in KINDS for f in FORMS[k]])
def test_entry_forms(ctx, kind, vec):
    """n = 4097: all vector / scalar combinations of the operands (16 for
    Student-t, 8 for Cauchy), every partial asked for: a vector operand's is
    written, a scalar operand's is reduced into res."""
    ops, ref = problem(kind, 4097, vec)
    eo = entry_ops(kind, ops)
    res, gs = fused(ctx, kind, eo, 4097)
    check_dev(got_of(kind, res, gs, eo), ref, f"{NAME[kind]} form {vec}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_entry_partial_subsets(ctx, kind):
    """n = 4097, y and mu vectors, nu and sigma scalars: every subset of wanted
    partials.  A partial that is not asked for is not written (its reduced
    slot stays 0; `fused` checks the sentinels of the ones that are)."""
    vec = (True, False, True, False)
    ops, ref = problem(kind, 4097, vec)
    eo = entry_ops(kind, ops)
    for want in itertools.product((True, False), repeat=len(eo)):
        res, gs = fused(ctx, kind, eo, 4097, want=want)
        check_dev(got_of(kind, res, gs, eo, want), ref, f"{NAME[kind]} want {want}")


@gpu
@pytest.mark.parametrize("kind,include", [(0, i) for i in range(16)] + [(1, i) for i in range(8)])
def test_entry_include_masks(ctx, kind, include):
    """Every value of the mask (4 bits, Cauchy 3) at n = 4097 against the
    reference with the same terms dropped; all vectors and the common form."""
    for vec in ((True,) * 4, (True, False, True, False)):
        ops, ref = problem(kind, 4097, vec, include)
        eo = entry_ops(kind, ops)
        res, gs = fused(ctx, kind, eo, 4097, include=include)
        check_dev(got_of(kind, res, gs, eo), ref, f"{NAME[kind]} include {include} {vec}")
        if include == 0:
            assert res[0] == 0.0


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_entry_hoisting_is_not_a_different_function(ctx, kind):
    """A scalar nu and the constant vector of the same nu agree within the
    bound (both against the same reference), and so do a scalar sigma and its
    constant vector.  Equal bits are not asked for: the sums associate
    differently."""
    n = 4097
    y, nu, mu, sigma = inputs(n)
    cases = [("sigma", (y, nu, mu, SCALARS[3]), (y, nu, mu, np.full(n, SCALARS[3])))]
    if kind == 0:
        cases.append(("nu", (y, SCALARS[1], mu, sigma), (y, np.full(n, SCALARS[1]), mu, sigma)))
        cases.append(("nu, sigma", (y, SCALARS[1], mu, SCALARS[3]),
                      (y, np.full(n, SCALARS[1]), mu, np.full(n, SCALARS[3]))))
    for what, scalar_ops, vector_ops in cases:
        ref = ref_of(kind, scalar_ops, n=n)  # (the constant vector's reference is the same: it broadcasts)
        es, ev = entry_ops(kind, scalar_ops), entry_ops(kind, vector_ops)
        rs, gs = fused(ctx, kind, es, n)
        rv, gv = fused(ctx, kind, ev, n)
        got_s, got_v = got_of(kind, rs, gs, es), got_of(kind, rv, gv, ev)
        check_dev(got_s, ref, f"{NAME[kind]} scalar {what}")
        check_dev(got_v, ref, f"{NAME[kind]} constant vector {what}")
        # and against each other: logp, and the scalar's reduced partial against the vector's elements summed
        assert abs(got_s["logp"] - got_v["logp"]) <= 1e-12 * ref["logp"][1], what
        for k in got_s:
            if k.startswith("sum ") and k[4:] in got_v:
                assert abs(got_s[k] - math.fsum(got_v[k[4:]])) <= 1e-12 * ref[k][1], (what, k)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_entry_extremes(ctx, kind):
    """z in {0, 1e-8, 1, 1e6, +-1e150} x nu in {1e-3, 1, 4, 1e8} at sigma =
    1.5: every output finite and within the bound of the mpmath value, as
    vectors and with the reduced partials of a scalar sigma."""
    ops = extreme_grid(sigma=1.5)
    n = len(ops[0])
    ref = ref_of(kind, ops)
    mp = with_mp(ref, st_mp(*ops) if kind == 0 else cauchy_mp(ops[0], ops[2], ops[3]))
    for sigma in (ops[3], 1.5):
        eo = entry_ops(kind, (ops[0], ops[1], ops[2], sigma))
        res, gs = fused(ctx, kind, eo, n)
        assert np.all(np.isfinite(res))
        for k, v in gs.items():
            assert np.all(np.isfinite(v)), (k, v)
        check_dev(got_of(kind, res, gs, eo), mp, f"{NAME[kind]} extremes sigma {'vector' if sigma is ops[3] else 'scalar'}")


# (slot of (y, nu, mu, sigma), value, the flag its column must hold)
OFFENDERS = [(0, np.nan, 1), (1, 0.0, 1), (1, -1.0, 1), (1, np.nan, 1), (1, np.inf, 2), (2, np.inf, 1),
             (2, np.nan, 1), (3, 0.0, 1), (3, np.nan, 1), (3, np.inf, 2)]


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_entry_domain_flags(ctx, kind):
    """One bad element, at the first element, at the last and in the second
    block of an n = 8193 (three-block) call: its flag column holds its bit and
    the other flag columns stay 0; SMG_OK, and the context's status stays 0.
    A vector with an infinity and a non-positive element holds both bits.
    Scalar operands are flagged too."""
    n = 8193
    ops = inputs(n)
    for slot, v, bit in OFFENDERS:
        if kind == 1 and slot == 1:
            continue
        for at in (0, n - 1, 1024 + 5):
            bad = [o.copy() for o in ops]
            bad[slot][at] = v
            res, _ = fused(ctx, kind, entry_ops(kind, bad), n, want=(False,) * (4 - kind))
            flags = list(res[1:5])
            assert flags == [float(bit) if j == slot else 0.0 for j in range(4)], (slot, v, at, flags)
    both = [o.copy() for o in ops]
    both[3][5], both[3][n - 2] = np.inf, -1.0
    res, _ = fused(ctx, kind, entry_ops(kind, both), n, want=(False,) * (4 - kind))
    assert list(res[1:5]) == [0.0, 0.0, 0.0, 3.0]
    for slot, v, bit in OFFENDERS:
        if kind == 1 and slot == 1:
            continue
        sc = list(ops)
        sc[slot] = float(v)
        res, _ = fused(ctx, kind, entry_ops(kind, sc), n, want=(False,) * (4 - kind))
        assert list(res[1:5]) == [float(bit) if j == slot else 0.0 for j in range(4)], (slot, v, res[1:5])
    assert ctx.status() == 0


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_entry_two_calls_bitwise_equal(ctx, kind):
    n = 2097153
    ops = entry_ops(kind, inputs(n))
    a = fused(ctx, kind, ops, n)
    b = fused(ctx, kind, ops, n)
    assert same_bits(a[0], b[0])
    for k in a[1]:
        assert same_bits(a[1][k], b[1][k]), k


@gpu
def test_entry_argument_errors_and_empty(ctx):
    """A null context, n < 0 or a null res: SMG_ERR_ARG, nothing written, the
    status latch untouched; n = 0 writes nine zeros."""
    lib = ctx.lib
    n = 33
    y, nu, mu, sigma = (ctx.put(v) for v in inputs(n))
    res = ctx.put(np.full(9, np.nan))
    t, c = lib.smg_student_t_lpdf_fused, lib.smg_cauchy_lpdf_fused
    assert t(None, y, nu, mu, sigma, 0.0, 0.0, 0.0, 0.0, n, 15, res, None, None, None, None) == SMG_ERR_ARG
    assert t(ctx.ptr, y, nu, mu, sigma, 0.0, 0.0, 0.0, 0.0, -1, 15, res, None, None, None, None) == SMG_ERR_ARG
    assert t(ctx.ptr, y, nu, mu, sigma, 0.0, 0.0, 0.0, 0.0, n, 15, None, None, None, None, None) == SMG_ERR_ARG
    assert c(None, y, mu, sigma, 0.0, 0.0, 0.0, n, 7, res, None, None, None) == SMG_ERR_ARG
    assert c(ctx.ptr, y, mu, sigma, 0.0, 0.0, 0.0, -1, 7, res, None, None, None) == SMG_ERR_ARG
    assert c(ctx.ptr, y, mu, sigma, 0.0, 0.0, 0.0, n, 7, None, None, None, None) == SMG_ERR_ARG
    assert np.all(np.isnan(ctx.get(res, 9)))  # nothing was written
    assert ctx.status() == 0
    for kind in KINDS:
        for ops in ((y, nu, mu, sigma), (None,) * 4):  # vectors, and scalars (a scalar nu of 0: not evaluated)
            ctx.lib.smg_memcpy_h2d(ctx.ptr, res, np.full(9, np.nan).ctypes.data_as(ctypes.c_void_p), 72)
            ctx.sync()
            if kind == 0:
                ctx.call("smg_student_t_lpdf_fused", *ops, 0.0, 0.0, 0.0, 0.0, 0, 15, res, None, None, None, None)
            else:
                ctx.call("smg_cauchy_lpdf_fused", ops[0], ops[2], ops[3], 0.0, 0.0, 0.0, 0, 7, res, None, None, None)
            assert np.array_equal(ctx.get(res, 9), np.zeros(9)), kind
    assert ctx.status() == 0


@gpu
@pytest.mark.parametrize("vec", [(True,) * 4, (True, False, True, False)])
@pytest.mark.parametrize("kind", KINDS)
def test_entry_pinned_operands(ctx, kind, vec):
    """n = 4097 with every operand and output in smg_pinned_io memory (the host
    layer's zero-copy path) and once more in device memory: each within the
    bound, and the same bits."""
    ops, ref = problem(kind, 4097, vec)
    eo = entry_ops(kind, ops)
    dev = fused(ctx, kind, eo, 4097)
    pin = fused(ctx, kind, eo, 4097, pinned=True)
    check_dev(got_of(kind, *pin, eo), ref, f"{NAME[kind]} pinned {vec}")
    check_dev(got_of(kind, *dev, eo), ref, f"{NAME[kind]} device {vec}")
    assert same_bits(dev[0], pin[0])
    for k in dev[1]:
        assert same_bits(dev[1][k], pin[1][k]), k


# ------------------------------------------------------------ 3. through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_heavy_tail_lpdf")
TAPE_N = 1000
GP_N = 64


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@functools.lru_cache(maxsize=None)
def gp_inputs():
    """The latent GP: x (N) evenly spaced over (-3, 3) with a jitter, GP sigma
    1.1, length scale 0.6, eta uniform in (-1, 1), y = f + 0.5 t (t from the
    heavy-tailed table) at f = L eta; likelihood sigma 0.6, nu 3.5."""
    from _heavy_tail import T_TABLE
    N = GP_N
    x = np.linspace(-3.0, 3.0, N) + gen.unif(gen.SEED + 781, N, -0.02, 0.02)
    gs, gl = 1.1, 0.6
    eta = gen.unif(gen.SEED + 782, N, -1.0, 1.0)
    K = gs**2 * np.exp(-0.5 * (x[:, None] - x[None, :])**2 / gl**2) + 1e-6 * np.eye(N)
    f = np.linalg.cholesky(K) @ eta
    y = f + 0.5 * T_TABLE[(gen.u01(gen.SEED + 783, N) * len(T_TABLE)).astype(np.int64)]
    return x, gs, gl, eta, y, 0.6, 3.5


@functools.lru_cache(maxsize=None)
def tape():
    """One run of the binary's "tape" mode, shared by the tests below: {tag: values}."""
    ops = inputs(TAPE_N)
    x, gs, gl, eta, y, sigma, nu = gp_inputs()
    nums = np.concatenate(list(ops) + [SCALARS])
    gp = np.concatenate([x, [gs, gl], eta, y, [sigma, nu]])
    out = _run(f"tape {TAPE_N}\n" + " ".join(repr(float(v)) for v in nums) + f"\ngp {GP_N}\n"
               + " ".join(repr(float(v)) for v in gp) + "\n")
    res = {}
    for line in out.strip().splitlines():
        tag, _, vals = line.partition(" ")
        res[tag] = np.array(vals.split(), dtype=np.float64)
    return res


def masks(kind):
    k = 4 - kind
    return ["".join("v" if (m >> o) & 1 else "d" for o in range(k)) for m in range(1 << k)]


def tape_ref(kind, shape, mask, propto):
    """(ops, reference) of a tape case: include_summand<propto, ...> drops a
    term whose operands are all double."""
    vec = (True,) * 4 if shape == "vec" else (True, False, True, False)
    v = [c == "v" for c in mask]
    vy, vnu, vmu, vs = v if kind == 0 else (v[0], False, v[1], v[2])
    include = 15 if kind == 0 else 7
    if propto:
        include = (2 if vs else 0) | (4 if (vy or vnu or vmu or vs) else 0) | (8 if (kind == 0 and vnu) else 0)
    return problem(kind, TAPE_N, vec, include)


def check_tape_case(r, kind, shape, cont, path, mask, propto=False):
    tag = f"{'p' if propto else ''}_{kind}_{shape}_{cont}_{path}_{mask}"
    ops, ref = tape_ref(kind, shape, mask, propto)
    what = f"tape {NAME[kind]} {tag}"
    if "v" not in mask:
        assert ("grad" + tag) not in r
        if propto:
            assert r["fx" + tag][0] == 0.0
        else:
            check_dev({"logp": r["fx" + tag][0]}, ref, what)
        return
    got = {"logp": r["fx" + tag][0]}
    g, at = r["grad" + tag], 0
    names = PARTIALS if kind == 0 else ("y'", "mu'", "sigma'")
    for name, c, o in zip(names, mask, entry_ops(kind, ops)):
        if c != "v":
            continue
        if np.isscalar(o):
            got["sum " + name] = g[at]
            at += 1
        else:
            got[name] = g[at:at + TAPE_N]
            at += TAPE_N
    assert at == len(g), (tag, at, len(g))
    check_dev(got, ref, what)


@gpu
@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("cont", ["std", "eig"])
@pytest.mark.parametrize("kind", KINDS)
def test_tape_every_var_double_combination(kind, cont, path):
    """Value and gradient at n = 1000 for every var / double combination of the
    operands (15 with a var for Student-t, 7 for Cauchy, and the all-double
    value), as std::vector and as Eigen vectors, through the host loop and
    through the device, all vectors and with nu, sigma scalars: each within
    the bound of the reference."""
    r = tape()
    for shape in ("vec", "mix"):
        for mask in masks(kind):
            check_tape_case(r, kind, shape, cont, path, mask)


@gpu
@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_tape_propto(kind, path):
    """propto drops the terms whose operands are all double: the value against
    the reference with those terms dropped, the gradient unchanged in meaning;
    all operands double returns 0."""
    r = tape()
    for shape in ("vec", "mix"):
        for mask in masks(kind):
            check_tape_case(r, kind, shape, "std", path, mask, propto=True)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_tape_latent_gp_device_operands(kind):
    """y device data, mu = L eta a device matrix of vars, sigma (and nu) vars:
    the gradient over (GP sigma, length scale, eta, sigma, nu) matches the same
    model with f brought to the host within 1e-10 relative; the stacks are
    empty afterwards."""
    r = tape()
    gd, gh = r[f"grad_gp_{kind}_dev"], r[f"grad_gp_{kind}_host"]
    assert len(gd) == GP_N + (4 if kind == 0 else 3) and np.all(np.isfinite(gd))
    ratio = np.abs(gd - gh) / np.abs(gh)
    print(f"latent GP {NAME[kind]}: worst |dev - host| / |host| = {ratio.max():.3e}")
    assert ratio.max() <= 1e-10
    fd, fh = r[f"fx_gp_{kind}_dev"][0], r[f"fx_gp_{kind}_host"][0]
    assert abs(fd - fh) <= 1e-10 * abs(fh)
    assert list(r["stack"]) == [0.0, 0.0]


# ------------------------------------------------------------ 4. errors
@functools.lru_cache(maxsize=None)
def errors():
    got = {}
    for line in _run("errors\n").strip().splitlines():
        case, kind, moved, msg = line.split("|", 3)
        got[case] = (kind, moved, msg)
    return got


SIZES_MSG = ("; a function was called with arguments of different scalar, array, vector, or matrix types, and they "
             "were not consistently sized;  all arguments must be scalars or multidimensional values of the same "
             "shape.")
Y, NU, MU, SG = "Random variable", "Degrees of freedom parameter", "Location parameter", "Scale parameter"


def dom(fn, what):
    return ("domain_error", "0", f"{fn}_lpdf: {what}")


def size(fn, name, have, want=4):
    return ("invalid_argument", "0", f"{fn}_lpdf: {name} has dimension = {have}, expecting dimension = {want}" + SIZES_MSG)


EXPECTED = {
    "t_y_nan": dom("student_t", f"{Y}[2] is nan, but must not be nan!"),
    "t_nu_zero": dom("student_t", f"{NU}[3] is 0, but must be > 0!"),
    "t_nu_neg": dom("student_t", f"{NU}[1] is -1, but must be > 0!"),
    "t_nu_nan": dom("student_t", f"{NU}[4] is nan, but must be > 0!"),
    "t_nu_inf": dom("student_t", f"{NU}[2] is inf, but must be finite!"),
    "t_nu_inf_then_neg": dom("student_t", f"{NU}[3] is -1, but must be > 0!"),
    "t_mu_inf": dom("student_t", f"{MU}[1] is inf, but must be finite!"),
    "t_mu_nan": dom("student_t", f"{MU}[4] is nan, but must be finite!"),
    "t_sigma_zero": dom("student_t", f"{SG}[4] is 0, but must be > 0!"),
    "t_sigma_nan": dom("student_t", f"{SG}[2] is nan, but must be > 0!"),
    "t_sigma_inf": dom("student_t", f"{SG}[3] is inf, but must be finite!"),
    "t_sigma_inf_then_zero": dom("student_t", f"{SG}[2] is 0, but must be > 0!"),
    "c_y_nan": dom("cauchy", f"{Y}[4] is nan, but must not be nan!"),
    "c_mu_inf": dom("cauchy", f"{MU}[2] is -inf, but must be finite!"),
    "c_sigma_neg": dom("cauchy", f"{SG}[1] is -2, but must be > 0!"),
    "c_sigma_inf": dom("cauchy", f"{SG}[4] is inf, but must be finite!"),
    "c_sigma_inf_then_nan": dom("cauchy", f"{SG}[3] is nan, but must be > 0!"),
    "t_y_and_sigma": dom("student_t", f"{Y}[3] is nan, but must not be nan!"),
    "t_nu_and_mu": dom("student_t", f"{NU}[4] is inf, but must be finite!"),
    "t_mu_and_sigma": dom("student_t", f"{MU}[3] is nan, but must be finite!"),
    "c_mu_and_sigma": dom("cauchy", f"{MU}[3] is inf, but must be finite!"),
    "t_scalar_y_nan": dom("student_t", f"{Y} is nan, but must not be nan!"),
    "t_scalar_nu_zero": dom("student_t", f"{NU} is 0, but must be > 0!"),
    "t_scalar_nu_inf": dom("student_t", f"{NU} is inf, but must be finite!"),
    "t_scalar_mu_inf": dom("student_t", f"{MU} is inf, but must be finite!"),
    "t_scalar_sigma_neg": dom("student_t", f"{SG} is -1.5, but must be > 0!"),
    "t_scalar_sigma_inf": dom("student_t", f"{SG} is inf, but must be finite!"),
    "c_scalar_y_nan": dom("cauchy", f"{Y} is nan, but must not be nan!"),
    "c_scalar_mu_nan": dom("cauchy", f"{MU} is nan, but must be finite!"),
    "c_scalar_sigma_zero": dom("cauchy", f"{SG} is 0, but must be > 0!"),
    "c_scalar_sigma_inf": dom("cauchy", f"{SG} is inf, but must be finite!"),
    "t_double_nu_inf": dom("student_t", f"{NU}[2] is inf, but must be finite!"),
    "c_double_sigma_zero": dom("cauchy", f"{SG}[3] is 0, but must be > 0!"),
    "t_ragged_mu": size("student_t", MU, 3),
    "t_ragged_nu_and_mu": size("student_t", NU, 2),
    "t_ragged_y_short": size("student_t", Y, 2),
    "t_ragged_and_sigma_zero": dom("student_t", f"{SG}[4] is 0, but must be > 0!"),
    "t_ragged_and_mu_inf": dom("student_t", f"{MU}[3] is inf, but must be finite!"),
    "c_ragged_sigma": size("cauchy", SG, 3),
    "c_ragged_and_y_nan": dom("cauchy", f"{Y}[1] is nan, but must not be nan!"),
}
ZEROS = ("t_double_propto", "c_double_propto", "t_empty_nu", "c_empty_y")
VALUES = ("t_ok", "c_ok", "t_scalar_ok", "c_scalar_ok")
DEVOP = {
    "devop_t_y_nan": dom("student_t", f"{Y}[2] is nan, but must not be nan!"),
    "devop_t_mu_inf": dom("student_t", f"{MU}[3] is inf, but must be finite!"),
    "devop_c_mu_inf_and_sigma": dom("cauchy", f"{MU}[3] is inf, but must be finite!"),
    "devop_t_ragged_mu": size("student_t", MU, 3),
    "devop_t_ragged_and_y_nan": dom("student_t", f"{Y}[2] is nan, but must not be nan!"),
}


@gpu
@pytest.mark.parametrize("path", ["host", "dev"])
def test_cpp_argument_errors(path):
    """Every message verbatim, for scalar and vector operands, on the host
    path and on the device path: the checks in their order, "> 0" before
    "finite" within one operand, ragged sizes after the domain checks, an
    empty operand returning 0; the tape is as the call found it after each
    throw (the third field)."""
    e = errors()
    assert sum(1 for k in e if k.startswith(path + "_")) == len(EXPECTED) + len(ZEROS) + len(VALUES)
    for case, want in EXPECTED.items():
        assert e[f"{path}_{case}"] == want, case
    for case in ZEROS:
        assert e[f"{path}_{case}"] == ("value", "0", "0"), case
    for case in VALUES:
        kind, _, v = e[f"{path}_{case}"]
        assert kind == "value" and np.isfinite(float(v)) and float(v) < 0, case
    # the two paths agree on the values within the bound's scale
    for case in VALUES:
        a, b = float(e[f"host_{case}"][2]), float(e[f"dev_{case}"][2])
        assert abs(a - b) <= 1e-12 * (abs(a) + 10.0), case


@gpu
def test_cpp_argument_errors_device_operands():
    e = errors()
    for case, want in DEVOP.items():
        assert e[case] == want, case
    for case, host in (("devop_t_ok", "host_t_ok"), ("devop_c_ok", "host_c_ok")):
        a, b = float(e[case][2]), float(e[host][2])
        assert e[case][0] == "value" and abs(a - b) <= 1e-12 * (abs(a) + 10.0), case
    assert e["stack"] == ("0", "0", "")
