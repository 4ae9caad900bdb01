"""Indexing device vectors by group: the C entries smg_gather and
smg_segment_sum through ctypes, and gather / segment_sum / to_dev_index
through the tape (tests/cpp/test_index_ops.cpp).

The reference (tests/_index.py) is float64 numpy: `u[g - 1]` for the gather,
per destination the math.fsum of its terms for the sums.  `plan`, the Python
restatement of the host layer's counting sort, is held against numpy's stable
argsort and bincount without a GPU.

Bounds:
    gather: the bits of u[g - 1]; accumulating, the bits of dst0 + u[g - 1]
        (one rounded addition per element either way).
    segment sum of small integers (|v| <= 1000, fewer than 2^13 rows, so every
        partial sum is an integer below 2^53): EQUAL to the reference for every
        grouping and both values of `accumulate`, whatever the order.
    segment sum of real v (mixed sign, 12 decades): 1e-12, the project's bound
        for every device reducer, on the destination's sum of absolute terms
        (plus |out0| when accumulating); two runs give the same bits; an empty
        destination is 0 when writing and keeps its bits when accumulating.
    tape: values and partials at 1e-12 on the sum of the absolute values of
        their terms against the closed forms (fsum) or the host-vari form;
        segment_sum's gradient w[g - 1] bit for bit.

Sizes: with T the tile of smg_segment_sum (smg_index_launch_shape), R in
{1, 2, 63, 64, 65, 255, 257, T - 1, T, T + 1, 3T + 5}; the groupings of
_index.groupings at each.  No test hands a kernel an index outside 1..J.
"""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import gen
from _elt import worst
from _index import (SENTINEL, SMG_ERR_ARG, SMG_OK, Buf, IntBuf, SegmentPlan, gather, gather_ref, groupings, launch_shape,
                    plan, plan_numpy, segment_ref, shuffled)
from _reducers import same_bits
from _util import ROOT, prebuilt

gpu = pytest.mark.gpu
BOUND = 1e-12
SIZES = [1, 2, 63, 64, 65, 255, 257, "T-1", "T", "T+1", "3T+5"]


def resolve(size, T):
    return size if isinstance(size, int) else {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[size]


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


# ------------------------------------------------------------ 1. the yardstick (no GPU)
def test_plan_against_numpy():
    """No GPU: the restated counting sort against np.argsort(kind="stable")
    and np.bincount for every grouping at T = 16 and R in {1, 2, 15, 16, 17,
    53}; each destination's rows ascend; segment_ref sums what a loop over the
    rows sums."""
    T = 16
    for R in (1, 2, T - 1, T, T + 1, 3 * T + 5):
        for name, (g, J) in groupings(R, T).items():
            assert g.min() >= 1 and g.max() <= J, name
            perm, offs = plan(g, J)
            perm_np, offs_np = plan_numpy(g, J)
            assert np.array_equal(perm, perm_np) and np.array_equal(offs, offs_np), (R, name)
            assert offs[0] == 0 and offs[-1] == R and np.array_equal(np.diff(offs), np.bincount(g - 1, minlength=J))
            for j in range(J):
                rows = perm[offs[j]:offs[j + 1]]
                assert np.all(g[rows] == j + 1) and np.all(np.diff(rows) > 0), (R, name, j)
            v = np.arange(1.0, R + 1.0)
            s, a = segment_ref(v, g, J)
            loop = np.zeros(J)
            for i in range(R):
                loop[g[i] - 1] += v[i]
            assert np.array_equal(s, loop) and np.array_equal(a, loop)
    sk = groupings(3 * T + 5, T)
    for name, first, rows in (("skew aligned", T, 2 * T), ("skew shifted", T - 1, 2 * T),
                              ("skew straddling", T - 1, 2 * T + 2)):
        _, offs = plan_numpy(*sk[name])
        big = int(np.argmax(np.diff(offs)))
        assert offs[big] == first and offs[big + 1] - offs[big] == rows, name


# ------------------------------------------------------------ 2. the C entries
@gpu
@pytest.mark.parametrize("size", SIZES)
def test_gather(ctx, size):
    """Every grouping: the bits of u[g - 1], and accumulating the bits of
    dst0 + u[g - 1], in the default, the one-row and the two-row form."""
    R = resolve(size, launch_shape(ctx)["tile"])
    for width in (0, 1, 2):
        ctx.lib.smg_elt_set_width(ctx.ptr, width)
        for name, (g, J) in groupings(R, launch_shape(ctx)["tile"]).items():
            u = gen.unif(gen.SEED + 970, J, -3.0, 3.0)
            dst0 = gen.unif(gen.SEED + 971, R, -1.0, 1.0)
            ref = gather_ref(u, g)
            assert same_bits(gather(ctx, u, g), ref), (R, name, width)
            assert same_bits(gather(ctx, u, g, dst0), dst0 + ref), (R, name, width)


@gpu
@pytest.mark.parametrize("size", [65, "3T+5"])
def test_gather_alignment(ctx, size):
    """src and dst one double (8 bytes) past a 16-byte boundary, g 8 and 4
    bytes past one, each on its own and all together; the sentinels around dst
    show an overstep."""
    R = resolve(size, launch_shape(ctx)["tile"])
    g, J = groupings(R, launch_shape(ctx)["tile"])["seven shuffled"]
    u = gen.unif(gen.SEED + 970, J, -3.0, 3.0)
    dst0 = gen.unif(gen.SEED + 971, R, -1.0, 1.0)
    ref = gather_ref(u, g)
    for mis in ((True, 0, False), (False, 8, False), (False, 4, False), (False, 0, True), (True, 8, True),
                (True, 4, True)):
        assert same_bits(gather(ctx, u, g, None, mis), ref), mis
        assert same_bits(gather(ctx, u, g, dst0, mis), dst0 + ref), mis


@gpu
def test_gather_second_trip(ctx):
    """The smallest R that puts a lane of the two-row form on its second
    grid-stride trip, with the odd last row (from the launch constants)."""
    shape = launch_shape(ctx)
    assert shape["width"] == 2
    R = shape["map_threads"] * shape["map_max_blocks"] * 2 + 3
    J = 1000
    g = (1 + (gen.u01(gen.SEED + 972, R) * J).astype(np.int64)).astype(np.int32)
    u = gen.unif(gen.SEED + 970, J, -3.0, 3.0)
    assert same_bits(gather(ctx, u, g), gather_ref(u, g))


def integer_inputs(R, J):
    v = np.floor(gen.unif(gen.SEED + 973, R, -1000.0, 1001.0))
    out0 = np.floor(gen.unif(gen.SEED + 974, J, -1000.0, 1001.0))
    return v, out0


def real_inputs(R, J):
    """Mixed sign, magnitudes from 1e-6 to 1e6."""
    sign = np.where(gen.u01(gen.SEED + 975, R) < 0.5, -1.0, 1.0)
    v = sign * 10.0 ** gen.unif(gen.SEED + 976, R, -6.0, 6.0)
    out0 = gen.unif(gen.SEED + 977, J, -100.0, 100.0)
    return v, out0


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_segment_sum_exact(ctx, size):
    """Small integers: out equals the reference exactly, written and
    accumulated, for every grouping (a row skipped or taken twice at a tile
    edge has no tolerance to hide behind)."""
    T = launch_shape(ctx)["tile"]
    R = resolve(size, T)
    for name, (g, J) in groupings(R, T).items():
        v, out0 = integer_inputs(R, J)
        ref, _ = segment_ref(v, g, J)
        p = SegmentPlan(ctx, g, J)
        got = p.run(v, np.full(J, SENTINEL), 0)
        assert np.array_equal(got, ref), (R, name, np.flatnonzero(got != ref)[:8])
        got = p.run(v, out0, 1)
        assert np.array_equal(got, out0 + ref), (R, name, np.flatnonzero(got != out0 + ref)[:8])


@gpu
@pytest.mark.parametrize("size", SIZES)
def test_segment_sum_real(ctx, size):
    """Real v: the bound against fsum, the same bits from two runs, and the
    empty destinations: 0 when writing, their sentinel's bits when
    accumulating."""
    T = launch_shape(ctx)["tile"]
    R = resolve(size, T)
    for name, (g, J) in groupings(R, T).items():
        v, out0 = real_inputs(R, J)
        ref, scale = segment_ref(v, g, J)
        empty = np.bincount(g - 1, minlength=J) == 0
        out0 = np.where(empty, SENTINEL, out0)
        p = SegmentPlan(ctx, g, J)
        got = p.run(v, np.full(J, SENTINEL), 0)
        check(got, ref, f"R={R} {name} written", scale=np.where(empty, 1.0, scale))
        assert np.all(got[empty] == 0.0), (R, name)
        assert same_bits(got, p.run(v, np.full(J, SENTINEL), 0)), (R, name)
        acc = p.run(v, out0, 1)
        check(acc[~empty], (out0 + ref)[~empty], f"R={R} {name} accumulated", scale=(np.abs(out0) + scale)[~empty])
        assert same_bits(acc[empty], out0[empty]), (R, name)
        assert same_bits(acc, p.run(v, out0, 1)), (R, name)


@gpu
def test_segment_sum_alignment(ctx):
    """v and out one double past a 16-byte boundary, perm 4 and 8 bytes past
    one: the exact case at R = 3T + 5, one huge destination among singletons."""
    T = launch_shape(ctx)["tile"]
    R = 3 * T + 5
    g, J = groupings(R, T)["skew straddling, rows shuffled"]
    v, out0 = integer_inputs(R, J)
    ref, _ = segment_ref(v, g, J)
    for shift, mis in ((4, (False, False)), (8, (False, False)), (0, (True, False)), (0, (False, True)), (4, (True, True))):
        p = SegmentPlan(ctx, g, J, shift=shift)
        assert np.array_equal(p.run(v, out0, 1, mis), out0 + ref), (shift, mis)
        assert np.array_equal(p.run(v, np.full(J, SENTINEL), 0, mis), ref), (shift, mis)


@gpu
def test_arguments(ctx):
    """R = 0 and J = 0 are SMG_OK and write nothing; a null context or buffer
    or a negative size is SMG_ERR_ARG; the context's status stays 0."""
    lib, p = ctx.lib, ctx.ptr
    R, J = 33, 7
    g = groupings(R, launch_shape(ctx)["tile"])["seven shuffled"][0]
    perm, offs = plan_numpy(g, J)
    bu, bv = Buf(ctx, np.arange(1.0, J + 1.0)), Buf(ctx, np.arange(1.0, R + 1.0))
    bdst, bout, bws = (Buf(ctx, np.full(n, SENTINEL)) for n in (R, J, lib.smg_segment_sum_ws_doubles(R, J)))
    bg, bperm, boffs = IntBuf(ctx, g), IntBuf(ctx, perm), IntBuf(ctx, offs, dtype=np.int64)
    ga, ss = lib.smg_gather, lib.smg_segment_sum
    assert lib.smg_segment_sum_ws_doubles(0, 0) >= 1 and lib.smg_segment_sum_ws_doubles(R, J) >= 2
    for acc in (0, 1):
        assert ga(p, bu.ptr, bg.ptr, 0, acc, bdst.ptr) == SMG_OK
        assert ss(p, bv.ptr, bperm.ptr, boffs.ptr, 0, J, acc, bws.ptr, bout.ptr) == SMG_OK
        assert ss(p, bv.ptr, bperm.ptr, boffs.ptr, R, 0, acc, bws.ptr, bout.ptr) == SMG_OK
        assert ss(p, bv.ptr, bperm.ptr, boffs.ptr, 0, 0, acc, bws.ptr, bout.ptr) == SMG_OK
        assert ga(p, None, None, 0, acc, None) == SMG_OK
    assert ga(None, bu.ptr, bg.ptr, R, 0, bdst.ptr) == SMG_ERR_ARG
    assert ga(p, bu.ptr, bg.ptr, -1, 0, bdst.ptr) == SMG_ERR_ARG
    for args in ((None, bg.ptr, R, 0, bdst.ptr), (bu.ptr, None, R, 0, bdst.ptr), (bu.ptr, bg.ptr, R, 0, None)):
        assert ga(p, *args) == SMG_ERR_ARG
    good = [bv.ptr, bperm.ptr, boffs.ptr, R, J, 0, bws.ptr, bout.ptr]
    assert ss(None, *good) == SMG_ERR_ARG
    for k in (0, 1, 2, 6, 7):
        assert ss(p, *[None if i == k else a for i, a in enumerate(good)]) == SMG_ERR_ARG, k
    for k in (3, 4):
        assert ss(p, *[-1 if i == k else a for i, a in enumerate(good)]) == SMG_ERR_ARG, k
    s = (ctypes.c_int * 5)()
    assert lib.smg_index_launch_shape(None, s) == SMG_ERR_ARG and lib.smg_index_launch_shape(p, None) == SMG_ERR_ARG
    ctx.sync()
    for b in (bdst, bout, bws):
        assert np.all(b.read() == SENTINEL)  # nothing was written
    assert ctx.status() == 0


# ------------------------------------------------------------ 3. through the tape
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_index_ops")
TAPE_R, TAPE_J, TAPE_M = 257, 7, 8
SIGMA = 0.8


def _run(stdin):
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def _nums(*parts):
    return " ".join(repr(float(v)) for part in parts for v in np.atleast_1d(part))


@functools.lru_cache(maxsize=None)
def tape_data():
    """257 rows in 7 groups, group 4 empty, in shuffled order."""
    R, J, M = TAPE_R, TAPE_J, TAPE_M
    g = shuffled(np.array([1, 2, 3, 5, 6, 7], dtype=np.int32)[(gen.u01(gen.SEED + 980, R) * 6).astype(np.int64)],
                 gen.SEED + 981)
    assert set(g) == {1, 2, 3, 5, 6, 7}
    y = gen.unif(gen.SEED + 982, R, -2.0, 2.0)
    u = gen.unif(gen.SEED + 983, J, -1.0, 1.0)
    yc = np.floor(gen.unif(gen.SEED + 984, R, 0.0, 6.0))
    x = gen.unif(gen.SEED + 985, R * M, -1.0, 1.0)  # column-major R x M
    beta = gen.unif(gen.SEED + 986, M, -1.0, 1.0) * np.sqrt(3.0 / M)
    v = gen.unif(gen.SEED + 987, R, -2.0, 2.0)
    w = gen.unif(gen.SEED + 988, J, 0.2, 2.0) * np.where(gen.u01(gen.SEED + 989, J) < 0.5, -1.0, 1.0)
    return g, y, u, yc, x, beta, v, w


@functools.lru_cache(maxsize=None)
def tape():
    """One run of the binary's tape mode: {tag: values}."""
    g, y, u, yc, x, beta, v, w = tape_data()
    out = _run(f"tape {TAPE_R} {TAPE_J} {TAPE_M}\n{' '.join(str(int(k)) for k in g)}\n"
               f"{_nums(y, u, SIGMA, yc, x, beta, v, w)}\n")
    res = {}
    for line in out.strip().splitlines():
        tag, _, vals = line.partition(" ")
        res[tag] = np.array(vals.split(), dtype=np.float64)
    return res


def by_group(terms, g, J):
    """Per group the fsum of its rows' terms and of their absolute values."""
    return segment_ref(terms, g, J)


def normal_ref(y, mu, sigma):
    """Rows' terms of normal_lpdf, and d/dmu, d/dsigma per row."""
    z = (y - mu) / sigma
    terms = np.concatenate([-0.5 * z * z, -np.log(sigma) * np.ones_like(z), np.full(len(z), -0.5 * math.log(2.0 * math.pi))])
    return terms, z / sigma, -1.0 / sigma + z * z / sigma


@gpu
@pytest.mark.parametrize("form", ["hostvec", "leaf", "sigma"])
def test_tape_gather_normal(form):
    """normal_lpdf(y | gather(u, idx), sigma): u a std::vector<var>, u a
    dev_var_matrix leaf, and sigma a var too; the value and every partial
    against the closed form."""
    g, y, u, *_ = tape_data()
    r = tape()
    terms, dmu, dsig = normal_ref(y, gather_ref(u, g), SIGMA)
    check(r[f"fx_normal_{form}"][0], math.fsum(terms), f"normal {form} value", scale=math.fsum(np.abs(terms)))
    du, du_scale = by_group(dmu, g, TAPE_J)
    grad = r[f"grad_normal_{form}"]
    assert len(grad) == TAPE_J + (form == "sigma")
    check(grad[:TAPE_J], du, f"normal {form} u'", scale=np.where(du_scale == 0.0, 1.0, du_scale))
    assert grad[3] == 0.0  # the empty group
    if form == "sigma":
        # (a row's two terms are -1 / sigma and z^2 / sigma)
        check(grad[TAPE_J], math.fsum(dsig), "normal sigma'", scale=math.fsum(dsig + 2.0 / SIGMA))


@gpu
def test_tape_gather_poisson_glm():
    """poisson_log_glm_lpmf(y, x, gather(u, idx), beta), M = 8, against the
    host form of the same call (alpha a std::vector<var>, alpha[i] =
    u[g[i]-1]): the value and the gradient over (u, beta)."""
    g, _, u, yc, x, beta, *_ = tape_data()
    r = tape()
    X = x.reshape(TAPE_M, TAPE_R).T
    theta = X @ beta + gather_ref(u, g)
    lam = np.exp(theta)
    resid = yc - lam
    vterms = np.concatenate([yc * theta, -lam, [-math.lgamma(k + 1.0) for k in yc]])
    check(r["fx_poisson_dev"][0], r["fx_poisson_host"][0], "poisson value", scale=math.fsum(np.abs(vterms)))
    check(r["fx_poisson_host"][0], math.fsum(vterms), "poisson host value", scale=math.fsum(np.abs(vterms)))
    _, u_scale = by_group(resid, g, TAPE_J)
    b_scale = np.array([math.fsum(np.abs(X[:, m] * resid)) for m in range(TAPE_M)])
    scale = np.concatenate([np.where(u_scale == 0.0, 1.0, u_scale), b_scale])
    gd, gh = r["grad_poisson_dev"], r["grad_poisson_host"]
    assert len(gd) == TAPE_J + TAPE_M and np.any(gd != 0.0)
    check(gd, gh, "poisson gradient, device against host form", scale=scale)
    assert gd[3] == 0.0 and gh[3] == 0.0


@gpu
def test_tape_segment_sum():
    """sum(elt_multiply(segment_sum(v, idx), w)), w device data: the gradient
    is w[g - 1] bit for bit."""
    g, *_, v, w = tape_data()
    r = tape()
    assert same_bits(r["grad_segsum"], gather_ref(w, g))
    terms = gather_ref(w, g) * v
    check(r["fx_segsum"][0], math.fsum(terms), "segment_sum value", scale=math.fsum(np.abs(terms)))


@gpu
def test_tape_gather_composed_with_maps():
    """exp(gather(u, idx)) as the scale of normal_lpdf(y | 0, .)."""
    g, y, u, *_ = tape_data()
    r = tape()
    s = np.exp(gather_ref(u, g))
    z = y / s
    terms = np.concatenate([-0.5 * z * z, -np.log(s), np.full(TAPE_R, -0.5 * math.log(2.0 * math.pi))])
    check(r["fx_scale"][0], math.fsum(terms), "scale value", scale=math.fsum(np.abs(terms)))
    du, _ = by_group(z * z - 1.0, g, TAPE_J)
    _, du_scale = by_group(z * z + 1.0, g, TAPE_J)
    check(r["grad_scale"], du, "scale u'", scale=np.where(du_scale == 0.0, 1.0, du_scale))


@gpu
def test_tape_nested_twice_and_data():
    """gather inside gradient(), twice, with the index built once outside:
    identical bits (the index survives the nested recovery), equal to the
    first evaluation; gather of constant device data; the stacks end empty."""
    g, _, u, *_ = tape_data()
    r = tape()
    for k in ("fx", "grad"):
        assert same_bits(r[f"{k}_twice_a"], r[f"{k}_twice_b"])
        assert same_bits(r[f"{k}_twice_a"], r[f"{k}_normal_hostvec"])
    assert same_bits(r["gather_data"], gather_ref(u, g))
    assert list(r["stack"]) == [0.0, 0.0]


@functools.lru_cache(maxsize=None)
def errors():
    return {k: tuple(v) for k, *v in (line.split("|") for line in _run("errors\n").strip().splitlines())}


RANGE = "to_dev_index: accessing element out of range. index {} out of range; {}; position = {}"


@gpu
def test_cpp_errors_and_empty():
    """An index outside 1..size throws std::out_of_range with check_range's
    message before the tape or the arena is touched (size 0: the "container is
    empty" form); a u of the wrong length or shape throws
    std::invalid_argument naming both sizes; R = 0 gives an empty result and
    no node."""
    e = errors()
    same = ("tape unchanged", "arena unchanged")
    assert e["index_zero"] == ("out_of_range", RANGE.format(0, "expecting index to be between 1 and 4", 3)) + same
    assert e["index_past"] == ("out_of_range", RANGE.format(5, "expecting index to be between 1 and 4", 2)) + same
    assert e["index_empty"] == ("out_of_range", RANGE.format(1, "container is empty and cannot be indexed", 1)) + same
    assert e["index_negative_size"][0] == "invalid_argument" and e["index_negative_size"][2:] == same
    for case, sizes in (("gather_short", ("4", "3 x 1")), ("gather_matrix", ("4", "2 x 2")),
                        ("gather_short_hostvec", ("4", "3 x 1")), ("gather_short_data", ("4", "3 x 1")),
                        ("segment_sum_short", ("5", "4 x 1"))):
        kind, msg, *marks = e[case]
        assert kind == "invalid_argument" and all(s in msg for s in sizes) and tuple(marks) == same, (case, e[case])
        assert msg.startswith(case.split("_short")[0].split("_matrix")[0] + ": ")
    assert e["gather_none"][:3] == ("value", "0x1:0", "tape unchanged")
    assert e["gather_none_data"][:3] == ("value", "0", "tape unchanged")
    assert e["gather_row"][:2] == ("value", "5x1:5")
    kind, v, *_ = e["segment_sum_none"]
    assert kind == "value" and v.split()[:3] == ["4x1:4", "no", "node"] and [float(t) for t in v.split()[3:]] == [0.0] * 4
    assert e["stack"] == ("0", "0")
