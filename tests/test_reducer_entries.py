"""The C entries of normal_lpdf (smg_normal_lpdf, smg_normal_lpdf_fused), the
argument checks (smg_check_domain, smg_check_bounded_int) and the two small
publishers (smg_publish_to_host, smg_gather_scalars) through ctypes.

normal_lpdf.  Reference: `_reducers.normal_ref` (float64 + math.fsum), held to
50-digit mpmath at n = 257 without a GPU.  Bounds on the device: the value and
every reduced partial (a stride-0 / scalar operand's) within 1e-13 of the sum
of their terms' absolute values -- test_gpu_kernels.test_normal's tolerance,
moved to the cancellation-safe scale (the value's three groups and the sigma
partial's -1/sigma and z^2/sigma count as separate terms); vector partials
within 1e-13 relative, element by element.  `_reducers.normal_inputs` keeps
|z^2 - 1| >= 0.36 so that this relative bound is meaningful for the sigma
partial (z^2 - 1) / sigma.  Where a partial is accumulated onto a nonzero
preload p, the device rounds p + g once more (2^-53 |p + g|) and the test's
own expected sum p + ref, formed in float64, is rounded too (2^-53 again):
2^-52 |p + g| is added to the bound there and nowhere else.

The yardstick holds normal_ref's sums to 1.5e-15 of the same scales (ten
times the worst it measures, 1.34e-16) and its element-wise partials to 5e-15
relative: (z^2 - 1) / sigma is four roundings of 2^-53 from exact before its
cancellation and at most 6 times that after it, 2.7e-15 (measured: 1.25e-15).
The measured ratios are printed.

The checks' expected answers are a table written from the header
(include/smg_hip.h: kind 0 check_not_nan, 1 check_finite, 2 check_positive, 3
check_positive_finite), not computed by the expressions of the kernel.
"""
import ctypes
import functools

import numpy as np
import pytest

import gen
from _reducers import (check_normal_fused, host_view, normal_fused, normal_inputs, normal_mp, normal_ref,
                       same_bits)
from _util import worst

gpu = pytest.mark.gpu

SMG_ERR_ARG = 16
DBL_MAX = 1.7976931348623157e308
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


STRIDES = [(sy, smu, ss) for sy in (1, 0) for smu in (1, 0) for ss in (1, 0)]
NAMES = ("gy", "gmu", "gs")


@functools.lru_cache(maxsize=None)
def problem(n, strides, include=7):
    """(operands, normal_ref of them) at n elements; a stride-0 operand has one."""
    ops = normal_inputs(n, *(s == 1 for s in strides), seed=gen.SEED + 300 + 13 * n + 4 * strides[0] + 2 * strides[1]
                        + strides[2])
    return ops, normal_ref(*ops, include=include, n=n)


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("strides", STRIDES)
def test_normal_reference_against_mpmath(strides):
    """No GPU: normal_ref against 50-digit mpmath at n = 257: the value and the
    three partial sums within 1.5e-15 of their absolute-term sums, the
    element-wise partials within 5e-15 relative."""
    ops, ref = problem(257, strides)
    z = (ops[0] - ops[1]) / ops[2]
    assert np.all(np.abs(z * z - 1.0) >= 0.35)
    mp = normal_mp(*ops, n=257)
    for k in ("value", "sum gy", "sum gmu", "sum gs"):
        r = worst(ref[k][0], *mp[k])
        print(f"ref vs mpmath strides {strides} {k}: |diff| / abs-term sum = {r:.3e}")
        assert r <= 1.5e-15, (k, r)
    for k in NAMES:
        r = worst(ref[k], mp[k], np.abs(mp[k]))
        print(f"ref vs mpmath strides {strides} {k}: worst element-wise relative = {r:.3e}")
        assert r <= 5e-15, (k, r)


# ------------------------------------------------------------ 2. smg_normal_lpdf
def preload(n, stride, which):
    """A known nonzero adjoint: n elements for a vector operand, 3 for a
    stride-0 one (only element 0 may move)."""
    if stride == 0:
        return np.array([0.75, -1.25, 2.5]) * (which + 1)
    return (0.5 + 0.125 * (np.arange(n) % 5)) * (1.0 if which != 1 else -1.0)


def normal_dev(ctx, ops, strides, n, include=7, want=(True, True, True), pre=None):
    """smg_normal_lpdf into a NaN-prefilled out; the partials accumulate onto
    `pre` (default zeros).  -> (out[0], [adjoint array or None] * 3)."""
    d = [ctx.put(np.asarray(o, dtype=np.float64)) for o in ops]
    out = ctx.put(np.full(1, np.nan))
    g, sizes = [], []
    for i in range(3):
        k = len(pre[i]) if pre is not None else (n if strides[i] else 3)
        sizes.append(k)
        if not want[i]:
            g.append(None)
        else:
            g.append(ctx.put(pre[i]) if pre is not None else ctx.zeros(k))
    ctx.call("smg_normal_lpdf", d[0], strides[0], d[1], strides[1], d[2], strides[2], n, include, out, *g)
    return ctx.get(out, 1)[0], [None if p is None else ctx.get(p, k) for p, k in zip(g, sizes)]


def check_normal(out, gs, ref, strides, want, what, pre=None):
    r = worst(out, *ref["value"])
    print(f"{what} value: |diff| / abs-term sum = {r:.3e}")
    assert r <= 1e-13, (what, r)
    for i, k in enumerate(NAMES):
        if not want[i]:
            assert gs[i] is None
            continue
        p = pre[i] if pre is not None else np.zeros_like(gs[i])
        # two roundings of 2^-53: the device's preload + partial, and `p + ref` formed in float64 below
        slack = ULP if pre is not None else 0.0
        if strides[i]:
            tot = p + ref[k]
            r = worst(gs[i] - p, ref[k], np.abs(ref[k]))
            print(f"{what} {k}: worst element-wise relative = {r:.3e}")
            assert np.all(np.abs(gs[i] - tot) <= 1e-13 * np.abs(ref[k]) + slack * np.abs(tot)), (what, k, r)
        else:
            s, a = ref["sum " + k]
            assert same_bits(gs[i][1:], p[1:]), (what, k, "an element past 0 moved")
            r = worst(gs[i][0] - p[0], s, a)
            print(f"{what} sum {k}: |diff| / abs-term sum = {r:.3e}")
            assert abs(gs[i][0] - (p[0] + s)) <= 1e-13 * a + slack * abs(p[0] + s), (what, k, r)


@gpu
@pytest.mark.parametrize("strides", STRIDES)
def test_normal_strides(ctx, strides):
    """All eight vector / stride-0 combinations at n = 257, onto zeroed adjoints:
    a stride-0 operand gets its summed partial in element 0 alone."""
    ops, ref = problem(257, strides)
    out, gs = normal_dev(ctx, ops, strides, 257)
    check_normal(out, gs, ref, strides, (True,) * 3, f"normal_lpdf strides {strides}")


@gpu
@pytest.mark.parametrize("include", range(1, 8))
def test_normal_include_masks(ctx, include):
    ops, ref = problem(33, (1, 1, 1), include)
    out, gs = normal_dev(ctx, ops, (1, 1, 1), 33, include)
    check_normal(out, gs, ref, (1, 1, 1), (True,) * 3, f"normal_lpdf include {include}")


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262145])  # 262145: one past 1024 blocks x 256 threads
@pytest.mark.parametrize("strides", [(1, 1, 1), (1, 0, 0)])
def test_normal_sizes_accumulate(ctx, n, strides):
    """The adjoints accumulate: preload + partial, element-wise for a vector
    operand, element 0 alone (by the summed partial) for a stride-0 one."""
    ops, ref = problem(n, strides)
    pre = [preload(n, strides[i], i) for i in range(3)]
    out, gs = normal_dev(ctx, ops, strides, n, pre=pre)
    check_normal(out, gs, ref, strides, (True,) * 3, f"normal_lpdf n={n} strides {strides}", pre=pre)


@gpu
def test_normal_empty_and_null_partials(ctx):
    """n = 0: out[0] == 0.0 from a NaN prefill and no adjoint moves; a NULL
    partial pointer skips that partial and leaves the rest right."""
    one = (np.array([0.3]), np.array([0.1]), np.array([1.3]))
    for strides in ((1, 1, 1), (0, 0, 0)):
        pre = [preload(3, strides[i], i) for i in range(3)]
        out, gs = normal_dev(ctx, one, strides, 0, pre=pre)
        assert out == 0.0 and not np.signbit(out)
        for g, p in zip(gs, pre):
            assert same_bits(g[:len(p)], p)
    for strides in ((1, 1, 1), (1, 0, 0)):
        ops, ref = problem(257, strides)
        for want in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
            out, gs = normal_dev(ctx, ops, strides, 257, want=want)
            check_normal(out, gs, ref, strides, want, f"normal_lpdf strides {strides} want {want}")


# ------------------------------------------------------------ 3. smg_normal_lpdf_fused
FORMS = {"vvv": (True, True, True), "vss": (True, False, False), "svv": (False, True, True)}


def fused_ops(ops, vec):
    """A scalar operand as a float (passed as y0 / mu0 / sigma0, NULL pointer)."""
    return [o if v else float(o[0]) for o, v in zip(ops, vec)]


@gpu
@pytest.mark.parametrize("n", [1, 1024, 4096, 4097, 20000])  # 4096: the last single-block size
@pytest.mark.parametrize("form", list(FORMS))
def test_fused_sizes(ctx, n, form):
    """Vector partials are written (from a NaN prefill), a scalar operand's g
    pointer only requests the sum in res[4..6] and its target stays
    unwritten, clean inputs leave the three flags 0.0, two calls agree bitwise."""
    vec = FORMS[form]
    ops, ref = problem(n, tuple(int(v) for v in vec))
    res, gs = normal_fused(ctx, *fused_ops(ops, vec), n)
    check_normal_fused(res, gs, ref, vec, (True,) * 3, f"fused n={n} {form}")


@gpu
def test_fused_value_only_past_the_block_cap(ctx):
    """n = 2097153 = 512 blocks x 4096 + 1: the capped grid's stride loop wraps.
    y a vector, mu and sigma scalar, no partials."""
    n = 2097153
    y = gen.unif(gen.SEED + 390, n, -2.0, 2.0)
    ref = normal_ref(y, [0.1], [1.3])
    res, gs = normal_fused(ctx, y, 0.1, 1.3, n, want=(False,) * 3, twice=False)
    check_normal_fused(res, gs, ref, (True, False, False), (False,) * 3, "fused n=2097153 value only")


@gpu
@pytest.mark.parametrize("include", [1, 2, 4, 6])
def test_fused_include_masks(ctx, include):
    ops, ref = problem(33, (1, 1, 1), include)
    res, gs = normal_fused(ctx, *ops, 33, include=include)
    check_normal_fused(res, gs, ref, (True,) * 3, (True,) * 3, f"fused include {include}")


@gpu
@pytest.mark.parametrize("form", ["vvv", "vss"])
def test_fused_pinned_matches_device(ctx, form):
    """n = 1024 with every operand and output in smg_pinned_io memory (the host
    layer's zero-copy path) and once more in device memory: the same bits, and
    both within the bounds."""
    vec = FORMS[form]
    ops, ref = problem(1024, tuple(int(v) for v in vec))
    dev = normal_fused(ctx, *fused_ops(ops, vec), 1024)
    pin = normal_fused(ctx, *fused_ops(ops, vec), 1024, pinned=True)
    check_normal_fused(*pin, ref, vec, (True,) * 3, f"fused pinned {form}")
    check_normal_fused(*dev, ref, vec, (True,) * 3, f"fused device {form}")
    assert same_bits(dev[0], pin[0])
    for a, b in zip(dev[1], pin[1]):
        assert (a is None and b is None) or same_bits(a, b)


@gpu
def test_fused_flags(ctx):
    """A NaN in y, an infinity in mu, a sigma of 0, negative or NaN, each alone,
    in the first block and in the last element of an n = 20000 (five-block)
    call: its flag in res[1..3] is nonzero (the blocks' flags are summed) and
    the other two are exactly 0.0."""
    n = 20000
    ops, _ = problem(n, (1, 1, 1))
    offenders = [(0, np.nan), (1, np.inf), (1, -np.inf), (2, 0.0), (2, -0.0), (2, -1.0), (2, np.nan)]
    for which, v in offenders:
        for at in (5, n - 1):
            bad = [o.copy() for o in ops]
            bad[which][at] = v
            res, _ = normal_fused(ctx, *bad, n, want=(False,) * 3, twice=False)
            flags = res[1:4]
            assert flags[which] != 0.0 and np.isfinite(flags[which]), (which, v, at, flags)
            assert all(flags[j] == 0.0 for j in range(3) if j != which), (which, v, at, flags)
    # scalar operands are checked too (one block and five)
    for m in (33, n):
        y = np.ascontiguousarray(ops[0][:m])
        for which, v in ((1, np.inf), (2, 0.0)):
            sc = [0.1, 1.3]
            sc[which - 1] = v
            res, _ = normal_fused(ctx, y, sc[0], sc[1], m, want=(False,) * 3, twice=False)
            assert res[1 + which] != 0.0 and all(res[1 + j] == 0.0 for j in range(3) if j != which), (m, which, res)


# ------------------------------------------------------------ 4. the checks
VALUES = [np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -1.0, DBL_MAX]
#         nan inf -inf 0.0 -0.0 5e-324 -1 DBL_MAX        (1: the check fails)
DOMAIN_FAILS = {0: [1, 0, 0, 0, 0, 0, 0, 0],   # check_not_nan
                1: [1, 1, 1, 0, 0, 0, 0, 0],   # check_finite
                2: [1, 0, 1, 1, 1, 0, 1, 0],   # check_positive
                3: [1, 1, 1, 1, 1, 0, 1, 0]}   # check_positive_finite
INTS = [-2**31, -1, 0, 1, 2, 2**31 - 1]
BOUNDS = [(0, 1), (0, 2**31 - 1)]
BOUNDED_FAILS = {(0, 1): [1, 1, 0, 0, 1, 1], (0, 2**31 - 1): [1, 1, 0, 0, 0, 0]}


def positions(n):
    """0, n - 1, and an index between; at n = 262145 (1024 blocks x 256 threads
    + 1) index n - 1 is the only one of the second grid sweep and 262143 the
    last of the first."""
    return sorted({0, n - 1, 262143 if n == 262145 else n // 2})


def poke(ctx, base, index, value, dtype):
    a = np.array([value], dtype=dtype)
    rc = ctx.lib.smg_memcpy_h2d(ctx.ptr, base + index * a.itemsize, ctypes.c_void_p(a.ctypes.data), a.itemsize)
    assert rc == 0
    ctx.sync()


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 262145])
def test_check_domain(ctx, n):
    """Each value of the table as the only offender among n valid entries (1.0),
    for every kind: a failing value sets a 0.0 flag to 1.0, a passing one
    leaves a preset 0.0 and a preset 1.0 alone."""
    base = ctx.put(np.ones(n))
    for at in positions(n):
        for iv, v in enumerate(VALUES):
            poke(ctx, base, at, v, np.float64)
            flags = ctx.put(np.array([0.0] * 4 + [1.0] * 4))
            for kind in range(4):
                ctx.call("smg_check_domain", base, n, kind, flags + 8 * kind)
                ctx.call("smg_check_domain", base, n, kind, flags + 8 * (4 + kind))
            got = ctx.get(flags, 8)
            want = [float(DOMAIN_FAILS[kind][iv]) for kind in range(4)] + [1.0] * 4
            assert list(got) == want, (n, at, v, got)
        poke(ctx, base, at, 1.0, np.float64)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 262145])
def test_check_bounded_int(ctx, n):
    base = ctx.put((np.arange(n) & 1).astype(np.int32))
    for at in positions(n):
        for iv, v in enumerate(INTS):
            poke(ctx, base, at, v, np.int32)
            flags = ctx.put(np.array([0.0] * 2 + [1.0] * 2))
            for ib, (lo, hi) in enumerate(BOUNDS):
                ctx.call("smg_check_bounded_int", base, n, lo, hi, flags + 8 * ib)
                ctx.call("smg_check_bounded_int", base, n, lo, hi, flags + 8 * (2 + ib))
            got = ctx.get(flags, 4)
            want = [float(BOUNDED_FAILS[b][iv]) for b in BOUNDS] + [1.0] * 2
            assert list(got) == want, (n, at, v, got)
        poke(ctx, base, at, at & 1, np.int32)


@gpu
def test_checks_empty_and_argument_errors(ctx):
    """n = 0 is SMG_OK with the flag untouched, even with a null data pointer; a
    kind of 4 or a null flag is SMG_ERR_ARG."""
    lib = ctx.lib
    flags = ctx.put(np.array([0.0, 1.0, np.nan]))
    bad = ctx.put(np.array([np.nan]))
    badi = ctx.put(np.array([7], dtype=np.int32))
    for f in range(3):
        for data in (None, bad):
            for kind in range(4):
                assert lib.smg_check_domain(ctx.ptr, data, 0, kind, flags + 8 * f) == 0
        for data in (None, badi):
            assert lib.smg_check_bounded_int(ctx.ptr, data, 0, 0, 1, flags + 8 * f) == 0
    assert lib.smg_check_domain(ctx.ptr, bad, 1, 4, flags) == SMG_ERR_ARG
    assert lib.smg_check_domain(ctx.ptr, bad, 1, -1, flags) == SMG_ERR_ARG
    assert lib.smg_check_domain(ctx.ptr, bad, 1, 0, None) == SMG_ERR_ARG
    assert lib.smg_check_bounded_int(ctx.ptr, badi, 1, 0, 1, None) == SMG_ERR_ARG
    assert same_bits(ctx.get(flags, 3), np.array([0.0, 1.0, np.nan]))


# ------------------------------------------------------------ 5. the publishers
@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_publish_to_host(ctx, n):
    """The bits of the device source are in smg_pinned_result memory on return
    (no sync in between), and nothing past them is written."""
    src = gen.unif(gen.SEED + 400 + n, n + 1, -1e3, 1e3)[:n]
    d = ctx.put(src) if n else None
    hp = ctx.lib.smg_pinned_result(ctx.ptr, 8 * (n + 1))
    assert hp
    hv = host_view(hp, n + 1)
    hv[:] = np.nan
    ctx.call("smg_publish_to_host", d, n, hp)
    got = hv.copy()
    assert same_bits(got[:n], src) and np.isnan(got[n])


@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])  # GATHER_MAX = 64 scalars per launch
@pytest.mark.parametrize("with_status", [False, True])
def test_gather_scalars(ctx, n, with_status):
    """n device scalars scattered through one buffer arrive in order in
    smg_pinned_result memory.  With status_out, an injected status of 8 arrives
    there too, disarms the context and stays latched (read and cleared here)."""
    lib = ctx.lib
    vals = gen.unif(gen.SEED + 450 + n, 3 * n + 1, -1e3, 1e3)
    buf = ctx.put(vals)
    # scalar i sits at double 3 ((11 i) mod n) + 1 of the buffer (11 is coprime to every n here)
    where = (np.arange(n) * 11) % max(n, 1) * 3 + 1 if n else np.zeros(0, dtype=np.int64)
    assert len(set(where.tolist())) == n
    ptrs = np.array([buf + 8 * int(w) for w in where], dtype=np.uint64)
    hp = lib.smg_pinned_result(ctx.ptr, 8 * (n + 2))
    assert hp
    hv = host_view(hp, n + 1)
    hv[:] = np.nan
    st = host_view(hp + 8 * (n + 1), 2, np.int32)
    st[:] = -1
    if with_status:
        assert lib.smg_status_inject(ctx.ptr, 8) == 0
    ctx.call("smg_gather_scalars", ptrs.ctypes.data if n else None, n, hp, hp + 8 * (n + 1) if with_status else None)
    got, word = hv.copy(), st.copy()
    assert same_bits(got[:n], vals[where]) and np.isnan(got[n])
    if with_status:
        assert list(word) == [8, -1]
        armed = ctypes.c_int(-1)
        assert lib.smg_status_armed(ctx.ptr, ctypes.byref(armed)) == 0 and armed.value == 0
        assert ctx.status() == 8  # still latched; reading clears it
    else:
        assert list(word) == [-1, -1]
