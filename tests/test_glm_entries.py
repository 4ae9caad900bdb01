"""The fused GLM pass (k_glm_reg in math_amd/csrc/glm.hip) for kinds 0, 1 and 2
-- smg_bernoulli_logit_glm, smg_normal_id_glm, smg_poisson_log_glm -- and the
two forms of the bernoulli entry that stan::math::bernoulli_logit_glm_lpmf
takes: smg_bernoulli_logit_glm_checked (the y-bounds count fused in) and
smg_bernoulli_logit_glm_io (parameters as kernel arguments, k_glm_io_final
behind a self-resetting ticket, the result published to pinned host memory).

Reference: `_reducers.glm_ref`, a float64 + math.fsum restatement of the
formulas in glm.hip's header comment, itself held to 50-digit mpmath without a
GPU (test_reference_against_mpmath).

Bounds.  Every sum is compared on the scale of the sum of its terms' absolute
values (`_util.check_sums`): within 1e-12 of it; alpha' and beta' also pass
within 1e-10 of their own value where that is looser.  These are the bounds
of test_glm_neg_binomial.py for the same kernel body.  The yardstick test
holds glm_ref to 2.1e-15 of the same scales: ten times the worst ratio it
measures (2.05e-16, poisson's alpha' at scale 8, where a rounding of theta ~ 8
is multiplied by exp theta; the ratios are printed) and 500 times below the
device bound.

The cutoff test's reference is the three-branch function itself in mpmath
(`glm_mp(..., cutoffs=True)`): at ytheta < -20 the reference implementation
defines theta' = sign, 2e-9 away from the smooth derivative, so the smooth
function cannot serve there.  In the mixed rows a wrong branch at |ytheta| =
20 exactly would move a sum by 2e-18 to 6e-8 of a scale of ~500, so two
uniform cases (every row at ytheta = 20, every row at -20) make it visible:
there the middle branch differs from its neighbour by 1e-9 (value at +20), 2e-9
(theta' at both) and 1e-10 (value at -20) of the sum itself.

Inputs (`inputs`): x uniform in (-1, 1), beta = scale u / sum |u|, alpha = 0.1;
y bernoulli(1/2) (kind 0), uniform in [-2, 2) with sigma = 1.7 (kind 1),
floor(exp(theta) (-log(1 - u))) (kind 2).
"""
import functools

import numpy as np
import pytest

import gen
from _reducers import (glm_mp, glm_ref, host_view, normal_fused, check_normal_fused, normal_inputs, normal_ref,
                       same_bits)
from _util import check_sums

gpu = pytest.mark.gpu

SMG_ERR_ARG = 16
ALPHA = 0.1
SIGMA = 1.7
ENTRY = {0: "smg_bernoulli_logit_glm", 1: "smg_normal_id_glm", 2: "smg_poisson_log_glm"}
WIDTH = {0: 2, 1: 2, 2: 3}  # out has M + WIDTH doubles


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


# ------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(kind, R, M, scale=1.0):
    """x (R, M), y (R; int32, float64 for kind 1), beta (M); read-only."""
    x = gen.unif(gen.SEED + 201 + 7 * R + M, R * M, -1.0, 1.0).reshape(M, R).T.copy()
    u = gen.unif(gen.SEED + 202 + M, M, -1.0, 1.0)
    beta = scale * u / max(np.abs(u).sum(), 1e-300)
    if kind == 0:
        y = gen.bernoulli(gen.SEED + 203 + R, R, 0.5)
    elif kind == 1:
        y = gen.unif(gen.SEED + 204 + R, R, -2.0, 2.0)
    else:
        theta = x @ beta + ALPHA
        y = np.floor(np.exp(theta) * -np.log1p(-gen.u01(gen.SEED + 205 + R, R))).astype(np.int32)
    for a in (x, y, beta):
        a.setflags(write=False)
    return x, y, beta


@functools.lru_cache(maxsize=None)
def ref(kind, R, M, scale=1.0):
    x, y, beta = inputs(kind, R, M, scale)
    return glm_ref(kind, y, x, ALPHA, beta, SIGMA)


# ------------------------------------------------------------ 1. the yardstick (no GPU)
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("R,M,scale", [(1000, 8, 1.0), (257, 3, 8.0), (97, 0, 1.0)])
def test_reference_against_mpmath(kind, R, M, scale):
    """No GPU: glm_ref against 50-digit mpmath from the defining expressions
    (kind 0: -log(1 + exp(-ytheta)), no cutoffs; |theta| <= 8.1 reaches none):
    every sum within 2.1e-15 of the sum of its terms' absolute values."""
    x, y, beta = inputs(kind, R, M, scale)
    if scale > 1:
        assert 6 < np.abs(x @ beta + ALPHA).max() < 8.1
    r = ref(kind, R, M, scale)
    check_sums({k: v[0] for k, v in r.items()}, glm_mp(kind, y, x, ALPHA, beta, SIGMA),
               f"ref vs mpmath kind {kind} {R}x{M} scale {scale}", b_sum=2.1e-15, b_rel=None)


# ------------------------------------------------------------ 2. the entries
def unpack(kind, o, M):
    got = {"value": o[0], "alpha'": o[1], "beta'": o[2:M + 2]}
    if kind == 2:
        got["lgamma"] = o[M + 2]
    return got


class Dev:
    """One problem on the device: y, x (leading dimension ldx, the padding rows
    NaN; no x at all when M == 0), the parameters, a workspace."""

    def __init__(self, ctx, kind, y, x, alpha, beta, sigma=SIGMA, ldx=None):
        self.ctx, self.kind, self.alpha = ctx, kind, float(alpha)
        self.R, self.M = x.shape
        R, M = x.shape
        self.ldx = R if ldx is None else ldx
        xf = np.full((self.ldx, M), np.nan)
        xf[:R] = x
        self.beta = np.ascontiguousarray(beta, dtype=np.float64)  # (host: the _io entry reads it)
        self.ws = ctx.zeros(int(ctx.lib.smg_glm_ws_doubles(R, M)))
        self.dy = ctx.put(np.ascontiguousarray(y, dtype=np.float64 if kind == 1 else np.int32)) if R else None
        self.dx = ctx.put(F(xf)) if R * M else None
        self.dab = ctx.put(np.concatenate([[alpha], self.beta, [sigma] if kind == 1 else []]))

    def plain(self, twice=True):
        """The kind's plain entry, called twice into a NaN-prefilled out: the
        two results must agree bitwise."""
        W = self.M + WIDTH[self.kind]
        return self._twice(lambda out: self.ctx.call(ENTRY[self.kind], self.dy, self.dx, self.R, self.M, self.ldx,
                                                     self.dab, self.ws, out), W, twice)

    def checked(self, twice=True):
        return self._twice(lambda out: self.ctx.call("smg_bernoulli_logit_glm_checked", self.dy, self.dx, self.R,
                                                     self.M, self.ldx, self.dab, self.ws, out), self.M + 3, twice)

    def io(self, host=True, twice=True):
        """smg_bernoulli_logit_glm_io -> out, or (out, out_h) with out_h from
        smg_pinned_result, NaN-prefilled before each call and read through
        the host pointer right after it."""
        ctx, M = self.ctx, self.M
        seen = []

        def call(out):
            hp = None
            if host:
                hp = ctx.lib.smg_pinned_result(ctx.ptr, 8 * (M + 3))
                assert hp
                hv = host_view(hp, M + 3)
                hv[:] = np.nan
            ctx.call("smg_bernoulli_logit_glm_io", self.dy, self.dx, self.R, M, self.ldx, self.alpha,
                     self.beta.ctypes.data if M else None, self.ws, out, hp)
            if host:
                seen.append(hv.copy())
        out = self._twice(call, M + 3, twice)
        if not host:
            return out
        assert not twice or same_bits(seen[0], seen[1]), "two calls differ bitwise (out_h)"
        return out, seen[0]

    def _twice(self, call, W, twice):
        outs = []
        for _ in range(2 if twice else 1):
            out = self.ctx.put(np.full(W, np.nan))
            call(out)
            outs.append(self.ctx.get(out, W))
        assert not twice or same_bits(outs[0], outs[1]), "two calls differ bitwise"
        return outs[0]


SHAPES = [(1, 8, None), (31, 8, None), (32, 8, None), (33, 8, None),   # both sides of a 32-row tile
          (97, 0, None), (97, 1, None), (97, 17, None), (97, 255, None), (97, 256, None),  # live column groups
          (33, 8, 38),          # ldx = R + 5, NaN padding rows
          (40003, 8, None)]     # 1251 tiles over 512 workgroups: both register buffers and the wrap


@gpu
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("R,M,ldx", SHAPES)
def test_entry_against_reference(ctx, kind, R, M, ldx):
    x, y, beta = inputs(kind, R, M)
    got = unpack(kind, Dev(ctx, kind, y, x, ALPHA, beta, ldx=ldx).plain(), M)
    check_sums(got, ref(kind, R, M), f"{ENTRY[kind]} {R}x{M} ldx={ldx}")


@gpu
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_entry_wide_predictor(ctx, kind):
    """The 257 x 3 case of the yardstick test (|theta| up to ~8) on the device."""
    x, y, beta = inputs(kind, 257, 3, 8.0)
    got = unpack(kind, Dev(ctx, kind, y, x, ALPHA, beta).plain(), 3)
    check_sums(got, ref(kind, 257, 3, 8.0), f"{ENTRY[kind]} 257x3 scale 8")


def bernoulli_forms(ctx, y, x, alpha, beta, ldx, r, what):
    """_checked, _io with out_h and _io without meet the reference `r`, count
    0.0, and carry the plain entry's bits."""
    M = x.shape[1]
    d = Dev(ctx, 0, y, x, alpha, beta, ldx=ldx)
    plain, chk = d.plain(), d.checked()
    io, io_h = d.io(host=True)
    io_n = d.io(host=False)
    for name, o in (("plain", plain), ("checked", chk), ("io", io), ("io out_h", io_h), ("io no out_h", io_n)):
        check_sums(unpack(0, o, M), r, f"{what} {name}")
    for name, o in (("checked", chk), ("io", io), ("io out_h", io_h), ("io no out_h", io_n)):
        assert o[M + 2] == 0.0, (name, o[M + 2])
        assert same_bits(o[:M + 2], plain), f"{name} differs bitwise from the plain entry"


@gpu
@pytest.mark.parametrize("R,M,ldx", SHAPES + [(257, 3, None)])
def test_bernoulli_forms(ctx, R, M, ldx):
    """k_glm_io_final sums in k_reduce_partials' order, so all four outputs are
    the same bits, and each is within the bounds of the reference."""
    scale = 8.0 if (R, M) == (257, 3) else 1.0
    x, y, beta = inputs(0, R, M, scale)
    bernoulli_forms(ctx, y, x, ALPHA, beta, ldx, ref(0, R, M, scale), f"bernoulli {R}x{M} ldx={ldx}")


@gpu
def test_io_ticket_reuse(ctx):
    """_io back to back at M = 8, 256 and 1 on one context (the final kernel's
    grid is 11, 259 and 4 workgroups; its ticket in red_counter_d + 1 must be
    back at zero each time), a two-block smg_normal_lpdf_fused (n = 4097, the
    ticket in red_counter_d + 0) between them; every result against its
    reference."""
    ny, nmu, ns = normal_inputs(4097, True, True, True, gen.SEED + 260)
    nref = normal_ref(ny, nmu, ns)
    devs = []
    for R, M in ((33, 8), (97, 256), (97, 1)):
        x, y, beta = inputs(0, R, M)
        devs.append((Dev(ctx, 0, y, x, ALPHA, beta), ref(0, R, M), R, M))
    for rep in range(2):
        for d, r, R, M in devs:
            out, out_h = d.io(host=True, twice=False)
            assert same_bits(out, out_h)
            assert out[M + 2] == 0.0
            check_sums(unpack(0, out_h, M), r, f"ticket round {rep} io {R}x{M}")
            res, gs = normal_fused(ctx, ny, nmu, ns, 4097, twice=False)
            check_normal_fused(res, gs, nref, (True,) * 3, (True,) * 3, f"ticket round {rep} normal after M={M}")


# ------------------------------------------------------------ 3. the y-bounds count
BAD = [2, -1, -2**31]


@gpu
@pytest.mark.parametrize("R,rows", [(33, (0, 32, 17)),          # row 32: the ragged second tile
                                    (40003, (0, 40002, 19205))])  # row 19205: tile 600, a workgroup's second buffer
def test_y_bounds_count(ctx, R, rows):
    """k rows of y outside {0, 1} (2, -1, -2^31): slot M + 2 is exactly k; valid
    y gives exactly 0.0 (test_bernoulli_forms).  Nothing is asserted about the
    other slots."""
    M = 8
    x, y, beta = inputs(0, R, M)
    cases = [[(rows[i], BAD[i])] for i in range(3)] + [[(rows[i], BAD[(i + 1) % 3]) for i in range(3)]]
    for case in cases:
        yb = y.copy()
        for row, v in case:
            yb[row] = v
        d = Dev(ctx, 0, yb, x, ALPHA, beta)
        chk = d.checked()
        io, io_h = d.io(host=True)
        for name, o in (("checked", chk), ("io", io), ("io out_h", io_h)):
            assert o[M + 2] == float(len(case)), (name, case, o[M + 2])


# ------------------------------------------------------------ 4. the cutoff branches
XCUT = np.array([25.0, -25.0, 20.0, -20.0, 19.999, -19.999, 20.001, -20.001, 0.0])


@gpu
@pytest.mark.parametrize("case", ["mixed", "all +20", "all -20"])
def test_cutoff_branches(ctx, case):
    """One column, beta = 1, alpha = 0, 64 rows, so ytheta = +-x exactly.
    mixed: x cycles through +-25, +-20, +-19.999, +-20.001, 0 and y alternates
    (9 and 2 are coprime: every x meets both y).  all +20 / all -20: x = 20 with
    y = 1 / y = 0 in every row, so ytheta is exactly 20 / -20 and must take the
    middle branch (the module docstring has the sizes).  Reference: the
    three-branch function in mpmath."""
    R = 64
    if case == "mixed":
        x = XCUT[np.arange(R) % len(XCUT)].reshape(R, 1)
        y = (np.arange(R) % 2).astype(np.int32)
    else:
        x = np.full((R, 1), 20.0)
        y = np.full(R, 1 if case == "all +20" else 0, dtype=np.int32)
    beta = np.array([1.0])
    r = glm_mp(0, y, x, 0.0, beta, cutoffs=True)
    if case != "mixed":  # the neighbouring branch is outside the bounds: the test can tell them apart
        yt = 20.0 if case == "all +20" else -20.0
        other = R * (-np.exp(-yt) if yt > 0 else yt)
        assert abs(other - r["value"][0]) > 50 * 1e-12 * r["value"][1]
    bernoulli_forms(ctx, y, x, 0.0, beta, None, r, f"cutoffs {case}")


# ------------------------------------------------------------ 5. the general paths
@gpu
def test_general_path_m257(ctx):
    """M = 257 > 256: eta and beta' by GEMM, theta' by k_glm_rows, and for
    _checked / _io the separate bounds check (ws sized by smg_glm_ws_doubles);
    then one bad y: the count is 1.0."""
    R, M = 64, 257
    x, y, beta = inputs(0, R, M)
    r = ref(0, R, M)
    d = Dev(ctx, 0, y, x, ALPHA, beta)
    check_sums(unpack(0, d.plain(twice=False), M), r, "general plain 64x257")
    chk = d.checked(twice=False)
    io, io_h = d.io(host=True, twice=False)
    io_n = d.io(host=False, twice=False)
    for name, o in (("checked", chk), ("io", io), ("io out_h", io_h), ("io no out_h", io_n)):
        check_sums(unpack(0, o, M), r, f"general {name} 64x257")
        assert o[M + 2] == 0.0, (name, o[M + 2])
    yb = y.copy()
    yb[R - 1] = 2
    d = Dev(ctx, 0, yb, x, ALPHA, beta)
    assert d.checked(twice=False)[M + 2] == 1.0
    io, io_h = d.io(host=True, twice=False)
    assert io[M + 2] == 1.0 and io_h[M + 2] == 1.0


@gpu
def test_empty_rows(ctx):
    """R = 0 at M = 8: every entry turns a NaN-prefilled out into zeros, over
    M + 2 (bernoulli, normal_id) or M + 3 (poisson, _checked, _io) slots."""
    M = 8
    _, _, beta = inputs(0, 33, M)
    x = np.zeros((0, M))
    for kind in (0, 1, 2):
        y = np.zeros(0, dtype=np.float64 if kind == 1 else np.int32)
        d = Dev(ctx, kind, y, x, ALPHA, beta)
        assert d.dy is None and d.dx is None
        assert same_bits(d.plain(), np.zeros(M + WIDTH[kind])), kind
        if kind == 0:
            assert same_bits(d.checked(), np.zeros(M + 3))
            io, io_h = d.io(host=True)
            assert same_bits(io, np.zeros(M + 3)) and same_bits(io_h, np.zeros(M + 3))
            assert same_bits(d.io(host=False), np.zeros(M + 3))


# ------------------------------------------------------------ 6. argument errors
@gpu
def test_argument_errors(ctx):
    """ldx < R with M > 0; null ab, ws or out; M = 257 on normal_id / poisson;
    null beta with M > 0 on _io: SMG_ERR_ARG (16), out untouched, the context's
    status still 0."""
    R, M = 33, 8
    lib = ctx.lib
    ws = ctx.zeros(int(lib.smg_glm_ws_doubles(R, 257)))
    for kind, name, W in ((0, ENTRY[0], M + 2), (1, ENTRY[1], M + 2), (2, ENTRY[2], M + 3),
                          (0, "smg_bernoulli_logit_glm_checked", M + 3)):
        x, y, beta = inputs(kind, R, M)
        dy, dx = ctx.put(y), ctx.put(F(x))
        dab = ctx.put(np.concatenate([[ALPHA], beta, [SIGMA], np.zeros(257)]))
        out = ctx.put(np.full(W, np.nan))
        fn = getattr(lib, name)
        assert fn(ctx.ptr, dy, dx, R, M, R - 1, dab, ws, out) == SMG_ERR_ARG, name
        assert fn(ctx.ptr, dy, dx, R, M, R, None, ws, out) == SMG_ERR_ARG, name
        assert fn(ctx.ptr, dy, dx, R, M, R, dab, None, out) == SMG_ERR_ARG, name
        assert fn(ctx.ptr, dy, dx, R, M, R, dab, ws, None) == SMG_ERR_ARG, name
        if kind in (1, 2):
            assert fn(ctx.ptr, dy, dx, R, 257, R, dab, ws, out) == SMG_ERR_ARG, name
        assert np.all(np.isnan(ctx.get(out, W))), name  # nothing was written
        assert ctx.status() == 0
    x, y, beta = inputs(0, R, M)
    dy, dx = ctx.put(y), ctx.put(F(x))
    out = ctx.put(np.full(M + 3, np.nan))
    hp = lib.smg_pinned_result(ctx.ptr, 8 * (M + 3))
    hv = host_view(hp, M + 3)
    hv[:] = np.nan
    io = lib.smg_bernoulli_logit_glm_io
    b = beta.ctypes.data
    assert io(ctx.ptr, dy, dx, R, M, R - 1, ALPHA, b, ws, out, hp) == SMG_ERR_ARG
    assert io(ctx.ptr, dy, dx, R, M, R, ALPHA, None, ws, out, hp) == SMG_ERR_ARG
    assert io(ctx.ptr, dy, dx, R, M, R, ALPHA, b, None, out, hp) == SMG_ERR_ARG
    assert io(ctx.ptr, dy, dx, R, M, R, ALPHA, b, ws, None, hp) == SMG_ERR_ARG
    assert np.all(np.isnan(ctx.get(out, M + 3))) and np.all(np.isnan(hv))
    assert ctx.status() == 0
