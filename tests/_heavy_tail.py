"""References, inputs and ctypes callers of student_t_lpdf and cauchy_lpdf
(tests/test_heavy_tail_lpdf.py).

`st_ref` and `cauchy_ref` are float64 numpy restatements of the formulas of
prim/scal/prob/student_t_lpdf.hpp and cauchy_lpdf.hpp with every sum by
math.fsum; `st_mp` and `cauchy_mp` are the same outputs in 60-digit mpmath.
With z = (y - mu) / sigma, q = z^2 / nu, h = nu / 2:

    logp   = sum -log sqrt(pi) + lgamma(h + 1/2) - lgamma(h) - 1/2 log nu
                 - log sigma - (h + 1/2) log1p(q)
    y'     = -(nu + 1) z / (sigma nu (1 + q)),   mu' = -y'
    nu'    = 1/2 [digamma(h + 1/2) - digamma(h) - 1/nu - log1p(q) + (nu + 1) q / (nu (1 + q))]
    sigma' = -1/sigma + (nu + 1) q / (sigma (1 + q))
    Cauchy: logp = sum -log pi - log sigma - log1p(z^2), y' = -2z / (sigma (1 + z^2)),
            mu' = -y', sigma' = (z^2 - 1) / (sigma (1 + z^2))

Each returns {name: (value, scale)} with scale the sum of the absolute values
of the output's terms, a term being every separately rounded piece of the
expressions above: for logp the constant, lgamma(h + 1/2), lgamma(h),
1/2 log nu, log sigma and (h + 1/2) log1p(q) of each element (the two lgamma
are ~8e8 at nu = 1e8 and their difference is 9: no float64 evaluation is
better than 2^-53 of the larger); for nu' the five pieces in its bracket, each
halved; for sigma' its two (Cauchy: z^2 / (sigma (1 + z^2)) and
1 / (sigma (1 + z^2)), which sum to 1 / sigma); y' and mu' are single terms,
their scale is |value|.  Names: "logp"; "y'", "nu'", "mu'", "sigma'" the
element-wise partials (arrays of n); "sum y'", ... their sums over the
elements (what a scalar operand receives).
"""
import functools
import math

import numpy as np
from scipy.special import digamma, gammaln

import gen
from _reducers import host_view

NEG_LOG_SQRT_PI = -0.57236494292470008707
NEG_LOG_PI = -1.1447298858494001741
PARTIALS = ("y'", "nu'", "mu'", "sigma'")

# 64 degrees of freedom log-spaced over [0.5, 200]
NU_TABLE = 0.5 * (400.0 ** (np.arange(64) / 63.0))
# a fixed heavy-tailed table: quantiles of the t with 2 degrees of freedom at
# 61 probabilities from 0.001 to 0.999, t = (2p - 1) / sqrt(2 p (1 - p))
_P = np.concatenate([[0.001, 0.01], np.linspace(0.02, 0.98, 57), [0.99, 0.999]])
T_TABLE = (2.0 * _P - 1.0) / np.sqrt(2.0 * _P * (1.0 - _P))


def _bc(n, *ops):
    ops = [np.asarray(o, dtype=np.float64).ravel() for o in ops]
    n = max(len(o) for o in ops) if n is None else n
    return n, [np.broadcast_to(o, (n,)) for o in ops]


def _pack(n, logp_terms, el):
    """logp_terms: list of arrays (n); el: {name: list of term arrays (n)}."""
    res = {}
    t = np.concatenate(logp_terms) if logp_terms else np.zeros(0)
    res["logp"] = (math.fsum(t), math.fsum(np.abs(t)))
    for k, terms in el.items():
        terms = np.array(terms)
        val = terms.sum(axis=0) if len(terms) > 1 else terms[0]
        res[k] = (val, np.abs(terms).sum(axis=0))
        if n <= 1 << 17:  # (the sums are what scalar operands receive: never asked for beyond this)
            res["sum " + k] = (math.fsum(terms.ravel()), math.fsum(np.abs(terms).ravel()))
    return res


def st_ref(y, nu, mu, sigma, include=15, n=None):
    """include bits: 1 the constant, 2 -log sigma, 4 the log1p term, 8 the nu-only terms."""
    n, (y, nu, mu, s) = _bc(n, y, nu, mu, sigma)
    with np.errstate(over="ignore"):
        z = (y - mu) / s
        q = z * z / nu
        h = 0.5 * nu
        l = np.log1p(q)
        terms = []
        if include & 1:
            terms.append(np.full(n, NEG_LOG_SQRT_PI))
        if include & 8:
            terms += [gammaln(h + 0.5), -gammaln(h), -0.5 * np.log(nu)]
        if include & 2:
            terms.append(-np.log(s))
        if include & 4:
            terms.append(-(h + 0.5) * l)
        gy = -(nu + 1.0) * z / (s * nu * (1.0 + q))
        e = (nu + 1.0) * q / (nu * (1.0 + q))
        el = {"y'": [gy], "mu'": [-gy],
              "nu'": [0.5 * digamma(h + 0.5), -0.5 * digamma(h), -0.5 / nu, -0.5 * l, 0.5 * e],
              "sigma'": [-1.0 / s, (nu + 1.0) * q / (s * (1.0 + q))]}
    return _pack(n, terms, el)


def cauchy_ref(y, mu, sigma, include=7, n=None):
    n, (y, mu, s) = _bc(n, y, mu, sigma)
    with np.errstate(over="ignore"):
        z = (y - mu) / s
        z2 = z * z
        terms = []
        if include & 1:
            terms.append(np.full(n, NEG_LOG_PI))
        if include & 2:
            terms.append(-np.log(s))
        if include & 4:
            terms.append(-np.log1p(z2))
        gy = -2.0 * z / (s * (1.0 + z2))
        # z^2 / (1 + z^2) as 1 / (1 + 1 / z^2) past z^2 = 1: no inf / inf at |z| = 1e155 and beyond
        frac = np.where(z2 > 1.0, 1.0 / (1.0 + 1.0 / np.maximum(z2, 1.0)), z2 / (1.0 + z2))
        el = {"y'": [gy], "mu'": [-gy], "sigma'": [frac / s, -1.0 / (s * (1.0 + z2))]}
    return _pack(n, terms, el)


def _mp_outputs(kind, y, nu, mu, s, include, n):
    import mpmath as mp
    with mp.workdps(60):
        zero = mp.mpf(0)
        names = ("y'", "nu'", "mu'", "sigma'") if kind == 0 else ("y'", "mu'", "sigma'")
        lp = zero
        el = {k: [] for k in names}
        for i in range(n):
            yi, mi, si = (mp.mpf(float(v[i])) for v in (y, mu, s))
            ni = mp.mpf(float(nu[i])) if kind == 0 else mp.mpf(1)
            z = (yi - mi) / si
            q = z * z / ni
            h = ni / 2
            if include & 1:
                lp -= mp.log(mp.sqrt(mp.pi)) if kind == 0 else mp.log(mp.pi)
            if kind == 0 and include & 8:
                lp += mp.loggamma(h + mp.mpf(1) / 2) - mp.loggamma(h) - mp.log(ni) / 2
            if include & 2:
                lp -= mp.log(si)
            if include & 4:
                lp -= (h + mp.mpf(1) / 2) * mp.log(1 + q)
            gy = -(ni + 1) * z / (si * ni * (1 + q))
            el["y'"].append(gy)
            el["mu'"].append(-gy)
            el["sigma'"].append(-1 / si + (ni + 1) * q / (si * (1 + q)))
            if kind == 0:
                el["nu'"].append((mp.digamma(h + mp.mpf(1) / 2) - mp.digamma(h) - 1 / ni - mp.log(1 + q)
                                  + (ni + 1) * q / (ni * (1 + q))) / 2)
        res = {"logp": float(lp)}
        for k, v in el.items():
            res[k] = np.array([float(e) for e in v])
            res["sum " + k] = float(mp.fsum(v))
        return res


def st_mp(y, nu, mu, sigma, include=15, n=None):
    """{name: value} of st_ref's outputs in 60-digit mpmath."""
    n, (y, nu, mu, s) = _bc(n, y, nu, mu, sigma)
    return _mp_outputs(0, y, nu, mu, s, include, n)


def cauchy_mp(y, mu, sigma, include=7, n=None):
    n, (y, mu, s) = _bc(n, y, mu, sigma)
    return _mp_outputs(1, y, None, mu, s, include, n)


def with_mp(ref, mp):
    """{name: (mpmath value, the reference's scale)}."""
    return {k: (mp[k], ref[k][1]) for k in ref}


# ------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(n, seed=0):
    """(y, nu, mu, sigma), n elements each, read-only: nu from NU_TABLE, mu in
    (-2, 2), log sigma in (-1.5, 1.5), y = mu + sigma t with t from T_TABLE."""
    s0 = gen.SEED + 700 + 11 * seed
    nu = NU_TABLE[(gen.u01(s0, n) * 64).astype(np.int64)]
    mu = gen.unif(s0 + 1, n, -2.0, 2.0)
    sigma = np.exp(gen.unif(s0 + 2, n, -1.5, 1.5))
    y = mu + sigma * T_TABLE[(gen.u01(s0 + 3, n) * len(T_TABLE)).astype(np.int64)]
    out = tuple(np.ascontiguousarray(v) for v in (y, nu, mu, sigma))
    for a in out:
        a.setflags(write=False)
    return out


def yardstick_grid():
    """The yardstick's main grid: 400 elements, mu in (-2, 2), log sigma in
    (-1.5, 1.5), nu log-uniform in (0.5, 200), y = mu + sigma t, t a draw of
    the t with 2 degrees of freedom (by its quantile function)."""
    s0 = gen.SEED + 760
    n = 400
    mu = gen.unif(s0, n, -2.0, 2.0)
    sigma = np.exp(gen.unif(s0 + 1, n, -1.5, 1.5))
    nu = 0.5 * 400.0 ** gen.u01(s0 + 2, n)
    p = np.clip(gen.u01(s0 + 3, n), 1e-6, 1.0 - 1e-6)
    y = mu + sigma * (2.0 * p - 1.0) / np.sqrt(2.0 * p * (1.0 - p))
    return y, nu, mu, sigma


def extreme_grid(sigma=1.5, mu=0.0):
    """z in {0, 1e-8, 1, 1e6, 1e150, -1e150} x nu in {1e-3, 1, 4, 1e8}: 24
    elements (y = mu + sigma z; at mu = 0 every z is met to rounding)."""
    zs = np.array([0.0, 1e-8, 1.0, 1e6, 1e150, -1e150])
    nus = np.array([1e-3, 1.0, 4.0, 1e8])
    z, nu = (a.ravel() for a in np.meshgrid(zs, nus, indexing="ij"))
    return mu + sigma * z, nu.copy(), np.full(z.size, mu), np.full(z.size, sigma)


# ------------------------------------------------------------ the C entries
SENTINEL = -7.25
TAIL = 3  # sentinel doubles after each vector partial


def fused(ctx, kind, ops, n, include=None, want=None, pinned=False):
    """smg_student_t_lpdf_fused (kind 0, ops = (y, nu, mu, sigma)) or
    smg_cauchy_lpdf_fused (kind 1, ops = (y, mu, sigma)).  A float operand is
    passed as the scalar with a NULL pointer, an array as a vector.  want[i]:
    a vector operand gets a sentinel-prefilled partial vector with TAIL
    sentinels after it, a scalar operand a pointer to one sentinel (it asks
    for the reduced partial and must stay unwritten).  pinned: everything in
    one smg_pinned_io block.  -> (res[9], {name: partial vector}) with the
    sentinels before and after each partial and the unwritten targets
    checked."""
    k = len(ops)
    names = PARTIALS if kind == 0 else ("y'", "mu'", "sigma'")
    include = (15 if kind == 0 else 7) if include is None else include
    want = (True,) * k if want is None else want
    vec = [not np.isscalar(o) for o in ops]
    scal = [0.0 if v else float(o) for v, o in zip(vec, ops)]
    sizes = [n if v else 1 for v in vec]

    def dev_buffer(a):
        """a on the device behind two sentinel doubles -> (pointer to a, pointer to the block)."""
        base = ctx.put(np.concatenate([[SENTINEL, SENTINEL], a]))
        return base + 16, base
    if pinned:
        total = 16 + sum(n for v in vec if v) + sum(sz + TAIL for sz, w in zip(sizes, want) if w)
        base = ctx.lib.smg_pinned_io(ctx.ptr, 8 * total)
        assert base
        buf = host_view(base, total)
        buf[:] = np.nan
        at = [16]

        def take(cnt):
            at[0] += cnt
            return base + 8 * (at[0] - cnt), buf[at[0] - cnt:at[0]]
        res_p = base
    else:
        res_p = ctx.put(np.full(9, np.nan))
    vp, gp, gread = [], [], []
    for i, (o, v) in enumerate(zip(ops, vec)):
        if not v:
            vp.append(None)
        elif pinned:
            p, view = take(n)
            view[:] = o
            vp.append(p)
        else:
            vp.append(dev_buffer(np.asarray(o, dtype=np.float64))[0])
    for i, (sz, w) in enumerate(zip(sizes, want)):
        if not w:
            gp.append(None)
            gread.append(None)
        elif pinned:
            p, view = take(sz + TAIL)
            view[:] = SENTINEL
            gp.append(p)
            gread.append(lambda view=view: view.copy())
        else:
            p, block = dev_buffer(np.full(sz + TAIL, SENTINEL))
            gp.append(p)

            def read(block=block, sz=sz):
                g = ctx.get(block, 2 + sz + TAIL)
                assert np.all(g[:2] == SENTINEL), "wrote before its vector"
                return g[2:]
            gread.append(read)
    if kind == 0:
        ctx.call("smg_student_t_lpdf_fused", *vp, *scal, n, include, res_p, *gp)
    else:
        ctx.call("smg_cauchy_lpdf_fused", *vp, *scal, n, include, res_p, *gp)
    res = buf[:9].copy() if pinned else ctx.get(res_p, 9)
    gs = {}
    for name, v, sz, r in zip(names, vec, sizes, gread):
        if r is None:
            continue
        g = r()
        assert np.all(g[sz:] == SENTINEL), (name, "wrote past its vector")
        if v:
            assert not np.any(g[:sz] == SENTINEL), (name, "not fully written")
            gs[name] = g[:sz]
        else:
            assert g[0] == SENTINEL, (name, "the g pointer of a scalar operand was written")
    return res, gs


def got_of(kind, res, gs, ops, want=None):
    """The outputs of `fused` under the reference's names; the flag columns
    must be 0 and the reduced slot of a vector operand, or of one that asked
    for nothing, exactly 0."""
    names = PARTIALS if kind == 0 else ("y'", "mu'", "sigma'")
    cols = (5, 6, 7, 8) if kind == 0 else (5, 7, 8)
    want = (True,) * len(ops) if want is None else want
    assert list(res[1:5]) == [0.0] * 4, res[1:5]
    if kind == 1:
        assert res[6] == 0.0
    got = {"logp": res[0]}
    for name, c, o, w in zip(names, cols, ops, want):
        if np.isscalar(o) and w:
            got["sum " + name] = res[c]
        else:
            assert res[c] == 0.0, (name, res[c])
            if w:
                got[name] = gs[name]
    return got
