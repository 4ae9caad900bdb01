"""References, inputs and the ctypes caller of test_glm_vec_intercept.py: the
four row-wise GLMs (kind 0 bernoulli_logit, 1 normal_id, 2 poisson_log, 3
neg_binomial_2_log) with one intercept per row.

The float64 reference is the formulas of the header comment of
math_amd/csrc/glm.hip with theta_i = x_i beta + alpha_i; every sum is taken with
math.fsum, so a reference carries the rounding of its terms and no summation
error.  `vec_ref` returns the reduced sums as {name: (value, sum of the terms'
absolute values)} under the names the scalar references use (kinds 0-2:
"value", "alpha'", "beta'", kind 2 also "lgamma"; kind 3: "A", "B", "C", "D",
"alpha'", "beta'", "phi'"), and per row theta' with the sum of its terms'
absolute values:

    kind 0  theta' = sign exp(-ytheta) / (1 + exp(-ytheta)), at most 1 in size   scale 1
    kind 1  mu' = (y - x beta - alpha) / sigma^2      scale (|y| + sum_j |x_j beta_j| + |alpha|) / sigma^2
    kind 2  theta' = y - exp(theta)                   scale |y| + exp(theta)
    kind 3  theta' = y - (y + phi) s                  scale |y| + (y + phi) s

`vec_mp` is the same from the defining expressions in 50-digit mpmath.
"""
import functools
import math

import numpy as np
from scipy.special import digamma, gammaln

import gen
from _reducers import fsum_abs, same_bits

KINDS = (0, 1, 2, 3)
NAMES = {0: "bernoulli_logit", 1: "normal_id", 2: "poisson_log", 3: "neg_binomial_2_log"}
SIGMA = 1.3
PHI = 0.7


def F(a):  # column-major flat
    return np.asfortranarray(a).ravel(order="F")


def out_width(kind, M):
    return M + (6 if kind == 3 else 2 if kind == 1 else 3)


def extra_of(kind):
    """The kind's third parameter: sigma, phi, or none."""
    return SIGMA if kind == 1 else PHI if kind == 3 else None


@functools.lru_cache(maxsize=None)
def inputs(kind, R, M, scale=1.0):
    """x (R, M) uniform in (-1, 1), beta (M) = scale u / sum |u|, alpha_vec (R)
    uniform in (-0.5, 0.5), and y of the kind: a Bernoulli draw at
    logistic(theta), theta + sigma (a uniform in (-2, 2)), or the
    exponentially mixed count floor(exp(theta) (-log(1 - u))); read-only."""
    x = gen.unif(gen.SEED + 201 + 7 * R + M, R * M, -1.0, 1.0).reshape(M, R).T.copy()
    u = gen.unif(gen.SEED + 202 + M, M, -1.0, 1.0)
    beta = scale * u / max(np.abs(u).sum(), 1e-300)
    av = gen.unif(gen.SEED + 204 + R, R, -0.5, 0.5)
    theta = x @ beta + av
    u = gen.u01(gen.SEED + 203 + R, R)
    if kind == 0:
        y = (u < 1.0 / (1.0 + np.exp(-theta))).astype(np.int32)
    elif kind == 1:
        y = theta + SIGMA * (4.0 * u - 2.0)
    else:
        y = np.floor(np.exp(theta) * -np.log1p(-u)).astype(np.int32)
    for a in (x, y, beta, av):
        a.setflags(write=False)
    return x, y, beta, av


def theta_rows(x, av, beta):
    """(x beta + alpha per row, sum_j |x_j beta_j| per row), the products summed with fsum."""
    p = x * np.asarray(beta, dtype=np.float64)[None, :]
    eta = np.array([math.fsum(row) for row in p]) if x.shape[1] else np.zeros(x.shape[0])
    return eta + np.asarray(av, dtype=np.float64), np.abs(p).sum(axis=1)


def vec_ref(kind, y, x, av, beta, extra=None):
    """-> (sums {name: (value, abs)}, theta' (R), its per-row scale (R))."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    av = np.asarray(av, dtype=np.float64)
    theta, eabs = theta_rows(x, av, beta)
    res = {}
    if kind == 0:
        sgn = 2.0 * y - 1.0
        yt = sgn * theta
        with np.errstate(over="ignore"):
            ex = np.exp(-yt)
            lp = np.where(yt > 20.0, -ex, np.where(yt < -20.0, yt, -np.log1p(ex)))
            th = np.where(yt > 20.0, -ex, np.where(yt < -20.0, sgn, sgn * ex / (ex + 1.0)))
        res["value"] = fsum_abs(lp)
        tsc = np.ones(len(y))
    elif kind == 1:
        ys = (y - theta) / extra
        th = ys / extra
        res["value"] = fsum_abs(ys * ys)
        tsc = (np.abs(y) + eabs + np.abs(av)) / (extra * extra)
    elif kind == 2:
        ex = np.exp(theta)
        th = y - ex
        res["value"] = fsum_abs(y * theta - ex)
        res["lgamma"] = fsum_abs(gammaln(y + 1.0))
        tsc = np.abs(y) + ex
    else:
        phi = extra
        lphi = np.log(phi)
        d = theta - lphi
        e = np.exp(-np.abs(d))
        lse = np.maximum(theta, lphi) + np.log1p(e)
        inv = 1.0 / (1.0 + e)
        s = np.where(d >= 0, inv, e * inv)
        s1 = np.where(d >= 0, e * inv, inv)
        yp = y + phi
        th = y - yp * s
        tsc = np.abs(y) + yp * s
        res["A"], res["B"] = fsum_abs(yp * lse), fsum_abs(y * theta)
        res["C"], res["D"] = fsum_abs(gammaln(y + 1.0)), fsum_abs(gammaln(yp))
        g = np.concatenate([1.0 - yp * s1 / phi, lphi - lse, digamma(yp) - digamma(phi)])
        res["phi'"] = fsum_abs(g)
    res["alpha'"] = fsum_abs(th)
    tb = x * th[:, None]
    cols = [fsum_abs(tb[:, j]) for j in range(x.shape[1])]
    res["beta'"] = (np.array([c[0] for c in cols]), np.array([c[1] for c in cols]))
    return res, th, tsc


def vec_mp(kind, y, x, av, beta, extra=None):
    """vec_ref's sums from the defining expressions in 50-digit mpmath (kind 0:
    -log(1 + exp(-ytheta)) and its derivative; kind 3: exp(theta) formed
    directly) -> (sums, theta' (R) rounded to float64)."""
    import mpmath as mp
    with mp.workdps(50):
        R, M = x.shape
        z = mp.mpf(0)
        names = {0: ("value",), 1: ("value",), 2: ("value", "lgamma"), 3: ("A", "B", "C", "D", "phi'")}[kind]
        out = {k: [z, z] for k in names + ("alpha'",)}
        bsum, babs, ths = [z] * M, [z] * M, []

        def add(k, *ts):
            out[k][0] += sum(ts)
            out[k][1] += sum(abs(t) for t in ts)

        ex_ = None if extra is None else mp.mpf(float(extra))
        for i in range(R):
            yi = mp.mpf(float(y[i]))
            theta = mp.mpf(float(av[i]))
            for j in range(M):
                theta += mp.mpf(float(x[i, j])) * mp.mpf(float(beta[j]))
            if kind == 0:
                sgn = 2 * yi - 1
                e = mp.exp(-sgn * theta)
                add("value", -mp.log(1 + e))
                th = sgn * e / (e + 1)
            elif kind == 1:
                ys = (yi - theta) / ex_
                add("value", ys * ys)
                th = ys / ex_
            elif kind == 2:
                e = mp.exp(theta)
                add("value", yi * theta - e)
                add("lgamma", mp.loggamma(yi + 1))
                th = yi - e
            else:
                et = mp.exp(theta)
                lse = mp.log(et + ex_)
                s = et / (et + ex_)
                yp = yi + ex_
                add("A", yp * lse)
                add("B", yi * theta)
                add("C", mp.loggamma(yi + 1))
                add("D", mp.loggamma(yp))
                add("phi'", 1 - yp * (1 - s) / ex_, mp.log(ex_) - lse, mp.digamma(yp) - mp.digamma(ex_))
                th = yi - yp * s
            add("alpha'", th)
            ths.append(float(th))
            for j in range(M):
                t = mp.mpf(float(x[i, j])) * th
                bsum[j] += t
                babs[j] += abs(t)
        res = {k: (float(v[0]), float(v[1])) for k, v in out.items()}
        res["beta'"] = (np.array([float(v) for v in bsum]), np.array([float(v) for v in babs]))
        return res, np.array(ths)


# ------------------------------------------------------------ the C entries
PAD = 64          # doubles behind alpha_vec (NaN) and theta_adj (a sentinel)
SENTINEL = -1234.5


def ab_of(kind, beta, extra, alpha=0.0):
    """[alpha, beta(M)(, sigma | phi)], alpha 0 by default; vec_dev passes NaN in
    slot 0, which the vector entry must not read."""
    tail = [] if extra is None else [extra]
    return np.concatenate([[alpha], beta, tail])


def ws_doubles(lib, kind, R, M):
    f = lib.smg_neg_binomial_2_log_glm_ws_doubles if kind == 3 else lib.smg_glm_ws_doubles
    return int(f(max(R, 1), M))


def split_out(kind, o, M):
    """The entry's `out` under the references' names."""
    d = {"alpha'": o[1], "beta'": o[2:M + 2]}
    if kind == 3:
        d.update({"A": o[0], "B": o[M + 2], "C": o[M + 3], "D": o[M + 4], "phi'": o[M + 5]})
    else:
        d["value"] = o[0]
        if kind == 2:
            d["lgamma"] = o[M + 2]
        if kind == 0:
            d["bad y"] = o[M + 2]
    return d


def vec_dev(ctx, kind, y, x, av, beta, extra=None, ldx=None, want_theta=True, calls=2):
    """smg_glm_vec_intercept -> (out (raw), theta_adj (R) or None).  x is stored
    with leading dimension ldx, the padding rows NaN; alpha_vec is followed by
    PAD NaNs and theta_adj by PAD sentinels, which must be unchanged; ab[0] is
    NaN (ignored); `calls` calls on the same buffers must agree bitwise."""
    R, M = x.shape
    ldx = R if ldx is None else ldx
    xf = np.full((ldx, M), np.nan)
    xf[:R] = x
    W = out_width(kind, M)
    ws = ctx.zeros(ws_doubles(ctx.lib, kind, R, M))
    dy = ctx.put(np.ascontiguousarray(y, dtype=np.float64 if kind == 1 else np.int32)) if R else None
    dx = ctx.put(F(xf)) if R * M else None
    dav = ctx.put(np.concatenate([np.asarray(av, dtype=np.float64), np.full(PAD, np.nan)]))
    dab = ctx.put(ab_of(kind, beta, extra, np.nan))
    dth = ctx.put(np.full(R + PAD, SENTINEL)) if want_theta else None
    runs = []
    for _ in range(calls):
        out = ctx.put(np.full(W, np.nan))
        ctx.call("smg_glm_vec_intercept", kind, dy, dx, R, M, ldx, dav, dab, ws, out, dth)
        o = ctx.get(out, W)
        th = None
        if want_theta:
            t = ctx.get(dth, R + PAD)
            assert np.all(t[R:] == SENTINEL), "theta_adj was written beyond row R - 1"
            th = t[:R]
        runs.append((o, th))
    for o, th in runs[1:]:
        assert same_bits(o, runs[0][0]), "two calls differ bitwise (out)"
        assert th is None or same_bits(th, runs[0][1]), "two calls differ bitwise (theta_adj)"
    return runs[0]


SCALAR = {0: "smg_bernoulli_logit_glm_checked", 1: "smg_normal_id_glm", 2: "smg_poisson_log_glm",
          3: "smg_neg_binomial_2_log_glm"}


def scalar_dev(ctx, kind, y, x, alpha, beta, extra=None):
    """The kind's scalar entry (kind 0: _checked) -> out (raw)."""
    R, M = x.shape
    W = out_width(kind, M)
    ws = ctx.zeros(ws_doubles(ctx.lib, kind, R, M))
    dy = ctx.put(np.ascontiguousarray(y, dtype=np.float64 if kind == 1 else np.int32))
    dx = ctx.put(F(x)) if R * M else None
    out = ctx.put(np.full(W, np.nan))
    ctx.call(SCALAR[kind], dy, dx, R, M, R, ctx.put(ab_of(kind, beta, extra, alpha)), ws, out)
    return ctx.get(out, W)
