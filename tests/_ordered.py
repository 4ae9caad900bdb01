"""ordered_logistic_glm_lpmf: inputs and references shared by tests/test_glm_ordered.py.

With eta = x beta, cut-points c_1 < ... < c_{C-1}, c_0 = -inf, c_C = +inf,
k = y_i, a = c_k - eta, b = c_{k-1} - eta, e(z) = exp(-|z|):

    ll(z) = min(z, 0) - log1p(e(z))                        (log logistic(z))
    lg(z) = 1 / (1 + e(z)) if z >= 0 else e(z) / (1 + e(z))    (logistic(z))
    gap = c_k - c_{k-1};  lm = log(-expm1(-gap)) if gap < ln 2 else log1p(-exp(-gap));
    r = 1 / expm1(gap)                                     (lm = r = 0 for k = 1 and k = C)
    log P  = [k < C] ll(a) + [k > 1] ll(-b) + lm
    d_hi   = [k < C] (lg(-a) + r)        d_lo = [k > 1] (-lg(b) - r)
    theta' = [k > 1] lg(b) - [k < C] lg(-a)
    beta' = x^T theta'      cuts'_j = sum_{y = j} d_hi + sum_{y = j + 1} d_lo

`ol_ref` is the float64 numpy restatement (every sum by math.fsum); `ol_mp`
evaluates log(logistic(a) - logistic(b)) and its derivatives directly in
multi-precision mpmath.
"""
import functools
import math

import numpy as np

import gen

LN2 = math.log(2.0)


def spread_cuts(C, lo=-2.0, hi=2.0):
    """C - 1 cut-points, unevenly spaced in [lo, hi]."""
    K = C - 1
    if K <= 0:
        return np.zeros(0)
    if K == 1:
        return np.array([0.25])
    t = np.arange(K) / (K - 1)
    return lo + (hi - lo) * (0.7 * t + 0.3 * t * t)


@functools.lru_cache(maxsize=None)
def inputs(R, M, C, scale=3.0):
    """x (R, M) uniform in (-1, 1), y (R, int32) uniform in 1..C, beta (M) =
    scale u / sum |u| (|eta| < scale), cuts (C - 1); read-only."""
    x = gen.unif(gen.SEED + 301 + 7 * R + M, R * M, -1.0, 1.0).reshape(M, R).T.copy()
    u = gen.unif(gen.SEED + 302 + M, M, -1.0, 1.0)
    beta = scale * u / max(np.abs(u).sum(), 1e-300)
    y = (1 + np.minimum(np.floor(gen.u01(gen.SEED + 303 + R + C, R) * C), C - 1)).astype(np.int32)
    cuts = spread_cuts(C)
    for a in (x, y, beta, cuts):
        a.setflags(write=False)
    return x, y, beta, cuts


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def _fsum_cols(a):
    return np.array([_fsum(a[:, j]) for j in range(a.shape[1])])


def ol_ref(y, x, beta, cuts):
    """The float64 restatement: {name: (value, sum of the terms' absolute values)}
    for "logp" (terms ll(a), ll(-b), lm of each row), "beta'" (terms x_ij theta'_i)
    and "cuts'" (terms d_hi, d_lo of each row)."""
    y = np.asarray(y, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    cuts = np.asarray(cuts, dtype=np.float64)
    R, M = x.shape
    K = len(cuts)
    C = K + 1
    eta = x @ np.asarray(beta, dtype=np.float64) if M else np.zeros(R)
    ce = np.concatenate([[-np.inf], cuts, [np.inf]])
    lm, r = np.zeros(C + 1), np.zeros(C + 1)
    for k in range(2, C):
        gap = ce[k] - ce[k - 1]
        lm[k] = math.log(-math.expm1(-gap)) if gap < LN2 else math.log1p(-math.exp(-gap))
        em = math.expm1(gap) if gap < 709.0 else math.inf
        r[k] = 1.0 / em
    hi, lo = y < C, y > 1
    a, b = ce[y] - eta, ce[y - 1] - eta
    ea, eb = np.exp(-np.abs(a)), np.exp(-np.abs(b))
    lla = np.where(hi, np.minimum(a, 0.0) - np.log1p(ea), 0.0)
    llb = np.where(lo, np.minimum(-b, 0.0) - np.log1p(eb), 0.0)
    lgna = np.where(a <= 0, 1.0 / (1.0 + ea), ea / (1.0 + ea))
    lgb = np.where(b >= 0, 1.0 / (1.0 + eb), eb / (1.0 + eb))
    dhi = np.where(hi, lgna + r[y], 0.0)
    dlo = np.where(lo, -lgb - r[y], 0.0)
    th = np.where(lo, lgb, 0.0) - np.where(hi, lgna, 0.0)
    tb = x * th[:, None]
    cv, ca = np.zeros(K), np.zeros(K)
    for j in range(1, C):
        t = np.concatenate([dhi[y == j], dlo[y == j + 1]])
        cv[j - 1], ca[j - 1] = _fsum(t), _fsum(np.abs(t))
    return {
        "logp": (_fsum(np.concatenate([lla, llb, lm[y]])), _fsum(np.abs(lla) + np.abs(llb) + np.abs(lm[y]))),
        "beta'": (_fsum_cols(tb), _fsum_cols(np.abs(tb))),
        "cuts'": (cv, ca),
    }


def ol_mp(y, x, beta, cuts, dps=50):
    """{name: value} from the defining expressions in `dps`-digit mpmath:
    P = logistic(a) - logistic(b), logp = sum log P, and with l'(z) =
    logistic(z)(1 - logistic(z)): dlogP/dc_k = l'(a) / P, dlogP/dc_{k-1} =
    -l'(b) / P, dlogP/deta = (l'(b) - l'(a)) / P.  (1 - logistic(b) at b = 800
    needs ~350 digits: the callers with |eta| that large pass dps = 420.)"""
    import mpmath as mp
    with mp.workdps(dps):
        R, M = x.shape
        K = len(cuts)
        C = K + 1
        one, z = mp.mpf(1), mp.mpf(0)
        c = [None] + [mp.mpf(float(v)) for v in cuts] + [None]
        logp, bsum, csum = z, [z] * M, [z] * K

        def lg(v):
            return one / (one + mp.exp(-v))

        for i in range(R):
            k = int(y[i])
            eta = z
            for j in range(M):
                eta += mp.mpf(float(x[i, j])) * mp.mpf(float(beta[j]))
            la = lg(c[k] - eta) if k < C else one
            lb = lg(c[k - 1] - eta) if k > 1 else z
            P = la - lb
            da = la * (one - la) if k < C else z
            db = lb * (one - lb) if k > 1 else z
            logp += mp.log(P)
            if k < C:
                csum[k - 1] += da / P
            if k > 1:
                csum[k - 2] -= db / P
            th = (db - da) / P
            for j in range(M):
                bsum[j] += mp.mpf(float(x[i, j])) * th
        return {"logp": float(logp), "beta'": np.array([float(v) for v in bsum]),
                "cuts'": np.array([float(v) for v in csum])}
