"""References and ctypes callers shared by test_glm_entries.py and
test_reducer_entries.py.

The references are float64 numpy restatements of the formulas in the header
comments of math_amd/csrc/glm.hip and of normal_lpdf
(prim/scal/prob/normal_lpdf.hpp:36-119); every sum is taken with math.fsum, so
a reference carries the rounding of its terms and no summation error.  Each
returns {name: (value, sum of the terms' absolute values)}.  The *_mp functions
are the same sums from the defining expressions in 50-digit mpmath.
"""
import ctypes
import math

import numpy as np
from scipy.special import gammaln

from _util import worst

NEG_LOG_SQRT_TWO_PI = -0.91893853320467274178


def fsum_abs(t):
    """(fsum of t, fsum of |t|)."""
    t = np.asarray(t, dtype=np.float64).ravel()
    return math.fsum(t), math.fsum(np.abs(t))


def host_view(addr, n, dtype=np.float64):
    """numpy view of n elements of pinned host memory at address `addr`."""
    ct = {np.float64: ctypes.c_double, np.int32: ctypes.c_int}[dtype]
    return np.frombuffer((ct * int(n)).from_address(int(addr)), dtype=dtype)


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------ GLM kinds 0, 1, 2
def glm_theta(x, alpha, beta):
    """x beta + alpha per row, the products summed with fsum."""
    R, M = x.shape
    if M == 0:
        return np.full(R, float(alpha))
    p = x * np.asarray(beta, dtype=np.float64)[None, :]
    return np.array([math.fsum(row) for row in p]) + alpha


def glm_ref(kind, y, x, alpha, beta, sigma=None):
    """kind 0 bernoulli_logit (the reference's three branches at ytheta > 20
    and < -20), 1 normal_id (value = sum y_scaled^2, partial mu'), 2
    poisson_log (value = sum y theta - exp theta, partial theta', and
    "lgamma" = sum lgamma(y + 1))."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    theta = glm_theta(x, alpha, beta)
    res = {}
    if kind == 0:
        sgn = 2.0 * y - 1.0
        yt = sgn * theta
        with np.errstate(over="ignore"):
            ex = np.exp(-yt)
            lp = np.where(yt > 20.0, -ex, np.where(yt < -20.0, yt, -np.log1p(ex)))
            th = np.where(yt > 20.0, -ex, np.where(yt < -20.0, sgn, sgn * ex / (ex + 1.0)))
    elif kind == 1:
        ys = (y - theta) / sigma
        lp = ys * ys
        th = ys / sigma
    else:
        ex = np.exp(theta)
        lp = y * theta - ex
        th = y - ex
        res["lgamma"] = fsum_abs(gammaln(y + 1.0))
    res["value"] = fsum_abs(lp)
    res["alpha'"] = fsum_abs(th)
    tb = x * th[:, None]
    cols = [fsum_abs(tb[:, j]) for j in range(x.shape[1])]
    res["beta'"] = (np.array([c[0] for c in cols]), np.array([c[1] for c in cols]))
    return res


def glm_mp(kind, y, x, alpha, beta, sigma=None, cutoffs=False):
    """The sums of glm_ref in 50-digit mpmath.  Kind 0 is -log(1 + exp(-ytheta))
    and its derivative; with `cutoffs` the three-branch function that the
    reference implementation defines, evaluated exactly."""
    import mpmath as mp
    with mp.workdps(50):
        R, M = x.shape
        z = mp.mpf(0)
        out = {k: [z, z] for k in ("value", "alpha'") + (("lgamma",) if kind == 2 else ())}
        bsum, babs = [z] * M, [z] * M

        def add(k, t):
            out[k][0] += t
            out[k][1] += abs(t)

        for i in range(R):
            yi = mp.mpf(float(y[i]))
            theta = mp.mpf(float(alpha))
            for j in range(M):
                theta += mp.mpf(float(x[i, j])) * mp.mpf(float(beta[j]))
            if kind == 0:
                sgn = 2 * yi - 1
                yt = sgn * theta
                ex = mp.exp(-yt)
                if cutoffs and yt > 20:
                    lp, th = -ex, -ex
                elif cutoffs and yt < -20:
                    lp, th = yt, sgn
                else:
                    lp, th = -mp.log(1 + ex), sgn * ex / (ex + 1)
            elif kind == 1:
                ys = (yi - theta) / mp.mpf(float(sigma))
                lp, th = ys * ys, ys / mp.mpf(float(sigma))
            else:
                ex = mp.exp(theta)
                lp, th = yi * theta - ex, yi - ex
                add("lgamma", mp.loggamma(yi + 1))
            add("value", lp)
            add("alpha'", th)
            for j in range(M):
                t = mp.mpf(float(x[i, j])) * th
                bsum[j] += t
                babs[j] += abs(t)
        res = {k: (float(v[0]), float(v[1])) for k, v in out.items()}
        res["beta'"] = (np.array([float(v) for v in bsum]), np.array([float(v) for v in babs]))
        return res


# ------------------------------------------------------------ normal_lpdf
def normal_ref(y, mu, sigma, include=7, n=None):
    """y, mu, sigma: arrays of n or of one element (broadcast; n is given when
    all three have one).  "value" with its three included groups as separate
    terms; the element-wise partials
    "gy", "gmu", "gs" (arrays of n); and their sums "sum gy", "sum gmu",
    "sum gs" as (value, abs), gs' two terms -1/sigma and z^2/sigma separate."""
    y, mu, s = (np.asarray(v, dtype=np.float64).ravel() for v in (y, mu, sigma))
    n = max(len(y), len(mu), len(s)) if n is None else n
    y, mu, s = (np.broadcast_to(v, (n,)) for v in (y, mu, s))
    inv = 1.0 / s
    z = (y - mu) * inv
    z2 = z * z
    terms = []
    if include & 1:
        terms.append(np.full(n, NEG_LOG_SQRT_TWO_PI))
    if include & 2:
        terms.append(-np.log(s))
    if include & 4:
        terms.append(-0.5 * z2)
    sc = inv * z
    return {
        "value": fsum_abs(np.concatenate(terms)) if terms else (0.0, 0.0),
        "gy": -sc, "gmu": sc, "gs": -inv + inv * z2,
        "sum gy": fsum_abs(-sc), "sum gmu": fsum_abs(sc), "sum gs": fsum_abs(np.concatenate([-inv, inv * z2])),
    }


def normal_mp(y, mu, sigma, include=7, n=None):
    """normal_ref's sums and element-wise partials in 50-digit mpmath."""
    import mpmath as mp
    y, mu, s = (np.asarray(v, dtype=np.float64).ravel() for v in (y, mu, sigma))
    n = max(len(y), len(mu), len(s)) if n is None else n
    y, mu, s = (np.broadcast_to(v, (n,)) for v in (y, mu, s))
    with mp.workdps(50):
        zero = mp.mpf(0)
        acc = {k: [zero, zero] for k in ("value", "sum gy", "sum gmu", "sum gs")}
        el = {"gy": [], "gmu": [], "gs": []}

        def add(k, t):
            acc[k][0] += t
            acc[k][1] += abs(t)

        for i in range(n):
            si = mp.mpf(float(s[i]))
            z = (mp.mpf(float(y[i])) - mp.mpf(float(mu[i]))) / si
            if include & 1:
                add("value", -mp.log(mp.sqrt(2 * mp.pi)))
            if include & 2:
                add("value", -mp.log(si))
            if include & 4:
                add("value", -z * z / 2)
            add("sum gy", -z / si)
            add("sum gmu", z / si)
            add("sum gs", -1 / si)
            add("sum gs", z * z / si)
            el["gy"].append(float(-z / si))
            el["gmu"].append(float(z / si))
            el["gs"].append(float((z * z - 1) / si))
        res = {k: (float(v[0]), float(v[1])) for k, v in acc.items()}
        res.update({k: np.array(v) for k, v in el.items()})
        return res


def normal_inputs(n, vy, vmu, vs, seed):
    """(y, mu, sigma), each of n elements (vector) or of one (scalar), read-only.
    sigma in (0.5, 1.5); z = (y - mu) / sigma is kept in 0.05 <= |z| <= 0.8 or
    1.2 <= |z| <= 2 wherever a vector operand lets it be chosen (both scalar:
    z = 0.3 / sigma in (0.2, 0.6)), so that the partial of sigma,
    (z^2 - 1) / sigma, loses at most a factor (1 + z^2) / |z^2 - 1| < 6 to
    cancellation and an element-wise relative bound on it is meaningful."""
    import gen
    m = max(n, 1)
    s = gen.unif(seed, m if vs else 1, 0.5, 1.5)
    u, w = gen.u01(seed + 1, m), gen.u01(seed + 2, m)
    zt = np.where(u < 0.5, 0.05 + 0.75 * w, 1.2 + 0.8 * w) * np.where(gen.u01(seed + 3, m) < 0.5, -1.0, 1.0)
    if vy:
        mu = gen.unif(seed + 4, m if vmu else 1, -0.4, 0.4)
        y = mu + s * zt
    elif vmu:
        y = np.array([0.3])
        mu = y - s * zt
    else:
        y, mu = np.array([0.3]), np.array([0.0])
    out = tuple(np.ascontiguousarray(v[:n] if vec else v[:1]) for v, vec in ((y, vy), (mu, vmu), (s, vs)))
    for a in out:
        a.setflags(write=False)
    return out


def normal_fused(ctx, y, mu, sigma, n, include=7, want=(True, True, True), pinned=False, twice=True):
    """smg_normal_lpdf_fused.  An operand that is a float is passed as the scalar
    y0 / mu0 / sigma0 with a NULL pointer, an array as a vector.  want[i]: a
    vector operand gets a NaN-prefilled partial vector, a scalar operand a g
    pointer to a NaN sentinel (it only requests the sum in res[4 + i] and must
    stay unwritten).  pinned: every operand and output in one smg_pinned_io
    block instead of device memory.  Two calls must agree bitwise.
    -> (res[7], [partial vector or None] * 3)."""
    ops = (y, mu, sigma)
    vec = [not np.isscalar(o) for o in ops]
    scal = [0.0 if v else float(o) for v, o in zip(vec, ops)]
    runs = []
    for _ in range(2 if twice else 1):
        if pinned:
            total = 8 + sum(n for v in vec if v) + sum(n if v else 1 for v, w in zip(vec, want) if w)
            base = ctx.lib.smg_pinned_io(ctx.ptr, 8 * total)
            assert base
            buf = host_view(base, total)
            buf[:] = np.nan
            at = [8]

            def take(k, at=at, base=base):
                at[0] += k
                return base + 8 * (at[0] - k), buf[at[0] - k:at[0]]
            res_p = base
            get_res = lambda: buf[:7].copy()  # noqa: E731
        else:
            res_p = ctx.put(np.full(8, np.nan))
            get_res = lambda res_p=res_p: ctx.get(res_p, 7)  # noqa: E731
        vp, gp, gread = [], [], []
        for o, v in zip(ops, vec):
            if not v:
                vp.append(None)
            elif pinned:
                p, view = take(n)
                view[:] = o
                vp.append(p)
            else:
                vp.append(ctx.put(np.asarray(o, dtype=np.float64)))
        for v, w in zip(vec, want):
            k = n if v else 1
            if not w:
                gp.append(None)
                gread.append(None)
            elif pinned:
                p, view = take(k)
                gp.append(p)
                gread.append(lambda view=view: view.copy())
            else:
                p = ctx.put(np.full(max(k, 1), np.nan))
                gp.append(p)
                gread.append(lambda p=p, k=k: ctx.get(p, k))
        ctx.call("smg_normal_lpdf_fused", vp[0], vp[1], vp[2], scal[0], scal[1], scal[2], n, include, res_p,
                 gp[0], gp[1], gp[2])
        res = get_res()
        gs = [None if r is None else r() for r in gread]
        for v, g in zip(vec, gs):
            if g is not None and not v:
                assert np.all(np.isnan(g)), "the g pointer of a scalar operand was written"
        runs.append((res, [g if v else None for v, g in zip(vec, gs)]))
    if twice:
        (r0, g0), (r1, g1) = runs
        assert same_bits(r0, r1), "two calls differ bitwise (res)"
        for a, b in zip(g0, g1):
            assert (a is None and b is None) or same_bits(a, b), "two calls differ bitwise (partials)"
    return runs[0]


def check_normal_fused(res, gs, ref, vec, want, what, flags=True):
    """res / partial vectors of normal_fused against normal_ref's dict: value
    and reduced partials within 1e-13 of their absolute-term sums, vector
    partials within 1e-13 relative element-wise (fully written: no NaN left),
    reduced slots of operands that asked for nothing exactly 0.0."""
    r = worst(res[0], *ref["value"])
    print(f"{what} value: |diff| / abs-term sum = {r:.3e}")
    assert r <= 1e-13, (what, r)
    if flags:
        assert list(res[1:4]) == [0.0, 0.0, 0.0], (what, res[1:4])
    for i, k in enumerate(("gy", "gmu", "gs")):
        if vec[i]:
            assert res[4 + i] == 0.0, (what, k, res[4 + i])
            if want[i]:
                assert np.all(np.isfinite(gs[i])), (what, k, "not fully written")
                r = worst(gs[i], ref[k], np.abs(ref[k]))
                print(f"{what} {k}: worst element-wise relative = {r:.3e}")
                assert r <= 1e-13, (what, k, r)
        elif want[i]:
            r = worst(res[4 + i], *ref["sum " + k])
            print(f"{what} sum {k}: |diff| / abs-term sum = {r:.3e}")
            assert r <= 1e-13, (what, k, r)
        else:
            assert res[4 + i] == 0.0, (what, k, res[4 + i])
