"""The GP prelude generated straight into the Cholesky factor's buffer:
deferred values of gp_*_cov / add_diag (amd/matrix.hpp), the generator
smg_gp_chol_source_fill and the smg_cholesky_fwd_gp_* entries, and the
inverse-form reducer without K's values (smg_gp_cov_inverse_adjoint_x).

Every comparison between the deferred path and the same process with
deferral switched off (tests/cpp/test_gp_fused_prelude.cpp) is bitwise
(np.array_equal); the tape's fx and gradient are also checked against float64
numpy closed forms at the tolerances of tests/test_gp_families.py (fx 1e-12,
gradient 1e-10).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from _util import ROOT, near_rel, prebuilt

pytestmark = pytest.mark.gpu

FAMILIES = {"exp_quad": 0, "exponential": 1, "matern32": 2, "matern52": 3}
SIG, ELL, DIAG = 1.3, 0.9, 0.37
THETA = (1.3, 0.7, 0.5)
BIN = os.path.join(ROOT, "tests", "cpp", "_bin", "test_gp_fused_prelude")


class GpSource(ctypes.Structure):  # smg_gp_source (include/smg_hip.h)
    _fields_ = [("family", ctypes.c_int), ("D", ctypes.c_int), ("n", ctypes.c_int), ("pad_", ctypes.c_int),
                ("x", ctypes.c_void_p), ("sigma", ctypes.c_double), ("l", ctypes.c_double), ("d", ctypes.c_double)]


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


def colmajor(flat, ld, n):
    """(ld, n) view of a column-major buffer: column j at [:, j]."""
    return flat.reshape(n, ld).T


# --------------------------------------------------- 1. generator against composition
@functools.lru_cache(maxsize=None)
def points(n, D):
    """x (n, D) with a coincident pair (x[7] = x[3]) when there is room."""
    x = np.random.default_rng(31 * n + D).uniform(-5, 5, (n, D))
    if n > 7:
        x[7] = x[3]
    x.setflags(write=False)
    return x


def composition(ctx, fam, x, sigma, l, d):
    """tril(add_diag(gp_cov(x), d)) with zeros above, from the stored-matrix
    entries smg_gp_cov_fwd and smg_add_diag_fwd."""
    n, D = x.shape
    dx = ctx.put(x.ravel())
    dK, dKd = ctx.put(np.full(n * n, np.nan)), ctx.put(np.full(n * n, np.nan))
    ctx.call("smg_gp_cov_fwd", fam, dx, D, n, sigma, l, dK, n)
    ctx.call("smg_add_diag_fwd", dK, n, n, d, None, dKd, n)
    return dx, dKd, np.tril(colmajor(ctx.get(dKd, n * n), n, n))


@pytest.mark.parametrize("n", [2, 64, 65, 128, 301, 576])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_generator_against_composition(ctx, family, D, n):
    """smg_gp_chol_source_fill into a NaN-filled buffer: the strict lower
    triangle is K's, the diagonal sigma^2 + d, the strict upper zero, bit for
    bit what the three passes left (64, 128, 576 with D == 1: the 16-byte
    column form; 2, 65, 301 and D == 3: the generic form); with ldl = n + 2
    the padding rows stay untouched."""
    fam = FAMILIES[family]
    x = points(n, D)
    dx, _, want = composition(ctx, fam, x, SIG, ELL, DIAG)
    if n > 7:
        assert want[7, 3] == SIG * SIG  # the coincident pair
    for ldl in (n, n + 2) if n in (65, 128) else (n,):
        src = GpSource(fam, D, n, 0, dx, SIG, ELL, DIAG)
        dL = ctx.put(np.full(ldl * n, np.nan))
        ctx.call("smg_gp_chol_source_fill", ctypes.byref(src), dL, ldl)
        got = colmajor(ctx.get(dL, ldl * n), ldl, n)
        assert np.array_equal(got[:n], want), (family, D, n, ldl)
        assert np.all(np.isnan(got[n:]))
        assert np.array_equal(np.diag(got[:n]), np.full(n, SIG * SIG + DIAG))


def test_generator_argument_errors(ctx):
    n = 8
    dx, dL = ctx.put(points(n, 1).ravel()), ctx.zeros(n * n)
    fill = ctx.lib.smg_gp_chol_source_fill
    ok = dict(family=0, D=1, n=n, pad_=0, x=dx, sigma=SIG, l=ELL, d=DIAG)
    assert fill(ctx.ptr, ctypes.byref(GpSource(**ok)), dL, n) == 0
    for bad in (dict(family=4), dict(family=-1), dict(D=0), dict(n=-1), dict(x=None), dict(sigma=0.0),
                dict(sigma=np.inf), dict(l=-1.0), dict(l=np.nan), dict(d=np.inf), dict(d=np.nan)):
        assert fill(ctx.ptr, ctypes.byref(GpSource(**{**ok, **bad})), dL, n) == 16, bad
    assert fill(ctx.ptr, None, dL, n) == 16
    assert fill(ctx.ptr, ctypes.byref(GpSource(**ok)), None, n) == 16
    assert fill(ctx.ptr, ctypes.byref(GpSource(**ok)), dL, n - 1) == 16
    assert fill(ctx.ptr, ctypes.byref(GpSource(**{**ok, "n": 0, "x": None})), None, 0) == 0
    assert ctx.lib.smg_cholesky_fwd_gp_mark(ctx.ptr, None, dL, n, None) == 16


@pytest.mark.parametrize("entry,n", [("mark", 576), ("mark", 301), ("inv", 1024), ("winv", 1024), ("stream", 600)])
def test_factorisation_from_source(ctx, entry, n):
    """smg_cholesky_fwd_gp_mark / _inv / _winv / _stream against the checked
    entries on the stored K + d I: the factor, the block inverses, the
    progressive workspace and the streamed host copy bit for bit."""
    lib = ctx.lib
    x = points(n, 1)
    dx, dKd, _ = composition(ctx, 0, x, SIG, ELL, DIAG)
    src = GpSource(0, 1, n, 0, dx, SIG, ELL, DIAG)
    na, nw, T = lib.smg_cholesky_aux_doubles(n), lib.smg_cholesky_mvn_rev_ws_doubles(n), n * (n + 1) // 2
    out = []
    for gen in (False, True):
        dL, dD = ctx.put(np.full(n * n, np.nan)), ctx.zeros(na)
        ws = ctx.zeros(nw) if entry != "mark" else None
        started = ctypes.c_int(-1)
        a = (ctypes.byref(src),) if gen else (dKd, n, n)
        name = ("smg_cholesky_fwd_gp_mark" if gen else "smg_cholesky_fwd_checked_mark") + \
            ("" if entry == "mark" else "_" + entry)
        host = None
        if entry == "mark":
            ctx.call(name, *a, dL, n, dD)
        elif entry == "stream":
            dP = ctx.zeros(T)
            host = lib.smg_host_scratch(ctx.ptr, T * 8)
            assert host
            ctx.call(name, *a, dL, n, dD, ws, ctypes.byref(started), dP, host, 3)
            for p in range(lib.smg_cholesky_stream_panels(n)):
                ctx.call("smg_marker_wait", 3 + p)
            host = np.ctypeslib.as_array(ctypes.cast(host, ctypes.POINTER(ctypes.c_double)), shape=(T,)).copy()
        else:
            ctx.call(name, *a, dL, n, dD, ws, ctypes.byref(started))
        st = ctypes.c_int(-1)
        ctx.call("smg_status_mark_wait", ctypes.byref(st))
        assert st.value == 0
        if entry == "winv":
            ctx.call("smg_cholesky_inverse_wait")
        ctx.call("smg_join_async")
        ctx.sync()
        out.append((ctx.get(dL, n * n), ctx.get(dD, na), ctx.get(ws, nw) if ws else None, host, started.value))
    (L0, D0, w0, h0, s0), (L1, D1, w1, h1, s1) = out
    assert s0 == s1  # (the same schedule: *started)
    if entry == "winv":
        assert s1 == 3
    assert np.all(np.isfinite(L1)) and np.array_equal(L0, L1)
    assert np.array_equal(D0, D1)
    if entry == "winv":  # W = L^{-1} in the first n^2 doubles
        assert np.array_equal(w0[:n * n], w1[:n * n], equal_nan=True)
    if entry == "stream":
        assert np.array_equal(h0, h1)


@pytest.mark.parametrize("N,D,k", [(64, 1, 1), (301, 1, 1), (128, 3, 1), (512, 1, 2)])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_inverse_adjoint_without_values(ctx, family, N, D, k):
    """smg_gp_cov_inverse_adjoint_x (K0 recomputed from x) against
    smg_gp_cov_inverse_adjoint on the stored K0: the same sums in the same
    order over the same values, [d', sigma', l'] bit for bit (pair form 64 /
    512, generic form 301 and D == 3); d' alone with out2 = NULL."""
    fam = FAMILIES[family]
    rng = np.random.default_rng(N * 7 + D + k)
    M = rng.uniform(-1, 1, (N, N))
    C = M @ M.T / N + np.eye(N)
    s = rng.uniform(-1, 1, (k, 2 * N))
    x = rng.uniform(-3, 3, (N, D))
    sig, ell, adj = 1.3, 0.7, 0.8
    dC, ds, dx = ctx.put(F(C)), ctx.put(s.ravel()), ctx.put(x.ravel())
    dK = ctx.zeros(N * N)
    ctx.call("smg_gp_cov_fwd", fam, dx, D, N, sig, ell, dK, N)
    dd0, o0 = ctx.put(np.array([np.nan])), ctx.put(np.array([np.nan, np.nan]))
    ctx.call("smg_gp_cov_inverse_adjoint", fam, dC, N, N, ds, k, 2 * N, adj, dK, N, dx, D, sig, ell, dd0, o0)
    dd1, o1 = ctx.put(np.array([np.nan])), ctx.put(np.array([np.nan, np.nan]))
    ctx.call("smg_gp_cov_inverse_adjoint_x", fam, dC, N, N, ds, k, 2 * N, adj, dx, D, sig, ell, dd1, o1)
    dd2 = ctx.put(np.array([np.nan]))
    ctx.call("smg_gp_cov_inverse_adjoint_x", fam, dC, N, N, ds, k, 2 * N, adj, dx, D, sig, ell, dd2, None)
    r0 = np.concatenate([ctx.get(dd0, 1), ctx.get(o0, 2)])
    r1 = np.concatenate([ctx.get(dd1, 1), ctx.get(o1, 2)])
    ulp = np.abs(r1 - r0) / np.spacing(np.abs(r0))
    print(f"{family} N={N} D={D} k={k}: stored {r0} recomputed {r1} ulps {ulp}")
    assert np.array_equal(r0, r1)
    assert np.array_equal(ctx.get(dd2, 1), r0[:1])
    assert ctx.lib.smg_gp_cov_inverse_adjoint_x(ctx.ptr, fam, dC, N, N, ds, k, 2 * N, adj, None, D, sig, ell, dd1,
                                                o1) == 16


# ------------------------------------------------------------ the tape (C++ driver)
@functools.lru_cache(maxsize=None)
def tape_inputs(N):
    rng = np.random.default_rng(1000 + N)
    x = rng.uniform(-10, 10, N)
    y = rng.standard_normal(N)
    x[N // 3] = x[N // 5]  # a coincident pair
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def drive(scenario, family, N, evals=1):
    """{mode: {tag: [row, ...]}} of one run of the driver (eager and deferred
    in the same process); message rows as strings."""
    x, y = tape_inputs(N)
    head = f"{scenario} {family} {N} {evals} " + " ".join(repr(float(v)) for v in THETA)
    stdin = head + "\n" + " ".join(repr(float(v)) for v in x) + "\n" + " ".join(repr(float(v)) for v in y) + "\n"
    p = subprocess.run([prebuilt(BIN)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "stack 0 0", lines[-1]
    out = {"eager": {}, "deferred": {}}
    for ln in lines[:-1]:
        mode, rest = ln.split(" ", 1)
        if "|" in rest:
            tag, msg = rest.split("|", 1)
            out[mode].setdefault(tag, []).append(msg)
        else:
            tag, *vals = rest.split(" ")
            out[mode].setdefault(tag, []).append(np.array([float(v) for v in vals]))
    return out


def same_bits(out, skip=()):
    """Every observation of the deferred run equals the eager run's, bit for bit."""
    e, d = out["eager"], out["deferred"]
    assert sorted(e) == sorted(d)
    for tag in e:
        if tag in skip:
            continue
        assert len(e[tag]) == len(d[tag]), tag
        for a, b in zip(e[tag], d[tag]):
            if isinstance(a, str):
                assert a == b, (tag, a, b)
            else:
                assert np.array_equal(a, b), (tag, np.max(np.abs(a - b) / np.spacing(np.abs(a))))


@functools.lru_cache(maxsize=None)
def marginal_ref(N):
    """(fx, [dsigma, dl, dnoise]) of the exp_quad GP marginal in numpy:
    G = (alpha alpha^T - Kd^{-1}) / 2 against dK/dsigma = 2 K / sigma,
    dK/dl = K d^2 / l^3, dKd/dnoise = 2 noise I."""
    x, y = tape_inputs(N)
    sigma, l, noise = THETA
    d2 = (x[:, None] - x[None, :]) ** 2
    K = sigma * sigma * np.exp(-d2 / (2 * l * l))
    Kd = K + noise * noise * np.eye(N)
    L = np.linalg.cholesky(Kd)
    Kinv = np.linalg.inv(Kd)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    fx = -0.5 * y @ alpha - np.sum(np.log(np.diag(L))) - 0.5 * N * np.log(2 * np.pi)
    G = 0.5 * (np.outer(alpha, alpha) - Kinv)
    return fx, np.array([np.sum(G * 2 * K / sigma), np.sum(G * K * d2 / l ** 3), 2 * noise * np.trace(G)])


# ------------------------------------------------------------------ 2. tape gradient
@pytest.mark.parametrize("N,evals", [(64, 1), (192, 1), (576, 1), (1024, 2), (301, 1)])
def test_tape_gradient(N, evals):
    """(fx, dsigma, dl, dnoise) of the benchmark's composition under
    gradient(): 64 one tile, 192 one panel, 576 two panels with look-ahead,
    1024 the progressive-K^{-1} schedule on its second evaluation, 301 the
    generic generator -- the deferred run's bits are the eager run's, and both
    match the numpy closed forms."""
    out = drive("grad", "exp_quad", N, evals)
    fx, g = marginal_ref(N)
    for mode in ("eager", "deferred"):
        assert len(out[mode]["fx"]) == evals
        for f, gr in zip(out[mode]["fx"], out[mode]["grad"]):
            print(f"{mode} N={N}: fx {f[0]!r} (ref {fx!r}) grad {gr} (ref {g})")
            near_rel(f, fx, 1e-12, what="fx")
            near_rel(gr, g, 1e-10, what="grad")
    for a, b in zip(out["eager"]["grad"], out["deferred"]["grad"]):
        print(f"N={N}: gradient ulps eager vs deferred {np.abs(a - b) / np.spacing(np.abs(a))}")
    same_bits(out)


@pytest.mark.parametrize("family", ["exponential", "matern32", "matern52"])
def test_tape_gradient_families(family):
    """The other families through the same path (64: column form, 301: generic)."""
    for N in (64, 301):
        same_bits(drive("grad", family, N, 2))


# ------------------------------------------------------ 3. deferred values are complete
def test_values_and_adjoints_after_fused_factorisation():
    """After a factorisation that formed neither K nor Kd, K.val() and
    Kd.val() are the eager ones, and so are K.adj() and Kd.adj() after grad()."""
    out = drive("values", "exp_quad", 128)
    same_bits(out, skip=("formed_before_reads", "formed"))
    e, d = out["eager"], out["deferred"]
    assert e["formed_before_reads"][0][0] == 0 and d["formed_before_reads"][0][0] == 0
    assert e["formed"][0][0] == 0 and d["formed"][0][0] == 2  # K, then Kd (which finds K formed)
    K, Kd = d["K"][0].reshape(128, 128), d["Kd"][0].reshape(128, 128)
    assert np.array_equal(K, K.T) and np.all(np.isfinite(K))
    assert np.array_equal(np.diag(Kd), np.full(128, THETA[0] ** 2 + THETA[2] ** 2))
    L = d["L"][0].reshape(128, 128).T
    assert np.all(np.triu(L, 1) == 0.0)
    near_rel(L @ L.T, Kd, 1e-12, atol=1e-12, what="L L^T")
    fx, g = marginal_ref(128)
    near_rel(d["fx"][0], fx, 1e-12, what="fx")
    near_rel(d["grad"][0], g, 1e-10, what="grad")


@pytest.mark.parametrize("scenario,N", [("before", 128), ("between", 128), ("shared", 128), ("multiply", 128),
                                        ("vecdiag", 128), ("nested", 128), ("winv", 1024), ("eigen", 128),
                                        ("twice", 128)])
def test_deferred_scenarios(scenario, N):
    """K read before add_diag / between add_diag and cholesky_decompose, K
    under two chains, K also under multiply (the dense reverse), a vector
    diagonal, a nested tape, cholesky_decompose_with_inverse, the Eigen-typed
    functor, and a second evaluation after recover_memory()."""
    out = drive(scenario, "exp_quad", N)
    same_bits(out, skip=("formed_before_reads", "formed"))
    d = out["deferred"]
    if scenario in ("before", "between"):
        assert np.array_equal(d["K_early"][0], d["K"][0])
        assert d["formed_before_reads"][0][0] == 1  # K alone: Kd went into the factor's buffer
    if scenario == "twice":
        for tag in ("fx", "grad", "K", "Kd"):
            assert np.array_equal(d[tag][0], d[tag][1]), tag
    if scenario in ("nested", "winv", "twice", "eigen"):
        fx, g = marginal_ref(N)
        near_rel(d["fx"][0], fx, 1e-12, what="fx")
        near_rel(d["grad"][0], g, 1e-10, what="grad")


# ------------------------------------------------------------------------- 4. errors
@pytest.mark.parametrize("scenario", ["notpd", "nanx"])
def test_error_messages(scenario):
    """d = -2 sigma^2: not positive definite (from the panels); a dev_data x
    holding a NaN: not symmetric (the generator's flag, then Kd formed for the
    message) -- string for string the eager path's.  Both are status-word errors."""
    out = drive(scenario, "exp_quad", 128)
    e, d = out["eager"][scenario][0], out["deferred"][scenario][0]
    print(e)
    assert e == d
    assert e.startswith("domain_error|cholesky_decompose: ")
    assert ("not positive definite" if scenario == "notpd" else "is not symmetric") in e


# ----------------------------------------------------------- 5. nothing formed when fast
def test_no_values_formed_in_the_fast_case():
    """One benchmark-shaped gradient at n = 1024 forms no deferred matrix; a
    tape whose K is read afterwards forms exactly that one."""
    out = drive("count", "exp_quad", 1024)
    d = out["deferred"]
    assert d["formed_by_gradient"][0][0] == 0
    assert d["formed_before_reads"][0][0] == 0
    assert d["formed"][0][0] == 1
    assert out["eager"]["formed"][0][0] == 0  # (nothing is deferred with the switch off)
    same_bits(out, skip=("formed",))
