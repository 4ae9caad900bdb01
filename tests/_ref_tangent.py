"""Plain numpy references (np.longdouble, or float64 where the size asks for
BLAS) of the tangent, LU and matrix-helper entry points, and the padded
column-major buffers their kernel-level tests place every operand in.

Nothing here touches the device or the oracle library.
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SMG_ERR_ARG = 16


def gamma(k):
    return k * U / (1.0 - k * U)


def elem_bound(a0, inc, c=0):
    """|result - (a0 + inc)| for result = fl(a0 + fl(inc)) where forming inc
    takes c roundings beyond the final add (with or without an FMA)."""
    a0, inc = np.abs(np.asarray(a0, dtype=LD)), np.abs(np.asarray(inc, dtype=LD))
    return (U * (c * inc + 2.0 * (a0 + inc))).astype(np.float64)


# ------------------------------------------------------------------ layout
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def sentinel(size, seed=0):
    """A finite, position-dependent pattern no kernel produces by accident."""
    return 1.0e3 + 0.25 * ((np.arange(size, dtype=np.float64) * 7 + seed) % 4093)


class Mat:
    """A rows x cols matrix in a column-major backing buffer of ld * (cols + 1)
    doubles, ld > rows.  pad: what the padding rows and the spare column hold
    (np.nan for an input: a read of it poisons the result; "sentinel" for an
    output: a write of it shows).  A kernel that oversteps the matrix still
    lands in this buffer."""

    def __init__(self, a, ld, pad="sentinel", seed=0, name="matrix"):
        a = np.asarray(a, dtype=np.float64)
        self.name = name
        self.rows, self.cols, self.ld = a.shape[0], a.shape[1], ld
        assert ld > self.rows
        size = ld * (self.cols + 1)
        buf = sentinel(size, seed) if isinstance(pad, str) else np.full(size, pad, dtype=np.float64)
        self.block(buf)[...] = a
        self.host = buf
        self.dev = None

    def block(self, buf):
        return buf.reshape(self.cols + 1, self.ld).T[:self.rows, :self.cols]

    @property
    def a(self):
        return self.block(self.host)

    def put(self, ctx):
        self.dev = ctx.put(self.host)
        return self.dev

    def get(self, ctx):
        """The matrix now on the device, after asserting that nothing outside
        it changed."""
        now = ctx.get(self.dev, self.host.size)
        mask = np.ones(self.host.size, bool)
        self.block(mask)[...] = False
        assert same_bits(now[mask], self.host[mask]), f"{self.name}: written outside its {self.rows} x {self.cols}"
        return self.block(now).copy()


def vec(ctx, v, extra=8, seed=0):
    """A device vector followed by `extra` sentinel doubles; returns (pointer,
    reader): reader() gives the vector after asserting the tail is untouched."""
    v = np.asarray(v, dtype=np.float64).ravel()
    host = np.concatenate([v, sentinel(extra, seed)])
    p = ctx.put(host)

    def read():
        now = ctx.get(p, host.size)
        assert same_bits(now[v.size:], host[v.size:]), "tail written"
        return now[:v.size]

    return p, read


def lds(n, count, shift=0):
    """`count` pairwise different leading dimensions > n (odd and even)."""
    return [n + 1 + shift + k for k in range(count)]


# ------------------------------------------------------------------ Cholesky tangent
def phi(X):
    return np.tril(X, -1) + 0.5 * np.diag(np.diag(X))


def inv_lower(L):
    """L^{-1} of a lower-triangular L by forward substitution, in L's dtype."""
    n = L.shape[0]
    W = np.zeros_like(L)
    for i in range(n):
        r = -(L[i, :i] @ W[:i, :i]) if i else np.zeros(0, dtype=L.dtype)
        W[i, :i] = r / L[i, i]
        W[i, i] = 1 / L[i, i]
    return W


def chol_tangent_fwd_ref(L, Ad, dtype=LD):
    """W = L^{-1}, Y = W A' W^T, P = Phi(Y), L' = L P."""
    L, Ad = np.tril(L).astype(dtype), Ad.astype(dtype)
    if dtype is LD:
        W = inv_lower(L)
    else:
        from scipy.linalg import solve_triangular
        W = np.tril(solve_triangular(L, np.eye(L.shape[0]), lower=True))
    Y = W @ Ad @ W.T
    P = phi(Y)
    return W, Y, P, L @ P


def chol_tangent_rev_ref(L, W, Y, P, Ldbar):
    """The increments of Ladj (lower) and A'adj for a lower L'bar."""
    dtype = W.dtype
    L = np.tril(L).astype(dtype)
    T = np.tril(Ldbar).astype(dtype)
    Pbar = np.tril(L.T @ T)
    S = phi(Pbar) + phi(Pbar).T
    WtS = W.T @ S
    return np.tril(T @ P.T) - np.tril(WtS @ Y), 0.5 * (WtS @ W)


def chol_tangent_inputs(n):
    """A = B B^T / n + I (condition number about 2.2), L = chol(A), A' = R +
    R^T, L'bar = tril(R2)."""
    rng = np.random.default_rng(4000 + n)
    B = rng.uniform(-1.0, 1.0, (n, n))
    A = B @ B.T / n + np.eye(n)
    A = 0.5 * (A + A.T)
    R = rng.uniform(-1.0, 1.0, (n, n))
    return A, np.linalg.cholesky(A), R + R.T, np.tril(rng.uniform(-1.0, 1.0, (n, n)))


@functools.lru_cache(maxsize=None)
def chol_tangent_case(n, dtype_name=None):
    """Inputs and the six reference quantities (W, Y, P, L', dLadj, dA'adj) as
    float64 arrays: longdouble arithmetic for n <= 200, float64 BLAS above."""
    A, L, Ad, Ldbar = chol_tangent_inputs(n)
    dtype = {None: LD if n <= 200 else np.float64, "ld": LD, "f64": np.float64}[dtype_name]
    W, Y, P, Ld = chol_tangent_fwd_ref(L, Ad, dtype)
    dL, dA = chol_tangent_rev_ref(L, W, Y, P, Ldbar)
    ref = {k: np.asarray(v, dtype=np.float64) for k, v in
           dict(W=W, Y=Y, P=P, Ld=Ld, dLadj=dL, dAadj=dA).items()}
    for v in ref.values():
        v.setflags(write=False)
    return A, L, Ad, Ldbar, ref


# ------------------------------------------------------------------ gp_exp_quad_cov tangent
def gp_tangent_fwd_ref(x, sigma, l, ds, dl):
    x = x.astype(LD)
    d2 = (x[:, None] - x[None, :]) ** 2
    e = np.exp(-d2 / (2 * LD(l) ** 2))
    Kd = 2 * LD(sigma) * LD(ds) * e + LD(sigma) ** 2 * LD(dl) * d2 * e / LD(l) ** 3
    Kd[np.diag_indices_from(Kd)] = 2 * LD(sigma) * LD(ds)
    return Kd


def gp_tangent_rev_ref(x, sigma, l, ds, dl, Kdadj):
    """(the out4 increment, the sum of its terms' absolute values) -- the
    diagonal contributes to S_e only."""
    x, A = x.astype(LD), Kdadj.astype(LD)
    s, l, ds, dl = LD(sigma), LD(l), LD(ds), LD(dl)
    d2 = (x[:, None] - x[None, :]) ** 2
    e = np.exp(-d2 / (2 * l ** 2))
    off = ~np.eye(len(x), dtype=bool)

    def sums(M):
        return M.sum(), (M * d2)[off].sum(), (M * d2 * d2)[off].sum()

    def out(Se, S2, S4, ab=lambda v: v):
        return np.array([ab(2 * ds) * Se + ab(2 * s * dl) * S2 / l ** 3,
                         ab(2 * s * ds) * S2 / l ** 3 + ab(s * s * dl) * (S4 / l ** 6 + ab(LD(-3)) * S2 / l ** 4),
                         2 * s * Se, s * s * S2 / l ** 3], dtype=LD)

    return out(*sums(A * e)), out(*sums(np.abs(A) * e), ab=np.abs)


# ------------------------------------------------------------------ log_sum_exp / GLM tangents
def lse_tangent_ref(x, xd):
    """(lse, t, p): the softmax p in longdouble."""
    x, xd = x.astype(LD), xd.astype(LD)
    m = x.max()
    s = np.exp(x - m).sum()
    lse = m + np.log(s)
    p = np.exp(x - lse)
    return lse, (p * xd).sum(), p


def glm_theta_derivative_ref(y, theta):
    """The reference's theta_derivative d of bernoulli_logit_glm_lpmf, branch by
    branch as written (cutoff 20), and dd = d d / d theta of that expression."""
    s = (2 * y - 1).astype(LD)
    yt = s * theta.astype(LD)
    e = np.exp(-yt)
    d = np.where(yt > 20, -e, np.where(yt < -20, s, s * e / (1 + e)))
    dd = np.where(yt > 20, s * e, np.where(yt < -20, LD(0), -e / (1 + e) ** 2))
    return d, dd


# ------------------------------------------------------------------ LU
def apply_swaps(A, piv):
    """P A for LAPACK-style sequential row swaps (0-based)."""
    PA = A.copy()
    for k, p in enumerate(piv):
        if p != k:
            PA[[k, p]] = PA[[p, k]]
    return PA
