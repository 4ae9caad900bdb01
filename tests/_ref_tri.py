"""Plain substitution in np.longdouble for op(tri(A))^{-1} B, and what the
triangular-solve tests (test_tri_solve_kernels.py) derive from it: C, adjB and
adjA of mdivide_left_tri, and w, sd and lp of multi_normal_cholesky_lpdf.

Only the named triangle of A is looked at: the other one may hold anything
(the tests put NaN there).  Nothing here touches the device.
"""
import numpy as np

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))

# the pieces of the two n = 512 shapes that are compared in longdouble
COLS_512 = (0, 1, 63, 64, 255, 256, 510, 511)


def rows_512(m):
    return (0, 511, 512, 1023, 1024, m - 1)


def tri_of(A, lower):
    """The named triangle of A with zeros in the other one (A's dtype)."""
    i, j = np.indices(A.shape)
    return np.where(i >= j if lower else i <= j, A, 0)


def tri_solve_ld(A, B, lower, trans):
    """X with op(tri(A)) X = B by substitution in longdouble, op = transpose
    for trans; A's other triangle is never read."""
    m = A.shape[0]
    T = tri_of(np.asarray(A), lower).astype(LD)
    M = T.T if trans else T
    X = np.array(B, dtype=LD).reshape(m, -1)
    if bool(lower) != bool(trans):  # op(tri(A)) is lower: forward
        for i in range(m):
            if i:
                X[i] -= M[i, :i] @ X[:i]
            X[i] /= M[i, i]
    else:
        for i in range(m - 1, -1, -1):
            if i < m - 1:
                X[i] -= M[i, i + 1:] @ X[i + 1:]
            X[i] /= M[i, i]
    return X


def mdivide_ref(A, B, Cadj, lower, pieces=False):
    """C = tri(A)^{-1} B, adjB = tri(A)^{-T} Cadj, adjA = -tri(adjB C^T) in
    longdouble.  pieces: the columns COLS_512 of C and adjB and the rows
    rows_512(m) of adjA only (each row is on its triangle, zero elsewhere):
        adjB[i, :] = (tri(A)^{-1} e_i)^T Cadj,
        adjA[i, :]^T = -tri(A)^{-1} (B adjB[i, :]^T),
    so that no full n-column solve is needed."""
    m = A.shape[0]
    if not pieces:
        C = tri_solve_ld(A, B, lower, 0)
        adjB = tri_solve_ld(A, Cadj, lower, 1)
        return C, adjB, -tri_of(adjB @ C.T, lower)
    cols, rows = list(COLS_512), list(rows_512(m))
    C = tri_solve_ld(A, B[:, cols], lower, 0)
    adjB = tri_solve_ld(A, Cadj[:, cols], lower, 1)
    E = np.zeros((m, len(rows)))
    E[rows, range(len(rows))] = 1.0
    adjB_rows = tri_solve_ld(A, E, lower, 0).T @ Cadj.astype(LD)      # len(rows) x n
    adjA_rows = -tri_solve_ld(A, B.astype(LD) @ adjB_rows.T, lower, 0).T  # len(rows) x m
    j = np.arange(m)
    for k, i in enumerate(rows):
        adjA_rows[k, (j > i) if lower else (j < i)] = 0
    return C, adjB, adjA_rows


def mvn_ref(L, y, mu):
    """w = L^{-1} (y - mu), sd = L^{-T} w, lp = -0.5 w.w - sum log diag L -
    0.5 N log(2 pi), in longdouble (mu = None: zero)."""
    n = L.shape[0]
    res = np.asarray(y, dtype=LD) - (0 if mu is None else np.asarray(mu, dtype=LD))
    w = tri_solve_ld(L, res, 1, 0)[:, 0]
    sd = tri_solve_ld(L, w, 1, 1)[:, 0]
    lp = -LD(0.5) * (w @ w) - np.log(np.diag(L).astype(LD)).sum() - LD(0.5) * n * np.log(2 * PI)
    return w, sd, lp


def spd_inputs(m, n):
    """S S^T / m + I with S uniform(-1, 1), its numpy Cholesky factor T, and
    uniform(-1, 1) B, Cadj (m x n), Aadj0 (m x m), Badj0 (m x n); seeded from
    (m, n)."""
    rng = np.random.default_rng([m, n])
    S = rng.uniform(-1.0, 1.0, (m, m))
    A = S @ S.T / m + np.eye(m)
    A = 0.5 * (A + A.T)
    return (A, np.linalg.cholesky(A), rng.uniform(-1, 1, (m, n)), rng.uniform(-1, 1, (m, n)),
            rng.uniform(-1, 1, (m, m)), rng.uniform(-1, 1, (m, n)))


def relerr(got, ref):
    """max |got - ref| / max |ref| (inf when got is not finite)."""
    got = np.asarray(got, dtype=LD)
    if not np.all(np.isfinite(got)):
        return np.inf
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(got - ref).max() / np.abs(ref).max())
