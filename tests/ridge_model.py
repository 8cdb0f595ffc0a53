"""Host model of SPEC §31.1, the pinned-order ridge solve, in numpy: every product and every difference is one binary64 operation
(numpy has no fma), every entry's updates come in ascending k. Right-looking, one column at a time — each entry of the trailing
matrix takes column k's product before column k + 1's, which is the order of §31.1's chains whatever the blocking — and the two
substitutions as column sweeps (ascending forward, descending backward). scg_ridge_solve reproduces every bit."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

PANEL = 256         # factor() updates the trailing matrix by column panels of this width (no entry's operations depend on it)


def system(A, mu: float, lam) -> np.ndarray:
    """M of §31.1 as a full symmetric float64 matrix: the lower triangle of A widened, its diagonal plus mu * lam (one product, one
    sum), mirrored. What the upper triangle of A holds is not read."""
    M = np.tril(np.asarray(A, np.float32)).astype(np.float64)
    M = M + np.tril(M, -1).T
    M[np.diag_indices_from(M)] = np.diagonal(M) + float(mu) * np.asarray(lam, np.float64)
    return M


def factor(M):
    """(L, info): §31.1's Cholesky factor of the symmetric float64 M (only its lower triangle matters), float64 lower triangular,
    and 0 — or j + 1 where column j's pivot failed !(t > 0), NaN included: L then holds the columns before j, the rest is 0."""
    M = np.array(M, np.float64)
    F = M.shape[0]
    L = np.zeros((F, F), np.float64)
    with np.errstate(all="ignore"):
        for k in range(F):
            t = M[k, k]
            if not (t > 0):
                return L, k + 1
            d = np.sqrt(t)
            L[k, k] = d
            col = M[k + 1:, k] / d
            L[k + 1:, k] = col
            for c0 in range((k + 1) // PANEL * PANEL, F, PANEL):       # the trailing matrix by column panels, each from its
                lo = max(k + 1, c0)                                     # first row on or below the diagonal down: the entries
                M[lo:, lo:c0 + PANEL] -= np.multiply.outer(col[lo - k - 1:], col[lo - k - 1:c0 + PANEL - k - 1])   # above are never read
    return L, 0


def substitute(L, b) -> np.ndarray:
    """x with L L^T x = double(b): z by the forward substitution (each row's terms in ascending k), x by the backward one (descending
    from F - 1), as column sweeps."""
    t = np.asarray(b).astype(np.float64)                       # (a copy; binary32 widens exactly)
    F = len(t)
    with np.errstate(all="ignore"):
        for k in range(F):
            t[k] = t[k] / L[k, k]
            t[k + 1:] -= L[k + 1:, k] * t[k]
        for k in range(F - 1, -1, -1):
            t[k] = t[k] / L[k, k]
            t[:k] -= L[k, :k] * t[k]
    return t


def ridge_solve(A, B, lam, mu, skip=None):
    """scg_ridge_solve on the host: A float32 [n_mat][F][F], B float32 [n_mat][n_rhs][F] or [n_mat][F], lam float64 [F], mu [n_mat],
    skip [n_mat] or None. Returns (Delta float64 of B's shape, L float64 [n_mat][F][F] with zeros above the diagonal — and all zeros
    for a skipped matrix —, info int32 [n_mat]). A skipped or failed matrix has Delta = +0."""
    A, B = np.asarray(A), np.asarray(B)
    n_mat, F = A.shape[0], A.shape[1]
    Bv = B.reshape(n_mat, -1, F)
    delta = np.zeros(Bv.shape, np.float64)
    L = np.zeros((n_mat, F, F), np.float64)
    info = np.zeros(n_mat, np.int32)
    def one(g):
        L[g], info[g] = factor(system(A[g], mu[g], lam))
        if info[g] == 0:
            for c in range(Bv.shape[1]):
                delta[g, c] = substitute(L[g], Bv[g, c])

    todo = [g for g in range(n_mat) if skip is None or not skip[g]]
    with ThreadPoolExecutor(max_workers=8) as pool:            # (the matrices are independent; numpy's loops release the lock)
        list(pool.map(one, todo))
    return delta.reshape(B.shape), L, info


def ridge_solve_like_valuefit(A, b, n, ridge: float, scale) -> np.ndarray:
    """valuefit.ridge_solve's arguments and meaning (A [n_act][F][F], b [n_act][F], counts n, `scale` [F]) on the model: what
    valuefit.ridge_solve_pinned computes, by bits. A failed pivot raises ValueError."""
    n = np.asarray(n, np.int64).reshape(-1)
    lam = 1.0 / np.asarray(scale, np.float64) ** 2
    mu = [float(ridge) * max(int(v), 1) for v in n]
    delta, _, info = ridge_solve(np.asarray(A, np.float32), np.asarray(b, np.float32), lam, mu, skip=n == 0)
    if info.any():
        raise ValueError(f"not positive definite: info = {info.tolist()}")
    return delta


def backward_error(M, x, b) -> float:
    """eta = ||M x - b||_inf / (||M||_inf ||x||_inf + ||b||_inf), the residual in float64."""
    M, x, b = (np.asarray(v, np.float64) for v in (M, x, b))
    den = np.abs(M).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()
    return float(np.abs(M @ x - b).max() / den) if den > 0 else 0.0
