"""The sample-weighted FALKON fit (odx/weighted.py) in numpy f64 — TEST ORACLE ONLY — built on oracle/falkon_ref's
conjugate_gradient and tests/matern_ref's kernels, and a dense solve of the same normal equations as the independent check.

Objective over f = K alpha: (1 / n) sum_i w_i (f_i - y_i)^2 + lam alpha' (K_MM + eps M I) alpha, n = the number of rows
(falkon's convention: the weights do not change n).  Preconditioner: T = chol_upper(K_MM + eps M I),
A = chol_upper(T diag(w_Z) T' / M + lam I) with w_Z the weights of the centres, as falkon's weighted preconditioner."""
import numpy as np
import scipy.linalg as sla

from oracle import falkon_ref as fr
from tests.matern_ref import radial_kernel


def _solve(U, v, trans):
    return sla.solve_triangular(U, v, lower=False, trans=trans, check_finite=False)


def weighted_fit(X, y, w, Z, w_Z, kernel, lam, maxiter, pc_eps=1e-5, cg_epsilon=1e-7, knm=None):
    """alpha (M, 1) f64.  kernel: a Gaussian's width or a kernel object (tests/matern_ref.radial_kernel).  knm: the stored
    block to iterate on instead of the f64 kernel of (X, Z) — the oracle then states what the SOLVER must produce on it."""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    y, w, wZ = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (y, w, w_Z))
    n, M = X.shape[0], Z.shape[0]
    K = np.asarray(knm, dtype=np.float64) if knm is not None else radial_kernel(X, Z, kernel, np.float64)
    assert K.shape == (n, M) and w.shape == (n,) and wZ.shape == (M,)
    C = radial_kernel(Z, Z, kernel, np.float64)
    C[np.diag_indices(M)] += pc_eps * M
    T = sla.cholesky(C, lower=False, check_finite=False)          # T' T = K_MM + eps M I
    AA = (T * wZ[None, :]) @ T.T / M
    AA[np.diag_indices(M)] += lam
    A = sla.cholesky(AA, lower=False, check_finite=False)         # A' A = T diag(w_Z) T' / M + lam I
    b = _solve(A, _solve(T, K.T @ (w * y / n), 1), 1)

    def mmv(S):
        v = _solve(A, S, 0)
        cc = K.T @ (w[:, None] * (K @ _solve(T, v, 0))) / n
        return _solve(A, _solve(T, cc, 1) + lam * v, 1)

    beta = fr.conjugate_gradient(b[:, None], mmv, maxiter, np.float64, cg_epsilon)
    return _solve(T, _solve(A, beta, 0), 0)


def dense_weighted(K, Kmm, y, w, lam, pc_eps):
    """The solution alpha (M, 1) of (K' W K / n + lam (K_MM + eps M I)) alpha = K' W y / n by a direct f64 solve."""
    K, Kmm = np.asarray(K, dtype=np.float64), np.asarray(Kmm, dtype=np.float64)
    y, w = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1)
    n, M = K.shape
    H = K.T @ (w[:, None] * K) / n + lam * (Kmm + pc_eps * M * np.eye(M))
    return np.linalg.lstsq(H, K.T @ (w * y) / n, rcond=None)[0][:, None]
