"""The logistic FALKON fit (odx/logistic.py) in numpy f64 — TEST ORACLE ONLY — built on oracle/falkon_ref's kernel,
conjugate_gradient and triangular solves, and a dense Newton solve of the same M-dimensional objective as the independent check.

Labels y in {-1, +1}; l(y, t) = c(y) log(1 + exp(-y t)), c(+1) = 1, c(-1) = neg_weight; with s = 1 / (1 + exp(y t)):
l' = -c y s, l'' = c s (1 - s).  Objective over f = K alpha: (1 / n) sum l(y_i, f_i) + (lam / 2) alpha' (K_MM + eps M I) alpha."""
import numpy as np
import scipy.linalg as sla
from scipy.special import expit

from oracle import falkon_ref as fr


def loss_terms(y, t, neg_weight):
    """(l', l'', l) per row, f64."""
    y, t = np.asarray(y, dtype=np.float64), np.asarray(t, dtype=np.float64)
    c = np.where(y > 0, 1.0, float(neg_weight))
    z = y * t
    s, s1 = expit(-z), expit(z)
    # (scipy's expit returns 0 where the value is subnormal, |z| > 708.4; there 1 + exp(-|z|) is 1 to the last bit and the
    # value is exp(-|z|) itself, which numpy's exp rounds correctly into the subnormals)
    s, s1 = np.where(z > 700.0, np.exp(-np.abs(z)), s), np.where(z < -700.0, np.exp(-np.abs(z)), s1)
    return -c * y * s, c * s * s1, c * np.logaddexp(0.0, -z)


def _solve(U, v, trans):
    return sla.solve_triangular(U, v, lower=False, trans=trans, check_finite=False)


def logistic_fit(X, y, Z, y_centres, sigma, penalties, iters, neg_weight=1.0, pc_eps=1e-5, cg_epsilon=1e-7, cg_tolerance=fr.CG_TOLERANCE,
                 full_gradient_every=fr.CG_FULL_GRADIENT_EVERY, knm=None, kernel=None, objective_out=None):
    """alpha (M, 1) f64 of the schedule zip(penalties, iters).  knm: the stored block to iterate on instead of the f64 kernel
    of (X, Z) — the oracle then states what the SOLVER must produce on that block.  kernel: f(X1, X2, sigma, dtype) in the place
    of fr.gaussian_kernel.  objective_out: a list that receives the objective before every step and behind the last."""
    kern = kernel or fr.gaussian_kernel
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    y, yM = np.asarray(y, dtype=np.float64).reshape(-1), np.asarray(y_centres, dtype=np.float64).reshape(-1)
    n, M = X.shape[0], Z.shape[0]
    K = np.asarray(knm, dtype=np.float64) if knm is not None else kern(X, Z, sigma, np.float64)
    assert K.shape == (n, M)
    C = kern(Z, Z, sigma, np.float64)
    C[np.diag_indices(M)] += pc_eps * M
    T = sla.cholesky(C, lower=False, check_finite=False)          # T' T = K_MM + eps M I
    beta, alpha, f = np.zeros(M), np.zeros(M), np.zeros(n)

    def objective(lam):
        return float(loss_terms(y, f, neg_weight)[2].sum()) / n + 0.5 * lam * float(beta @ beta)

    for lam, m in zip(penalties, iters):
        wM = loss_terms(yM, T.T @ beta, neg_weight)[1]
        AA = (T * wM[None, :]) @ T.T / M
        AA[np.diag_indices(M)] += lam
        A = sla.cholesky(AA, lower=False, check_finite=False)
        g, d, _ = loss_terms(y, f, neg_weight)
        if objective_out is not None:
            objective_out.append(objective(lam))
        b = _solve(A, _solve(T, K.T @ g / n, 1) + lam * beta, 1)

        def mmv(S):
            v = _solve(A, S, 0)
            cc = K.T @ (d[:, None] * (K @ _solve(T, v, 0))) / n
            return _solve(A, _solve(T, cc, 1) + lam * v, 1)

        s = fr.conjugate_gradient(b[:, None], mmv, m, np.float64, cg_epsilon, cg_tolerance, full_gradient_every)[:, 0]
        v = _solve(A, s, 0)
        da = _solve(T, v, 0)
        beta, alpha, f = beta - v, alpha - da, f - K @ da
    if objective_out is not None:
        objective_out.append(objective(penalties[-1]))
    return alpha[:, None]


def dense_newton(X, y, Z, sigma, lam, neg_weight=1.0, pc_eps=1e-5, kernel=None, steps=100, knm=None):
    """The minimiser alpha (M, 1) of the same objective at one penalty by undamped-then-halved dense Newton steps in f64: the
    independent check (no preconditioner, no CG, no T-coordinates)."""
    kern = kernel or fr.gaussian_kernel
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, M = X.shape[0], Z.shape[0]
    K = np.asarray(knm, dtype=np.float64) if knm is not None else kern(X, Z, sigma, np.float64)
    Q = kern(Z, Z, sigma, np.float64)
    Q[np.diag_indices(M)] += pc_eps * M

    def obj(a):
        return float(loss_terms(y, K @ a, neg_weight)[2].sum()) / n + 0.5 * lam * float(a @ Q @ a)

    a = np.zeros(M)
    for _ in range(steps):
        g, d, _ = loss_terms(y, K @ a, neg_weight)
        grad = K.T @ g / n + lam * (Q @ a)
        H = K.T @ (d[:, None] * K) / n + lam * Q
        step = np.linalg.solve(H, grad)
        t, o = 1.0, obj(a)
        while obj(a - t * step) > o and t > 1e-10:
            t *= 0.5
        a = a - t * step
        if np.linalg.norm(t * step) <= 1e-14 * max(1.0, np.linalg.norm(a)):
            break
    return a[:, None]
