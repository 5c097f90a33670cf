"""The f64 numpy statement of odx/leverage.py — TEST ORACLE ONLY.

For a dictionary Z (rows) with weights c:  A = K_ZZ + lam diag(c),  L = chol(A),  Li = L^-1,  q(x) = |Li k_Zx|^2,
l(x) = (1 - q(x)) / (lam n).  Kernels come through tests/matern_ref.radial_kernel (a width, or an object with .sigma and,
for a Matern kernel, .nu), always evaluated in f64.
"""
import math

import numpy as np
import scipy.linalg as sla

from tests.matern_ref import radial_kernel

TINY = np.finfo(np.float64).tiny


def _k(kernel):
    if getattr(kernel, "nu", None) is not None:
        return kernel
    return float(getattr(kernel, "sigma", kernel))


def kernel_matrix(X1, X2, kernel):
    return radial_kernel(np.asarray(X1, dtype=np.float64), np.asarray(X2, dtype=np.float64), _k(kernel), np.float64)


def dictionary_matrix(Z, kernel, lam, weights=None):
    m = len(Z)
    c = np.full(m, float(m)) if weights is None else np.asarray(weights, dtype=np.float64)
    return kernel_matrix(Z, Z, kernel) + lam * np.diag(c)


def inverse_factor(A):
    L = np.linalg.cholesky(A)
    return sla.solve_triangular(L, np.eye(len(A)), lower=True)


def row_quad(K, Li):
    """q[r] = sum_j (sum_{c <= j} K[r, c] Li[j, c])^2."""
    T = np.asarray(K, dtype=np.float64) @ np.tril(Li).T
    return (T * T).sum(1)


def approx_scores(X, Z, kernel, lam, weights=None, n_total=None, return_q=False):
    n_total = len(X) if n_total is None else n_total
    if len(Z) == 0:
        q = np.zeros(len(X))
    else:
        q = row_quad(kernel_matrix(X, Z, kernel), inverse_factor(dictionary_matrix(Z, kernel, lam, weights)))
    s = (1.0 - q) / (lam * n_total)
    return (s, q) if return_q else s


def exact_scores(X, kernel, lam):
    """diag(K (K + lam n I)^-1), by the dense inverse."""
    n = len(X)
    K = kernel_matrix(X, X, kernel)
    return np.einsum("ij,ji->i", K, np.linalg.inv(K + lam * n * np.eye(n)))


class TorchDraws:
    """The draws of odx.LeverageSelector for a seed: per level one permutation, then the uniforms."""

    def __init__(self, seed):
        import torch
        self.torch = torch
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(int(seed))

    def perm(self, n):
        return self.torch.randperm(n, generator=self.gen).numpy()

    def uniform(self, m):
        return self.torch.rand(m, generator=self.gen, dtype=self.torch.float64).numpy()


def bottom_up(X, kernel, lam, draws, q=2.0, q1=2.0, q2=2.0, cap=None, merge_counts=True, scale_rm=True):
    """The bottom-up sampler.  draws: an object with perm(n) and uniform(m) (TorchDraws).  merge_counts / scale_rm: False
    drops the division by cnt / the factor R M_h of the weights (to see by hand that the quality bands notice).
    Returns a dict: indices, weights, d_eff, levels [(lam_h, R, d, M_h, |J_h|)], candidates, scores, prev_indices, prev_weights."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    cap = n if cap is None else int(cap)
    H = max(1, int(math.ceil(math.log(1.0 / lam) / math.log(q))))
    lams = [q ** -h for h in range(1, H)] + [lam]
    J, c = np.zeros(0, dtype=np.int64), np.zeros(0)
    out = {"levels": []}
    for lam_h in lams:
        R = min(n, int(math.ceil(q1 / lam_h)))
        U = np.asarray(draws.perm(n))[:R]
        ell = approx_scores(X[U], X[J], kernel, lam_h, c, n)
        out.update(candidates=U, scores=ell, prev_indices=J, prev_weights=c)
        ell = np.maximum(ell, TINY)
        tot = ell.sum()
        p = ell / tot
        d = float(n) / R * float(tot)
        Mh = min(cap, max(1, int(math.ceil(q2 * d))))
        u = np.asarray(draws.uniform(Mh))
        pos = np.minimum(np.searchsorted(np.cumsum(p), u, side="right"), R - 1)
        uniq, cnt = np.unique(pos, return_counts=True)
        J = U[uniq]
        c = p[uniq] * (R * Mh if scale_rm else 1.0) / (cnt if merge_counts else 1.0)
        out["levels"].append((lam_h, R, d, Mh, len(J)))
    out.update(indices=J, weights=c, d_eff=out["levels"][-1][2])
    return out
