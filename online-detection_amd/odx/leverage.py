"""Ridge leverage scores and Nystroem centres sampled by them (FALKON-BLESS: Rudi, Calandriello, Carratino, Rosasco,
NeurIPS 2018, "On fast leverage score sampling and optimal learning").

For a dictionary J of rows of X with positive weights c, all f64 (radial kernels: k(x, x) = 1):

    A = K_JJ + lam diag(c),   L = chol(A),   q(x) = k_xJ A^-1 k_Jx = |L^-1 k_Jx|^2,   l(x) = (1 - q(x)) / (lam n).

With J = all rows and c = n this is the ridge leverage score (K (K + lam n I)^-1)_ii exactly; a uniform subset of m rows takes
c = m.  sum_i l_i is the effective dimension d_eff(lam): how many centres a fit needs at all.

The kernel entries k_xJ are the f32 K_nM block the fits use (any of the three radial kernels, `backend.knm`), built a chunk of
rows at a time; A, its factor and the inverse factor are f64 (`kmm_f64`, `chol_inverse`), and q is summed in f64 from the f32
entries by one kernel that never stores the n x |J| product (`row_quad`: odx_knm_rowquad_f64).  A chunked call gives the bits of
the unchunked one.  DESIGN.md, section 2, has the error model.
"""
import math

import torch

from . import backend as _backend
from .falkon import _kernel_arg

TINY = torch.finfo(torch.float64).tiny
BLOCK_BYTES = 1 << 30          # the f32 block of one chunk of rows (leverage_scores' default chunk_rows)


def _karg(kernel):
    """What the backend takes for `kernel`: a kernel object's sigma (Gaussian) or the object (Matern), or a plain width."""
    return _kernel_arg(kernel) if hasattr(kernel, "sigma") else float(kernel)


def _features(be, X):
    return X if (hasattr(X, "n") and hasattr(X, "D") and not torch.is_tensor(X)) else be.features(X)


def _f32_rows(be, F):
    return be.f32(F) if hasattr(be, "f32") else F


def _block(be, F, Zf, karg, route_rows):
    """The f32-format block of a chunk of rows, built by the route a block of route_rows rows takes (HipBackend.knm_f32);
    a backend without formats (the tests' CPU one) has one build."""
    if hasattr(be, "knm_f32"):
        return be.knm_f32(F, Zf, karg, route_rows)
    return be.knm(F, Zf, karg)


def leverage_scores(X, centres, kernel, penalty, weights=None, n_total=None, chunk_rows=None, return_q=False, backend=None):
    """The approximate ridge leverage scores (1 - q) / (penalty n_total) of every row of X for the dictionary `centres`, as an
    (n,) f64 tensor on the backend's device.

    X, centres: (n, D) and (|J|, D) rows (tensors, arrays or a backend's Features).  kernel: a GaussianKernel / MaternKernel, or
    a Gaussian width.  weights: c, one positive number per centre (default |J| for every centre: a uniform subset).  n_total:
    the n of the formula (default: the rows of X).  The f32 K block is built chunk_rows rows at a time (default: as many as a
    1 GiB block holds) in f32 format whatever the storage option says; chunking does not change a bit of the result.
    return_q: also return q."""
    be = backend if backend is not None else _backend.get_backend()
    F, Zf = _f32_rows(be, _features(be, X)), _f32_rows(be, _features(be, centres))
    n, M = F.n, Zf.n
    penalty = float(penalty)
    if not penalty > 0.0:
        raise ValueError("leverage_scores: penalty must be positive, got %r" % (penalty,))
    n_total = n if n_total is None else int(n_total)
    karg = _karg(kernel)
    q = torch.zeros(n, dtype=torch.float64, device=be.device)
    if M > 0 and n > 0:
        if weights is None:
            A = be.kmm_f64(Zf, karg, None, penalty * M)
        else:
            w = torch.as_tensor(weights, dtype=torch.float64).reshape(-1)
            if w.numel() != M or not bool((w > 0).all()):
                raise ValueError("leverage_scores: weights must be %d positive numbers" % M)
            A = be.kmm_f64(Zf, karg, w, penalty)
        Li, _ = be.chol_inverse(A)
        if chunk_rows is None:
            chunk_rows = max(128, BLOCK_BYTES // (4 * ((M + 3) // 4 * 4)) // 128 * 128)
        chunk_rows = max(1, int(chunk_rows))
        if chunk_rows >= n:
            be.row_quad(_block(be, F, Zf, karg, n), Li, out=q)
        else:
            if hasattr(be, "share_split"):
                be.share_split(F, Zf, karg)          # (the chunks then carry the split of ALL rows, as the whole block does)
            for lo in range(0, n, chunk_rows):
                hi = min(n, lo + chunk_rows)
                Fc = be.rows(F, torch.arange(lo, hi))
                be.row_quad(_block(be, Fc, Zf, karg, n), Li, out=q[lo:hi])
    scores = (1.0 - q) / (penalty * n_total)
    return (scores, q) if return_q else scores


class LeverageSelector:
    """Nystroem centres drawn by approximate ridge leverage scores, bottom-up over a ladder of penalties (BLESS):

        H = max(1, ceil(log(1 / penalty) / log q)),  lam_h = q^-h for h < H,  lam_H = penalty,  J_0 = {}
        level h:  R = min(n, ceil(q1 / lam_h));  U = the first R entries of a permutation of the rows;
                  l_u = max(tiny, (1 - q_u) / (lam_h n)) with q_u from (J_{h-1}, c_{h-1}) at lam_h (0 while J is empty);
                  p = l / sum l;  d = (n / R) sum l;  M_h = min(M, max(1, ceil(q2 d)));
                  M_h draws from U by the inverse CDF of p, with replacement; a row drawn cnt times enters J_h once with
                  c_j = R M_h p_j / cnt.

    ``select(X, Y)`` has CenterSelector's contract (the chosen rows, or (rows, Y[idx])), so
    ``InCoreFalkon(center_selection=LeverageSelector(...))`` needs nothing else.  M caps the centres of every level (None: no
    cap).  Every draw comes from a private CPU generator seeded with `seed`: the global RNG is untouched, and two calls give the
    same centres.  The permutation, the CDF and the draws are f64 on the host (one copy of p per level).

    After select: indices_ (|J|,) int64, weights_ (|J|,) f64, d_eff_ (the last level's estimate of d_eff(penalty)), levels_ (a
    list of (lam_h, R, d, M_h, |J_h|)) and the last level's candidates_, scores_ (their l, before the floor), prev_indices_,
    prev_weights_ (the dictionary those scores came from).

    The fit does not use weights_: FALKON's preconditioner is the uniform-sampling one.  A preconditioner that takes the
    sampling weights (the paper's FALKON-BLESS) is a later change."""

    def __init__(self, kernel, penalty, M=None, q=2.0, q1=2.0, q2=2.0, seed=0, chunk_rows=None, backend=None):
        self.kernel, self.penalty, self.M = kernel, float(penalty), M
        self.q, self.q1, self.q2, self.seed = float(q), float(q1), float(q2), int(seed)
        self.chunk_rows, self.backend = chunk_rows, backend
        if not self.penalty > 0.0 or not self.q > 1.0 or not self.q1 > 0.0 or not self.q2 > 0.0:
            raise ValueError("LeverageSelector: needs penalty > 0, q > 1, q1 > 0, q2 > 0")
        if M is not None and int(M) < 1:
            raise ValueError("LeverageSelector: the cap M must be at least 1")
        self.indices_ = self.weights_ = self.d_eff_ = self.levels_ = None
        self.candidates_ = self.scores_ = self.prev_indices_ = self.prev_weights_ = None

    def ladder(self):
        """[lam_1, ..., lam_H]."""
        H = max(1, int(math.ceil(math.log(1.0 / self.penalty) / math.log(self.q))))
        return [self.q ** -h for h in range(1, H)] + [self.penalty]

    def sample(self, X):
        """Run the sampler on the rows X; fills and returns indices_ (host int64)."""
        be = self.backend if self.backend is not None else _backend.get_backend()
        F = _f32_rows(be, _features(be, X))
        n = F.n
        if n < 1:
            raise ValueError("LeverageSelector: no rows")
        gen = torch.Generator(device="cpu")
        gen.manual_seed(self.seed)
        cap = n if self.M is None else int(self.M)
        J = torch.zeros(0, dtype=torch.int64)
        c = torch.zeros(0, dtype=torch.float64)
        self.levels_ = []
        for lam_h in self.ladder():
            R = min(n, int(math.ceil(self.q1 / lam_h)))
            U = torch.randperm(n, generator=gen)[:R]
            if J.numel():
                ell = leverage_scores(be.rows(F, U), be.rows(F, J), self.kernel, lam_h, weights=c, n_total=n,
                                      chunk_rows=self.chunk_rows, backend=be).cpu()
            else:
                ell = torch.full((R,), 1.0 / (lam_h * n), dtype=torch.float64)
            self.candidates_, self.scores_, self.prev_indices_, self.prev_weights_ = U, ell, J, c
            ell = ell.clamp_min(TINY)
            tot = ell.sum()
            p = ell / tot
            d = float(n) / R * float(tot)
            Mh = min(cap, max(1, int(math.ceil(self.q2 * d))))
            u = torch.rand(Mh, generator=gen, dtype=torch.float64)
            pos = torch.searchsorted(torch.cumsum(p, 0), u, right=True).clamp_max(R - 1)
            uniq, cnt = torch.unique(pos, return_counts=True)          # (sorted by position in U)
            J = U[uniq]
            c = R * Mh * p[uniq] / cnt.to(torch.float64)
            self.levels_.append((lam_h, R, d, Mh, int(J.numel())))
        self.indices_, self.weights_, self.d_eff_ = J, c, self.levels_[-1][2]
        return J

    def select(self, X, Y):
        idx = self.sample(X)
        if not torch.is_tensor(X):
            X = torch.as_tensor(X)
        picked = X[idx.to(X.device)]
        if Y is None:
            return picked
        if not torch.is_tensor(Y):
            Y = torch.as_tensor(Y)
        return picked, Y[idx.to(Y.device)]
