"""Incremental FALKON: a model that absorbs new rows and forgets old ones without a refit.

With the centres fixed, FALKON's conjugate gradient touches the rows only through K_nM' K_nM v and K_nM' y.  So the model keeps

    G = K_nM' W K_nM  (M x M, f64),   b = K_nM' W y  (M, f64),   n = sum w

and nothing of size n: rows are added by accumulating their chunk's products into G and b (``partial_fit``), removed by the same
call with negated weights (``remove``), forgotten by a scale of all three (``decay``), and every solve runs falkon's CG schedule
with one read of G per iteration (``solver.falkon_fit_stats``) behind the preconditioner of the centres, which no row changes.
The result is the FALKON iterate of a fit on all rows the statistics hold, up to f64 rounding (the K entries are the f32 ones of
the stored-block fits; their products and sums are f64: odx_knm_gram_f64).

Nothing in G depends on the labels: a model of T outputs (``outputs=T``) keeps ONE G and T right-hand sides, summed from the same
read of each chunk (odx_knm_gram_rhsn_f64) and solved in lock step (``solver.falkon_fit_stats_multi``); and nothing in G, b or T's
factors depends on the penalty: ``solve_path`` fits a lambda path from the same statistics (``solver.falkon_fit_stats_path``).
"""
import math

import torch

from . import backend as _backend
from .falkon import Falkon, GaussianKernel, MaternKernel, _FalkonBase, _kernel_arg
from .leverage import BLOCK_BYTES, _block, _f32_rows
from .solver import falkon_fit_stats, falkon_fit_stats_multi, falkon_fit_stats_path

_DERIVED = ("_zf", "_P")          # rebuilt from ny_points_ / penalty on the next use: not copied, not pickled


class IncrementalFalkon(_FalkonBase):
    """FALKON on M x M sufficient statistics.

    kernel: a GaussianKernel or a MaternKernel.  centres: the (M, D) Nystroem centres; None: they are selected from the rows of
    the FIRST ``partial_fit`` exactly as ``InCoreFalkon.fit`` selects them (``center_selection``, ``M``), and stay.  chunk_rows:
    rows per K block (default: as many as a 1 GiB f32 block holds); the block buffer is reused from chunk to chunk and dropped
    when the call returns.  outputs: the number T of label columns (default: one label column per model).  With T > 1 the rows
    carry a label matrix (n, T) — one-vs-rest heads over the same stream of rows and the same centres — and the model keeps one
    G and T right-hand sides.  There is ONE weight per row, shared by the outputs (``sample_weight``, negated weights and
    ``decay`` act on all of them): that sharing is what makes G shareable, and a weight per output would need T matrices G.

    After a solve: ``alpha_`` (M, 1), ``ny_points_``, ``n_seen_`` (the total weight held), ``gram_`` (M, ld) and ``rhs_`` (M,);
    with outputs = T > 1 ``alpha_`` is (M, T), ``rhs_`` (T, Mp) with Mp = M rounded up to even, and ``predict`` returns (n, T).
    ``predict`` is the other estimators'; ``as_falkon()`` hands the fitted model out as a plain ``Falkon``."""

    def __init__(self, kernel, penalty, M=None, centres=None, center_selection="uniform", maxiter=20, options=None, chunk_rows=None,
                 outputs=1):
        if not isinstance(kernel, (GaussianKernel, MaternKernel)):
            raise ValueError("IncrementalFalkon: kernel must be a GaussianKernel or a MaternKernel, got %r" % (kernel,))
        if centres is None and isinstance(center_selection, str) and M is None:
            raise ValueError("IncrementalFalkon: needs centres, or M for the uniform selection from the first rows")
        if isinstance(outputs, bool) or int(outputs) != outputs or not 1 <= int(outputs) <= 1024:
            raise ValueError("IncrementalFalkon: outputs must be an integer in 1 .. 1024, got %r" % (outputs,))
        super().__init__(kernel, penalty, M, center_selection=center_selection, maxiter=maxiter, options=options)
        self.outputs = int(outputs)
        self.centres = centres
        self.chunk_rows = chunk_rows
        self.n_seen_ = 0.0
        self.gram_ = None
        self.rhs_ = None

    # ------------------------------------------------------------------ what is derived
    def __getstate__(self):
        d = dict(self.__dict__)
        for k in _DERIVED:
            d.pop(k, None)
        return d

    def _centre_features(self, be):
        """The centres as the backend's kernel operand (row norms, packed split): the model's centre cache (_centres)."""
        return _f32_rows(be, self._centres())

    def _precond(self, be):
        """The preconditioner of (centres, kernel, penalty): built at the first use and after a change of penalty."""
        c = self.__dict__.get("_P")
        lam = float(self.penalty)
        if c is None or c[0] is not be or c[1] != lam:
            P = be.precond(self._centre_features(be), _kernel_arg(self.kernel), lam, self.options.solver_options().pc_epsilon)
            self._P = c = (be, lam, P)
        return c[2]

    # ------------------------------------------------------------------ rows in, rows out
    def _refuse(self, be, X):
        if torch.is_tensor(X) and X.dtype in _backend.B16_DTYPES and getattr(be, "native16", False):
            raise ValueError("IncrementalFalkon: 16-bit native rows are not offered (the statistics are summed from the f32 "
                             "K_nM entries); pass f32 rows or switch native16 off")
        if getattr(be, "knm_storage", None) == "stream":
            raise ValueError("IncrementalFalkon: knm_storage='stream' stores no K_nM block to take the statistics from")

    def _first(self, be, F):
        """Fix the centres: the given ones, or selected from these rows as _FalkonBase._fit selects them."""
        if self.centres is not None:
            Zf = be.features(self.centres)
        elif isinstance(self.center_selection, str):
            Zf = be.rows(F, torch.randperm(F.n)[: self.M])
        else:
            sel = self.center_selection.select(F.X, None)
            Zf = be.features(sel[0] if isinstance(sel, tuple) else sel)
        if Zf.D != F.D:
            raise ValueError("IncrementalFalkon: the rows have %d features, the centres %d" % (F.D, Zf.D))
        self.M = M = Zf.n
        self.ny_points_ = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        self._centres(Zf)
        self.gram_ = be.zeros(M * ((M + 1) // 2 * 2)).view(M, (M + 1) // 2 * 2)
        T = self.outputs
        self.rhs_ = be.zeros(M) if T == 1 else be.zeros(T * ((M + 1) // 2 * 2)).view(T, (M + 1) // 2 * 2)
        self.n_seen_ = 0.0
        self.alpha_ = None

    def _update(self, X, Y, sample_weight, decay, sign, solve):
        be = _backend.get_backend()
        self._refuse(be, X)
        decay = float(decay)
        if not (0.0 <= decay <= 1.0):
            raise ValueError("IncrementalFalkon: decay must lie in [0, 1], got %r" % (decay,))
        F = _f32_rows(be, be.features(X))
        n = F.n
        if n < 1:
            raise ValueError("IncrementalFalkon: no rows")
        y = torch.as_tensor(Y).reshape(n, -1)
        T = self.outputs
        if T == 1 and y.shape[1] != 1:
            raise ValueError("IncrementalFalkon fits one label column per model; got Y with %d columns" % y.shape[1])
        if y.shape[1] != T:
            raise ValueError("IncrementalFalkon(outputs=%d) takes Y with %d label columns; got %d" % (T, T, y.shape[1]))
        if self.ny_points_ is not None and F.D != self.ny_points_.shape[1]:
            raise ValueError("IncrementalFalkon: the rows have %d features, the centres %d" % (F.D, self.ny_points_.shape[1]))
        w = None
        if sample_weight is not None:
            sw = torch.as_tensor(sample_weight)
            if sw.dim() > 1 and sw.shape[-1] != 1 and sw.numel() != n:
                raise ValueError("IncrementalFalkon: sample_weight must hold ONE weight per row, shared by the outputs; got %r "
                                 "(a weight per output would need a G per output)" % (tuple(sw.shape),))
            w = be.vec(sw.reshape(-1))
            if w.numel() != n:
                raise ValueError("IncrementalFalkon: sample_weight must hold one weight per row (%d), got %d" % (n, w.numel()))
            total = float(w.sum())
            if sign < 0:
                w = -w
        else:
            total = float(n)
            if sign < 0:
                w = be.zeros(n) - 1.0
        seen = decay * self.n_seen_ + sign * total
        if sign < 0 and self.ny_points_ is None:
            raise ValueError("IncrementalFalkon: removing rows from a model that holds none (a total weight of %g)" % seen)
        if not seen > 0.0:          # (before G is touched: a model must keep a positive total weight to be solved)
            raise ValueError("IncrementalFalkon: %s these rows would leave a total weight of %g; nothing is changed"
                             % ("removing" if sign < 0 else "adding", seen))
        if self.ny_points_ is None:
            self._first(be, F)
        Zf, karg, M = self._centre_features(be), _kernel_arg(self.kernel), self.M
        if T == 1:
            yv = be.vec(y[:, 0])
        else:
            # the (n, T) label matrix with rows 16-byte aligned (T odd: one pad column, never read)
            Yd = be.zeros(n * ((T + 1) // 2 * 2)).view(n, (T + 1) // 2 * 2)
            Yd[:, :T] = be.vec(y)
        ldk = (M + 3) // 4 * 4
        chunk = self.chunk_rows
        if chunk is None:
            chunk = max(128, BLOCK_BYTES // (4 * ldk) // 128 * 128)
        chunk = max(1, min(int(chunk), n))
        # one buffer for every chunk's block (a backend without formats builds its own)
        buf = be.knm_chunk_buffer(chunk, M) if hasattr(be, "knm_chunk_buffer") else None
        if chunk < n and hasattr(be, "share_split"):
            be.share_split(F, Zf, karg)              # (the chunks then carry the split of ALL rows, as the whole block does)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            Fc = F if chunk >= n else be.rows(F, torch.arange(lo, hi))
            K = be.knm_f32(Fc, Zf, karg, n, out=buf) if buf is not None else _block(be, Fc, Zf, karg, n)
            wc, beta = None if w is None else w[lo:hi], decay if lo == 0 else 1.0
            if T == 1:
                be.knm_gram(K, w=wc, y=yv[lo:hi], beta=beta, G=self.gram_, b=self.rhs_)
            else:
                be.knm_gram_multi(K, w=wc, Y=Yd[lo:hi, :T], beta=beta, G=self.gram_, B=self.rhs_)
            del K
        self.n_seen_ = seen
        if solve:
            self.solve()
        return self

    def partial_fit(self, X, Y, sample_weight=None, decay=1.0, solve=True):
        """Add the rows (X, Y), with weights sample_weight (default ones), to the statistics: G and b are first scaled by decay
        (1: nothing is forgotten; 0: a fresh model on these rows with the same centres), ``n_seen_`` becomes
        decay * n_seen_ + sum(w), and the model is solved again unless solve=False (several batches, one solve).  The first
        call fixes the centres and builds the preconditioner.  Raises, and changes nothing, if the arguments are refused or the
        total weight would not stay positive.  G and b are summed chunk by chunk and ``n_seen_`` is set behind the last chunk:
        an error raised in between (out of memory, a failed launch) leaves statistics that hold part of the batch — start
        over with ``fit`` then."""
        return self._update(X, Y, sample_weight, decay, 1.0, solve)

    def remove(self, X, Y, sample_weight=None, solve=True):
        """Take rows that were added (with these labels and weights) out again: ``partial_fit`` with negated weights.  Raises,
        and changes nothing, if the total weight would not stay positive.  The rows' K entries are built again, by the route a
        block of THIS call's rows takes (direct differences or a tile core, and the split scale of this batch): where that is
        not the route they were added by, the entries agree to f32 accuracy, not bit for bit, and so does the removal."""
        return self._update(X, Y, sample_weight, 1.0, -1.0, solve)

    def fit(self, X, Y, Xts=None, Yts=None):
        """A fresh model on these rows: the statistics and (unless given) the centres are dropped first."""
        for k in _DERIVED:
            self.__dict__.pop(k, None)
        self.ny_points_ = self.alpha_ = self.gram_ = self.rhs_ = None
        self.n_seen_ = 0.0
        return self.partial_fit(X, Y)

    def _not_offered(self, *a, **k):
        raise NotImplementedError("IncrementalFalkon: fit_path, fit_multi, fit_grid and fit_cv are not offered: several outputs "
                                  "from one G are the constructor's outputs=, a lambda path from the same statistics is "
                                  "solve_path(penalties); grids and cross-validation are not offered")

    fit_multi = fit_path = fit_cv = fit_grid = _not_offered

    # ------------------------------------------------------------------ the model
    def solve(self, penalty=None):
        """(Re)fit from G, b and n alone; penalty: a new penalty (it stays), which costs a new preconditioner and no K."""
        if self.gram_ is None or not self.n_seen_ > 0.0:
            raise RuntimeError("IncrementalFalkon.solve called before any rows were added")
        if penalty is not None:
            self.penalty = float(penalty)
        be = _backend.get_backend()
        if self.outputs == 1:
            alpha = falkon_fit_stats(be, self.gram_, self.rhs_, self.n_seen_, self._precond(be), float(self.penalty), int(self.maxiter),
                                     self.options.solver_options()).reshape(-1, 1)
        else:
            alpha = falkon_fit_stats_multi(be, self.gram_, self.rhs_, self.n_seen_, self._precond(be), float(self.penalty),
                                           int(self.maxiter), self.options.solver_options()).t().contiguous()      # (M, T)
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        self.alpha_ = alpha
        return self

    def solve_path(self, penalties):
        """The models of a lambda path from G, b and n alone: one fitted ``Falkon`` per penalty, in the order given, from ONE
        be.precond_path (the members share T's factors) and ONE lock-step run over all penalties and outputs
        (solver.falkon_fit_stats_path): no K is built and no row is touched.  The members share one ``ny_points_`` tensor, so
        ``odx.predict_path`` scores a path of one-output members from one kernel evaluation; a member of a model with T outputs
        has ``alpha_`` (M, T).  This model's own ``penalty`` and ``alpha_`` stay as they are."""
        if self.gram_ is None or not self.n_seen_ > 0.0:
            raise RuntimeError("IncrementalFalkon.solve_path called before any rows were added")
        lams = [float(x) for x in penalties]
        if not lams or any(not (math.isfinite(x) and x > 0.0) for x in lams):
            raise ValueError("IncrementalFalkon.solve_path: penalties must be a non-empty sequence of finite positive values, "
                             "got %r" % (lams,))
        be = _backend.get_backend()
        opt = self.options.solver_options()
        Ps = be.precond_path(self._centre_features(be), _kernel_arg(self.kernel), lams, opt.pc_epsilon)
        B = self.rhs_ if self.outputs > 1 else self.rhs_.view(1, -1)
        alphas = falkon_fit_stats_path(be, self.gram_, B, self.n_seen_, Ps, lams, int(self.maxiter), opt)
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        ny = self.ny_points_.clone().cpu()
        members = []
        for l, lam in enumerate(lams):
            est = Falkon(self.kernel, lam, self.M, maxiter=self.maxiter, options=self.options)
            est.alpha_, est.ny_points_ = alphas[l].t().contiguous().cpu(), ny
            members.append(est)
        return members

    def as_falkon(self):
        """The fitted model as a ``Falkon`` (alpha_, ny_points_, kernel, penalty): what predict_path, the heads and storage
        take.  Its tensors are copies: later updates of this model do not reach it."""
        if self.alpha_ is None:
            raise RuntimeError("as_falkon called before a solve")
        est = Falkon(self.kernel, self.penalty, self.M, maxiter=self.maxiter, options=self.options)
        est.alpha_, est.ny_points_ = self.alpha_.clone().cpu(), self.ny_points_.clone().cpu()
        return est
