"""LogisticFalkon: Newton steps on a weighted logistic loss over one stored K_nM block, each solved by falkon's CG.

Labels are y in {-1, +1}; the loss is l(y, t) = c(y) log(1 + exp(-y t)) with c(+1) = 1 and c(-1) = ``neg_weight`` (a weight on
the negatives: what a detector's classifier with ~10 % positives wants), and the objective over the Nystroem model f = K_nM alpha
is (1 / n) sum_i l(y_i, f_i) + (lam / 2) alpha' (K_MM + eps M I) alpha.

Once per fit: L_T = chol_lower(K_MM + eps M I) in f64, T = L_T'.  The iterate lives in T-coordinates, beta = T alpha (so the
regulariser is lam |beta|^2 / 2), and f = K alpha is held over all rows; both start at 0.  Step t, with (lam_t, m_t) of the
schedule:
    w_M = l''(y_M, L_T beta)                      the loss's curvature at the centres (K_MM alpha up to eps M alpha: no K_MM)
    A   = chol_upper(T diag(w_M) T' / M + lam_t I)
    g, d = l'(y, f), l''(y, f)                    over the rows
    b   = A^-T (T^-T K' g / n + lam_t beta)
    s   : m_t iterations of falkon's CG on  s -> A^-T [ T^-T K' (d o (K T^-1 A^-1 s)) / n + lam_t A^-1 s ]
    beta -= A^-1 s,  alpha -= T^-1 A^-1 s,  f -= K T^-1 A^-1 s
The last term is the CG's accumulated row products sum_i a_i (K v_i) (solver.scores_from_cg), not a pass of its own, so a step
reads K m_t times for the Hessian products (plus once per periodic full residual when m_t >= 10) and once for K' g.  Every
array operation is a libodx kernel reached through the backend (odx/logistic_ops.py); this file sequences them.  No host
synchronisation inside a step or between steps.
"""
import dataclasses
import math
import types

import torch

from . import backend as _backend
from .falkon import _FalkonBase, _kernel_arg
from .solver import SolverOptions, _CG, _cg_run, _check_pivots, _slots


class LogisticLoss:
    """l(y, t) = c(y) log(1 + exp(-y t)), c(+1) = 1, c(-1) = neg_weight > 0."""

    def __init__(self, neg_weight=1.0):
        neg_weight = float(neg_weight)
        if not (math.isfinite(neg_weight) and neg_weight > 0.0):
            raise ValueError("LogisticLoss: neg_weight must be positive and finite, got %r" % (neg_weight,))
        self.neg_weight = neg_weight

    def __repr__(self):
        return "LogisticLoss(neg_weight=%g)" % self.neg_weight


def _schedule(who, penalties, iters):
    penalties, iters = list(penalties), list(iters)
    if not penalties or len(penalties) != len(iters):
        raise ValueError("%s: penalty_list and iter_list must be non-empty and of one length, got %d and %d"
                         % (who, len(penalties), len(iters)))
    if any(not (math.isfinite(float(p)) and float(p) > 0.0) for p in penalties):
        raise ValueError("%s: every penalty must be positive and finite, got %r" % (who, penalties))
    if any(int(m) != m or int(m) < 1 for m in iters):
        raise ValueError("%s: every iteration count must be a positive integer, got %r" % (who, iters))
    return [float(p) for p in penalties], [int(m) for m in iters]


def falkon_fit_logistic(be, F, y, Zf, y_centres, kernel_arg, penalties, iters, loss, opt=None, objective_out=None):
    """Fit one binary logistic FALKON problem (the module's algorithm) over one stored shard.

    be          backend (odx.backend.HipBackend in the product)
    F, y        Features of the n rows and their labels, (n,) f64 device vector of +-1 (checked by the caller)
    Zf, y_centres
                Features of the M centres and their labels, (M,) f64
    kernel_arg  a Gaussian's width or a kernel object (falkon._kernel_arg)
    penalties, iters
                the schedule: step t runs iters[t] CG iterations at penalty penalties[t]
    loss        a LogisticLoss
    objective_out
                optional list: receives the objective (at the step's penalty) before every step and behind the last one —
                one host read per value, the only host synchronisation of the fit
    returns     alpha (M, 1) f64

    K' g / n of step 0 comes out of the block's build (knm_rhs with w = l'(y, 0) / n); every Hessian product is one
    be.ktk_rw.  A streamed shard and a block with a column map are refused (ValueError)."""
    opt = opt or SolverOptions()
    penalties, iters = _schedule("falkon_fit_logistic", penalties, iters)
    n, M = F.n, Zf.n
    if n < 1 or M < 1:
        raise ValueError("falkon_fit_logistic: needs rows and centres, got n = %d, M = %d" % (n, M))
    nw = float(loss.neg_weight)
    if y.numel() != n or y_centres.numel() != M:
        raise ValueError("falkon_fit_logistic: y must hold %d labels and y_centres %d" % (n, M))
    st = be.precond_logistic_begin(Zf, kernel_arg, opt.pc_epsilon)
    f, g, d, tk, df = (be.zeros(n) for _ in range(5))
    lv = be.zeros(n) if objective_out is not None else None
    be.logistic_rows(f, y, nw, g, d, lv)
    K, ktg = be.knm_rhs(F, Zf, kernel_arg, g * (1.0 / n))          # the block, and step 0's K' g / n from the same launch
    if getattr(K, "fmt", None) == "stream":
        raise ValueError("falkon_fit_logistic: needs a stored K_nM block (a streamed shard's rows pass in chunks: no row weights)")
    if getattr(K, "cmap", None) is not None:
        raise ValueError("falkon_fit_logistic: not built for a block of distinct columns (a column map)")
    Mp = (M + 1) // 2 * 2
    TT, CC = be.zeros(Mp).view(1, Mp), be.zeros(Mp).view(1, Mp)
    beta, alpha, dalpha, wM = (be.zeros(M) for _ in range(4))
    cg_opt = dataclasses.replace(opt, check_pivots=False)          # (the status words are looked at once, behind the last step)
    infos = [st.info]

    def exchange(k, rows):
        be.ktk_rw(K, TT[0, :M], d, out=CC[0, :M], t_out=tk if rows else None)

    def objective(lam):
        return float(lv.sum()) / n + 0.5 * lam * float((beta * beta).sum())

    for step, (lam, m) in enumerate(zip(penalties, iters)):
        be.logistic_rows(be.logistic_centre_scores(st, beta), y_centres, nw, None, wM, None)
        P = be.precond_logistic_step(st, wM, lam)
        infos.append(P.info)
        if step > 0:
            be.logistic_rows(f, y, nw, g, d, lv)
            ktg = be.ktk(K, w=g * (1.0 / n), out=ktg)
        if objective_out is not None:
            objective_out.append(objective(lam))
        B = be.trmv(P, "LAi", be.trmv(P, "LTi", ktg, alpha=1.0, beta=lam, z=beta))      # A^-T (T^-T K' g / n + lam beta)
        X, R, Pv, AP = (be.zeros(M) for _ in range(4))
        c = _CG(P, lam, B, X, R, Pv, AP, None, be.zeros(4), (be.zeros(M), None), _slots(TT, CC, M), dalpha, tk, df)
        be.cg_init(B, X, R, Pv, c.state)
        df.zero_()
        _cg_run(be, [c], exchange, float(n), m, cg_opt, False)
        be.axpby(-1.0, be.trmv(P, "LAit", X), 1.0, beta)
        be.axpby(-1.0, c.alpha, 1.0, alpha)
        be.axpby(-1.0, df, 1.0, f)
    if objective_out is not None:
        be.logistic_rows(f, y, nw, None, None, lv)
        objective_out.append(objective(penalties[-1]))
    if opt.check_pivots:
        # one host read for the status words of T's factorisation and every step's A
        _check_pivots(be, types.SimpleNamespace(info=torch.stack([i.reshape(-1)[0] for i in infos]).max().reshape(1)))
    return alpha.reshape(-1, 1)


class LogisticFalkon(_FalkonBase):
    """falkon's LogisticFalkon: a Nystroem kernel classifier fitted by Newton steps on a weighted logistic loss.

    kernel: a GaussianKernel or a MaternKernel.  penalty_list / iter_list: the schedule, one (penalty, CG iterations) per Newton
    step — penalties usually fall towards the wanted one.  loss: a LogisticLoss (default: unweighted).  ``fit(X, Y)`` takes
    labels in {-1, +1}, one column, and selects the centres as ``InCoreFalkon.fit`` does; a ``center_selection`` object is
    called as ``select(X, Y)`` and must return ``(Z, Y_Z)``, the centres WITH their labels.  After a fit: ``alpha_`` (M, 1),
    ``ny_points_``, and ``objective_`` with record_objective=True (the objective before every step and behind the last, a host
    read each).  ``predict`` returns the decision values K alpha, ``predict_proba`` their sigmoid: P(y = +1 | x)."""

    def __init__(self, kernel, penalty_list, iter_list, loss=None, M=None, center_selection="uniform", seed=None, options=None,
                 record_objective=False, **_ignored):
        penalty_list, iter_list = _schedule("LogisticFalkon", penalty_list, iter_list)
        if isinstance(center_selection, str) and M is None:
            raise ValueError("LogisticFalkon: needs M for the uniform selection of centres")
        super().__init__(kernel, penalty_list[-1], M, center_selection=center_selection, maxiter=iter_list[-1], seed=seed,
                         options=options)
        self.penalty_list, self.iter_list = penalty_list, iter_list
        self.loss = loss if loss is not None else LogisticLoss()
        if not isinstance(self.loss, LogisticLoss):
            raise ValueError("LogisticFalkon: loss must be a LogisticLoss, got %r" % (loss,))
        self.record_objective = bool(record_objective)
        self.objective_ = None

    def fit(self, X, Y, Xts=None, Yts=None):
        be = _backend.get_backend()
        if torch.is_tensor(X) and X.dtype in _backend.B16_DTYPES and getattr(be, "native16", False):
            raise ValueError("LogisticFalkon: 16-bit native rows are not offered; pass f32 rows or switch native16 off")
        if getattr(be, "knm_storage", None) == "stream":
            raise ValueError("LogisticFalkon: knm_storage='stream' stores no K_nM block (the Newton steps weight its rows)")
        F = be.features(X)
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1:
            raise ValueError("LogisticFalkon fits one label column per model; got Y with %d columns" % y.shape[1])
        y = y[:, 0].to(torch.float64)

        def check(lab, what):
            if lab.numel() == 0 or not bool(((lab == 1.0) | (lab == -1.0)).all()):
                raise ValueError("LogisticFalkon: %s must be -1 or +1" % what)
        check(y, "the labels")
        if isinstance(self.center_selection, str):
            gen = None
            if self.seed is not None:
                gen = torch.Generator()
                gen.manual_seed(int(self.seed))
            idx = torch.randperm(F.n, generator=gen)[: self.M]
            Zf = be.rows(F, idx)
            yz = y[idx.to(y.device)]
        else:
            sel = self.center_selection.select(F.X, y.to(F.X.device).reshape(-1, 1))
            if not isinstance(sel, tuple) or len(sel) != 2 or sel[1] is None:
                raise ValueError("LogisticFalkon: center_selection.select(X, Y) must return (Z, Y_Z), the centres with their labels")
            Zf = be.features(sel[0])
            yz = torch.as_tensor(sel[1]).reshape(-1).to(torch.float64)
            if yz.numel() != Zf.n:
                raise ValueError("LogisticFalkon: the selector returned %d centres and %d labels" % (Zf.n, yz.numel()))
            check(yz, "the centres' labels")
        self.M = Zf.n
        obj = [] if self.record_objective else None
        alpha = falkon_fit_logistic(be, F, be.vec(y), Zf, be.vec(yz), _kernel_arg(self.kernel), self.penalty_list, self.iter_list,
                                    self.loss, self.options.solver_options(), objective_out=obj)
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        self.alpha_ = alpha
        self.ny_points_ = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        self.objective_ = obj
        if self._cpu_model:
            self.alpha_, self.ny_points_ = self.alpha_.cpu(), self.ny_points_.cpu()
        else:
            self._centres(Zf)
        return self

    def _not_offered(self, *a, **k):
        raise NotImplementedError("LogisticFalkon: lambda paths, grids, cross-validation and several outputs are not offered; "
                                  "penalty_list is the schedule of ONE fit")

    fit_multi = fit_path = fit_cv = fit_grid = _not_offered

    def predict_proba(self, X):
        """P(y = +1 | x) = sigmoid(predict(X)), (n, 1) f32."""
        return torch.sigmoid(self.predict(X))
