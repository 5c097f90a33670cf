"""falkon-shaped estimator objects backed by libodx.

The reference never touches FALKON's arithmetic itself; it constructs
``kernels.GaussianKernel(sigma)``, ``FalkonOptions(...)`` and ``InCoreFalkon`` / ``Falkon`` and
calls ``fit`` / ``predict`` / ``kernel.mmv``
(src/modules/region-classifier/FALKONWrapper_with_centers_selection_incore.py:50-82,
 FALKONWrapper_with_centers_selection.py:49-78,
 mrcnn_modified/modeling/roi_heads/box_head/roi_box_predictors.py:136-158,
 mrcnn_modified/modeling/rpn/rpn.py:197-225).  This module provides objects with that
surface — constructor keywords, ``fit(X, Y)``, ``predict(X) -> (n, 1)``, attributes
``ny_points_ / alpha_ / M / kernel`` (re-assignable, deep-copyable, picklable) — so that
the drop-in wrappers in ``src/modules/region-classifier`` stay as thin as the reference's,
and so that ``sys.modules['falkon'] = odx.falkon`` is a valid binding for the reference's
own wrapper files.
"""
import os
import types

import torch

from . import backend as _backend
from . import options as _options
from .solver import SolverOptions, cv_folds, falkon_fit, falkon_fit_cv, falkon_fit_grid, falkon_fit_multi, falkon_fit_path


class FalkonOptions:
    """Accepts falkon's option keywords.  The ones that steer arithmetic are honoured
    (pc_epsilon_32, cg_epsilon_32, cg_tolerance, cg_full_gradient_every); the memory /
    dispatch knobs the reference passes (min_cuda_iter_size_*, min_cuda_pc_size_*,
    keops_active, store_kernel_d_threshold — FALKONWrapper_..._incore.py:56) have nothing to
    select here: K_nM is materialised on the GPU (or, under the option knm_storage = "stream", recomputed by every CG pass
    through a ring in the Infinity Cache) and nothing runs on the CPU."""

    def __init__(self, **kw):
        self.pc_epsilon_32 = kw.pop("pc_epsilon_32", 1e-5)
        self.cg_epsilon_32 = kw.pop("cg_epsilon_32", 1e-7)
        self.cg_tolerance = kw.pop("cg_tolerance", 1e-7)
        self.cg_full_gradient_every = kw.pop("cg_full_gradient_every", 10)
        self.extra = dict(kw)

    def solver_options(self):
        return SolverOptions(pc_epsilon=self.pc_epsilon_32, cg_epsilon=self.cg_epsilon_32,
                             cg_tolerance=self.cg_tolerance, cg_full_gradient_every=self.cg_full_gradient_every)


class _RadialKernel:
    """A radial kernel of the backend (`kind`: ODX_KERNEL_* of include/odx.h) with falkon's ``mmv``."""
    kind = 0

    def _arg(self):
        """What the backend wrappers get as `sigma`: the width itself for the Gaussian (the same float as ever), the kernel
        object for any other kind — a wrapper that does not know the kinds fails at its float(sigma)."""
        return self.sigma if self.kind == 0 else self

    def mmv(self, X1, X2, v, out=None, opt=None, dense=False):
        """K(X1, X2) @ v -> (n, T) f32.  A block-structured v (the heads' alpha_parallel) is
        detected and only its non-zero row range per column is visited.  ``dense=True``: every column weighs every
        centre (a multi-output model, the members of a lambda path) — no ranges are looked for and the backend may
        evaluate K once for all columns (HipBackend.shared_mmv_min).  For a fitted model this is today's result bit
        for bit: the range of a column whose first and last entries are non-zero is [0, M) anyway."""
        be = _backend.get_backend()
        F = be.features(X1)
        Zf = X2 if (hasattr(X2, "sq") or hasattr(X2, "n")) and not torch.is_tensor(X2) else be.features(X2)     # a backend's Features
        v = torch.as_tensor(v)
        if v.dim() == 1:
            v = v[:, None]
        ranges = block_ranges(v) if v.shape[1] > 1 and not dense else None      # one column (model.predict): every centre counts
        res = be.mmv(F, Zf, self._arg(), v, ranges)
        if out is not None:
            out.copy_(res)
            return out
        return res


class GaussianKernel(_RadialKernel):
    """K(x, z) = exp(-|x - z|^2 / (2 sigma^2)); ``mmv`` is the fused scoring kernel."""
    kernel_name = "gaussian"
    kind = 0                    # ODX_KERNEL_GAUSS

    def __init__(self, sigma, opt=None):
        self.sigma = float(sigma)

    def __repr__(self):
        return "GaussianKernel(sigma=%g)" % self.sigma


class MaternKernel(_RadialKernel):
    """falkon's MaternKernel(sigma, nu) for nu = 3/2 and 5/2: with u = sqrt(2 nu) |x - z| / sigma,
    K = (1 + u) exp(-u) and K = (1 + u + u^2 / 3) exp(-u).  The entries come from the Gaussian tiles' contraction X Z' with
    another epilogue (odx_radial_*), so fit, fit_multi, fit_path, fit_cv, predict and predict_path run as for the Gaussian,
    on stored blocks of every format.  nu = inf is the Gaussian itself (kind 0).  The estimators hand this object to the
    backend where a Gaussian fit hands its sigma; it deliberately has no __float__, so that a route that was not taught the
    kinds raises TypeError instead of evaluating a Gaussian."""
    kernel_name = "matern"
    _KINDS = {1.5: 1, 2.5: 2, float("inf"): 0}       # ODX_KERNEL_MATERN32 / _MATERN52 / _GAUSS

    def __init__(self, sigma, nu, opt=None):
        self.sigma = float(sigma)
        self.nu = float(nu)
        if self.nu == 0.5:
            raise NotImplementedError(
                "MaternKernel: nu = 1/2 is not offered: exp(-r / sigma) has an unbounded slope in d^2 at 0, where the f32 "
                "evaluation of d^2 is off by up to 8e-4 for rows that are centres, so alpha misses the 1e-4 bar ten times over")
        if self.nu not in self._KINDS:
            raise ValueError("MaternKernel: nu must be 1.5, 2.5 or inf (the Gaussian), got %r" % (nu,))
        self.kind = self._KINDS[self.nu]

    def __repr__(self):
        return "MaternKernel(sigma=%g, nu=%g)" % (self.sigma, self.nu)


def _kernel_arg(kernel):
    """The `sigma` argument an estimator hands down for its kernel: kernel.sigma for a Gaussian (any object with a sigma and
    no kind, as ever), the kernel object itself for another kind."""
    return kernel if getattr(kernel, "kind", 0) else kernel.sigma


def _grid_refuse(kernel, what):
    if getattr(kernel, "kind", 0):
        raise NotImplementedError("%s: the sigma grid is Gaussian-only (its kernels take a width per block / column); got %r" % (what, kernel))


class CVResult:
    """What `fit_cv` returns.  estimators: one per penalty, fitted on ALL rows and sharing `ny_points_` (predict_path accepts
    them); empty without refit.  scores: (n, L) f32, column l the scores of every row by the model of penalty l that never
    saw the row's fold.  fold_of: (n,) the fold assignment used.  fold_alphas: (L, folds, M) f64, the fold fits.
    mse: (L,) f64, the mean over the rows of (scores - Y)^2."""

    def __init__(self, estimators, scores, fold_of, fold_alphas, mse):
        self.estimators, self.scores, self.fold_of, self.fold_alphas, self.mse = estimators, scores, fold_of, fold_alphas, mse


def block_ranges(v):
    """Per column: [first non-zero row, last non-zero row + 1) as an int32 (T, 2) tensor."""
    nz = v != 0
    Mtot, T = v.shape
    if Mtot == 0:
        return torch.zeros((T, 2), dtype=torch.int32, device=v.device)
    idx = torch.arange(Mtot, device=v.device)[:, None]
    big = torch.where(nz, idx, torch.full_like(idx, Mtot)).amin(0)
    end = torch.where(nz, idx + 1, torch.zeros_like(idx)).amax(0)
    lo = torch.minimum(big, end)
    return torch.stack([lo, end], dim=1).to(torch.int32)


class _FalkonBase:
    """Common fit / predict.  ``center_selection.select(X, Y)`` follows MyCenterSelector
    (src/modules/region-classifier/MyCenterSelector.py:7-15)."""
    _cpu_model = False

    def __init__(self, kernel, penalty, M, center_selection="uniform", maxiter=20, seed=None,
                 error_fn=None, error_every=1, options=None, weight_fn=None, **_ignored):
        self.kernel = kernel
        # falkon's weight_fn(Y, X, indices) -> one weight per row (None: the unweighted fit, as ever).  With it, fit() is the
        # sample-weighted squared-loss fit (odx/weighted.py) and every other fit method refuses.
        self.weight_fn = weight_fn
        self.penalty = penalty
        self.M = M
        self.maxiter = maxiter
        self.center_selection = center_selection
        self.options = options if options is not None else FalkonOptions()
        self.seed = seed
        self.alpha_ = None
        self.ny_points_ = None

    def fit(self, X, Y, Xts=None, Yts=None):
        if self.__dict__.get("weight_fn") is not None:
            return self._fit_weighted(X, Y)
        return self._fit(X, Y, multi=False)

    def _no_weights(self, what):
        """The fit methods that know no row weights refuse an estimator with a weight_fn instead of fitting unweighted."""
        if self.__dict__.get("weight_fn") is not None:
            raise NotImplementedError("%s: sample weights (weight_fn) are offered by fit(X, Y) only; %s would fit unweighted"
                                      % (type(self).__name__, what))

    def _fit_weighted(self, X, Y):
        """fit(X, Y) with a weight_fn: the centres WITH their labels and indices, the weights of the rows
        (weight_fn(Y, X, None)) and of the centres (weight_fn(Y_Z, Z, idx)), then weighted.falkon_fit_weighted.  Uniform
        selection has the indices; a ``center_selection`` object is called as ``select(X, Y)`` and must return ``(Z, Y_Z)``
        or ``(Z, Y_Z, idx)`` (LogisticFalkon's rule; idx is None for the first form)."""
        from .weighted import falkon_fit_weighted
        name = type(self).__name__
        be = _backend.get_backend()
        F = be.features(X)
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1:
            raise ValueError("odx FALKON fits one right-hand side per model (the reference trains one "
                             "binary classifier per fit); got Y with %d columns" % y.shape[1])
        y = y.to(F.X.device)
        if isinstance(self.center_selection, str):
            gen = None
            if self.seed is not None:
                gen = torch.Generator()
                gen.manual_seed(int(self.seed))
            idx = torch.randperm(F.n, generator=gen)[: self.M]
            Zf = be.rows(F, idx)
            yz = y[idx.to(y.device)]
        else:
            sel = self.center_selection.select(F.X, y)
            if not isinstance(sel, tuple) or len(sel) not in (2, 3) or sel[1] is None:
                raise ValueError("%s: with a weight_fn, center_selection.select(X, Y) must return (Z, Y_Z) or (Z, Y_Z, idx): "
                                 "the centres with their labels" % name)
            Zf = be.features(sel[0])
            yz = torch.as_tensor(sel[1]).reshape(-1, 1).to(F.X.device)
            idx = sel[2] if len(sel) == 3 else None
            if yz.shape[0] != Zf.n:
                raise ValueError("%s: the selector returned %d centres and %d labels" % (name, Zf.n, yz.shape[0]))
        self.M = Zf.n

        def weights(lab, rows, ind, count, what, total):
            wv = torch.as_tensor(self.weight_fn(lab, rows, ind)).reshape(-1).to(torch.float64)
            if wv.numel() != count:
                raise ValueError("%s: weight_fn returned %d weights for %s, expected %d" % (name, wv.numel(), what, count))
            if not bool(torch.isfinite(wv).all()) or bool((wv < 0).any()) or (total and not float(wv.sum()) > 0.0):
                raise ValueError("%s: the weights of %s must be finite and >= 0%s" % (name, what, " with a positive sum" if total else ""))
            return be.vec(wv)
        w = weights(y, F.X, None, F.n, "the rows", True)
        wz = weights(yz, Zf.X, idx, Zf.n, "the centres", False)
        alpha = falkon_fit_weighted(be, F, be.vec(y[:, 0]), w, Zf, wz, _kernel_arg(self.kernel), float(self.penalty),
                                    int(self.maxiter), self.options.solver_options()).reshape(-1, 1)
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        self.alpha_ = alpha
        self.ny_points_ = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        if self._cpu_model:
            self.alpha_, self.ny_points_ = self.alpha_.cpu(), self.ny_points_.cpu()
        else:
            self._centres(Zf)
        return self

    def fit_multi(self, X, Y):
        """Fit the T >= 1 columns of Y (n, T) as T outputs of ONE model over the same rows and centres, from one K_nM block
        and one preconditioner (solver.falkon_fit_multi): `alpha_` becomes (M, T) and `predict` returns (n, T), as the upstream
        estimator's fit does for a label matrix.  Centres, `ny_points_` and the centre cache are handled as by `fit`; one column
        takes `fit`'s code path, bit for bit.  (`fit` itself keeps refusing more than one column.)"""
        self._no_weights("fit_multi")
        return self._fit(X, Y, multi=True)

    def _fit(self, X, Y, multi):
        be = _backend.get_backend()
        F = be.features(X)
        if isinstance(self.center_selection, str):
            idx = torch.randperm(F.n)[: self.M]
            Zf = be.rows(F, idx)
        else:
            sel = self.center_selection.select(F.X, None)
            Z = sel[0] if isinstance(sel, tuple) else sel
            Zf = be.features(Z)
        self.M = Zf.n
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1 and not (multi and y.shape[1] > 1):
            raise ValueError("odx FALKON fits one right-hand side per model (the reference trains one "
                             "binary classifier per fit); got Y with %d columns" % y.shape[1])
        if y.shape[1] == 1:
            yv = be.vec(y[:, 0])
            alpha = falkon_fit(be, F, yv, Zf, _kernel_arg(self.kernel), float(self.penalty), int(self.maxiter),
                               self.options.solver_options()).reshape(-1, 1)
        else:
            # T label columns over the same rows and centres: one block, one preconditioner
            alpha = falkon_fit_multi(be, F, be.vec(y), Zf, _kernel_arg(self.kernel), float(self.penalty), int(self.maxiter),
                                     self.options.solver_options()).t().contiguous()          # (M, T), as upstream's alpha_
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()          # (a chain of 4096 centres or more made helper streams: not left behind idle)
        ny = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        self.alpha_ = alpha
        self.ny_points_ = ny
        if self._cpu_model:
            self.alpha_ = self.alpha_.cpu()
            self.ny_points_ = self.ny_points_.cpu()
        else:
            self._centres(Zf)
        return self

    def fit_path(self, X, Y, penalties):
        """One fitted estimator of this class per penalty, from one K_nM block (solver.falkon_fit_path): the centres are
        selected once and shared (`ny_points_`), each estimator has its own `penalty` and `alpha_`.  This estimator is the
        template and stays as it is.  Under knm_storage "stream" (no block: K is recomputed by the passes) up to 8 penalties
        cost one recompute of K per CG iteration, 9 .. 16 one per iteration plus one per full residual."""
        import copy
        self._no_weights("fit_path")
        be = _backend.get_backend()
        F = be.features(X)
        if isinstance(self.center_selection, str):
            Zf = be.rows(F, torch.randperm(F.n)[: self.M])
        else:
            sel = self.center_selection.select(F.X, None)
            Zf = be.features(sel[0] if isinstance(sel, tuple) else sel)
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1:
            raise ValueError("odx FALKON fits one right-hand side per model (the reference trains one "
                             "binary classifier per fit); got Y with %d columns" % y.shape[1])
        penalties = [float(p) for p in penalties]
        alphas = falkon_fit_path(be, F, be.vec(y[:, 0]), Zf, _kernel_arg(self.kernel), penalties, int(self.maxiter),
                                 self.options.solver_options())
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        ny = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        out = []
        for l, pen in enumerate(penalties):
            est = copy.copy(self)
            est.__dict__.pop("_zf", None)
            est.penalty, est.M = pen, Zf.n
            est.alpha_, est.ny_points_ = alphas[l].clone().reshape(-1, 1), ny
            if est._cpu_model:
                est.alpha_, est.ny_points_ = est.alpha_.cpu(), est.ny_points_.cpu()
            else:
                est._centres(Zf)
            out.append(est)
        return out

    def fit_cv(self, X, Y, penalties, folds=5, fold_of=None, seed=0, refit=True):
        """A `folds`-fold cross-validation of `penalties` from ONE K_nM block (solver.falkon_fit_cv): the held-out score of
        every row at every penalty and, with refit, one estimator per penalty fitted on all rows — a CVResult.  The centres
        are selected once, from all rows, as in fit_path, and every fold fit uses them.  fold_of: the caller's (n,)
        assignment with values in [0, folds); None: cv_folds(n, folds, seed), which leaves the global RNG alone.  This
        estimator is the template and stays as it is."""
        import copy
        self._no_weights("fit_cv")
        be = _backend.get_backend()
        F = be.features(X)
        if isinstance(self.center_selection, str):
            Zf = be.rows(F, torch.randperm(F.n)[: self.M])
        else:
            sel = self.center_selection.select(F.X, None)
            Zf = be.features(sel[0] if isinstance(sel, tuple) else sel)
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1:
            raise ValueError("odx FALKON fits one right-hand side per model (the reference trains one "
                             "binary classifier per fit); got Y with %d columns" % y.shape[1])
        penalties, folds = [float(p) for p in penalties], int(folds)
        if fold_of is None:
            fold_of = cv_folds(F.n, folds, seed)
        yv = be.vec(y[:, 0])
        alphas, heldout = falkon_fit_cv(be, F, yv, Zf, _kernel_arg(self.kernel), penalties, fold_of, folds, int(self.maxiter),
                                        self.options.solver_options(), refit=refit)
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        host = self._cpu_model and not (torch.is_tensor(X) and X.is_cuda)
        scores = heldout.t().to(torch.float32).contiguous()
        mse = ((scores.double() - yv[:, None]) ** 2).mean(0)
        fold_alphas = alphas[:, :folds].clone()
        if host:
            scores, mse, fold_alphas = scores.cpu(), mse.cpu(), fold_alphas.cpu()
        ny = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        if self._cpu_model:
            ny = ny.cpu()                    # once: the members share ONE tensor (predict_path asks for that)
        out = []
        for l, pen in enumerate(penalties if refit else []):
            est = copy.copy(self)
            est.__dict__.pop("_zf", None)
            est.penalty, est.M = pen, Zf.n
            est.alpha_, est.ny_points_ = alphas[l, folds].clone().reshape(-1, 1), ny
            if est._cpu_model:
                est.alpha_ = est.alpha_.cpu()
            else:
                est._centres(Zf)
            out.append(est)
        return CVResult(out, scores, torch.as_tensor(fold_of), fold_alphas, mse)

    def fit_grid(self, X, Y, sigmas, penalties):
        """One fitted estimator of this class per (sigma, penalty): S lists of L estimators, from one contraction of X Z' per
        group of widths where the backend has one (solver.falkon_fit_grid).  The centres are selected once, as in fit_path,
        and shared by all members (`ny_points_`); each member has its own GaussianKernel(sigma), `penalty` and `alpha_`.
        This estimator is the template and stays as it is."""
        import copy
        self._no_weights("fit_grid")
        _grid_refuse(self.kernel, "fit_grid")
        be = _backend.get_backend()
        F = be.features(X)
        if isinstance(self.center_selection, str):
            Zf = be.rows(F, torch.randperm(F.n)[: self.M])
        else:
            sel = self.center_selection.select(F.X, None)
            Zf = be.features(sel[0] if isinstance(sel, tuple) else sel)
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1:
            raise ValueError("odx FALKON fits one right-hand side per model (the reference trains one "
                             "binary classifier per fit); got Y with %d columns" % y.shape[1])
        sigmas, penalties = [float(s) for s in sigmas], [float(p) for p in penalties]
        alphas = falkon_fit_grid(be, F, be.vec(y[:, 0]), Zf, sigmas, penalties, int(self.maxiter), self.options.solver_options())
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        ny = Zf.X.contiguous() if Zf.X.stride(0) != Zf.D else Zf.X
        if self._cpu_model:
            ny = ny.cpu()                    # once: the members share ONE tensor (predict_grid asks for that)
        out = []
        for s, sigma in enumerate(sigmas):
            row = []
            for l, pen in enumerate(penalties):
                est = copy.copy(self)
                est.__dict__.pop("_zf", None)
                est.kernel = GaussianKernel(sigma)
                est.penalty, est.M = pen, Zf.n
                est.alpha_, est.ny_points_ = alphas[s, l].clone().reshape(-1, 1), ny
                if est._cpu_model:
                    est.alpha_ = est.alpha_.cpu()
                else:
                    est._centres(Zf)
                row.append(est)
            out.append(row)
        return out

    def _centres(self, Zf=None):
        """The centres as kernel operands (row norms, packed f16 split), kept with the model while `ny_points_` is the
        same, unmodified tensor: a predict is ~100 us of GPU work and re-deriving them was a third of its launches.
        Same bits as a fresh derivation (the split's scale comes from the centres alone)."""
        be, ny = _backend.get_backend(), self.ny_points_
        if Zf is not None:
            if ny is Zf.X and getattr(Zf, "own_pack", True):
                self._zf = (ny, ny._version, be, Zf)
            return Zf
        c = self.__dict__.get("_zf")
        if c is not None and c[0] is ny and c[1] == ny._version and c[2] is be:
            if ny.is_cuda:          # possibly made on another stream than the one that scores with them now
                cur = torch.cuda.current_stream()
                z32 = getattr(c[3], "f32", None)          # 16-bit centres: the f32 form the fallbacks read, if it exists
                for z in (c[3], z32):
                    for t in (() if z is None else (z.X, z.sq, getattr(z, "P", None), getattr(z, "meta", None))):
                        if t is not None:
                            t.record_stream(cur)
            return c[3]
        Zf = be.features(ny)
        if torch.is_tensor(ny):
            self._zf = (ny, ny._version, be, Zf)
        return Zf

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_zf", None)          # derived data, tied to this process's backend: not copied, not pickled
        return d

    def predict(self, X):
        if self.alpha_ is None:
            raise RuntimeError("predict called before fit")
        if self.alpha_.dim() == 2 and self.alpha_.shape[1] > 1:     # a multi-output model: all columns share the centres
            res = self.kernel.mmv(X, self._centres(), self.alpha_, dense=True)
        else:
            res = self.kernel.mmv(X, self._centres(), self.alpha_)
        if self._cpu_model and not (torch.is_tensor(X) and X.is_cuda):
            res = res.cpu()
        return res

    def __bool__(self):
        return True


def _same_tensor(a, b):
    return a is b or (torch.is_tensor(a) and torch.is_tensor(b) and a.data_ptr() == b.data_ptr() and a.shape == b.shape
                      and a.stride() == b.stride() and a.dtype == b.dtype and a.device == b.device)


def predict_path(estimators, X):
    """(n, L) f32: column l is ``estimators[l].predict(X)[:, 0]``, bit for bit, from ONE dense mmv over the stacked
    alphas — the members of a ``fit_path``, or any fitted estimators that share their centres (one ``ny_points_``
    tensor), sigma and have one output each.  Scoring a path on held-out rows then costs one contraction where the
    backend evaluates K once for all columns (HipBackend.shared_mmv_min) instead of L.  The first member's centre
    cache is used; a host model (``Falkon``) returns a host tensor for host rows, as ``predict`` does."""
    estimators = list(estimators)
    if not estimators:
        raise ValueError("predict_path: no estimators")
    first = estimators[0]
    for est in estimators:
        if est.alpha_ is None or est.ny_points_ is None:
            raise RuntimeError("predict_path called before fit")
        if not _same_tensor(est.ny_points_, first.ny_points_):
            raise ValueError("predict_path: the estimators must share one ny_points_ tensor (the members of a fit_path do)")
        if float(est.kernel.sigma) != float(first.kernel.sigma):
            raise ValueError("predict_path: the estimators must share sigma, got %g and %g" % (first.kernel.sigma, est.kernel.sigma))
        if getattr(est.kernel, "kind", 0) != getattr(first.kernel, "kind", 0):
            raise ValueError("predict_path: the estimators must share the kernel function, got %r and %r" % (first.kernel, est.kernel))
        if est.alpha_.dim() != 2 or tuple(est.alpha_.shape) != (first.ny_points_.shape[0], 1):
            raise ValueError("predict_path: every alpha_ must be (M, 1), got %s" % (tuple(est.alpha_.shape),))
    V = torch.cat([est.alpha_ for est in estimators], dim=1)
    res = first.kernel.mmv(X, first._centres(), V, dense=True)
    if first._cpu_model and not (torch.is_tensor(X) and X.is_cuda):
        res = res.cpu()
    return res


def predict_grid(estimators, X):
    """(n, T) f32: column t is ``estimators[t].predict(X)[:, 0]`` for fitted one-output estimators that share their centres
    (one ``ny_points_`` tensor) and have ANY kernel widths — the members of a ``fit_grid``, flattened in any order — from
    ONE dense scoring call over the stacked alphas (backend ``mmv_sigmas``: one contraction of X Z' per group of up to 8
    columns on HipBackend, every column with its own exponent; bit for bit each distinct sigma's ``predict_path``).
    ``predict_path`` keeps refusing mixed widths.  A backend without ``mmv_sigmas`` scores width by width.  The first
    member's centre cache is used; a host model returns a host tensor for host rows, as ``predict`` does."""
    estimators = list(estimators)
    if not estimators:
        raise ValueError("predict_grid: no estimators")
    first = estimators[0]
    for est in estimators:
        if est.alpha_ is None or est.ny_points_ is None:
            raise RuntimeError("predict_grid called before fit")
        if not _same_tensor(est.ny_points_, first.ny_points_):
            raise ValueError("predict_grid: the estimators must share one ny_points_ tensor (the members of a fit_grid do)")
        if est.alpha_.dim() != 2 or tuple(est.alpha_.shape) != (first.ny_points_.shape[0], 1):
            raise ValueError("predict_grid: every alpha_ must be (M, 1), got %s" % (tuple(est.alpha_.shape),))
        _grid_refuse(est.kernel, "predict_grid")
    sigmas = [float(est.kernel.sigma) for est in estimators]
    V = torch.cat([est.alpha_ for est in estimators], dim=1)
    be = _backend.get_backend()
    F, Zf = be.features(X), first._centres()
    if hasattr(be, "mmv_sigmas"):
        res = be.mmv_sigmas(F, Zf, sigmas, V)
    else:
        res = torch.cat([be.mmv(F, Zf, s, V[:, t:t + 1].contiguous()) for t, s in enumerate(sigmas)], dim=1)
    if first._cpu_model and not (torch.is_tensor(X) and X.is_cuda):
        res = res.cpu()
    return res


def _refuse_weighted(estimators, what):
    """The batched fits know no row weights: an estimator with a weight_fn is refused instead of fitted unweighted."""
    for est in estimators:
        if getattr(est, "weight_fn", None) is not None:
            raise NotImplementedError("%s: sample weights (weight_fn) are offered by fit(X, Y) only; the batched fit would "
                                      "fit %s unweighted" % (what, type(est).__name__))


def fit_batch(estimators, Xs, Ys, streams=None):
    """Fit several independent estimators (the classes of one Minibootstrap round) with ONE batched preconditioner
    launch chain (backend.precond_batched) instead of one ~400-launch chain each; the K_nM build and the CG of every
    class then run as in ``fit`` — on `streams` round-robin when given (the classes are independent), each reusing its
    slice of the batched factors.  Every estimator ends up exactly as its own ``fit(X, Y)`` would leave it (same bits:
    the batched factors equal the single-class ones).  The reference has no counterpart: it trains the classes one
    after the other (OnlineRegionClassifier_incore.py:96-155)."""
    _refuse_weighted(estimators, "fit_batch")
    be = _backend.get_backend()
    if not hasattr(be, "precond_batched"):
        for est, X, Y in zip(estimators, Xs, Ys):
            est.fit(X, Y)
        return estimators
    # First only what the factorisation chains need — the centres — so that the GPU starts on K_MM while the host is still
    # preparing the rest: the row norms of the training sets and the uploads of the labels (a launch / a copy per class, ~2 ms
    # of host time for the 30 classes of a round) are issued behind the chains (`finish` below), for the K_nM builds.
    Fs, Zfs, yvs = [], [], []
    for est, X, Y in zip(estimators, Xs, Ys):
        if isinstance(est.center_selection, str):
            F = be.features(X)                           # (the uniform selection gathers norms and packed rows along)
            Zf = be.rows(F, torch.randperm(F.n)[: est.M])
        else:
            F = be.features(X, norms=False) if hasattr(be, "row_matrix") else be.features(X)
            sel = est.center_selection.select(F.X, None)
            Zf = be.features(sel[0] if isinstance(sel, tuple) else sel)
        est.M = Zf.n
        if hasattr(be, "f32"):
            be.f32(Zf)          # 16-bit centres: their f32 form (the chains' operand) is made HERE, on the caller's stream, which
            #                     the chains' side streams and the builds' class streams all wait for
        y = torch.as_tensor(Y).reshape(F.n, -1)
        if y.shape[1] != 1:
            raise ValueError("odx FALKON fits one right-hand side per model; got Y with %d columns" % y.shape[1])
        Fs.append(F), Zfs.append(Zf), yvs.append(y)

    def finish(i):
        if getattr(Fs[i], "sq", 0) is None:
            Fs[i] = be.with_norms(Fs[i]) if hasattr(be, "with_norms") else be.features(Fs[i].X)
        if yvs[i].dim() == 2:
            yvs[i] = be.vec(yvs[i][:, 0])
    # classes that share (sigma, penalty, jitter) share a chain; the reference's classes always do
    groups = {}
    for i, est in enumerate(estimators):
        o = est.options.solver_options()
        # (another kernel kind: the object travels as sigma and precond_batched, which knows the Gaussian only, refuses it)
        groups.setdefault((_kernel_arg(est.kernel) if getattr(est.kernel, "kind", 0) else float(est.kernel.sigma), float(est.penalty),
                           o.pc_epsilon), []).append(i)
    from . import solver as _solver
    cur = torch.cuda.current_stream() if streams else None
    for (sigma, lam, eps), members in groups.items():
        for c0 in range(0, len(members), be.MAX_CLASS_BATCH):
            chunk = members[c0:c0 + be.MAX_CLASS_BATCH]
            opts = [estimators[i].options.solver_options() for i in chunk]
            iters = {int(estimators[i].maxiter) for i in chunk}
            same = len(iters) == 1 and all(o == opts[0] for o in opts) and hasattr(be, "cg_solve_batched")
            if same and hasattr(be, "knm_format"):
                # the lock-step library loop needs one storage format and one pass configuration for the chunk: decided BEFORE
                # anything is built (otherwise every K_nM block would be built here, held, and built again below)
                fmts = {be.knm_format(Fs[i].n, Zfs[i].n) for i in chunk}
                same = len(fmts) == 1 and (not hasattr(be, "cg_batched_supported") or
                                           be.cg_batched_supported([Fs[i].n for i in chunk], [Zfs[i].n for i in chunk], fmts.pop()))
            if same:
                Mmax = max(Zfs[i].n for i in chunk)
                b0s = torch.zeros((len(chunk), (Mmax + 1) // 2 * 2), dtype=torch.float64, device=be.device)
                if streams:
                    for s in streams:           # before the chain is queued: the builds below start beside it, not after it
                        s.wait_stream(cur)
            if streams and len(chunk) >= 2 * int(_options.current().chain_split_min):
                # two half chains side by side: a chain is a dependent sequence of short launches, a third of them one
                # workgroup per class (the 128 x 128 diagonal factorisations), and a half's products fill what the other
                # half's diagonal steps leave idle.  Both write their classes' slots of ONE factor block (the lock-step CG
                # wants a uniform stride); per class the factors are those of any other grouping, bit for bit.
                Mmax_c = max(Zfs[i].n for i in chunk)
                block = torch.empty((len(chunk), 4, Mmax_c, (Mmax_c + 1) // 2 * 2), dtype=torch.float64, device=be.device)
                h = (len(chunk) + 1) // 2
                side = _chain_stream(0)
                side.wait_stream(cur)
                # (neither half on the caller's stream — usually the device's default stream: measured 4 % of a Minibootstrap
                # round faster than with the first half there)
                side_a = _chain_stream(1)
                side_a.wait_stream(cur)
                with torch.cuda.stream(side_a):
                    Ps = be.precond_batched([Zfs[i] for i in chunk[:h]], sigma, lam, eps, out=block[:h], ws_key="precond_batched_fit", Mmax=Mmax_c)
                for P in Ps:
                    P.info.record_stream(cur)
                with torch.cuda.stream(side):
                    Pb = be.precond_batched([Zfs[i] for i in chunk[h:]], sigma, lam, eps, out=block[h:], ws_key="precond_batched_fit_b", Mmax=Mmax_c)
                for P in Pb:
                    P.info.record_stream(cur)
                Ps = Ps + Pb
            else:
                side = side_a = None
                Ps = be.precond_batched([Zfs[i] for i in chunk], sigma, lam, eps, ws_key="precond_batched_fit")
            for i in chunk:
                finish(i)
            if same and streams:
                for s in streams:               # the builds read the norms and labels just queued on the caller's stream
                    s.wait_stream(cur)
            alphas = None
            if same:
                # K_nM builds (f16 split of the rows, one Gaussian launch, the right-hand side: ~10 short kernels per
                # class) on the streams while the factorisation chain runs, then ALL CG loops of the chunk in lock step
                Ks = []
                for row, i in enumerate(chunk):
                    with (torch.cuda.stream(streams[row % len(streams)]) if streams else _nullcontext()):
                        K, _ = be.knm_rhs(Fs[i], Zfs[i], sigma, yvs[i] * (1.0 / Fs[i].n), rhs_out=b0s[row, :Zfs[i].n])
                        if streams:
                            K.K.record_stream(cur)      # allocated on a side stream, read by the CG on the caller's
                    Ks.append(K)
                if streams:
                    for s in streams:
                        cur.wait_stream(s)
                # (ONE lock-step CG over both halves: a CG per half, the first started beside the tail of the second chain,
                # measured slower — twice the launches, each half the width the triangular products stream best at)
                if side is not None:
                    cur.wait_stream(side_a)
                    cur.wait_stream(side)
                alphas = be.cg_solve_batched(Ks, Ps, b0s, [Fs[i].n for i in chunk], lam, iters.pop(), opts[0])
            if side is not None:
                cur.wait_stream(side_a)
                cur.wait_stream(side)
            for row, (i, P) in enumerate(zip(chunk, Ps)):
                est = estimators[i]
                if alphas is not None:
                    alpha = alphas[row, :Zfs[i].n].clone()
                    if opts[row].check_pivots:
                        _solver._check_pivots(be, P)
                else:       # classes in different pass configurations (or a backend without the batched loop): one CG each
                    if streams:
                        streams[i % len(streams)].wait_stream(cur)
                    with (torch.cuda.stream(streams[i % len(streams)]) if streams else _nullcontext()):
                        alpha = falkon_fit(be, Fs[i], yvs[i], Zfs[i], _kernel_arg(est.kernel), float(est.penalty), int(est.maxiter),
                                           opts[row], precond=P)
                ny = Zfs[i].X.contiguous() if Zfs[i].X.stride(0) != Zfs[i].D else Zfs[i].X
                est.alpha_, est.ny_points_ = alpha.reshape(-1, 1), ny
                if est._cpu_model:
                    est.alpha_, est.ny_points_ = est.alpha_.cpu(), est.ny_points_.cpu()
                else:
                    est._centres(Zfs[i])
    if streams:
        for s in streams:
            cur.wait_stream(s)
    if hasattr(be, "release_helper_streams"):
        be.release_helper_streams()              # (see InCoreFalkon.fit)
    return estimators


class BatchFit:
    """fit_batch in two phases, for callers that can hand over the classes of a round in groups: ``add`` prepares a group's
    centres and queues its factorisation chain at once (on a side stream of its own), ``finish`` queues everything that
    needs all groups — row norms, K_nM builds, ONE lock-step CG over all classes — and leaves every estimator as its own
    ``fit`` would (same bits).  Between two ``add`` calls the caller is free to synchronise with the host and prepare the
    next group while the first group's chain already runs (the Minibootstrap reads a group's selections, gathers its rows
    and draws its centres: ~2.5 ms of host work per half round that used to pass with the GPU idle).
    The fast path needs what a Minibootstrap round has: a GPU backend with the batched chain and CG, side streams, at most
    32 classes with one (sigma, penalty, jitter, iterations, options) and pre-chosen centres; anything else is collected and
    goes through fit_batch in ``finish``."""

    def __init__(self, streams=None):
        self.be = _backend.get_backend()
        self.streams = list(streams) if streams else None
        self.est, self.Xs, self.Ys = [], [], []
        self.Fs, self.Zfs, self.ys = [], [], []
        self.segments = []            # (first class, count, Preconds of the group, its chain's stream)
        self.block = None
        self.key = None
        self.fast = bool(self.streams) and hasattr(self.be, "precond_batched") and hasattr(self.be, "cg_solve_batched") \
            and hasattr(self.be, "row_matrix") and torch.cuda.is_available()
        self.cur = torch.cuda.current_stream() if self.fast else None

    def _key(self, est):
        o = est.options.solver_options()
        return (_kernel_arg(est.kernel) if getattr(est.kernel, "kind", 0) else float(est.kernel.sigma), float(est.penalty), o.pc_epsilon, int(est.maxiter),
                (o.cg_epsilon, o.cg_tolerance, o.cg_full_gradient_every, o.check_pivots))

    def add(self, estimators, Xs, Ys, expect_total=None, centres_cap=None):
        """expect_total: classes the caller will add in all (sizes the shared factor block at the first group); centres_cap:
        the most centres any class can have (the block's slot size: a later group with more centres than the first group's
        largest class would otherwise force everything through the general path)."""
        be = self.be
        estimators = list(estimators)
        _refuse_weighted(estimators, "BatchFit")
        first = len(self.est)
        self.est += list(estimators)
        self.Xs += list(Xs)
        self.Ys += list(Ys)
        if not self.fast or not estimators:
            return
        if any(isinstance(e.center_selection, str) or e.center_selection is None for e in estimators):
            self.fast = False
            return
        keys = {self._key(e) for e in estimators}
        if len(keys) != 1 or (self.key is not None and keys != {self.key}):
            self.fast = False
            return
        self.key = next(iter(keys))
        self.opt = estimators[0].options.solver_options()
        total = max(int(expect_total or 0), len(self.est))
        if total > be.MAX_CLASS_BATCH:
            self.fast = False
            return
        Fs, Zfs, ys = [], [], []
        for est, X, Y in zip(estimators, Xs, Ys):
            F = be.features(X, norms=False)
            sel = est.center_selection.select(F.X, None)
            Zf = be.features(sel[0] if isinstance(sel, tuple) else sel)
            est.M = Zf.n
            if hasattr(be, "f32"):
                be.f32(Zf)      # (as in fit_batch: the centres' f32 form on the caller's stream, before the chain is queued)
            y = torch.as_tensor(Y).reshape(F.n, -1)
            if y.shape[1] != 1:
                raise ValueError("odx FALKON fits one right-hand side per model; got Y with %d columns" % y.shape[1])
            Fs.append(F), Zfs.append(Zf), ys.append(y)
        Mmax = max(z.n for z in Zfs)
        sigma, lam, eps = self.key[0], self.key[1], self.key[2]
        if self.block is None:
            slot = max(Mmax, int(centres_cap or 0))
            self.block = torch.empty((total, 4, slot, (slot + 1) // 2 * 2), dtype=torch.float64, device=be.device)
        if Mmax > self.block.shape[2] or first + len(estimators) > self.block.shape[0]:
            self.fast = False          # (a later group with more centres than the block was cut for: everything through fit_batch)
            return
        g = len(self.segments)
        side = _chain_stream(g % 2)
        side.wait_stream(self.cur)
        with torch.cuda.stream(side):
            Ps = be.precond_batched(Zfs, sigma, lam, eps, out=self.block[first:first + len(estimators)],
                                    ws_key="precond_batched_fit" + ("_b" if g % 2 else ""), Mmax=int(self.block.shape[2]))
        for P in Ps:
            P.info.record_stream(self.cur)
        self.Fs += Fs
        self.Zfs += Zfs
        self.ys += ys
        self.segments.append((first, len(estimators), Ps, side))

    def abort(self):
        """Give up the round: the caller's stream waits for every chain queued so far (they read rows and caches the caller
        may free or rewrite next), nothing is fitted."""
        for _, _, _, side in self.segments:
            if side is not None and self.cur is not None:
                self.cur.wait_stream(side)
        self.segments = []

    def finish(self):
        be, cur, streams = self.be, self.cur, self.streams
        done = sum(c for _, c, _, _ in self.segments)
        if not self.fast or done != len(self.est):
            if self.segments:                 # chains already queued for some groups: let them drain, then the general path
                for _, _, _, side in self.segments:
                    cur.wait_stream(side)
            return fit_batch(self.est, self.Xs, self.Ys, streams=self.streams)
        from . import solver as _solver
        sigma, lam, eps, maxiter, opt = self.key[0], self.key[1], self.key[2], self.key[3], self.opt
        n_cls = len(self.est)
        Fs, Zfs = self.Fs, self.Zfs
        fmts = {be.knm_format(Fs[i].n, Zfs[i].n) for i in range(n_cls)}
        if len(fmts) != 1 or (hasattr(be, "cg_batched_supported")
                              and not be.cg_batched_supported([f.n for f in Fs], [z.n for z in Zfs], next(iter(fmts)))):
            for _, _, _, side in self.segments:
                cur.wait_stream(side)
            return fit_batch(self.est, self.Xs, self.Ys, streams=self.streams)
        for i in range(n_cls):                # behind the chains: row norms of the training sets, label uploads
            Fs[i] = be.with_norms(Fs[i]) if hasattr(be, "with_norms") else be.features(Fs[i].X)
        yvs = [be.vec(y[:, 0]) for y in self.ys]
        Mmax = int(self.block.shape[2])
        b0s = torch.zeros((n_cls, (Mmax + 1) // 2 * 2), dtype=torch.float64, device=be.device)
        for s in streams:
            s.wait_stream(cur)
        Ks = []
        for i in range(n_cls):
            with torch.cuda.stream(streams[i % len(streams)]):
                K, _ = be.knm_rhs(Fs[i], Zfs[i], sigma, yvs[i] * (1.0 / Fs[i].n), rhs_out=b0s[i, :Zfs[i].n])
                K.K.record_stream(cur)
            Ks.append(K)
        for s in streams:
            cur.wait_stream(s)
        Ps = []
        for _, _, P, side in self.segments:
            cur.wait_stream(side)
            Ps += P
        alphas = be.cg_solve_batched(Ks, Ps, b0s, [f.n for f in Fs], lam, maxiter, opt)
        if alphas is None:
            return fit_batch(self.est, self.Xs, self.Ys, streams=self.streams)
        for i, (est, P) in enumerate(zip(self.est, Ps)):
            alpha = alphas[i, :Zfs[i].n].clone()
            if opt.check_pivots:
                _solver._check_pivots(be, P)
            ny = Zfs[i].X.contiguous() if Zfs[i].X.stride(0) != Zfs[i].D else Zfs[i].X
            est.alpha_, est.ny_points_ = alpha.reshape(-1, 1), ny
            if est._cpu_model:
                est.alpha_, est.ny_points_ = est.alpha_.cpu(), est.ny_points_.cpu()
            else:
                est._centres(Zfs[i])
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()          # (see InCoreFalkon.fit)
        return self.est


_chain_streams = {}


def _chain_stream(k=0):
    """Side stream k (0, 1) of the calling stream for the half chains of fit_batch: the first two of the streams measured to
    sit on hardware queues of their own (odx/streams.py; the callers' class streams are taken from the ones behind them), a
    plain stream when the device has none to spare."""
    from . import streams as _streams
    own = _streams.distinct(2)
    if len(own) > k:
        return own[k]
    dev = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, k)
    if dev not in _chain_streams:
        _chain_streams[dev] = torch.cuda.Stream()
    return _chain_streams[dev]


class _nullcontext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class InCoreFalkon(_FalkonBase):
    """GPU-resident estimator (FALKONWrapper_with_centers_selection_incore.py:58-68)."""


class Falkon(_FalkonBase):
    """The reference's `--CPU` estimator (FALKONWrapper_with_centers_selection.py:53-64) keeps
    data and model on the host; here the rows are staged to the GPU for the fit and the model
    tensors are handed back on the host, so the callers' device moves stay valid."""
    _cpu_model = True


# `from falkon import kernels` / `from falkon.options import *` surfaces
kernels = types.SimpleNamespace(GaussianKernel=GaussianKernel, MaternKernel=MaternKernel)
options = types.SimpleNamespace(FalkonOptions=FalkonOptions)
