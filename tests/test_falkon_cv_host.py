"""Host logic of the K-fold cross-validation of a lambda path (odx.solver.falkon_fit_cv, odx.cv_folds, _FalkonBase.fit_cv)
on the numpy oracle backend: the fold fits are fits with row weights over ONE K_nM block and one preconditioner per penalty,
and a row's held-out score is summed from the row products of the state that never saw its fold.  No GPU."""
import numpy as np
import pytest
import torch

import odx
from oracle import falkon_ref as fr
from tests.oracle_backend import OracleBackend
from tests.synth import blob_problem

SIGMA, LAMS, FOLDS = 6.0, [1e-4, 1e-3], 3


class CvBackend(OracleBackend):
    """The oracle backend with what falkon_fit_cv drives, in numpy, and call counters: ktkn_rows, ktwn, precond_path, trmvn,
    ktkn_width, and the score entries of scores_from_cg (f32-accurate "f32" blocks; cg_scores=False stores the block as
    "bf16" in name, which sends the held-out scores through mmv).  Each row is multiplied as the oracle backend's ktk / trmv
    multiply one vector (tests/test_falkon_multi_host.py, GroupedBackend, says why)."""
    gauss = "h2"
    fold = False

    def __init__(self, cg_scores=True, fmt=None):
        super().__init__(np.float64)
        self.fmt = fmt or ("f32" if cg_scores else "bf16")
        self.calls = {"knm_rhs": 0, "precond_path": 0, "precond": 0, "ktwn": 0, "mmv": 0, "trmv": 0}
        self.rows_calls = []             # per ktkn_rows: (vectors, wrow, whether t_out was given)

    def knm(self, F, Zf, sigma, out=None):
        K = super().knm(F, Zf, sigma, out=out)
        K.fmt = self.fmt
        return K

    def knm_rhs(self, *a, **kw):
        self.calls["knm_rhs"] += 1
        return super().knm_rhs(*a, **kw)

    def precond(self, *a, **kw):
        self.calls["precond"] += 1
        return super().precond(*a, **kw)

    def precond_path(self, Zf, sigma, lams, eps):
        self.calls["precond_path"] += 1
        return [OracleBackend.precond(self, Zf, sigma, lam, eps) for lam in lams]

    def ktkn_width(self, K):
        return 8

    def ktkn_rows(self, K, V, Dw, wrow, out=None, t_out=None):
        self.rows_calls.append((V.shape[0], tuple(wrow), t_out is not None))
        Kd = K.K.double()
        for l in range(V.shape[0]):
            t = Kd @ V[l, :K.M]
            if t_out is not None:
                t_out[l, :K.n].copy_(t)
            if wrow[l] >= 0:
                t = t * Dw[wrow[l], :K.n]
            out[l, :K.M].copy_(Kd.t() @ t)
        return out

    def ktwn(self, K, W, out=None):
        self.calls["ktwn"] += 1
        Kt = K.K.double().t()
        for t in range(W.shape[0]):
            out[t, :K.M].copy_(Kt @ W[t, :K.n])
        return out

    def trmv(self, *a, **kw):
        self.calls["trmv"] += 1
        return super().trmv(*a, **kw)

    def trmvn(self, P, name, X, alpha=1.0, beta=0.0, Z=None, out=None):
        for t in range(X.shape[0]):
            r = alpha * (getattr(P, name) @ X[t, :P.M])
            if beta != 0.0:
                r = r + beta * Z[t, :P.M]
            out[t, :P.M].copy_(r)
        return out

    def cg_scores_axpy(self, state, t, S):
        if state[2] != 0:
            return
        S.add_(state[3] * t)

    def cg_scores_store(self, S, out):
        out.copy_(S.float().reshape(out.shape))
        return out

    def mmv(self, *a, **kw):
        self.calls["mmv"] += 1
        return super().mmv(*a, **kw)


def _problem(n=900, D=24, M=90, seed=61):
    """blob_problem's rows with M DISTINCT centres.  (tests.synth.centres draws the positives with replacement.  With 80
    distinct centres among 90, two f64 evaluations of the same fold fit that add the rows in another order — all rows with
    zero weights here, the training rows alone in the oracle — measured 1.4e-3 apart in alpha and 3e-4 of the largest score
    after 20 CG steps at lambda = 1e-4, and 1e-15 with distinct centres: that would measure the fixture, not the wiring.)"""
    X, y, rng = blob_problem(n, D, seed=seed)
    idx = sorted(rng.choice(n, M, replace=False).tolist())
    return X, y.astype(np.float64), idx, odx.cv_folds(n, FOLDS, seed=seed)


_REFS = {}


def _refs(seed=61):
    """The oracle's fold fits and held-out scores of _problem(seed), computed once: alphas[l][f] (f = FOLDS: all rows) and
    heldout[l] (n,)."""
    if seed not in _REFS:
        X, y, idx, fold_of = _problem(seed=seed)
        X64, fo = X.astype(np.float64), fold_of.numpy()
        alphas, held = [], []
        for lam in LAMS:
            row, h = [], np.zeros(len(X))
            for f in range(FOLDS):
                tr = np.nonzero(fo != f)[0]
                a = fr.falkon_fit_centers(X64[tr], y[tr], X64[idx], SIGMA, lam, len(tr), 20, np.float64, 1e-5, 1e-7)[0]
                te = np.nonzero(fo == f)[0]
                h[te] = fr.falkon_predict(X64[te], X64[idx], a, SIGMA)[:, 0]
                row.append(a[:, 0])
            row.append(fr.falkon_fit(X64, y, idx, SIGMA, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)[0][:, 0])
            alphas.append(row), held.append(h)
        _REFS[seed] = (alphas, held)
    return _REFS[seed]


def _fit(be, X, y, idx, fold_of, lams=LAMS, folds=FOLDS, **kw):
    F = be.features(torch.from_numpy(X))
    return odx.falkon_fit_cv(be, F, be.vec(y), be.rows(F, idx), SIGMA, lams, fold_of, folds, kw.pop("maxiter", 20), **kw)


def _rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("cg_scores", [True, False])
def test_fold_fits_and_heldout_scores_equal_the_oracle(cg_scores):
    """Every fold alpha against the oracle's fit on that fold's training rows alone, the refit member against its fit on all
    rows (1e-6 relative: the bound tests/test_falkon_multi_host.py holds a column to), and heldout[l, i] against
    falkon_predict of the fold's oracle alpha at 1e-9 max(1, max|ref|) — summed from the row products, and through the
    mmv route of a block scores_from_cg does not take."""
    X, y, idx, fold_of = _problem()
    ref_a, ref_h = _refs()
    be = CvBackend(cg_scores=cg_scores)
    alphas, heldout = _fit(be, X, y, idx, fold_of)
    assert tuple(alphas.shape) == (2, FOLDS + 1, len(idx)) and alphas.dtype == torch.float64
    assert tuple(heldout.shape) == (2, len(X)) and heldout.dtype == torch.float64
    assert be.calls["mmv"] == (0 if cg_scores else 1)
    for l in range(2):
        for f in range(FOLDS + 1):
            rel = _rel(alphas[l, f].numpy(), ref_a[l][f])
            print("lam %g state %d: alpha rel err %.2e" % (LAMS[l], f, rel))
            assert rel < 1e-6, (l, f, rel)
        err = np.abs(heldout[l].numpy() - ref_h[l]).max()
        bound = (1e-9 if cg_scores else 1e-6) * max(1.0, np.abs(ref_h[l]).max())      # (mmv hands back f32: its rounding, 6e-8)
        print("lam %g: held-out score err %.2e (max |ref| %.2f)" % (LAMS[l], err, np.abs(ref_h[l]).max()))
        assert err <= bound, (l, err)
    # without the refit: the fold members alone, bit for bit what they were beside it
    a2, h2 = _fit(CvBackend(cg_scores=cg_scores), X, y, idx, fold_of, refit=False)
    assert tuple(a2.shape) == (2, FOLDS, len(idx)) and torch.equal(a2, alphas[:, :FOLDS]) and torch.equal(h2, heldout)


@pytest.mark.parametrize("maxiter", [9, 10, 11, 20, 25])
def test_one_build_one_preconditioner_chain_one_pass_per_iteration(maxiter):
    X, y, idx, fold_of = _problem()
    be = CvBackend()
    _fit(be, X, y, idx, fold_of, maxiter=maxiter)
    assert be.calls["knm_rhs"] == 1 and be.calls["precond_path"] == 1 and be.calls["precond"] == 0 and be.calls["ktwn"] == 1
    assert be.calls["mmv"] == 0 and be.calls["trmv"] == 0            # every triangular product through trmvn
    full = sum(1 for it in range(maxiter - 1) if (it + 1) % 10 == 0)   # (none behind the last step)
    per_lam = maxiter + full
    assert len(be.rows_calls) == len(LAMS) * per_lam
    wrow = tuple(range(FOLDS)) + (-1,)
    for l in range(len(LAMS)):
        calls = be.rows_calls[l * per_lam:(l + 1) * per_lam]
        assert all(c[0] == FOLDS + 1 and c[1] == wrow for c in calls)
        # the direction exchange of every iteration hands out the row products; the full-residual exchange behind
        # iterations 10, 20, .. does not (it would overwrite a state's K v with K x)
        want = []
        for it in range(maxiter):
            want.append(True)
            if (it + 1) % 10 == 0 and it != maxiter - 1:
                want.append(False)
        assert [c[2] for c in calls] == want


def test_a_state_that_stops_at_once_leaves_the_others_alone():
    """Labels that are zero outside fold 0: state 0 (fitted on folds 1 and 2) has b = 0, raises its stop flag in the first
    cg_finish and returns alpha = 0; states 1, 2 and the refit still equal the oracle's fits, and the held-out scores of
    folds 1 and 2 the oracle's."""
    X, y, idx, fold_of = _problem(seed=62)
    fo = fold_of.numpy()
    y = np.where(fo == 0, y, 0.0)
    X64 = X.astype(np.float64)
    alphas, heldout = _fit(CvBackend(), X, y, idx, fold_of, lams=[1e-3])
    assert torch.count_nonzero(alphas[0, 0]) == 0 and torch.isfinite(alphas).all() and torch.isfinite(heldout).all()
    assert torch.count_nonzero(heldout[0][fold_of == 0]) == 0
    for f in (1, 2):
        tr, te = np.nonzero(fo != f)[0], np.nonzero(fo == f)[0]
        a = fr.falkon_fit_centers(X64[tr], y[tr], X64[idx], SIGMA, 1e-3, len(tr), 20, np.float64, 1e-5, 1e-7)[0]
        assert _rel(alphas[0, f].numpy(), a[:, 0]) < 1e-6, f
        p = fr.falkon_predict(X64[te], X64[idx], a, SIGMA)[:, 0]
        assert np.abs(heldout[0].numpy()[te] - p).max() <= 1e-9 * max(1.0, np.abs(p).max()), f
    a = fr.falkon_fit(X64, y, idx, SIGMA, 1e-3, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)[0]
    assert _rel(alphas[0, FOLDS].numpy(), a[:, 0]) < 1e-6


def test_refusals():
    X, y, idx, fold_of = _problem()
    n = len(X)
    with pytest.raises(ValueError, match="at least 2 folds"):
        _fit(CvBackend(), X, y, idx, torch.zeros(n, dtype=torch.int64), folds=1)
    empty = fold_of.clone()
    empty[empty == 1] = 2
    with pytest.raises(ValueError, match="fold 1 has no rows"):
        _fit(CvBackend(), X, y, idx, empty)
    with pytest.raises(ValueError, match="holds all rows"):
        _fit(CvBackend(), X, y, idx, torch.full((n,), 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="fold_of must be an integer tensor"):
        _fit(CvBackend(), X, y, idx, fold_of[:-1])
    with pytest.raises(ValueError, match="fold_of must be an integer tensor"):
        _fit(CvBackend(), X, y, idx, fold_of.double())
    for bad in (-1, FOLDS):
        wrong = fold_of.clone()
        wrong[5] = bad
        with pytest.raises(ValueError, match=r"values in \[0, 3\)"):
            _fit(CvBackend(), X, y, idx, wrong)
    for lams in ([], [1e-3, 0.0], [float("nan")], [-1e-3], [float("inf")]):
        with pytest.raises(ValueError, match="lams must be"):
            _fit(CvBackend(), X, y, idx, fold_of, lams=lams)
    with pytest.raises(ValueError, match="streamed shard"):
        _fit(CvBackend(fmt="stream"), X, y, idx, fold_of)
    with pytest.raises(NotImplementedError, match="ktkn_rows"):          # no silent slow path
        _fit(OracleBackend(np.float64), X, y, idx, fold_of)


def test_cv_folds_is_balanced_reproducible_and_leaves_the_global_rng_alone():
    torch.manual_seed(1234)
    state = torch.get_rng_state()
    a = odx.cv_folds(1003, 5, seed=7)
    assert torch.equal(torch.get_rng_state(), state)
    assert a.dtype == torch.int64 and tuple(a.shape) == (1003,)
    counts = torch.bincount(a, minlength=5)
    assert int(counts.min()) >= 1003 // 5 and int(counts.max()) <= 1003 // 5 + 1 and int(counts.sum()) == 1003
    assert torch.equal(a, odx.cv_folds(1003, 5, seed=7))
    assert not torch.equal(a, odx.cv_folds(1003, 5, seed=8))
    assert not torch.equal(a, torch.arange(1003) % 5)                # shuffled, not striped
    for n, folds in ((10, 1), (3, 4)):
        with pytest.raises(ValueError):
            odx.cv_folds(n, folds)


def test_estimator_fit_cv():
    from odx.wrappers import CenterSelector
    X, y, idx, fold_of = _problem(n=600, D=24, M=60, seed=63)
    odx.set_backend(CvBackend())
    try:
        def make():
            return odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=SIGMA), penalty=1e-3, M=len(idx), maxiter=20,
                                    center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
        Xt, Yt = torch.from_numpy(X), torch.from_numpy(y)
        tpl = make()
        torch.manual_seed(5)
        state = torch.get_rng_state()
        res = tpl.fit_cv(Xt, Yt, LAMS, folds=4, seed=3)
        assert torch.equal(torch.get_rng_state(), state)
        assert tpl.alpha_ is None and tpl.penalty == 1e-3                       # the template stays as it is
        assert torch.equal(res.fold_of, odx.cv_folds(600, 4, seed=3))
        assert tuple(res.scores.shape) == (600, 2) and res.scores.dtype == torch.float32
        assert tuple(res.fold_alphas.shape) == (2, 4, 60) and tuple(res.mse.shape) == (2,)
        want = ((res.scores.double() - Yt.double()[:, None]) ** 2).mean(0)
        assert torch.allclose(res.mse, want, rtol=1e-12, atol=0.0) and torch.isfinite(res.mse).all()
        path = make().fit_path(Xt, Yt, LAMS)
        assert len(res.estimators) == 2
        for est, ref in zip(res.estimators, path):
            assert est.penalty == ref.penalty and est.ny_points_ is res.estimators[0].ny_points_
            assert _rel(est.alpha_.numpy(), ref.alpha_.numpy()) < 1e-8
        p = odx.predict_path(res.estimators, Xt[:50])
        assert tuple(p.shape) == (50, 2)
        # the caller's own folds, and no refit
        res2 = make().fit_cv(Xt, Yt, LAMS, folds=4, fold_of=res.fold_of, refit=False)
        assert res2.estimators == [] and torch.equal(res2.scores, res.scores) and torch.equal(res2.fold_alphas, res.fold_alphas)
        with pytest.raises(ValueError, match="one right-hand side"):
            make().fit_cv(Xt, torch.stack([Yt, Yt], 1), LAMS)
    finally:
        odx.set_backend(None)
