"""Host logic of the logistic estimator (odx.falkon_fit_logistic, odx.LogisticFalkon) on the numpy oracle backend with numpy
statements of the three new backend operations (ktk_rw, logistic_rows, precond_logistic_begin / _step) and call counters,
against tests/logistic_ref.py.  No GPU."""
import copy
import os
import pickle
import re

import numpy as np
import pytest
import torch

import odx
from odx import backend as _backend
from oracle import falkon_ref as fr
from tests import logistic_ref as lr
from tests.oracle_backend import OracleBackend, _Precond
from tests.synth import blob_problem

SHAPES = [(777, 129, 36, 5.0, 1e-3), (1500, 257, 70, 5.0, 1e-4), (3000, 300, 1024, 15.0, 1e-5)]       # tests/test_gpu_incremental.py
SCHEDULES = {
    "A": [(1e-1, 3), (1e-2, 3), (1e-3, 3), (1e-4, 8), (1e-4, 8), (1e-4, 8)],
    "B": [(1e-2, 3), (1e-3, 3), (1e-4, 5), (1e-5, 8), (1e-5, 8)],
    "C": [(1e-3, 4), (1e-5, 4), (1e-6, 10), (1e-6, 10)],
}


class LogisticOracleBackend(OracleBackend):
    """The oracle backend with the logistic estimator's operations in numpy / torch f64 and counters: reads of the block
    (`reads`: one per ktk_rw, one per ktk), calls of the row kernel and of the two preconditioner parts."""

    def __init__(self, dtype_k=np.float32):
        super().__init__(dtype_k)
        self.reads = {"ktk_rw": 0, "ktk": 0, "knm_rhs": 0}
        self.calls = {"logistic_rows": 0, "begin": 0, "step": 0}
        self.rw_t_out = []

    def knm(self, F, Zf, sigma, out=None):
        K = super().knm(F, Zf, sigma, out=out)
        K.fmt = "f32"
        return K

    def knm_rhs(self, F, Zf, sigma, w, out=None, rhs_out=None):
        self.reads["knm_rhs"] += 1
        K = self.knm(F, Zf, sigma, out=out)
        return K, OracleBackend.ktk(self, K, w=w, out=rhs_out)

    def ktk(self, K, v=None, w=None, out=None):
        self.reads["ktk"] += 1
        return super().ktk(K, v=v, w=w, out=out)

    def ktk_rw(self, K, v, d, out=None, t_out=None):
        self.reads["ktk_rw"] += 1
        self.rw_t_out.append(t_out is not None)
        Kd = K.K.double()
        t = Kd @ v
        if t_out is not None:
            t_out.copy_(t)
        r = Kd.t() @ (t if d is None else d * t)
        if out is not None:
            out.copy_(r)
            return out
        return r

    def cg_scores_axpy(self, state, t, S):
        if state[2] != 0:
            return
        S.add_(state[3] * t)

    def logistic_rows(self, t, y, neg_weight, g, w, l=None):
        self.calls["logistic_rows"] += 1
        a, b, c = lr.loss_terms(y.numpy(), t.numpy(), neg_weight)
        for dst, src in ((g, a), (w, b), (l, c)):
            if dst is not None:
                dst.copy_(torch.from_numpy(src))

    def precond_logistic_begin(self, Zf, kernel, eps):
        self.calls["begin"] += 1
        Z = Zf.X.numpy().astype(np.float64)
        C = fr.gaussian_kernel(Z, Z, float(kernel), np.float64)
        C[np.diag_indices(Zf.n)] += eps * Zf.n
        st = _Precond()
        st.M = Zf.n
        st.L = torch.from_numpy(np.linalg.cholesky(C))
        Li = np.linalg.inv(st.L.numpy())
        st.LTi, st.LTit = torch.from_numpy(np.ascontiguousarray(Li)), torch.from_numpy(np.ascontiguousarray(Li.T))
        st.info = torch.zeros(1, dtype=torch.int32)
        return st

    def logistic_centre_scores(self, st, beta):
        return st.L @ beta

    def precond_logistic_step(self, st, w_M, lam):
        self.calls["step"] += 1
        L = st.L.numpy()
        AA = L.T @ (w_M.numpy()[:, None] * L) / st.M + lam * np.eye(st.M)
        LAi = np.linalg.inv(np.linalg.cholesky(AA))
        P = _Precond()
        P.M, P.ld = st.M, st.M
        P.LTi, P.LTit = st.LTi, st.LTit
        P.LAi, P.LAit = torch.from_numpy(np.ascontiguousarray(LAi)), torch.from_numpy(np.ascontiguousarray(LAi.T))
        P.info = torch.zeros(1, dtype=torch.int32)
        return P


@pytest.fixture()
def be():
    b = LogisticOracleBackend()
    old = _backend._BACKEND
    _backend.set_backend(b)
    yield b
    _backend.set_backend(old)


_cache = {}


def _problem(shape):
    """(X f32, y f64, centre indices) of a shape: blob_problem's rows and M distinct centres, once."""
    if shape not in _cache:
        n, M, D, sigma, _ = shape
        X, y, rng = blob_problem(n, D, seed=500 + n)
        idx = np.sort(rng.choice(n, M, replace=False))
        _cache[shape] = (X, y.astype(np.float64), idx)
    return _cache[shape]


def _fit(be, shape, sched, nw, objective_out=None):
    X, y, idx = _problem(shape)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    return odx.falkon_fit_logistic(be, F, be.vec(y), Zf, be.vec(y[idx]), shape[3], [p for p, _ in sched], [m for _, m in sched],
                                   odx.LogisticLoss(nw), objective_out=objective_out).numpy()


def _rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("nw", [1.0, 0.25])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d" % s[:2])
def test_alpha_is_the_reference_and_the_objective_never_rises(be, shape, name, nw):
    """(a) alpha within 1e-4 relative of logistic_ref on f64 entries (the oracle backend evaluates K in f32: the tile cores'
    entry error) and within 1e-6 on the same block via knm=; (b) the recorded objective never rises; (d) the block is read
    iter + 1 times per step, plus once per periodic full residual."""
    sched = SCHEDULES[name]
    X, y, idx = _problem(shape)
    pens, its = [p for p, _ in sched], [m for _, m in sched]
    obj = []
    alpha = _fit(be, shape, sched, nw, objective_out=obj)
    X64 = X.astype(np.float64)
    ref = lr.logistic_fit(X64, y, X64[idx], y[idx], shape[3], pens, its, nw)
    same = lr.logistic_fit(X64, y, X64[idx], y[idx], shape[3], pens, its, nw,
                           knm=fr.gaussian_kernel(X, X[idx], shape[3], np.float32))
    r64, rsame = _rel(alpha, ref), _rel(alpha, same)
    print("logistic host %s %s nw=%g: alpha vs f64 %.2e, vs same block %.2e" % (shape[:2], name, nw, r64, rsame))
    assert r64 < 1e-4
    assert rsame < 1e-6
    assert len(obj) == len(sched) + 1
    assert all(b <= a for a, b in zip(obj, obj[1:])), obj
    # reads: step 0's K' g / n comes out of the build; every later step has one ktk; per step m products and one full
    # residual per completed group of 10 iterations that is not the last iteration
    assert be.reads["knm_rhs"] == 1 and be.reads["ktk"] == len(sched) - 1
    assert be.reads["ktk_rw"] == sum(m + (m - 1) // 10 for m in its)
    assert sum(be.rw_t_out) == sum(its)          # the direction passes hand out their row products, the residual's does not
    assert be.calls["begin"] == 1 and be.calls["step"] == len(sched)


@pytest.mark.parametrize("lam", [1e-2, 1e-3])
@pytest.mark.parametrize("shape", SHAPES[:2] + [(2000, 256, 256, 10.0, 0.0)], ids=lambda s: "n%d-M%d" % s[:2])
def test_the_oracle_converges_to_the_dense_newton_solution(shape, lam):
    """(c) the oracle alone: eight Newton steps of 20 CG iterations end within 1e-3 relative of the dense Newton minimiser of
    the same objective (cg_epsilon keeps it from going lower)."""
    X, y, idx = _problem(shape)
    X64 = X.astype(np.float64)
    a = lr.logistic_fit(X64, y, X64[idx], y[idx], shape[3], [lam] * 8, [20] * 8, 0.25)
    ref = lr.dense_newton(X64, y, X64[idx], shape[3], lam, 0.25)
    r = _rel(a, ref)
    print("logistic oracle %s lam=%g: vs dense Newton %.2e" % (shape[:2], lam, r))
    assert r < 1e-3


def _est(**kw):
    args = dict(kernel=odx.GaussianKernel(5.0), penalty_list=[1e-2, 1e-3], iter_list=[3, 3], M=40)
    args.update(kw)
    return odx.LogisticFalkon(**args)


def test_estimator_fits_predicts_and_pickles(be, tmp_path):
    X, y, _ = _problem(SHAPES[0])
    Xt = torch.from_numpy(X)
    torch.manual_seed(3)
    est = _est(loss=odx.LogisticLoss(0.25), record_objective=True).fit(Xt, torch.from_numpy(y))
    assert tuple(est.alpha_.shape) == (40, 1) and tuple(est.ny_points_.shape) == (40, X.shape[1])
    assert len(est.objective_) == 3 and est.objective_[0] >= est.objective_[-1]
    s, p = est.predict(Xt), est.predict_proba(Xt)
    assert tuple(p.shape) == (len(X), 1)
    assert torch.equal(p, torch.sigmoid(s))
    assert float(((s[:, 0] > 0).double() * 2 - 1 == torch.from_numpy(y)).double().mean()) > 0.9
    again = pickle.loads(pickle.dumps(est))
    assert torch.equal(again.alpha_, est.alpha_) and again.loss.neg_weight == 0.25 and again.penalty_list == [1e-2, 1e-3]
    assert torch.equal(again.predict(Xt), s)
    both = odx.predict_path([est, copy.copy(est)], Xt)
    assert torch.equal(both[:, :1], s) and torch.equal(both[:, 1:], s)
    from odx import storage
    storage.save_models(str(tmp_path), "detector", classifier=[est])
    back = storage.load_models(str(tmp_path), "detector")[0][0]
    assert isinstance(back, odx.LogisticFalkon) and torch.equal(back.predict(Xt), s)
    # the seed fixes the uniform selection
    a, b = _est(seed=7).fit(Xt, y), _est(seed=7).fit(Xt, y)
    assert torch.equal(a.ny_points_, b.ny_points_) and torch.equal(a.alpha_, b.alpha_)


def test_a_selector_hands_the_centres_with_their_labels(be):
    X, y, idx = _problem(SHAPES[0])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)

    class Sel:
        def select(self, Xs, Ys):
            assert Ys is not None and Ys.shape[0] == Xs.shape[0]
            return Xs[idx], Ys[idx]

    class NoLabels:
        def select(self, Xs, Ys):
            return Xs[idx]

    est = _est(M=None, center_selection=Sel()).fit(Xt, yt)
    sched = [(1e-2, 3), (1e-3, 3)]
    assert est.M == len(idx)
    assert _rel(est.alpha_.numpy(), _fit(be, SHAPES[0], sched, 1.0)) < 1e-12
    with pytest.raises(ValueError, match="Y_Z"):
        _est(M=None, center_selection=NoLabels()).fit(Xt, yt)


def test_refusals(be):
    X, y, _ = _problem(SHAPES[0])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    with pytest.raises(ValueError, match="-1 or \\+1"):
        _est().fit(Xt, torch.where(yt > 0, yt, torch.zeros_like(yt)))
    with pytest.raises(ValueError, match="one length"):
        _est(penalty_list=[1e-2], iter_list=[3, 3])
    with pytest.raises(ValueError, match="non-empty"):
        _est(penalty_list=[], iter_list=[])
    with pytest.raises(ValueError, match="penalty"):
        _est(penalty_list=[1e-2, 0.0])
    with pytest.raises(ValueError, match="iteration"):
        _est(iter_list=[3, 0])
    with pytest.raises(ValueError, match="neg_weight"):
        odx.LogisticLoss(0.0)
    with pytest.raises(ValueError, match="one label column"):
        _est().fit(Xt, torch.stack([yt, yt], 1))
    be.knm_storage = "stream"
    with pytest.raises(ValueError, match="stream"):
        _est().fit(Xt, yt)
    be.knm_storage = "auto"
    be.native16 = True
    with pytest.raises(ValueError, match="16-bit"):
        _est().fit(Xt.to(torch.bfloat16), yt)
    be.native16 = False
    for name in ("fit_multi", "fit_path", "fit_cv", "fit_grid"):
        with pytest.raises(NotImplementedError):
            getattr(_est(), name)(Xt, yt, [1e-3])


def test_a_streamed_shard_is_refused_by_the_solver(be):
    X, y, idx = _problem(SHAPES[0])
    F = be.features(torch.from_numpy(X))
    knm = be.knm

    def streamed(*a, **kw):
        K = knm(*a, **kw)
        K.fmt = "stream"
        return K
    be.knm = streamed
    with pytest.raises(ValueError, match="stored"):
        odx.falkon_fit_logistic(be, F, be.vec(y), be.rows(F, idx), be.vec(y[idx]), 5.0, [1e-2], [2], odx.LogisticLoss())


def test_the_two_entries_are_bound_with_the_headers_argument_counts():
    from odx import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "odx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("odx_knm_fwd_bwd_rw", "odx_logistic_rows_f64"):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
        assert m, name
        assert len(hip.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    # the weighted pass reuses its twin's workspace: no query of its own
    assert "odx_knm_fwd_bwd_rw_workspace_bytes" not in hip.SIGNATURES and "odx_knm_fwd_bwd_rw_workspace_bytes" not in header
