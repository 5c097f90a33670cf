"""Host logic of the sample-weighted fit (odx.falkon_fit_weighted, odx.Falkon(weight_fn=...)) on the numpy oracle backend with
numpy statements of the backend operations it uses (ktk_w, precond_logistic_begin / _step) and call counters, against
tests/weighted_ref.py; and that reference against a dense solve of the same normal equations.  No GPU."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import odx
from odx import backend as _backend
from oracle import falkon_ref as fr
from tests import weighted_ref as wr
from tests.oracle_backend import OracleBackend, _Precond
from tests.synth import blob_problem

SHAPES = [(777, 129, 36, 5.0, 1e-3), (1500, 257, 70, 5.0, 1e-4), (3000, 300, 1024, 15.0, 1e-5)]       # tests/test_logistic_host.py


class WeightedOracleBackend(OracleBackend):
    """The oracle backend with the weighted fit's operations in numpy / torch f64 and counters: reads of the block (one per
    ktk_w), whether a pass handed out its row products, and the calls of the two preconditioner parts."""
    gauss = "h2"          # (with fmt "f32" below: solver.scores_from_cg holds, as on the GPU's f32 blocks)

    def __init__(self, dtype_k=np.float32):
        super().__init__(dtype_k)
        self.reads = {"ktk_w": 0, "ktk": 0, "knm_rhs": 0}
        self.calls = {"begin": 0, "step": 0}
        self.w_t_out = []
        self.step_weights = None

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

    def ktk_w(self, K, v, d, out=None, t_out=None):
        self.reads["ktk_w"] += 1
        self.w_t_out.append(t_out is not None)
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

    def cg_scores_store(self, S, out):
        out.copy_(S)

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

    def precond_logistic_step(self, st, w_M, lam):
        self.calls["step"] += 1
        self.step_weights = w_M.clone()
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
    b = WeightedOracleBackend()
    old = _backend._BACKEND
    _backend.set_backend(b)
    yield b
    _backend.set_backend(old)


_cache = {}


def _problem(shape):
    """(X f32, y f64, centre indices, row weights) of a shape, once: blob_problem's rows, M distinct centres, and weights
    (9 on the positives, 1 otherwise) x U(0.5, 1.5) with a few zeros."""
    if shape not in _cache:
        n, M, D, sigma, _ = shape
        X, y, rng = blob_problem(n, D, seed=500 + n)
        idx = np.sort(rng.choice(n, M, replace=False))
        w = np.where(y > 0, 9.0, 1.0) * rng.uniform(0.5, 1.5, n)
        w[rng.random(n) < 0.02] = 0.0
        _cache[shape] = (X, y.astype(np.float64), idx, w)
    return _cache[shape]


def _rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def _fit(be, shape, maxiter=20, **kw):
    X, y, idx, w = _problem(shape)
    F = be.features(torch.from_numpy(X))
    return odx.falkon_fit_weighted(be, F, be.vec(y), be.vec(w), be.rows(F, idx), be.vec(w[idx]), shape[3], shape[4], maxiter, **kw).numpy()


# ------------------------------------------------------------------ 1. the reference against the dense solve
def test_the_reference_is_the_dense_weighted_solution_on_scores():
    """alpha is ill-determined (K_MM's small eigenvalues), the scores K alpha are not: within 1e-2 relative of the dense
    solve's after 20 iterations (an f64 study of this shape measured 3.5e-4: an algebra pin, not a precision bar); and the
    weights matter: the weighted and the unweighted alpha differ by more than 0.1 relative (measured: 0.98)."""
    n, D, M, sigma, lam = 3000, 64, 300, 15.0, 1e-3
    X, y, rng = blob_problem(n, D, 7)
    X, y = X.astype(np.float64), y.astype(np.float64)
    idx = np.sort(rng.choice(n, M, replace=False))
    w = np.where(y > 0, 9.0, 1.0) * rng.uniform(0.5, 1.5, n)
    Z = X[idx]
    K, Kmm = fr.gaussian_kernel(X, Z, sigma, np.float64), fr.gaussian_kernel(Z, Z, sigma, np.float64)
    a = wr.weighted_fit(X, y, w, Z, w[idx], sigma, lam, 20)
    dense = wr.dense_weighted(K, Kmm, y, w, lam, 1e-5)
    plain = wr.weighted_fit(X, y, np.ones(n), Z, np.ones(M), sigma, lam, 20)
    unweighted = fr.falkon_fit(X, y, idx, sigma, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)[0]
    r_scores, r_w, r_ones = _rel(K @ a, K @ dense), _rel(a, plain), _rel(plain, unweighted)
    print("weighted oracle: scores vs dense %.2e, weighted vs unweighted alpha %.2e, ones vs falkon_ref %.2e" % (r_scores, r_w, r_ones))
    assert r_scores < 1e-2
    assert r_w > 0.1
    assert r_ones < 1e-9          # weights of one: falkon_ref's own fit (the same algebra, A without weights)


# ------------------------------------------------------------------ 2. the solver on the oracle backend
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d" % s[:2])
def test_alpha_is_the_reference(be, shape):
    """alpha within 1e-4 relative of weighted_ref on f64 entries (the oracle backend evaluates K in f32: the tile cores' entry
    error) and within 1e-6 on the same block via knm= — the bars of tests/test_logistic_host.py for the same comparison; 21
    reads of the block for the default 20 iterations, the residual's pass without row products; the A factor made from the
    centres' weights."""
    X, y, idx, w = _problem(shape)
    S = torch.full((len(X),), float("nan"), dtype=torch.float64)
    blocks = []
    alpha = _fit(be, shape, scores_out=S, knm_blocks=blocks)
    X64 = X.astype(np.float64)
    ref = wr.weighted_fit(X64, y, w, X64[idx], w[idx], shape[3], shape[4], 20)[:, 0]
    K32 = fr.gaussian_kernel(X, X[idx], shape[3], np.float32)
    same = wr.weighted_fit(X64, y, w, X64[idx], w[idx], shape[3], shape[4], 20, knm=K32)[:, 0]
    r64, rsame = _rel(alpha, ref), _rel(alpha, same)
    rs = float(np.abs(S.numpy() - K32.astype(np.float64) @ alpha).max())
    print("weighted host %s: alpha vs f64 %.2e, vs same block %.2e, scores_out err %.2e" % (shape[:2], r64, rsame, rs))
    assert r64 < 1e-4
    assert rsame < 1e-6
    assert rs < 1e-9 * max(1.0, float(np.abs(S.numpy()).max()))
    assert be.reads == {"ktk_w": 21, "ktk": 0, "knm_rhs": 1}
    assert sum(be.w_t_out) == 20 and be.w_t_out[10] is False          # iteration 10: its step, then the full residual
    assert be.calls == {"begin": 1, "step": 1}
    assert np.array_equal(be.step_weights.numpy(), w[idx])
    assert len(blocks) == 1 and blocks[0].n == len(X)


def test_iteration_counts_and_no_scores(be):
    _fit(be, SHAPES[0], maxiter=7)
    assert be.reads["ktk_w"] == 7 and be.w_t_out == [False] * 7
    be.reads["ktk_w"] = 0
    _fit(be, SHAPES[0], maxiter=10)          # the full residual of the last iteration is not taken
    assert be.reads["ktk_w"] == 10


# ------------------------------------------------------------------ 3. the estimator
class Weigh:
    """falkon's weight_fn: 9 on the positives, 1 otherwise; records its calls."""

    def __init__(self):
        self.seen = []

    def __call__(self, Y, X, indices):
        self.seen.append((tuple(Y.shape), tuple(X.shape), None if indices is None else torch.as_tensor(indices).clone()))
        return torch.where(torch.as_tensor(Y).reshape(-1) > 0, 9.0, 1.0)


class Pick:
    def __init__(self, idx, with_idx=True):
        self.idx, self.with_idx = torch.as_tensor(np.asarray(idx)), with_idx

    def select(self, Xs, Ys):
        if Ys is None:                      # an estimator without a weight_fn asks for the centres alone, as ever
            return Xs[self.idx]
        assert Ys.shape[0] == Xs.shape[0]
        return (Xs[self.idx], Ys[self.idx], self.idx) if self.with_idx else (Xs[self.idx], Ys[self.idx])


def _est(cls=None, **kw):
    args = dict(kernel=odx.GaussianKernel(5.0), penalty=1e-3, M=40, maxiter=5)
    args.update(kw)
    return (cls or odx.Falkon)(**args)


@pytest.mark.parametrize("cls", [odx.Falkon, odx.InCoreFalkon])
def test_weight_fn_is_called_with_rows_then_centres_and_the_model_is_the_function_level_fit(be, cls):
    X, y, idx, _ = _problem(SHAPES[0])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    fn = Weigh()
    est = _est(cls, M=None, center_selection=Pick(idx), weight_fn=fn).fit(Xt, yt)
    n, D, M = len(X), X.shape[1], len(idx)
    assert [s[:2] for s in fn.seen] == [((n, 1), (n, D)), ((M, 1), (M, D))]
    assert fn.seen[0][2] is None and torch.equal(fn.seen[1][2], torch.as_tensor(idx))
    assert est.M == M and tuple(est.alpha_.shape) == (M, 1) and tuple(est.ny_points_.shape) == (M, D)
    w = np.where(y > 0, 9.0, 1.0)
    F = be.features(Xt)
    direct = odx.falkon_fit_weighted(be, F, be.vec(y), be.vec(w), be.rows(F, idx), be.vec(w[idx]), 5.0, 1e-3, 5).numpy()
    assert _rel(est.alpha_.numpy()[:, 0], direct) < 1e-12
    plain = _est(cls, M=None, center_selection=Pick(idx)).fit(Xt, yt)
    assert _rel(est.alpha_.numpy(), plain.alpha_.numpy()) > 0.1
    # a selector without the indices: the centres' weight_fn call gets None
    fn2 = Weigh()
    other = _est(cls, M=None, center_selection=Pick(idx, with_idx=False), weight_fn=fn2).fit(Xt, yt)
    assert fn2.seen[1][2] is None and torch.equal(other.alpha_, est.alpha_)


def test_uniform_selection_hands_weight_fn_the_indices_and_the_model_pickles(be):
    X, y, _, _ = _problem(SHAPES[0])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    fn = Weigh()
    est = _est(seed=7, weight_fn=fn).fit(Xt, yt)
    idx = fn.seen[1][2]
    assert idx.numel() == 40 and torch.equal(est.ny_points_, Xt[idx])
    again = _est(seed=7, weight_fn=Weigh()).fit(Xt, yt)
    assert torch.equal(again.alpha_, est.alpha_)
    back = pickle.loads(pickle.dumps(est))
    assert isinstance(back.weight_fn, Weigh) and torch.equal(back.alpha_, est.alpha_)
    assert torch.equal(back.predict(Xt), est.predict(Xt))
    # weight_fn=None is the estimator as it was
    torch.manual_seed(11)
    a = _est().fit(Xt, yt)
    torch.manual_seed(11)
    b = _est(weight_fn=None).fit(Xt, yt)
    assert torch.equal(a.alpha_, b.alpha_) and be.reads["ktk_w"] == 2 * 5


def test_the_selector_contract(be):
    X, y, idx, _ = _problem(SHAPES[0])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)

    class NoLabels:
        def select(self, Xs, Ys):
            return Xs[idx]

    class ShortLabels:
        def select(self, Xs, Ys):
            return Xs[idx], Ys[idx[:-1]]

    with pytest.raises(ValueError, match="Y_Z"):
        _est(M=None, center_selection=NoLabels(), weight_fn=Weigh()).fit(Xt, yt)
    with pytest.raises(ValueError, match="labels"):
        _est(M=None, center_selection=ShortLabels(), weight_fn=Weigh()).fit(Xt, yt)
    # without a weight_fn the same selector is called as ever, with no labels
    assert _est(M=None, center_selection=NoLabels()).fit(Xt, yt).M == len(idx)


def test_refusals(be):
    X, y, idx, w = _problem(SHAPES[0])
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    # the estimator's checks of the weights
    for bad, what in ((lambda Y, X_, i: -torch.ones(Y.shape[0]), "finite and >= 0"),
                      (lambda Y, X_, i: torch.full((Y.shape[0],), float("nan")), "finite and >= 0"),
                      (lambda Y, X_, i: torch.zeros(Y.shape[0]), "positive sum"),
                      (lambda Y, X_, i: torch.ones(Y.shape[0] + 1), "expected")):
        with pytest.raises(ValueError, match=what):
            _est(weight_fn=bad).fit(Xt, yt)
    with pytest.raises(ValueError, match="one right-hand side"):
        _est(weight_fn=Weigh()).fit(Xt, torch.stack([yt, yt], 1))
    # the fit methods that know no weights
    for name, args in (("fit_multi", ()), ("fit_path", ([1e-3],)), ("fit_cv", ([1e-3],)), ("fit_grid", ([5.0], [1e-3]))):
        with pytest.raises(NotImplementedError, match="weight"):
            getattr(_est(weight_fn=Weigh()), name)(Xt, yt, *args)
    from odx.falkon import BatchFit, fit_batch
    with pytest.raises(NotImplementedError, match="weight"):
        fit_batch([_est(), _est(weight_fn=Weigh())], [Xt, Xt], [yt, yt])
    with pytest.raises(NotImplementedError, match="weight"):
        BatchFit().add([_est(weight_fn=Weigh())], [Xt], [yt])
    # the solver's
    F = be.features(Xt)
    Zf = be.rows(F, idx)
    args = (be.vec(y), be.vec(w), Zf, be.vec(w[idx]), 5.0, 1e-3, 3)
    with pytest.raises(ValueError, match="allreduce"):
        odx.falkon_fit_weighted(be, F, *args, allreduce=lambda v: v)
    with pytest.raises(ValueError, match="shard"):
        odx.falkon_fit_weighted(be, F, *args, shard=object())
    be.knm_storage = "stream"
    with pytest.raises(ValueError, match="stream"):
        odx.falkon_fit_weighted(be, F, *args)
    with pytest.raises(ValueError, match="stream"):
        _est(weight_fn=Weigh()).fit(Xt, yt)
    be.knm_storage = "auto"
    Zf.cmap = object()
    with pytest.raises(ValueError, match="column map"):
        odx.falkon_fit_weighted(be, F, *args)
    Zf.cmap = None
    F.b16 = True
    with pytest.raises(ValueError, match="16-bit"):
        odx.falkon_fit_weighted(be, F, *args)
    F.b16 = False
    with pytest.raises(ValueError, match="w_centres"):
        odx.falkon_fit_weighted(be, F, be.vec(y), be.vec(w), Zf, be.vec(w[idx[:-1]]), 5.0, 1e-3, 3)
    assert be.reads["ktk_w"] == 0


def test_a_streamed_or_mapped_block_is_refused_by_the_solver(be):
    X, y, idx, w = _problem(SHAPES[0])
    F = be.features(torch.from_numpy(X))
    knm = be.knm
    for attr, value, what in (("fmt", "stream", "stored"), ("cmap", object(), "column map")):
        def built(*a, **kw):
            K = knm(*a, **kw)
            setattr(K, attr, value)
            return K
        be.knm = built
        with pytest.raises(ValueError, match=what):
            odx.falkon_fit_weighted(be, F, be.vec(y), be.vec(w), be.rows(F, idx), be.vec(w[idx]), 5.0, 1e-3, 3)


# ------------------------------------------------------------------ 4. the bindings
def test_the_entry_is_bound_with_the_headers_argument_count():
    """odx_knm_fwd_bwd_q_rw and the twin whose slabs it takes (odx_knm_fwd_bwd_q_workspace_bytes: the entry has no query of
    its own, as odx_knm_fwd_bwd_rw has none — tests/test_workspace_guard_host.py holds every query the header declares to a
    case of tests/test_gpu_workspace_contract.py)."""
    from odx import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "odx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("odx_knm_fwd_bwd_q_rw", "odx_knm_fwd_bwd_q_workspace_bytes"):
        m = re.search(r"\bint(?:64_t)?\s+%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
        assert m, name
        assert len(hip.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
    assert "odx_knm_fwd_bwd_q_rw_workspace_bytes" not in hip.SIGNATURES and "odx_knm_fwd_bwd_q_rw_workspace_bytes" not in header
    from odx.weighted_ops import WeightedOps
    assert WeightedOps.rw_q_min_columns == 5085
    assert issubclass(_backend.HipBackend, WeightedOps)
