"""odx.LeverageSelector and odx.leverage_scores on the CPU: the host logic of odx/leverage.py driven by a numpy / scipy backend,
against the f64 restatement tests/leverage_ref.py fed the same draws; the quality of the sampler against the exact ridge leverage
scores; the edges."""
import numpy as np
import pytest
import scipy.linalg as sla

torch = pytest.importorskip("torch")

import odx  # noqa: E402
from tests import leverage_ref as lr  # noqa: E402
from tests.matern_ref import radial_kernel  # noqa: E402
from tests.oracle_backend import OracleBackend  # noqa: E402
from tests.synth import blob_problem  # noqa: E402


class _Knm:
    pass


class LeverageOracleBackend(OracleBackend):
    """OracleBackend plus the three operations of the leverage scores, by numpy / scipy in f64 (K entries in f64 too, so that
    the selector's arithmetic is the restatement's)."""

    def __init__(self):
        super().__init__(dtype_k=np.float64)

    def knm(self, F, Zf, sigma, out=None):
        K = _Knm()
        K.K = torch.from_numpy(radial_kernel(F.X.numpy().astype(np.float64), Zf.X.numpy().astype(np.float64), lr._k(sigma), np.float64))
        K.n, K.M, K.ld = F.n, Zf.n, Zf.n
        return K

    def kmm_f64(self, Zf, kernel, diag=None, diag_scale=0.0):
        Z = Zf.X.numpy().astype(np.float64)
        A = radial_kernel(Z, Z, lr._k(kernel), np.float64)
        d = np.ones(len(Z)) if diag is None else np.asarray(diag, dtype=np.float64)
        return torch.from_numpy(np.tril(A + diag_scale * np.diag(d)))

    def chol_inverse(self, A):
        a = A.numpy()
        a = np.tril(a) + np.tril(a, -1).T
        L = np.linalg.cholesky(a)                      # (LinAlgError for a non-positive pivot)
        return torch.from_numpy(sla.solve_triangular(L, np.eye(len(a)), lower=True)), torch.zeros(1, dtype=torch.int32)

    def row_quad(self, K, Li, out=None):
        q = torch.from_numpy(lr.row_quad(K.K.numpy(), Li.numpy()))
        if out is not None:
            out.copy_(q)
            return out
        return q


@pytest.fixture(scope="module")
def be():
    return LeverageOracleBackend()


PROBLEMS = {"s25": (1500, 70, 25.0, 1e-3), "s40": (1500, 70, 40.0, 1e-4)}
_cache = {}


def problem(name):
    """(X f32, exact scores f64) of a quality problem: computed once, shared, never changed."""
    if name not in _cache:
        n, D, sigma, lam = PROBLEMS[name]
        X = blob_problem(n, D, seed=7)[0]
        ex = lr.exact_scores(X, sigma, lam)
        X.setflags(write=False)
        ex.setflags(write=False)
        _cache[name] = (X, ex)
    return _cache[name]


@pytest.mark.parametrize("kernel", [odx.GaussianKernel(12.0), odx.MaternKernel(12.0, 2.5), 9.0], ids=["gauss", "matern52", "width"])
def test_selector_is_the_restatement_on_the_same_draws(be, kernel):
    X = blob_problem(400, 20, seed=3)[0]
    lam, seed = 2e-3, 11
    state = torch.get_rng_state().clone()
    sel = odx.LeverageSelector(kernel, lam, None, seed=seed, backend=be)
    rows = sel.select(torch.from_numpy(X), None)
    assert torch.equal(torch.get_rng_state(), state), "the global RNG was touched"
    ref = lr.bottom_up(X, kernel, lam, lr.TorchDraws(seed))
    assert np.array_equal(sel.indices_.numpy(), ref["indices"])
    assert np.array_equal(rows.numpy(), X[ref["indices"]])
    np.testing.assert_allclose(sel.weights_.numpy(), ref["weights"], rtol=1e-12, atol=0)
    assert len(sel.levels_) == len(ref["levels"]) >= 2
    for a, b in zip(sel.levels_, ref["levels"]):
        assert (a[1], a[3], a[4]) == (b[1], b[3], b[4])
        np.testing.assert_allclose([a[0], a[2]], [b[0], b[2]], rtol=1e-12, atol=0)
    np.testing.assert_allclose(sel.d_eff_, ref["d_eff"], rtol=1e-12)
    assert np.array_equal(sel.candidates_.numpy(), ref["candidates"]) and np.array_equal(sel.prev_indices_.numpy(), ref["prev_indices"])
    np.testing.assert_allclose(sel.scores_.numpy(), ref["scores"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(sel.prev_weights_.numpy(), ref["prev_weights"], rtol=1e-12, atol=0)
    # the same seed again: the same centres; another seed: others
    again = odx.LeverageSelector(kernel, lam, None, seed=seed, backend=be)
    again.select(torch.from_numpy(X), None)
    assert torch.equal(again.indices_, sel.indices_) and torch.equal(again.weights_, sel.weights_)
    other = odx.LeverageSelector(kernel, lam, None, seed=seed + 1, backend=be)
    other.select(torch.from_numpy(X), None)
    assert not torch.equal(other.indices_, sel.indices_)


def test_leverage_scores_is_the_restatement_and_exact_with_all_rows(be):
    X = blob_problem(300, 20, seed=5)[0]
    g = np.random.default_rng(0)
    idx = g.permutation(300)[:40]
    w = g.uniform(0.5, 2.0, 40) * 40
    s, q = odx.leverage_scores(X, X[idx], 9.0, 1e-3, weights=w, n_total=1234, return_q=True, backend=be)
    rs, rq = lr.approx_scores(X, X[idx], 9.0, 1e-3, w, 1234, return_q=True)
    np.testing.assert_allclose(q.numpy(), rq, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(s.numpy(), rs, rtol=1e-9, atol=1e-18)
    # default weights: |J| each; chunked = unchunked
    s2 = odx.leverage_scores(X, X[idx], 9.0, 1e-3, backend=be)
    np.testing.assert_allclose(s2.numpy(), lr.approx_scores(X, X[idx], 9.0, 1e-3), rtol=1e-9, atol=1e-18)
    assert torch.equal(odx.leverage_scores(X, X[idx], 9.0, 1e-3, chunk_rows=64, backend=be), s2)
    # J = all rows, c = n: the ridge leverage scores themselves
    full = odx.leverage_scores(X, X, 9.0, 1e-3, backend=be)
    np.testing.assert_allclose(full.numpy(), lr.exact_scores(X, 9.0, 1e-3), rtol=1e-7, atol=1e-12)
    with pytest.raises(ValueError):
        odx.leverage_scores(X, X[idx], 9.0, 1e-3, weights=-w, backend=be)
    with pytest.raises(ValueError):
        odx.leverage_scores(X, X[idx], 9.0, 0.0, backend=be)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_quality_against_the_exact_scores(be, name, seed):
    """Default q, q1, q2, no cap.  The numpy restatement alone stayed within [1.14, 1.29] (sum ratio) and [0.24, 2.35] (pointwise)
    on these problems."""
    n, D, sigma, lam = PROBLEMS[name]
    X, exact = problem(name)
    sel = odx.LeverageSelector(odx.GaussianKernel(sigma), lam, None, seed=seed, backend=be)
    Z = sel.select(torch.from_numpy(X.copy()), None)
    approx = odx.leverage_scores(X.copy(), Z, sigma, lam, weights=sel.weights_, backend=be).numpy()
    d_eff = float(exact.sum())
    ratio = approx / exact
    print("%s seed %d: d_eff %.1f, |J| %d, sum ratio %.3f, pointwise [%.3f, %.3f], d_eff_ %.1f"
          % (name, seed, d_eff, len(sel.indices_), approx.sum() / d_eff, ratio.min(), ratio.max(), sel.d_eff_))
    assert 1.0 <= approx.sum() / d_eff <= 1.5
    assert ratio.min() >= 1.0 / 8 and ratio.max() <= 4.0
    assert len(sel.indices_) <= 3 * d_eff
    assert len(np.unique(sel.indices_.numpy())) == len(sel.indices_) and bool((sel.weights_ > 0).all())


def test_edges(be):
    X, y = blob_problem(200, 10, seed=9)[:2]
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(y.astype(np.float32))[:, None]
    # lam >= 1: one level
    sel = odx.LeverageSelector(8.0, 1.5, None, backend=be)
    assert len(sel.ladder()) == 1 and sel.ladder()[0] == 1.5
    sel.select(Xt, None)
    assert len(sel.levels_) == 1 and sel.levels_[0][1] == 2 and sel.prev_indices_.numel() == 0
    assert len(odx.LeverageSelector(8.0, 1.0, None, backend=be).ladder()) == 1
    # n < ceil(q1 / lam): every level past the first few takes all rows as candidates
    sel = odx.LeverageSelector(8.0, 1e-3, None, backend=be)
    sel.select(Xt, None)
    assert sel.levels_[-1][1] == 200 and sorted(sel.candidates_.tolist()) == list(range(200))
    assert all(lv[1] == min(200, int(np.ceil(2.0 / lv[0]))) for lv in sel.levels_)
    # a cap
    sel = odx.LeverageSelector(8.0, 1e-3, 5, backend=be)
    Z, Yz = sel.select(Xt, Yt)
    assert 1 <= len(sel.indices_) <= 5 and all(lv[3] <= 5 and lv[4] <= 5 for lv in sel.levels_)
    # select(X, Y) pairs Y with the rows
    assert torch.equal(Z, Xt[sel.indices_]) and torch.equal(Yz, Yt[sel.indices_]) and Yz.shape == (len(sel.indices_), 1)
    # n = 1
    sel = odx.LeverageSelector(8.0, 1e-2, None, backend=be)
    Z = sel.select(Xt[:1], None)
    assert sel.indices_.tolist() == [0] and Z.shape == (1, 10) and all(lv[1] == 1 and lv[4] == 1 for lv in sel.levels_)
    with pytest.raises(ValueError):
        odx.LeverageSelector(8.0, 0.0, None)
    with pytest.raises(ValueError):
        odx.LeverageSelector(8.0, 1e-3, 0)


def test_estimator_takes_the_selector(be):
    """InCoreFalkon(center_selection=LeverageSelector(...)): the estimators call select(F.X, None) and fit on the rows it hands over."""
    from odx import backend as _backend
    X, y = blob_problem(300, 12, seed=2)[:2]
    old = _backend._BACKEND
    _backend.set_backend(be)
    try:
        sel = odx.LeverageSelector(odx.GaussianKernel(9.0), 1e-3, 40, seed=4)
        est = odx.InCoreFalkon(kernel=odx.GaussianKernel(9.0), penalty=1e-3, M=40, center_selection=sel, maxiter=5)
        est.fit(torch.from_numpy(X), torch.from_numpy(y)[:, None])
        assert est.M == len(sel.indices_) <= 40
        assert np.array_equal(est.ny_points_.cpu().numpy(), X[sel.indices_.numpy()])
    finally:
        _backend.set_backend(old)
