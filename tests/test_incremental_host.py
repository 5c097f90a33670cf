"""odx.IncrementalFalkon and solver.falkon_fit_stats on the CPU: the host logic of odx/incremental.py driven by the numpy oracle
backend plus numpy f64 statements of the two new backend operations (knm_gram, symv), against oracle/falkon_ref in f64 on the
rows the statistics hold.  The K entries are rounded to f32 (OracleBackend's default), as the product's are."""
import copy
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import odx  # noqa: E402
from odx import backend as _backend  # noqa: E402
from oracle import falkon_ref as fr  # noqa: E402
from tests.oracle_backend import OracleBackend  # noqa: E402
from tests.synth import blob_problem, centres  # noqa: E402


class IncrementalOracleBackend(OracleBackend):
    """OracleBackend plus knm_gram and symv in numpy f64 (the lower triangle computed and mirrored, w folded into one operand, as
    odx_knm_gram_f64 does), and call counters."""

    def __init__(self):
        super().__init__()
        self.calls = {"knm": 0, "knm_gram": 0, "symv": 0, "precond": 0, "ktk": 0}

    def knm(self, F, Zf, sigma, out=None):
        self.calls["knm"] += 1
        return super().knm(F, Zf, sigma, out=out)

    def ktk(self, *a, **k):
        self.calls["ktk"] += 1
        return super().ktk(*a, **k)

    def precond(self, Zf, sigma, lam, eps):
        self.calls["precond"] += 1
        return super().precond(Zf, sigma, lam, eps)

    def knm_gram(self, K, w=None, y=None, beta=1.0, G=None, b=None):
        self.calls["knm_gram"] += 1
        Kd = K.K.numpy().astype(np.float64)
        n, M = Kd.shape
        wv = np.ones(n) if w is None else w.numpy()[:n]
        g = (wv[:, None] * Kd).T @ Kd
        g = np.tril(g) + np.tril(g, -1).T
        if G is None:
            G, beta = torch.zeros((M, M), dtype=torch.float64), 0.0
            if y is not None and b is None:
                b = torch.zeros(M, dtype=torch.float64)
        Gn = G.numpy()
        Gn[:M, :M] = g + (beta * Gn[:M, :M] if beta != 0.0 else 0.0)
        if y is not None:
            bn = b.numpy()
            bn[:M] = Kd.T @ (wv * y.numpy()[:n]) + (beta * bn[:M] if beta != 0.0 else 0.0)
        return G, b

    def symv(self, G, X, alpha=1.0, out=None):
        self.calls["symv"] += 1
        M = G.shape[0]
        r = alpha * (X[:, :M] @ G[:, :M].t())
        if out is None:
            out = torch.zeros_like(X)
        out[:, :M] = r
        return out


@pytest.fixture()
def be():
    b = IncrementalOracleBackend()
    old = _backend._BACKEND
    _backend.set_backend(b)
    yield b
    _backend.set_backend(old)


SHAPES = [(777, 129, 36, 5.0, 1e-3), (1500, 257, 70, 5.0, 1e-4), (3000, 300, 1024, 15.0, 1e-5)]
_cache = {}


def problem(shape):
    """(X, y, Z, cuts) of a parity shape — three uneven batches — computed once, shared, never changed."""
    if shape not in _cache:
        n, M, D, sigma, lam = shape
        X, y, rng = blob_problem(n, D, seed=n + M)
        Z = np.ascontiguousarray(X[centres(y, M, rng)])
        cuts = (0, n // 2 + 7, n // 2 + 7 + n // 5, n)
        for a in (X, y, Z):
            a.setflags(write=False)
        _cache[shape] = (X, y, Z, cuts)
    return _cache[shape]


def oracle_alpha(X, y, Z, sigma, lam, rows=None):
    X, y = (X, y) if rows is None else (X[rows], y[rows])
    return fr.falkon_fit_centers(X.astype(np.float64), y.astype(np.float64), Z.astype(np.float64), sigma, lam, len(X), maxiter=20,
                                 dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)[0][:, 0]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def T(a):
    return torch.from_numpy(np.array(a))


def model(shape, Z, **kw):
    n, M, D, sigma, lam = shape
    return odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, centres=T(Z), **kw)


def feed(est, X, y, cuts, batches=(0, 1, 2), **kw):
    for i in batches:
        est.partial_fit(T(X[cuts[i]:cuts[i + 1]]), T(y[cuts[i]:cuts[i + 1]])[:, None], **kw)
    return est


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d" % s[:2])
def test_three_batches_give_the_oracle_on_all_rows_and_removal_the_oracle_on_the_rest(be, shape):
    n, M, D, sigma, lam = shape
    X, y, Z, cuts = problem(shape)
    est = feed(model(shape, Z), X, y, cuts)
    assert est.n_seen_ == n and tuple(est.alpha_.shape) == (M, 1) and est.gram_.shape[0] == M and est.rhs_.shape[0] == M
    assert be.calls["precond"] == 1 and be.calls["knm"] == 3 and be.calls["ktk"] == 0
    assert torch.equal(est.gram_[:, :M], est.gram_[:, :M].t())
    r = rel(est.alpha_.numpy(), oracle_alpha(X, y, Z, sigma, lam))
    print("after adding: alpha rel err %.2e" % r)
    assert r < 1e-4, r
    est.remove(T(X[cuts[2]:]), T(y[cuts[2]:])[:, None])
    assert est.n_seen_ == cuts[2] and be.calls["precond"] == 1
    r = rel(est.alpha_.numpy(), oracle_alpha(X, y, Z, sigma, lam, slice(0, cuts[2])))
    print("after removing the last batch: alpha rel err %.2e" % r)
    assert r < 1e-4, r
    assert np.array_equal(est.ny_points_.numpy(), Z)


def test_weight_two_is_the_row_given_twice(be):
    shape = SHAPES[0]
    X, y, Z, cuts = problem(shape)
    sub = np.arange(0, len(X), 3)
    w = np.ones(len(X))
    w[sub] = 2.0
    a = model(shape, Z).partial_fit(T(X), T(y)[:, None], sample_weight=T(w))
    b = model(shape, Z).partial_fit(T(np.concatenate([X, X[sub]])), T(np.concatenate([y, y[sub]]))[:, None])
    assert a.n_seen_ == b.n_seen_ == len(X) + len(sub)
    r = rel(a.alpha_.numpy(), b.alpha_.numpy())
    print("weights: alpha rel diff %.2e" % r)
    assert r < 1e-10, r


def test_decay_zero_is_a_fresh_model_on_the_batch(be):
    shape = SHAPES[0]
    X, y, Z, cuts = problem(shape)
    a = feed(model(shape, Z), X, y, cuts, batches=(0,))
    a.partial_fit(T(X[cuts[1]:cuts[2]]), T(y[cuts[1]:cuts[2]])[:, None], decay=0.0)
    b = feed(model(shape, Z), X, y, cuts, batches=(1,))
    assert a.n_seen_ == b.n_seen_ == cuts[2] - cuts[1]
    assert torch.equal(a.gram_, b.gram_) and torch.equal(a.rhs_, b.rhs_) and torch.equal(a.alpha_, b.alpha_)
    # a decay in between scales all three
    c = feed(model(shape, Z), X, y, cuts, batches=(0,))
    c.partial_fit(T(X[cuts[1]:cuts[2]]), T(y[cuts[1]:cuts[2]])[:, None], decay=0.5, solve=False)
    assert c.n_seen_ == 0.5 * cuts[1] + (cuts[2] - cuts[1])
    first = feed(model(shape, Z), X, y, cuts, batches=(0,))
    np.testing.assert_allclose(c.gram_.numpy(), 0.5 * first.gram_.numpy() + b.gram_.numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(c.rhs_.numpy(), 0.5 * first.rhs_.numpy() + b.rhs_.numpy(), rtol=1e-13, atol=1e-13)
    with pytest.raises(ValueError, match="decay"):
        c.partial_fit(T(X[:10]), T(y[:10])[:, None], decay=1.5)


def test_a_new_penalty_uses_the_same_statistics_and_builds_no_block(be):
    shape = SHAPES[1]
    n, M, D, sigma, lam = shape
    X, y, Z, cuts = problem(shape)
    est = feed(model(shape, Z), X, y, cuts, solve=False)
    assert est.alpha_ is None and be.calls["precond"] == 0 and be.calls["symv"] == 0
    est.solve()
    before = dict(be.calls)
    G0 = est.gram_.clone()
    est.solve(penalty=1e-3)
    assert est.penalty == 1e-3
    assert be.calls["knm"] == before["knm"] and be.calls["knm_gram"] == before["knm_gram"] and be.calls["ktk"] == 0
    assert be.calls["precond"] == before["precond"] + 1 and torch.equal(est.gram_, G0)
    # 20 iterations: 19 directions, two of them with the folded full residual's second vector, all in one symv each
    assert be.calls["symv"] - before["symv"] == 20
    r = rel(est.alpha_.numpy(), oracle_alpha(X, y, Z, sigma, 1e-3))
    print("new penalty: alpha rel err %.2e" % r)
    assert r < 1e-4, r
    est.solve()                      # the same penalty again: the preconditioner is kept
    assert be.calls["precond"] == before["precond"] + 1


def test_chunking_does_not_change_the_model(be):
    shape = SHAPES[0]
    X, y, Z, cuts = problem(shape)
    a = model(shape, Z, chunk_rows=100).partial_fit(T(X), T(y)[:, None])
    assert be.calls["knm"] == 8 and be.calls["knm_gram"] == 8
    b = model(shape, Z, chunk_rows=10000).partial_fit(T(X), T(y)[:, None])
    assert be.calls["knm"] == 9
    r = rel(a.alpha_.numpy(), b.alpha_.numpy())
    print("chunking: alpha rel diff %.2e" % r)
    assert r < 1e-10, r


def test_centres_are_selected_once_as_fit_selects_them(be):
    shape = SHAPES[0]
    n, M, D, sigma, lam = shape
    X, y, Z, cuts = problem(shape)
    torch.manual_seed(5)
    ref = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma), penalty=lam, M=50, maxiter=2).fit(T(X[:cuts[1]]), T(y[:cuts[1]])[:, None])
    state = torch.get_rng_state().clone()
    torch.manual_seed(5)
    est = odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, M=50)
    est.partial_fit(T(X[:cuts[1]]), T(y[:cuts[1]])[:, None])
    assert torch.equal(torch.get_rng_state(), state), "the global RNG is not where fit leaves it"
    assert torch.equal(est.ny_points_, ref.ny_points_) and est.M == 50
    ny = est.ny_points_
    est.partial_fit(T(X[cuts[1]:]), T(y[cuts[1]:])[:, None])
    assert torch.equal(torch.get_rng_state(), state) and est.ny_points_ is ny
    # a selector object: asked once
    class Sel:
        asked = 0

        def select(self, Xs, Ys):
            Sel.asked += 1
            return Xs[:40]
    est = odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, center_selection=Sel())
    feed(est, X, y, cuts)
    assert Sel.asked == 1 and est.M == 40 and np.array_equal(est.ny_points_.numpy(), X[:40])


def test_refusals(be):
    shape = SHAPES[0]
    n, M, D, sigma, lam = shape
    X, y, Z, cuts = problem(shape)
    Xt, Yt = T(X[:200]), T(y[:200])[:, None]
    with pytest.raises(ValueError, match="GaussianKernel or a MaternKernel"):
        odx.IncrementalFalkon(5.0, lam, M=10)
    with pytest.raises(ValueError, match="centres, or M"):
        odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam)
    est = model(shape, Z)
    be.native16 = True
    with pytest.raises(ValueError, match="16-bit native rows"):
        est.partial_fit(Xt.to(torch.bfloat16), Yt)
    be.native16 = False
    be.knm_storage = "stream"
    with pytest.raises(ValueError, match="knm_storage='stream'"):
        est.partial_fit(Xt, Yt)
    be.knm_storage = "auto"
    with pytest.raises(ValueError, match="features"):
        est.partial_fit(Xt[:, :D - 1], Yt)
    with pytest.raises(ValueError, match="one label column"):
        est.partial_fit(Xt, torch.cat([Yt, Yt], 1))
    with pytest.raises(ValueError, match="total weight"):
        est.remove(Xt, Yt)                       # nothing was added yet
    with pytest.raises(RuntimeError):
        est.solve()
    with pytest.raises(RuntimeError):
        est.as_falkon()
    assert be.calls["knm"] == 0 and est.gram_ is None
    est.partial_fit(Xt, Yt)
    with pytest.raises(ValueError, match="features"):
        est.partial_fit(Xt[:, :D - 1], Yt)
    G0, n0 = est.gram_.clone(), est.n_seen_
    with pytest.raises(ValueError, match="total weight"):
        est.remove(Xt, Yt)                       # all of it
    with pytest.raises(ValueError, match="total weight"):
        est.remove(T(X[:300]), T(y[:300])[:, None])
    assert torch.equal(est.gram_, G0) and est.n_seen_ == n0
    with pytest.raises(ValueError, match="sample_weight"):
        est.partial_fit(Xt, Yt, sample_weight=torch.ones(3))
    with pytest.raises(ValueError, match="total weight"):          # weights that sum to <= 0: refused before G is touched
        est.partial_fit(Xt, Yt, sample_weight=-2.0 * torch.ones(200, dtype=torch.float64))
    assert torch.equal(est.gram_, G0) and est.n_seen_ == n0
    fresh = model(shape, Z)
    with pytest.raises(ValueError, match="total weight"):
        fresh.partial_fit(Xt, Yt, sample_weight=torch.zeros(200, dtype=torch.float64))
    assert fresh.gram_ is None and fresh.ny_points_ is None
    with pytest.raises(NotImplementedError):
        est.fit_path(Xt, Yt, [1e-3])


def test_pickle_copy_and_as_falkon(be):
    shape = SHAPES[0]
    n, M, D, sigma, lam = shape
    X, y, Z, cuts = problem(shape)
    est = feed(model(shape, Z), X, y, cuts, batches=(0, 1))
    assert "_P" in est.__dict__
    state = est.__getstate__()
    assert "_P" not in state and "_zf" not in state
    back = pickle.loads(pickle.dumps(est))
    assert "_P" not in back.__dict__ and "_zf" not in back.__dict__
    assert torch.equal(back.gram_, est.gram_) and torch.equal(back.rhs_, est.rhs_) and back.n_seen_ == est.n_seen_
    Xq = T(X[cuts[2]:])
    p = est.predict(Xq)
    assert tuple(p.shape) == (n - cuts[2], 1) and torch.equal(back.predict(Xq), p)
    pre = be.calls["precond"]
    for m in (est, back, copy.deepcopy(est)):
        feed(m, X, y, cuts, batches=(2,))
    assert be.calls["precond"] == pre + 2       # the two copies rebuilt theirs, the original kept its own
    assert torch.equal(back.alpha_, est.alpha_)
    f = est.as_falkon()
    assert isinstance(f, odx.Falkon) and f.penalty == est.penalty and f.kernel is est.kernel
    assert torch.equal(f.alpha_, est.alpha_) and torch.equal(f.ny_points_, est.ny_points_)
    assert torch.equal(f.predict(Xq), est.predict(Xq))
    assert torch.equal(odx.predict_path([f], Xq), est.predict(Xq))
    # fit() starts over
    est.fit(T(X[:cuts[1]]), T(y[:cuts[1]])[:, None])
    assert est.n_seen_ == cuts[1]
    assert torch.equal(est.alpha_, feed(model(shape, Z), X, y, cuts, batches=(0,)).alpha_)


def test_fit_stats_is_the_schedule_of_falkon_fit(be):
    """falkon_fit_stats over G = K'K, b = K'y against solver.falkon_fit on the same backend (the same CG schedule, K'K v taken
    as G v instead of K' (K v)): equal to f64 rounding amplified by 20 CG steps."""
    shape = SHAPES[0]
    n, M, D, sigma, lam = shape
    X, y, Z, cuts = problem(shape)
    F, Zf = be.features(T(X)), be.features(T(Z))
    a_fit = odx.falkon_fit(be, F, be.vec(y.copy()), Zf, sigma, lam, 20)
    K = be.knm(F, Zf, sigma)
    G, b = be.knm_gram(K, y=be.vec(y.copy()))
    a_stats = odx.falkon_fit_stats(be, G, b, n, be.precond(Zf, sigma, lam, 1e-5), lam, 20)
    r = rel(a_stats.numpy(), a_fit.numpy())
    print("fit_stats vs falkon_fit: %.2e" % r)
    assert r < 1e-8, r
    with pytest.raises(ValueError):
        odx.falkon_fit_stats(be, G, b, 0.0, be.precond(Zf, sigma, lam, 1e-5), lam, 20)
