"""odx.IncrementalFalkon with several outputs and lambda paths on the CPU: the host logic of odx/incremental.py and
solver.falkon_fit_stats_multi / falkon_fit_stats_path driven by the numpy oracle backend of tests/test_incremental_host.py plus
numpy f64 statements of knm_gram_multi, trmvn and precond_path, against oracle/falkon_ref in f64 with a label MATRIX; the
call counts the design promises (one block and one Gram per chunk whatever T is, ceil(k L T / 8) reads of G per CG iteration,
one precond_path per solve_path); the refusals; and outputs = 1 as the model was."""
import copy
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import odx  # noqa: E402
from odx import backend as _backend  # noqa: E402
from oracle import falkon_ref as fr  # noqa: E402
from tests.oracle_backend import OracleBackend  # noqa: E402
from tests.test_incremental_host import IncrementalOracleBackend, T as tt, problem, rel  # noqa: E402

SMALL = (777, 129, 36, 5.0, 1e-3)
PENALTIES = [1e-2, 1e-3, 1e-4]


class MultiOracleBackend(IncrementalOracleBackend):
    """IncrementalOracleBackend plus knm_gram_multi (the Gram as knm_gram states it, the T right-hand sides beside it), trmvn and
    precond_path in numpy f64.  symv logs the rows of every call: a call of r rows is ceil(r / 8) reads of G in the product."""

    def __init__(self):
        super().__init__()
        self.calls.update({"knm_gram_multi": 0, "precond_path": 0, "trmvn": 0, "trmv": 0})
        self.symv_rows = []

    def knm_gram_multi(self, K, w=None, Y=None, beta=1.0, G=None, B=None):
        self.calls["knm_gram_multi"] += 1
        self.calls["knm_gram"] -= 1                       # (the Gram below is this call's, not a knm_gram of the model's)
        Kd = K.K.numpy().astype(np.float64)
        n, M = Kd.shape
        Tn = Y.shape[1]
        if G is None:
            B = torch.zeros((Tn, (M + 1) // 2 * 2), dtype=torch.float64)
        elif beta == 0.0:
            B[:, :M] = 0.0
        G, _ = self.knm_gram(K, w=w, beta=beta, G=G)
        wv = np.ones(n) if w is None else w.numpy()[:n]
        Bn = B.numpy()
        Bn[:, :M] = (Kd.T @ (wv[:, None] * Y.numpy()[:n])).T + beta * Bn[:, :M]
        return G, B

    def symv(self, G, X, alpha=1.0, out=None):
        self.symv_rows.append(int(X.shape[0]))
        return super().symv(G, X, alpha=alpha, out=out)

    def trmv(self, *a, **kw):
        self.calls["trmv"] += 1
        return super().trmv(*a, **kw)

    def trmvn(self, P, name, X, alpha=1.0, beta=0.0, Z=None, out=None):
        self.calls["trmvn"] += 1
        for t in range(X.shape[0]):
            r = alpha * (getattr(P, name) @ X[t, :P.M])
            if beta != 0.0:
                r = r + beta * Z[t, :P.M]
            out[t, :P.M].copy_(r)
        return out

    def precond_path(self, Zf, sigma, lams, eps):
        self.calls["precond_path"] += 1
        Ps = [OracleBackend.precond(self, Zf, sigma, lam, eps) for lam in lams]
        for P in Ps[1:]:                                  # (the members share T's factors, as the product's do)
            P.LTi, P.LTit = Ps[0].LTi, Ps[0].LTit
        return Ps


@pytest.fixture()
def be():
    b = MultiOracleBackend()
    old = _backend._BACKEND
    _backend.set_backend(b)
    yield b
    _backend.set_backend(old)


_labels = {}


def labels(shape, T):
    """The (n, T) f64 label matrix of a parity shape: column 0 the problem's labels; the others +-1 labels of other seeded
    splits of the rows (the sign of a seeded random direction of the features about its median); the last column of T >= 3
    real-valued (tanh of such a direction).  Computed once, shared, never changed."""
    if (shape, T) not in _labels:
        X, y, Z, cuts = problem(shape)
        rng = np.random.default_rng(4242 + T)
        Y = np.empty((len(X), T))
        Y[:, 0] = y
        for t in range(1, T):
            p = X.astype(np.float64) @ rng.standard_normal(X.shape[1])
            p = (p - np.median(p)) / p.std()
            Y[:, t] = np.tanh(p) if (t == T - 1 and T >= 3) else np.where(p > 0, 1.0, -1.0)
        Y.setflags(write=False)
        _labels[(shape, T)] = Y
    return _labels[(shape, T)]


def oracle_alphas(X, Y, Z, kernel, lam, rows=None):
    """alpha (M, T) of the f64 oracle on a label matrix."""
    X, Y = (X, Y) if rows is None else (X[rows], Y[rows])
    return fr.falkon_fit_centers(X.astype(np.float64), Y.astype(np.float64), Z.astype(np.float64), kernel, lam, len(X), maxiter=20,
                                 dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)[0]


def model(shape, Z, **kw):
    n, M, D, sigma, lam = shape
    return odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, centres=tt(Z), **kw)


def feed(est, X, Y, cuts, batches=(0, 1, 2), **kw):
    for i in batches:
        est.partial_fit(tt(X[cuts[i]:cuts[i + 1]]), tt(Y[cuts[i]:cuts[i + 1]]), **kw)
    return est


def reads(rows):
    return sum((r + 7) // 8 for r in rows)


@pytest.mark.parametrize("chunk_rows", [None, 256], ids=["whole", "chunks256"])
@pytest.mark.parametrize("T", [3, 9])
def test_every_column_is_the_oracle_and_removal_the_oracle_on_the_rest(be, T, chunk_rows):
    n, M, D, sigma, lam = SMALL
    X, y, Z, cuts = problem(SMALL)
    Y = labels(SMALL, T)
    est = feed(model(SMALL, Z, outputs=T, chunk_rows=chunk_rows), X, Y, cuts)
    Mp = (M + 1) // 2 * 2
    assert est.n_seen_ == n and tuple(est.alpha_.shape) == (M, T) and tuple(est.rhs_.shape) == (T, Mp)
    assert est.rhs_.dtype == torch.float64 and torch.equal(est.gram_[:, :M], est.gram_[:, :M].t())
    chunks = 3 if chunk_rows is None else sum(-(-(cuts[i + 1] - cuts[i]) // chunk_rows) for i in range(3))
    # per chunk one block and one Gram, whatever T is; one preconditioner; no pass over rows
    assert be.calls["knm"] == chunks and be.calls["knm_gram_multi"] == chunks and be.calls["knm_gram"] == 0
    assert be.calls["precond"] == 1 and be.calls["ktk"] == 0
    ref = oracle_alphas(X, Y, Z, sigma, lam)
    one = feed(model(SMALL, Z, chunk_rows=chunk_rows), X, Y[:, :1], cuts)
    print("T %d column 0 against the one-output model: %.2e" % (T, rel(est.alpha_[:, 0].numpy(), one.alpha_.numpy())))
    for t in range(T):
        r = rel(est.alpha_[:, t].numpy(), ref[:, t])
        print("T %d column %d: alpha rel err %.2e" % (T, t, r))
        assert r < 1e-4, (t, r)
    Xq = X[::7]
    p = est.predict(tt(Xq)).numpy()
    pref = fr.falkon_predict(Xq.astype(np.float64), Z.astype(np.float64), ref, sigma)
    assert p.shape == (len(Xq), T)
    s = np.abs(p - pref).max(0)
    print("T %d: score err per column %s" % (T, " ".join("%.1e" % v for v in s)))
    assert (s < 1e-4).all(), s
    est.remove(tt(X[cuts[1]:cuts[2]]), tt(Y[cuts[1]:cuts[2]]))
    left = np.r_[0:cuts[1], cuts[2]:n]
    assert est.n_seen_ == len(left) and be.calls["precond"] == 2        # (the one-output model above built its own)
    ref = oracle_alphas(X, Y, Z, sigma, lam, left)
    for t in range(T):
        r = rel(est.alpha_[:, t].numpy(), ref[:, t])
        print("T %d column %d after removing the middle batch: alpha rel err %.2e" % (T, t, r))
        assert r < 1e-4, (t, r)
    # the batch taken out is now held out: its scores by the model against the oracle's on the rows left
    Xh = X[cuts[1]:cuts[2]]
    s = np.abs(est.predict(tt(Xh)).numpy() - fr.falkon_predict(Xh.astype(np.float64), Z.astype(np.float64), ref, sigma)).max(0)
    print("T %d: held-out score err per column %s" % (T, " ".join("%.1e" % v for v in s)))
    assert (s < 1e-4).all(), s


@pytest.mark.parametrize("T", [3, 9])
def test_a_solve_reads_G_once_per_eight_vectors(be, T):
    """20 iterations: 20 exchanges of T rows, the 10th with the folded full residual's T iterates beside them; every triangular
    product through trmvn; no block built."""
    X, y, Z, cuts = problem(SMALL)
    est = feed(model(SMALL, Z, outputs=T), X, labels(SMALL, T), cuts, solve=False)
    assert est.alpha_ is None and be.symv_rows == [] and be.calls["precond"] == 0
    before = dict(be.calls)
    est.solve()
    assert be.symv_rows == [T] * 9 + [2 * T] + [T] * 10
    assert reads(be.symv_rows) == 19 * ((T + 7) // 8) + (2 * T + 7) // 8
    assert be.calls["knm"] == before["knm"] and be.calls["knm_gram_multi"] == before["knm_gram_multi"]
    assert be.calls["trmv"] == 0 and be.calls["trmvn"] > 0 and be.calls["precond"] == 1


@pytest.mark.parametrize("T", [1, 3])
def test_solve_path_members_are_the_oracle_at_their_penalty(be, T):
    n, M, D, sigma, lam = SMALL
    X, y, Z, cuts = problem(SMALL)
    Y = labels(SMALL, T)
    est = feed(model(SMALL, Z, outputs=T), X, Y, cuts)
    a0, G0, b0 = est.alpha_.clone(), est.gram_.clone(), est.rhs_.clone()
    before = dict(be.calls)
    be.symv_rows.clear()
    members = est.solve_path(PENALTIES)
    L = len(PENALTIES)
    assert be.calls["precond_path"] == 1 and be.calls["precond"] == before["precond"] and be.calls["knm"] == before["knm"]
    assert be.calls["ktk"] == 0 and be.calls["knm_gram"] == before["knm_gram"] and be.calls["knm_gram_multi"] == before["knm_gram_multi"]
    assert be.symv_rows == [L * T] * 9 + [2 * L * T] + [L * T] * 10
    assert reads(be.symv_rows) == 19 * ((L * T + 7) // 8) + (2 * L * T + 7) // 8
    assert est.penalty == lam and torch.equal(est.alpha_, a0) and torch.equal(est.gram_, G0) and torch.equal(est.rhs_, b0)
    assert [m.penalty for m in members] == PENALTIES and all(isinstance(m, odx.Falkon) for m in members)
    assert all(m.ny_points_ is members[0].ny_points_ for m in members)
    for m, pen in zip(members, PENALTIES):
        ref = oracle_alphas(X, Y, Z, sigma, pen)
        assert tuple(m.alpha_.shape) == (M, T)
        for t in range(T):
            r = rel(m.alpha_[:, t].numpy(), ref[:, t])
            print("T %d penalty %g column %d: alpha rel err %.2e" % (T, pen, t, r))
            assert r < 1e-4, (pen, t, r)
    # the member at the model's own penalty against the model's solve: the same schedule beside other states
    print("member at the model's penalty against solve(): %.2e" % rel(members[1].alpha_.numpy(), a0.numpy()))
    Xq = tt(X[:50])
    if T == 1:
        P = odx.predict_path(members, Xq)
        for l, m in enumerate(members):
            assert torch.equal(P[:, l], m.predict(Xq)[:, 0])
    else:
        assert tuple(members[0].predict(Xq).shape) == (50, T)


def test_refusals_leave_the_statistics_alone(be):
    n, M, D, sigma, lam = SMALL
    X, y, Z, cuts = problem(SMALL)
    Y = labels(SMALL, 3)
    for bad in (0, -2, 1025, 2.5, True):
        with pytest.raises(ValueError, match="outputs"):
            model(SMALL, Z, outputs=bad)
    est = model(SMALL, Z, outputs=3)
    with pytest.raises(RuntimeError, match="solve_path"):
        est.solve_path(PENALTIES)
    with pytest.raises(ValueError, match="label columns"):
        est.partial_fit(tt(X[:200]), tt(Y[:200, :2]))
    assert est.gram_ is None and est.ny_points_ is None and be.calls["knm"] == 0
    feed(est, X, Y, cuts, batches=(0,))
    G0, b0, n0, a0 = est.gram_.clone(), est.rhs_.clone(), est.n_seen_, est.alpha_.clone()
    calls = dict(be.calls)
    Xb, Yb = tt(X[cuts[1]:cuts[2]]), tt(Y[cuts[1]:cuts[2]])
    for width in (1, 2, 4):
        with pytest.raises(ValueError, match="label columns"):
            est.partial_fit(Xb, tt(labels(SMALL, 9)[cuts[1]:cuts[2], :width]))
        with pytest.raises(ValueError, match="label columns"):
            est.remove(Xb, tt(labels(SMALL, 9)[cuts[1]:cuts[2], :width]))
    with pytest.raises(ValueError, match="sample_weight"):
        est.partial_fit(Xb, Yb, sample_weight=torch.ones((len(Xb), 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="sample_weight"):
        est.partial_fit(Xb, Yb, sample_weight=torch.ones(5, dtype=torch.float64))
    with pytest.raises(ValueError):
        est.solve_path([])
    with pytest.raises(ValueError):
        est.solve_path([1e-3, -1.0])
    with pytest.raises(NotImplementedError, match="outputs=.*solve_path"):
        est.fit_multi(Xb, Yb)
    for name in ("fit_path", "fit_cv", "fit_grid"):
        with pytest.raises(NotImplementedError):
            getattr(est, name)(Xb, Yb, [1e-3])
    assert torch.equal(est.gram_, G0) and torch.equal(est.rhs_, b0) and est.n_seen_ == n0 and torch.equal(est.alpha_, a0)
    assert be.calls["knm"] == calls["knm"] and be.calls["knm_gram_multi"] == calls["knm_gram_multi"]


def test_one_weight_per_row_acts_on_every_output(be):
    """A weight of two is the row given twice, decay scales all T right-hand sides, and a negated batch takes every output's
    rows out: rows of the statistics, column by column."""
    X, y, Z, cuts = problem(SMALL)
    Y = labels(SMALL, 3)
    sub = np.arange(0, len(X), 3)
    w = np.ones(len(X))
    w[sub] = 2.0
    a = model(SMALL, Z, outputs=3).partial_fit(tt(X), tt(Y), sample_weight=tt(w))
    b = model(SMALL, Z, outputs=3).partial_fit(tt(np.concatenate([X, X[sub]])), tt(np.concatenate([Y, Y[sub]])))
    assert a.n_seen_ == b.n_seen_ and rel(a.alpha_.numpy(), b.alpha_.numpy()) < 1e-10
    c = feed(model(SMALL, Z, outputs=3), X, Y, cuts, batches=(0,), solve=False)
    first = c.rhs_.clone()
    c.partial_fit(tt(X[cuts[1]:cuts[2]]), tt(Y[cuts[1]:cuts[2]]), decay=0.5, solve=False)
    d = feed(model(SMALL, Z, outputs=3), X, Y, cuts, batches=(1,), solve=False)
    np.testing.assert_allclose(c.rhs_.numpy(), 0.5 * first.numpy() + d.rhs_.numpy(), rtol=1e-13, atol=1e-13)
    assert c.n_seen_ == 0.5 * cuts[1] + (cuts[2] - cuts[1])


def test_pickle_copy_and_as_falkon_carry_every_output(be):
    n, M, D, sigma, lam = SMALL
    X, y, Z, cuts = problem(SMALL)
    Y = labels(SMALL, 3)
    est = feed(model(SMALL, Z, outputs=3), X, Y, cuts, batches=(0, 1))
    back = pickle.loads(pickle.dumps(est))
    assert "_P" not in back.__dict__ and back.outputs == 3
    assert tuple(back.rhs_.shape) == (3, (M + 1) // 2 * 2) and torch.equal(back.rhs_, est.rhs_) and torch.equal(back.gram_, est.gram_)
    for m in (est, back, copy.deepcopy(est)):
        feed(m, X, Y, cuts, batches=(2,))
    assert torch.equal(back.alpha_, est.alpha_)
    f = est.as_falkon()
    Xq = tt(X[:64])
    assert isinstance(f, odx.Falkon) and tuple(f.alpha_.shape) == (M, 3) and torch.equal(f.alpha_, est.alpha_)
    assert tuple(f.predict(Xq).shape) == (64, 3) and torch.equal(f.predict(Xq), est.predict(Xq))
    est.fit(tt(X[:cuts[1]]), tt(Y[:cuts[1]]))
    assert est.n_seen_ == cuts[1] and tuple(est.rhs_.shape) == (3, (M + 1) // 2 * 2)


def test_outputs_one_is_the_model_as_it_was(be):
    """The default and outputs=1: knm_gram + falkon_fit_stats, rhs_ (M,), alpha_ (M, 1), the same calls and the same bits; a
    second label column is still refused by name."""
    n, M, D, sigma, lam = SMALL
    X, y, Z, cuts = problem(SMALL)
    Y1 = np.ascontiguousarray(y[:, None].astype(np.float64))
    a = feed(model(SMALL, Z), X, Y1, cuts)
    calls_a, rows_a = dict(be.calls), list(be.symv_rows)
    for k in be.calls:
        be.calls[k] = 0
    be.symv_rows.clear()
    b = feed(model(SMALL, Z, outputs=1), X, Y1, cuts)
    assert be.calls == calls_a and be.symv_rows == rows_a
    assert calls_a["knm_gram"] == 3 and calls_a["knm_gram_multi"] == 0 and calls_a["trmvn"] == 0 and calls_a["precond_path"] == 0
    assert rows_a == ([1] * 9 + [2] + [1] * 10) * 3
    assert tuple(a.rhs_.shape) == tuple(b.rhs_.shape) == (M,) and tuple(b.alpha_.shape) == (M, 1)
    assert torch.equal(a.gram_, b.gram_) and torch.equal(a.rhs_, b.rhs_) and torch.equal(a.alpha_, b.alpha_)
    assert rel(a.alpha_.numpy(), oracle_alphas(X, Y1, Z, sigma, lam)) < 1e-4
    for m in (a, b):
        with pytest.raises(ValueError, match="one label column"):
            m.partial_fit(tt(X[:100]), tt(np.concatenate([Y1[:100], Y1[:100]], 1)))


def test_fit_stats_multi_is_fit_stats_column_by_column(be):
    """solver.falkon_fit_stats_multi and a one-member falkon_fit_stats_path against falkon_fit_stats on each row of B: the same
    schedule in lock step, equal to f64 rounding amplified by 20 CG steps."""
    n, M, D, sigma, lam = SMALL
    X, y, Z, cuts = problem(SMALL)
    Y = labels(SMALL, 3)
    F, Zf = be.features(tt(X)), be.features(tt(Z))
    K = be.knm(F, Zf, sigma)
    G, B = be.knm_gram_multi(K, Y=be.vec(Y.copy()))
    P = be.precond(Zf, sigma, lam, 1e-5)
    multi = odx.falkon_fit_stats_multi(be, G, B, n, P, lam, 20)
    path = odx.falkon_fit_stats_path(be, G, B, n, be.precond_path(Zf, sigma, [lam], 1e-5), [lam], 20)
    assert tuple(multi.shape) == (3, M) and tuple(path.shape) == (1, 3, M)
    for t in range(3):
        one = odx.falkon_fit_stats(be, G, B[t], n, P, lam, 20)
        r = rel(multi[t].numpy(), one.numpy())
        print("column %d: multi against fit_stats %.2e" % (t, r))
        assert r < 1e-8 and rel(path[0, t].numpy(), one.numpy()) < 1e-8
    with pytest.raises(ValueError):
        odx.falkon_fit_stats_multi(be, G, B, 0.0, P, lam, 20)
