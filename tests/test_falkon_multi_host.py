"""Host logic of the multi-output fit (odx.solver.falkon_fit_multi, _FalkonBase.fit_multi) on the numpy
oracle backend: T fits from one K_nM block and one preconditioner, each column following falkon_fit's schedule.  No GPU."""
import threading

import numpy as np
import pytest
import torch

import odx
from oracle import falkon_ref as fr
from tests.oracle_backend import OracleBackend
from tests.synth import blob_problem, centres


class CountingBackend(OracleBackend):
    """The oracle backend with call counters; no two-vector pass is offered, so a single fit takes the plain sequence.
    ktk counts the CG passes (v given); rhs counts the right-hand sides K' w asked for on their own (columns 1 .. T - 1: the
    one of column 0 is part of knm_rhs and is not counted)."""
    fold = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = {"knm_rhs": 0, "ktk": 0, "ktk2": 0, "precond": 0, "rhs": 0}
        self._in_rhs = False

    def knm_rhs(self, *a, **kw):
        self.calls["knm_rhs"] += 1
        self._in_rhs = True
        try:
            return super().knm_rhs(*a, **kw)
        finally:
            self._in_rhs = False

    def ktk(self, K, v=None, w=None, out=None):
        if v is not None:
            self.calls["ktk"] += 1
        elif not self._in_rhs:
            self.calls["rhs"] += 1
        return super().ktk(K, v=v, w=w, out=out)

    def ktk2(self, *a, **kw):
        self.calls["ktk2"] += 1
        return super().ktk2(*a, **kw)

    def precond(self, *a, **kw):
        self.calls["precond"] += 1
        return super().precond(*a, **kw)


class GroupedBackend(OracleBackend):
    """The oracle backend with numpy ktwn / trmvn over row matrices, recording their use.  Each row is multiplied as the
    oracle backend's ktk / trmv multiply a single vector (one matrix-vector product per row, not one matrix-matrix product:
    another order of additions moves alpha by ~5e-11 after 20 CG steps at lambda = 1e-5, which would hide a wiring error
    of that size behind the bound of the comparison with the loop route)."""
    fold = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.used = {"ktwn": 0, "trmvn": 0, "trmv": 0, "trmvn_rows": set()}

    def trmv(self, *a, **kw):
        self.used["trmv"] += 1
        return super().trmv(*a, **kw)

    def ktwn(self, K, W, out=None):
        self.used["ktwn"] += 1
        Kt = K.K.double().t()
        for t in range(W.shape[0]):
            out[t, :K.M].copy_(Kt @ W[t, :K.n])
        return out

    def trmvn(self, P, name, X, alpha=1.0, beta=0.0, Z=None, out=None):
        self.used["trmvn"] += 1
        self.used["trmvn_rows"].add(X.shape[0])
        for t in range(X.shape[0]):
            r = alpha * (getattr(P, name) @ X[t, :P.M])
            if beta != 0.0:
                r = r + beta * Z[t, :P.M]
            out[t, :P.M].copy_(r)
        return out


def _problem(n=1500, D=48, M=150, seed=41, T=3):
    """blob_problem's rows and labels as column 0, then T - 1 further +-1 labellings of the same rows."""
    X, y, rng = blob_problem(n, D, seed=seed)
    idx = centres(y, M, rng)
    g = np.random.default_rng(seed + 1000)
    cols = [y.astype(np.float64)]
    for t in range(1, T):
        w = g.standard_normal(D)
        cols.append(np.where(X @ w + 0.3 * g.standard_normal(n) > 0, 1.0, -1.0))
    return X, np.stack(cols, 1), idx


def _ref(X, y, idx, sigma, lam, maxiter=20):
    return fr.falkon_fit(X.astype(np.float64), y, idx, sigma, lam, maxiter=maxiter, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)[0][:, 0]


def test_rows_equal_the_oracle_on_every_column():
    """Every row against oracle.falkon_ref.falkon_fit on that column: the bound of
    tests/test_falkon_path_host.py::test_path_rows_equal_the_oracle_at_every_lambda (1e-6 relative)."""
    X, Y, idx = _problem(T=4)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    alphas = odx.falkon_fit_multi(be, F, be.vec(Y), be.rows(F, idx), 10.0, 1e-5, 20)
    assert tuple(alphas.shape) == (4, len(idx)) and alphas.dtype == torch.float64
    for t in range(4):
        ref = _ref(X, Y[:, t], idx, 10.0, 1e-5)
        rel = np.linalg.norm(alphas[t].numpy() - ref) / np.linalg.norm(ref)
        print("column %d: alpha rel err %.2e" % (t, rel))
        assert rel < 1e-6, (t, rel)


def test_one_column_is_falkon_fit():
    X, Y, idx = _problem(seed=42, T=1)
    be = CountingBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    a1 = odx.falkon_fit(be, F, be.vec(Y[:, 0]), Zf, 10.0, 1e-5, 20)
    am = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, 10.0, 1e-5, 20)
    assert tuple(am.shape) == (1, len(idx)) and torch.equal(am[0], a1)


def test_a_column_equals_itself_fitted_alone():
    X, Y, idx = _problem(seed=43, T=3)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    three = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, 6.0, 1e-4, 20)
    for t in range(3):
        single = odx.falkon_fit_multi(be, F, be.vec(Y[:, t:t + 1]), Zf, 6.0, 1e-4, 20)
        assert torch.equal(single[0], three[t]), t


@pytest.mark.parametrize("maxiter", [9, 10, 11, 20, 25])
def test_one_build_one_preconditioner_and_the_passes_of_one_fit_per_column(maxiter):
    X, Y, idx = _problem(seed=44, T=3)
    one = CountingBackend(np.float64)
    F = one.features(torch.from_numpy(X))
    a1 = odx.falkon_fit(one, F, one.vec(Y[:, 1]), one.rows(F, idx), 10.0, 1e-5, maxiter)
    assert one.calls["knm_rhs"] == 1 and one.calls["ktk2"] == 0 and one.calls["rhs"] == 0
    be = CountingBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    alphas = odx.falkon_fit_multi(be, F, be.vec(Y), be.rows(F, idx), 10.0, 1e-5, maxiter)
    assert be.calls["knm_rhs"] == 1 and be.calls["precond"] == 1
    assert be.calls["ktk"] == 3 * one.calls["ktk"] and be.calls["ktk2"] == 0
    assert be.calls["rhs"] == 2                      # the right-hand sides of columns 1 and 2
    assert torch.equal(alphas[1], a1)                # the plain sequence of falkon_fit, operation for operation
    ref = _ref(X, Y[:, 2], idx, 10.0, 1e-5, maxiter)
    assert np.linalg.norm(alphas[2].numpy() - ref) / np.linalg.norm(ref) < 1e-6


def test_a_zero_column_and_an_early_stop_leave_the_others_alone():
    """Column 1 is all zeros (b = 0: its stop flag rises at once, its alpha is 0); column 2 lies in the span of a few centres
    and converges early under a loose tolerance.  Columns 0 and 3 must come out as they do when fitted without them."""
    X, Y, idx = _problem(seed=45, T=4)
    Y[:, 1] = 0.0
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    opt = odx.SolverOptions(cg_tolerance=3e-2)       # (sqrt(||r||^2) < 9e-4: met by some columns before maxiter, not by all)
    full = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, 10.0, 1e-3, 20, opt)
    assert torch.count_nonzero(full[1]) == 0
    assert torch.isfinite(full).all()
    for t in (0, 2, 3):
        alone = odx.falkon_fit_multi(be, F, be.vec(Y[:, t:t + 1]), Zf, 10.0, 1e-3, 20, opt)
        assert torch.equal(alone[0], full[t]), t
    # the tolerance stops at least one column early: its alpha differs from the one of a run that never stops
    never = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, 10.0, 1e-3, 20, odx.SolverOptions(cg_tolerance=0.0))
    assert any(not torch.equal(never[t], full[t]) for t in (0, 2, 3))


def test_the_grouped_route_is_taken_and_agrees_with_the_loops():
    X, Y, idx = _problem(seed=46, T=5, M=151)        # (odd M: rows of the shared matrices are padded)
    loop = OracleBackend(np.float64)
    loop.fold = False
    F = loop.features(torch.from_numpy(X))
    a_loop = odx.falkon_fit_multi(loop, F, loop.vec(Y), loop.rows(F, idx), 10.0, 1e-5, 20)
    be = GroupedBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    a_grp = odx.falkon_fit_multi(be, F, be.vec(Y), be.rows(F, idx), 10.0, 1e-5, 20)
    assert be.used["ktwn"] == 1
    # 2 for B, 4 per W (20 steps + 1 full residual), 2 for alpha; every one over all 5 states; no per-state product
    assert be.used["trmvn"] == 2 + 4 * 21 + 2 and be.used["trmvn_rows"] == {5} and be.used["trmv"] == 0
    for t in range(5):
        rel = float((a_grp[t] - a_loop[t]).norm() / a_loop[t].norm())
        assert rel < 1e-12, (t, rel)
    # one column: nothing to group, the plain sequence
    be1 = GroupedBackend(np.float64)
    F = be1.features(torch.from_numpy(X))
    a_one = odx.falkon_fit_multi(be1, F, be1.vec(Y[:, :1]), be1.rows(F, idx), 10.0, 1e-5, 20)
    assert be1.used["trmvn"] == 0 and be1.used["ktwn"] == 0 and torch.equal(a_one[0], a_loop[0])


def test_replicated_row_shards_give_the_one_shard_alphas():
    """Two halves of the rows, each driven by its own thread, with an allreduce stub that sums in place over the two: the
    alphas of the whole block to f64 rounding (tests/test_falkon_path_host.py, same construction)."""
    X, Y, idx = _problem(seed=47, T=3)
    n, T = len(X), 3
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    whole = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, 10.0, 1e-5, 20)
    barrier, slots, shapes = threading.Barrier(2), [None, None], [[], []]

    def make_allreduce(rank):
        def allreduce(v):
            shapes[rank].append(tuple(v.shape))
            slots[rank] = v
            barrier.wait()
            total = slots[0] + slots[1]
            barrier.wait()
            v.copy_(total)
            return v
        return allreduce

    out, errs = [None, None], []

    def run(rank):
        try:
            rows = torch.arange(rank * (n // 2), n // 2 if rank == 0 else n)
            b = OracleBackend(np.float64)
            Fr = b.features(torch.from_numpy(X)[rows])
            out[rank] = odx.falkon_fit_multi(b, Fr, b.vec(Y)[rows], Zf, 10.0, 1e-5, 20, n_total=n, allreduce=make_allreduce(rank))
        except Exception as e:      # noqa: BLE001 — reported below; the other thread must not wait for ever
            errs.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errs, errs
    Mp = (len(idx) + 1) // 2 * 2
    # the right-hand side of column 0, the matrix of the others, then ONE (T, Mp) matrix per pass: 20 steps + 1 full residual
    assert shapes[0] == [(len(idx),), (T - 1, Mp)] + [(T, Mp)] * 21
    for r in range(2):
        for t in range(T):
            rel = float((out[r][t] - whole[t]).norm() / whole[t].norm())
            assert rel < 1e-9, (r, t, rel)
    assert torch.equal(out[0], out[1])


def test_estimator_fits_and_predicts_all_columns():
    from odx.wrappers import CenterSelector
    X, Y, idx = _problem(n=600, D=24, M=60, seed=48, T=3)
    odx.set_backend(OracleBackend(np.float64))
    try:
        def make():
            return odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=6.0), penalty=1e-3, M=len(idx), maxiter=20,
                                    center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
        Xt, Yt = torch.from_numpy(X), torch.from_numpy(Y)
        m = make().fit_multi(Xt, Yt)
        assert tuple(m.alpha_.shape) == (60, 3) and m.M == 60
        p = m.predict(Xt[:50])
        assert tuple(p.shape) == (50, 3)
        for t in range(3):
            one = make().fit(Xt, Yt[:, t])
            assert tuple(one.alpha_.shape) == (60, 1)
            assert np.linalg.norm((one.alpha_[:, 0] - m.alpha_[:, t]).numpy()) / np.linalg.norm(one.alpha_.numpy()) < 1e-8
            assert np.abs(one.predict(Xt[:50]).numpy()[:, 0] - p.numpy()[:, t]).max() < 1e-5
        with pytest.raises(ValueError, match="one right-hand side"):
            make().fit(Xt, Yt)                                   # (fit keeps its refusal: fit_multi is the entry)
        with pytest.raises(ValueError, match="one right-hand side"):
            make().fit_path(Xt, Yt, [1e-3, 1e-4])
        with pytest.raises(ValueError, match="one right-hand side"):
            odx.falkon.fit_batch([make()], [Xt], [Yt])
    finally:
        odx.set_backend(None)
