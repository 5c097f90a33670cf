"""Host logic of the lambda path (odx.solver.falkon_fit_path, _FalkonBase.fit_path) on the numpy oracle backend: L fits
from one K_nM block, each member following falkon_fit's schedule.  No GPU."""
import threading

import numpy as np
import pytest
import torch

import odx
from oracle import falkon_ref as fr
from tests.oracle_backend import OracleBackend
from tests.synth import blob_problem, centres

LAMS = [1e-6, 1e-5, 1e-4, 1e-3]          # the range of the shipped classifier penalties


class CountingBackend(OracleBackend):
    """The oracle backend with call counters; no two-vector pass is offered, so a single fit takes the plain sequence."""
    fold = False

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = {"knm_rhs": 0, "ktk": 0, "ktk2": 0, "precond": 0}

    def knm_rhs(self, *a, **kw):
        self.calls["knm_rhs"] += 1
        return super().knm_rhs(*a, **kw)

    def ktk(self, K, v=None, w=None, out=None):
        if v is not None:                 # (the right-hand side K' w of knm_rhs is not a CG pass)
            self.calls["ktk"] += 1
        return super().ktk(K, v=v, w=w, out=out)

    def ktk2(self, *a, **kw):
        self.calls["ktk2"] += 1
        return super().ktk2(*a, **kw)

    def precond(self, *a, **kw):
        self.calls["precond"] += 1
        return super().precond(*a, **kw)


def _problem(n=1500, D=48, M=150, seed=31):
    X, y, rng = blob_problem(n, D, seed=seed)
    return X, y, centres(y, M, rng)


def test_path_rows_equal_the_oracle_at_every_lambda():
    """Every row of the path against oracle.falkon_ref.falkon_fit at its lambda, under the bound of
    tests/test_host_logic.py::test_solver_equals_oracle for falkon_fit on this backend (1e-6 relative)."""
    X, y, idx = _problem()
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    alphas = odx.falkon_fit_path(be, F, be.vec(y), be.rows(F, idx), 10.0, LAMS, 20)
    assert tuple(alphas.shape) == (len(LAMS), len(idx)) and alphas.dtype == torch.float64
    for l, lam in enumerate(LAMS):
        ref, _ = fr.falkon_fit(X.astype(np.float64), y, idx, 10.0, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        rel = np.linalg.norm(alphas[l].numpy() - ref[:, 0]) / np.linalg.norm(ref[:, 0])
        print("lam %g: alpha rel err %.2e" % (lam, rel))
        assert rel < 1e-6, (lam, rel)


@pytest.mark.parametrize("maxiter", [9, 10, 11, 20, 25])
def test_one_build_and_the_passes_of_one_fit_per_member(maxiter):
    X, y, idx = _problem(seed=32)
    one = CountingBackend(np.float64)
    F = one.features(torch.from_numpy(X))
    a1 = odx.falkon_fit(one, F, one.vec(y), one.rows(F, idx), 10.0, LAMS[1], maxiter)
    assert one.calls["knm_rhs"] == 1 and one.calls["ktk2"] == 0
    be = CountingBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    alphas = odx.falkon_fit_path(be, F, be.vec(y), be.rows(F, idx), 10.0, LAMS, maxiter)
    assert be.calls["knm_rhs"] == 1 and be.calls["precond"] == len(LAMS)
    assert be.calls["ktk"] == len(LAMS) * one.calls["ktk"] and be.calls["ktk2"] == 0
    assert torch.equal(alphas[1], a1)          # the plain sequence of falkon_fit, operation for operation


def test_a_path_of_one_equals_its_row_in_a_path_of_three():
    X, y, idx = _problem(seed=33)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    three = odx.falkon_fit_path(be, F, be.vec(y), Zf, 6.0, [1e-3, 1e-5, 1e-4], 20)
    single = odx.falkon_fit_path(be, F, be.vec(y), Zf, 6.0, [1e-5], 20)
    assert tuple(single.shape) == (1, len(idx)) and torch.equal(single[0], three[1])


def test_replicated_row_shards_give_the_one_shard_alphas():
    """Two halves of the rows, each driven by its own thread, with an allreduce stub that sums in place over the two:
    the alphas of the whole block to f64 rounding (the partial products are added in another order)."""
    X, y, idx = _problem(seed=34)
    n = len(X)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    whole = odx.falkon_fit_path(be, F, be.vec(y), Zf, 10.0, LAMS, 20)
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
            out[rank] = odx.falkon_fit_path(b, Fr, b.vec(y)[rows], Zf, 10.0, LAMS, 20, n_total=n, allreduce=make_allreduce(rank))
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
    # the right-hand side once, then ONE (L, Mp) matrix per pass: 20 steps + 1 full residual
    assert shapes[0] == [(len(idx),)] + [(len(LAMS), Mp)] * 21
    for r in range(2):
        for l in range(len(LAMS)):
            rel = float((out[r][l] - whole[l]).norm() / whole[l].norm())
            assert rel < 1e-9, (r, l, rel)
    assert torch.equal(out[0], out[1])


@pytest.mark.parametrize("lams", [[], [0.0], [1e-5, -1e-5], [float("nan")], [float("inf"), 1e-5]])
def test_bad_penalties_are_refused(lams):
    X, y, idx = _problem(n=300, D=16, M=30, seed=35)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    with pytest.raises(ValueError):
        odx.falkon_fit_path(be, F, be.vec(y), be.rows(F, idx), 10.0, lams, 5)


def test_estimator_fit_path():
    from odx.wrappers import CenterSelector
    X, y, rng = blob_problem(600, 24, seed=8)
    idx = centres(y, 60, rng)
    odx.set_backend(OracleBackend(np.float64))
    try:
        m = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=6.0), penalty=1e-3, M=len(idx), maxiter=20,
                             center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
        Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
        models = m.fit_path(Xt, yt, LAMS)
        assert m.alpha_ is None and m.penalty == 1e-3                      # the template is left alone
        assert len(models) == len(LAMS) and all(type(e) is type(m) for e in models)
        Z = X[np.asarray(idx).reshape(-1)].astype(np.float64)
        Kxz = fr.gaussian_kernel(X[:50].astype(np.float64), Z, 6.0, np.float64)
        for e, lam in zip(models, LAMS):
            assert e.penalty == lam and e.M == 60 and tuple(e.alpha_.shape) == (60, 1)
            assert e.ny_points_ is models[0].ny_points_
            ref, _ = fr.falkon_fit(X.astype(np.float64), y, idx, 6.0, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
            assert np.linalg.norm(e.alpha_.numpy()[:, 0] - ref[:, 0]) / np.linalg.norm(ref[:, 0]) < 1e-6
            p = e.predict(Xt[:50])
            assert tuple(p.shape) == (50, 1)
            assert np.abs(p.numpy()[:, 0] - Kxz @ e.alpha_.numpy()[:, 0]).max() < 1e-5      # f32 scores of an f64 product
        one = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=6.0), penalty=LAMS[2], M=len(idx), maxiter=20,
                               center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no")).fit(Xt, yt)
        assert np.linalg.norm((one.alpha_ - models[2].alpha_).numpy()) / np.linalg.norm(one.alpha_.numpy()) < 1e-8
    finally:
        odx.set_backend(None)
