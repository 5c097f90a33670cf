"""Scores summed from the CG's own passes (solver.scores_from_cg), sequencing only, on the CPU: the tests' oracle backend with
the three pieces the product backend offers — passes with a t_out, cg_scores_axpy, cg_scores_store — driven by
solver.falkon_fit, solver.falkon_fit_lockstep and LockstepClassJob.  K alpha = sum_i a_i K v_i must hold for exactly the
steps the iterate received: also when the stop flag goes up before maxiter, and when it goes up in the cg_finish of the very
iteration whose step was just taken."""
import numpy as np
import pytest
import torch

from odx import solver
from odx.job import LockstepClassJob
from tests.oracle_backend import OracleBackend
from tests.test_dist_gloo import _job_problem


class CgScoresOracleBackend(OracleBackend):
    """f32-stored, f32-accurate blocks (as HipBackend's under gauss "h2"), a dense knm_mv, and the t_out / score entries."""
    gauss = "h2"

    def __init__(self, fold=True):
        super().__init__(np.float64)
        self.fold = fold
        self.mv_calls = self.mv_reads = self.axpy_calls = self.store_calls = self.t_calls = 0

    def knm(self, F, Zf, sigma, out=None):
        K = super().knm(F, Zf, sigma, out=out)
        K.fmt = "f32"
        return K

    def ktk(self, K, v=None, w=None, out=None, t_out=None):
        if t_out is not None:
            self.t_calls += 1
            t_out.copy_(K.K.double() @ v)
        return super().ktk(K, v=v, w=w, out=out)

    def ktk2(self, K, v1, v2, out1=None, out2=None, t_out=None):
        return self.ktk(K, v=v1, out=out1, t_out=t_out), self.ktk(K, v=v2, out=out2)

    def cg_scores_axpy(self, state, t, S):
        self.axpy_calls += 1
        if state[2] != 0:
            return
        S.add_(state[3] * t)

    def cg_scores_store(self, S, out):
        self.store_calls += 1
        out.copy_(S.float().reshape(out.shape))
        return out

    def knm_mv(self, K, alpha, out=None, summed=None):
        self.mv_calls += 1
        if summed is not None:                                  # the fit's own sum: rounded, the block is not read
            return self.cg_scores_store(summed, out if out is not None else torch.empty((K.n, 1), dtype=torch.float32))
        self.mv_reads += 1
        r = (K.K.double() @ alpha.double()).float()[:, None]
        if out is not None:
            out.copy_(r)
            return out
        return r


def _problem(n=600, D=12, M=40, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    y = np.where(X[:, 0] + 0.3 * rng.standard_normal(n) > 0, 1.0, -1.0)
    idx = rng.choice(n, M, replace=False)
    return X, y, idx


def _close(S, K, alpha):
    want = K.K.double() @ alpha
    # two f64 evaluations of the same sum: eps64 times a condition factor; 1e-9 of the scale leaves that factor 1e7
    assert float((S - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), float((S - want).abs().max())


# cg_tolerance -> the fit's stop threshold is its square: 0 never stops; 1e3 stops in the first cg_finish (the step of
# iteration 0 taken, every later one dropped); 0.3 somewhere in between on this problem (checked below, not assumed)
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("cg_tolerance", [0.0, 1e3, 0.3])
def test_fit_accumulates_exactly_the_steps_taken(fold, cg_tolerance):
    be = CgScoresOracleBackend(fold=fold)
    X, y, idx = _problem()
    F = be.features(X)
    Zf = be.rows(F, idx)
    opt = solver.SolverOptions(cg_tolerance=cg_tolerance)
    S = torch.full((F.n,), 7.0, dtype=torch.float64)            # (the fit zeroes it)
    Ks = []
    alpha = solver.falkon_fit(be, F, be.vec(y), Zf, 4.0, 1e-3, 20, opt, knm_blocks=Ks, scores_out=S)
    plain = solver.falkon_fit(CgScoresOracleBackend(fold=fold), F, be.vec(y), Zf, 4.0, 1e-3, 20, opt)
    assert torch.equal(alpha, plain)                            # asking for scores changes nothing the fit returns
    assert be.axpy_calls == 20 and be.t_calls == 20             # one per iteration, none for the unfolded full residual
    _close(S, Ks[0], alpha)
    if cg_tolerance == 1e3:                                     # flag raised by iteration 0's cg_finish: its step stays in S
        one = solver.falkon_fit(CgScoresOracleBackend(fold=fold), F, be.vec(y), Zf, 4.0, 1e-3, 1, opt)
        assert torch.equal(alpha, one) and float(S.abs().max()) > 0
    if cg_tolerance == 0.3:
        short = [solver.falkon_fit(CgScoresOracleBackend(fold=fold), F, be.vec(y), Zf, 4.0, 1e-3, k, opt) for k in (1, 19)]
        assert torch.equal(alpha, short[1]) and not torch.equal(alpha, short[0])     # stopped after step 1, before step 20


def test_fit_without_the_entries_or_with_another_format_leaves_scores_alone():
    X, y, idx = _problem()
    for be in (OracleBackend(np.float64), CgScoresOracleBackend()):
        F = be.features(X)
        Zf = be.rows(F, idx)
        if isinstance(be, CgScoresOracleBackend):
            be.knm = lambda F, Zf, sigma, out=None, _k=OracleBackend.knm, _be=be: _k(_be, F, Zf, sigma, out=out)      # no .fmt: not a stored u24 / f32 block
        S = torch.full((F.n,), 7.0, dtype=torch.float64)
        Ks = []
        solver.falkon_fit(be, F, be.vec(y), Zf, 4.0, 1e-3, 5, knm_blocks=Ks, scores_out=S)
        assert not solver.scores_from_cg(be, Ks[0]) and bool((S == 7.0).all())


def test_lockstep_fit_on_one_rank_accumulates():
    be = CgScoresOracleBackend()
    X, y, idx = _problem()
    F = be.features(X)
    Zf = be.rows(F, idx)
    S = torch.full((F.n,), 7.0, dtype=torch.float64)
    Ks = []
    alphas = solver.falkon_fit_lockstep(be, F, [be.vec(y)], [Zf], 4.0, 1e-3, 20, knm_blocks=Ks, scores_out=[S])
    ref = solver.falkon_fit(CgScoresOracleBackend(), F, be.vec(y), Zf, 4.0, 1e-3, 20)
    assert torch.equal(alphas[0], ref)
    _close(S, Ks[0], alphas[0])


@pytest.mark.parametrize("exchange", ["lockstep", "allreduce"])
def test_job_on_one_rank_skips_knm_mv(exchange):
    """The job with scores_from_cg on (the default) against off: same alphas bit for bit, knm_mv reads no block (it is handed
    the fit's sum), scores equal to the ones it computes from the block up to the last f32 bit where the two f64 sums straddle a rounding boundary."""
    N, D, M, C = 600, 16, 40, 6
    X, cidx = _job_problem(N, D, M, C)
    row_ids = torch.arange(N)
    got = {}
    for on in (True, False):
        be = CgScoresOracleBackend()
        alphas = {}
        job = LockstepClassJob(be, torch.from_numpy(X), N, M, lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).double(),
                               [torch.from_numpy(i) for i in cidx], 6.0, 1e-4, 20, exchange=exchange, scores_from_cg=on)
        job.run(be.features(job.X), alphas_out=alphas)
        assert be.mv_calls == C                                  # one scoring call per class either way
        got[on] = (job.scores.numpy().copy(), {c: a.numpy().copy() for c, a in alphas.items()}, be.mv_reads, be.store_calls)
    (s1, a1, mv1, st1), (s2, a2, mv2, st2) = got[True], got[False]
    assert (mv1, st1) == (0, C) and (mv2, st2) == (C, 0)
    for c in range(C):
        assert np.array_equal(a1[c], a2[c]), c
    tol = 1e-9 * np.maximum(1.0, np.abs(s2).max(0)) + np.spacing(np.abs(s2))
    assert (np.abs(s1 - s2) <= tol).all(), float(np.abs(s1 - s2).max())


def test_job_without_score_from_knm_keeps_the_contraction():
    N, D, M, C = 600, 16, 40, 3
    X, cidx = _job_problem(N, D, M, C)
    row_ids = torch.arange(N)
    be = CgScoresOracleBackend()
    job = LockstepClassJob(be, torch.from_numpy(X), N, M, lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).double(),
                           [torch.from_numpy(i) for i in cidx], 6.0, 1e-4, 20, score_from_knm=False)
    job.run(be.features(job.X))
    assert job.sbuf is None and (be.mv_calls, be.store_calls, be.axpy_calls) == (0, 0, 0)
