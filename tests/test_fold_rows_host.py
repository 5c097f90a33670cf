"""The CG's fold step over accumulated scores without a GPU: the launch sequence of solver._cg_run with and without scores
(the tests' oracle backend with a ktk_rows, through test_solver_schedule's recorder), the routes that must never reach the
new entry, the arithmetic of the schedule (S = K T^-1 A^-1 x at the fold, also under a raised stop flag), and the calls and
refusals of HipBackend.ktk_rows against the recording fake library of tests/test_knm_calls_host.py."""
import numpy as np
import pytest
import torch

from odx import hip, solver
from odx.cols import column_map
from odx.job import LockstepClassJob
from tests.oracle_backend import OracleBackend
from tests.test_dist_gloo import _job_problem
from tests.test_knm_calls_host import Rec
from tests.test_scores_from_cg_host import CgScoresOracleBackend, _close, _problem
from tests.test_solver_schedule import LoggedShard, Recorder, StoredPathBackend, _Phase


class FoldRowsOracleBackend(CgScoresOracleBackend):
    """CgScoresOracleBackend with the one-forward / two-backward pass: out1 = K'(K v), out2 = K' s, t_out = K v."""
    rows_on = True

    def __init__(self, fold=True):
        super().__init__(fold=fold)
        self.rows_calls = 0
        self.seen_s = []

    def can_ktk_rows(self, K):
        return self.rows_on and self.can_ktk2(K)

    def ktk_rows(self, K, v, s, out1=None, out2=None, t_out=None):
        self.rows_calls += 1
        self.seen_s.append(s.clone())
        return self.ktk(K, v=v, out=out1, t_out=t_out), OracleBackend.ktk(self, K, w=s, out=out2)


def _fit(be, maxiter=20, cg_tolerance=1e-7, scores=True, log=None, **kw):
    X, y, idx = _problem()
    F = be.features(X)
    S = torch.full((F.n,), 7.0, dtype=torch.float64) if scores else None
    Ks = []
    rec = be if log is None else Recorder(be, log)
    alpha = solver.falkon_fit(rec, F, be.vec(y), be.rows(F, idx), 4.0, 1e-3, maxiter, solver.SolverOptions(cg_tolerance=cg_tolerance),
                              knm_blocks=Ks, scores_out=S, **kw)
    return alpha, S, Ks[0]


def _launches(log):
    return [e for e in log if not e.startswith("phase")]


def _route_off_log():
    """The log of the fit with scores and the route switched off: the two-vector fold with a t_out."""
    log = []
    be = FoldRowsOracleBackend()
    be.rows_on = False
    _fit(be, log=log)
    assert be.rows_calls == 0 and "ktk2:t_out" in log
    return log


def test_launch_sequence_of_the_fold_iteration():
    """Iteration 9 (the 10th: the full residual) where the rank can sum the row products: A^-1 of both vectors, T^-1 of the
    direction only, one ktk_rows, the unchanged tail; where it cannot (a block that does not qualify for scores_from_cg): the
    two-vector sequence as it was."""
    with_scores, without = [], []
    be = FoldRowsOracleBackend()
    _fit(be, log=with_scores, phase=lambda name: _Phase(with_scores, name))
    other = FoldRowsOracleBackend()
    other.gauss = None                                              # scores_from_cg(be, K) does not hold: nothing is summed
    _fit(other, scores=False, log=without)
    assert other.rows_calls == 0 and other.axpy_calls == 0
    got = _launches(with_scores)
    i = got.index("ktk_rows")
    assert got[i - 3:i + 8] == ["trmv:LAit", "trmv:LTit", "trmv:LAit", "ktk_rows", "trmv:LTi", "trmv:LAi", "trmv:LTi", "trmv:LAi",
                                "cg_step:full=1", "cg_scores_axpy", "cg_residual"]
    assert got.count("ktk_rows") == 1 and "ktk2" not in got and "ktk2:t_out" not in got and be.rows_calls == 1
    old = _launches(without)
    j = old.index("ktk2")
    assert old[j - 4:j + 7] == ["trmv:LAit", "trmv:LTit", "trmv:LAit", "trmv:LTit", "ktk2", "trmv:LTi", "trmv:LAi", "trmv:LTi", "trmv:LAi",
                                "cg_step:full=1", "cg_residual"]
    assert "ktk_rows" not in old
    # against the same fit with the route off: one product with T's inverse fewer, the pass swapped, nothing else
    off = _launches(_route_off_log())
    same = lambda seq: [e for e in seq if e not in ("ktk_rows", "ktk2:t_out")]      # noqa: E731
    j = off.index("ktk2:t_out")
    assert same(got) == same(off[:j - 1] + off[j:]) and off[j - 1] == "trmv:LTit"
    # the phase of the launch stays the fold's
    k = with_scores.index("ktk_rows")
    assert with_scores[k - 1] == "phase+ktk2" and with_scores[k + 1] == "phase-ktk2"


@pytest.mark.parametrize("cg_tolerance", [0.0, 1e3, 0.3])
def test_fold_over_scores_is_the_two_vector_fold_up_to_rounding(cg_tolerance):
    """alpha and S against the route switched off; S = K alpha; and at the fold the pass was handed S_old = K T^-1 A^-1 x_old,
    also when the stop flag went up before it (0.3: somewhere before iteration 10 on this problem; 1e3: in iteration 0)."""
    on, off = FoldRowsOracleBackend(), FoldRowsOracleBackend()
    off.rows_on = False
    a1, S1, K = _fit(on, cg_tolerance=cg_tolerance)
    a0, S0, _ = _fit(off, cg_tolerance=cg_tolerance)
    assert on.rows_calls == 1 and off.rows_calls == 0
    rel = float((a1 - a0).norm() / a0.norm())
    assert rel <= 1e-9, rel
    _close(S1, K, a1)
    # what the fold read: the scores of the first nine steps — K alpha of the fit stopped after nine iterations
    a9, S9, _ = _fit(FoldRowsOracleBackend(), maxiter=9, cg_tolerance=cg_tolerance)
    assert torch.equal(on.seen_s[0], S9)
    _close(on.seen_s[0], K, a9)
    if cg_tolerance > 0:
        # the flag was up before the fold: X and S froze together, the fold changed neither
        assert torch.equal(a1, a9) and torch.equal(S1, S9)


def test_asking_for_scores_changes_nothing_in_the_fit():
    """A fit that could sum its row products sums them whether or not the caller wants them (a buffer of its own): the same
    launches, the same alpha bit for bit."""
    asked, silent = FoldRowsOracleBackend(), FoldRowsOracleBackend()
    a1, S, K = _fit(asked)
    a0, none, _ = _fit(silent, scores=False)
    assert none is None and torch.equal(a1, a0)
    assert (asked.rows_calls, asked.axpy_calls, asked.t_calls) == (silent.rows_calls, silent.axpy_calls, silent.t_calls) == (1, 20, 20)
    # the lock-step driver on one rank alike
    X, y, idx = _problem()
    for scores in (True, False):
        be = FoldRowsOracleBackend()
        F = be.features(X)
        S = [torch.full((F.n,), 7.0, dtype=torch.float64)] if scores else None
        al = solver.falkon_fit_lockstep(be, F, [be.vec(y)], [be.rows(F, idx)], 4.0, 1e-3, 20, scores_out=S)
        assert be.rows_calls == 1 and torch.equal(al[0], a1)


def test_routes_without_scores_never_call_the_entry():
    X, y, idx = _problem()
    # a block that does not qualify for scores_from_cg; no fold
    nosum = FoldRowsOracleBackend()
    nosum.gauss = None
    for be, scores in ((nosum, False), (nosum, True), (FoldRowsOracleBackend(fold=False), True)):
        _fit(be, scores=scores)
        assert be.rows_calls == 0
    # owner mode over row shards: the owner alone holds the step sizes, nobody accumulates
    be = FoldRowsOracleBackend()
    log = []
    F = be.features(X)
    S = torch.full((F.n,), 7.0, dtype=torch.float64)
    solver.falkon_fit(be, F, be.vec(y), be.rows(F, idx), 4.0, 1e-3, 20, shard=LoggedShard(2, 0, log), owner=0, n_total=2 * F.n, scores_out=S)
    assert be.rows_calls == 0 and bool((S == 7.0).all())
    # a lambda path and a multi-output fit over a stored block
    class Both(StoredPathBackend, FoldRowsOracleBackend):
        pass
    for fit in (lambda b, F: solver.falkon_fit_path(b, F, b.vec(y), b.rows(F, idx), 4.0, [1e-4, 1e-3], 20),
                lambda b, F: solver.falkon_fit_multi(b, F, torch.stack([b.vec(y), -b.vec(y)], 1), b.rows(F, idx), 4.0, 1e-3, 20)):
        b = Both()
        fit(b, b.features(torch.from_numpy(X)))
        assert b.rows_calls == 0


def test_replicated_shards_sum_both_partials():
    """The allreduce form over a shard object without an owner: every rank accumulates its own rows, the fold reads them, the
    (2, Mp) matrix of partials goes through the one exchange that exists."""
    be = FoldRowsOracleBackend()
    log = []
    _fit(be, log=log, shard=LoggedShard(1, 0, log))
    assert be.rows_calls == 1
    i = log.index("ktk_rows")
    assert log[i + 1].startswith("all_reduce:")                     # the pass's partials, before anything reads them
    assert int(log[i + 1].split(":")[1]) == 2 * 40 * 8               # both rows of the exchange matrix


@pytest.mark.parametrize("exchange", ["lockstep", "allreduce"])
def test_job_on_one_rank_folds_over_the_scores(exchange):
    N, D, M, C = 600, 16, 40, 3
    X, cidx = _job_problem(N, D, M, C)
    row_ids = torch.arange(N)
    got = {}
    for on in (True, False):
        be = FoldRowsOracleBackend()
        be.rows_on = on
        alphas = {}
        job = LockstepClassJob(be, torch.from_numpy(X), N, M, lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).double(),
                               [torch.from_numpy(i) for i in cidx], 6.0, 1e-4, 20, exchange=exchange)
        job.run(be.features(job.X), alphas_out=alphas)
        assert be.rows_calls == (C if on else 0)
        got[on] = {c: a.numpy().copy() for c, a in alphas.items()}
    for c in range(C):
        rel = np.linalg.norm(got[True][c] - got[False][c]) / np.linalg.norm(got[False][c])
        assert rel <= 1e-9, (c, rel)


# ------------------------------------------------------------------------------------------------- the wrapper's calls
N_, M_ = 10, 21


def test_wrapper_calls():
    r = Rec()
    K = r.block("u24", N_, M_)
    o1, o2 = r.be.ktk_rows(K, r.vec("v", M_), r.vec("s", N_), out1=r.vec("o1", M_), out2=r.vec("o2", M_), t_out=r.vec("t", N_))
    (call,) = r.calls
    assert call[0] == "odx_knm_fwd_bwd_q_rows_t" and len(call) - 1 == len(hip.SIGNATURES["odx_knm_fwd_bwd_q_rows_t"][1])
    assert call[1:8] == [["K", 0], K.ld, ["Klo", 0], K.ld, hip.KNM_U24, N_, M_]
    assert call[8:13] == [["v", 0], ["s", 0], ["o1", 0], ["o2", 0], ["t", 0]]
    # the workspace: twice the two-vector pass's
    assert r.ws == [["ktk", 2 * (64 + 16 * (1 * N_ + 2 * M_ + 3 * hip.KNM_U24))]] and call[13] == ["ws:ktk", 0] and call[14] == r.ws[0][1]
    assert call[15] is None
    assert o1.data_ptr() == r.named["o1"].data_ptr() and o2.data_ptr() == r.named["o2"].data_ptr()
    # a block of distinct columns: the _cols entry, vectors of the list's length, the map behind Mv
    r = Rec()
    idx = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6]
    cmap = column_map(torch.tensor(idx))
    K = r.block("bf16", N_, cmap.Md)
    K.cmap, K.Mv = cmap, cmap.Mv
    for name, t in zip(("first", "col_of", "start", "pos"), cmap.on("cpu")):
        r.t("map." + name, t)
    r.be.ktk_rows(K, r.vec("v", M_), r.vec("s", N_))
    (call,) = r.calls
    assert call[0] == "odx_knm_fwd_bwd_q_rows_cols_t" and call[6:8] == [N_, 9] and call[12] is None
    assert call[15:] == [M_, ["map.col_of", 0], ["map.start", 0], ["map.pos", 0], None]


def test_wrapper_refusals():
    r = Rec()
    K = r.block("u24", N_, M_)
    with pytest.raises(ValueError):
        r.be.ktk_rows(K, r.vec("v", M_), None)                       # null s
    with pytest.raises(ValueError):
        r.be.ktk_rows(K, r.vec("v", M_), r.vec("s", N_ - 1))         # not the block's rows
    with pytest.raises(ValueError):
        r.be.ktk_rows(r.block("f32", N_, M_), r.vec("v", M_), r.vec("s2", N_))
    assert r.calls == []
    # an unsupported width: the predicate says no, the call raises before any launch
    r = Rec(unsupported=["odx_knm_fwd_bwd2_q_workspace_bytes"])
    K = r.block("u24", N_, M_)
    assert not r.be.can_ktk_rows(K)
    with pytest.raises(hip.OdxError):
        r.be.ktk_rows(K, r.vec("v", M_), r.vec("s", N_))
    assert r.calls == []
    r = Rec(width=1)                                                 # no two-vector pass at this width: no fold, no rows pass
    assert not r.be.can_ktk_rows(r.block("u24", N_, M_))
    r = Rec()
    assert r.be.can_ktk_rows(r.block("u24", N_, M_)) and not r.be.can_ktk_rows(r.block("f32", N_, M_))
    r.be.fold_rows = False
    assert not r.be.can_ktk_rows(r.block("u24", N_, M_))


def test_the_library_keeps_its_pass_names_and_refuses_without_a_launch():
    """The real library without a GPU: odx_knm_pass_kernel_name answers for nv = 1, 2 as before (bench.py asks it), and the
    new entry refuses a null s, a null out and a width outside the two-vector rule before it touches a device."""
    import ctypes
    lib = hip.load()
    assert lib.odx_knm_pass_kernel_name(10_000, hip.KNM_U24, 1) == b"knm_passq_stag_kernel<10,2,1>"
    assert lib.odx_knm_pass_kernel_name(10_000, hip.KNM_U24, 2) == b"knm_passq_kernel<512,5,2,2,1,2>"
    buf = torch.zeros(1 << 16, dtype=torch.float64)
    p = ctypes.c_void_p(buf.data_ptr())

    def call(M, v=p, s=p, out2=p):
        return lib.odx_knm_fwd_bwd_q_rows_t(p, (M + 7) // 8 * 8, p, (M + 7) // 8 * 8, hip.KNM_U24, 5, M, v, s, p, out2, None, p, buf.numel() * 8, None)
    # ODX_ERR_INVALID = -1, ODX_ERR_UNSUPPORTED = -3 (include/odx.h)
    assert call(4100, s=None) == -1 and call(4100, v=None) == -1 and call(4100, out2=None) == -1
    for M in (300, 4096, 10_204, 12_000):
        assert int(lib.odx_knm_fwd_bwd2_q_workspace_bytes(5, M, hip.KNM_U24)) < 0 and call(M) == -3
