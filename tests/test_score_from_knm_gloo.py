"""LockstepClassJob's scoring from the stored K_nM blocks (score_from_knm) under 8 gloo ranks on the CPU: a backend that
offers knm_mv (the tests' oracle backend with a dense one) must score every class from ITS OWN block and alpha in both
exchange forms — the lock-step batches with rotating owners and the replicated all-reduce form — and give the scores the
Gaussian contraction (mmv) gives."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.oracle_backend import OracleBackend
from tests.test_dist_gloo import _free_port, _job_problem


class KnmMvOracleBackend(OracleBackend):
    """The oracle backend with f32-stored, f32-accurate blocks (as HipBackend's under gauss "h2") and a dense knm_mv."""
    gauss = "h2"

    def __init__(self):
        super().__init__(np.float64)
        self.mv_calls = 0

    def knm(self, F, Zf, sigma, out=None):
        K = super().knm(F, Zf, sigma, out=out)
        K.fmt = "f32"
        return K

    def knm_mv(self, K, alpha, out=None):
        self.mv_calls += 1
        r = (K.K.double() @ alpha.double()).float()[:, None]
        if out is not None:
            out.copy_(r)
            return out
        return r


def _worker(rank, world, port, N, D, M, C, exchange, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import odx
        from odx.dist import RowShard
        from odx.job import LockstepClassJob
        be = KnmMvOracleBackend()
        odx.set_backend(be)
        X, cidx = _job_problem(N, D, M, C)
        shard = RowShard()
        lo, hi = shard.bounds(N)
        row_ids = torch.arange(lo, hi)
        got = {}
        for from_knm in (True, False):
            be.mv_calls = 0
            alphas = {}
            job = LockstepClassJob(be, torch.from_numpy(X[lo:hi]), N, M, lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).double(),
                                   [torch.from_numpy(i) for i in cidx], 6.0, 1e-4, 20, shard=shard, exchange=exchange,
                                   score_from_knm=from_knm)
            job.run(be.features(job.X), alphas_out=alphas)
            got[from_knm] = (job.scores.numpy().copy(), {c: a.numpy().copy() for c, a in alphas.items()}, be.mv_calls)
        ret[rank] = got
    finally:
        odx.set_backend(None)
        dist.destroy_process_group()


def _run(exchange):
    N, D, M, C, world = 2400, 16, 40, 30, 8
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), N, D, M, C, exchange, ret), nprocs=world, join=True)
    assert sorted(ret.keys()) == list(range(world))
    for r in range(world):
        (s1, a1, calls1), (s2, a2, calls2) = ret[r][True], ret[r][False]
        assert calls1 == C and calls2 == 0, (r, calls1, calls2)        # every class scored from its block on every rank
        assert sorted(a1) == list(range(C))
        for c in range(C):
            assert np.array_equal(a1[c], a2[c]), (r, c)
        # the same f64 value rounded to f32 both ways, up to the last bit where the two f64 sums straddle a rounding boundary
        tol = 1e-9 * np.maximum(1.0, np.abs(s2).max(0)) + np.spacing(np.abs(s2))
        assert (np.abs(s1 - s2) <= tol).all(), (r, float(np.abs(s1 - s2).max()))


def test_lockstep_job_scores_each_class_from_its_own_block():
    _run("lockstep")


def test_replicated_job_scores_each_class_from_its_own_block():
    _run("allreduce")
