"""knm_storage "stream" without a GPU: the option, the memory plan, and the host logic (solver.falkon_fit, LockstepClassJob)
driven by an oracle backend whose K_nM shards are never stored — every pass recomputes K — against the stored-mode oracle,
in one process and under gloo at world sizes 2 and 3."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from odx import options, plan
from tests.oracle_backend import OracleBackend
from tests.test_dist_gloo import _free_port, _job_problem

GB = 1e9


class _Stream:
    """What StreamOracleBackend.knm_rhs hands out: no block, the operands to recompute it from."""
    fmt = "stream"

    def __init__(self, F, Zf, sigma):
        self.F, self.Zf, self.sigma, self.n, self.M = F, Zf, sigma, F.n, Zf.n
        self.K = F.X


class StreamOracleBackend(OracleBackend):
    """The oracle backend under knm_storage "stream": K recomputed inside every pass and the builds counted; any stored
    block (knm) or a read of one (knm_mv) fails the test."""
    gauss = "h2"
    knm_storage = "stream"

    def __init__(self):
        super().__init__(np.float64)
        self.builds = 0
        self.passes = 0

    def knm_format(self, n, M):
        return "stream"

    def knm_bytes(self, n, M, D=None):
        return 1 << 10

    def knm(self, F, Zf, sigma, out=None):
        raise AssertionError("a K_nM block was stored under knm_storage 'stream'")

    def knm_mv(self, K, alpha, out=None):
        raise AssertionError("knm_mv called on a streamed shard")

    def _build(self, K):
        self.builds += 1
        blk = super().knm(K.F, K.Zf, K.sigma)
        assert blk.K.shape == (K.n, K.M)
        return blk

    def knm_rhs(self, F, Zf, sigma, w, out=None, rhs_out=None):
        K = _Stream(F, Zf, sigma)
        return K, self.ktk(K, w=w, out=rhs_out)

    def ktk(self, K, v=None, w=None, out=None):
        assert K.fmt == "stream"
        self.passes += 1
        return super().ktk(self._build(K), v=v, w=w, out=out)

    def ktk2(self, K, v1, v2, out1=None, out2=None):
        self.passes += 1
        blk = self._build(K)                 # one build serves both vectors
        return super().ktk(blk, v=v1, out=out1), super().ktk(blk, v=v2, out=out2)

    def cg_batched_supported(self, ns, Ms, fmt="f32"):
        return fmt != "stream"


# ---------------------------------------------------------------- option and plan

def test_option_accepts_stream_and_default_is_unchanged():
    assert options.Options().knm_storage == "auto"
    assert "stream" in options._CHOICES["knm_storage"]
    assert options._coerce("knm_storage", "stream") == "stream"
    loaded = options.Options()
    try:
        options.reset()
        assert options.load({"ODX_KNM": "stream"}).knm_storage == "stream"
    finally:
        options.reset()
    assert options.current().knm_storage == "auto" and loaded.knm_storage == "auto"
    with pytest.raises(ValueError):
        options._coerce("knm_storage", "streamed")


def test_auto_never_streams():
    for n, M in ((5_000_000, 20_000), (1_000_000, 10_000), (100, 10)):
        assert plan.knm_format_rule(n, M) != "stream"
    assert plan.knm_format_rule(5_000_000, 20_000, "stream") == "stream"
    assert not plan.plan_lockstep(5e6, 1024, 2e4, 100, 1).feasible          # auto at one GPU stays infeasible


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_config5_feasible_streamed(world):
    p = plan.plan_lockstep(5e6, 1024, 2e4, 100, world, storage="stream")
    assert p.feasible, p.summary()
    assert p.knm_format == "stream"
    assert p.parts["knm_shards"] <= p.b * plan.STREAM_BYTES
    assert p.parts["knm_shards"] == p.b * plan.knm_bytes_rule(p.n_loc, 2e4, "stream")
    assert p.total_bytes <= 0.9 * 288 * GB
    # a streamed shard costs its ring whatever the rows: far below one stored 24-bit shard of the same rows
    assert plan.knm_bytes_rule(p.n_loc, 20_000, "stream") * 50 < plan.knm_bytes_rule(p.n_loc, 20_000, "u24")


# ---------------------------------------------------------------- host logic against the stored-mode oracle

def _problem(N=2400, D=16, M=40, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)).astype(np.float32)
    X *= 5.0 / np.linalg.norm(X, axis=1).mean()
    y = np.where(rng.random(N) < 0.3, 1.0, -1.0)
    idx = rng.choice(N, M, replace=False)
    return X, y, idx


def _fit(be, X, y, idx, sigma=5.0, lam=1e-4, maxiter=25):
    from odx import solver
    F = be.features(torch.from_numpy(X))
    Zf = be.features(torch.from_numpy(X[idx]))
    return solver.falkon_fit(be, F, torch.from_numpy(y), Zf, sigma, lam, maxiter=maxiter).numpy().copy()


def test_falkon_fit_streamed_matches_stored():
    X, y, idx = _problem()
    stored = _fit(OracleBackend(np.float64), X, y, idx)
    be = StreamOracleBackend()
    streamed = _fit(be, X, y, idx)
    assert np.abs(streamed - stored).max() <= 1e-12 * np.abs(stored).max()
    assert be.builds == be.passes and be.passes < 25 + 5          # one build per pass; the full residuals were folded in


def _job_run(be, X, N, M, C, shard, exchange="lockstep"):
    from odx.job import LockstepClassJob
    lo, hi = shard.bounds(N)
    row_ids = torch.arange(lo, hi)
    X, cidx = X
    job = LockstepClassJob(be, torch.from_numpy(X[lo:hi]), N, M, lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).double(),
                           [torch.from_numpy(i) for i in cidx], 6.0, 1e-4, 20, shard=shard, exchange=exchange)
    alphas = {}
    job.run(be.features(job.X), alphas_out=alphas)
    return job.scores.numpy().copy(), {c: a.numpy().copy() for c, a in alphas.items()}


def _compare(got, ref):
    (s1, a1), (s2, a2) = got, ref
    assert sorted(a1) == sorted(a2)
    for c in a2:
        assert np.abs(a1[c] - a2[c]).max() <= 1e-12 * max(1.0, np.abs(a2[c]).max()), c
    assert np.abs(s1 - s2).max() <= 1e-12 * max(1.0, np.abs(s2).max()) + np.spacing(np.abs(s2)).max()


def test_lockstep_job_streamed_matches_stored():
    import odx
    from odx.dist import RowShard
    N, D, M, C = 2400, 16, 40, 6
    prob = _job_problem(N, D, M, C)
    try:
        ref_be = OracleBackend(np.float64)
        odx.set_backend(ref_be)
        ref = _job_run(ref_be, prob, N, M, C, RowShard())
        be = StreamOracleBackend()
        odx.set_backend(be)
        got = _job_run(be, prob, N, M, C, RowShard())
    finally:
        odx.set_backend(None)
    _compare(got, ref)
    assert be.builds == be.passes > 0


def _worker(rank, world, port, N, D, M, C, exchange, ret):
    torch.cuda.is_available = lambda: False
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import odx
        from odx.dist import RowShard
        prob = _job_problem(N, D, M, C)
        ref_be = OracleBackend(np.float64)
        odx.set_backend(ref_be)
        ref = _job_run(ref_be, prob, N, M, C, RowShard(), exchange)
        be = StreamOracleBackend()
        odx.set_backend(be)
        got = _job_run(be, prob, N, M, C, RowShard(), exchange)
        ret[rank] = (got, ref, be.builds, be.passes)
    finally:
        odx.set_backend(None)
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("exchange", ["lockstep", "allreduce"])
def test_lockstep_job_streamed_gloo(world, exchange):
    N, D, M, C = 2400, 16, 40, 6
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), N, D, M, C, exchange, ret), nprocs=world, join=True)
    assert sorted(ret.keys()) == list(range(world))
    for r in range(world):
        got, ref, builds, passes = ret[r]
        _compare(got, ref)
        assert builds == passes > 0
