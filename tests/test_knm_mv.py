"""odx_knm_mv (HipBackend.knm_mv): scores as one read of a stored K_nM block, and the job's scoring from the blocks its fits
stored (LockstepClassJob(score_from_knm=True)) against the Gaussian contraction it replaces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    import odx
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return odx.get_backend()


def _block(be, n, M, fmt, seed):
    """A stored block of the given format with random entries in [0, 1] (pad columns zero, as the builds leave them)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    K = be._knm_block(n, M, fmt, None)
    v = torch.rand((n, M), generator=g, dtype=torch.float64)
    if fmt == "u24":
        q = torch.zeros((n, K.ld), dtype=torch.int32)
        q[:, :M] = torch.round(v * 2.0 ** 24).clamp(max=2 ** 24 - 1).to(torch.int32)
        K.K.copy_(((q >> 8) & 0xFFFF).to(torch.int16).to(be.device))       # (bit pattern: values >= 2^15 wrap to negative int16)
        K.lo.copy_((q & 0xFF).to(torch.uint8).to(be.device))
    elif fmt == "f32":
        w = torch.zeros((n, K.ld), dtype=torch.float32)
        w[:, :M] = v.float()
        K.K.copy_(w.to(be.device))
    else:
        w = torch.zeros((n, K.ld), dtype=torch.float32)
        w[:, :M] = v.float()
        K.K.copy_((w.view(torch.int32) >> 16).to(torch.int16).to(be.device))
    return K


def _check(be, K, seed, ldo=1, col=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    alpha = torch.randn(K.M, generator=g, dtype=torch.float64) * 10.0
    want = K.dense().double().cpu() @ alpha
    bound = K.dense().double().cpu().abs() @ alpha.abs()
    big = torch.full((K.n, ldo), -7.0, dtype=torch.float32, device=be.device)
    out = big[:, col:col + 1]
    be.knm_mv(K, alpha.to(be.device), out=out)
    torch.cuda.synchronize()
    got = out[:, 0].double().cpu()
    # f64 sums rounded once to f32: half an f32 ulp of the value, plus the f64 summation's own error
    tol = 6.0e-8 * want.abs() + 1e-13 * bound + 1e-30
    err = (got - want).abs()
    assert bool((err <= tol).all()), (K.fmt, K.n, K.M, float((err / tol).max()))
    others = torch.cat([big[:, :col], big[:, col + 1:]], dim=1)
    assert bool((others == -7.0).all())                     # a strided column: nothing else written
    return out.clone(), alpha


@pytest.mark.parametrize("fmt", ["u24", "f32", "bf16"])
@pytest.mark.parametrize("n,M", [(1, 1), (1, 10_000), (37, 3), (3, 2000), (1001, 2000), (513, 8193), (777, 10_000),
                                 (301, 20_000), (70_001, 1000)])
def test_knm_mv_against_dense_f64(be, fmt, n, M):
    """Every format against a dense f64 K @ alpha of the same stored block: n = 1, tails shorter than a row group, widths
    from 1 to 20 000 columns, a shard long enough that every wave walks several row groups; output into a strided column."""
    K = _block(be, n, M, fmt, seed=n * 31 + M)
    _check(be, K, seed=M, ldo=5, col=3)


@pytest.mark.parametrize("fmt", ["u24", "f32", "bf16"])
def test_knm_mv_row_subblock_and_repeatability(be, fmt):
    """A row sub-block of a stored shard (Knm.rows) is a valid argument, and two launches agree bit for bit."""
    K = _block(be, 4099, 10_000, fmt, seed=5)
    sub = K.rows(1001, 3000)
    a, alpha = _check(be, sub, seed=9)
    b = torch.empty_like(a)
    be.knm_mv(sub, alpha.to(be.device), out=b)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_knm_mv_rejects_what_it_cannot_hold(be):
    import odx
    K = _block(be, 4, 30_000, "f32", seed=1)
    with pytest.raises(odx.hip.OdxError):
        be.knm_mv(K, torch.zeros(30_000, dtype=torch.float64, device=be.device))


def _job_scores(be, X, N, M, C, run, labels, cidx, score_from_knm, shard=None):
    from odx.job import LockstepClassJob
    from odx.solver import SolverOptions
    calls = []
    orig = be.knm_mv
    be.knm_mv = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        alphas = {}
        job = LockstepClassJob(be, X, N, M, labels, cidx, 15.0, 1e-5, 20, SolverOptions(check_pivots=False), classes=C, shard=shard,
                               score_from_knm=score_from_knm)
        job.run(be.features(X), run, alphas_out=alphas)
        torch.cuda.synchronize()
        out = ({c: alphas[c].cpu() for c in run}, job.scores[:, list(run)].cpu(), len(calls))
        job.release()
    finally:
        del be.knm_mv
        be.release_workspaces()
        torch.cuda.empty_cache()
    return out


def _compare(a, b):
    (al1, sc1, _), (al2, sc2, _) = a, b
    for c in al1:
        assert torch.equal(al1[c], al2[c]), c                  # nothing before alpha changed
    assert torch.isfinite(sc1).all() and torch.isfinite(sc2).all()
    d = float((sc1 - sc2).abs().max())
    scale = max(1.0, float(sc2.abs().max()))
    print("max |scores(stored block) - scores(contraction)| = %.3e (scale %.3e)" % (d, scale))
    assert d <= 1e-5 * scale, (d, scale)


@pytest.mark.parametrize("storage", ["auto", "f32", "bf16"])
def test_job_scores_from_stored_blocks(be, storage):
    """LockstepClassJob at N = 1e5, M = 1e4 (test_headline_kernels_alpha_at_m1e4's shape), scored from the stored blocks and
    by the contraction: alpha identical bit for bit, scores within 1e-5 of the scale for 24-bit and f32 storage.  bf16 blocks
    are ~1e-3 off, so the job must keep recomputing their scores."""
    import bench
    N, D, M, C = 100_000, 1024, 10_000, 30
    dev = be.device
    seed = 1234 + 3
    X = bench.synth_rows(0, N, D, C, seed, dev)
    cidx = [torch.from_numpy(i).to(dev) for i in bench.centre_indices(N, C, M, seed)]
    row_ids = torch.arange(N, device=dev)
    labels = lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).to(torch.float64)            # noqa: E731
    run = [0, 1, 2]
    prev, be.knm_storage = be.knm_storage, storage
    try:
        assert be.knm_format(N, M) == {"auto": "u24", "f32": "f32", "bf16": "bf16"}[storage]
        stored = _job_scores(be, X, N, M, len(run), run, labels, cidx, True)
        contraction = _job_scores(be, X, N, M, len(run), run, labels, cidx, False)
    finally:
        be.knm_storage = prev
    assert contraction[2] == 0
    if storage == "bf16":
        assert stored[2] == 0                                  # routed to the contraction
    else:
        assert stored[2] == len(run)
    _compare(stored, contraction)


def test_emulated_rank_scores_from_stored_blocks(be):
    """The same comparison for ONE rank of an 8-rank job (odx.dist.EmulatedShard, bench.py --emulate-world): the lock-step
    batches of 8 classes with their owner rotation and alpha gathers — every class is scored from its own block with its own
    alpha."""
    import bench
    from odx.dist import EmulatedShard
    world, rank = 8, 0
    N, D, M, C = 8 * 20_000, 1024, 10_000, 10
    dev = be.device
    seed = 1234 + 3
    shard = EmulatedShard(world, rank)
    lo, hi = shard.bounds(N)
    X = bench.synth_rows(lo, hi, D, C, seed, dev)

    def fold(idx):                                             # bench.py's folding of the centres onto this rank's rows
        cls = idx % C
        first = lo + ((cls - lo) % C)
        cnt = np.maximum((hi - first + C - 1) // C, 1)
        return first + C * ((idx // C) % cnt)
    cidx = [torch.from_numpy(fold(i)).to(dev) for i in bench.centre_indices(N, C, M, seed)]
    row_ids = torch.arange(lo, hi, device=dev)
    labels = lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).to(torch.float64)            # noqa: E731
    run = list(range(C))
    assert be.knm_format(hi - lo, M) in ("u24", "f32")
    stored = _job_scores(be, X, N, M, C, run, labels, cidx, True, shard=shard)
    contraction = _job_scores(be, X, N, M, C, run, labels, cidx, False, shard=EmulatedShard(world, rank))
    assert stored[2] == C and contraction[2] == 0
    _compare(stored, contraction)
