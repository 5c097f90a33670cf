"""Scores summed from the CG's own passes on the GPU: the passes' t_out (odx_knm_fwd_bwd[2][_q]_t) against an f64 K v of the
decoded block, `out` bitwise unchanged by it; the accumulated scores (odx_cg_scores_axpy_f64 / _store_f32 through
solver.falkon_fit) against knm_mv of the same block and alpha; the job with the path on and off."""
import contextlib

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_knm_mv import _block                                  # noqa: E402  (stored blocks with known entries)


@pytest.fixture(scope="module")
def be():
    import odx
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return odx.get_backend()


def _vec(n, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, generator=g, dtype=torch.float64).to(dev)


def _t_out_buffer(n, dev):
    big = torch.full((n + 64,), -7.0, dtype=torch.float64, device=dev)
    return big, big[:n]


def _check_rows(big, t, K, v):
    want = K.dense().double().cpu() @ v.cpu()
    err = float((t.cpu() - want).abs().max())
    print("t_out: max |K v - f64 reference| = %.3e at scale %.3e (%s, n = %d, M = %d)" % (err, float(want.abs().max()), K.fmt, K.n, K.M))
    assert err <= 1e-12 * float(want.abs().max()), (K.fmt, K.n, K.M, err)
    assert bool((big[K.n:] == -7.0).all())                            # rows >= n are not written


# the staggered kernel's widths (chunks <= 512, <= 1024 and the headline's 8192 < M <= 10240), the barrier form's
# (M <= 1024, 4096 < M <= 8192, M > 10240), n never a multiple of the row block (16, 8, 4, 3, 2, 4, 1 rows)
@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,M", [(1001, 300), (1003, 2000), (1001, 3001), (1001, 6000), (4099, 10_000), (4099, 8200), (1001, 11_000),
                                 (301, 13_000), (1, 10_000)])
def test_one_vector_pass_t_out_compact(be, fmt, n, M):
    K = _block(be, n, M, fmt, seed=n + M)
    v, w = _vec(M, 1, be.device), _vec(n, 2, be.device)
    plain = be.ktk(K, v=v, w=w)
    big, t = _t_out_buffer(n, be.device)
    out = be.ktk(K, v=v, w=w, t_out=t)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)                                    # the pass's own result: bit for bit
    _check_rows(big, t, K, v)                                         # ... and K v before w is added


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,M", [(4099, 10_000), (1001, 4100), (513, 8193)])
def test_two_vector_pass_t_out_compact(be, fmt, n, M):
    K = _block(be, n, M, fmt, seed=n + M + 1)
    assert be.can_ktk2(K)
    v1, v2 = _vec(M, 3, be.device), _vec(M, 4, be.device)
    p1, p2 = be.ktk2(K, v1, v2)
    big, t = _t_out_buffer(n, be.device)
    o1, o2 = be.ktk2(K, v1, v2, t_out=t)
    torch.cuda.synchronize()
    assert torch.equal(o1, p1) and torch.equal(o2, p2)
    _check_rows(big, t, K, v1)                                        # the FIRST vector's products


@pytest.mark.parametrize("n,M", [(37, 3), (1001, 300), (1003, 2000), (1001, 4100), (515, 10_000), (301, 13_000)])
def test_one_vector_pass_t_out_f32(be, n, M):
    K = _block(be, n, M, "f32", seed=n + M + 2)
    v, w = _vec(M, 5, be.device), _vec(n, 6, be.device)
    plain = be.ktk(K, v=v, w=w)
    big, t = _t_out_buffer(n, be.device)
    out = be.ktk(K, v=v, w=w, t_out=t)
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
    _check_rows(big, t, K, v)


@pytest.mark.parametrize("n,M", [(1001, 4100), (515, 10_000)])
def test_two_vector_pass_t_out_f32(be, n, M):
    K = _block(be, n, M, "f32", seed=n + M + 3)
    assert be.can_ktk2(K)
    v1, v2 = _vec(M, 7, be.device), _vec(M, 8, be.device)
    p1, p2 = be.ktk2(K, v1, v2)
    big, t = _t_out_buffer(n, be.device)
    o1, o2 = be.ktk2(K, v1, v2, t_out=t)
    torch.cuda.synchronize()
    assert torch.equal(o1, p1) and torch.equal(o2, p2)
    _check_rows(big, t, K, v1)


def test_t_out_is_refused_where_it_cannot_be_given(be):
    K = _block(be, 64, 300, "f32", seed=1)
    with pytest.raises(ValueError):
        be.ktk(K, w=_vec(64, 1, be.device), t_out=torch.empty(64, dtype=torch.float64, device=be.device))      # no v
    with pytest.raises(ValueError):
        be.ktk(K, v=_vec(300, 1, be.device), t_out=torch.empty(63, dtype=torch.float64, device=be.device))     # wrong length


def test_scores_axpy_and_store(be):
    n = 100_003
    t, S0 = _vec(n, 9, be.device), _vec(n, 10, be.device)
    for flag, a in ((0.0, 0.37), (1.0, 0.37)):
        state = torch.tensor([1.0, 1.0, flag, a], dtype=torch.float64, device=be.device)
        S = S0.clone()
        be.cg_scores_axpy(state, t, S)
        want = S0 if flag else torch.addcmul(S0, t, torch.tensor(a, dtype=torch.float64, device=be.device))
        # one fma per entry against a rounded product plus a rounded sum
        assert float((S - want).abs().max()) <= 4.5e-16 * float((S0.abs() + a * t.abs()).max())
    big = torch.full((n, 3), -7.0, dtype=torch.float32, device=be.device)
    be.cg_scores_store(S0, big[:, 1:2])
    torch.cuda.synchronize()
    assert torch.equal(big[:, 1], S0.float()) and bool((big[:, 0] == -7.0).all()) and bool((big[:, 2] == -7.0).all())


def _fit_scores(be, storage, n, D, M, cg_tolerance, maxiter=20):
    import odx
    from odx.solver import SolverOptions
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(n, D, seed=77)
    idx = centres(y, M, rng)
    prev, be.knm_storage = be.knm_storage, storage
    try:
        F = be.features(torch.from_numpy(X))
        Zf = be.rows(F, idx)
        S = torch.full((n,), 7.0, dtype=torch.float64, device=be.device)
        Ks = []
        opt = SolverOptions(cg_tolerance=cg_tolerance)
        ph = lambda name: contextlib.nullcontext()                    # noqa: E731  (a phase hook: all three fits run the statement loop)
        alpha = odx.falkon_fit(be, F, be.vec(y), Zf, 10.0, 1e-5, maxiter, opt, knm_blocks=Ks, scores_out=S, phase=ph)
        plain = odx.falkon_fit(be, F, be.vec(y), Zf, 10.0, 1e-5, maxiter, opt, phase=ph)
        first = odx.falkon_fit(be, F, be.vec(y), Zf, 10.0, 1e-5, 1, opt, phase=ph)
        K = Ks[0]
        got = torch.empty((n, 1), dtype=torch.float32, device=be.device)
        be.cg_scores_store(S, got)
        want = be.knm_mv(K, alpha)
        torch.cuda.synchronize()
        return K.fmt, alpha.cpu(), plain.cpu(), first.cpu(), got[:, 0].cpu(), want[:, 0].cpu()
    finally:
        be.knm_storage = prev
        be.release_workspaces()
        torch.cuda.empty_cache()


# (storage, n, M): an f32 block on the small one-vector kernel; a 24-bit block wide and tall enough for the folded two-vector pass
# of iteration 10 (4096 < M, n >= 8 M).  cg_tolerance: the stop threshold is its square — 0 never stops, 1e3 stops in the cg_finish
# of iteration 0: the one step taken must be in the scores, none of the later ones.
@pytest.mark.parametrize("cg_tolerance", [0.0, 1e3])
@pytest.mark.parametrize("storage,n,M", [("f32", 3001, 300), ("u24", 33_001, 4100)])
def test_accumulated_scores_equal_knm_mv(be, storage, n, M, cg_tolerance):
    fmt, alpha, plain, first, got, want = _fit_scores(be, storage, n, 64, M, cg_tolerance)
    assert fmt == storage
    assert torch.equal(alpha, plain)                                  # asking for the scores changes nothing in the fit
    if cg_tolerance > 0:
        assert torch.equal(alpha, first)                              # the flag went up behind step 1 ...
    else:
        assert not torch.equal(alpha, first)                          # ... or never
    d = (got.double() - want.double()).abs()
    scale = max(1.0, float(want.abs().max()))
    print("max |scores(CG) - scores(knm_mv)| = %.3e at scale %.3e (%s)" % (float(d.max()), scale, fmt))
    # both are f64 sums rounded once to f32: one f32 ulp where the two f64 values straddle a rounding boundary, plus the f64
    # sums' own difference (eps64 times a condition factor; 1e-9 of the scale leaves that factor 1e7)
    tol = torch.from_numpy(__import__("numpy").spacing(want.abs().numpy())).double() + 1e-9 * scale
    assert bool((d <= tol).all()), float((d / tol).max())
    assert float(want.abs().max()) > 0


def test_job_scores_from_cg_against_knm_mv(be):
    """LockstepClassJob at N = 1e5, M = 1e4 (24-bit blocks, the staggered kernel and the folded two-vector pass): with
    scores_from_cg (the default) no odx_knm_mv launch is made, alpha is bit for bit the other path's, scores agree to f32 rounding."""
    import bench
    from odx.job import LockstepClassJob
    from odx.solver import SolverOptions

    def _job_scores(scores_from_cg):
        """alphas, scores and the number of odx_knm_mv launches (reads of a stored block) of one job run."""
        reads = []
        orig = be.lib.odx_knm_mv
        be.lib.odx_knm_mv = lambda *a: (reads.append(1), orig(*a))[1]
        try:
            alphas = {}
            job = LockstepClassJob(be, X, N, M, labels, cidx, 15.0, 1e-5, 20, SolverOptions(check_pivots=False), classes=len(run),
                                   scores_from_cg=scores_from_cg)
            job.run(be.features(X), run, alphas_out=alphas)
            torch.cuda.synchronize()
            out = ({c: alphas[c].cpu() for c in run}, job.scores[:, list(run)].cpu(), len(reads))
            job.release()
        finally:
            be.lib.odx_knm_mv = orig
            be.release_workspaces()
            torch.cuda.empty_cache()
        return out
    N, D, M, C = 100_000, 1024, 10_000, 30
    dev = be.device
    seed = 1234 + 3
    X = bench.synth_rows(0, N, D, C, seed, dev)
    cidx = [torch.from_numpy(i).to(dev) for i in bench.centre_indices(N, C, M, seed)]
    row_ids = torch.arange(N, device=dev)
    labels = lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).to(torch.float64)            # noqa: E731
    run = [0, 1, 2]
    assert be.knm_format(N, M) == "u24"
    summed = _job_scores(True)
    stored = _job_scores(False)
    assert summed[2] == 0 and stored[2] == len(run)
    for c in run:
        assert torch.equal(summed[0][c], stored[0][c]), c
    d = (summed[1].double() - stored[1].double()).abs()
    scale = max(1.0, float(stored[1].abs().max()))
    print("max |scores(CG) - scores(knm_mv)| = %.3e at scale %.3e" % (float(d.max()), scale))
    tol = torch.from_numpy(__import__("numpy").spacing(stored[1].abs().numpy())).double() + 1e-9 * scale
    assert bool((d <= tol).all()), float((d / tol).max())
