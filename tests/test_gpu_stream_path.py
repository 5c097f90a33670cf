"""A lambda path over streamed shards on the MI355X: odx_gauss_ktk_stream_h2n (several vectors from ONE build of K),
HipBackend.ktkn / ktkn_span on a KnmStream against single streamed passes and against the stored 24-bit block of the same
rows, and odx.falkon_fit_path under knm_storage "stream" against the stored path and the f64 oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MIB = 1 << 20


@pytest.fixture(scope="module")
def be():
    import odx
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    b = odx.get_backend()
    yield b
    b.release_workspaces()
    torch.cuda.empty_cache()


def _storage(value):
    from odx import options
    return options.override(knm_storage=value)


def _operands(be, n, M, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn((n, D), generator=g) * (4.0 / np.sqrt(D))
    near = min(n, M // 2)                 # centres close to rows (large entries) and centres elsewhere
    Z = torch.cat([X[:near] + 0.05 * torch.randn((near, D), generator=g) / np.sqrt(D),
                   torch.randn((M - near, D), generator=g) * (4.0 / np.sqrt(D))])
    return be.features(X.to(be.device)), be.features(Z.to(be.device))


def _stream_shard(be, F, Zf, sigma, ring=None):
    from odx.backend import KnmStream
    be.pack(F), be.pack(Zf)
    return KnmStream(F, Zf, sigma, ring)


def test_symbol_limits_and_span(be):
    """The entry exists; its workspace twin refuses nv = 0, 17 and M = 20441 and stays within the 256 MiB per streamed shard
    that odx/plan.py counts, for every group configuration; one build serves 16 vectors while a read of the ring serves 2."""
    from odx import hip, plan
    lib = be.lib
    assert hasattr(lib, "odx_gauss_ktk_stream_h2n") and hip.STREAM_MAX_VECTORS == 16
    wb = lib.odx_gauss_ktk_stream_h2n_workspace_bytes
    assert wb(1000, 2000, 64, 0) < 0 and wb(1000, 2000, 64, 17) < 0 and wb(1000, 20441, 64, 4) < 0
    assert wb(0, 2000, 64, 4) == 0 and wb(1000, 20440, 64, 16) > 0
    assert plan.STREAM_BYTES == 256 * MIB
    for M in (300, 2000, 2524, 2525, 5084, 5085, 10_000, 10_007, 20_000):
        for D in (64, 1024, 2048):
            R = int(lib.odx_gauss_ktk_stream_h2n_rows(M, D))
            assert R > 0 and R % 256 == 0, (M, D, R)
            for nv in (1, 8, 16):
                nbytes = int(wb(1_000_000, M, D, nv))
                assert 0 < nbytes <= 256 * MIB, (M, D, nv, nbytes)
                assert nbytes >= R * ((M + 7) // 8 * 8) * 3
    F, Zf = _operands(be, 600, 300, 64, seed=2)
    with _storage("stream"):
        S, _ = be.knm_rhs(F, Zf, 5.0, torch.ones(600, dtype=torch.float64, device=be.device))
        assert S.fmt == "stream" and be.ktkn_span(S) == 16 and be.ktkn_width(S) == 2
    K = be._knm_store(F, Zf, 5.0, "u24", None, None, None)[0]
    assert be.ktkn_span(K) == be.ktkn_width(K) == 8


# (M, D, sigma, rows past two whole chunks): every group kernel — the 8-wide pass (M = 300, 2001), the 4-wide (4500), the
# two-vector pass (4500 behind the 4-wide groups; 8000, where it is the widest), singles (remainders everywhere; 10 007 and
# 20 000 have nothing else) — and a ragged last chunk that is not a multiple of 256 rows
PASS_SHAPES = [(300, 64, 4.0, 777), (2001, 1000, 15.0, 1003), (4500, 256, 10.0, 515), (8000, 128, 8.0, 901), (10_007, 1000, 15.0, 1301),
               (20_000, 64, 4.0, 300)]
NVS = (1, 2, 3, 5, 8, 11, 16)


@pytest.mark.parametrize("M,D,sigma,tail", PASS_SHAPES)
def test_ktkn_on_a_streamed_shard(be, M, D, sigma, tail):
    """Each row of ktkn over a streamed shard, for nv in NVS, against ktk on the same streamed shard and against ktk / ktkn on
    the stored 24-bit block of the same rows: <= 1e-12 max|reference row| (the same entries; only the f64 summation order
    differs — the bound of test_stream_pass_against_stored and _against_single_passes).  Two calls give identical bits; a
    caller's ring that is large enough, and one that is too small (the backend's workspace serves), give those bits too."""
    R = int(be.lib.odx_gauss_ktk_stream_h2n_rows(M, D))
    n = 2 * R + tail
    assert n % R != 0 and n % 256 != 0
    F, Zf = _operands(be, n, M, D, seed=n + M)
    K = be._knm_store(F, Zf, sigma, "u24", None, None, None)[0]
    S = _stream_shard(be, F, Zf, sigma)
    ld = (M + 1) // 2 * 2
    g = torch.Generator(device="cpu").manual_seed(M)
    V = (torch.randn((16, ld), generator=g, dtype=torch.float64) * torch.logspace(0, -3, 16, dtype=torch.float64)[:, None]).to(be.device)
    single_stream = [be.ktk(S, v=V[q, :M].contiguous()) for q in range(16)]
    single_stored = [be.ktk(K, v=V[q, :M].contiguous()) for q in range(16)]
    worst = 0.0
    for nv in NVS:
        out = torch.full((nv, ld), float("nan"), dtype=torch.float64, device=be.device)
        be.ktkn(S, V[:nv], out=out)
        assert torch.isnan(out[:, M:]).all() and bool(torch.isfinite(out[:, :M]).all())
        stored_n = be.ktkn(K, V[:nv])
        for q in range(nv):
            for name, ref in (("streamed ktk", single_stream[q]), ("stored ktk", single_stored[q]), ("stored ktkn", stored_n[q, :M])):
                err = float((out[q, :M] - ref).abs().max()) / float(ref.abs().max())
                worst = max(worst, err)
                assert err <= 1e-12, (M, nv, q, name, err)
        again = torch.full_like(out, float("nan"))
        be.ktkn(S, V[:nv], out=again)
        assert torch.equal(again[:, :M], out[:, :M])
        if nv in (5, 16):
            need = int(be.lib.odx_gauss_ktk_stream_h2n_workspace_bytes(n, M, D, nv))
            for nbytes in (need, 4096):
                ring = torch.zeros(nbytes, dtype=torch.uint8, device=be.device)
                got = be.ktkn(_stream_shard(be, F, Zf, sigma, ring), V[:nv])
                assert torch.equal(got[:, :M], out[:, :M]), (nv, nbytes)
                if nbytes == 4096:
                    assert int(ring.max()) == 0                      # never written
    print("M=%d D=%d n=%d (R=%d): worst row error %.2e of max|reference row|" % (M, D, n, R, worst))


def test_no_rows_gives_zeros(be):
    F, Zf = _operands(be, 64, 40, 36, seed=5)
    S = _stream_shard(be, F, Zf, 5.0)
    S.n = 0
    out = torch.full((3, 40), 7.0, dtype=torch.float64, device=be.device)
    be.ktkn(S, torch.ones((3, 40), dtype=torch.float64, device=be.device), out=out)
    assert float(out.abs().max()) == 0.0


# test_falkon_fit_streamed_against_stored's shapes, each with its penalty.  A path needs several penalties: the shape's own and
# the two decades ABOVE it.  The 1e-8 bar was established at each shape's own penalty; the preconditioned system gets better
# conditioned as the penalty grows, so rounding differences are amplified less and the bar carries over upwards, not downwards.
@pytest.mark.parametrize("n,M,D,sigma,lam", [(5000, 500, 256, 10.0, 1e-5), (3000, 300, 1024, 15.0, 1e-5), (777, 129, 36, 5.0, 1e-3)])
def test_path_streamed_against_stored(be, n, M, D, sigma, lam):
    """falkon_fit_path under "stream" (full residual folded into the step's build) against the same path over the stored 24-bit
    block (plain residual): <= 1e-8 relative per member, the bar of test_falkon_fit_streamed_against_stored.

    A first version of this test also fitted lam / 10.  At (3000, 300, 1024) and lam = 1e-6 that member read 2.3e-8 — and so
    does code this path does not touch: falkon_fit streamed against falkon_fit stored, the existing test's own comparison,
    reads 2.0e-8 at that penalty, and the streamed path WITHOUT the fold 1.6e-8 against the stored path.  Below a shape's own
    penalty the f64 summation order alone (chunks of rows against one sweep) moves alpha by more than the bar, so the
    comparison says nothing about the fold there; the other two shapes read 7.8e-10 and 7.0e-13 at lam / 10."""
    import odx
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(n, D, seed=n + M)
    idx = centres(y, M, rng)
    lams = [lam, lam * 10, lam * 100]
    got = {}
    for storage in ("u24", "stream"):
        with _storage(storage):
            F = be.features(torch.from_numpy(X))
            Zf = be.rows(F, idx)
            blocks = []
            got[storage] = odx.falkon_fit_path(be, F, be.vec(y), Zf, sigma, lams, 20, knm_blocks=blocks).cpu().numpy()
            assert blocks[0].fmt == storage
    for l, lm in enumerate(lams):
        a, s = got["u24"][l], got["stream"][l]
        rel = np.linalg.norm(s - a) / np.linalg.norm(a)
        print("n=%d M=%d lam=%g: streamed against stored %.2e" % (n, M, lm, rel))
        assert rel <= 1e-8, (lm, rel)


# two rows of tests/test_gpu_falkon_path.py PATH_GRID: two penalties, and every distinct penalty the reference ships (L = 5:
# the folded iteration sends 10 vectors through one build)
PATH_ROWS = [(15.0, 2000, 2048, [1e-3, 1e-5]), (5.0, 2000, 2048, [1e-4, 1e-3, 1e-5, 1e-6, 1e-7])]


def _grid_rows(sigma, M, D, n=8000):
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(n, D, seed=int(sigma * 1000) + M + D)
    return X, y, centres(y, M, rng)


def _check_path(be, X, y, idx, sigma, lams, alpha_bar=1e-4):
    import odx
    from oracle import falkon_ref as fr
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    blocks = []
    alphas = odx.falkon_fit_path(be, F, be.vec(y), Zf, sigma, lams, 20, knm_blocks=blocks)
    assert tuple(alphas.shape) == (len(lams), Zf.n) and len(blocks) == 1
    scores = be.mmv(F, Zf, sigma, alphas.t().contiguous()).cpu().numpy()
    for l, lam in enumerate(lams):
        ref, Z = fr.falkon_fit(X.astype(np.float64), y.astype(np.float64), idx, sigma, lam, maxiter=20, dtype=np.float64,
                               pc_eps=1e-5, cg_epsilon=1e-7)
        rel = np.linalg.norm(alphas[l].cpu().numpy() - ref[:, 0]) / np.linalg.norm(ref[:, 0])
        pref = fr.falkon_predict(X.astype(np.float64), Z, ref, sigma)[:, 0]
        serr = np.abs(scores[:, l] - pref).max()
        print("sigma=%g M=%d lam=%g fmt=%s: alpha rel err %.2e, score err %.2e (max |ref| %.2f)"
              % (sigma, Zf.n, lam, blocks[0].fmt, rel, serr, np.abs(pref).max()))
        assert rel < alpha_bar, (lam, rel)
        assert serr < 1e-4 * max(1.0, float(np.abs(pref).max())), (lam, serr)
    return blocks[0]


@pytest.mark.parametrize("sigma,M,D,lams", PATH_ROWS)
def test_streamed_path_on_the_reference_grid(be, sigma, M, D, lams):
    """alpha < 1e-4 relative and scores < 1e-4 max(1, max|ref|) against the f64 oracle at every penalty: the project's bars."""
    X, y, idx = _grid_rows(sigma, M, D)
    with _storage("stream"):
        K = _check_path(be, X, y, idx, sigma, lams)
    assert K.fmt == "stream"


def test_estimator_fit_path_streamed(be):
    """InCoreFalkon.fit_path under knm_storage "stream" equals per-penalty fit (1e-6, as test_estimator_fit_path_on_the_gpu)."""
    import odx
    from odx import options
    from odx.wrappers import CenterSelector
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(3000, 64, seed=9)
    idx = centres(y, 300, rng)
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    mk = lambda pen: odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=8.0), penalty=pen, M=len(idx), maxiter=20,      # noqa: E731
                                      center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
    with options.override(knm_storage="stream"):
        models = mk(1e-3).fit_path(Xt, yt, [1e-5, 1e-4])
        for e, lam in zip(models, [1e-5, 1e-4]):
            one = mk(lam).fit(Xt, yt)
            assert float((e.alpha_ - one.alpha_).norm() / one.alpha_.norm()) < 1e-6
            assert float((e.predict(Xt[:100]) - one.predict(Xt[:100])).abs().max()) < 1e-5


def test_headline_shape_path_streamed_against_stored(be):
    """N = 1e6, D = 1024, M = 1e4, L = 4 (the shipped range of penalties): the streamed path (one build of K per CG iteration,
    pairs of vectors over the resident chunk) within 1e-8 per member of the path over the stored 24-bit block."""
    import bench
    import odx
    N, D, M, C, sigma = 1_000_000, 1024, 10_000, 30, 15.0
    lams = [1e-6, 1e-5, 1e-4, 1e-3]
    X = bench.synth_rows(0, N, D, C, 1234, be.device)
    cidx = torch.from_numpy(bench.centre_indices(N, C, M, 1234)[0]).to(be.device)
    y = torch.where((torch.arange(N, device=be.device) % C) == 0, 1.0, -1.0).to(torch.float64)
    res = {}
    for storage in ("u24", "stream"):
        with _storage(storage):
            F = be.features(X)
            Zf = be.rows(F, cidx)
            blocks = []
            res[storage] = odx.falkon_fit_path(be, F, y, Zf, sigma, lams, 20, knm_blocks=blocks).cpu()
            assert blocks[0].fmt == storage
            del blocks, F, Zf
            be.release_workspaces()
            torch.cuda.empty_cache()
    for l, lam in enumerate(lams):
        a, s = res["u24"][l], res["stream"][l]
        rel = float((s - a).norm() / a.norm())
        print("lam=%g: streamed against stored %.2e" % (lam, rel))
        assert rel <= 1e-8, (lam, rel)
