"""knm_storage "stream" on the MI355X: the streamed CG pass (odx_gauss_ktk_stream_h2, HipBackend.ktk / ktk2 on a KnmStream)
against passes over the stored 24-bit block of the same shard, the ring's entries against that block bit for bit, FALKON fits
streamed against stored and against the f64 reference, the headline shape, and BASELINE config 5 on ONE GPU (a shard whose
stored block would not fit in HBM)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    import odx
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    b = odx.get_backend()
    yield b
    b.release_workspaces()
    torch.cuda.empty_cache()


def _storage(be, value):
    from odx import options
    return options.override(knm_storage=value)


def _operands(be, n, M, D, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn((n, D), generator=g) * (4.0 / np.sqrt(D))
    near = min(n, M // 2)                 # centres close to rows (large entries) and centres elsewhere
    Z = torch.cat([X[:near] + 0.05 * torch.randn((near, D), generator=g) / np.sqrt(D),
                   torch.randn((M - near, D), generator=g) * (4.0 / np.sqrt(D))])
    return X, Z, be.features(X.to(be.device)), be.features(Z.to(be.device))


def _stored_u24(be, F, Zf, sigma):
    """The stored block the streamed pass must reproduce: odx_gauss_knm_h2_store in 24-bit fixed point."""
    return be._knm_store(F, Zf, sigma, "u24", None, None, None)[0]


def _rel(a, b, scale):
    return float((a - b).abs().max()) / max(float(scale), 1e-300)


SHAPES = [(129, 7, 36, 5.0), (1000, 500, 256, 10.0), (40_003, 2001, 1000, 15.0), (20_011, 10_007, 1000, 15.0), (300, 20_000, 64, 4.0)]


@pytest.mark.parametrize("n,M,D,sigma", SHAPES)
def test_stream_pass_against_stored(be, n, M, D, sigma):
    """One streamed pass against ktk over the stored 24-bit block of the same shard (1e-12 relative: only the f64 summation
    order differs) and against the dense f64 product of that block; one and two vectors, with and without w, v = 0 and
    v = None; two identical calls give identical bits.  Shapes: n past several ring chunks and not a multiple of 256, M not a
    multiple of 8 or 256, D = 1000, and the widest M the compact passes serve."""
    from odx.backend import KnmStream
    from oracle import falkon_ref as fr
    X, Z, F, Zf = _operands(be, n, M, D, seed=n + M)
    K = _stored_u24(be, F, Zf, sigma)
    with _storage(be, "stream"):
        S, b0 = be.knm_rhs(F, Zf, sigma, torch.ones(n, dtype=torch.float64, device=be.device) / n)
    assert isinstance(S, KnmStream) and S.fmt == "stream"
    Kd = K.dense().double()
    g = torch.Generator(device="cpu").manual_seed(7)
    v = (torch.randn(M, generator=g, dtype=torch.float64)).to(be.device)
    v2 = (torch.randn(M, generator=g, dtype=torch.float64)).to(be.device)
    w = (torch.randn(n, generator=g, dtype=torch.float64)).to(be.device)
    zero = torch.zeros(M, dtype=torch.float64, device=be.device)

    def check(got, vv, ww):
        want_stored = be.ktk(K, v=vv, w=ww)
        t = (Kd @ vv if vv is not None else torch.zeros(n, dtype=torch.float64, device=be.device)) + (ww if ww is not None else 0)
        want = Kd.t() @ t
        scale = Kd.abs().t() @ ((Kd.abs() @ vv.abs() if vv is not None else 0) + (ww.abs() if ww is not None else 0))
        scale = float(scale.max()) if torch.is_tensor(scale) else 1.0
        assert _rel(got, want_stored, scale) <= 1e-12, (n, M, _rel(got, want_stored, scale))
        assert _rel(got, want, scale) <= 1e-12, (n, M, _rel(got, want, scale))

    check(b0, None, torch.ones(n, dtype=torch.float64, device=be.device) / n)
    for vv, ww in ((v, None), (v, w), (None, w), (zero, w)):
        got = be.ktk(S, v=vv, w=ww)
        check(got, vv, ww)
        again = be.ktk(S, v=vv, w=ww)
        assert torch.equal(got, again)                      # bitwise reproducible
    c1, c2 = be.ktk2(S, v, v2)
    check(c1, v, None)
    check(c2, v2, None)
    d1, d2 = be.ktk2(S, v, v2)
    assert torch.equal(c1, d1) and torch.equal(c2, d2)
    # both vectors and w (two reads of each resident chunk)
    o1, o2 = torch.empty_like(v), torch.empty_like(v)
    be._ktk_stream(S, v, v2, w, o1, o2)
    check(o1, v, w)
    check(o2, v2, None)
    # v = w = None: a zero vector without a pass
    o3 = torch.full_like(v, 5.0)
    be._ktk_stream(S, None, None, None, o3, None)
    assert float(o3.abs().max()) == 0.0
    # the entries themselves: the block against the dense f64 kernel (the gauss_knm bounds of the 24-bit format)
    if n * M <= 5_000_000:
        from tests.test_gpu_kernels import assert_k_close
        assert_k_close(Kd.cpu().numpy(), fr.gaussian_kernel(X.double().numpy(), Z.double().numpy(), sigma), sigma, "h2w256u24")


@pytest.mark.parametrize("n,M,D", [(40_003, 2001, 1000), (7000, 10_007, 256)])
def test_ring_holds_the_stored_entries(be, n, M, D):
    """After a pass the ring holds the last chunk of rows, bit for bit what the stored 24-bit build wrote into those rows."""
    from odx.backend import KnmStream
    sigma = 12.0
    _, _, F, Zf = _operands(be, n, M, D, seed=3 * n + M)
    K = _stored_u24(be, F, Zf, sigma)
    R = int(be.lib.odx_gauss_ktk_stream_h2_rows(M, D))
    assert R > 0 and R % 256 == 0 and n > R
    ring = torch.zeros(be._stream_bytes(n, M, D), dtype=torch.uint8, device=be.device)
    with _storage(be, "stream"):
        S = KnmStream(F, Zf, sigma, ring)
        be.ktk(S, v=torch.ones(M, dtype=torch.float64, device=be.device))
    torch.cuda.synchronize()
    r0 = (n - 1) // R * R
    rows = n - r0
    ld = K.ld
    lo_off = (R * ld * 2 + 255) // 256 * 256
    hi = ring[: R * ld * 2].view(torch.int16).view(R, ld)[:rows]
    lo = ring[lo_off: lo_off + R * ld].view(R, ld)[:rows]
    assert torch.equal(hi, K.K[r0:n]) and torch.equal(lo, K.lo[r0:n])


def test_stream_needs_the_split_kernels(be):
    from odx import options
    _, _, F, Zf = _operands(be, 300, 40, 64, seed=1)
    for gauss in ("f32", "f8"):
        with options.override(knm_storage="stream", gauss=gauss):
            with pytest.raises(ValueError):
                be.knm_format(300, 40)
            with pytest.raises(ValueError):
                be.knm_rhs(F, Zf, 5.0, torch.ones(300, dtype=torch.float64, device=be.device))
    with options.override(knm_storage="stream"):
        with pytest.raises(ValueError):
            be.knm(F, Zf, 5.0)                               # nothing stores a block under the option
        assert not be.cg_batched_supported([300], [40], "stream")


@pytest.mark.parametrize("n,M,D,sigma,lam", [(5000, 500, 256, 10.0, 1e-5), (3000, 300, 1024, 15.0, 1e-5),
                                              (777, 129, 36, 5.0, 1e-3)])
def test_falkon_fit_streamed_against_stored(be, n, M, D, sigma, lam):
    """falkon_fit with streamed passes against the same fit over the stored 24-bit block (1e-8 relative), and both against the
    f64 reference (1e-4, the parity bar of tests/test_gpu_kernels.py)."""
    import odx
    from oracle import falkon_ref as fr
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(n, D, seed=n + M)
    idx = centres(y, M, rng)
    ref, _ = fr.falkon_fit(X.astype(np.float64), y.astype(np.float64), idx, sigma, lam, maxiter=20, dtype=np.float64,
                           pc_eps=1e-5, cg_epsilon=1e-7)
    got = {}
    for storage in ("u24", "stream"):
        with _storage(be, storage):
            F = be.features(torch.from_numpy(X))
            Zf = be.rows(F, idx)
            got[storage] = odx.falkon_fit(be, F, be.vec(y), Zf, sigma, lam, 20).cpu().numpy()
    a, s = got["u24"], got["stream"]
    assert np.linalg.norm(s - a) <= 1e-8 * np.linalg.norm(a), np.linalg.norm(s - a) / np.linalg.norm(a)
    for alpha in (a, s):
        assert np.linalg.norm(alpha - ref[:, 0]) < 1e-4 * np.linalg.norm(ref[:, 0])


def _synth(be, N, D, C, M, seed=1234):
    import bench
    X = bench.synth_rows(0, N, D, C, seed, be.device)
    cidx = bench.centre_indices(N, C, M, seed)
    return X, [torch.from_numpy(i).to(be.device) for i in cidx]


def test_headline_shape_streamed_against_stored(be):
    """One class at the headline shape (N = 1e6, D = 1024, M = 1e4): alpha within 1e-8 and scores within 1e-6 of the fit over
    the stored 24-bit block (scored from the block by knm_mv; the streamed fit scores by the contraction)."""
    import odx
    N, D, M, C, sigma, lam = 1_000_000, 1024, 10_000, 30, 15.0, 1e-5
    X, cidx = _synth(be, N, D, C, M)
    y = torch.where((torch.arange(N, device=be.device) % C) == 0, 1.0, -1.0).to(torch.float64)
    res = {}
    for storage in ("u24", "stream"):
        with _storage(be, storage):
            F = be.features(X)
            Zf = be.rows(F, cidx[0])
            blocks = []
            alpha = odx.falkon_fit(be, F, y, Zf, sigma, lam, 20, knm_blocks=blocks)
            if storage == "u24":
                assert blocks[0].fmt == "u24"
                scores = be.knm_mv(blocks[0], alpha)[:, 0]
            else:
                assert blocks[0].fmt == "stream"
                scores = be.mmv(F, Zf, sigma, alpha)[:, 0]
            res[storage] = (alpha.cpu(), scores.double().cpu())
            del blocks, F, Zf
            torch.cuda.empty_cache()
    (a1, s1), (a2, s2) = res["u24"], res["stream"]
    assert float((a2 - a1).norm() / a1.norm()) <= 1e-8
    assert float((s2 - s1).abs().max()) <= 1e-6 * float(s1.abs().max())
    be.release_workspaces()
    torch.cuda.empty_cache()


def test_config5_on_one_gpu(be):
    """BASELINE config 5 (N = 5e6, D = 1024, M = 2e4) on ONE GPU, where the stored 24-bit block (300 GB) cannot exist: a
    LockstepClassJob under "stream" constructs and fits one class (finite alpha; 256 sampled scores against the dense f64
    K(x_i, Z) alpha), and one streamed pass equals the sum of stored passes over 1e6-row slices (1e-12 relative)."""
    from odx import plan
    from odx.job import LockstepClassJob
    from odx.solver import SolverOptions
    N, D, M, C, sigma, lam = 5_000_000, 1024, 20_000, 100, 15.0, 1e-5
    assert not plan.plan_lockstep(N, D, M, C, 1).feasible              # stored: the job needs more GPUs
    X, cidx = _synth(be, N, D, C, M)
    row_ids = torch.arange(N, device=be.device)
    labels = lambda c: torch.where((row_ids % C) == c, 1.0, -1.0).to(torch.float64)      # noqa: E731
    with _storage(be, "stream"):
        job = LockstepClassJob(be, X, N, M, labels, cidx[:1], sigma, lam, 20, SolverOptions(check_pivots=False), classes=1)
        assert job.plan.feasible and job.plan.knm_format == "stream"
        alphas = {}
        F = be.features(X)
        job.run(F, [0], alphas_out=alphas)
        torch.cuda.synchronize()
        alpha = alphas[0]
        assert bool(torch.isfinite(alpha).all()) and float(alpha.abs().max()) > 0
        # sampled scores against the dense f64 evaluation
        rows = torch.from_numpy(np.random.default_rng(5).choice(N, 256, replace=False)).to(be.device)
        Zd = X.index_select(0, cidx[0]).double().cpu()
        Xs = X.index_select(0, rows).double().cpu()
        d2 = (Xs * Xs).sum(1)[:, None] + (Zd * Zd).sum(1)[None, :] - 2.0 * Xs @ Zd.t()
        want = torch.exp(-d2.clamp(min=0) / (2 * sigma * sigma)) @ alpha.cpu()
        got = job.scores[:, 0].index_select(0, rows).double().cpu()
        assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
        del job
        torch.cuda.empty_cache()
        # one streamed pass against stored passes over 1e6-row slices
        Zf = be.rows(F, cidx[0])
        v = alpha.clone()
        w = labels(0) / N
        S, _ = be.knm_rhs(F, Zf, sigma, w)
        got = be.ktk(S, v=v, w=w).cpu()
    total = torch.zeros(M, dtype=torch.float64)
    scale = torch.zeros(M, dtype=torch.float64)
    step = 1_000_000
    for lo in range(0, N, step):
        Fs = be.rows(F, torch.arange(lo, lo + step, device=be.device))
        K = _stored_u24(be, Fs, Zf, sigma)
        total += be.ktk(K, v=v, w=w[lo:lo + step]).cpu()
        scale += be.ktk(K, v=v.abs(), w=w[lo:lo + step].abs()).cpu()
        del K, Fs
        torch.cuda.empty_cache()
    assert float((got - total).abs().max()) <= 1e-12 * float(scale.max())
    be.release_workspaces()
    torch.cuda.empty_cache()
