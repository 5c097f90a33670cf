"""The lambda path on the MI355X: the NV-vector pass over compact K_nM blocks (odx_knm_fwd_bwdn_q), HipBackend.ktkn /
ktkn_width / precond_path, and odx.falkon_fit_path against the f64 oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def storage(be):
    old = (be.gauss, be.knm_storage)
    yield be
    be.gauss, be.knm_storage = old
    be.pin_gauss_tile(0)


def _compact_block(rng, n, M, fmt):
    """A random K block in [0, 1] stored as `fmt` (u24 / bf16) with the library's layout, and the f64 values it encodes."""
    from odx.backend import Knm
    ld = (M + 7) // 8 * 8
    K = Knm()
    K.n, K.M, K.ld, K.fmt = n, M, ld, fmt
    if fmt == "u24":
        q = rng.integers(0, 1 << 24, (n, ld), dtype=np.int64)
        q[:, M:] = 0
        q[0, 0], q[-1, M - 1] = (1 << 24) - 1, 0                       # the extreme codes
        K.K = torch.from_numpy((q >> 8).astype(np.uint16).view(np.int16)).cuda()
        K.lo = torch.from_numpy((q & 255).astype(np.uint8)).cuda()
        vals = q[:, :M].astype(np.float64) * 2.0 ** -24
    else:
        f = rng.random((n, ld)).astype(np.float32)
        f[:, M:] = 0
        bits = (f.view(np.uint32) >> 16).astype(np.uint16)
        K.K = torch.from_numpy(bits.view(np.int16)).cuda()
        vals = (bits.astype(np.uint32) << 16).view(np.float32)[:, :M].astype(np.float64)
    return K, vals


# (n, M, NV): odd M, n not a multiple of any row block, n smaller than one block, every configuration of both widths,
# and M on both sides of each LDS limit (8 vectors: 2524 | 2525 -> served as 4 + ..; 4 vectors: 5084 | 5085 -> none)
PASS_SHAPES = [(777, 129, 3), (1, 100, 4), (3, 1023, 8), (1501, 1000, 8), (2001, 2000, 8), (999, 2045, 5), (530, 2524, 8),
               (530, 2525, 4), (2001, 2000, 4), (1000, 4000, 4), (515, 4099, 3), (300, 5084, 4)]


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,M,nv", PASS_SHAPES)
def test_nv_vector_pass(be, fmt, n, M, nv):
    """out[q] = K'(K v[q]) from one read: against the dense f64 product at 1e-11 max|ref| and against the single-vector pass
    at 1e-12 max|single| (the bounds of test_two_vector_pass_equals_two_passes), guard cells untouched, bit-repeatable."""
    rng = np.random.default_rng(n * 31 + M + nv)
    K, vals = _compact_block(rng, n, M, fmt)
    assert np.array_equal(K.dense().cpu().numpy().astype(np.float64), vals)
    assert be.ktkn_width(K) >= nv
    ld = (M + 1) // 2 * 2 + 6
    Vh = rng.standard_normal((nv, ld)) * np.logspace(0, -3, nv)[:, None]
    V = torch.from_numpy(Vh).cuda()
    out = torch.full((nv, ld), float("nan"), dtype=torch.float64, device="cuda")
    be.ktkn(K, V, out=out)
    assert torch.isnan(out[:, M:]).all()
    for q in range(nv):
        ref = vals.T @ (vals @ Vh[q, :M])
        err = np.abs(out[q, :M].cpu().numpy() - ref).max()
        assert err <= 1e-11 * np.abs(ref).max(), (q, err, np.abs(ref).max())
        single = be.ktk(K, v=V[q, :M].contiguous())
        assert float((out[q, :M] - single).abs().max()) <= 1e-12 * float(single.abs().max()), q
    again = torch.full_like(out, float("nan"))
    be.ktkn(K, V, out=again)
    assert torch.equal(again[:, :M], out[:, :M])


def test_widths_and_the_limits_of_the_entry(be):
    from odx import hip
    rng = np.random.default_rng(5)
    for M, want in ((2000, 8), (2524, 8), (2525, 4), (4000, 4), (5084, 4), (5085, 2), (10000, 2)):
        K, _ = _compact_block(rng, 8, M, "u24")
        assert be.ktkn_width(K) == want, (M, be.ktkn_width(K))
    lib = be.lib
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 2524, hip.KNM_U24, 8) > 0
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 2525, hip.KNM_U24, 8) < 0
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 2525, hip.KNM_U24, 5) < 0
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 5085, hip.KNM_BF16, 3) < 0
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 2000, hip.KNM_F32, 4) < 0
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 2000, hip.KNM_U24, 2) < 0
    assert lib.odx_knm_fwd_bwdn_q_workspace_bytes(1000, 2000, hip.KNM_U24, 9) < 0


def _against_single_passes(be, K, L, rng):
    M = K.M
    ld = (M + 1) // 2 * 2
    V = torch.from_numpy(rng.standard_normal((L, ld)) * 1e-2).cuda()
    out = be.ktkn(K, V)
    assert tuple(out.shape) == (L, ld)
    for l in range(L):
        single = be.ktk(K, v=V[l, :M].contiguous())
        assert float((out[l, :M] - single).abs().max()) <= 1e-12 * float(single.abs().max()), l


def test_ktkn_groups_f32_blocks_and_streamed_shards(be, storage):
    from odx.backend import Knm
    from tests.synth import blob_problem, centres
    rng = np.random.default_rng(11)
    K, _ = _compact_block(rng, 1200, 2000, "u24")
    assert be.ktkn_width(K) == 8
    _against_single_passes(be, K, 11, rng)                              # groups of 8 + 2 + 1 (no two-vector pass at M = 2000)
    K4, _ = _compact_block(rng, 700, 4500, "u24")
    assert be.ktkn_width(K4) == 4 and be.can_ktk2(K4)
    _against_single_passes(be, K4, 10, rng)                             # 4 + 4 + a two-vector pass
    Kf = Knm()
    f = rng.random((900, 300)).astype(np.float32)
    Kf.K, Kf.n, Kf.M, Kf.ld = torch.from_numpy(f).cuda(), 900, 300, 300
    assert be.ktkn_width(Kf) in (1, 2)
    _against_single_passes(be, Kf, 5, rng)
    X, y, r2 = blob_problem(3000, 64, seed=3)
    idx = centres(y, 300, r2)
    be.gauss, be.knm_storage = "h2", "stream"
    F = be.features(torch.from_numpy(X))
    S, _ = be.knm_rhs(F, be.rows(F, idx), 10.0, be.vec(y) / 3000)
    assert S.fmt == "stream" and be.ktkn_width(S) == 2
    _against_single_passes(be, S, 5, rng)


@pytest.mark.parametrize("M,D", [(1000, 256), (4100, 64)])
def test_precond_path_members_equal_single_preconditioners(be, M, D):
    """All four factors of every member bit for bit those of precond(lam_l), in the all-f64 chain and in the split-f16 chain
    (from 4096 centres on)."""
    rng = np.random.default_rng(M)
    Z = (rng.standard_normal((M, D)) * (20.0 / np.sqrt(D))).astype(np.float32)
    Zf = be.features(torch.from_numpy(Z))
    lams = [1e-3, 1e-6, 1e-4]
    Ps = be.precond_path(Zf, 15.0, lams, 1e-5)
    assert len(Ps) == 3 and Ps[0].LTi.data_ptr() == Ps[2].LTi.data_ptr() and Ps[0].LAi.data_ptr() != Ps[1].LAi.data_ptr()
    for P, lam in zip(Ps, lams):
        P1 = be.precond(Zf, 15.0, lam, 1e-5)
        assert int(P.info.item()) == 0 and int(P1.info.item()) == 0
        for name in ("LTi", "LTit", "LAi", "LAit"):
            a, b = getattr(P1, name), getattr(P, name)
            assert torch.equal(a, b), (lam, name, float((a - b).abs().max()))
    P0 = be.precond_path(Zf, 15.0, [1e-4], 1e-5)[0]                      # a path of one: factored in place
    assert torch.equal(P0.LAi, Ps[2].LAi) and torch.equal(P0.LTit, Ps[2].LTit)
    if M == 1000:                                                       # a failed Cholesky of L_T is every member's
        bad = be.features(torch.zeros((50, D)))
        assert all(int(P.info.item()) != 0 for P in be.precond_path(bad, 15.0, [0.0, 0.0], 0.0))


# rows of the reference's shipped (sigma, M, D) grid (tests/test_gpu_kernels.py REFERENCE_GRID) with the distinct penalties
# shipped at each: detector (D = 2048), on-line RPN (D = 1024), on-line segmentation (D = 256)
PATH_GRID = [
    (15.0, 2000, 2048, [1e-3, 1e-5]),
    (15.0, 1000, 2048, [1e-5, 1e-4]),
    (50.0, 1000, 1024, [1e-5, 1e-3]),
    (10.0, 500, 256, [1e-6]),
    (25.0, 500, 256, [1e-7]),
    (5.0, 2000, 2048, [1e-4, 1e-3, 1e-5, 1e-6, 1e-7]),      # one (sigma, M, D) under every distinct penalty the reference ships
]


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


@pytest.mark.parametrize("knm", ["f32", "u24"])
@pytest.mark.parametrize("sigma,M,D,lams", PATH_GRID)
def test_path_on_the_reference_grid(be, storage, knm, sigma, M, D, lams):
    """alpha < 1e-4 relative and scores < 1e-4 max(1, max|ref|) against the f64 oracle at every penalty: the project's bars."""
    be.gauss, be.knm_storage = "h2", knm
    be.pin_gauss_tile(256 if knm == "u24" else 0)
    X, y, idx = _grid_rows(sigma, M, D)
    K = _check_path(be, X, y, idx, sigma, lams)
    assert K.fmt == knm


def test_path_on_an_hbm_bound_block(be, storage):
    """2e5 x 2000, D = 256 (config 4's alpha-checked size), 24-bit storage: the passes are the 8-wide kernel."""
    from tests.synth import blob_problem, centres
    be.gauss, be.knm_storage = "h2", "u24"
    X, y, rng = blob_problem(200000, 256, seed=77)
    idx = centres(y, 2000, rng)
    K = _check_path(be, X, y, idx, 10.0, [1e-6, 1e-5, 1e-4, 1e-3])
    assert K.fmt == "u24" and be.ktkn_width(K) == 8


def test_estimator_fit_path_on_the_gpu(be):
    import odx
    from odx.wrappers import CenterSelector
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(3000, 64, seed=9)
    idx = centres(y, 300, rng)
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    mk = lambda pen: odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=8.0), penalty=pen, M=len(idx), maxiter=20,      # noqa: E731
                                      center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
    models = mk(1e-3).fit_path(Xt, yt, [1e-5, 1e-4])
    for e, lam in zip(models, [1e-5, 1e-4]):
        one = mk(lam).fit(Xt, yt)
        assert float((e.alpha_ - one.alpha_).norm() / one.alpha_.norm()) < 1e-6
        assert float((e.predict(Xt[:100]) - one.predict(Xt[:100])).abs().max()) < 1e-5
