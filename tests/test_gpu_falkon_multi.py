"""The multi-output fit on the MI355X: K' W for up to 8 weight vectors from one read of a compact block (odx_knm_bwdn_q), the
triangular product of up to 8 vectors from one read of a factor (odx_trmvn_f64), HipBackend.ktwn / trmvn, and
odx.falkon_fit_multi against the f64 oracle."""
import ctypes

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
    """A random K block in [0, 1] stored as `fmt` (u24 / bf16) with the library's layout, and the f64 values it encodes
    (as tests/test_gpu_falkon_path.py makes them)."""
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


# (n, M, nv): odd M, n below one row block (2 .. 8 rows, by width) and not a multiple of it, one and several column bands,
# M on both sides of the NV pass's LDS limits and up to the limit of the compact passes, every nv
BWD_SHAPES = [(777, 129, 3), (1, 100, 4), (3, 1023, 8), (7, 100, 2), (1501, 1000, 8), (2001, 2000, 8), (999, 2045, 5), (530, 2525, 7),
              (1001, 2000, 1), (1003, 2000, 2), (515, 5085, 6), (401, 10000, 8), (203, 10000, 3), (131, 20440, 8), (64, 20440, 4)]


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,M,nv", BWD_SHAPES)
def test_backward_nv_pass(be, fmt, n, M, nv):
    """out[q] = K' W[q] from one read: against the dense f64 product at 1e-11 max|ref| and against ktk(K, w=W[q]) at 1e-12
    max|single| (the bounds of test_nv_vector_pass), guard cells untouched, bit-repeatable."""
    from odx import hip
    rng = np.random.default_rng(n * 31 + M + nv)
    K, vals = _compact_block(rng, n, M, fmt)
    ldo, ldw = (M + 1) // 2 * 2 + 6, (n + 1) // 2 * 2 + 4
    Wh = np.zeros((nv, ldw))
    Wh[:, :n] = rng.standard_normal((nv, n)) * np.logspace(0, -3, nv)[:, None]
    Wh[:, n:] = np.nan                                      # weights past n are never read into a sum
    W = torch.from_numpy(Wh).cuda()
    code = {"u24": hip.KNM_U24, "bf16": hip.KNM_BF16}[fmt]
    nbytes = be.lib.odx_knm_bwdn_q_workspace_bytes(n, M, code, nv)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def run():
        out = torch.full((nv, ldo), float("nan"), dtype=torch.float64, device="cuda")
        hip.check(be.lib.odx_knm_bwdn_q(ctypes.c_void_p(K.K.data_ptr()), K.ld, ctypes.c_void_p(K.lo.data_ptr()) if fmt == "u24" else None,
                                        K.ld, code, n, M, nv, ctypes.c_void_p(W.data_ptr()), ldw, ctypes.c_void_p(out.data_ptr()), ldo,
                                        ctypes.c_void_p(ws.data_ptr()), nbytes, None), "odx_knm_bwdn_q")
        torch.cuda.synchronize()
        return out
    out = run()
    assert torch.isnan(out[:, M:]).all()
    for q in range(nv):
        ref = vals.T @ Wh[q, :n]
        err = np.abs(out[q, :M].cpu().numpy() - ref).max()
        print("n=%d M=%d nv=%d %s q=%d: err %.2e of max|ref| %.2e" % (n, M, nv, fmt, q, err, np.abs(ref).max()))
        assert err <= 1e-11 * np.abs(ref).max(), (q, err, np.abs(ref).max())
        single = be.ktk(K, w=W[q, :n].contiguous())
        assert float((out[q, :M] - single).abs().max()) <= 1e-12 * float(single.abs().max()), q
    assert torch.equal(run()[:, :M], out[:, :M])


def test_limits_of_the_backward_entry(be):
    from odx import hip
    lib = be.lib
    assert lib.odx_knm_bwdn_q_workspace_bytes(1000, 20440, hip.KNM_U24, 8) > 0
    assert lib.odx_knm_bwdn_q_workspace_bytes(1000, 20440, hip.KNM_BF16, 1) > 0
    assert lib.odx_knm_bwdn_q_workspace_bytes(1000, 20441, hip.KNM_U24, 8) < 0
    assert lib.odx_knm_bwdn_q_workspace_bytes(1000, 2000, hip.KNM_U24, 9) < 0
    assert lib.odx_knm_bwdn_q_workspace_bytes(1000, 2000, hip.KNM_U24, 0) < 0
    assert lib.odx_knm_bwdn_q_workspace_bytes(1000, 2000, hip.KNM_F32, 4) < 0
    out = torch.zeros((9, 2000), dtype=torch.float64, device="cuda")
    rc = lib.odx_knm_bwdn_q(None, 2000, None, 2000, hip.KNM_U24, 10, 2000, 9, ctypes.c_void_p(out.data_ptr()), 2000,
                            ctypes.c_void_p(out.data_ptr()), 2000, None, 0, None)
    assert rc != 0 and b"odx_knm_bwdn_q" in lib.odx_last_error_string()


def _trmvn_case(be, rng, M, nv, uplo, pad):
    from odx import hip
    ld = (M + 1) // 2 * 2 + pad
    ldx, ldz, ldy = (M + 1) // 2 * 2 + 2 * pad, M + 3 * pad, M + 1 + pad        # strided rows; only ldx needs to be even
    Th = rng.standard_normal((M, ld)) / np.sqrt(M)
    tri = np.triu(Th[:, :M]) if uplo else np.tril(Th[:, :M])
    Tg = Th.copy()
    Tg[:, :M][tri == 0] = np.nan                            # the other triangle (and the pad columns) must never be read
    Tg[:, M:] = np.nan
    Xh = rng.standard_normal((nv, ldx)) * np.logspace(0, -2, nv)[:, None]
    Zh = rng.standard_normal((nv, ldz))
    Tri, X = torch.from_numpy(Tg).cuda(), torch.from_numpy(Xh).cuda()
    alpha, beta = 0.37, -1.25
    for b, alias in ((0.0, False), (beta, False), (beta, True)):
        Z = torch.from_numpy(Zh).cuda()
        Y = Z if alias else torch.full((nv, ldy), float("nan"), dtype=torch.float64, device="cuda")
        ly = ldz if alias else ldy
        hip.check(be.lib.odx_trmvn_f64(ctypes.c_void_p(Tri.data_ptr()), ld, M, uplo, nv, ctypes.c_void_p(X.data_ptr()), ldx, alpha, b,
                                       None if b == 0.0 else ctypes.c_void_p(Z.data_ptr()), ldz, ctypes.c_void_p(Y.data_ptr()), ly, None),
                  "odx_trmvn_f64")
        torch.cuda.synchronize()
        got = Y.cpu().numpy()
        if alias:
            assert np.array_equal(got[:, M:], Zh[:, M:])    # guard cells
        else:
            assert np.isnan(got[:, M:]).all()
        for q in range(nv):
            ref = alpha * (tri @ Xh[q, :M]) + b * Zh[q, :M]
            # the forward bound of an M-term f64 sum in any order
            bound = 2 * M * 2.0 ** -53 * (abs(alpha) * (np.abs(tri) @ np.abs(Xh[q, :M])) + abs(b) * np.abs(Zh[q, :M]))
            err = np.abs(got[q, :M] - ref)
            assert (err <= bound).all(), (M, nv, uplo, q, b, alias, float((err / np.maximum(bound, 1e-300)).max()))
            y1 = torch.empty(M, dtype=torch.float64, device="cuda")
            z1 = torch.from_numpy(Zh[q]).cuda()
            hip.check(be.lib.odx_trmv_f64(ctypes.c_void_p(Tri.data_ptr()), ld, M, uplo, ctypes.c_void_p(X[q].data_ptr()), alpha, b,
                                          None if b == 0.0 else ctypes.c_void_p(z1.data_ptr()), ctypes.c_void_p(y1.data_ptr()), None),
                      "odx_trmv_f64")
            torch.cuda.synchronize()
            err1 = np.abs(got[q, :M] - y1.cpu().numpy())
            assert (err1 <= bound).all(), (M, nv, uplo, q, b, alias)


@pytest.mark.parametrize("uplo", [0, 1])
@pytest.mark.parametrize("M", [1, 2, 3, 129, 1000, 2001, 4100, 10000])
def test_trmvn(be, M, uplo):
    """Y[q] = alpha Tri X[q] + beta Z[q]: per entry within 2 M 2^-53 (|alpha| sum_j |t_ij| |x_qj| + |beta| |z_qi|) of numpy f64 and of
    odx_trmv_f64 on each vector; ld > M, strided rows, beta with Z, Y aliasing Z, the other triangle NaN, guard cells."""
    rng = np.random.default_rng(1000 * M + uplo)
    for nv in range(1, 9):
        _trmvn_case(be, rng, M, nv, uplo, pad=2 if M > 3 else 0)


def _rows_against_single(be, K, T, rng):
    M, n = K.M, K.n
    ldw = (n + 1) // 2 * 2
    W = torch.zeros((T, ldw), dtype=torch.float64, device="cuda")
    W[:, :n] = torch.from_numpy(rng.standard_normal((T, n)) * 1e-2).cuda()
    out = be.ktwn(K, W)
    assert tuple(out.shape) == (T, (M + 1) // 2 * 2)
    for t in range(T):
        single = be.ktk(K, w=W[t, :n].contiguous())
        assert float((out[t, :M] - single).abs().max()) <= 1e-12 * float(single.abs().max()), t


def test_ktwn_groups_f32_blocks_and_streamed_shards(be, storage):
    from odx.backend import Knm
    from tests.synth import blob_problem, centres
    rng = np.random.default_rng(13)
    K, _ = _compact_block(rng, 1200, 2000, "u24")
    _rows_against_single(be, K, 11, rng)                                # groups of 8 + 3
    K, _ = _compact_block(rng, 1201, 2000, "u24")
    _rows_against_single(be, K, 9, rng)                                 # 8 + a single ktk
    K10, _ = _compact_block(rng, 500, 10000, "u24")
    _rows_against_single(be, K10, 11, rng)
    Kf = Knm()
    f = rng.random((900, 300)).astype(np.float32)
    Kf.K, Kf.n, Kf.M, Kf.ld = torch.from_numpy(f).cuda(), 900, 300, 300
    _rows_against_single(be, Kf, 11, rng)
    X, y, r2 = blob_problem(3000, 64, seed=3)
    idx = centres(y, 300, r2)
    be.gauss, be.knm_storage = "h2", "stream"
    F = be.features(torch.from_numpy(X))
    S, _ = be.knm_rhs(F, be.rows(F, idx), 10.0, be.vec(y) / 3000)
    assert S.fmt == "stream"
    _rows_against_single(be, S, 11, rng)


def test_trmvn_groups(be):
    rng = np.random.default_rng(17)
    Z = (rng.standard_normal((301, 32)) * (20.0 / np.sqrt(32))).astype(np.float32)
    P = be.precond(be.features(torch.from_numpy(Z)), 15.0, 1e-4, 1e-5)
    X = torch.from_numpy(rng.standard_normal((11, P.ld))).cuda()
    Zm = torch.from_numpy(rng.standard_normal((11, P.ld))).cuda()
    for name in ("LTi", "LTit", "LAi", "LAit"):
        out = be.trmvn(P, name, X, alpha=0.5, beta=2.0, Z=Zm)
        for t in range(11):
            one = be.trmv(P, name, X[t], alpha=0.5, beta=2.0, z=Zm[t])
            assert float((out[t, :P.M] - one).abs().max()) <= 1e-13 * max(1.0, float(one.abs().max())), (name, t)


# the rows of PATH_GRID in tests/test_gpu_falkon_path.py (the reference's shipped (sigma, M, D) with the first penalty shipped
# at each): detector (D = 2048), on-line RPN (D = 1024), on-line segmentation (D = 256)
MULTI_GRID = [
    (15.0, 2000, 2048, 1e-3),
    (15.0, 1000, 2048, 1e-5),
    (50.0, 1000, 1024, 1e-5),
    (10.0, 500, 256, 1e-6),
    (25.0, 500, 256, 1e-7),
    (5.0, 2000, 2048, 1e-4),
]


def label_columns(X, y, T, seed):
    """blob_problem's own labels as column 0, then T - 1 further +-1 labellings of the same rows: the side of a random
    hyperplane through the (centred) rows — smooth in x at the kernel's scale, like a class against the rest, so that a
    fit of the column alone is as well conditioned as the fit of column 0."""
    g = np.random.default_rng(seed)
    cols = [y.astype(np.float64)]
    for _ in range(1, T):
        w = g.standard_normal(X.shape[1])
        s = X.astype(np.float64) @ w
        cols.append(np.where(s > np.quantile(s, 0.7), 1.0, -1.0))
    return np.ascontiguousarray(np.stack(cols, 1))


def _grid_rows(sigma, M, D, n=8000):
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(n, D, seed=int(sigma * 1000) + M + D)
    return X, y, centres(y, M, rng)


def _check_multi(be, X, Y, idx, sigma, lam):
    import odx
    from oracle import falkon_ref as fr
    T = Y.shape[1]
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    refs, prefs = [], []
    for t in range(T):
        ref, Z = fr.falkon_fit(X.astype(np.float64), Y[:, t], idx, sigma, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        refs.append(ref[:, 0])
        prefs.append(fr.falkon_predict(X.astype(np.float64), Z, ref, sigma)[:, 0])

    def bars(alpha, scores, t, what):
        rel = np.linalg.norm(alpha - refs[t]) / np.linalg.norm(refs[t])
        serr = np.abs(scores - prefs[t]).max()
        print("%s sigma=%g M=%d lam=%g column %d: alpha rel err %.2e, score err %.2e (max |ref| %.2f)"
              % (what, sigma, Zf.n, lam, t, rel, serr, np.abs(prefs[t]).max()))
        return rel < 1e-4 and serr < 1e-4 * max(1.0, float(np.abs(prefs[t]).max())), (what, t, rel, serr)
    # the fixture: every column fitted alone by odx.falkon_fit meets the bars (else the labelling is a bad fixture)
    for t in range(T):
        a1 = odx.falkon_fit(be, F, be.vec(Y[:, t]), Zf, sigma, lam, 20)
        ok, info = bars(a1.cpu().numpy(), be.mmv(F, Zf, sigma, a1).cpu().numpy().reshape(-1), t, "single")
        assert ok, ("bad fixture: the single fit of this column misses the bars", info)
    blocks = []
    alphas = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, sigma, lam, 20, knm_blocks=blocks)
    assert tuple(alphas.shape) == (T, Zf.n) and len(blocks) == 1
    scores = be.mmv(F, Zf, sigma, alphas.t().contiguous()).cpu().numpy()
    for t in range(T):
        ok, info = bars(alphas[t].cpu().numpy(), scores[:, t], t, "multi")
        assert ok, info
    return blocks[0]


@pytest.mark.parametrize("knm", ["f32", "u24"])
@pytest.mark.parametrize("sigma,M,D,lam", MULTI_GRID)
def test_multi_on_the_reference_grid(be, storage, knm, sigma, M, D, lam):
    """T = 5 label columns: alpha < 1e-4 relative and scores < 1e-4 max(1, max|ref|) per column against the f64 oracle (the
    project's bars), after the same bars were met by odx.falkon_fit on every column alone."""
    be.gauss, be.knm_storage = "h2", knm
    be.pin_gauss_tile(256 if knm == "u24" else 0)
    X, y, idx = _grid_rows(sigma, M, D)
    K = _check_multi(be, X, label_columns(X, y, 5, seed=M + D), idx, sigma, lam)
    assert K.fmt == knm


def test_multi_on_an_hbm_bound_block(be, storage):
    """2e5 x 2000, D = 256, 24-bit storage, T = 8: the passes are the 8-wide kernel, the right-hand sides odx_knm_bwdn_q."""
    from tests.synth import blob_problem, centres
    be.gauss, be.knm_storage = "h2", "u24"
    X, y, rng = blob_problem(200000, 256, seed=77)
    idx = centres(y, 2000, rng)
    K = _check_multi(be, X, label_columns(X, y, 8, seed=5), idx, 10.0, 1e-5)
    assert K.fmt == "u24" and be.ktkn_width(K) == 8


def test_multi_takes_the_four_wide_pass_and_a_pair(be, storage):
    """M = 4500, T = 6: ktkn serves the six directions as 4 + a two-vector pass."""
    from tests.synth import blob_problem, centres
    be.gauss, be.knm_storage = "h2", "u24"
    X, y, rng = blob_problem(20000, 64, seed=78)
    idx = centres(y, 4500, rng)
    K = _check_multi(be, X, label_columns(X, y, 6, seed=6), idx, 8.0, 1e-4)
    assert K.fmt == "u24" and be.ktkn_width(K) == 4 and be.can_ktk2(K)


def test_estimator_multi_on_the_gpu(be):
    import odx
    from odx.wrappers import CenterSelector
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(3000, 64, seed=9)
    idx = centres(y, 300, rng)
    Y = label_columns(X, y, 4, seed=10)
    Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    mk = lambda: odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=8.0), penalty=1e-4, M=len(idx), maxiter=20,      # noqa: E731
                                  center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
    m = mk().fit_multi(Xt, Yt)
    assert tuple(m.alpha_.shape) == (300, 4)
    p = m.predict(Xt[:100])
    assert tuple(p.shape) == (100, 4)
    for t in range(4):
        one = mk().fit(Xt, Yt[:, t])
        assert float((m.alpha_[:, t] - one.alpha_[:, 0]).norm() / one.alpha_.norm()) < 1e-6
        assert float((p[:, t] - one.predict(Xt[:100])[:, 0]).abs().max()) < 1e-5
    with pytest.raises(ValueError, match="one right-hand side"):
        mk().fit_path(Xt, Yt, [1e-4, 1e-5])
