"""K-fold cross-validation of a lambda path on the MI355X: the row-weighted NV-vector pass over compact K_nM blocks
(odx_knm_fwd_bwdn_q_rw), HipBackend.ktkn_rows / ktkn_rows_reads, odx.falkon_fit_cv against the f64 oracle's fits on each
fold's training rows, and the estimator's fit_cv."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_falkon_multi import MULTI_GRID, _compact_block, _grid_rows

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


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _weights(rng, n, ldd):
    """G = 3 rows of n row weights, NaN behind them: two 0/1 masks scaled by n / n_f (the folds of i % 2; one row survives
    where the mask would be empty) and one row of general positive weights."""
    D = np.full((3, ldd), np.nan)
    fold = np.arange(n) % 2
    for f in range(2):
        m = (fold != f).astype(np.float64)
        if m.sum() == 0:
            m[0] = 1.0
        D[f, :n] = m * (n / m.sum())
    D[2, :n] = rng.random(n) * 3.0 + 1e-3
    return D


# (n, M, nv): every instantiation ((256, 1), (512, 1), (512, 2), (512, 3) x widths 8 and 4), n below one row block and not a
# multiple of it, an odd M, both LDS limits (2524 at 8 vectors, 5084 at 4), every nv that runs padded (1, 2, 3, 5, 7)
RW_SHAPES = [(1, 100, 4), (7, 100, 2), (3, 1023, 8), (777, 129, 3), (1501, 1000, 8), (2001, 2000, 8), (999, 2045, 5), (530, 2524, 7),
             (1003, 2000, 1), (301, 4096, 4), (515, 5084, 3), (203, 5084, 1)]


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,M,nv", RW_SHAPES)
def test_row_weighted_nv_pass(be, fmt, n, M, nv):
    """out[q] = K' (D[wrow[q]] o (K V[q])) against dense f64 numpy at 1e-11 max|ref|; T_out[q][:n] = K V[q] within the forward
    bound of an M-term f64 sum, 2 M 2^-53 (|K| |v|), per entry; guard cells and weights past n untouched; bit-repeatable;
    `out` the same bits with and without T_out; every wrow = -1 without T_out bit for bit odx_knm_fwd_bwdn_q (nv >= 3)."""
    from odx import hip
    rng = np.random.default_rng(n * 37 + M + nv)
    K, vals = _compact_block(rng, n, M, fmt)
    ldv, ldo, ldd, ldt = (M + 1) // 2 * 2 + 6, (M + 1) // 2 * 2 + 4, (n + 1) // 2 * 2 + 4, n + 3
    Vh = np.zeros((nv, ldv))
    Vh[:, :M] = rng.standard_normal((nv, M)) * np.logspace(0, -3, nv)[:, None]
    Dh = _weights(rng, n, ldd)
    wrow = [(0, -1, 2, 1)[q % 4] for q in range(nv)]
    V, D = torch.from_numpy(Vh).cuda(), torch.from_numpy(Dh).cuda()
    code = hip.KNM_CODE[fmt]
    nbytes = be.lib.odx_knm_fwd_bwdn_q_rw_workspace_bytes(n, M, code, nv)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lo = _vp(K.lo) if fmt == "u24" else None

    def run(rows, with_t):
        out = torch.full((nv, ldo), float("nan"), dtype=torch.float64, device="cuda")
        T = torch.full((nv, ldt), float("nan"), dtype=torch.float64, device="cuda") if with_t else None
        hip.check(be.lib.odx_knm_fwd_bwdn_q_rw(_vp(K.K), K.ld, lo, K.ld, code, n, M, nv, _vp(V), ldv, _vp(D), ldd,
                                               (ctypes.c_int32 * nv)(*rows), _vp(out), ldo, _vp(T), ldt, _vp(ws), nbytes, None),
                  "odx_knm_fwd_bwdn_q_rw")
        torch.cuda.synchronize()
        return out, T
    out, T = run(wrow, True)
    assert torch.isnan(out[:, M:]).all() and torch.isnan(T[:, n:]).all()
    absK = np.abs(vals)
    for q in range(nv):
        t = vals @ Vh[q, :M]
        ref = vals.T @ (t * Dh[wrow[q], :n] if wrow[q] >= 0 else t)
        err = np.abs(out[q, :M].cpu().numpy() - ref).max()
        terr = np.abs(T[q, :n].cpu().numpy() - t)
        tbound = 2 * M * 2.0 ** -53 * (absK @ np.abs(Vh[q, :M]))
        print("n=%d M=%d nv=%d %s q=%d wrow=%d: out err %.2e of max|ref| %.2e, T err / bound %.2e"
              % (n, M, nv, fmt, q, wrow[q], err, np.abs(ref).max(), float((terr / np.maximum(tbound, 1e-300)).max())))
        assert err <= 1e-11 * np.abs(ref).max(), (q, err, np.abs(ref).max())
        assert (terr <= tbound).all(), (q, float((terr / np.maximum(tbound, 1e-300)).max()))
    again, T2 = run(wrow, True)
    assert torch.equal(again[:, :M], out[:, :M]) and torch.equal(T2[:, :n], T[:, :n])
    assert torch.equal(run(wrow, False)[0][:, :M], out[:, :M])
    if nv >= 3:
        plain = torch.full((nv, ldo), float("nan"), dtype=torch.float64, device="cuda")
        hip.check(be.lib.odx_knm_fwd_bwdn_q(_vp(K.K), K.ld, lo, K.ld, code, n, M, nv, _vp(V), ldv, _vp(plain), ldo, _vp(ws), nbytes, None),
                  "odx_knm_fwd_bwdn_q")
        torch.cuda.synchronize()
        assert torch.equal(run([-1] * nv, False)[0][:, :M], plain[:, :M])


def test_limits_of_the_row_weighted_entry(be):
    from odx import hip
    lib = be.lib
    twin = lib.odx_knm_fwd_bwdn_q_rw_workspace_bytes
    assert twin(1000, 2524, hip.KNM_U24, 8) > 0 and twin(1000, 5084, hip.KNM_BF16, 4) > 0 and twin(1000, 5084, hip.KNM_U24, 1) > 0
    bad = [(2525, hip.KNM_U24, 8), (2525, hip.KNM_U24, 5), (5085, hip.KNM_U24, 4), (5085, hip.KNM_BF16, 1), (2000, hip.KNM_F32, 4),
           (2000, hip.KNM_U24, 0), (2000, hip.KNM_U24, 9)]
    rng = np.random.default_rng(3)
    for M, fmt, nv in bad:
        assert twin(1000, M, fmt, nv) < 0, (M, fmt, nv)
        K, _ = _compact_block(rng, 10, M, "bf16" if fmt == hip.KNM_BF16 else "u24")
        ld = (M + 1) // 2 * 2
        buf = torch.zeros((9, ld), dtype=torch.float64, device="cuda")
        rc = lib.odx_knm_fwd_bwdn_q_rw(_vp(K.K), K.ld, _vp(K.lo) if K.fmt == "u24" else None, K.ld, fmt, 10, M, nv, _vp(buf), ld, None, 0,
                                       (ctypes.c_int32 * 9)(*([-1] * 9)), _vp(buf), ld, None, 0, _vp(buf), buf.numel() * 8, None)
        assert rc != 0 and b"odx_knm_fwd_bwdn_q_rw" in lib.odx_last_error_string(), (M, fmt, nv)


def _rows_against_dense(be, K, vals, L, rng, monkeypatch):
    """ktkn_rows over L vectors against the dense f64 product at the bound of test_row_weighted_nv_pass; the reads it made
    (entries that read the block, as be._call issues them) against ktkn_rows_reads."""
    M, n = K.M, K.n
    ldn = (n + 1) // 2 * 2
    Vh = rng.standard_normal((L, (M + 1) // 2 * 2)) * 1e-2
    Dh = _weights(rng, n, ldn)
    wrow = [(0, -1, 2, 1)[q % 4] for q in range(L)]
    V, D = torch.from_numpy(Vh).cuda(), torch.from_numpy(Dh).cuda()
    reads = []
    call = be._call
    monkeypatch.setattr(be, "_call", lambda entry, *a: (reads.append(entry) if entry.startswith("odx_knm_") else None, call(entry, *a))[1])
    T = torch.full((L, ldn), float("nan"), dtype=torch.float64, device="cuda")
    out = be.ktkn_rows(K, V, D, wrow, t_out=T)
    monkeypatch.undo()
    assert len(reads) == be.ktkn_rows_reads(K, L), (reads, be.ktkn_rows_reads(K, L))
    absK = np.abs(vals)
    for q in range(L):
        t = vals @ Vh[q, :M]
        ref = vals.T @ (t * Dh[wrow[q], :n] if wrow[q] >= 0 else t)
        err = np.abs(out[q, :M].cpu().numpy() - ref).max()
        assert err <= 1e-11 * np.abs(ref).max(), (q, err, np.abs(ref).max())
        assert (np.abs(T[q, :n].cpu().numpy() - t) <= 2 * M * 2.0 ** -53 * (absK @ np.abs(Vh[q, :M]))).all(), q
    assert torch.equal(be.ktkn_rows(K, V, D, wrow)[:, :M], out[:, :M])          # the same bits without t_out
    return reads


def test_ktkn_rows_routes(be, storage, monkeypatch):
    from odx.backend import Knm
    from tests.synth import blob_problem, centres
    rng = np.random.default_rng(19)
    K, vals = _compact_block(rng, 1200, 2000, "u24")
    reads = _rows_against_dense(be, K, vals, 11, rng, monkeypatch)          # groups of 8 + 3, one read each
    assert reads == ["odx_knm_fwd_bwdn_q_rw"] * 2 and be.ktkn_rows_reads(K, 11) == 2 and be.ktkn_rows_reads(K, 9) == 2
    K10, vals = _compact_block(rng, 500, 10000, "u24")
    reads = _rows_against_dense(be, K10, vals, 11, rng, monkeypatch)        # two reads per group of up to 8
    assert reads == ["odx_knm_fwdn_q", "odx_knm_bwdn_q"] * 2
    assert be.wide_pass_min is None and be.ktkn_rows_reads(K10, 2) == 2     # (two reads whatever wide_pass_min says)
    Kf = Knm()
    f = rng.random((900, 300)).astype(np.float32)
    Kf.K, Kf.n, Kf.M, Kf.ld = torch.from_numpy(f).cuda(), 900, 300, 300
    reads = _rows_against_dense(be, Kf, f.astype(np.float64), 11, rng, monkeypatch)
    assert len(reads) == 22
    # refusals: a block with a column map, a streamed shard
    V = torch.zeros((2, 2000), dtype=torch.float64, device="cuda")
    D = torch.ones((1, 1200), dtype=torch.float64, device="cuda")
    K.cmap = object()
    with pytest.raises(ValueError, match="column map"):
        be.ktkn_rows(K, V, D, [0, -1])
    K.cmap = None
    with pytest.raises(ValueError, match="wrow"):
        be.ktkn_rows(K, V, D, [0, 1])
    X, y, r2 = blob_problem(3000, 64, seed=3)
    idx = centres(y, 300, r2)
    be.gauss, be.knm_storage = "h2", "stream"
    F = be.features(torch.from_numpy(X))
    S, _ = be.knm_rhs(F, be.rows(F, idx), 10.0, be.vec(y) / 3000)
    assert S.fmt == "stream"
    with pytest.raises(ValueError, match="streamed shard"):
        be.ktkn_rows(S, torch.zeros((2, 300), dtype=torch.float64, device="cuda"), torch.ones((1, 3000), dtype=torch.float64, device="cuda"), [0, -1])
    import odx
    with pytest.raises(ValueError, match="streamed shard"):
        odx.falkon_fit_cv(be, F, be.vec(y), be.rows(F, idx), 10.0, [1e-4], odx.cv_folds(3000, 3), 3)


_ORACLE = {}


def _oracle(key, X, y, idx, fold_of, folds, sigma, lams):
    """The f64 oracle of one problem, computed once and shared by its storage formats: per penalty the fit on each fold's
    training rows alone and its scores of the held-out rows, then the fit on all rows."""
    if key not in _ORACLE:
        from oracle import falkon_ref as fr
        X64, y64, Z = X.astype(np.float64), y.astype(np.float64), X[idx].astype(np.float64)
        out = []
        for lam in lams:
            alphas, held = [], np.zeros(len(X))
            for f in range(folds):
                tr, te = np.nonzero(fold_of != f)[0], np.nonzero(fold_of == f)[0]
                a = fr.falkon_fit_centers(X64[tr], y64[tr], Z, sigma, lam, len(tr), 20, np.float64, 1e-5, 1e-7)[0]
                held[te] = fr.falkon_predict(X64[te], Z, a, sigma)[:, 0]
                alphas.append(a[:, 0])
            alphas.append(fr.falkon_fit_centers(X64, y64, Z, sigma, lam, len(X), 20, np.float64, 1e-5, 1e-7)[0][:, 0])
            out.append((alphas, held))
        _ORACLE[key] = out
    return _ORACLE[key]


def _check_cv(be, key, X, y, idx, sigma, lams, folds=3):
    """The project's bars (alpha relative < 1e-4, scores < 1e-4 max(1, max|ref|)) for falkon_fit_cv, after odx.falkon_fit on
    each fold's training rows alone met them (else the fixture is bad)."""
    import odx
    fold_of = odx.cv_folds(len(X), folds, seed=1)
    fo = fold_of.numpy()
    ref = _oracle(key, X, y, idx, fo, folds, sigma, lams)
    Xt = torch.from_numpy(X)
    F = be.features(Xt)
    Zf = be.rows(F, idx)
    yv = be.vec(y)

    def rel(a, r):
        return float(np.linalg.norm(a - r) / np.linalg.norm(r))
    for l, lam in enumerate(lams):
        for f in range(folds):
            tr, te = np.nonzero(fo != f)[0], np.nonzero(fo == f)[0]
            Ftr = be.features(Xt[tr])
            a1 = odx.falkon_fit(be, Ftr, be.vec(y[tr]), Zf, sigma, lam, 20)
            s1 = be.mmv(be.features(Xt[te]), Zf, sigma, a1).cpu().numpy().reshape(-1)
            r1, e1 = rel(a1.cpu().numpy(), ref[l][0][f]), np.abs(s1 - ref[l][1][te]).max()
            print("single sigma=%g M=%d lam=%g fold %d: alpha rel err %.2e, score err %.2e" % (sigma, Zf.n, lam, f, r1, e1))
            assert r1 < 1e-4 and e1 < 1e-4 * max(1.0, float(np.abs(ref[l][1][te]).max())), \
                ("bad fixture: the single fit of this fold misses the bars", lam, f, r1, e1)
    blocks = []
    alphas, heldout = odx.falkon_fit_cv(be, F, yv, Zf, sigma, lams, fold_of, folds, 20, knm_blocks=blocks)
    assert tuple(alphas.shape) == (len(lams), folds + 1, Zf.n) and tuple(heldout.shape) == (len(lams), len(X)) and len(blocks) == 1
    bad = []
    for l, lam in enumerate(lams):
        for f in range(folds + 1):
            r = rel(alphas[l, f].cpu().numpy(), ref[l][0][f])
            print("cv sigma=%g M=%d lam=%g state %d: alpha rel err %.2e" % (sigma, Zf.n, lam, f, r))
            if not r < 1e-4:
                bad.append(("alpha", lam, f, r))
        e = np.abs(heldout[l].cpu().numpy() - ref[l][1]).max()
        print("cv sigma=%g M=%d lam=%g: held-out score err %.2e (max |ref| %.2f)" % (sigma, Zf.n, lam, e, np.abs(ref[l][1]).max()))
        if not e < 1e-4 * max(1.0, float(np.abs(ref[l][1]).max())):
            bad.append(("heldout", lam, e))
    assert not bad, bad
    return blocks[0]


CV_GRID = [MULTI_GRID[1], MULTI_GRID[3], MULTI_GRID[5]]
assert CV_GRID == [(15.0, 1000, 2048, 1e-5), (10.0, 500, 256, 1e-6), (5.0, 2000, 2048, 1e-4)]


@pytest.mark.parametrize("knm", ["f32", "u24"])
@pytest.mark.parametrize("sigma,M,D,lam", CV_GRID)
def test_cv_on_the_reference_grid(be, storage, knm, sigma, M, D, lam):
    """Three folds, two penalties (the row's own and ten times it): every fold alpha, the refit alpha and the held-out scores
    against the f64 oracle's fits on each fold's training rows."""
    be.gauss, be.knm_storage = "h2", knm
    be.pin_gauss_tile(256 if knm == "u24" else 0)
    X, y, idx = _grid_rows(sigma, M, D)
    K = _check_cv(be, (sigma, M, D), X, y, idx, sigma, [lam, 10 * lam])
    assert K.fmt == knm
    if knm == "u24":
        assert be.ktkn_rows_reads(K, 4) == 1


def test_cv_above_the_lds_limit(be, storage):
    """M = 5200: no one-read pass exists, the four states take the two-read route."""
    from tests.synth import blob_problem, centres
    be.gauss, be.knm_storage = "h2", "u24"
    X, y, rng = blob_problem(6000, 64, seed=79)
    idx = centres(y, 5200, rng)
    K = _check_cv(be, "wide", X, y, idx, 8.0, [1e-4])
    assert K.fmt == "u24" and be.ktkn_rows_reads(K, 4) == 2


def test_cv_on_a_bf16_block_scores_through_mmv(be, storage):
    import odx
    from tests.synth import blob_problem, centres
    be.gauss, be.knm_storage = "h2", "bf16"
    X, y, rng = blob_problem(3000, 64, seed=11)
    idx = centres(y, 300, rng)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    fold_of = odx.cv_folds(3000, 3, seed=2)
    blocks = []
    alphas, heldout = odx.falkon_fit_cv(be, F, be.vec(y), Zf, 8.0, [1e-4, 1e-3], fold_of, 3, 20, knm_blocks=blocks)
    assert blocks[0].fmt == "bf16" and not odx.solver.scores_from_cg(be, blocks[0])
    assert torch.isfinite(alphas).all()
    sc = be.mmv(F, Zf, 8.0, alphas[:, :3].reshape(6, 300).t().contiguous())
    fo = fold_of.cuda()
    for l in range(2):
        want = sc[:, 3 * l:3 * l + 3].gather(1, fo[:, None])[:, 0].double()
        assert torch.equal(heldout[l], want), l


def test_estimator_fit_cv_on_the_gpu(be):
    import odx
    from odx.wrappers import CenterSelector
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(3000, 64, seed=9)
    idx = centres(y, 300, rng)
    Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    mk = lambda: odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=8.0), penalty=1e-4, M=len(idx), maxiter=20,      # noqa: E731
                                  center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
    pens = [1e-4, 1e-3, 1e-2]
    res = mk().fit_cv(Xt, Yt, pens, folds=4)
    assert tuple(res.scores.shape) == (3000, 3) and res.scores.dtype == torch.float32 and res.scores.is_cuda
    assert tuple(res.fold_alphas.shape) == (3, 4, 300) and tuple(res.fold_of.shape) == (3000,)
    want = ((res.scores.double() - Yt.double()[:, None]) ** 2).mean(0)
    assert torch.isfinite(res.mse).all() and torch.allclose(res.mse, want, rtol=1e-12, atol=0.0)
    path = mk().fit_path(Xt, Yt, pens)
    assert len(res.estimators) == 3
    for est, ref in zip(res.estimators, path):
        assert float((est.alpha_ - ref.alpha_).norm() / ref.alpha_.norm()) < 1e-6
    p = odx.predict_path(res.estimators, Xt[:100])
    assert tuple(p.shape) == (100, 3)
    assert float((p - odx.predict_path(path, Xt[:100])).abs().max()) < 1e-5
