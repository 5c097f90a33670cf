"""Ridge leverage scores on the GPU: odx_knm_rowquad_f64 and odx_radial_kmm_f64 by ctypes against numpy, the backend's
chol_inverse, odx.leverage_scores against the f64 restatement (tests/leverage_ref.py) under bars derived from the build
kernels' own entry bars, and odx.LeverageSelector end to end."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import leverage_ref as lr  # noqa: E402
from tests.synth import blob_problem  # noqa: E402
from tests.test_gpu_kernels import ktol  # noqa: E402

U = 2.0 ** -53
ODX_ERR_INVALID = -1


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture(autouse=True)
def _options_back_to_what_they_were():
    import odx
    before = odx.options.as_dict()
    yield
    if odx.options.as_dict() != before:
        odx.options.set(**before)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


# ------------------------------------------------------------------ A. odx_knm_rowquad_f64
def _rowquad_inputs(n, M):
    rng = np.random.default_rng(1000 * n + M)
    ldk, ldl = (M + 3) // 4 * 4 + 4, M + 2
    K = np.full((n, ldk), np.nan, dtype=np.float32)
    K[:, :M] = rng.uniform(-1.0, 1.0, (n, M)).astype(np.float32)
    Li = np.full((M, ldl), np.nan, dtype=np.float64)
    Li[:, :M] = np.where(np.tri(M, dtype=bool), rng.standard_normal((M, M)), np.nan)
    return K, Li


# (n, M) past M = 257: 17 and 18 column tiles of 64, the last of one column (M = 1024 + 1 and 1024 + 65), the factor's clean
# loader form kt + BK <= j0 over up to 64 and 68 k-tiles of 16 with a ragged k-tile of one column behind them, two row blocks
# of K with 1 and 2 rows in the second
ROWQUAD_SHAPES = [(n, M) for M in (1, 7, 16, 17, 128, 129, 257) for n in (1, 127, 129, 300)] + [(129, 1025), (130, 1089)]


@pytest.mark.parametrize("n,M", ROWQUAD_SHAPES)
def test_rowquad_kernel(be, n, M):
    """q against an extended-precision evaluation under 4 (M + 2) u sum_j (sum_c |K_rc| |Li_jc|)^2; NaN in every cell the
    kernel must not use; nothing written past row n; the same bits twice and for a row sub-block.  (The bar holds no width:
    (M + 2) u bounds the M-term sum T_rj within (M + 2) u S_rj, its square within twice that of S_rj^2, and the sum of the M
    squares adds (M + 2) u of itself: 3 (M + 2) u to first order, 4 with the second-order terms while M u << 1.)  Past
    M = 257 the factor at a leading dimension of the other parity (16-byte loads for 8-byte ones) gives the same bits as well."""
    K, Li = _rowquad_inputs(n, M)
    Lt = np.tril(np.nan_to_num(Li[:, :M])).astype(np.longdouble)
    Kx = K[:, :M].astype(np.longdouble)
    T = Kx @ Lt.T
    ref = (T * T).sum(1)
    S = np.abs(Kx) @ np.abs(Lt).T
    bar = (4.0 * (M + 2) * U * (S * S).sum(1)).astype(np.float64)
    dK, dL = torch.from_numpy(K).cuda(), torch.from_numpy(Li).cuda()

    def call(k, rows, L=None):
        L = dL if L is None else L
        q = torch.full((rows + 3,), -7.0, dtype=torch.float64, device="cuda")
        rc = be.lib.odx_knm_rowquad_f64(_p(k), K.shape[1], rows, M, _p(L), L.shape[1], _p(q), be._stream())
        assert rc == 0, be.lib.odx_last_error_string()
        q = q.cpu().numpy()
        assert (q[rows:] == -7.0).all(), "written past row n"
        return q[:rows]

    q = call(dK, n)
    err = np.abs(q.astype(np.longdouble) - ref).astype(np.float64)
    print("n %d M %d: max err / bar %.3f" % (n, M, float((err / bar).max())))
    assert np.isfinite(q).all() and (err <= bar).all(), float((err / bar).max())
    assert np.array_equal(call(dK, n), q), "two calls differ"
    lo, hi = (37, 201) if n >= 201 else (min(37, n - 1), n)
    assert np.array_equal(call(dK[lo:], hi - lo), q[lo:hi]), "a row sub-block gives other bits"
    if M > 257:
        other = torch.full((M, Li.shape[1] + 1), float("nan"), dtype=torch.float64, device="cuda")
        other[:, :M] = dL[:, :M]                                   # a leading dimension of the other parity: the other loads
        assert np.array_equal(call(dK, n, other), q), "the factor at a leading dimension of the other parity gives other bits"


def test_rowquad_contract(be):
    """Empty shapes write nothing (zeros for M = 0); bad alignment / leading dimensions are ODX_ERR_INVALID; an aligned, even-ld
    factor (16-byte loads) gives the bits of the same factor at an odd ld (8-byte loads)."""
    n, M = 130, 70
    K, Li = _rowquad_inputs(n, M)
    dK, dL = torch.from_numpy(K).cuda(), torch.from_numpy(Li).cuda()
    ldk, ldl = K.shape[1], Li.shape[1]
    fn, s = be.lib.odx_knm_rowquad_f64, be._stream()
    q = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    assert fn(_p(dK), ldk, 0, M, _p(dL), ldl, _p(q), s) == 0 and fn(_p(dK), ldk, -3, M, _p(dL), ldl, _p(q), s) == 0
    assert fn(_p(dK), ldk, n, -1, _p(dL), ldl, _p(q), s) == 0 and bool((q == -7.0).all())
    assert fn(_p(dK), ldk, 5, 0, None, 0, _p(q), s) == 0
    assert bool((q[:5] == 0.0).all()) and bool((q[5:] == -7.0).all())
    flat = dK.view(-1)
    assert fn(_p(flat[1:]), ldk, n - 1, M, _p(dL), ldl, _p(q), s) == ODX_ERR_INVALID          # K off a 16-byte boundary
    assert fn(_p(dK), ldk - 2, n, M, _p(dL), ldl, _p(q), s) == ODX_ERR_INVALID                # ldk % 4 != 0
    assert fn(_p(dK), 68, n, M, _p(dL), ldl, _p(q), s) == ODX_ERR_INVALID                     # ldk < M
    assert fn(_p(dK), ldk, n, M, _p(dL), M - 1, _p(q), s) == ODX_ERR_INVALID                  # ldl < M
    assert bool((q[5:] == -7.0).all())
    assert fn(_p(dK), ldk, n, M, _p(dL), ldl, _p(q), s) == 0                                  # ldl = 72: even, aligned
    odd = torch.full((M, M + 3), float("nan"), dtype=torch.float64, device="cuda")
    odd[:, :M] = dL[:, :M]
    q2 = torch.empty_like(q)
    assert fn(_p(dK), ldk, n, M, _p(odd), M + 3, _p(q2), s) == 0
    assert torch.equal(q, q2)


# ------------------------------------------------------------------ B. odx_radial_kmm_f64
def _direct(Z, sigma, kind):
    """The f64 kernel matrix from the differences themselves, row by row."""
    M = len(Z)
    d2 = np.stack([((Z[i] - Z) ** 2).sum(1) for i in range(M)])
    if kind == 0:
        return np.exp(-d2 / (2.0 * sigma * sigma))
    u = np.sqrt(2.0 * (1.5 if kind == 1 else 2.5) * d2) / sigma
    return ((1 + u) if kind == 1 else (1 + u + u * u / 3.0)) * np.exp(-u)


# (kind, M, D); M = 1025: five column blocks of 256 in kmm_epilogue_kernel (the last of one column), 9 row blocks of 128 in the
# Gram GEMM's lower tiles
KMM_SHAPES = [(kind, M, D) for D in (36, 1024) for M in (7, 130, 257) for kind in (0, 1, 2)] + [(kind, 1025, 36) for kind in (0, 1, 2)]


@pytest.mark.parametrize("kind,M,D", KMM_SHAPES)
def test_radial_kmm(be, kind, M, D):
    """Per entry 8 D u (|z_i|^2 + |z_j|^2) s, s the kernel's largest slope in d^2 (1 / (2 sigma^2), x 3 and x 5/3 for the Matern
    kinds); the diagonal addition is one rounding."""
    sigma = 9.0
    rng = np.random.default_rng(100 * M + D + kind)
    Z = rng.standard_normal((M, D)) * (20.0 / np.sqrt(D))
    Z[M // 2:] = Z[: M - M // 2] + 0.01 * rng.standard_normal((M - M // 2, D))         # near-duplicate centres
    ldz, ldk = (D + 1) // 2 * 2 + 2, M + 1
    Zd = torch.zeros((M, ldz), dtype=torch.float64, device="cuda")
    Zd[:, :D] = torch.from_numpy(Z)
    ref = _direct(Z, sigma, kind)
    sq = (Z * Z).sum(1)
    slope = {0: 1.0, 1: 3.0, 2: 5.0 / 3.0}[kind] / (2.0 * sigma * sigma)
    bar = 8.0 * D * U * (sq[:, None] + sq[None, :]) * slope
    low = np.tri(M, dtype=bool)
    diag = rng.uniform(0.5, 2.0, M)
    dd = torch.from_numpy(diag).cuda()

    def run(d, scale):
        A = torch.full((M, ldk), float("nan"), dtype=torch.float64, device="cuda")
        zsq = torch.empty(M, dtype=torch.float64, device="cuda")
        rc = be.lib.odx_radial_kmm_f64(_p(Zd), ldz, M, D, sigma, kind, _p(d), scale, _p(A), ldk, _p(zsq), be._stream())
        assert rc == 0, be.lib.odx_last_error_string()
        np.testing.assert_allclose(zsq.cpu().numpy(), sq, rtol=1e-13)
        return A.cpu().numpy()[:, :M]

    bare = run(None, 0.0)
    err = np.abs(bare - ref)
    print("kind %d M %d D %d: max err / bar %.3f" % (kind, M, D, float((err / bar)[low].max())))
    assert np.isfinite(bare[low]).all() and (err[low] <= bar[low]).all(), float((err / bar)[low].max())
    off = low & ~np.eye(M, dtype=bool)
    for d, scale in ((dd, 1e-3), (None, 0.37)):
        got = run(d, scale)
        assert np.array_equal(got[off], bare[off])
        want = np.diag(bare).astype(np.longdouble) + np.longdouble(scale) * (diag.astype(np.longdouble) if d is not None else 1)
        assert (np.abs(np.diag(got).astype(np.longdouble) - want) <= np.spacing(np.diag(got))).all()
    A = torch.empty((M, ldk), dtype=torch.float64, device="cuda")
    zsq = torch.empty(M, dtype=torch.float64, device="cuda")
    assert be.lib.odx_radial_kmm_f64(_p(Zd), ldz, M, D, sigma, 3, None, 0.0, _p(A), ldk, _p(zsq), be._stream()) == ODX_ERR_INVALID
    assert be.lib.odx_radial_kmm_f64(_p(Zd), ldz - 1, M, D, sigma, kind, None, 0.0, _p(A), ldk, _p(zsq), be._stream()) == ODX_ERR_INVALID


# ------------------------------------------------------------------ C. chol_inverse
@pytest.mark.parametrize("M", [7, 130, 257, 1025])
def test_chol_inverse(be, M):
    """Li against numpy's inverse of the f64 Cholesky factor of the same matrix, to 1e-7 max(1, |Li|_max) (the bar
    test_gpu_matern.py::test_preconditioner holds the same chain to); A itself is left alone; a negative pivot raises."""
    import odx
    D, sigma, lam = 36, 9.0, 1e-4
    rng = np.random.default_rng(M)
    Z = (rng.standard_normal((M, D)) * (20.0 / np.sqrt(D))).astype(np.float32)
    Z[M // 2:] = Z[: M - M // 2] + 0.01 * rng.standard_normal((M - M // 2, D)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, M) * M
    Zf = be.features(torch.from_numpy(Z))
    A = be.kmm_f64(Zf, sigma, diag=torch.from_numpy(w), diag_scale=lam)
    a = np.tril(A.cpu().numpy()[:, :M])                   # (the lower triangle is the matrix)
    np.testing.assert_allclose(a, np.tril(lr.dictionary_matrix(Z, sigma, lam, w)), rtol=0, atol=1e-11)
    Li, info = be.chol_inverse(A)
    assert int(info.item()) == 0 and np.array_equal(np.tril(A.cpu().numpy()[:, :M]), a)
    want = np.linalg.inv(np.linalg.cholesky(a + np.tril(a, -1).T))
    got = Li.cpu().numpy()[:, :M]
    err = np.abs(got - want).max()
    print("M %d: err %.2e bound %.2e" % (M, err, 1e-7 * max(1.0, np.abs(want).max())))
    assert err <= 1e-7 * max(1.0, np.abs(want).max()) and (np.triu(got, 1) == 0).all()
    bad = A.clone()
    bad[M // 2, M // 2] = -1.0
    with pytest.raises(odx.hip.OdxError, match="non-positive pivot"):
        be.chol_inverse(bad)


def test_row_quad_refuses_other_formats(be):
    from odx.backend import Knm
    K = Knm()
    K.fmt, K.n, K.M = "u24", 4, 4
    with pytest.raises(ValueError, match="u24"):
        be.row_quad(K, torch.eye(4, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------ D. leverage_scores
# "d": one dictionary of 1100 centres (18 column tiles in the row quadratic form, 9 blocks of 128 in the dictionary's matrix and
# its inverse factor) against 1300 rows, 11 row blocks of K
CASES = {"a": (300, 130, 70, 10.0, 1e-3), "b": (513, 257, 70, 5.0, 1e-3), "c": (333, 130, 1024, 15.0, 1e-4),
         "d": (1300, 1100, 36, 5.0, 1e-3)}
_cases = {}


def _case(name, nu=None):
    """Rows, centres (the first five are copies of rows), weights and the f64 reference of a case: made once, never changed."""
    import odx
    key = (name, nu)
    if key not in _cases:
        n, M, D, sigma, lam = CASES[name]
        X, _, rng = blob_problem(n + M, D, seed=31 + n + M + D)
        Z = X[n:].copy()
        Z[:5] = X[:5]
        X = X[:n].copy()
        w = rng.uniform(0.5, 2.0, M) * M
        kernel = sigma if nu is None else odx.MaternKernel(sigma, nu)
        Kxz = lr.kernel_matrix(X, Z, kernel)
        Li = lr.inverse_factor(lr.dictionary_matrix(Z, kernel, lam, w))
        G = Kxz @ Li.T @ Li                                   # g_r = A^-1 k_r, rows
        q = lr.row_quad(Kxz, Li)
        scale = {None: 1.0, 1.5: 3.0, 2.5: 5.0 / 3.0}[nu]
        e = np.where(Kxz <= 0.99, ktol(sigma), max(ktol(sigma), 8e-4 / sigma ** 2)) * scale
        bar = 2.0 * (e * np.abs(G)).sum(1) / (lam * n)
        for a in (X, Z, w, q, bar):
            a.setflags(write=False)
        _cases[key] = (X, Z, w, kernel, lam, (1.0 - q) / (lam * n), bar)
    return _cases[key]


def _check_scores(be, name, nu, tile):
    import odx
    X, Z, w, kernel, lam, ref, bar = _case(name, nu)
    be.pin_gauss_tile(tile)
    got = odx.leverage_scores(torch.from_numpy(X.copy()), torch.from_numpy(Z.copy()), kernel, lam, weights=w.copy())
    assert got.dtype == torch.float64 and got.device.type == "cuda" and got.shape == (len(X),)
    err = np.abs(got.cpu().numpy() - ref)
    print("case %s nu %s tile %d: max err %.2e, max err / bar %.3f, bar %.1e .. %.1e"
          % (name, nu, tile, err.max(), float((err / bar).max()), bar.min(), bar.max()))
    assert (err <= bar).all(), float((err / bar).max())
    chunked = odx.leverage_scores(torch.from_numpy(X.copy()), torch.from_numpy(Z.copy()), kernel, lam, weights=w.copy(), chunk_rows=100)
    assert torch.equal(chunked, got), "chunk_rows=100 gives other bits"


@pytest.mark.parametrize("tile", [0, 128, 256])
@pytest.mark.parametrize("name", sorted(CASES))
def test_leverage_scores(be, name, tile):
    """|dq_r| <= 2 sum_c e_rc |g_rc| with g_r = A^-1 k_r and e the build's entry bar (test_gpu_kernels.ktol; 8e-4 / sigma^2 where
    the entry is above 0.99); the score bar is that over lam n.  Default route and both pinned tile cores; chunked = unchunked."""
    _check_scores(be, name, None, tile)


@pytest.mark.parametrize("tile", [0, 128, 256])
@pytest.mark.parametrize("nu", [1.5, 2.5])
def test_leverage_scores_matern(be, nu, tile):
    _check_scores(be, "b", nu, tile)


def test_leverage_scores_default_weights_and_q(be):
    import odx
    X, Z, _, kernel, lam, _, _ = _case("a")
    s, q = odx.leverage_scores(torch.from_numpy(X.copy()), torch.from_numpy(Z.copy()), odx.GaussianKernel(kernel), lam, n_total=5000,
                               return_q=True)
    rs, rq = lr.approx_scores(X, Z, kernel, lam, None, 5000, return_q=True)
    np.testing.assert_allclose(q.cpu().numpy(), rq, rtol=0, atol=1e-4)
    np.testing.assert_allclose(s.cpu().numpy(), (1.0 - q.cpu().numpy()) / (lam * 5000), rtol=1e-14)
    assert np.abs(s.cpu().numpy() - rs).max() <= 1e-4 / (lam * 5000)


# ------------------------------------------------------------------ E. the selector
def test_selector_on_the_gpu(be):
    import odx
    from oracle import falkon_ref as fr
    n, D, sigma, lam, cap = 1500, 70, 25.0, 1e-3, 400
    X, y, _ = blob_problem(n, D, seed=7)
    state = torch.get_rng_state().clone()
    sel = odx.LeverageSelector(odx.GaussianKernel(sigma), lam, cap, seed=0)
    Xd = torch.from_numpy(X).cuda()
    Z, Yz = sel.select(Xd, torch.from_numpy(y)[:, None])
    assert torch.equal(torch.get_rng_state(), state)
    idx = sel.indices_.numpy()
    assert len(np.unique(idx)) == len(idx) <= cap and idx.min() >= 0 and idx.max() < n and bool((sel.weights_ > 0).all())
    assert np.array_equal(Z.cpu().numpy(), X[idx]) and np.array_equal(Yz.numpy()[:, 0], y[idx])
    assert all(lv[3] <= cap and lv[4] <= cap for lv in sel.levels_)
    # the last level's scores from the dictionary they were computed with, in f64, under D's bar
    U_, J, c = sel.candidates_.numpy(), sel.prev_indices_.numpy(), sel.prev_weights_.numpy()
    lam_h = sel.levels_[-1][0]
    Kxz = lr.kernel_matrix(X[U_], X[J], sigma)
    Li = lr.inverse_factor(lr.dictionary_matrix(X[J], sigma, lam_h, c))
    ref = (1.0 - lr.row_quad(Kxz, Li)) / (lam_h * n)
    e = np.where(Kxz <= 0.99, ktol(sigma), max(ktol(sigma), 8e-4 / sigma ** 2))
    bar = 2.0 * (e * np.abs(Kxz @ Li.T @ Li)).sum(1) / (lam_h * n)
    err = np.abs(sel.scores_.numpy() - ref)
    print("selector: |J| %d, levels %d, max err / bar %.3f" % (len(idx), len(sel.levels_), float((err / bar).max())))
    assert (err <= bar).all(), float((err / bar).max())
    d_eff = float(lr.exact_scores(X, sigma, lam).sum())
    print("selector: d_eff_ %.1f exact %.1f" % (sel.d_eff_, d_eff))
    assert 1.0 <= sel.d_eff_ / d_eff <= 1.5
    # the estimator takes it as it takes a CenterSelector
    sel2 = odx.LeverageSelector(odx.GaussianKernel(sigma), lam, cap, seed=0)
    est = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma), penalty=lam, M=cap, center_selection=sel2, maxiter=20)
    est.fit(Xd, torch.from_numpy(y)[:, None].cuda())
    assert torch.equal(sel2.indices_, sel.indices_)
    o = est.options.solver_options()
    want, _ = fr.falkon_fit(X.astype(np.float64), y.astype(np.float64), idx, sigma, lam, maxiter=20, dtype=np.float64,
                            pc_eps=o.pc_epsilon, cg_epsilon=o.cg_epsilon)
    rel = float(np.linalg.norm(est.alpha_.cpu().numpy()[:, 0] - want[:, 0]) / np.linalg.norm(want[:, 0]))
    print("selector: alpha rel err %.2e" % rel)
    assert rel < 1e-4
