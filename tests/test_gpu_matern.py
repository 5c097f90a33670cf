"""Matern 3/2 and 5/2 kernels on the MI355X (odx.MaternKernel, the odx_radial_* entries): the preconditioner, the build in
the three storage formats, the scoring kernels, the estimators — every figure against the f64 oracle with its
gaussian_kernel replaced by tests/matern_ref.radial_kernel — and the refusals of every route that stayed Gaussian-only."""
import copy
import ctypes

import numpy as np
import pytest

from tests.matern_ref import radial_kernel
from tests.synth import blob_problem, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NUS = [1.5, 2.5]
# the largest slope of k in d^2 over the Gaussian's 1 / (2 sigma^2): 3 / (2 sigma^2) and 5 / (6 sigma^2)
SLOPE = {1.5: 3.0, 2.5: 5.0 / 3.0}


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def h2(be):
    """The split-f16 kernels with the storage, the scoring route and the tile pin restored afterwards."""
    old = (be.gauss, be.knm_storage, be.shared_mmv_min)
    be.gauss = "h2"
    yield be
    be.gauss, be.knm_storage, be.shared_mmv_min = old
    be.pin_gauss_tile(0)


@pytest.fixture
def matern_oracle(monkeypatch):
    """The whole f64 oracle on the kernel object it is handed: Preconditioner, falkon_fit, falkon_predict."""
    from oracle import falkon_ref as fr
    monkeypatch.setattr(fr, "gaussian_kernel", radial_kernel)
    return fr


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------ 1. the preconditioner
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("M", [7, 130, 257])
def test_preconditioner(be, matern_oracle, nu, M):
    """be.precond and be.precond_path (two penalties) against numpy f64 factors of the oracle's Preconditioner on that
    kernel, with a block of near-duplicate centres: 1e-7 x scale on the four inverse factors, info == 0."""
    import odx
    fr = matern_oracle
    D, sigma, eps, lams = 36, 9.0, 1e-5, [1e-4, 1e-2]
    rng = np.random.default_rng(M + D)
    Z = (rng.standard_normal((M, D)) * (20.0 / np.sqrt(D))).astype(np.float32)
    Z[M // 2:] = Z[: M - M // 2] + 0.01 * rng.standard_normal((M - M // 2, D)).astype(np.float32)   # near-duplicate centres
    k = odx.MaternKernel(sigma, nu)
    Zf = be.features(torch.from_numpy(Z))
    sc = lambda a: max(1.0, np.abs(a).max())          # noqa: E731

    def check(P, lam, note):
        assert int(P.info.item()) == 0
        ref = fr.Preconditioner(Z.astype(np.float64), k, lam, eps, np.float64)
        Ti, Ai = np.linalg.inv(ref.T), np.linalg.inv(ref.A)
        for name, want in (("LTit", Ti), ("LTi", Ti.T), ("LAit", Ai), ("LAi", Ai.T)):
            err = np.abs(getattr(P, name).cpu().numpy()[:, :M] - want).max()
            print("nu %g M %d %s %s: err %.2e bound %.2e" % (nu, M, note, name, err, 1e-7 * sc(want)))
            assert err < 1e-7 * sc(want), (note, name, err)

    check(be.precond(Zf, k, lams[0], eps), lams[0], "precond")
    Ps = be.precond_path(Zf, k, lams, eps)
    assert len(Ps) == 2
    for P, lam in zip(Ps, lams):
        check(P, lam, "path %g" % lam)
    # and it is not the Gaussian's
    G = be.precond(Zf, sigma, lams[0], eps)
    assert not torch.equal(G.LTi, be.precond(Zf, k, lams[0], eps).LTi)


# ------------------------------------------------------------------ 2. the build
BUILD_SHAPES = [(129, 7, 36, 5.0), (333, 130, 1024, 15.0), (257, 513, 70, 5.0)]
_build = {}


def _build_problem(n, M, D):
    """Rows, centres (the first five are copies of rows) and row weights of a build shape, made once."""
    if (n, M, D) not in _build:
        X, _, rng = blob_problem(n + M, D, seed=2000 + n + M + D)
        Xr, Z = X[:n].copy(), X[n:].copy()
        Z[:5] = Xr[10:15]
        _build[(n, M, D)] = (Xr, Z, rng.standard_normal(n))
    return _build[(n, M, D)]


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("fmt", ["f32", "u24", "bf16"])
@pytest.mark.parametrize("n,M,D,sigma", BUILD_SHAPES)
def test_build(h2, nu, fmt, n, M, D, sigma):
    """be.knm_rhs with a Matern kernel in every storage format: entries against f64 — generic ones at c max(1e-6, 5e-5 /
    (2 sigma^2)), reference values > 0.99 at c 8e-4 / sigma^2, c = 3 (nu = 3/2) or 5/3 (nu = 5/2) the kernel's largest slope in
    d^2 over the Gaussian's, bf16 blocks 2^-8 relative on top —, exact zeros in the pad columns, finite everywhere, copies of
    rows within 1e-4 of 1, K' w the stored block's own column sums, and the same bits into caller-provided storage."""
    import odx
    be = h2
    be.knm_storage = fmt
    Xr, Z, wh = _build_problem(n, M, D)
    k = odx.MaternKernel(sigma, nu)
    F, Zf = be.features(torch.from_numpy(Xr)), be.features(torch.from_numpy(Z))
    w = torch.from_numpy(wh).cuda()
    K, b = be.knm_rhs(F, Zf, k, w)
    assert K.fmt == fmt and (K.n, K.M) == (n, M)
    if K.ld > M:
        assert float(K.K[:, M:].float().abs().max()) == 0.0 and (K.K[:, M:] == 0).all()
        if K.lo is not None:
            assert int(K.lo[:, M:].max()) == 0
    got = K.dense().double()
    assert torch.isfinite(got).all() and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    ref = radial_kernel(Xr.astype(np.float64), Z.astype(np.float64), k, np.float64)
    err = np.abs(got.cpu().numpy() - ref)
    c = SLOPE[nu]
    generic = c * max(1e-6, 5e-5 / (2.0 * sigma * sigma))
    near_bar = c * 8e-4 / sigma ** 2
    extra = 2.0 ** -8 * ref if fmt == "bf16" else 0.0
    near = ref > 0.99
    assert int(near.sum()) >= 5
    over_generic = (err - extra)[~near].max(initial=-1.0)
    over_near = (err - extra)[near].max(initial=-1.0)
    print("nu %g %s (%d, %d, %d, %g): generic err %.2e (bar %.2e)  near-duplicate err %.2e (bar %.2e)"
          % (nu, fmt, n, M, D, sigma, err[~near].max(initial=0.0), generic, err[near].max(initial=0.0), near_bar))
    assert over_generic < generic, over_generic
    assert over_near < near_bar, over_near
    copies = got[10:15, :5].diagonal().cpu().numpy()
    assert np.abs(copies - 1.0).max() < 1e-4, copies
    want = got.t().cuda() @ w
    tol = 1e-12 * n * torch.clamp(want.abs(), min=1.0)
    assert bool(((b - want).abs() <= tol).all()), float((b - want).abs().max())
    buf = torch.empty(be.knm_bytes(n, M) + 16, dtype=torch.uint8, device="cuda")
    buf = buf[(-buf.data_ptr()) % 16:]
    K2, b2 = be.knm_rhs(F, Zf, k, w, out=buf)
    assert K2.K.data_ptr() == buf.data_ptr()
    assert torch.equal(K2.K, K.K) and (K.lo is None or torch.equal(K2.lo, K.lo)) and torch.equal(b2, b)
    # be.knm: the same block without the right-hand side
    K3 = be.knm(F, Zf, k)
    assert torch.equal(K3.K, K.K) and (K.lo is None or torch.equal(K3.lo, K.lo))


# ------------------------------------------------------------------ 3. the Gaussian through the new entries
def test_gauss_kind_through_the_radial_entries_is_bitwise_the_gaussian_entries(h2):
    from odx import hip
    be = h2
    n, M, D, sigma = 333, 130, 1024, 15.0
    Xr, Z, wh = _build_problem(n, M, D)
    F, Zf = be.features(torch.from_numpy(Xr)), be.features(torch.from_numpy(Z))
    be.pack(F), be.pack(Zf)
    lib, st = be.lib, be._stream()
    ops = [_p(F.P), F.P.stride(0), _p(F.meta), _p(F.sq), n, _p(Zf.P), Zf.P.stride(0), _p(Zf.meta), _p(Zf.sq), M, D]
    w = torch.from_numpy(wh).cuda()
    nb = lib.odx_gauss_knm_h2_rhs_workspace_bytes(n, M)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for fmt in ("f32", "u24", "bf16"):
        code = hip.KNM_CODE[fmt]
        Ka, Kb = be._knm_block(n, M, fmt, None), be._knm_block(n, M, fmt, None)
        ba, bb = (torch.full((M,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
        hip.check(lib.odx_gauss_knm_h2_store(*ops, sigma, code, _p(Ka.K), Ka.ld, _p(Ka.lo), Ka.ld, _p(w), _p(ba), _p(ws), nb, st))
        hip.check(lib.odx_radial_knm_h2_store(*ops, sigma, hip.KERNEL_GAUSS, code, _p(Kb.K), Kb.ld, _p(Kb.lo), Kb.ld, _p(w), _p(bb),
                                              _p(ws), nb, st))
        assert torch.equal(Ka.K, Kb.K) and (Ka.lo is None or torch.equal(Ka.lo, Kb.lo)) and torch.equal(ba, bb), fmt
        assert lib.odx_radial_knm_h2_store(*ops, sigma, 3, code, _p(Kb.K), Kb.ld, _p(Kb.lo), Kb.ld, _p(w), _p(bb), _p(ws), nb, st) == -1
    rng = np.random.default_rng(3)
    for T in (1, 3):
        V = torch.from_numpy(rng.standard_normal((M, T))).cuda()
        ranges = torch.tensor([[0, M]] * T, dtype=torch.int32, device="cuda")
        nb = lib.odx_gauss_mmv_h2_workspace_bytes(n, M, T)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        oa, ob = (torch.full((n, T), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
        hip.check(lib.odx_gauss_mmv_h2(*ops, sigma, _p(V), T, _p(ranges), T, _p(oa), T, _p(ws), nb, st))
        hip.check(lib.odx_radial_mmv_h2(*ops, sigma, hip.KERNEL_GAUSS, _p(V), T, _p(ranges), T, _p(ob), T, _p(ws), nb, st))
        assert torch.equal(oa, ob), T
        assert lib.odx_radial_mmv_h2(*ops, sigma, -1, _p(V), T, _p(ranges), T, _p(ob), T, _p(ws), nb, st) == -1
        oa, ob = (torch.full((n, T), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2))
        hip.check(lib.odx_gauss_mmvn_h2(*ops, sigma, _p(V), T, T, _p(oa), T, _p(ws), nb, st))
        hip.check(lib.odx_radial_mmvn_h2(*ops, sigma, hip.KERNEL_GAUSS, _p(V), T, T, _p(ob), T, _p(ws), nb, st))
        assert torch.equal(oa, ob), T
        assert lib.odx_radial_mmvn_h2(*ops, sigma, 7, _p(V), T, T, _p(ob), T, _p(ws), nb, st) == -1
    # the preconditioner entries: an unknown kind is refused
    Zs = be.f32(Zf)
    mats = torch.empty((4, M, M), dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    nb = lib.odx_falkon_precond_workspace_bytes(M, D)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.odx_falkon_precond_radial_f64(_p(Zs.X), Zs.ld, M, D, sigma, 5, 1e-4, 1e-5, _p(mats[0]), _p(mats[1]), _p(mats[2]),
                                             _p(mats[3]), M, _p(info), _p(ws), nb, st) == -1


# ------------------------------------------------------------------ 4. scoring
_score = {}


def _score_problem(n, M, D):
    if (n, M, D) not in _score:
        X, _, rng = blob_problem(n + M, D, seed=3000 + n + M + D)
        _score[(n, M, D)] = (X[:n].copy(), X[n:].copy(), rng.standard_normal((M, 9)) * np.logspace(0, -2, 9)[None, :])
    return _score[(n, M, D)]


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("n,M,D", [(300, 130, 256), (1000, 513, 70)])
def test_scoring(h2, nu, n, M, D):
    """be.mmv with one column, with a block-structured 3-column V (ranges) and on the shared-column route with T = 3 and T = 9
    against f64 K @ V at 5e-5 max(1, |ref|), the bar of the shared-scoring tests; the shared route equals the per-column
    launch bit for bit, as for the Gaussian."""
    import odx
    from odx.falkon import block_ranges
    be = h2
    sigma = 8.0
    Xr, Z, Vh = _score_problem(n, M, D)
    k = odx.MaternKernel(sigma, nu)
    F, Zf = be.features(torch.from_numpy(Xr)), be.features(torch.from_numpy(Z))
    Kref = radial_kernel(Xr.astype(np.float64), Z.astype(np.float64), k, np.float64)

    def check(got, V, note):
        ref = Kref @ V
        got = got.cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        err, bound = np.abs(got - ref).max(), 5e-5 * max(1.0, np.abs(ref).max())
        print("nu %g (%d, %d, %d) %s: err %.2e bound %.2e" % (nu, n, M, D, note, err, bound))
        assert err < bound, (note, err)

    be.shared_mmv_min = None
    check(be.mmv(F, Zf, k, torch.from_numpy(Vh[:, :1]).cuda()), Vh[:, :1], "one column")
    Vb = np.zeros((M, 3))
    cuts = [0, M // 3, M // 3 + 5, M]
    for c in range(3):
        Vb[cuts[c]:cuts[c + 1], c] = Vh[cuts[c]:cuts[c + 1], c]
    Vbt = torch.from_numpy(Vb).cuda()
    ranges = block_ranges(Vbt)
    assert ranges.cpu().tolist() == [[cuts[c], cuts[c + 1]] for c in range(3)]
    check(be.mmv(F, Zf, k, Vbt, ranges), Vb, "three ranges")
    check(be.mmv(F, Zf, k, Vbt, ranges, max_range=int(max(np.diff(cuts)))), Vb, "three ranges, max_range")
    for T in (3, 9):
        V = torch.from_numpy(Vh[:, :T]).cuda()
        be.shared_mmv_min = None
        per_column = be.mmv(F, Zf, k, V, None).clone()
        be.shared_mmv_min = 2
        shared = be.mmv(F, Zf, k, V, None)
        check(shared, Vh[:, :T], "shared T = %d" % T)
        assert torch.equal(shared, per_column), T


# ------------------------------------------------------------------ 5. fits
class _Selector:
    """MyCenterSelector's contract: the rows of a fixed index list."""

    def __init__(self, idx):
        self.idx = torch.as_tensor(idx, dtype=torch.int64)

    def select(self, X, Y):
        return X[self.idx.to(X.device)]


def _estimator(k, idx, lam):
    import odx
    return odx.InCoreFalkon(kernel=k, penalty=lam, M=len(idx), maxiter=20, center_selection=_Selector(idx),
                            options=odx.FalkonOptions(pc_epsilon_32=1e-5, cg_epsilon_32=1e-7))


_fits = {}


def _fit_reference(fr, n, M, D, sigma, lam, nu):
    """Problem and f64 reference fit of a case, computed once and shared by the storage variants."""
    import odx
    key = (n, M, D, sigma, lam, nu)
    if key not in _fits:
        X, y, rng = blob_problem(n, D, seed=n + M)
        idx = centres(y, M, rng)
        k = odx.MaternKernel(sigma, nu)
        Xd = X.astype(np.float64)
        ref, Z = fr.falkon_fit(Xd, y.astype(np.float64), idx, k, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        _fits[key] = (X, y, idx, ref, fr.falkon_predict(Xd, Z, ref, k))
    return _fits[key]


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("storage", ["auto", "u24"])
@pytest.mark.parametrize("n,M,D,sigma,lam", [(5000, 500, 256, 10.0, 1e-5), (777, 129, 36, 5.0, 1e-3)])
def test_fit_alpha_parity(h2, matern_oracle, nu, storage, n, M, D, sigma, lam):
    """InCoreFalkon(kernel=MaternKernel): alpha_ within 1e-4 relative of the f64 oracle on that kernel (pc_eps 1e-5, cg_epsilon
    1e-7, 20 iterations) and predict within 1e-4 of its scores — the project's bar for the Gaussian, unwidened."""
    import odx
    be = h2
    be.knm_storage = storage
    X, y, idx, ref, pref = _fit_reference(matern_oracle, n, M, D, sigma, lam, nu)
    est = _estimator(odx.MaternKernel(sigma, nu), idx, lam)
    Xt = torch.from_numpy(X).cuda()
    est.fit(Xt, torch.from_numpy(y).cuda())
    assert tuple(est.alpha_.shape) == (M, 1)
    rel = _rel(est.alpha_.cpu().numpy()[:, 0], ref[:, 0])
    perr = float(np.abs(est.predict(Xt).cpu().numpy() - pref).max())
    print("nu %g storage %s (%d, %d, %d, %g, %g): alpha rel %.2e  score err %.2e" % (nu, storage, n, M, D, sigma, lam, rel, perr))
    assert rel < 1e-4, rel
    assert perr < 1e-4, perr


# ------------------------------------------------------------------ 6. everything built on one block
@pytest.mark.parametrize("nu", NUS)
def test_path_multi_cv_and_predict_path(h2, nu):
    import odx
    be = h2
    n, M, D, sigma = 777, 129, 36, 5.0
    X, y, rng = blob_problem(n, D, seed=n + M)
    idx = centres(y, M, rng)
    k = odx.MaternKernel(sigma, nu)
    Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    pens = [1e-3, 1e-4, 1e-2]
    rel = lambda a, b: float((a - b).norm() / b.norm())          # noqa: E731
    # fit_path: three single fits
    path = _estimator(k, idx, pens[0]).fit_path(Xt, Yt, pens)
    singles = [_estimator(k, idx, lam).fit(Xt, Yt) for lam in pens]
    for m, s, lam in zip(path, singles, pens):
        assert m.kernel is k and m.penalty == lam
        print("nu %g lam %g: path against single fit %.2e" % (nu, lam, rel(m.alpha_, s.alpha_)))
        assert rel(m.alpha_, s.alpha_) < 1e-9
    # fit_multi: three fits
    Y3 = torch.stack([Yt, -Yt, torch.where(torch.arange(n, device="cuda") % 3 == 0, 1.0, -1.0).to(Yt.dtype)], dim=1)
    multi = _estimator(k, idx, pens[0]).fit_multi(Xt, Y3)
    assert tuple(multi.alpha_.shape) == (M, 3)
    for t in range(3):
        one = _estimator(k, idx, pens[0]).fit(Xt, Y3[:, t])
        print("nu %g column %d: multi against single fit %.2e" % (nu, t, rel(multi.alpha_[:, t], one.alpha_[:, 0])))
        assert rel(multi.alpha_[:, t], one.alpha_[:, 0]) < 1e-9
    pm = multi.predict(Xt[:200])
    assert tuple(pm.shape) == (200, 3) and torch.isfinite(pm).all()
    # fit_cv: the refit members are fit_path's; a held-out score is the fold fit's predict on the held-out rows
    res = _estimator(k, idx, pens[0]).fit_cv(Xt, Yt, pens[:2], folds=3, seed=0, refit=True)
    assert len(res.estimators) == 2 and tuple(res.fold_alphas.shape) == (2, 3, M)
    fold_of = torch.as_tensor(res.fold_of).cuda()
    for l in range(2):
        print("nu %g lam %g: refit against path %.2e" % (nu, pens[l], rel(res.estimators[l].alpha_, path[l].alpha_)))
        assert rel(res.estimators[l].alpha_, path[l].alpha_) < 1e-9
        for f in range(3):
            member = copy.copy(path[l])
            member.alpha_ = res.fold_alphas[l, f].reshape(-1, 1).to(path[l].alpha_.device)
            held = fold_of == f
            want = member.predict(Xt[held])[:, 0]
            err = float((res.scores[held, l] - want).abs().max())
            print("nu %g lam %g fold %d: held-out score err %.2e" % (nu, pens[l], f, err))
            assert err < 1e-4, (l, f, err)
    # predict_path: the members' predict, bit for bit
    both = odx.predict_path(path, Xt[:300])
    assert tuple(both.shape) == (300, 3)
    for l, m in enumerate(path):
        assert torch.equal(both[:, l:l + 1], m.predict(Xt[:300])), l
    # and the estimator pickles with its kernel
    import pickle
    back = pickle.loads(pickle.dumps(path[0]))
    assert back.kernel.kind == k.kind and torch.equal(back.predict(Xt[:50]), path[0].predict(Xt[:50]))


# ------------------------------------------------------------------ 7. refusals
def test_refusals(h2):
    import odx
    be = h2
    n, M, D, sigma = 777, 129, 36, 5.0
    X, y, rng = blob_problem(n, D, seed=n + M)
    idx = centres(y, M, rng)
    Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    k = odx.MaternKernel(sigma, 1.5)
    with pytest.raises(NotImplementedError):
        odx.MaternKernel(sigma, 0.5)
    with pytest.raises(NotImplementedError):
        _estimator(k, idx, 1e-3).fit_grid(Xt, Yt, [4.0, 5.0], [1e-3])
    be.knm_storage = "stream"
    with pytest.raises(NotImplementedError, match="stream"):
        _estimator(k, idx, 1e-3).fit(Xt, Yt)
    be.knm_storage = "auto"
    be.gauss = "f32"
    with pytest.raises(NotImplementedError, match="h2"):
        _estimator(k, idx, 1e-3).fit(Xt, Yt)
    F, Zf = be.features(Xt), be.features(Xt[:M].contiguous())
    with pytest.raises(NotImplementedError, match="h2"):
        be.mmv(F, Zf, k, torch.zeros(M, 1, dtype=torch.float64))
    be.gauss = "h2"
    with pytest.raises(TypeError):
        be.precond_batched([Zf], k, 1e-3, 1e-5)
    with pytest.raises(TypeError):
        be.knm_rhs_sigmas(F, Zf, [k], None)
    with pytest.raises(TypeError):
        be.mmv_sigmas(F, Zf, [k], torch.zeros(M, 1, dtype=torch.float64))
    # 16-bit rows at native width stay Gaussian-only
    Fb, Zb = be.features(Xt.to(torch.bfloat16)), be.features(Xt[:M].to(torch.bfloat16).contiguous())
    if be._native16_pair(Fb, Zb):
        with pytest.raises(NotImplementedError, match="native"):
            be.knm_rhs(Fb, Zb, k, None)
    gm = _estimator(odx.GaussianKernel(sigma), idx, 1e-3).fit_path(Xt, Yt, [1e-3])[0]
    mm = copy.copy(gm)
    mm.kernel = k
    with pytest.raises(ValueError, match="kernel function"):
        odx.predict_path([gm, mm], Xt[:10])
