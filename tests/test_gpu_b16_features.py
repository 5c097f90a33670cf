"""Gaussian FALKON on rows that are bf16 / f16 already, at native width (HipBackend.native16): odx_row_sqnorm_b16,
odx_gauss_knm_b16_store, odx_gauss_mmv_b16, odx_gauss_mmvn_b16 and everything above them, up to InCoreFalkon.fit(X_bf16).

The oracle is the f64 one on `X.double()` of the 16-bit rows: the rounding of the features is the caller's, the arithmetic
after it is held to the project's own bars, imported from tests/test_gpu_kernels.py (the per-entry rule around `ktol`), 1e-12
relative for the f64 right-hand side against the STORED values, alpha < 1e-4 relative and scores < 1e-4 max(1, max |ref|)
for fits.  The compact storage formats are held to their existing statement: the block is the f32 block of the same build,
entry by entry rounded (test_u24_stored_knm_is_the_rounded_f32_block / test_bf16_stored_knm)."""
import copy
import io
import pickle

import numpy as np
import pytest

from tests.test_gpu_kernels import assert_k_close, kdense

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
NEW_ENTRIES = ("odx_row_sqnorm_b16", "odx_gauss_knm_b16_store_workspace_bytes", "odx_gauss_knm_b16_store",
               "odx_gauss_mmv_b16_workspace_bytes", "odx_gauss_mmv_b16", "odx_gauss_mmvn_b16_workspace_bytes", "odx_gauss_mmvn_b16")


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def native(be):
    """The backend with native16 on, every switch the tests touch put back afterwards."""
    from odx import options
    own = "native16" in vars(be)           # (an instance attribute of its own: put back; else removed again, so that the class's counts)
    old = (be.native16, be.knm_storage, be.gauss, options.current().h2_tile, be.shared_mmv_min, "shared_mmv_min" in vars(be))
    be.native16 = True
    yield be
    be.knm_storage, be.gauss = old[1:3]
    be.pin_gauss_tile(old[3])
    if own:
        be.native16 = old[0]
    else:
        del be.native16
    if old[5]:
        be.shared_mmv_min = old[4]
    else:
        vars(be).pop("shared_mmv_min", None)


def rows16(rng, n, D, dtype):
    """n rows of the reference's norm (20), rounded to `dtype`: the 16-bit tensor and its exact f64 values."""
    X = torch.from_numpy((rng.standard_normal((n, D)) * (20.0 / np.sqrt(D))).astype(np.float32)).to(dtype)
    return X, X.double().numpy()


# ------------------------------------------------------------------------------------------------ 1. norms
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("n,D", [(300, 256), (5, 36), (129, 1000), (3, 8)])
def test_row_norms_of_16bit_rows(native, dt, n, D):
    """Squares of 16-bit values are exact in f32; a lane adds at most 8 ceil(D / 512) of them in sequence and the wave's tree
    adds six more times, all terms non-negative: at most 8 ceil(D / 512) + 6 roundings of 2^-24 relative each."""
    X, X64 = rows16(np.random.default_rng(n + D), n, D, DTYPES[dt])
    F = native.features(X.cuda())
    assert F.b16 and F.X.dtype == DTYPES[dt] and F.sq.dtype == torch.float32
    ref = (X64 ** 2).sum(1)
    bound = (8 * -(-D // 512) + 6) * 2.0 ** -24
    assert np.abs(F.sq.cpu().numpy().astype(np.float64) - ref).max() <= bound * ref.max()


# ------------------------------------------------------------------------------------------------ 2. build
BUILD_SHAPES = [(300, 70, 36), (257, 513, 64), (513, 300, 65), (1000, 1300, 1000)]


@pytest.fixture(scope="module")
def build_problem():
    """(X16, X64, Z16, Z64, w, {sigma: f64 kernel}) per (dtype, shape), made once: the centres are half fresh rows, half rows
    drawn from X (exact duplicates, K = 1)."""
    from oracle import falkon_ref as fr
    cache = {}

    def get(dt, shape):
        key = (dt, shape)
        if key not in cache:
            n, M, D = shape
            rng = np.random.default_rng(n + M + D)
            X, X64 = rows16(rng, n, D, DTYPES[dt])
            Zn, _ = rows16(rng, M - M // 2, D, DTYPES[dt])
            Z = torch.cat([Zn, X[torch.from_numpy(rng.integers(0, n, M // 2))]])
            Z64 = Z.double().numpy()
            cache[key] = (X, X64, Z, Z64, rng.standard_normal(n), {s: fr.gaussian_kernel(X64, Z64, s) for s in (5.0, 15.0)})
        return cache[key]
    return get


@pytest.mark.parametrize("sigma", [5.0, 15.0])
@pytest.mark.parametrize("shape", BUILD_SHAPES)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_build_on_16bit_rows(native, build_problem, dt, shape, sigma):
    """All three storage formats, with and without the fused right-hand side, on the wide core (D <= 64: a single stage)."""
    n, M, D = shape
    X, X64, Z, Z64, w, refs = build_problem(dt, shape)
    ref = refs[sigma]
    native.pin_gauss_tile(256)
    F, Zf = native.features(X.cuda()), native.features(Z.cuda())
    wd = torch.from_numpy(w).cuda()
    native.knm_storage = "f32"
    K32 = native.knm(F, Zf, sigma)
    assert K32.fmt == "f32"
    k32 = kdense(K32)
    assert_k_close(k32, ref, sigma, note=("f32", dt, shape))
    dup = ref > 1.0 - 1e-9                   # centres drawn from the rows
    assert dup.any() and np.abs(k32[dup] - 1.0).max() < 8e-4 / sigma ** 2
    for fmt in ("f32", "u24", "bf16"):
        native.knm_storage = fmt
        K, ktw = native.knm_rhs(F, Zf, sigma, wd)
        assert K.fmt == fmt
        got = kdense(K)
        if fmt == "f32":
            assert np.array_equal(got, k32)
        elif fmt == "u24":
            q = np.minimum(np.rint(k32.astype(np.float64) * 2.0 ** 24), 2.0 ** 24 - 1)
            assert np.array_equal(got.astype(np.float64), q * 2.0 ** -24)
            assert np.array_equal(kdense(native.knm(F, Zf, sigma)), got)          # without the right-hand side: the same block
        else:
            assert np.array_equal(got, torch.from_numpy(k32).to(torch.bfloat16).to(torch.float32).numpy())
            assert np.array_equal(kdense(native.knm(F, Zf, sigma)), got)
        want = got.astype(np.float64).T @ w          # the sums are over the entries that were stored
        assert np.abs(ktw.cpu().numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) * n
    assert F.P is None and Zf.P is None and F.f32 is None and Zf.f32 is None          # nothing was packed, nothing upcast


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_build_on_the_distinct_columns_of_repeated_16bit_centres(native, build_problem, dt):
    """A centre list with repeats under u24: the block of the distinct centres (the column-map path), built on the 16-bit rows."""
    from odx.cols import column_map
    shape, sigma = (513, 300, 65), 15.0
    n, M, D = shape
    X, X64, Z, Z64, w, refs = build_problem(dt, shape)
    pick = np.random.default_rng(7).integers(0, M // 3, M)           # every list position names one of the first M / 3 centres
    native.pin_gauss_tile(256)
    F, Zf = native.features(X.cuda()), native.features(Z[torch.from_numpy(pick)].cuda())
    Zf.cmap = column_map(pick)
    first, col_of = (t.cpu().numpy() for t in Zf.cmap.on(native.device)[:2])
    native.knm_storage = "f32"
    k32 = kdense(native.knm(F, native.rows(Zf, first), sigma))
    assert_k_close(k32, refs[sigma][:, pick][:, first], sigma, note=("distinct", dt))
    native.knm_storage = "u24"
    K, ktw = native.knm_rhs(F, Zf, sigma, torch.from_numpy(w).cuda())
    assert K.fmt == "u24" and K.cmap is Zf.cmap and K.Mv == M and K.M == len(np.unique(pick)) < M
    got = kdense(K).astype(np.float64)
    assert np.array_equal(got, np.minimum(np.rint(k32.astype(np.float64) * 2.0 ** 24), 2.0 ** 24 - 1) * 2.0 ** -24)
    want = (got.T @ w)[col_of]
    assert np.abs(ktw.cpu().numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) * n
    assert Zf.P is None and F.P is None and Zf.f32 is None


class _Calls(list):
    lib = None


def _spy(be, names):
    """be.lib replaced by a wrapper that appends the name of every call of `names` to the returned list; its `.lib` is the
    library to put back."""
    calls = _Calls()
    calls.lib = lib = be.lib

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in names:
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    be.lib = Spy()
    return calls


# ------------------------------------------------------------------------------------------------ 3. scoring
SCORE_BAR = 5e-5          # test_mmv_block_structure's: |scores - ref| < 5e-5 max(1, max |ref|)


@pytest.fixture(scope="module")
def score_problem():
    """(X16, Z16, f64 kernel) per (dtype, n, M, D, sigma), made once."""
    from oracle import falkon_ref as fr
    cache = {}

    def get(dt, n, M, D, sigma):
        key = (dt, n, M, D, sigma)
        if key not in cache:
            rng = np.random.default_rng(n + 3 * M + 7 * D)
            X, X64 = rows16(rng, n, D, DTYPES[dt])
            Z, Z64 = rows16(rng, M, D, DTYPES[dt])
            cache[key] = (X, Z, fr.gaussian_kernel(X64, Z64, sigma))
        return cache[key]
    return get


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("D", [36, 65, 150, 300, 1000])
@pytest.mark.parametrize("M", [70, 1300])
@pytest.mark.parametrize("n", [1, 300, 513])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_scoring_on_16bit_rows(native, score_problem, dt, n, M, D, tile):
    """mmv with per-column centre ranges (one starting and ending off every tile boundary, one empty) and the shared-centre
    mmvn with 1, 8 and 11 columns (shared_mmv_min = 1: one column takes mmvn's two-column kernel, 8 its eight-column one, 11
    that and the four-column one), on both tile cores.  Stages of 64 features: D = 36 is 1, 65 is 2, 150 is 3, 300 is 5,
    1000 is 16.  The 128 x 128 core's k-tile is two stages, so 36 is a lone half k-tile, 150 and 300 are one and two full
    k-tiles followed by a half one (the backed-off prefetch inside the loop, the clearing on the last iteration only), and
    65 and 1000 have no half k-tile."""
    sigma = 15.0
    X, Z, Kref = score_problem(dt, n, M, D, sigma)
    rng = np.random.default_rng(n + M + D + tile)
    native.pin_gauss_tile(tile)
    F, Zf = native.features(X.cuda()), native.features(Z.cuda())
    ranges = np.array([[0, M], [M // 3 + 1, M - 5], [M // 2, M // 2], [3, min(M, 131)]], dtype=np.int32)
    V = np.zeros((M, len(ranges)))
    for c, (a, b) in enumerate(ranges):
        V[a:b, c] = rng.standard_normal(b - a)
    ref = Kref @ V
    got = native.mmv(F, Zf, sigma, torch.from_numpy(V).cuda(), torch.from_numpy(ranges).cuda(),
                     max_range=int((ranges[:, 1] - ranges[:, 0]).max())).cpu().numpy()
    assert np.abs(got - ref).max() < SCORE_BAR * max(1.0, np.abs(ref).max()), ("mmv", np.abs(got - ref).max())
    assert np.all(got[:, 2] == 0.0)
    calls = _spy(native, ("odx_gauss_mmv_b16", "odx_gauss_mmvn_b16"))
    try:
        for T in (1, 8, 11):
            Vd = rng.standard_normal((M, T))
            ref = Kref @ Vd
            native.shared_mmv_min = 1
            got = native.mmv(F, Zf, sigma, torch.from_numpy(Vd).cuda()).cpu().numpy()
            assert np.abs(got - ref).max() < SCORE_BAR * max(1.0, np.abs(ref).max()), ("mmvn", T, np.abs(got - ref).max())
            native.shared_mmv_min = None          # the same columns one by one (odx_gauss_mmv_b16): the same bits
            assert np.array_equal(native.mmv(F, Zf, sigma, torch.from_numpy(Vd).cuda()).cpu().numpy(), got)
    finally:
        native.lib = calls.lib
    assert calls == ["odx_gauss_mmvn_b16", "odx_gauss_mmv_b16"] * 3
    assert F.P is None and Zf.P is None and F.f32 is None and Zf.f32 is None


# ------------------------------------------------------------------------------------------------ 4. fallbacks
def _check_build_and_scores(be, F, Zf, Kref, sigma, w, V):
    K, ktw = be.knm_rhs(F, Zf, sigma, torch.from_numpy(w).cuda())
    if K.fmt == "stream":          # no block: K' w from recomputed entries, each within ktol of the f64 kernel
        from tests.test_gpu_kernels import ktol
        assert np.abs(ktw.cpu().numpy() - Kref.T @ w).max() < ktol(sigma) * np.abs(w).sum()
    else:
        got = kdense(K)
        assert_k_close(got, Kref, sigma)
        want = got.astype(np.float64).T @ w
        assert np.abs(ktw.cpu().numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max()) * len(w)
    ref = Kref @ V
    got = be.mmv(F, Zf, sigma, torch.from_numpy(V).cuda()).cpu().numpy()
    assert np.abs(got - ref).max() < SCORE_BAR * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("case", ["b16_rows_f32_centres", "f32_rows_b16_centres", "bf16_rows_f16_centres", "stream", "direct_small"])
def test_what_has_no_16bit_kernel_goes_through_the_f32_form(native, case):
    """Mixed types, the streamed shard and a direct_small block: nothing raises on a 16-bit Features, the same bars hold."""
    from oracle import falkon_ref as fr
    n, M, D, sigma = (40, 30, 36, 15.0) if case == "direct_small" else (600, 300, 100, 15.0)
    rng = np.random.default_rng(11)
    X, X64 = rows16(rng, n, D, torch.bfloat16)
    Z, Z64 = rows16(rng, M, D, torch.float16 if case == "bf16_rows_f16_centres" else torch.bfloat16)
    Xd = X.float().cuda() if case == "f32_rows_b16_centres" else X.cuda()
    Zd = Z.float().cuda() if case == "b16_rows_f32_centres" else Z.cuda()
    if case == "stream":
        native.knm_storage = "stream"
    if case != "direct_small":
        native.pin_gauss_tile(256)
    F, Zf = native.features(Xd), native.features(Zd)
    assert F.b16 == (case != "f32_rows_b16_centres") and Zf.b16 == (case != "b16_rows_f32_centres")
    if case == "direct_small":
        assert native.direct_small(n, M, D)
    _check_build_and_scores(native, F, Zf, fr.gaussian_kernel(X64, Z64, sigma), sigma, rng.standard_normal(n), rng.standard_normal((M, 3)))
    assert (F.P is None or not F.b16) and (Zf.P is None or not Zf.b16)          # whatever was packed is the f32 form's
    assert (F.f32 is not None or not F.b16) and (Zf.f32 is not None or not Zf.b16)


def test_other_backend_calls_take_a_16bit_features(native):
    """precond, the grouped build, the per-column widths and a plain product: each runs on the f32 form and agrees with the
    same call on the upcast rows, bit for bit."""
    rng = np.random.default_rng(5)
    X, _ = rows16(rng, 400, 70, torch.bfloat16)
    Z, _ = rows16(rng, 90, 70, torch.bfloat16)
    native.pin_gauss_tile(256)
    F, Zf = native.features(X.cuda()), native.features(Z.cuda())
    F32, Z32 = native.features(X.float().cuda()), native.features(Z.float().cuda())
    assert F.b16 and not F32.b16
    P, P32 = native.precond(Zf, 10.0, 1e-4, 1e-5), native.precond(Z32, 10.0, 1e-4, 1e-5)
    assert torch.equal(P.LTi, P32.LTi) and torch.equal(P.LAi, P32.LAi)
    w = torch.from_numpy(rng.standard_normal(400)).cuda()
    for (K, b), (K2, b2) in zip(native.knm_rhs_sigmas(F, Zf, [5.0, 15.0], w), native.knm_rhs_sigmas(F32, Z32, [5.0, 15.0], w)):
        assert torch.equal(K.dense(), K2.dense()) and torch.equal(b, b2)
    V = torch.from_numpy(rng.standard_normal((90, 2))).cuda()
    assert torch.equal(native.mmv_sigmas(F, Zf, [5.0, 15.0], V), native.mmv_sigmas(F32, Z32, [5.0, 15.0], V))
    assert torch.equal(native.gemm_nt(F, Zf), native.gemm_nt(F32, Z32))


# ------------------------------------------------------------------------------------------------ 5. estimators
N_FIT, M_FIT, D_FIT, SIGMA_FIT, LAM_FIT = 4000, 500, 256, 10.0, 1e-4


@pytest.fixture(scope="module")
def fit_problem():
    """bf16 rows, labels, centre indices and the f64 reference fits (one per penalty of the path) on the upcast rows."""
    from oracle import falkon_ref as fr
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(N_FIT, D_FIT, seed=77)
    idx = np.asarray(centres(y, M_FIT, rng))
    X16 = torch.from_numpy(X).to(torch.bfloat16)
    X64 = X16.double().numpy()
    refs = {}
    for lam in (LAM_FIT, 1e-3, 1e-5):
        ref, Z = fr.falkon_fit(X64, y.astype(np.float64), idx, SIGMA_FIT, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        refs[lam] = (ref[:, 0], fr.falkon_predict(X64, Z, ref, SIGMA_FIT)[:, 0])
    return X16, y, idx, refs


def _estimator(idx, lam=LAM_FIT):
    from odx.falkon import GaussianKernel, InCoreFalkon
    from odx.wrappers import CenterSelector
    return InCoreFalkon(kernel=GaussianKernel(SIGMA_FIT), penalty=lam, M=len(idx), maxiter=20,
                        center_selection=CenterSelector(torch.as_tensor(idx, dtype=torch.int64)))


def _held_to_the_reference(est, Xd, ref):
    alpha = est.alpha_.cpu().numpy()[:, 0]
    rel = np.linalg.norm(alpha - ref[0]) / np.linalg.norm(ref[0])
    assert rel < 1e-4, rel
    scores = est.predict(Xd).cpu().numpy()[:, 0]
    assert np.abs(scores - ref[1]).max() < 1e-4 * max(1.0, np.abs(ref[1]).max()), np.abs(scores - ref[1]).max()
    return scores


@pytest.mark.parametrize("storage,tile", [("f32", 256), ("f32", 0), ("u24", 0)])
def test_fit_on_bf16_rows(native, fit_problem, storage, tile):
    """InCoreFalkon.fit(X_bf16): alpha and scores against the f64 reference on the same rows; the model keeps bf16 centres
    and survives deepcopy and pickle with the same bits.  (f32 storage, tile not pinned: the shape's 128 x 128 build has no
    16-bit kernel and takes the f32 form; the other two build on the 16-bit rows.)"""
    X16, y, idx, refs = fit_problem
    native.knm_storage = storage
    native.pin_gauss_tile(tile)
    Xd = X16.cuda()
    est = _estimator(idx).fit(Xd, torch.from_numpy(y))
    assert est.ny_points_.dtype == torch.bfloat16 and tuple(est.ny_points_.shape) == (M_FIT, D_FIT)
    assert est._centres().b16 and est._centres().P is None
    scores = _held_to_the_reference(est, Xd, refs[LAM_FIT])
    for other in (copy.deepcopy(est), pickle.loads(pickle.dumps(est))):
        assert other.ny_points_.dtype == torch.bfloat16
        assert np.array_equal(other.predict(Xd).cpu().numpy()[:, 0], scores)
    buf = io.BytesIO()
    torch.save(est, buf)
    assert buf.getbuffer().nbytes < M_FIT * D_FIT * 2 + M_FIT * 8 + 16384          # 2 bytes per centre entry, not 4
    # an f32 model scores bf16 rows, and this one scores f32 rows, through the upcast
    assert np.array_equal(est.predict(Xd.float()).cpu().numpy()[:, 0], est.kernel.mmv(Xd.float(), est.ny_points_.float(), est.alpha_).cpu().numpy()[:, 0])


def test_path_and_batch_fits_on_bf16_rows(native, fit_problem):
    """predict_path over a three-penalty fit_path (every member against its reference; the shared scoring equals the
    members' own), and a fit_batch of three classes against their single fits, bit for bit."""
    from odx.falkon import fit_batch, predict_path
    X16, y, idx, refs = fit_problem
    native.knm_storage = "u24"
    Xd, yd = X16.cuda(), torch.from_numpy(y)
    lams = [LAM_FIT, 1e-3, 1e-5]
    members = _estimator(idx).fit_path(Xd, yd, lams)
    assert all(m.ny_points_.dtype == torch.bfloat16 for m in members)
    S = predict_path(members, Xd).cpu().numpy()
    for l, (m, lam) in enumerate(zip(members, lams)):
        own = _held_to_the_reference(m, Xd, refs[lam])
        assert np.array_equal(S[:, l], own)
    # three classes: the labels of the problem, their negation, and a third of the rows relabelled
    y3 = y.copy()
    y3[::3] = -y3[::3]
    ys = [torch.from_numpy(v) for v in (y, -y, y3)]
    singles = [_estimator(idx).fit(Xd, v) for v in ys]
    batch = fit_batch([_estimator(idx) for _ in ys], [Xd] * 3, ys)
    for a, b in zip(singles, batch):
        assert b.ny_points_.dtype == torch.bfloat16
        assert torch.equal(a.alpha_, b.alpha_) and torch.equal(a.ny_points_, b.ny_points_)


def test_batch_fit_on_side_streams_through_the_f32_form(native, fit_problem):
    """Eight classes (two half preconditioner chains on side streams) with the K_nM builds on two class streams, at a shape
    whose build has no 16-bit kernel (f32 storage on the 128 x 128 core): the cached f32 form of rows and centres is made on
    one stream and read on others.  Every class equals its single fit on the caller's stream, bit for bit; the rows'
    norms are completed on the operand that exists."""
    from odx.falkon import fit_batch
    X16, y, idx, refs = fit_problem
    native.knm_storage = "f32"
    native.pin_gauss_tile(0)
    Xd = X16[:, :200].contiguous().cuda()          # D % 64 != 0: the operand is a padded copy
    rng = np.random.default_rng(3)
    ys = [torch.from_numpy(np.where(rng.random(len(y)) < 0.1 * (k + 1), -y, y).astype(np.float32)) for k in range(8)]
    singles = [_estimator(idx).fit(Xd, v) for v in ys]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    batch = fit_batch([_estimator(idx) for _ in ys], [Xd] * 8, ys, streams=streams)
    torch.cuda.synchronize()
    for a, b in zip(singles, batch):
        assert b.ny_points_.dtype == torch.bfloat16 and torch.equal(a.alpha_, b.alpha_)
    F = native.features(Xd, norms=False)
    assert F.sq is None and F.ld == 256
    G = native.with_norms(F)
    assert G is F and torch.equal(F.sq, native.features(Xd).sq)
    # the f32 form follows the rows: rewritten in place, it is made again
    first = native.f32(F)
    assert native.f32(F) is first
    F.X.mul_(2)
    assert native.f32(F) is not first and torch.equal(native.f32(F).X, F.X.float())


def test_fit_grid_on_bf16_rows(native, fit_problem):
    """fit_grid has no 16-bit kernel (the grouped build): its members, fitted through the f32 form, meet the fit's bars."""
    X16, y, idx, refs = fit_problem
    native.knm_storage = "u24"
    Xd = X16.cuda()
    grid = _estimator(idx).fit_grid(Xd, torch.from_numpy(y), [SIGMA_FIT], [LAM_FIT, 1e-3])
    assert grid[0][0].ny_points_.dtype == torch.bfloat16
    for m, lam in zip(grid[0], (LAM_FIT, 1e-3)):
        _held_to_the_reference(m, Xd, refs[lam])


def test_heads_score_16bit_features_against_16bit_models(native, fit_problem):
    """The heads' batched scoring keeps the centres 16-bit when the features and every model's centres share the type."""
    from odx.heads import OnlineBoxPredictor
    X16, y, idx, refs = fit_problem
    native.knm_storage = "u24"
    Xd = X16.cuda()
    models = [_estimator(idx).fit(Xd, torch.from_numpy(v)) for v in (y, -y)]
    head = OnlineBoxPredictor(classifiers=models, regressors=None, stats=None)
    s = head._scores(native.features(Xd[:300]), 300)
    assert head._cls_cache[0].b16 and head._cls_cache[0].P is None
    for c, m in enumerate(models):
        own = m.predict(Xd[:300]).cpu().numpy()[:, 0]
        assert np.abs(s[:, c].cpu().numpy() - own).max() < 1e-4 * max(1.0, np.abs(own).max())


# ------------------------------------------------------------------------------------------------ 6. the 16-bit path ran
def test_it_is_the_16bit_path_that_runs(be, native):
    from odx import hip
    for name in NEW_ENTRIES:
        assert name in hip.SIGNATURES and getattr(be.lib, name) is not None
    rng = np.random.default_rng(1)
    X, _ = rows16(rng, 600, 128, torch.bfloat16)
    Z, _ = rows16(rng, 300, 128, torch.bfloat16)
    Xd, Zd = X.cuda(), Z.cuda()
    native.pin_gauss_tile(256)
    F, Zf = native.features(Xd), native.features(Zd)
    assert F.b16 and F.P is None and F.meta is None and F.X.dtype == torch.bfloat16 and F.sq.dtype == torch.float32
    assert F.X.data_ptr() == Xd.data_ptr()                        # D % 64 == 0, rows back to back: adopted, not copied
    called = _spy(native, ("odx_gauss_knm_b16_store", "odx_gauss_mmv_b16", "odx_gauss_mmvn_b16", "odx_split_f16", "odx_split_f16_premax"))
    try:
        native.knm_rhs(F, Zf, 10.0, torch.ones(600, dtype=torch.float64, device="cuda"))
        V = torch.from_numpy(rng.standard_normal((300, 3))).cuda()
        native.mmv(F, Zf, 10.0, V)
        native.mmv(F, Zf, 10.0, V, torch.tensor([[0, 300], [10, 200], [5, 5]], dtype=torch.int32))
    finally:
        native.lib = called.lib
    assert called == ["odx_gauss_knm_b16_store", "odx_gauss_mmvn_b16", "odx_gauss_mmv_b16"]
    assert F.P is None and Zf.P is None and F.f32 is None and Zf.f32 is None
    # the switch off: today's f32 Features, packed by the first Gaussian call
    native.native16 = False
    F = native.features(Xd)
    assert not F.b16 and F.X.dtype == torch.float32 and F.meta is not None
    native.knm_rhs(F, native.features(Zd), 10.0, torch.ones(600, dtype=torch.float64, device="cuda"))
    assert F.P is not None
