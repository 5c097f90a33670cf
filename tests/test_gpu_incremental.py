"""Incremental FALKON on the GPU: odx_knm_gram_f64 and odx_symvn_f64 by ctypes against extended-precision evaluations under
rounding-error bounds, the backend wrappers' refusals, and odx.IncrementalFalkon end to end against oracle/falkon_ref in f64 on
the rows the statistics hold."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.matern_ref import radial_kernel  # noqa: E402
from tests.synth import blob_problem, centres  # noqa: E402

U = 2.0 ** -53
ODX_ERR_INVALID = -1
NAN = float("nan")


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


# ------------------------------------------------------------------ A. odx_knm_gram_f64
def _gram_inputs(n, M):
    """K, w, y, G0, b0 with NaN in every cell the kernel must not use: K's pad columns, the entries of w and y past n, G0's pad
    columns and rows past M.  G0 is symmetric (a Gram being accumulated)."""
    rng = np.random.default_rng(1000 * n + M)
    ldk, ldg = (M + 3) // 4 * 4 + 4, M + 3
    K = np.full((max(n, 1), ldk), np.nan, dtype=np.float32)
    K[:n, :M] = rng.uniform(-1.0, 1.0, (n, M)).astype(np.float32)
    K = K[:n]
    w = np.full(n + 3, np.nan)
    y = np.full(n + 3, np.nan)
    w[:n] = rng.standard_normal(n)
    y[:n] = rng.standard_normal(n)
    G0 = np.full((M + 2, ldg), np.nan)
    A = rng.standard_normal((M, M))
    G0[:M, :M] = A + A.T
    b0 = np.full(M + 3, np.nan)
    b0[:M] = rng.standard_normal(M)
    return K, w, y, G0, b0


def _gram_call(be, dK, ldk, n, M, w, y, beta, G, ldg, b):
    rc = be.lib.odx_knm_gram_f64(_p(dK), ldk, n, M, _p(w), _p(y), float(beta), _p(G), ldg, _p(b), be._stream())
    assert rc == 0, be.lib.odx_last_error_string()


def _start(G0, b0, beta):
    """Device copies of the accumulators a call starts from; beta == 0: NaN everywhere (never read)."""
    G = torch.from_numpy(np.full_like(G0, np.nan) if beta == 0.0 else G0.copy()).cuda()
    b = torch.from_numpy(np.full_like(b0, np.nan) if beta == 0.0 else b0.copy()).cuda()
    return G, b


# Workgroup x of knm_gram_kernel takes tile row bi = 8 (local / tiles_n) + xcd and tile column local % tiles_n (local = x >> 3,
# xcd = x & 7; 128-row, 64-column tiles; grid 8 ceil(tiles_m / 8) tiles_n).  Up to M = 1024 the round local / tiles_n is 0.  The
# smallest shapes at which the rest of that mapping runs:
#   (1, 1025)   9 tile rows: bi = 8 is the first of round 1, on XCD 0, with one valid row (the half tile j0 = 1088 lies past M
#               and returns); XCD slots 1 .. 7 of round 1 return; one k-tile of one row
#   (33, 1025)  the same with two k-tiles, the second of one row
#   (33, 1089)  M = 1024 + 65: bi = 8 has its diagonal tile and its half tile j0 = i0 + 64, the latter one column wide
#   (40, 1153)  M = 9 x 128 + 1, 10 tile rows: round 1 on XCDs 0 and 1, bi = 8 full, bi = 9 one row
#   (33, 2113)  M = 16 x 128 + 65, 17 tile rows: round 2 (bi = 16, XCD 0) with a one-column half tile; round 1 on all eight XCDs
# A beta = 0 call starts from NaN everywhere, so a tile nobody visits fails isfinite and one stored elsewhere fails the bound.
GRAM_SHAPES = [(n, M) for M in (1, 7, 63, 65, 129, 257) for n in (1, 31, 33, 300)]
GRAM_SHAPES_PAST_ONE_ROUND = [(1, 1025), (33, 1025), (33, 1089), (40, 1153), (33, 2113)]


@pytest.mark.parametrize("n,M", GRAM_SHAPES + GRAM_SHAPES_PAST_ONE_ROUND)
def test_gram_kernel(be, n, M):
    """G and b against a longdouble evaluation under 2 (n + 4) u (|beta G0| + sum_r |w K K|) per entry (the gamma bound of an
    (n + 1)-term sum with one pre-rounded factor), for beta in {0, 1, 0.5}; G == G' bit for bit; nothing written outside
    M x M; the same bits twice; w = NULL is a vector of ones bit for bit; a row sub-block is that block."""
    K, w, y, G0, b0 = _gram_inputs(n, M)
    ldk, ldg = K.shape[1], G0.shape[1]
    Kx, wx, yx = K[:, :M].astype(np.longdouble), w[:n].astype(np.longdouble), y[:n].astype(np.longdouble)
    S = (wx[:, None] * Kx).T @ Kx
    Sabs = (np.abs(wx)[:, None] * np.abs(Kx)).T @ np.abs(Kx)
    sb = Kx.T @ (wx * yx)
    sbabs = np.abs(Kx).T @ np.abs(wx * yx)
    dK, dw, dy = torch.from_numpy(K).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(y).cuda()
    for beta in (0.0, 1.0, 0.5):
        G, b = _start(G0, b0, beta)
        _gram_call(be, dK, ldk, n, M, dw, dy, beta, G, ldg, b)
        Gh, bh = G.cpu().numpy(), b.cpu().numpy()
        base = 0.0 if beta == 0.0 else beta * G0[:M, :M].astype(np.longdouble)
        baseb = 0.0 if beta == 0.0 else beta * b0[:M].astype(np.longdouble)
        bar = (2.0 * (n + 4) * U * (np.abs(base) + Sabs)).astype(np.float64)
        barb = (2.0 * (n + 4) * U * (np.abs(baseb) + sbabs)).astype(np.float64)
        err = np.abs(Gh[:M, :M].astype(np.longdouble) - (base + S)).astype(np.float64)
        errb = np.abs(bh[:M].astype(np.longdouble) - (baseb + sb)).astype(np.float64)
        print("n %d M %d beta %g: G max err / bar %.3f, b %.3f" % (n, M, beta, float((err / bar).max()), float((errb / barb).max())))
        assert np.isfinite(Gh[:M, :M]).all() and (err <= bar).all(), float((err / bar).max())
        assert np.isfinite(bh[:M]).all() and (errb <= barb).all(), float((errb / barb).max())
        assert np.array_equal(Gh[:M, :M], Gh[:M, :M].T), "G is not its transpose bit for bit"
        assert np.isnan(Gh[:M, M:]).all() and np.isnan(Gh[M:]).all() and np.isnan(bh[M:]).all(), "written outside M x M"
        G2, b2 = _start(G0, b0, beta)
        _gram_call(be, dK, ldk, n, M, dw, dy, beta, G2, ldg, b2)
        assert np.array_equal(G2.cpu().numpy()[:M, :M], Gh[:M, :M]) and np.array_equal(b2.cpu().numpy()[:M], bh[:M]), "two calls differ"
    # without y and b: the same G
    G3, _ = _start(G0, b0, 0.5)
    _gram_call(be, dK, ldk, n, M, dw, None, 0.5, G3, ldg, None)
    assert np.array_equal(G3.cpu().numpy()[:M, :M], Gh[:M, :M])
    # w = NULL against ones
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    Ga, ba = _start(G0, b0, 0.0)
    Gb, bb = _start(G0, b0, 0.0)
    _gram_call(be, dK, ldk, n, M, None, dy, 0.0, Ga, ldg, ba)
    _gram_call(be, dK, ldk, n, M, ones, dy, 0.0, Gb, ldg, bb)
    assert torch.equal(Ga[:M, :M], Gb[:M, :M]) and torch.equal(ba[:M], bb[:M]), "w = NULL is not a vector of ones"
    # a row sub-block (a view into the block) against a copy of those rows
    lo, hi = (37, 201) if n >= 201 else (min(5, n - 1), n)
    sub = dK[lo:hi].clone()
    Gs, bs = _start(G0, b0, 0.0)
    Gc, bc = _start(G0, b0, 0.0)
    _gram_call(be, dK[lo:], ldk, hi - lo, M, dw[lo:], dy[lo:], 0.0, Gs, ldg, bs)
    _gram_call(be, sub, ldk, hi - lo, M, dw[lo:hi].clone(), dy[lo:hi].clone(), 0.0, Gc, ldg, bc)
    assert torch.equal(Gs[:M, :M], Gc[:M, :M]) and torch.equal(bs[:M], bc[:M]), "a row sub-block gives other bits"


def test_gram_contract(be):
    """n <= 0 only scales by beta (nothing at all for beta == 1), M <= 0 does nothing; bad alignment, leading dimensions and y
    without b are ODX_ERR_INVALID and write nothing."""
    n, M = 70, 66
    K, w, y, G0, b0 = _gram_inputs(n, M)
    ldk, ldg = K.shape[1], G0.shape[1]
    dK, dw, dy = torch.from_numpy(K).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(y).cuda()
    fn, s = be.lib.odx_knm_gram_f64, be._stream()

    def same(a, b):
        return np.array_equal(a, b, equal_nan=True)

    for nn in (0, -3):
        G, b = _start(G0, b0, 1.0)
        assert fn(_p(dK), ldk, nn, M, _p(dw), _p(dy), 1.0, _p(G), ldg, _p(b), s) == 0
        assert same(G.cpu().numpy(), G0) and same(b.cpu().numpy(), b0)
        assert fn(None, 0, nn, M, None, _p(dy), 0.5, _p(G), ldg, _p(b), s) == 0
        Gh, bh = G.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(Gh[:M, :M], 0.5 * G0[:M, :M]) and np.array_equal(bh[:M], 0.5 * b0[:M])
        assert np.isnan(Gh[:M, M:]).all() and np.isnan(Gh[M:]).all() and np.isnan(bh[M:]).all()
        G, b = _start(G0, b0, 0.0)
        assert fn(None, 0, nn, M, None, _p(dy), 0.0, _p(G), ldg, _p(b), s) == 0
        assert bool((G[:M, :M] == 0.0).all()) and bool((b[:M] == 0.0).all()) and bool(torch.isnan(G[:M, M:]).all())
    G, b = _start(G0, b0, 1.0)
    for MM in (0, -1):
        assert fn(_p(dK), ldk, n, MM, _p(dw), _p(dy), 0.0, _p(G), ldg, _p(b), s) == 0
    flat = dK.view(-1)
    assert fn(_p(flat[1:]), ldk, n - 1, M, _p(dw), _p(dy), 1.0, _p(G), ldg, _p(b), s) == ODX_ERR_INVALID     # K off a 16-byte boundary
    assert fn(_p(dK), ldk - 2, n, M, _p(dw), _p(dy), 1.0, _p(G), ldg, _p(b), s) == ODX_ERR_INVALID           # ldk % 4 != 0
    assert fn(_p(dK), 64, n, M, _p(dw), _p(dy), 1.0, _p(G), ldg, _p(b), s) == ODX_ERR_INVALID                # ldk < M
    assert fn(_p(dK), ldk, n, M, _p(dw), _p(dy), 1.0, _p(G), M - 1, _p(b), s) == ODX_ERR_INVALID             # ldg < M
    assert fn(_p(dK), ldk, n, M, _p(dw), _p(dy), 1.0, _p(G), ldg, None, s) == ODX_ERR_INVALID                # y without b
    assert fn(_p(dK), ldk, n, M, _p(dw), None, 1.0, _p(G), ldg, _p(b), s) == ODX_ERR_INVALID                 # b without y
    assert fn(_p(dK), ldk, n, M, _p(dw), _p(dy), 1.0, None, ldg, _p(b), s) == ODX_ERR_INVALID                # no G
    assert same(G.cpu().numpy(), G0) and same(b.cpu().numpy(), b0)


def test_gram_over_row_halves_agrees_to_rounding(be):
    """Two calls over row halves (the second accumulating) against one call: equal to the bound of the sums, not bit for bit.
    At M = 1089 the second call reads and adds to the tiles of the second round of tile rows (bi = 8, its half tile included)."""
    for n, M, h in ((300, 129, 157), (65, 1089, 33)):
        K, w, y, G0, b0 = _gram_inputs(n, M)
        ldk, ldg = K.shape[1], G0.shape[1]
        dK, dw, dy = torch.from_numpy(K).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(y).cuda()
        G1, b1 = _start(G0, b0, 0.0)
        _gram_call(be, dK, ldk, n, M, dw, dy, 0.0, G1, ldg, b1)
        G2, b2 = _start(G0, b0, 0.0)
        _gram_call(be, dK, ldk, h, M, dw, dy, 0.0, G2, ldg, b2)
        _gram_call(be, dK[h:], ldk, n - h, M, dw[h:], dy[h:], 1.0, G2, ldg, b2)
        Sabs = (np.abs(w[:n])[:, None] * np.abs(K[:, :M]).astype(np.float64)).T @ np.abs(K[:, :M]).astype(np.float64)
        err = np.abs(G1.cpu().numpy()[:M, :M] - G2.cpu().numpy()[:M, :M])
        bar = 4.0 * (n + 4) * U * Sabs
        print("n %d M %d halves at %d: max err / bar %.3f" % (n, M, h, float((err / bar).max())))
        assert np.isfinite(G2.cpu().numpy()[:M, :M]).all() and (err <= bar).all(), (n, M)
        assert torch.equal(G2[:M, :M], G2[:M, :M].t())


# ------------------------------------------------------------------ B. odx_symvn_f64
# (M, nv) past M = 1000: 1025 (257 row blocks of four rows, the last with one row; the odd last element) and 4099 (1025 row
# blocks, 257 workgroups, 32 steps of the 16-byte loop and a ragged 33rd), for each of the three instantiations
SYMVN_SHAPES = [(M, nv) for nv in (1, 2, 3, 8) for M in (1, 2, 63, 129, 1000)] + [(M, nv) for nv in (1, 3, 8) for M in (1025, 4099)]


@pytest.mark.parametrize("M,nv", SYMVN_SHAPES)
def test_symvn(be, M, nv):
    """Y against a longdouble evaluation under 2 (M + 2) u |alpha| (|G| |x|); NaN in the pad columns of G, X and Y (never read,
    never written); alpha applied once; the same bits twice; with two vectors, each column agrees with its own call."""
    rng = np.random.default_rng(10 * M + nv)
    ldg, ldx, ldy = M + M % 2 + 2, M + M % 2 + 4, M + 3
    G = np.full((M, ldg), np.nan)
    G[:, :M] = rng.standard_normal((M, M))
    X = np.full((nv, ldx), np.nan)
    X[:, :M] = rng.standard_normal((nv, M))
    dG, dX = torch.from_numpy(G).cuda(), torch.from_numpy(X).cuda()
    Gx, Xx = G[:, :M].astype(np.longdouble), X[:, :M].astype(np.longdouble)
    ref = Xx @ Gx.T
    mag = (np.abs(Xx) @ np.abs(Gx).T).astype(np.float64)

    def call(x, k, alpha):
        Y = torch.full((k, ldy), NAN, dtype=torch.float64, device="cuda")
        rc = be.lib.odx_symvn_f64(_p(dG), ldg, M, k, _p(x), ldx, float(alpha), _p(Y), ldy, be._stream())
        assert rc == 0, be.lib.odx_last_error_string()
        Y = Y.cpu().numpy()
        assert np.isnan(Y[:, M:]).all(), "written past column M"
        return Y[:, :M]

    y1 = call(dX, nv, 1.0)
    err = np.abs(y1.astype(np.longdouble) - ref).astype(np.float64)
    bar = 2.0 * (M + 2) * U * mag
    print("M %d nv %d: max err / bar %.3f" % (M, nv, float((err / np.maximum(bar, 1e-300)).max())))
    assert np.isfinite(y1).all() and (err <= bar).all()
    alpha = -0.75
    ya = call(dX, nv, alpha)
    assert np.array_equal(ya, alpha * y1), "alpha is not applied once, to the finished sum"
    assert np.array_equal(call(dX, nv, 1.0), y1), "two calls differ"
    if nv == 2:
        for q in range(2):
            yq = call(dX[q], 1, 1.0)
            assert (np.abs(yq[0] - y1[q]) <= bar[q]).all()


def test_symvn_contract(be):
    M = 10
    G = torch.zeros((M, 12), dtype=torch.float64, device="cuda")
    X = torch.zeros((9, 12), dtype=torch.float64, device="cuda")
    Y = torch.full((9, 12), -7.0, dtype=torch.float64, device="cuda")
    fn, s = be.lib.odx_symvn_f64, be._stream()
    assert fn(_p(G), 12, 0, 1, _p(X), 12, 1.0, _p(Y), 12, s) == 0
    for nv in (0, 9):
        assert fn(_p(G), 12, M, nv, _p(X), 12, 1.0, _p(Y), 12, s) == ODX_ERR_INVALID
    assert fn(_p(G), 11, M, 1, _p(X), 12, 1.0, _p(Y), 12, s) == ODX_ERR_INVALID             # odd ldg
    assert fn(_p(G), 8, M, 1, _p(X), 12, 1.0, _p(Y), 12, s) == ODX_ERR_INVALID              # ldg < M
    assert fn(_p(G.view(-1)[1:]), 12, M - 1, 1, _p(X), 12, 1.0, _p(Y), 12, s) == ODX_ERR_INVALID
    assert fn(_p(G), 12, M, 2, _p(X), 8, 1.0, _p(Y), 12, s) == ODX_ERR_INVALID              # rows of X closer than M
    assert fn(_p(G), 12, M, 1, _p(X), 12, 1.0, _p(X), 12, s) == ODX_ERR_INVALID             # Y is X
    assert fn(_p(G), 12, M, 3, _p(X), 12, 1.0, _p(X[2]), 12, s) == ODX_ERR_INVALID          # Y starts inside X
    assert fn(_p(G), 12, M, 2, _p(X[1]), 12, 1.0, _p(X), 12, s) == ODX_ERR_INVALID          # X starts inside Y
    assert fn(_p(G), 12, M, 1, _p(X), 12, 1.0, _p(X.view(-1)[M - 1:]), 12, s) == ODX_ERR_INVALID   # the last element of X
    assert fn(_p(G), 12, M, 2, _p(X), 12, 1.0, _p(X[2]), 12, s) == 0                        # behind X: fine
    X.zero_()
    assert bool((Y == -7.0).all())


def test_backend_wrappers(be):
    """HipBackend.knm_gram / symv: fresh statistics, accumulation, more than 8 vectors, and the refusals by name."""
    import odx
    X, y, rng = blob_problem(500, 40, seed=3)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, np.arange(70))
    K = be.knm_f32(F, Zf, 6.0)
    yv = be.vec(y)
    G, b = be.knm_gram(K, y=yv)
    Kd = K.dense().double()
    ref = Kd.t() @ Kd
    assert tuple(G.shape) == (70, 70) and float((G - ref).abs().max()) < 1e-10 * float(ref.abs().max())
    assert float((b - Kd.t() @ yv).abs().max()) < 1e-10 * float(b.abs().max())
    G2, b2 = be.knm_gram(K.rows(0, 200), y=yv[:200])
    be.knm_gram(K.rows(200, 500), y=yv[200:], G=G2, b=b2)
    assert float((G2 - G).abs().max()) < 1e-10 * float(ref.abs().max()) and torch.equal(G2, G2.t())
    V = torch.zeros((11, 70), dtype=torch.float64, device="cuda")
    V.copy_(torch.from_numpy(rng.standard_normal((11, 70))))
    out = be.symv(G, V, alpha=0.5)
    assert float((out - 0.5 * V @ G.t()).abs().max()) < 1e-10 * float(out.abs().max())
    fake = K.rows(0, 10)
    fake.fmt = "u24"
    with pytest.raises(ValueError, match="f32-format"):
        be.knm_gram(fake)
    fake.fmt, fake.cmap = "f32", object()
    with pytest.raises(ValueError, match="column map"):
        be.knm_gram(fake)
    with pytest.raises(ValueError, match="together"):
        be.knm_gram(K, y=yv, G=G)
    with pytest.raises(ValueError, match="must not overlap"):
        be.symv(G, V, out=V)
    with pytest.raises(ValueError, match="must not overlap"):
        be.symv(G, V[:3], out=V[2:5])
    with pytest.raises(ValueError):
        be.symv(G, V.float())
    assert odx.IncrementalFalkon is not None


# ------------------------------------------------------------------ C. odx.IncrementalFalkon end to end
# The last shape has 9 tile rows of 128 centres, a second round of odx_knm_gram_f64's tile rows.  It is benign enough for the
# parity bars: oracle/falkon_ref alone, iterating on a K block evaluated in f32 (entries within 9.7e-6 of the f64 ones) instead of
# the f64 block, gives alpha within 5.8e-7 relative and the scores within 3.9e-6 of the f64 fit, alpha within 3.9e-7 after the
# removal (with the f64 entries rounded to f32: 5.3e-10, 1.8e-9, 7.1e-10) — more than an order of magnitude inside 1e-4.
SHAPES = [(777, 129, 36, 5.0, 1e-3), (1500, 257, 70, 5.0, 1e-4), (3000, 300, 1024, 15.0, 1e-5), (2600, 1100, 36, 5.0, 1e-3)]
_refs = {}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _reference(fr, shape, kernel):
    """(X, y, Z, cuts, alpha on all rows, scores of all rows, alpha without the last batch) in f64: computed once per shape
    and kernel, shared, never changed."""
    key = (shape, repr(kernel))
    if key not in _refs:
        n, M, D, sigma, lam = shape
        X, y, rng = blob_problem(n, D, seed=n + M)
        Z = np.ascontiguousarray(X[centres(y, M, rng)])
        cuts = (0, n // 2 + 7, n // 2 + 7 + n // 5, n)
        Xd, yd, Zd = X.astype(np.float64), y.astype(np.float64), Z.astype(np.float64)
        kw = dict(maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        a_all = fr.falkon_fit_centers(Xd, yd, Zd, kernel, lam, n, **kw)[0]
        scores = fr.falkon_predict(Xd, Zd, a_all, kernel)
        a_rest = fr.falkon_fit_centers(Xd[:cuts[2]], yd[:cuts[2]], Zd, kernel, lam, cuts[2], **kw)[0]
        _refs[key] = (X, y, Z, cuts, a_all[:, 0], scores, a_rest[:, 0])
    return _refs[key]


def _run(est, X, y, cuts):
    for i in range(3):
        est.partial_fit(torch.from_numpy(X[cuts[i]:cuts[i + 1]]), torch.from_numpy(y[cuts[i]:cuts[i + 1]])[:, None])
    return est


@pytest.mark.parametrize("chunk_rows", [None, 256], ids=["whole", "chunks256"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d" % s[:2])
def test_incremental_fit_is_the_oracle_on_the_rows_held(be, shape, chunk_rows):
    """Three uneven partial_fit calls: alpha within 1e-4 relative and the scores within 1e-4 absolute of the f64 oracle on all
    rows; after remove of the last batch alpha within 1e-4 relative of the oracle on the remaining rows."""
    import odx
    from oracle import falkon_ref as fr
    n, M, D, sigma, lam = shape
    X, y, Z, cuts, a_all, scores, a_rest = _reference(fr, shape, sigma)
    est = _run(odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, centres=torch.from_numpy(Z), chunk_rows=chunk_rows), X, y, cuts)
    assert est.n_seen_ == n and tuple(est.alpha_.shape) == (M, 1) and torch.equal(est.gram_[:, :M], est.gram_[:, :M].t())
    r = _rel(est.alpha_.cpu().numpy(), a_all)
    s = float(np.abs(est.predict(torch.from_numpy(X)).cpu().numpy() - scores).max())
    print("n %d M %d: alpha rel err %.2e, score err %.2e" % (n, M, r, s))
    assert r < 1e-4, r
    assert s < 1e-4, s
    f = est.as_falkon()
    assert torch.equal(f.predict(torch.from_numpy(X[:100])), est.predict(torch.from_numpy(X[:100])).cpu())
    est.remove(torch.from_numpy(X[cuts[2]:]), torch.from_numpy(y[cuts[2]:])[:, None])
    r = _rel(est.alpha_.cpu().numpy(), a_rest)
    print("n %d M %d: after remove alpha rel err %.2e" % (n, M, r))
    assert est.n_seen_ == cuts[2] and r < 1e-4, r


def test_incremental_fit_matern(be, monkeypatch):
    import odx
    from oracle import falkon_ref as fr
    monkeypatch.setattr(fr, "gaussian_kernel", radial_kernel)
    shape = SHAPES[1]
    n, M, D, sigma, lam = shape
    k = odx.MaternKernel(5.0, 2.5)
    X, y, Z, cuts, a_all, scores, a_rest = _reference(fr, shape, k)
    est = _run(odx.IncrementalFalkon(k, lam, centres=torch.from_numpy(Z)), X, y, cuts)
    r = _rel(est.alpha_.cpu().numpy(), a_all)
    s = float(np.abs(est.predict(torch.from_numpy(X)).cpu().numpy() - scores).max())
    print("matern 5/2: alpha rel err %.2e, score err %.2e" % (r, s))
    assert r < 1e-4, r
    assert s < 1e-4, s
    est.remove(torch.from_numpy(X[cuts[2]:]), torch.from_numpy(y[cuts[2]:])[:, None])
    r = _rel(est.alpha_.cpu().numpy(), a_rest)
    print("matern 5/2: after remove alpha rel err %.2e" % r)
    assert r < 1e-4, r


def test_selected_centres_new_penalty_and_pickle(be):
    """Centres drawn from the first batch as InCoreFalkon.fit draws them; solve(penalty) against a full fit at that penalty on the
    same centres; a pickled model goes on where the original does."""
    import pickle
    import odx
    n, M, D, sigma, lam = 1200, 150, 48, 6.0, 1e-4
    X, y, _ = blob_problem(n, D, seed=77)
    Xt, Yt = torch.from_numpy(X), torch.from_numpy(y)[:, None]
    torch.manual_seed(9)
    ref = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma), penalty=lam, M=M).fit(Xt[:700], Yt[:700])
    state = torch.get_rng_state().clone()
    torch.manual_seed(9)
    est = odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, M=M).partial_fit(Xt[:700], Yt[:700])
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(est.ny_points_, ref.ny_points_)
    assert _rel(est.alpha_.cpu().numpy(), ref.alpha_.cpu().numpy()) < 1e-5
    back = pickle.loads(pickle.dumps(est))
    assert "_P" not in back.__dict__ and "_zf" not in back.__dict__
    for m in (est, back):
        m.partial_fit(Xt[700:], Yt[700:], solve=False)
        m.solve(penalty=1e-3)
    assert torch.equal(back.alpha_, est.alpha_)

    class Fixed:
        def select(self, Xs, Ys):
            return est.ny_points_
    full = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma), penalty=1e-3, M=M, center_selection=Fixed()).fit(Xt, Yt)
    r = _rel(est.alpha_.cpu().numpy(), full.alpha_.cpu().numpy())
    print("new penalty against a full fit: %.2e" % r)
    assert r < 1e-5, r
