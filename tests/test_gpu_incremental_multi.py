"""Several outputs and lambda paths from one set of incremental statistics, on the GPU: odx_knm_gram_rhsn_f64 by ctypes against
an extended-precision evaluation under a rounding-error bound and against odx_knm_gram_f64 bit for bit, its contract, and
odx.IncrementalFalkon(outputs=T) / solve_path end to end against oracle/falkon_ref in f64 on a label matrix."""
import ctypes
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.matern_ref import radial_kernel  # noqa: E402
from tests.test_incremental_multi_host import PENALTIES, labels, oracle_alphas  # noqa: E402
from tests.test_incremental_host import problem, rel  # noqa: E402

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


# ------------------------------------------------------------------ A. odx_knm_gram_rhsn_f64
def _inputs(n, M, nt):
    """K, w, Y, G0, B0 with NaN in every cell the kernel must not use: K's pad columns, w past n, Y's pad columns and its rows
    past n, G0 outside M x M, B0 outside nt x M.  G0 is symmetric (a Gram being accumulated)."""
    rng = np.random.default_rng(100000 * nt + 1000 * n + M)
    ldk, ldg, ldy, ldb = (M + 3) // 4 * 4 + 4, M + 3, (nt + 1) // 2 * 2 + 2, M + 3
    K = np.full((n, ldk), np.nan, dtype=np.float32)
    K[:, :M] = rng.uniform(-1.0, 1.0, (n, M)).astype(np.float32)
    w = np.full(n + 3, np.nan)
    w[:n] = rng.standard_normal(n)
    Y = np.full((n + 2, ldy), np.nan)
    Y[:n, :nt] = rng.standard_normal((n, nt))
    G0 = np.full((M + 2, ldg), np.nan)
    A = rng.standard_normal((M, M))
    G0[:M, :M] = A + A.T
    B0 = np.full((nt + 1, ldb), np.nan)
    B0[:nt, :M] = rng.standard_normal((nt, M))
    return K, w, Y, G0, B0


def _call(be, K, ldk, n, M, w, Y, ldy, nt, beta, G, ldg, B, ldb):
    rc = be.lib.odx_knm_gram_rhsn_f64(_p(K), ldk, n, M, _p(w), _p(Y), ldy, nt, float(beta), _p(G), ldg, _p(B), ldb, be._stream())
    assert rc == 0, be.lib.odx_last_error_string()


def _start(G0, B0, beta):
    """Device copies of the accumulators a call starts from; beta == 0: NaN everywhere (never read)."""
    G = torch.from_numpy(np.full_like(G0, np.nan) if beta == 0.0 else G0.copy()).cuda()
    B = torch.from_numpy(np.full_like(B0, np.nan) if beta == 0.0 else B0.copy()).cuda()
    return G, B


# Workgroup x of knm_gram_rhsn_kernel takes tile column bj = local % tiles_all (local = x >> 3, xcd = x & 7; tiles_all =
# ceil(M / 64) + ceil(nt / 64); grid 8 ceil(tiles_m / 8) tiles_all).  Tile columns below ceil(M / 64) are odx_knm_gram_f64's G
# tiles, of tile row 8 (local / tiles_all) + xcd; tile column ceil(M / 64) + c is the right-hand-side tile of 128 columns of K
# against label columns 64 c .. 64 c + 63, of tile row 8 (local / tiles_all) + 7 - xcd.  What each shape runs:
#   (1, 1, 1)        one G tile, one right-hand-side tile with one output; one k-tile of one row
#   (33, 7, 2)       a pair load of two label columns; a second k-tile of one row
#   (31, 63, 63)     one right-hand-side tile one column short of full: an odd nt, the single-element tail of a pair load
#   (33, 65, 65)     a second right-hand-side tile column with ONE label column (the tail again); K column 64 is the first of
#                    the second G tile column
#   (300, 129, 64)   exactly one full right-hand-side tile column; two tile rows, the second with one K column; ten k-tiles
#   (300, 257, 130)  three right-hand-side tile columns, the last two label columns wide; three tile rows
#   (33, 129, 1)     one label column against two tile rows
#   (1, 257, 65)     one row of K: three tile rows by two right-hand-side tile columns
#   (33, 1089, 65)   nine tile rows: bi = 8 is round 1 of the tile map, where local / tiles_all must use tiles_all = 20 and not
#                    the 18 G columns; its G tiles run on XCD 0, its two right-hand-side tiles (65 K columns) on XCD 7
#   (40, 1153, 2)    ten tile rows: round 1 has G tiles on XCDs 0 and 1 and right-hand-side tiles on XCDs 7 and 6, bi = 9 with
#                    one K column
# A beta = 0 call starts from NaN everywhere, so a tile nobody visits fails isfinite and one stored elsewhere fails the bound.
RHSN_SHAPES = [(1, 1, 1), (33, 7, 2), (31, 63, 63), (33, 65, 65), (300, 129, 64), (300, 257, 130), (33, 129, 1), (1, 257, 65),
               (33, 1089, 65), (40, 1153, 2)]


@pytest.mark.parametrize("n,M,nt", RHSN_SHAPES)
def test_gram_rhsn_kernel(be, n, M, nt):
    """B against a longdouble evaluation under 2 (n + 4) u (|beta B0| + sum_r |K| |w Y|) per entry (the gamma bound of an
    (n + 1)-term sum with one pre-rounded factor: test_gram_kernel's), for beta in {0, 1, 0.5}; G bit for bit odx_knm_gram_f64's
    from the same start, and its own transpose; NaN left in every poisoned cell; the same bits twice; a column alone at nt = 1
    is its row of the full call bit for bit; w = NULL is a vector of ones; a row sub-block is that block; and at nt = 1 B agrees
    with odx_knm_gram_f64's b to rounding."""
    K, w, Y, G0, B0 = _inputs(n, M, nt)
    ldk, ldg, ldy, ldb = K.shape[1], G0.shape[1], Y.shape[1], B0.shape[1]
    Kx, wx, Yx = K[:, :M].astype(np.longdouble), w[:n].astype(np.longdouble), Y[:n, :nt].astype(np.longdouble)
    wy = (w[:n, None] * Y[:n, :nt]).astype(np.longdouble)             # (w y is rounded once, by the kernel too)
    S = (wx[:, None] * Yx).T @ Kx                                      # (nt, M)
    Sabs = np.abs(wy).T @ np.abs(Kx)
    dK, dw, dY = torch.from_numpy(K).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(Y).cuda()
    for beta in (0.0, 1.0, 0.5):
        G, B = _start(G0, B0, beta)
        _call(be, dK, ldk, n, M, dw, dY, ldy, nt, beta, G, ldg, B, ldb)
        Gh, Bh = G.cpu().numpy(), B.cpu().numpy()
        base = 0.0 if beta == 0.0 else beta * B0[:nt, :M].astype(np.longdouble)
        bar = (2.0 * (n + 4) * U * (np.abs(base) + Sabs)).astype(np.float64)
        err = np.abs(Bh[:nt, :M].astype(np.longdouble) - (base + S)).astype(np.float64)
        print("n %d M %d nt %d beta %g: B max err / bar %.3f" % (n, M, nt, beta, float((err / bar).max())))
        assert np.isfinite(Bh[:nt, :M]).all() and (err <= bar).all(), float((err / bar).max())
        Gr, _ = _start(G0, B0, beta)
        rc = be.lib.odx_knm_gram_f64(_p(dK), ldk, n, M, _p(dw), None, float(beta), _p(Gr), ldg, None, be._stream())
        assert rc == 0, be.lib.odx_last_error_string()
        assert np.array_equal(Gh, Gr.cpu().numpy(), equal_nan=True), "G is not odx_knm_gram_f64's, bit for bit"
        assert np.isfinite(Gh[:M, :M]).all() and np.array_equal(Gh[:M, :M], Gh[:M, :M].T), "G is not its transpose bit for bit"
        assert np.isnan(Gh[:M, M:]).all() and np.isnan(Gh[M:]).all(), "G written outside M x M"
        assert np.isnan(Bh[:nt, M:]).all() and np.isnan(Bh[nt:]).all(), "B written outside nt x M"
        G2, B2 = _start(G0, B0, beta)
        _call(be, dK, ldk, n, M, dw, dY, ldy, nt, beta, G2, ldg, B2, ldb)
        assert np.array_equal(G2.cpu().numpy(), Gh, equal_nan=True) and np.array_equal(B2.cpu().numpy(), Bh, equal_nan=True), "two calls differ"
    # beta = 0 from here on
    G, B = _start(G0, B0, 0.0)
    _call(be, dK, ldk, n, M, dw, dY, ldy, nt, 0.0, G, ldg, B, ldb)
    # a column alone, at nt = 1, against its row of the full call: the first and last of every block of 64, and one inside
    for t in sorted({0, 1, 31, 62, 63, 64, 65, 127, 128, nt - 1} & set(range(nt))):
        y1 = torch.full((n + 1, 2), NAN, dtype=torch.float64, device="cuda")
        y1[:n, 0] = dY[:n, t]
        G1, B1 = _start(G0, B0[:2], 0.0)
        _call(be, dK, ldk, n, M, dw, y1, 2, 1, 0.0, G1, ldg, B1, ldb)
        assert torch.equal(B1[0, :M], B[t, :M]), "row %d of B depends on the other columns" % t
        assert bool(torch.isnan(B1[1]).all()) and torch.equal(G1[:M, :M], G[:M, :M])
    # nt = 1 against odx_knm_gram_f64's b: another order of the same sum
    bg = torch.full((M + 3,), NAN, dtype=torch.float64, device="cuda")
    Gg, _ = _start(G0, B0, 0.0)
    y0 = dY[:, 0].contiguous()
    assert be.lib.odx_knm_gram_f64(_p(dK), ldk, n, M, _p(dw), _p(y0), 0.0, _p(Gg), ldg, _p(bg), be._stream()) == 0
    bar0 = (4.0 * (n + 4) * U * Sabs[0]).astype(np.float64)
    assert (np.abs(bg.cpu().numpy()[:M] - B.cpu().numpy()[0, :M]) <= bar0).all()
    # w = NULL against ones
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    Ga, Ba = _start(G0, B0, 0.0)
    Gb, Bb = _start(G0, B0, 0.0)
    _call(be, dK, ldk, n, M, None, dY, ldy, nt, 0.0, Ga, ldg, Ba, ldb)
    _call(be, dK, ldk, n, M, ones, dY, ldy, nt, 0.0, Gb, ldg, Bb, ldb)
    assert torch.equal(Ga[:M, :M], Gb[:M, :M]) and torch.equal(Ba[:nt, :M], Bb[:nt, :M]), "w = NULL is not a vector of ones"
    # a row sub-block (views into K, w and Y) against copies of those rows
    lo, hi = (37, 201) if n >= 201 else (min(5, n - 1), n)
    Gs, Bs = _start(G0, B0, 0.0)
    Gc, Bc = _start(G0, B0, 0.0)
    _call(be, dK[lo:], ldk, hi - lo, M, dw[lo:], dY[lo:], ldy, nt, 0.0, Gs, ldg, Bs, ldb)
    _call(be, dK[lo:hi].clone(), ldk, hi - lo, M, dw[lo:hi].clone(), dY[lo:hi].clone(), ldy, nt, 0.0, Gc, ldg, Bc, ldb)
    assert torch.equal(Gs[:M, :M], Gc[:M, :M]) and torch.equal(Bs[:nt, :M], Bc[:nt, :M]), "a row sub-block gives other bits"


def test_gram_rhsn_contract(be):
    """n <= 0 only scales by beta (nothing at all for beta == 1), M <= 0 does nothing; every refusal is ODX_ERR_INVALID and
    writes nothing."""
    n, M, nt = 70, 66, 5
    K, w, Y, G0, B0 = _inputs(n, M, nt)
    ldk, ldg, ldy, ldb = K.shape[1], G0.shape[1], Y.shape[1], B0.shape[1]
    dK, dw, dY = torch.from_numpy(K).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(Y).cuda()
    fn, s = be.lib.odx_knm_gram_rhsn_f64, be._stream()

    def same(a, b):
        return np.array_equal(a, b, equal_nan=True)

    for nn in (0, -3):
        G, B = _start(G0, B0, 1.0)
        assert fn(_p(dK), ldk, nn, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(B), ldb, s) == 0
        assert same(G.cpu().numpy(), G0) and same(B.cpu().numpy(), B0)
        assert fn(None, 0, nn, M, None, _p(dY), ldy, nt, 0.5, _p(G), ldg, _p(B), ldb, s) == 0
        Gh, Bh = G.cpu().numpy(), B.cpu().numpy()
        assert np.array_equal(Gh[:M, :M], 0.5 * G0[:M, :M]) and np.array_equal(Bh[:nt, :M], 0.5 * B0[:nt, :M])
        assert np.isnan(Gh[:M, M:]).all() and np.isnan(Gh[M:]).all() and np.isnan(Bh[:nt, M:]).all() and np.isnan(Bh[nt:]).all()
        G, B = _start(G0, B0, 0.0)
        assert fn(None, 0, nn, M, None, _p(dY), ldy, nt, 0.0, _p(G), ldg, _p(B), ldb, s) == 0
        assert bool((G[:M, :M] == 0.0).all()) and bool((B[:nt, :M] == 0.0).all()) and bool(torch.isnan(B[:nt, M:]).all())
    G, B = _start(G0, B0, 1.0)
    for MM in (0, -1):
        assert fn(_p(dK), ldk, n, MM, _p(dw), _p(dY), ldy, nt, 0.0, _p(G), ldg, _p(B), ldb, s) == 0
    flatK, flatY, flatB = dK.view(-1), dY.view(-1), B.view(-1)
    bad = [
        (_p(dK), ldk, n, M, _p(dw), None, ldy, nt, 1.0, _p(G), ldg, _p(B), ldb),                    # no Y
        (_p(dK), ldk, n, M, _p(dw), _p(flatY[1:]), ldy, nt, 1.0, _p(G), ldg, _p(B), ldb),           # Y off a 16-byte boundary
        (_p(dK), ldk, n, M, _p(dw), _p(dY), nt - 1, nt, 1.0, _p(G), ldg, _p(B), ldb),               # ldy < nt
        (_p(dK), ldk, n, M, _p(dw), _p(dY), nt, nt, 1.0, _p(G), ldg, _p(B), ldb),                   # ldy odd
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, None, ldb),                   # no B
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, ctypes.c_void_p(B.data_ptr() + 4), ldb),   # B off 8 bytes
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(B), M - 1),                # ldb < M
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, 0, 1.0, _p(G), ldg, _p(B), ldb),                   # nt = 0
        (_p(dK), ldk, n, M, _p(dw), _p(dY), 1026, 1025, 1.0, _p(G), ldg, _p(B), ldb),               # nt = 1025
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(G[2]), ldg),               # B inside G
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(flatB[2:]), ldg, _p(B), ldb),          # G starts inside B
        (_p(flatK[1:]), ldk, n - 1, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(B), ldb),       # K off a 16-byte boundary
        (_p(dK), ldk - 2, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(B), ldb),              # ldk % 4 != 0
        (_p(dK), 64, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(B), ldb),                   # ldk < M
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), M - 1, _p(B), ldb),                # ldg < M
        (_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, None, ldg, _p(B), ldb),                   # no G
        (None, ldk, n, M, _p(dw), _p(dY), ldy, nt, 1.0, _p(G), ldg, _p(B), ldb),                    # no K with rows
    ]
    for args in bad:
        assert fn(*args, s) == ODX_ERR_INVALID, args
    assert same(G.cpu().numpy(), G0) and same(B.cpu().numpy(), B0)
    # B right behind G's last entry is no overlap
    buf = torch.zeros(M * ldg + nt * ldb, dtype=torch.float64, device="cuda")
    assert fn(_p(dK), ldk, n, M, _p(dw), _p(dY), ldy, nt, 0.0, _p(buf), ldg, _p(buf[(M - 1) * ldg + M:]), ldb, s) == 0


def test_backend_wrapper(be):
    """HipBackend.knm_gram_multi: fresh statistics, accumulation over row halves, G the bits of knm_gram's, the refusals."""
    from tests.synth import blob_problem
    X, y, rng = blob_problem(500, 40, seed=3)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, np.arange(70))
    K = be.knm_f32(F, Zf, 6.0)
    Y = torch.zeros((500, 4), dtype=torch.float64, device="cuda")
    Y[:, :3] = torch.from_numpy(rng.standard_normal((500, 3))).cuda()
    G, B = be.knm_gram_multi(K, Y=Y[:, :3])
    Kd = K.dense().double()
    assert tuple(G.shape) == (70, 70) and tuple(B.shape) == (3, 70) and torch.equal(G, be.knm_gram(K)[0])
    ref = Y[:, :3].t() @ Kd
    assert float((B - ref).abs().max()) < 1e-10 * float(ref.abs().max())
    G2, B2 = be.knm_gram_multi(K.rows(0, 200), Y=Y[:200, :3])
    be.knm_gram_multi(K.rows(200, 500), Y=Y[200:, :3], G=G2, B=B2)
    assert float((B2 - B).abs().max()) < 1e-10 * float(ref.abs().max()) and torch.equal(G2, G2.t())
    with pytest.raises(ValueError, match="Y must be"):
        be.knm_gram_multi(K)
    with pytest.raises(ValueError, match="Y must be"):
        be.knm_gram_multi(K, Y=Y[:, :3].float())
    with pytest.raises(ValueError, match="16-byte aligned"):
        be.knm_gram_multi(K, Y=torch.zeros((500, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="together"):
        be.knm_gram_multi(K, Y=Y[:, :3], B=B)
    with pytest.raises(ValueError, match="B must be"):
        be.knm_gram_multi(K, Y=Y[:, :3], G=G, B=B[:2])
    fake = K.rows(0, 10)
    fake.fmt = "u24"
    with pytest.raises(ValueError, match="f32-format"):
        be.knm_gram_multi(fake, Y=Y[:10, :3])


# ------------------------------------------------------------------ B. odx.IncrementalFalkon(outputs=T) end to end
SMALL, LARGE = (777, 129, 36, 5.0, 1e-3), (2600, 1100, 36, 5.0, 1e-3)       # (LARGE: a second round of tile rows in both kernels)
_refs = {}


def _t(a):
    return torch.from_numpy(np.array(a))          # (a copy: the shared problem arrays are read-only)


def _reference(shape, T, kernel, lam=None):
    """(X, Y, Z, cuts, alpha (M, T) on all rows, the rows left without the middle batch, alpha on them) in f64: computed once
    per shape, T, kernel and penalty, shared, never changed."""
    key = (shape, T, repr(kernel), lam)
    if key not in _refs:
        X, y, Z, cuts = problem(shape)
        Y = labels(shape, T)
        left = np.r_[0:cuts[1], cuts[2]:len(X)]
        pen = shape[4] if lam is None else lam
        _refs[key] = (X, Y, Z, cuts, oracle_alphas(X, Y, Z, kernel, pen), left,
                      None if lam is not None else oracle_alphas(X, Y, Z, kernel, pen, left))
    return _refs[key]


def _model(shape, Z, kernel, **kw):
    import odx
    return odx.IncrementalFalkon(kernel, shape[4], centres=_t(Z), **kw)


def _feed(est, X, Y, cuts, last_only=False):
    for i in range(3):
        est.partial_fit(_t(X[cuts[i]:cuts[i + 1]]), _t((Y[cuts[i]:cuts[i + 1]])),
                        solve=not last_only or i == 2)
    return est


def _parity(est, X, Y, Z, cuts, a_all, left, a_left, kernel, tag):
    """Every column's alpha within 1e-4 relative of the oracle, the scores of every seventh row within 1e-4; after remove of the
    middle batch the same on the rows left, the scores on the batch taken out (held out by then)."""
    from oracle import falkon_ref as fr
    T = Y.shape[1]
    Zd = Z.astype(np.float64)
    r = [rel(est.alpha_[:, t].cpu().numpy(), a_all[:, t]) for t in range(T)]
    Xq = X[::7]
    s = np.abs(est.predict(_t(Xq)).cpu().numpy() - fr.falkon_predict(Xq.astype(np.float64), Zd, a_all, kernel)).max(0)
    print("%s: alpha rel err per column %s; score err %s" % (tag, " ".join("%.1e" % v for v in r), " ".join("%.1e" % v for v in s)))
    assert max(r) < 1e-4, r
    assert (s < 1e-4).all(), s
    est.remove(_t(X[cuts[1]:cuts[2]]), _t((Y[cuts[1]:cuts[2]])))
    assert est.n_seen_ == len(left)
    r = [rel(est.alpha_[:, t].cpu().numpy(), a_left[:, t]) for t in range(T)]
    Xh = X[cuts[1]:cuts[2]]
    s = np.abs(est.predict(_t(Xh)).cpu().numpy() - fr.falkon_predict(Xh.astype(np.float64), Zd, a_left, kernel)).max(0)
    print("%s after remove: alpha rel err per column %s; held-out score err %s"
          % (tag, " ".join("%.1e" % v for v in r), " ".join("%.1e" % v for v in s)))
    assert max(r) < 1e-4, r
    assert (s < 1e-4).all(), s


@pytest.mark.parametrize("chunk_rows", [None, 256], ids=["whole", "chunks256"])
@pytest.mark.parametrize("T", [3, 9])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=lambda s: "n%d-M%d" % s[:2])
def test_every_output_is_the_oracle_on_the_rows_held(be, shape, T, chunk_rows):
    """Three uneven partial_fit calls with an (n, T) label matrix, then remove of the middle batch: _parity's bars.  Printed, not
    gated: each column's distance to a one-output model fed the same batches (they differ by the order of f64 sums only)."""
    import odx
    n, M, D, sigma, lam = shape
    X, Y, Z, cuts, a_all, left, a_left = _reference(shape, T, sigma)
    est = _feed(_model(shape, Z, odx.GaussianKernel(sigma), outputs=T, chunk_rows=chunk_rows), X, Y, cuts)
    assert est.n_seen_ == n and tuple(est.alpha_.shape) == (M, T) and tuple(est.rhs_.shape) == (T, (M + 1) // 2 * 2)
    assert torch.equal(est.gram_[:, :M], est.gram_[:, :M].t())
    if chunk_rows is None:
        d = []
        for t in range(T):
            one = _feed(_model(shape, Z, odx.GaussianKernel(sigma)), X, Y[:, t:t + 1], cuts, last_only=True)
            d.append(rel(est.alpha_[:, t].cpu().numpy(), one.alpha_.cpu().numpy()))
            if t == 0:
                assert torch.equal(one.gram_, est.gram_), "G depends on the labels"
        print("n %d M %d T %d: distance to the one-output model per column %s" % (n, M, T, " ".join("%.1e" % v for v in d)))
    _parity(est, X, Y, Z, cuts, a_all, left, a_left, sigma, "n %d M %d T %d" % (n, M, T))


def test_matern_outputs(be, monkeypatch):
    import odx
    from oracle import falkon_ref as fr
    monkeypatch.setattr(fr, "gaussian_kernel", radial_kernel)
    k = odx.MaternKernel(5.0, 1.5)
    X, Y, Z, cuts, a_all, left, a_left = _reference(SMALL, 3, k)
    est = _feed(_model(SMALL, Z, k, outputs=3), X, Y, cuts)
    _parity(est, X, Y, Z, cuts, a_all, left, a_left, k, "matern 3/2 T 3")


@pytest.mark.parametrize("T", [1, 3])
def test_solve_path_members_are_the_oracle_at_their_penalty(be, T):
    import odx
    n, M, D, sigma, lam = SMALL
    X, Y, Z, cuts = _reference(SMALL, T, sigma)[:4]
    est = _feed(_model(SMALL, Z, odx.GaussianKernel(sigma), outputs=T), X, Y, cuts)
    a0 = est.alpha_.clone()
    members = est.solve_path(PENALTIES)
    assert est.penalty == lam and torch.equal(est.alpha_, a0) and [m.penalty for m in members] == PENALTIES
    assert all(m.ny_points_ is members[0].ny_points_ for m in members)
    for m, pen in zip(members, PENALTIES):
        ref = _reference(SMALL, T, sigma, pen)[4]
        r = [rel(m.alpha_[:, t].cpu().numpy(), ref[:, t]) for t in range(T)]
        print("T %d penalty %g: alpha rel err per column %s" % (T, pen, " ".join("%.1e" % v for v in r)))
        assert tuple(m.alpha_.shape) == (M, T) and max(r) < 1e-4, (pen, r)
    print("T %d: the member at the model's penalty against solve(): %.1e" % (T, rel(members[1].alpha_.cpu().numpy(), a0.cpu().numpy())))
    Xq = _t(X[:200])
    if T == 1:
        P = odx.predict_path(members, Xq)
        assert tuple(P.shape) == (200, len(PENALTIES))
        for l, m in enumerate(members):
            assert torch.equal(P[:, l], m.predict(Xq)[:, 0])
    else:
        assert tuple(members[0].predict(Xq).shape) == (200, T)
    with pytest.raises(RuntimeError, match="solve_path"):
        _model(SMALL, Z, odx.GaussianKernel(sigma), outputs=T).solve_path(PENALTIES)


def test_pickle_and_as_falkon_carry_every_output(be):
    import odx
    n, M, D, sigma, lam = SMALL
    X, Y, Z, cuts = _reference(SMALL, 3, sigma)[:4]
    est = _model(SMALL, Z, odx.GaussianKernel(sigma), outputs=3)
    for i in range(2):
        est.partial_fit(_t(X[cuts[i]:cuts[i + 1]]), _t((Y[cuts[i]:cuts[i + 1]])))
    back = pickle.loads(pickle.dumps(est))
    assert "_P" not in back.__dict__ and back.outputs == 3 and tuple(back.rhs_.shape) == (3, (M + 1) // 2 * 2)
    assert torch.equal(back.rhs_, est.rhs_) and torch.equal(back.gram_, est.gram_)
    for m in (est, back):
        m.partial_fit(_t(X[cuts[2]:]), _t((Y[cuts[2]:])))
    assert torch.equal(back.alpha_, est.alpha_)
    f = est.as_falkon()
    Xq = _t(X[:100])
    assert isinstance(f, odx.Falkon) and tuple(f.alpha_.shape) == (M, 3)
    assert tuple(f.predict(Xq).shape) == (100, 3) and torch.equal(f.predict(Xq), est.predict(Xq).cpu())
    with pytest.raises(ValueError, match="label columns"):
        est.partial_fit(Xq, _t((Y[:100, :2])))
