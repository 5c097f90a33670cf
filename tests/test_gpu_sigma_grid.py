"""A (sigma, lambda) grid from one contraction of X Z' on the MI355X: odx_gauss_knm_h2_store_sigmas BITWISE against S calls of
odx_gauss_knm_h2_store (blocks with their pad columns, both planes, the fused right-hand sides), its error codes;
odx_gauss_mmvn_h2_sigmas BITWISE against odx_gauss_mmvn_h2 column by column and against the f64 oracle; odx.falkon_fit_grid
BITWISE against odx.falkon_fit_path per sigma and against the oracle; the estimators (fit_grid, predict_grid)."""
import copy
import ctypes

import numpy as np
import pytest

from tests.synth import blob_problem, centres
from tests.test_gpu_mmv_shared import CASES as MMV_CASES, _problem as _mmv_problem

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
TAIL = 64                                     # sentinel bytes behind every block


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def route(be):
    """The backend with its routing switches and the tile pin restored afterwards."""
    old = (be.gauss, be.knm_storage, be.shared_mmv_min, be.sigma_grid_min_features)
    be.gauss = "h2"
    yield be
    be.gauss, be.knm_storage, be.shared_mmv_min, be.sigma_grid_min_features = old
    be.pin_gauss_tile(0)


# ---------------------------------------------------------------- 1. the build entry
NS = [1, 255, 257, 700]                       # below, on both sides of and beyond the 256-row tile
MS = [1, 63, 257, 513, 1001]                  # one column, below a tile, tile + 1, two tiles + 1, four tiles (odd)
DS = [8, 96, 256]
FMTS = ["f32", "u24", "bf16"]
WIDTHS = [2.0, 5.0, 15.0, 50.0]
# 20 cases: every (n, M) pair once (4 and 5 are coprime); D, S, fmt, with / without w rotate
BUILD_CASES = [(NS[i % 4], MS[i % 5], DS[(i + i // 5) % 3], 1 + (i + i // 4) % 4, FMTS[(i + i // 3) % 3], (i + i // 2) % 2 == 0, i)
               for i in range(20)]


def _widths(S, i):
    """S widths out of {2, 5, 15, 50}, starting somewhere else per case; every third case with S >= 2 repeats its first."""
    s = [WIDTHS[(i + k) % 4] for k in range(S)]
    if S >= 2 and i % 3 == 0:
        s[-1] = s[0]
    return s


def test_the_build_cases_cover_what_they_should():
    assert {(c[0], c[1]) for c in BUILD_CASES} == {(n, M) for n in NS for M in MS}
    assert {c[2] for c in BUILD_CASES} == set(DS) and {c[3] for c in BUILD_CASES} == {1, 2, 3, 4}
    assert {(c[4], c[5]) for c in BUILD_CASES} == {(f, w) for f in FMTS for w in (True, False)}
    lists = [_widths(c[3], c[6]) for c in BUILD_CASES]
    assert any(len(set(s)) < len(s) for s in lists) and {x for s in lists for x in s} == set(WIDTHS)


def _operands(be, n, M, D, seed):
    X, _, rng = blob_problem(n + M, D, seed=seed)
    F, Zf = be.features(torch.from_numpy(X[:n])), be.features(torch.from_numpy(X[n:]))
    be.pack(F), be.pack(Zf)
    return F, Zf, rng


def _blocks(be, n, M, fmt, S):
    """S sentinel-filled raw buffers (block + TAIL bytes) and the Knm views into them."""
    from odx import hip
    need = int(be.lib.odx_knm_bytes(n, M, hip.KNM_CODE[fmt]))
    raws = [torch.full((need + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(S)]
    return raws, [be._knm_block(n, M, fmt, r[:need]) for r in raws], need


def _store_args(F, Zf):
    from odx.backend import _p
    return [_p(F.P), F.P.stride(0), _p(F.meta), _p(F.sq), F.n, _p(Zf.P), Zf.P.stride(0), _p(Zf.meta), _p(Zf.sq), Zf.n, F.D]


def _sigmas_call(be, F, Zf, sigmas, fmt, Ks, w, ktw, ldktw, ws, ws_bytes, S=None, sig=None):
    from odx import hip
    from odx.backend import _p
    S = len(sigmas) if S is None else S
    sig = (ctypes.c_double * max(len(sigmas), 1))(*sigmas) if sig is None else sig
    hi = (ctypes.c_void_p * max(len(Ks), 1))(*[K.K.data_ptr() if K is not None else None for K in Ks])
    lo = (ctypes.c_void_p * max(len(Ks), 1))(*[K.lo.data_ptr() if K is not None and K.lo is not None else None for K in Ks])
    ld = next((K.ld for K in Ks if K is not None), 8)
    return be.lib.odx_gauss_knm_h2_store_sigmas(*_store_args(F, Zf), sig, S, hip.KNM_CODE[fmt], hi, ld, lo if fmt == "u24" else None, ld,
                                                _p(w), _p(ktw), ldktw, _p(ws), ws_bytes, be._stream())


@pytest.mark.parametrize("n,M,D,S,fmt,with_w,i", BUILD_CASES)
def test_build_entry_bitwise_s_single_builds(be, n, M, D, S, fmt, with_w, i):
    from odx import hip
    from odx.backend import _p
    lib = be.lib
    F, Zf, rng = _operands(be, n, M, D, 4000 + i)
    sigmas = _widths(S, i)
    w = torch.from_numpy(rng.standard_normal(n) / max(n, 1)).cuda() if with_w else None
    per = int(lib.odx_gauss_knm_h2_rhs_workspace_bytes(n, M))
    assert lib.odx_gauss_knm_h2_store_sigmas_workspace_bytes(n, M, S) == S * per
    ws1 = torch.empty(max(per, 16), dtype=torch.uint8, device="cuda")
    # the reference: S calls of odx_gauss_knm_h2_store
    ref_raw, ref_K, need = _blocks(be, n, M, fmt, S)
    ref_ktw = torch.full((S, M), float("nan"), dtype=torch.float64, device="cuda")
    for s in range(S):
        K = ref_K[s]
        hip.check(lib.odx_gauss_knm_h2_store(*_store_args(F, Zf), float(sigmas[s]), hip.KNM_CODE[fmt], _p(K.K), K.ld, _p(K.lo), K.ld, _p(w),
                                             _p(ref_ktw[s] if with_w else None), _p(ws1 if with_w else None), per if with_w else 0,
                                             be._stream()), "odx_gauss_knm_h2_store")
    # the entry, twice
    ldktw = M + 3
    wsS = torch.empty(max(S * per, 16), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        raw, Ks, _ = _blocks(be, n, M, fmt, S)
        ktw = torch.full((S, ldktw), float("nan"), dtype=torch.float64, device="cuda")
        hip.check(_sigmas_call(be, F, Zf, sigmas, fmt, Ks, w, ktw if with_w else None, ldktw, wsS if with_w else None, S * per if with_w else 0),
                  "odx_gauss_knm_h2_store_sigmas")
        outs.append((raw, ktw))
    torch.cuda.synchronize()
    for raw, ktw in outs:
        for s in range(S):
            assert torch.equal(raw[s], ref_raw[s]), (s, sigmas[s])                 # the block, its pad columns, both planes, the tail
            assert bool((raw[s][need:] == SENTINEL).all())                         # bytes behind the block untouched
            if with_w:
                assert torch.equal(ktw[s, :M], ref_ktw[s]) and torch.isnan(ktw[s, M:]).all()
            else:
                assert torch.isnan(ktw).all()                                      # w NULL: ktw is not touched
    for s in range(1, S):
        if sigmas[s] == sigmas[0]:
            assert torch.equal(outs[0][0][s], outs[0][0][0])                       # equal widths, equal blocks
    assert not bool((ref_raw[0][:need] == SENTINEL).all())                         # (the reference did write)


# ---------------------------------------------------------------- 2. its error codes
def test_build_entry_error_codes(be):
    n, M, D, fmt = 300, 130, 64, "u24"
    F, Zf, rng = _operands(be, n, M, D, 4100)
    lib = be.lib
    w = torch.from_numpy(rng.standard_normal(n)).cuda()
    per = int(lib.odx_gauss_knm_h2_rhs_workspace_bytes(n, M))
    ws = torch.empty(5 * per, dtype=torch.uint8, device="cuda")
    raw, Ks, need = _blocks(be, n, M, fmt, 5)
    ktw = torch.full((5, M), float("nan"), dtype=torch.float64, device="cuda")
    five = (ctypes.c_double * 5)(2.0, 5.0, 15.0, 50.0, 10.0)
    INVALID, WORKSPACE = -1, -4
    assert _sigmas_call(be, F, Zf, [2.0, 5.0], fmt, Ks[:2], w, ktw, M, ws, ws.numel(), S=0) == INVALID
    assert _sigmas_call(be, F, Zf, [], fmt, Ks, w, ktw, M, ws, ws.numel(), S=5, sig=five) == INVALID
    assert _sigmas_call(be, F, Zf, [2.0, 0.0], fmt, Ks[:2], w, ktw, M, ws, ws.numel()) == INVALID
    assert _sigmas_call(be, F, Zf, [2.0, -5.0], fmt, Ks[:2], w, ktw, M, ws, ws.numel()) == INVALID
    assert _sigmas_call(be, F, Zf, [2.0, 5.0], fmt, [Ks[0], None], w, ktw, M, ws, ws.numel()) == INVALID      # a null block pointer
    assert _sigmas_call(be, F, Zf, [2.0, 5.0], fmt, Ks[:2], w, ktw, M, ws, 2 * per - 1) == WORKSPACE
    assert _sigmas_call(be, F, Zf, [2.0, 5.0], fmt, Ks[:2], w, ktw, M, None, 2 * per) == WORKSPACE
    assert lib.odx_gauss_knm_h2_store_sigmas_workspace_bytes(n, M, 2) == 2 * per
    F0 = copy.copy(F)
    F0.n = 0                                                                                               # n = 0: ODX_OK, nothing written
    assert _sigmas_call(be, F0, Zf, [2.0, 5.0], fmt, Ks[:2], w, ktw, M, None, 0) == 0
    torch.cuda.synchronize()
    assert all(bool((r == SENTINEL).all()) for r in raw) and torch.isnan(ktw).all()
    assert _sigmas_call(be, F, Zf, [2.0, 5.0], fmt, Ks[:2], w, ktw, M, ws, ws.numel()) == 0                 # and the same arguments do work
    torch.cuda.synchronize()
    assert not torch.isnan(ktw[:2]).any() and torch.isnan(ktw[2:]).all()


# ---------------------------------------------------------------- 3. the scoring entry, bit for bit
SCORE_CASES = [c for c in MMV_CASES if c[1] in (63, 257, 513, 1100) and c[3] in (2, 3, 5, 8, 9, 17)]
SCORE_LARGE = [c for c in SCORE_CASES if c[1] in (513, 1100)]


def test_the_scoring_cases_cover_what_they_should():
    assert {c[0] for c in SCORE_CASES} == {1, 127, 129, 255, 257, 700}
    assert {c[1] for c in SCORE_CASES} == {63, 257, 513, 1100} and {c[3] for c in SCORE_CASES} == {2, 3, 5, 8, 9, 17}
    assert len(SCORE_LARGE) >= 4


def _three(sigma):
    return [float(sigma), 2.0, 50.0]


def _patterns(T, sigma):
    a, b, c = _three(sigma)
    third = max(1, (T + 2) // 3)
    return {"equal": [a] * T,
            "sigma-major": ([a] * third + [b] * third + [c] * T)[:T],
            "alternating": [(a, b, c)[t % 3] for t in range(T)]}


@pytest.mark.parametrize("tile", [128, 256, 0])
@pytest.mark.parametrize("n,M,D,T,sigma", SCORE_CASES)
def test_scoring_entry_bitwise_the_shared_route_per_column(route, n, M, D, T, sigma, tile):
    be = route
    F, Zf, V, _, _, _ = _mmv_problem(be, n, M, D, T, sigma)
    assert V.stride(0) == T + 3
    be.pin_gauss_tile(tile)
    be.shared_mmv_min = 2
    ref = {s: be.mmv(F, Zf, s, V, None).clone() for s in _three(sigma)}           # odx_gauss_mmvn_h2 at every width, all T columns
    for name, sigmas in _patterns(T, sigma).items():
        wide = torch.full((n, T + 4), float("nan"), dtype=torch.float32, device="cuda")
        got = be.mmv_sigmas(F, Zf, sigmas, V, out=wide[:, 2:2 + T])
        assert got.data_ptr() == wide[:, 2:2 + T].data_ptr()
        assert torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 2 + T:]).all(), name
        assert torch.isfinite(got).all(), name
        for c in range(T):
            assert torch.equal(got[:, c], ref[sigmas[c]][:, c]), (name, c, sigmas[c])
        if name == "equal":
            assert torch.equal(got, ref[sigmas[0]])
        again = be.mmv_sigmas(F, Zf, sigmas, V)
        assert torch.equal(again, got), name


def test_scoring_entry_error_codes(route):
    from odx.backend import _p
    be = route
    n, M, D, T = 255, 511, 64, 9
    F, Zf, V, _, _, _ = _mmv_problem(be, n, M, D, T, 10.0)
    be.pack(F), be.pack(Zf)
    lib = be.lib
    nbytes = lib.odx_gauss_mmvn_h2_sigmas_workspace_bytes(n, M, T)
    assert nbytes == lib.odx_gauss_mmvn_h2_workspace_bytes(n, M, T) and nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((n, T), float("nan"), dtype=torch.float32, device="cuda")
    good = (ctypes.c_double * T)(*([10.0] * T))
    bad = (ctypes.c_double * T)(*([10.0] * (T - 1) + [0.0]))

    def call(sig, nn, wsp, wsb):
        return lib.odx_gauss_mmvn_h2_sigmas(*_store_args(F, Zf)[:4], nn, *_store_args(F, Zf)[5:], sig, _p(V), V.stride(0), T, _p(out), out.stride(0),
                                            wsp, wsb, be._stream())
    assert call(bad, n, _p(ws), nbytes) == -1
    assert call(good, n, _p(ws), nbytes - 1) == -4 and call(good, n, None, nbytes) == -4
    assert call(good, 0, None, 0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call(good, n, _p(ws), nbytes) == 0
    be.shared_mmv_min = 2
    assert torch.equal(out, be.mmv(F, Zf, 10.0, V, None))


# ---------------------------------------------------------------- 4. the scoring entry against f64
@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("n,M,D,T,sigma", [c for c in MMV_CASES if c[1] in (513, 1100)])
def test_scoring_entry_against_f64(route, n, M, D, T, sigma, tile):
    """Column c against oracle.falkon_ref.gaussian_kernel(X, Z, sigma_c) @ V[:, c] in f64, within 5e-5 max(1, max|ref|): the bar
    of test_gpu_mmv_shared.test_against_f64, on that file's LARGE shapes."""
    from oracle import falkon_ref as fr
    be = route
    F, Zf, V, Xr, Z, Vh = _mmv_problem(be, n, M, D, T, sigma)
    sigmas = _patterns(T, sigma)["alternating"]
    Ks = {s: fr.gaussian_kernel(Xr.astype(np.float64), Z.astype(np.float64), s, np.float64) for s in set(sigmas)}
    ref = np.stack([Ks[sigmas[c]] @ Vh[:, c] for c in range(T)], axis=1)
    be.pin_gauss_tile(tile)
    got = be.mmv_sigmas(F, Zf, sigmas, V).cpu().numpy()
    err, bound = np.abs(got - ref).max(), 5e-5 * max(1.0, np.abs(ref).max())
    print("n %d M %d D %d T %d tile %d: err %.3e bound %.3e" % (n, M, D, T, tile, err, bound))
    assert err < bound


# ---------------------------------------------------------------- 5. falkon_fit_grid = falkon_fit_path per sigma, bit for bit
class _Counted:
    """Counts the backend's knm_rhs_sigmas groups and knm_rhs calls while a grid is fitted."""

    def __init__(self, be):
        self.be, self.groups, self.singles = be, [], 0

    def __enter__(self):
        be, inner_sig, inner_one = self.be, self.be.knm_rhs_sigmas, self.be.knm_rhs

        def knm_rhs_sigmas(F, Zf, sigmas, w, outs=None):
            self.groups.append(len(sigmas))
            return inner_sig(F, Zf, sigmas, w, outs=outs)

        def knm_rhs(*a, **kw):
            self.singles += 1
            return inner_one(*a, **kw)
        be.knm_rhs_sigmas, be.knm_rhs = knm_rhs_sigmas, knm_rhs
        return self

    def __exit__(self, *exc):
        del self.be.knm_rhs_sigmas, self.be.knm_rhs
        return False


_fit_problem = {}


def _small_fit(be):
    if not _fit_problem:
        X, y, rng = blob_problem(3000, 64, seed=9)
        _fit_problem["p"] = (X, y, centres(y, 300, rng))
    X, y, idx = _fit_problem["p"]
    F = be.features(torch.from_numpy(X))
    return F, be.rows(F, idx), be.vec(y)


@pytest.mark.parametrize("knm,tile,entry", [("f32", 0, False), ("f32", 256, True), ("u24", 256, True), ("bf16", 256, True),
                                            ("stream", 0, False)])
def test_fit_grid_bitwise_fit_path_per_sigma(route, knm, tile, entry):
    import odx
    be = route
    be.knm_storage = knm
    be.pin_gauss_tile(tile)
    be.sigma_grid_min_features = 0                 # (this problem has 64 features: the shipped rule would loop everywhere)
    F, Zf, y = _small_fit(be)
    sigmas, lams = [4.0, 8.0, 12.0], [1e-3, 1e-5, 1e-4]
    paths = [odx.falkon_fit_path(be, F, y, Zf, s, lams, 20).clone() for s in sigmas]
    for width, want in ((4, [3]), (2, [2, 1]), (1, [1, 1, 1])):
        blocks = []
        with _Counted(be) as cnt:
            grid = odx.falkon_fit_grid(be, F, y, Zf, sigmas, lams, 20, blocks_at_once=width, knm_blocks=blocks)
        assert tuple(grid.shape) == (3, 3, Zf.n) and len(blocks) == 3 and all(K.fmt == knm for K in blocks)
        assert cnt.groups == want
        assert cnt.singles == (0 if entry else 3), (cnt.singles, knm, tile)      # the entry builds the blocks; elsewhere knm_rhs is looped
        for s in range(3):
            assert torch.equal(grid[s], paths[s]), (knm, tile, width, sigmas[s], float((grid[s] - paths[s]).abs().max()))


def test_knm_rhs_sigmas_entries_are_knm_rhs(route):
    """Five widths (a group of four and one more) on the entry route: every block and right-hand side is knm_rhs's."""
    be = route
    be.knm_storage = "u24"
    be.pin_gauss_tile(256)
    be.sigma_grid_min_features = 0
    F, Zf, y = _small_fit(be)
    w = y / 3000.0
    sigmas = [3.0, 6.0, 9.0, 6.0, 20.0]
    with _Counted(be) as cnt:
        got = be.knm_rhs_sigmas(F, Zf, sigmas, w)
    assert len(got) == 5 and cnt.singles == 0
    for (K, b), s in zip(got, sigmas):
        K1, b1 = be.knm_rhs(F, Zf, s, w)
        assert K.fmt == K1.fmt == "u24" and K.ld == K1.ld
        assert torch.equal(K.K, K1.K) and torch.equal(K.lo, K1.lo) and torch.equal(b, b1)


def test_the_shipped_rule_loops_below_its_feature_count(route):
    """sigma_grid_min_features (1024 as shipped, profiles/sigma_grid.md): 64 features go width by width through knm_rhs, None
    never takes the entry; the blocks are the same either way."""
    be = route
    be.knm_storage = "u24"
    be.pin_gauss_tile(256)
    F, Zf, y = _small_fit(be)
    w = y / 3000.0
    assert be.sigma_grid_min_features == 1024 and F.D == 64
    be.sigma_grid_min_features = 0
    want = be.knm_rhs_sigmas(F, Zf, [4.0, 8.0], w)
    for least in (1024, 65, None):
        be.sigma_grid_min_features = least
        with _Counted(be) as cnt:
            got = be.knm_rhs_sigmas(F, Zf, [4.0, 8.0], w)
        assert cnt.singles == 2, least
        assert all(torch.equal(a[0].K, b[0].K) and torch.equal(a[0].lo, b[0].lo) and torch.equal(a[1], b[1]) for a, b in zip(got, want))
    be.sigma_grid_min_features = 64
    with _Counted(be) as cnt:
        be.knm_rhs_sigmas(F, Zf, [4.0, 8.0], w)
    assert cnt.singles == 0


# ---------------------------------------------------------------- 6. falkon_fit_grid against the oracle
@pytest.mark.parametrize("knm", ["f32", "u24"])
def test_fit_grid_against_the_oracle(route, knm):
    """sigma 5 and 15 x lambda 1e-3 and 1e-5 at n = 8000, M = 2000, D = 2048 (rows of test_gpu_falkon_path.PATH_GRID): alpha < 1e-4
    relative, scores < 1e-4 max(1, max|ref|) against the f64 oracle at every member — the project's bars."""
    import odx
    from oracle import falkon_ref as fr
    be = route
    be.knm_storage = knm
    be.pin_gauss_tile(256 if knm == "u24" else 0)
    sigmas, lams = [5.0, 15.0], [1e-3, 1e-5]
    X, y, rng = blob_problem(8000, 2048, seed=5000 + 2000 + 2048)
    idx = centres(y, 2000, rng)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    blocks = []
    grid = odx.falkon_fit_grid(be, F, be.vec(y), Zf, sigmas, lams, 20, knm_blocks=blocks)
    assert tuple(grid.shape) == (2, 2, Zf.n) and [K.fmt for K in blocks] == [knm, knm]
    cols = [(s, l) for s in range(2) for l in range(2)]
    V = torch.stack([grid[s, l] for s, l in cols], dim=1).contiguous()
    scores = be.mmv_sigmas(F, Zf, [sigmas[s] for s, _ in cols], V).cpu().numpy()
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    for t, (s, l) in enumerate(cols):
        ref, Z = fr.falkon_fit(X64, y64, idx, sigmas[s], lams[l], maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        rel = np.linalg.norm(grid[s, l].cpu().numpy() - ref[:, 0]) / np.linalg.norm(ref[:, 0])
        pref = fr.falkon_predict(X64, Z, ref, sigmas[s])[:, 0]
        serr = np.abs(scores[:, t] - pref).max()
        print("sigma=%g lam=%g fmt=%s: alpha rel err %.2e, score err %.2e (max |ref| %.2f)" % (sigmas[s], lams[l], knm, rel, serr, np.abs(pref).max()))
        assert rel < 1e-4, (sigmas[s], lams[l], rel)
        assert serr < 1e-4 * max(1.0, float(np.abs(pref).max())), (sigmas[s], lams[l], serr)


# ---------------------------------------------------------------- 7. the estimators
def _estimator(idx, sigma=8.0):
    import odx
    from odx.wrappers import CenterSelector
    return odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=sigma), penalty=1e-4, M=len(idx), maxiter=10,
                            center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))


def test_estimator_fit_grid_and_predict_grid(route):
    import odx
    be = route
    X, y, rng = blob_problem(600, 64, seed=79)
    idx = centres(y[:450], 130, rng)
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    sigmas, lams = [5.0, 8.0, 12.0], [1e-5, 1e-3]
    template = _estimator(idx, 9.0)
    grid = template.fit_grid(Xt[:450], yt[:450], sigmas, lams)
    assert template.alpha_ is None and template.kernel.sigma == 9.0
    assert len(grid) == 3 and all(len(row) == 2 for row in grid)
    for s, sigma in enumerate(sigmas):
        path = _estimator(idx, sigma).fit_path(Xt[:450], yt[:450], lams)
        for l, lam in enumerate(lams):
            e = grid[s][l]
            assert e.kernel.sigma == sigma and e.penalty == lam and e.ny_points_ is grid[0][0].ny_points_
            assert torch.equal(e.alpha_, path[l].alpha_), (sigma, lam)
    flat = [grid[s][l] for l in range(2) for s in range(3)]                # lambda-major: the widths alternate along the columns
    Xval = Xt[450:]
    got = odx.predict_grid(flat, Xval)
    assert tuple(got.shape) == (150, 6) and got.dtype == torch.float32
    for sigma in sigmas:
        same = []
        for e in flat:                                                     # all members stacked, scored at ONE width
            c = copy.copy(e)
            c.kernel = odx.GaussianKernel(sigma=sigma)
            same.append(c)
        ref = odx.predict_path(same, Xval)
        for t, e in enumerate(flat):
            if e.kernel.sigma == sigma:
                assert torch.equal(got[:, t], ref[:, t]), (sigma, t)
    with pytest.raises(ValueError, match="sigma"):
        odx.predict_path(flat, Xval)                                       # predict_path keeps refusing mixed widths
    other = _estimator(idx, 5.0).fit(Xt[:450], yt[:450])                   # the same centres' values in a tensor of its own
    with pytest.raises(ValueError, match="ny_points_"):
        odx.predict_grid([flat[0], other], Xval)
