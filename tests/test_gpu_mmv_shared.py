"""Shared-centre scoring on the MI355X (odx_gauss_mmvn_h2, HipBackend.shared_mmv_min): all columns of a dense V from one
evaluation of K(X, Z) per group of up to 8 columns, BITWISE what the per-column launch (odx_gauss_mmv_h2, every range [0, M))
gives, on both tile cores and under the dispatch rule; against the f64 oracle; the C entry; the estimators through it."""
import ctypes

import numpy as np
import pytest

from tests.synth import blob_problem, centres

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NS = [1, 127, 129, 255, 257, 700]                 # row blocks of 128 and 256: below, on both sides of an edge, several
MS = [1, 63, 255, 257, 511, 513, 1100]            # tile edges at 128 and 256, the group of two wide tiles at 512, the s16 groups
DS = [8, 64, 96, 256]
TS = [2, 3, 4, 5, 7, 8, 9, 16, 17]                # every instantiated width, the padded ones, 8 + 1, two full groups, 16 + 1
# 42 cases: every (n, M) pair once (6 and 7 are coprime), every D, T and sigma several times
CASES = [(NS[i % 6], MS[i % 7], DS[(i + i // 7) % 4], TS[i % 9], (4.0, 10.0)[(i // 3) % 2]) for i in range(42)]
LARGE = [c for c in CASES if c[1] in (513, 1100)]


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def route(be):
    """The backend with the routing switch and the tile pin restored afterwards."""
    old = (be.gauss, be.shared_mmv_min)
    be.gauss = "h2"
    yield be
    be.gauss, be.shared_mmv_min = old
    be.pin_gauss_tile(0)


_problems = {}


def _problem(be, n, M, D, T, sigma):
    """Rows, centres and weights of a case, made once: V is a column block of a wider matrix (ldv = T + 3, its first element
    8 bytes into a row)."""
    key = (n, M, D, T, sigma)
    if key not in _problems:
        X, _, rng = blob_problem(n + M, D, seed=1000 + 7 * n + M + D + T)
        Xr, Z = X[:n], X[n:]
        Vw = rng.standard_normal((M, T + 3)) * np.logspace(0, -2, T + 3)[None, :]
        _problems[key] = (Xr, Z, Vw)
    Xr, Z, Vw = _problems[key]
    F, Zf = be.features(torch.from_numpy(Xr)), be.features(torch.from_numpy(Z))
    V = torch.from_numpy(Vw).cuda()[:, 1:1 + T]
    assert V.stride(0) == T + 3 and V.data_ptr() % 16 == 8
    return F, Zf, V, Xr, Z, Vw[:, 1:1 + T]


def _both(be, F, Zf, sigma, V, **kw):
    be.shared_mmv_min = None
    a = be.mmv(F, Zf, sigma, V, None, **kw)
    a = a.clone()
    be.shared_mmv_min = 2
    b = be.mmv(F, Zf, sigma, V, None, **kw)
    return a, b


@pytest.mark.parametrize("tile", [128, 256, 0])
@pytest.mark.parametrize("n,M,D,T,sigma", CASES)
def test_bitwise_the_per_column_launch(route, n, M, D, T, sigma, tile):
    be = route
    F, Zf, V, _, _, _ = _problem(be, n, M, D, T, sigma)
    be.pin_gauss_tile(tile)
    a, b = _both(be, F, Zf, sigma, V)
    assert tuple(b.shape) == (n, T) and torch.isfinite(b).all()
    assert torch.equal(a, b), (a - b).abs().max().item()


@pytest.mark.parametrize("tile", [128, 256])
def test_an_odd_leading_dimension(route, tile):
    """V (M, 3) contiguous: ldv = 3, columns at every 8-byte alignment."""
    be = route
    F, Zf, _, _, _, Vh = _problem(be, 257, 513, 96, 3, 10.0)
    V = torch.from_numpy(np.ascontiguousarray(Vh)).cuda()
    assert V.stride(0) == 3
    be.pin_gauss_tile(tile)
    a, b = _both(be, F, Zf, 10.0, V)
    assert torch.equal(a, b)


@pytest.mark.parametrize("tile", [128, 256])
def test_a_strided_column_block_of_out(route, tile):
    be = route
    n, M, D, T, sigma = 129, 257, 64, 5, 4.0
    F, Zf, V, _, _, _ = _problem(be, n, M, D, T, sigma)
    be.pin_gauss_tile(tile)
    be.shared_mmv_min = None
    ref = be.mmv(F, Zf, sigma, V, None)
    wide = torch.full((n, T + 4), float("nan"), dtype=torch.float32, device="cuda")
    be.shared_mmv_min = 2
    got = be.mmv(F, Zf, sigma, V, None, out=wide[:, 2:2 + T])
    assert got.data_ptr() == wide[:, 2:2 + T].data_ptr()
    assert torch.equal(wide[:, 2:2 + T], ref)
    assert torch.isnan(wide[:, :2]).all() and torch.isnan(wide[:, 2 + T:]).all()


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("n,M,D,T,sigma", LARGE)
def test_against_f64(route, n, M, D, T, sigma, tile):
    """Against oracle.falkon_ref.gaussian_kernel(X, Z, sigma) @ V in f64, within the bound the project uses for this kernel on
    this generator (test_mmv_block_structure): 5e-5 max(1, |ref|.max())."""
    from oracle import falkon_ref as fr
    be = route
    F, Zf, V, Xr, Z, Vh = _problem(be, n, M, D, T, sigma)
    ref = fr.gaussian_kernel(Xr.astype(np.float64), Z.astype(np.float64), sigma, np.float64) @ Vh
    be.pin_gauss_tile(tile)
    be.shared_mmv_min = 2
    got = be.mmv(F, Zf, sigma, V, None).cpu().numpy()
    err, bound = np.abs(got - ref).max(), 5e-5 * max(1.0, np.abs(ref).max())
    print("n %d M %d D %d T %d sigma %g tile %d: err %.3e bound %.3e" % (n, M, D, T, sigma, tile, err, bound))
    assert err < bound


def _entry_args(be, F, Zf, sigma, V, out):
    from odx.backend import _p
    be.pack(F), be.pack(Zf)
    T = V.shape[1]
    return [_p(F.P), F.P.stride(0), _p(F.meta), _p(F.sq), F.n, _p(Zf.P), Zf.P.stride(0), _p(Zf.meta), _p(Zf.sq), Zf.n, F.D,
            float(sigma), _p(V), V.stride(0), T, _p(out), out.stride(0)]


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("T", [1, 9])
def test_the_c_entry(route, T, tile):
    """A group of one column and 8 + 1 columns through odx_gauss_mmvn_h2 itself; a workspace one byte short; n = 0."""
    from odx import hip
    be = route
    n, M, D, sigma = 255, 511, 64, 10.0
    F, Zf, V9, _, _, _ = _problem(be, n, M, D, 9, sigma)
    V = V9[:, :T]
    be.pin_gauss_tile(tile)
    be.shared_mmv_min = None
    ref = be.mmv(F, Zf, sigma, V, None)
    lib, stream = be.lib, be._stream()
    nbytes = lib.odx_gauss_mmvn_h2_workspace_bytes(n, M, T)
    assert nbytes == lib.odx_gauss_mmv_h2_workspace_bytes(n, M, T) and nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((n, T + 1), float("nan"), dtype=torch.float32, device="cuda")
    args = _entry_args(be, F, Zf, sigma, V, out)
    hip.check(lib.odx_gauss_mmvn_h2(*args, ctypes.c_void_p(ws.data_ptr()), nbytes, stream), "odx_gauss_mmvn_h2")
    assert torch.equal(out[:, :T], ref) and torch.isnan(out[:, T]).all()
    out.fill_(float("nan"))
    assert lib.odx_gauss_mmvn_h2(*args, ctypes.c_void_p(ws.data_ptr()), nbytes - 1, stream) == -4          # ODX_ERR_WORKSPACE
    assert lib.odx_gauss_mmvn_h2(*args, None, nbytes, stream) == -4
    args0 = list(args)
    args0[4] = 0                                                                                           # n = 0
    assert lib.odx_gauss_mmvn_h2(*args0, None, 0, stream) == 0
    assert lib.odx_gauss_mmvn_h2_workspace_bytes(0, M, T) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("tile", [128, 256])
def test_bit_repeatable(route, tile):
    be = route
    F, Zf, V, _, _, _ = _problem(be, 700, 1100, 256, 17, 10.0)
    be.pin_gauss_tile(tile)
    be.shared_mmv_min = 2
    a = be.mmv(F, Zf, 10.0, V, None).clone()
    b = be.mmv(F, Zf, 10.0, V, None)
    assert torch.equal(a, b)


def _estimator(idx, sigma=8.0):
    import odx
    from odx.wrappers import CenterSelector
    return odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=sigma), penalty=1e-4, M=len(idx), maxiter=10,
                            center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))


def test_a_multi_output_model_predicts_through_the_route(route):
    be = route
    n, M, D, T = 600, 130, 64, 3
    X, y, rng = blob_problem(n, D, seed=77)
    idx = centres(y, M, rng)
    g = np.random.default_rng(78)
    Y = np.stack([y.astype(np.float64)] + [np.where(X @ g.standard_normal(D) > 0, 1.0, -1.0) for _ in range(T - 1)], 1)
    Xt = torch.from_numpy(X).cuda()
    m = _estimator(idx).fit_multi(Xt, torch.from_numpy(Y).cuda())
    assert tuple(m.alpha_.shape) == (len(idx), T)
    be.shared_mmv_min = None
    F = be.features(Xt)
    cols = [be.mmv(F, m._centres(), m.kernel.sigma, m.alpha_[:, t].contiguous(), None) for t in range(T)]
    before = m.predict(Xt)
    be.shared_mmv_min = 2
    got = m.predict(Xt)
    assert tuple(got.shape) == (n, T)
    assert torch.equal(got, torch.cat(cols, dim=1)) and torch.equal(got, before)


def test_predict_path_through_the_route(route):
    import odx
    be = route
    X, y, rng = blob_problem(600, 64, seed=79)
    idx = centres(y[:450], 130, rng)
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    members = _estimator(idx).fit_path(Xt[:450], yt[:450], [1e-5, 1e-4, 1e-3])
    Xval = Xt[450:]
    be.shared_mmv_min = None
    cols = torch.cat([e.predict(Xval) for e in members], dim=1)
    off = odx.predict_path(members, Xval)
    be.shared_mmv_min = 2
    on = odx.predict_path(members, Xval)
    assert tuple(on.shape) == (150, 3) and torch.equal(on, cols) and torch.equal(off, cols)
    other = _estimator(idx).fit(Xt[:450], yt[:450])          # the same centres' values in a tensor of its own
    with pytest.raises(ValueError, match="ny_points_"):
        odx.predict_path([members[0], other], Xval)
    import copy
    wider = copy.copy(members[1])
    wider.kernel = odx.GaussianKernel(sigma=9.0)
    with pytest.raises(ValueError, match="sigma"):
        odx.predict_path([members[0], wider], Xval)
