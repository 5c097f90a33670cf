"""The CG pass of up to 8 states above the LDS limit of the one-read pass (M > 5084) on the MI355X: T = K V for up to 8 vectors
from one read of a compact block (odx_knm_fwdn_q, HipBackend.kvn), HipBackend.ktkn through the two-read route
(odx_knm_fwdn_q + odx_knm_bwdn_q; wide_pass_min / ktkn_reads), and falkon_fit_multi / falkon_fit_path through it against the
f64 oracle."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_falkon_multi import _check_multi, label_columns
from tests.test_gpu_falkon_path import _check_path, _compact_block

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BAND = 1280      # columns of a band of odx_knm_fwdn_q (csrc/knm_fwd_nv.hip: FW_BCOLS)


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def route(be):
    """The backend with its routing switch restored afterwards."""
    old = be.wide_pass_min
    yield be
    be.wide_pass_min = old


@pytest.fixture
def storage(be):
    old = (be.gauss, be.knm_storage, be.wide_pass_min)
    yield be
    be.gauss, be.knm_storage, be.wide_pass_min = old
    be.pin_gauss_tile(0)


# (n, M, nv): the shapes of the issue — odd M, n below one row group (4 rows) and not a multiple of it, n below one
# workgroup's four groups, M on both sides of the one-read pass's LDS limits, one band and several, the widest block, every
# instantiated width and the odd widths served by the next one
FWD_SHAPES = [(777, 129, 3), (1, 100, 4), (3, 1023, 8), (7, 100, 1), (999, 2045, 5), (530, 2525, 7), (300, 5085, 8), (130, 10000, 8),
              (64, 10240, 5), (40, 20440, 8)]
# ... and one M on each side of every band boundary (k x 1280 | k x 1280 + 1, the latter odd), widths and row counts cycling
_NVS = [8, 3, 2, 5, 1, 4, 7, 6]
FWD_SHAPES += [(5 + 3 * k + s, k * BAND + s, _NVS[(2 * k + s) % 8]) for k in range(1, 20440 // BAND + 1) for s in (0, 1)]


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,M,nv", FWD_SHAPES)
def test_forward_nv_pass(be, fmt, n, M, nv):
    """T[q] = K V[q] from one read, per entry within 3 M 2^-53 (|K| @ |v|) of the dense f64 product: M u for the kernel's
    sum in any order, M u for numpy's, M u for the conversions.  Cells [n:] untouched, bit-repeatable."""
    rng = np.random.default_rng(n * 31 + M + nv)
    K, vals = _compact_block(rng, n, M, fmt)
    ldv, ldt = (M + 1) // 2 * 2 + 6, (n + 1) // 2 * 2 + 4
    Vh = rng.standard_normal((nv, ldv)) * np.logspace(0, -3, nv)[:, None]
    V = torch.from_numpy(Vh).cuda()
    out = torch.full((nv, ldt), float("nan"), dtype=torch.float64, device="cuda")
    be.kvn(K, V, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, n:]).all()
    got = out[:, :n].cpu().numpy()
    for q in range(nv):
        ref = vals @ Vh[q, :M]
        bound = 3 * M * 2.0 ** -53 * (np.abs(vals) @ np.abs(Vh[q, :M]))
        err = np.abs(got[q] - ref)
        print("n=%d M=%d nv=%d %s q=%d: max err / bound %.3f" % (n, M, nv, fmt, q, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), (q, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    again = torch.full_like(out, float("nan"))
    be.kvn(K, V, out=again)
    assert torch.equal(again[:, :n], out[:, :n])


def test_kvn_groups_more_than_eight_vectors(be):
    rng = np.random.default_rng(3)
    K, vals = _compact_block(rng, 333, 6001, "u24")
    Vh = rng.standard_normal((11, 6002))
    out = be.kvn(K, torch.from_numpy(Vh).cuda())
    assert tuple(out.shape) == (11, 334)
    ref = Vh[:, :6001] @ vals.T
    bound = 3 * 6001 * 2.0 ** -53 * (np.abs(Vh[:, :6001]) @ np.abs(vals).T)
    assert (np.abs(out[:, :333].cpu().numpy() - ref) <= bound).all()


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("L", [3, 8, 11])
@pytest.mark.parametrize("n,M", [(515, 5085), (401, 10000), (203, 20440)])
def test_ktkn_through_the_two_read_route(route, fmt, n, M, L):
    """out[l] = K'(K V[l]) with wide_pass_min = 3 (chunks of up to 8 vectors, two reads each) and with the route off (pairs
    and singles): the bounds of test_nv_vector_pass — 1e-11 max|ref| against the dense f64 product, 1e-12 max|single|
    against ktk — guard cells untouched, bit-repeatable."""
    be = route
    rng = np.random.default_rng(n * 31 + M + L)
    K, vals = _compact_block(rng, n, M, fmt)
    assert be.ktkn_width(K) <= 2
    ld = (M + 1) // 2 * 2 + 6
    Vh = rng.standard_normal((L, ld)) * np.logspace(0, -3, L)[:, None]
    V = torch.from_numpy(Vh).cuda()
    refs = [vals.T @ (vals @ Vh[q, :M]) for q in range(L)]
    singles = [be.ktk(K, v=V[q, :M].contiguous()) for q in range(L)]
    for wmin in (3, None):
        be.wide_pass_min = wmin
        pairs_reads = -(-L // 2) if be.can_ktk2(K) else L
        assert be.ktkn_reads(K, L) == (2 * -(-L // 8) if wmin else pairs_reads)
        out = torch.full((L, ld), float("nan"), dtype=torch.float64, device="cuda")
        be.ktkn(K, V, out=out)
        assert torch.isnan(out[:, M:]).all()
        for q in range(L):
            err = np.abs(out[q, :M].cpu().numpy() - refs[q]).max()
            assert err <= 1e-11 * np.abs(refs[q]).max(), (wmin, q, err, np.abs(refs[q]).max())
            assert float((out[q, :M] - singles[q]).abs().max()) <= 1e-12 * float(singles[q].abs().max()), (wmin, q)
        again = torch.full_like(out, float("nan"))
        be.ktkn(K, V, out=again)
        assert torch.equal(again[:, :M], out[:, :M])


def test_routing(route):
    be = route
    rng = np.random.default_rng(5)
    blocks = {M: _compact_block(rng, 8, M, "u24")[0] for M in (2000, 4500, 10000)}
    for wmin in (3, None):
        be.wide_pass_min = wmin
        assert [be.ktkn_width(blocks[M]) for M in (2000, 4500, 10000)] == [8, 4, 2]
        assert be.ktkn_reads(blocks[2000], 8) == 1
        assert be.ktkn_reads(blocks[4500], 8) == 2                      # two 4-wide reads, as before
        assert be.ktkn_reads(blocks[10000], 8) == (2 if wmin else 4)
    be.wide_pass_min = 3
    assert be.ktkn_reads(blocks[10000], 2) == 1 and be.ktkn_reads(blocks[10000], 10) == 3      # 8 by the route + a pair
    from odx.backend import Knm
    Kf = Knm()
    Kf.K, Kf.n, Kf.M, Kf.ld = torch.rand((90, 300), device="cuda"), 90, 300, 300
    assert Kf.fmt == "f32"
    with pytest.raises(ValueError, match="compact"):
        be.kvn(Kf, torch.zeros((2, 300), dtype=torch.float64, device="cuda"))
    assert be.ktkn_reads(Kf, 8) == 8 // be.ktkn_width(Kf)


def test_limits_of_the_forward_entry(be):
    from odx import hip
    lib = be.lib
    assert lib.odx_knm_fwdn_q_workspace_bytes(1000, 20440, hip.KNM_U24, 8) >= 0
    assert lib.odx_knm_fwdn_q_workspace_bytes(1000, 20440, hip.KNM_BF16, 1) >= 0
    assert lib.odx_knm_fwdn_q_workspace_bytes(1000, 20441, hip.KNM_U24, 8) < 0
    assert lib.odx_knm_fwdn_q_workspace_bytes(1000, 2000, hip.KNM_U24, 9) < 0
    assert lib.odx_knm_fwdn_q_workspace_bytes(1000, 2000, hip.KNM_U24, 0) < 0
    assert lib.odx_knm_fwdn_q_workspace_bytes(1000, 2000, hip.KNM_F32, 4) < 0
    rng = np.random.default_rng(9)
    K, _ = _compact_block(rng, 10, 2000, "u24")
    V = torch.zeros((9, 2000), dtype=torch.float64, device="cuda")
    out = torch.full((9, 16), float("nan"), dtype=torch.float64, device="cuda")

    def call(fmt, n, M, nv, T, ldt):
        return lib.odx_knm_fwdn_q(ctypes.c_void_p(K.K.data_ptr()), K.ld, ctypes.c_void_p(K.lo.data_ptr()), K.ld, fmt, n, M, nv,
                                  ctypes.c_void_p(V.data_ptr()), 2000, ctypes.c_void_p(T), ldt, None, 0, None)
    for fmt, M, nv in ((hip.KNM_F32, 2000, 4), (hip.KNM_U24, 20441, 4), (hip.KNM_U24, 2000, 0), (hip.KNM_U24, 2000, 9)):
        assert lib.odx_knm_fwdn_q_workspace_bytes(10, M, fmt, nv) < 0
        assert call(fmt, 10, M, nv, out.data_ptr(), 16) == -3                   # ODX_ERR_UNSUPPORTED (include/odx.h)
        assert b"odx_knm_fwdn_q" in lib.odx_last_error_string()
    assert call(hip.KNM_U24, 10, 2000, 4, out.data_ptr() + 8, 16) != 0          # rows of T not 16-byte aligned
    assert call(hip.KNM_U24, 10, 2000, 4, out.data_ptr(), 15) != 0              # odd ldt
    assert call(hip.KNM_U24, 10, 2000, 4, out.data_ptr(), 8) != 0               # ldt < n
    assert call(hip.KNM_U24, 0, 2000, 4, out.data_ptr(), 16) == 0               # n = 0: nothing is written
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert call(hip.KNM_U24, 10, 2000, 4, out.data_ptr(), 16) == 0
    torch.cuda.synchronize()
    assert float(out[:4, :10].abs().max()) == 0.0 and torch.isnan(out[:4, 10:]).all() and torch.isnan(out[4:]).all()


def _wide_rows():
    """20 000 rows, D = 64, 5200 centres: the recipe of test_multi_takes_the_four_wide_pass_and_a_pair moved just past the
    limit of the 4-wide one-read pass (profiles/wide_pass.md has the fixture's distance from the bars)."""
    from tests.synth import blob_problem, centres
    X, y, rng = blob_problem(20000, 64, seed=79)
    return X, y, centres(y, 5200, rng)


def test_multi_through_the_two_read_route(storage):
    """M = 5200, T = 8, wide_pass_min = 3: the eight directions of an iteration are ONE chunk of the two-read route; every
    column at the project's 1e-4 bars against the f64 oracle, after its single fit met them."""
    be = storage
    be.gauss, be.knm_storage, be.wide_pass_min = "h2", "u24", 3
    X, y, idx = _wide_rows()
    K = _check_multi(be, X, label_columns(X, y, 8, seed=7), idx, 8.0, 1e-4)
    assert K.fmt == "u24" and be.ktkn_width(K) == 2 and be.ktkn_reads(K, 8) == 2


def test_path_through_the_two_read_route(storage):
    """The same rows and centres under 8 penalties: falkon_fit_path at the bars of test_path_on_the_reference_grid."""
    be = storage
    be.gauss, be.knm_storage, be.wide_pass_min = "h2", "u24", 3
    X, y, idx = _wide_rows()
    K = _check_path(be, X, y, idx, 8.0, [1e-6, 3e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3, 3e-3])
    assert K.fmt == "u24" and be.ktkn_width(K) == 2 and be.ktkn_reads(K, 8) == 2
