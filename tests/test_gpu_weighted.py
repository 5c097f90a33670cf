"""GPU tests of the sample-weighted fit: odx_knm_fwd_bwd_q_rw (csrc/knm_pass_q_rw.hip) against the numpy f64 product on synthetic
24-bit and bf16 planes, HipBackend.ktk_w's routes, odx.falkon_fit_weighted against tests/weighted_ref.py in f64 on the block the
GPU built, the scores summed from the CG, and odx.Falkon(weight_fn=...).  Every measured error is printed
(profiles/weighted_falkon.md quotes them)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53
FMTS = ["u24", "bf16"]


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def storage(be):
    old = (be.gauss, be.knm_storage, be.rw_q_min_columns)
    yield be
    be.gauss, be.knm_storage, be.rw_q_min_columns = old
    be.pin_gauss_tile(0)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ A. odx_knm_fwd_bwd_q_rw
def _cfg(M):
    """(R, workgroups per CU) of the configuration knm_pass_q_rw.hip's pick_qrwcfg hands out for M columns."""
    chunks = (M + 3) // 4
    for cap, r, per_cu in ((256, 16, 2), (512, 8, 2), (1024, 4, 2), (2048, 3, 2), (2560, 6, 1), (3072, 4, 1), (5110, 1, 1)):
        if chunks <= cap:
            return r, per_cu
    raise ValueError(M)


def _need(be, n, M):
    """The bytes of workspace the entry needs: a slab of roundup(M, 4) doubles per workgroup (include/odx.h)."""
    R, per_cu = _cfg(M)
    return min(int(be.lib.odx_device_cus()) * per_cu, (n + R - 1) // R) * ((M + 3) // 4 * 4) * 8


def _block(rng, n, M, fmt, pad=8):
    """A compact block of n rows with ld = roundup(M, 8) + pad as the build stores it (24-bit codes with both extremes, or
    bf16 patterns of values in [0, 1)), TWICE: `poisoned` with 0xFF bytes in every pad column [M, ld) and in two rows past n
    (a NaN pattern in bf16, the largest code in 24 bits), `clean` with zeros there (what the builds leave, and what the older
    passes need).  Returns (poisoned, clean, the entries as f64)."""
    from odx.backend import Knm
    ld = (M + 7) // 8 * 8 + pad
    if fmt == "u24":
        codes = rng.integers(0, 1 << 24, (n, M), dtype=np.int64)
        codes[0, 0], codes[-1, M - 1] = (1 << 24) - 1, 0
        vals = codes.astype(np.float64) * 2.0 ** -24
    else:
        codes = (rng.random((n, M)).astype(np.float32).view(np.uint32) >> 16).astype(np.int64)
        vals = (codes.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    out = []
    for fill in (0xFF, 0x00):
        hi = np.full((n + 2, ld), fill * 0x0101, dtype=np.uint16)
        lo = np.full((n + 2, ld), fill, dtype=np.uint8)
        if fmt == "u24":
            hi[:n, :M], lo[:n, :M] = (codes >> 8).astype(np.uint16), (codes & 255).astype(np.uint8)
        else:
            hi[:n, :M] = codes.astype(np.uint16)
        K = Knm()
        K.n, K.M, K.ld, K.fmt = n + 2, M, ld, fmt
        K.K = torch.from_numpy(hi.view(np.int16)).cuda()
        K.lo = torch.from_numpy(lo).cuda() if fmt == "u24" else None
        out.append(K.rows(0, n))
    return out[0], out[1], vals


def _weights(rng, n):
    d = rng.standard_normal(n)
    d[rng.random(n) < 0.2] = 0.0
    d[rng.random(n) < 0.2] *= -1.0
    return d


def _entry(be, K, v, d, t, ws, nbytes, out):
    from odx import hip
    return be.lib.odx_knm_fwd_bwd_q_rw(_vp(K.K), K.ld, _vp(K.lo), K.ld, hip.KNM_CODE[K.fmt], K.n, K.M, _vp(v), _vp(d), _vp(out), _vp(t),
                                       _vp(ws), nbytes, None)


def _check_q_rw(be, rng, n, M, fmt):
    from odx import hip
    lib = be.lib
    K, K0, vals = _block(rng, n, M, fmt)
    v, d = rng.standard_normal(M), _weights(rng, n)
    vt, dt = torch.from_numpy(v).cuda(), torch.from_numpy(d).cuda()
    nbytes = int(lib.odx_knm_fwd_bwd_q_workspace_bytes(n, M, hip.KNM_CODE[fmt]))
    assert nbytes >= _need(be, n, M) > 0

    def run(dvec, with_t):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        out = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
        t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if with_t else None
        rc = _entry(be, K, vt, dvec, t, ws, nbytes, out)
        assert rc == 0, lib.odx_last_error_string()
        return out.cpu().numpy(), None if t is None else t.cpu().numpy()

    out, t = run(dt, True)
    tref = vals @ v
    tb = (M + 2) * U * (np.abs(vals) @ np.abs(v))
    ref = vals.T @ (d * tref)
    ob = (M + n + 8) * U * (np.abs(vals).T @ (np.abs(d) * (np.abs(vals) @ np.abs(v))))
    et, eo = np.abs(t - tref), np.abs(out - ref)
    print("q_rw %s n=%d M=%d: out err / bound %.2e, t_out err / bound %.2e" % (fmt, n, M, float((eo / np.maximum(ob, 1e-300)).max()),
                                                                               float((et / np.maximum(tb, 1e-300)).max())))
    assert np.all(et <= tb) and np.all(eo <= ob)          # (a NaN from the pad fails both)
    out2, _ = run(dt, False)
    assert np.array_equal(out, out2), "t_out changes out"
    out3, t3 = run(dt, True)
    assert np.array_equal(out, out3) and np.array_equal(t, t3), "two calls differ"
    ones, _ = run(torch.ones(n, dtype=torch.float64, device="cuda"), False)
    null, _ = run(None, False)
    assert np.array_equal(ones, null), "d = NULL is not a vector of ones"
    # the route it replaces (on the block with the zero pad the older passes need): agreement to the bound, and that route
    # within the bound of the exact product too
    two = be.ktk_rw(K0, vt, dt).cpu().numpy()
    assert np.all(np.abs(two - out) <= ob) and np.all(np.abs(two - ref) <= ob)
    # the backend's wrapper is the entry
    old, be.rw_q_min_columns = be.rw_q_min_columns, 1
    try:
        tw = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        assert np.array_equal(be.ktk_w(K, vt, dt, t_out=tw).cpu().numpy(), out) and np.array_equal(tw.cpu().numpy(), t)
    finally:
        be.rw_q_min_columns = old


# both sides of every switch of pick_qrwcfg (chunks 256 | 512 | 1024 | 2048 | 2560 | 3072), the widths around the NV pass's
# limit (5084) and the widest block
SMALL_M = [1, 7, 63, 65, 257, 1000]
WIDE_M = [1024, 1025, 2048, 2049, 4096, 4097, 5088, 5200, 8192, 8193, 10239, 10240, 10241, 12288, 12289, 20440]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M", SMALL_M + WIDE_M)
def test_q_rw_pass_against_numpy(be, M, fmt):
    """Componentwise: |out - ref| <= (M + n + 8) 2^-53 |K|' (|d| o (|K| |v|)), |t_out - K v| <= (M + 2) 2^-53 |K| |v| — the
    bounds of tests/test_gpu_logistic.py for the f32 twin: a row dot is M products and M - 1 + log2 additions of exactly
    decoded entries, a column sum n more —; the same bits with and without t_out, twice, and with d = NULL as with ones;
    ktk_rw within the bound of it.  Pad columns and the rows past n hold 0xFF bytes."""
    rng = np.random.default_rng(3000 + M + (fmt == "bf16"))
    R, _ = _cfg(M)
    ns = sorted({1, 33, 300, max(1, R - 1), R + 1}) if M in SMALL_M else sorted({33, R + 1})
    for n in ns:
        _check_q_rw(be, rng, n, M, fmt)


@pytest.mark.parametrize("M,fmt", [(1000, "u24"), (2000, "bf16"), (4000, "u24"), (8000, "bf16"), (10000, "u24"), (12000, "bf16"),
                                   (20440, "u24")])
def test_q_rw_pass_with_several_blocks_per_workgroup(be, M, fmt):
    """More row blocks than workgroups, one width per configuration: the persistent loop carries the next block's loads and
    descriptors across its reduction, and the last block is a partial one."""
    R, per_cu = _cfg(M)
    cus = int(be.lib.odx_device_cus())
    n = cus * per_cu * R * 2 + R + 1
    _check_q_rw(be, np.random.default_rng(4000 + M), n, M, fmt)


def test_q_rw_unsupported_width(be):
    from odx import hip
    rng = np.random.default_rng(7)
    M = 20441
    K, _, _ = _block(rng, 3, M, "u24")
    v = torch.zeros(M, dtype=torch.float64, device="cuda")
    out = torch.zeros(M, dtype=torch.float64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    assert _entry(be, K, v, None, None, ws, ws.numel(), out) == -3          # ODX_ERR_UNSUPPORTED (include/odx.h)
    assert b"odx_knm_fwd_bwd_q_rw" in be.lib.odx_last_error_string()
    assert be.lib.odx_knm_fwd_bwd_q_workspace_bytes(3, M, hip.KNM_CODE["u24"]) < 0
    with pytest.raises(hip.OdxError):
        old, be.rw_q_min_columns = be.rw_q_min_columns, 1
        try:
            be.ktk_w(K, v, None)
        finally:
            be.rw_q_min_columns = old


# ------------------------------------------------------------------ C. the workspace, the argument errors
@pytest.mark.parametrize("poison", [0xFF, 0x5A])
@pytest.mark.parametrize("n,M,fmt", [(300, 129, "u24"), (33, 5200, "bf16"), (40, 12300, "u24")])
def test_q_rw_workspace_is_held_to_its_size(be, n, M, fmt, poison):
    """Through the wrapper: the one query asked is odx_knm_fwd_bwd_q_workspace_bytes and nothing is written outside what it
    reported.  At the entry: with exactly the bytes its slabs take (include/odx.h: min(CUs x workgroups per CU, row blocks)
    x roundup(M, 4) doubles) between two poisoned bands, the same bits and both bands intact; with 8 bytes less,
    ODX_ERR_WORKSPACE."""
    from tests.workspace_guard import GUARD, guarded
    rng = np.random.default_rng(n + M)
    K, _, vals = _block(rng, n, M, fmt)
    v, d = rng.standard_normal(M), _weights(rng, n)
    vt, dt = torch.from_numpy(v).cuda(), torch.from_numpy(d).cuda()
    old, be.rw_q_min_columns = be.rw_q_min_columns, 1
    try:
        plain = be.ktk_w(K, vt, dt).cpu().numpy()
        with guarded(be, poison) as guard:
            out = be.ktk_w(K, vt, dt).cpu().numpy()
            assert guard.asked() == {"odx_knm_fwd_bwd_q_workspace_bytes"} and guard.keys() == ["ktk"]
            guard.check()
    finally:
        be.rw_q_min_columns = old
    assert np.array_equal(out, plain)
    need = _need(be, n, M)
    buf = torch.full((GUARD + need + GUARD,), poison, dtype=torch.uint8, device="cuda")
    o = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    assert _entry(be, K, vt, dt, None, buf[GUARD:GUARD + need], need, o) == 0, be.lib.odx_last_error_string()
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), plain)
    assert bool((buf[:GUARD] == poison).all()) and bool((buf[GUARD + need:] == poison).all())
    assert _entry(be, K, vt, dt, None, buf[GUARD:GUARD + need], need - 8, o) == -4          # ODX_ERR_WORKSPACE
    assert b"workspace" in be.lib.odx_last_error_string()


def test_q_rw_argument_errors(be):
    from odx import hip
    lib = be.lib
    rng = np.random.default_rng(5)
    n, M = 20, 10
    K, _, _ = _block(rng, n, M, "u24")
    v = torch.zeros(M, dtype=torch.float64, device="cuda")
    out = torch.zeros(M, dtype=torch.float64, device="cuda")
    nbytes = int(lib.odx_knm_fwd_bwd_q_workspace_bytes(n, M, hip.KNM_CODE["u24"]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call(Kp=K.K, ldk=K.ld, lo=K.lo, ldlo=K.ld, fmt=hip.KNM_CODE["u24"], n_=n, M_=M, v_=v, out_=out, ws_=ws, nb=nbytes):
        as_p = lambda x: _vp(x) if torch.is_tensor(x) else x          # noqa: E731
        return lib.odx_knm_fwd_bwd_q_rw(as_p(Kp), ldk, as_p(lo), ldlo, fmt, n_, M_, _vp(v_), None, _vp(out_), None, _vp(ws_), nb, None)
    assert call() == 0
    for bad in (dict(v_=None), dict(out_=None), dict(Kp=None), dict(lo=None), dict(ldk=K.ld + 2), dict(ldk=8), dict(ldlo=8), dict(M_=0),
                dict(fmt=0), dict(fmt=3), dict(Kp=ctypes.c_void_p(K.K.data_ptr() + 4)), dict(lo=ctypes.c_void_p(K.lo.data_ptr() + 2))):
        assert call(**bad) == -1 and b"odx_knm_fwd_bwd_q_rw" in lib.odx_last_error_string(), bad          # ODX_ERR_INVALID
    assert call(nb=nbytes // 1024) == -4 and b"workspace" in lib.odx_last_error_string()
    assert call(ws_=None) == -4
    assert call(fmt=hip.KNM_CODE["bf16"], lo=None, ldlo=0) == 0          # bf16 has no low-byte plane
    out.fill_(3.0)
    assert call(n_=0) == 0 and float(out.abs().max()) == 0.0
    # the wrapper's refusals and routes
    from odx.backend import Knm
    S = Knm()
    S.n, S.M, S.fmt, S.cmap = n, M, "stream", None
    with pytest.raises(ValueError, match="stored"):
        be.ktk_w(S, v, None)
    with pytest.raises(ValueError, match="contiguous f64"):
        be.ktk_w(K, v.float(), None)
    K.cmap = object()
    with pytest.raises(ValueError, match="column map"):
        be.ktk_w(K, v, None)


def test_ktk_w_routes_by_format_and_width(be, monkeypatch):
    """f32 blocks: odx_knm_fwd_bwd_rw; compact blocks from rw_q_min_columns columns on: the new entry; narrower ones, and
    every width with rw_q_min_columns = None: ktk_rw (odx_knm_fwd_bwdn_q_rw up to M = 5084, the two-read pair above)."""
    from tests.test_gpu_logistic import _block as f32_block
    rng = np.random.default_rng(11)
    entries = []
    call = be._call
    monkeypatch.setattr(be, "_call", lambda entry, *a: (entries.append(entry), call(entry, *a))[1])
    assert be.rw_q_min_columns == 5085

    def route(K, v):
        del entries[:]
        be.ktk_w(K, v, None)
        return list(entries)
    Kf, _ = f32_block(rng, 33, 300)
    assert route(Kf, torch.zeros(300, dtype=torch.float64, device="cuda")) == ["odx_knm_fwd_bwd_rw"]
    for M, want in ((5084, ["odx_knm_fwd_bwdn_q_rw"]), (5085, ["odx_knm_fwd_bwd_q_rw"])):
        _, K0, vals = _block(rng, 9, M, "u24")
        vn = rng.standard_normal(M)
        v = torch.from_numpy(vn).cuda()
        ob = torch.from_numpy((M + 9 + 8) * U * (np.abs(vals).T @ (np.abs(vals) @ np.abs(vn))))
        assert route(K0, v) == want, M
        first = be.ktk_w(K0, v, None).clone()
        be.rw_q_min_columns = None
        try:
            off = route(K0, v)
            assert off == (["odx_knm_fwdn_q", "odx_knm_bwdn_q"] if M > 5084 else want), (M, off)
            other = be.ktk_w(K0, v, None)
        finally:
            be.rw_q_min_columns = 5085
        assert bool(((first - other).abs().cpu() <= 2 * ob).all())          # each within the bound of the exact product


# ------------------------------------------------------------------ D. odx.falkon_fit_weighted against tests/weighted_ref.py
SHAPES = [(777, 129, 36, 5.0, 1e-3), (1500, 257, 70, 5.0, 1e-4), (3000, 300, 1024, 15.0, 1e-5)]        # tests/test_gpu_logistic.py
WIDE = (6000, 5200, 70, 5.0, 1e-4)
_problems, _refs = {}, {}


def _problem(n, M, D):
    """(X f32, y f64, centre indices, row weights): blob_problem's rows, M distinct centres, weights (9 on the positives, 1
    otherwise) x U(0.5, 1.5) with a few exact zeros."""
    if (n, M, D) not in _problems:
        from tests.synth import blob_problem
        X, y, rng = blob_problem(n, D, seed=500 + n)
        idx = np.sort(rng.choice(n, M, replace=False))
        w = np.where(y > 0, 9.0, 1.0) * rng.uniform(0.5, 1.5, n)
        w[rng.random(n) < 0.02] = 0.0
        _problems[(n, M, D)] = (X, y.astype(np.float64), idx, w)
    return _problems[(n, M, D)]


def _fit(be, shape, kernel, scores=False):
    """(alpha, the block, scores_out or None) of odx.falkon_fit_weighted at a shape of SHAPES / WIDE."""
    import odx
    from odx.falkon import _kernel_arg
    n, M, D, _, lam = shape
    X, y, idx, w = _problem(n, M, D)
    F = be.features(torch.from_numpy(X).cuda())
    Zf = be.rows(F, torch.from_numpy(idx))
    S = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if scores else None
    Ks = []
    alpha = odx.falkon_fit_weighted(be, F, be.vec(y), be.vec(w), Zf, be.vec(w[idx]), _kernel_arg(kernel), lam, 20, scores_out=S,
                                    knm_blocks=Ks)
    return alpha, Ks[0], S


def _reference(shape, kernel, K):
    """alpha of weighted_ref in f64 on the entries of the block the GPU built, once per (shape, kernel, storage)."""
    key = (shape, repr(kernel), K.fmt)
    if key not in _refs:
        from tests import weighted_ref as wr
        n, M, D, _, lam = shape
        X, y, idx, w = _problem(n, M, D)
        X64 = X.astype(np.float64)
        karg = kernel if hasattr(kernel, "nu") else float(kernel.sigma)
        _refs[key] = wr.weighted_fit(X64, y, w, X64[idx], w[idx], karg, lam, 20, knm=K.dense().double().cpu().numpy())[:, 0]
    return _refs[key]


def _fit_and_check(be, shape, kernel, what, fmt):
    alpha, K, _ = _fit(be, shape, kernel)
    assert K.fmt == fmt, K.fmt
    ref = _reference(shape, kernel, K)
    r = float(np.linalg.norm(alpha.cpu().numpy() - ref) / np.linalg.norm(ref))
    print("weighted %s n=%d M=%d: alpha rel err %.2e" % (what, shape[0], shape[1], r))
    assert r < 1e-4, r
    return alpha


def _recorded(be, monkeypatch):
    entries = []
    call = be._call
    monkeypatch.setattr(be, "_call", lambda entry, *a: (entries.append(entry), call(entry, *a))[1])
    return entries


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d" % s[:2])
def test_weighted_fit_is_the_reference_on_f32_blocks(be, storage, shape, monkeypatch):
    import odx
    entries = _recorded(be, monkeypatch)
    _fit_and_check(be, shape, odx.GaussianKernel(shape[3]), "f32", "f32")
    assert entries.count("odx_knm_fwd_bwd_rw") == 21 and "odx_knm_fwd_bwd_q_rw" not in entries


def test_weighted_fit_on_a_small_24_bit_block(be, storage, monkeypatch):
    """The block forced to the 24-bit format below rw_q_min_columns: every product is one odx_knm_fwd_bwdn_q_rw."""
    import odx
    be.gauss, be.knm_storage = "h2", "u24"
    be.pin_gauss_tile(256)
    entries = _recorded(be, monkeypatch)
    _fit_and_check(be, SHAPES[2], odx.GaussianKernel(SHAPES[2][3]), "u24 narrow", "u24")
    assert entries.count("odx_knm_fwd_bwdn_q_rw") == 21 and "odx_knm_fwd_bwd_q_rw" not in entries


def test_weighted_fit_with_a_matern_kernel(be, storage):
    import odx
    _fit_and_check(be, SHAPES[1], odx.MaternKernel(SHAPES[1][3], 2.5), "matern 5/2", "f32")


def test_weighted_fit_above_the_nv_limit_reads_the_block_once_per_product(be, storage, monkeypatch):
    """M = 5200 on a 24-bit block: 21 odx_knm_fwd_bwd_q_rw and no two-read pair; with rw_q_min_columns = None the other way
    round, under the same bar and against the same reference."""
    import odx
    be.gauss, be.knm_storage = "h2", "u24"
    be.pin_gauss_tile(256)
    kernel = odx.GaussianKernel(WIDE[3])
    entries = _recorded(be, monkeypatch)
    a1 = _fit_and_check(be, WIDE, kernel, "u24 one read", "u24")
    assert entries.count("odx_knm_fwd_bwd_q_rw") == 21
    assert entries.count("odx_knm_fwdn_q") == 0 and entries.count("odx_knm_bwdn_q") == 0
    del entries[:]
    be.rw_q_min_columns = None
    a2 = _fit_and_check(be, WIDE, kernel, "u24 two reads", "u24")
    assert entries.count("odx_knm_fwd_bwd_q_rw") == 0
    assert entries.count("odx_knm_fwdn_q") == 21 and entries.count("odx_knm_bwdn_q") == 21
    print("weighted one read vs two reads: alpha rel diff %.2e" % float((a1 - a2).norm() / a2.norm()))


# ------------------------------------------------------------------ E. scores_out
@pytest.mark.parametrize("case", ["f32", "u24-wide"])
def test_scores_out_is_knm_mv_of_alpha(be, storage, case):
    """scores_out, summed from the passes' UNWEIGHTED row products, against knm_mv of the same block and alpha, in the form of
    tests/test_scores_from_cg.py: both are f64 sums of 20 products rounded once to f32 — one f32 ulp where the two straddle
    a rounding boundary plus 1e-9 of the scale for the f64 sums' own difference; and asking for them changes nothing."""
    import odx
    shape = SHAPES[2] if case == "f32" else WIDE
    if case != "f32":
        be.gauss, be.knm_storage = "h2", "u24"
        be.pin_gauss_tile(256)
    kernel = odx.GaussianKernel(shape[3])
    alpha, K, S = _fit(be, shape, kernel, scores=True)
    plain, _, _ = _fit(be, shape, kernel)
    assert torch.equal(alpha, plain)
    got = torch.empty((shape[0], 1), dtype=torch.float32, device="cuda")
    be.cg_scores_store(S, got)
    want = be.knm_mv(K, alpha)
    d = (got.double() - want.double()).abs().cpu()
    scale = max(1.0, float(want.abs().max()))
    tol = torch.from_numpy(np.spacing(want.abs().cpu().numpy())).double() + 1e-9 * scale
    print("weighted scores_out %s: max |scores(CG) - knm_mv| = %.3e at scale %.3e" % (case, float(d.max()), scale))
    assert bool((d <= tol).all()), float((d / tol).max())
    assert float(want.abs().max()) > 0


# ------------------------------------------------------------------ F. the estimator
class _Pick:
    def __init__(self, idx):
        self.idx = torch.from_numpy(np.asarray(idx))

    def select(self, X, Y):
        i = self.idx.to(X.device)
        return X[i] if Y is None else (X[i], Y[i], self.idx)


def _pos9(Y, X, indices):
    return torch.where(torch.as_tensor(Y).reshape(-1) > 0, 9.0, 1.0)


@pytest.mark.parametrize("cls", ["Falkon", "InCoreFalkon"])
def test_estimator_with_weight_fn(be, storage, cls):
    """odx.Falkon(weight_fn=...) against weight_fn=None on the same centres, at the shape of tests/test_weighted_host.py's
    oracle check (blob_problem(3000, 64, 7), M = 300, sigma = 15, lam = 1e-3, 9 on the positives): the models differ by more
    than 0.1 relative, that check's bar for the same statement, and predict agrees with the f64 reference's scores (the bar of
    tests/test_gpu_logistic.py: 1e-4 of max(1, the largest score))."""
    import odx
    from tests import weighted_ref as wr
    from tests.matern_ref import radial_kernel
    from tests.synth import blob_problem
    n, M, D, sigma, lam = 3000, 300, 64, 15.0, 1e-3
    X, y, rng = blob_problem(n, D, 7)
    y = y.astype(np.float64)
    idx = np.sort(rng.choice(n, M, replace=False))
    w = np.where(y > 0, 9.0, 1.0)
    Xt = torch.from_numpy(X).cuda() if cls == "InCoreFalkon" else torch.from_numpy(X)
    make = lambda **kw: getattr(odx, cls)(odx.GaussianKernel(sigma), lam, None, center_selection=_Pick(idx), **kw)      # noqa: E731
    est = make(weight_fn=_pos9).fit(Xt, torch.from_numpy(y))
    plain = make().fit(Xt, torch.from_numpy(y))
    diff = float((est.alpha_.double().cpu() - plain.alpha_.double().cpu()).norm() / plain.alpha_.double().cpu().norm())
    X64 = X.astype(np.float64)
    ref = wr.weighted_fit(X64, y, w, X64[idx], w[idx], sigma, lam, 20)
    ref_s = radial_kernel(X64, X64[idx], sigma, np.float64) @ ref
    s = est.predict(Xt).cpu().numpy().astype(np.float64)
    r = float(np.linalg.norm(est.alpha_.cpu().numpy() - ref) / np.linalg.norm(ref))
    e, top = float(np.abs(s - ref_s).max()), float(np.abs(ref_s).max())
    print("weighted %s: alpha vs unweighted %.2e, alpha rel err vs f64 %.2e, score err %.2e (max |ref| %.2f)" % (cls, diff, r, e, top))
    assert diff > 0.1
    assert e < 1e-4 * max(1.0, top), (r, e, top)
    assert est.alpha_.is_cuda == (cls == "InCoreFalkon")
