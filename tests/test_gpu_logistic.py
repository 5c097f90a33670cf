"""GPU tests of the logistic estimator: odx_knm_fwd_bwd_rw against the numpy f64 product, odx_logistic_rows_f64 against numpy /
scipy, and odx.LogisticFalkon against tests/logistic_ref.py in f64.  Every measured error is printed (profiles/logistic_falkon.md
quotes them)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -53


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


@pytest.fixture
def storage(be):
    old = (be.gauss, be.knm_storage, be.rw_one_read)
    yield be
    be.gauss, be.knm_storage, be.rw_one_read = old
    be.pin_gauss_tile(0)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ A. odx_knm_fwd_bwd_rw
def _rows_per_block(M):
    """R of the configuration knm_pass.hip's pick_cfg hands out for M columns, and its workgroups per CU."""
    chunks = (M + 3) // 4
    for cap, r, per_cu in ((256, 16, 2), (512, 8, 2), (1024, 4, 2), (2048, 4, 1), (2560, 4, 1), (3072, 2, 1), (5000, 1, 1)):
        if chunks <= cap:
            return r, per_cu
    raise ValueError(M)


def _block(rng, n, M, pad=8):
    """An f32-format block of n rows with ldk = roundup(M, 4) + pad: NaN in the columns past roundup(M, 4) and in two rows past
    n, zeros in [M, roundup(M, 4)).  Returns (Knm, the entries as f64)."""
    from odx.backend import Knm
    ld = (M + 3) // 4 * 4 + pad
    vals = (rng.random((n, M)) * np.exp(-3.0 * rng.random((n, M)))).astype(np.float32)
    vals[rng.random((n, M)) < 0.05] = 1.0
    buf = np.full((n + 2, ld), np.nan, dtype=np.float32)
    buf[:n, :M] = vals
    buf[:n, M:(M + 3) // 4 * 4] = 0.0
    K = Knm()
    K.K = torch.from_numpy(buf).cuda()
    K.n, K.M, K.ld, K.fmt = n, M, ld, "f32"
    return K, vals.astype(np.float64)


def _weights(rng, n):
    d = rng.standard_normal(n)
    d[rng.random(n) < 0.2] = 0.0
    d[rng.random(n) < 0.2] *= -1.0
    return d


def _check_rw(be, rng, n, M):
    lib = be.lib
    K, vals = _block(rng, n, M)
    v, d = rng.standard_normal(M), _weights(rng, n)
    vt, dt = torch.from_numpy(v).cuda(), torch.from_numpy(d).cuda()
    nbytes = int(lib.odx_knm_fwd_bwd_workspace_bytes(n, M))
    assert nbytes > 0

    def run(dvec, with_t):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
        out = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
        t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if with_t else None
        rc = lib.odx_knm_fwd_bwd_rw(_vp(K.K), K.ld, n, M, _vp(vt), _vp(dvec), _vp(out), _vp(t), _vp(ws), nbytes, None)
        assert rc == 0, lib.odx_last_error_string()
        return out.cpu().numpy(), None if t is None else t.cpu().numpy()

    out, t = run(dt, True)
    tref = vals @ v
    tb = (M + 2) * U * (np.abs(vals) @ np.abs(v))
    ref = vals.T @ (d * tref)
    ob = (M + n + 8) * U * (np.abs(vals).T @ (np.abs(d) * (np.abs(vals) @ np.abs(v))))
    et, eo = np.abs(t - tref), np.abs(out - ref)
    print("rw n=%d M=%d: out err / bound %.3f, t_out err / bound %.3f" % (n, M, float((eo / np.maximum(ob, 1e-300)).max()),
                                                                          float((et / np.maximum(tb, 1e-300)).max())))
    assert np.all(et <= tb) and np.all(eo <= ob)
    out2, _ = run(dt, False)
    assert np.array_equal(out, out2), "t_out changes out"
    out3, t3 = run(dt, True)
    assert np.array_equal(out, out3) and np.array_equal(t, t3), "two calls differ"
    ones, _ = run(torch.ones(n, dtype=torch.float64, device="cuda"), False)
    null, _ = run(None, False)
    assert np.array_equal(ones, null), "d = NULL is not a vector of ones"
    # the two-call route it replaces: agreement to the bound, and that route within the bound of the exact product too
    tt = torch.empty(n, dtype=torch.float64, device="cuda")
    be.ktk(K, v=vt, t_out=tt)
    two = be.ktk(K, w=dt * tt).cpu().numpy()
    assert np.all(np.abs(two - out) <= ob) and np.all(np.abs(two - ref) <= ob)
    # the backend's wrapper is the entry
    assert np.array_equal(be.ktk_rw(K, vt, dt).cpu().numpy(), out)


SMALL_M = [1, 7, 63, 65, 129, 257, 1000]
WIDE_M = [1500, 2500, 4100, 8200, 10300, 12300, 20000]   # one in every further configuration of pick_cfg, and the widest block


@pytest.mark.parametrize("M", SMALL_M + WIDE_M)
def test_rw_pass_against_numpy(be, M):
    """Componentwise: |out - ref| <= (M + n + 8) 2^-53 |K|' (|d| o (|K| |v|)), |t_out - K v| <= (M + 2) 2^-53 |K| |v|; the same
    bits with and without t_out, twice, and with d = NULL as with ones; the two-call route within the bound of it."""
    rng = np.random.default_rng(1000 + M)
    R, _ = _rows_per_block(M)
    ns = sorted({1, 31, 33, 300, max(1, R - 1), R + 1}) if M in SMALL_M else sorted({33, R + 1})
    for n in ns:
        _check_rw(be, rng, n, M)


@pytest.mark.parametrize("M", [257, 1500, 2500, 4100, 8200, 10300, 12300])
def test_rw_pass_with_several_blocks_per_workgroup(be, M):
    """More row blocks than workgroups: the persistent loop carries the next block's loads across its reduction."""
    R, per_cu = _rows_per_block(M)
    cus = int(be.lib.odx_device_cus())
    n = cus * per_cu * R * 2 + R + 1
    _check_rw(be, np.random.default_rng(2000 + M), n, M)


@pytest.mark.parametrize("poison", [0xFF, 0x5A])
@pytest.mark.parametrize("n,M", [(300, 129), (33, 4100), (40, 12300)])
def test_rw_workspace_is_held_to_its_reported_size(be, n, M, poison):
    from tests.workspace_guard import guarded
    rng = np.random.default_rng(n + M)
    K, vals = _block(rng, n, M)
    v, d = rng.standard_normal(M), _weights(rng, n)
    vt, dt = torch.from_numpy(v).cuda(), torch.from_numpy(d).cuda()
    plain = be.ktk_rw(K, vt, dt).cpu().numpy()
    with guarded(be, poison) as guard:
        out = be.ktk_rw(K, vt, dt).cpu().numpy()
        assert guard.asked() == {"odx_knm_fwd_bwd_workspace_bytes"} and guard.keys() == ["ktk"]
        guard.check()
    assert np.array_equal(out, plain)


def test_rw_argument_errors(be):
    lib = be.lib
    rng = np.random.default_rng(5)
    n, M = 20, 10
    K, _ = _block(rng, n, M)
    v = torch.zeros(M, dtype=torch.float64, device="cuda")
    out = torch.zeros(M, dtype=torch.float64, device="cuda")
    nbytes = int(lib.odx_knm_fwd_bwd_workspace_bytes(n, M))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def call(Kp=K.K, ldk=K.ld, n_=n, M_=M, v_=v, out_=out, ws_=ws, nb=nbytes):
        return lib.odx_knm_fwd_bwd_rw(_vp(Kp) if torch.is_tensor(Kp) else Kp, ldk, n_, M_, _vp(v_), None, _vp(out_), None, _vp(ws_), nb, None)
    assert call() == 0
    for bad in (dict(v_=None), dict(out_=None), dict(Kp=None), dict(ldk=K.ld + 2), dict(ldk=8), dict(M_=0),
                dict(Kp=ctypes.c_void_p(K.K.data_ptr() + 4))):
        assert call(**bad) != 0 and b"odx_knm_fwd_bwd_rw" in lib.odx_last_error_string(), bad
    assert call(nb=nbytes // 1024) != 0 and b"workspace" in lib.odx_last_error_string()
    assert call(ws_=None) != 0
    assert call(M_=20001, ldk=20004) != 0
    out.fill_(3.0)
    assert call(n_=0) == 0 and float(out.abs().max()) == 0.0
    # the wrapper's refusals
    from odx.backend import Knm
    S = Knm()
    S.n, S.M, S.fmt, S.cmap = n, M, "stream", None
    with pytest.raises(ValueError, match="stored"):
        be.ktk_rw(S, v, None)
    K.cmap = object()
    with pytest.raises(ValueError, match="column map"):
        be.ktk_rw(K, v, None)


# ------------------------------------------------------------------ B. odx_logistic_rows_f64
GRID_T = [0.0, 1e-300, 1e-8, 1.0, 30.0, 40.0, 700.0, 745.0, 1e4]


def _rows_case(be, t, y, nw, skip=None):
    from tests.logistic_ref import loss_terms
    n = len(t)
    tt, yt = torch.from_numpy(t).cuda(), torch.from_numpy(y).cuda()
    outs = [None if k == skip else torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for k in range(3)]
    be.logistic_rows(tt, yt, nw, outs[0], outs[1], outs[2])
    refs = loss_terms(y, t, nw)
    worst = 0.0
    for name, got, ref in zip("gwl", outs, refs):
        if got is None:
            continue
        got = got.cpu().numpy()
        assert np.all(np.isfinite(got)), name
        # 16 ulp: 16 x 2^-53 relative, and an ulp of a subnormal result is 2^-1074
        bound = 16.0 * np.maximum(U * np.abs(ref), 2.0 ** -1074)
        err = np.abs(got - ref)
        worst = max(worst, float((err / bound).max()) * 16.0)
        k = int(np.argmax(err / bound))
        assert np.all(err <= bound), (name, nw, "t = %r, y = %g: got %r, reference %r" % (t[k], y[k], got[k], ref[k]))
    return worst


@pytest.mark.parametrize("nw", [1.0, 0.25, 4.0])
def test_logistic_rows_against_numpy(be, nw):
    """g, w and l within 16 ulp of numpy's (np.logaddexp, scipy.special.expit) per element — the ulp bounds the device library
    is held to for exp (3) and log1p (2) through at most four further roundings — on the grid of scores, on random ones, at
    the lengths around a workgroup, and with each output left out."""
    rng = np.random.default_rng(int(nw * 100))
    grid = np.array([s * t for t in GRID_T for s in (1.0, -1.0)])
    worst = 0.0
    for ysign in (1.0, -1.0):
        worst = max(worst, _rows_case(be, grid, np.full(len(grid), ysign), nw))
    t = np.concatenate([rng.standard_normal(5000) * 3.0, rng.standard_normal(4000) * 40.0, (rng.random(1000) - 0.5) * 1600.0])
    y = np.where(rng.random(len(t)) < 0.1, 1.0, -1.0)
    worst = max(worst, _rows_case(be, t, y, nw))
    for n in (1, 63, 65, 1000):
        worst = max(worst, _rows_case(be, t[:n].copy(), y[:n].copy(), nw))
    for skip in range(3):
        _rows_case(be, t[:65].copy(), y[:65].copy(), nw, skip=skip)
    print("logistic_rows neg_weight=%g: worst error %.2f ulp" % (nw, worst))


# ------------------------------------------------------------------ C. odx.LogisticFalkon end to end
SHAPES = [(777, 129, 36, 5.0, 1e-3), (1500, 257, 70, 5.0, 1e-4), (3000, 300, 1024, 15.0, 1e-5)]        # tests/test_gpu_incremental.py
SCHEDULES = {
    "A": [(1e-1, 3), (1e-2, 3), (1e-3, 3), (1e-4, 8), (1e-4, 8), (1e-4, 8)],
    "B": [(1e-2, 3), (1e-3, 3), (1e-4, 5), (1e-5, 8), (1e-5, 8)],
    "C": [(1e-3, 4), (1e-5, 4), (1e-6, 10), (1e-6, 10)],
}
_problems, _refs = {}, {}


def _problem(n, M, D):
    if (n, M, D) not in _problems:
        from tests.synth import blob_problem
        X, y, rng = blob_problem(n, D, seed=500 + n)
        _problems[(n, M, D)] = (X, y.astype(np.float64), np.sort(rng.choice(n, M, replace=False)))
    return _problems[(n, M, D)]


def _reference(n, M, D, kernel, name, nw):
    """(alpha, scores of the rows) of logistic_ref in f64, once per case."""
    key = (n, M, D, repr(kernel), name, nw)
    if key not in _refs:
        from tests import logistic_ref as lr
        from tests.matern_ref import radial_kernel
        X, y, idx = _problem(n, M, D)
        X64 = X.astype(np.float64)
        sched = SCHEDULES[name]
        a = lr.logistic_fit(X64, y, X64[idx], y[idx], kernel, [p for p, _ in sched], [m for _, m in sched], nw, kernel=radial_kernel)
        _refs[key] = (a, radial_kernel(X64, X64[idx], kernel, np.float64) @ a)
    return _refs[key]


class _Pick:
    def __init__(self, idx):
        self.idx = torch.from_numpy(np.asarray(idx))

    def select(self, X, Y):
        i = self.idx.to(X.device)
        return X[i], Y[i]


def _fit_and_check(n, M, D, kernel, name, nw, what):
    import odx
    X, y, idx = _problem(n, M, D)
    sched = SCHEDULES[name]
    karg = getattr(kernel, "sigma", kernel)
    ref_a, ref_s = _reference(n, M, D, kernel if hasattr(kernel, "nu") else float(karg), name, nw)
    est = odx.LogisticFalkon(kernel if hasattr(kernel, "sigma") else odx.GaussianKernel(kernel), [p for p, _ in sched],
                             [m for _, m in sched], loss=odx.LogisticLoss(nw), center_selection=_Pick(idx))
    Xt = torch.from_numpy(X).cuda()
    est.fit(Xt, torch.from_numpy(y))
    a = est.alpha_.cpu().numpy()
    s = est.predict(Xt).cpu().numpy().astype(np.float64)
    r = float(np.linalg.norm(a - ref_a) / np.linalg.norm(ref_a))
    e, top = float(np.abs(s - ref_s).max()), float(np.abs(ref_s).max())
    print("logistic %s n=%d M=%d %s nw=%g: alpha rel err %.2e, score err %.2e (max |ref| %.2f)" % (what, n, M, name, nw, r, e, top))
    assert r < 1e-4 and e < 1e-4 * max(1.0, top), (r, e, top)
    return est


@pytest.mark.parametrize("nw", [1.0, 0.25])
@pytest.mark.parametrize("name", ["A", "C"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d" % s[:2])
def test_logistic_fit_is_the_reference(be, storage, shape, name, nw, monkeypatch):
    """An f32 block: every Hessian product, the periodic full residuals included, is one odx_knm_fwd_bwd_rw."""
    n, M, D, sigma, _ = shape
    entries = []
    call = be._call
    monkeypatch.setattr(be, "_call", lambda entry, *a: (entries.append(entry), call(entry, *a))[1])
    _fit_and_check(n, M, D, sigma, name, nw, "f32")
    monkeypatch.undo()
    assert entries.count("odx_knm_fwd_bwd_rw") == sum(m + (m - 1) // 10 for _, m in SCHEDULES[name])
    assert "odx_knm_fwd_bwdn_q_rw" not in entries


def test_logistic_fit_on_a_24_bit_block(be, storage, monkeypatch):
    """The block forced to the 24-bit format: every Hessian product is one odx_knm_fwd_bwdn_q_rw."""
    be.gauss, be.knm_storage = "h2", "u24"
    be.pin_gauss_tile(256)
    entries = []
    call = be._call
    monkeypatch.setattr(be, "_call", lambda entry, *a: (entries.append(entry), call(entry, *a))[1])
    n, M, D, sigma, _ = SHAPES[2]
    _fit_and_check(n, M, D, sigma, "A", 0.25, "u24")
    monkeypatch.undo()
    its = sum(m for _, m in SCHEDULES["A"])
    assert entries.count("odx_knm_fwd_bwdn_q_rw") == its and "odx_knm_fwd_bwd_rw" not in entries


def test_logistic_fit_above_the_lds_limit(be, storage, monkeypatch):
    """M = 5200 on a 24-bit block: no one-read weighted pass exists, every Hessian product takes the two-read route."""
    be.gauss, be.knm_storage = "h2", "u24"
    be.pin_gauss_tile(256)
    entries = []
    call = be._call
    monkeypatch.setattr(be, "_call", lambda entry, *a: (entries.append(entry), call(entry, *a))[1])
    _fit_and_check(6000, 5200, 70, 5.0, "B", 1.0, "u24 two reads")
    monkeypatch.undo()
    its = sum(m for _, m in SCHEDULES["B"])
    assert entries.count("odx_knm_fwdn_q") == its and entries.count("odx_knm_bwdn_q") == its


def test_logistic_fit_with_a_matern_kernel(be, storage):
    import odx
    n, M, D, sigma, _ = SHAPES[1]
    _fit_and_check(n, M, D, odx.MaternKernel(sigma, 2.5), "A", 0.25, "matern 5/2")


def test_logistic_f32_route_without_the_new_kernel(be, storage):
    """rw_one_read = False: the f32 block through ktkn_rows' two-call route, the same bars."""
    be.rw_one_read = False
    n, M, D, sigma, _ = SHAPES[1]
    _fit_and_check(n, M, D, sigma, "C", 1.0, "f32 two calls")


def test_predict_path_and_proba_over_two_logistic_models(be, storage):
    import odx
    n, M, D, sigma, _ = SHAPES[0]
    X, y, idx = _problem(n, M, D)
    Xt = torch.from_numpy(X).cuda()
    a = _fit_and_check(n, M, D, sigma, "A", 1.0, "path member")
    b = odx.LogisticFalkon(odx.GaussianKernel(sigma), [1e-2, 1e-3], [3, 5], loss=odx.LogisticLoss(0.25), center_selection=_Pick(idx),
                           record_objective=True).fit(Xt, torch.from_numpy(y))
    assert len(b.objective_) == 3 and all(q <= p for p, q in zip(b.objective_, b.objective_[1:])), b.objective_
    b.ny_points_ = a.ny_points_          # (the same centres: predict_path asks for one tensor)
    both = odx.predict_path([a, b], Xt)
    assert torch.equal(both[:, :1], a.predict(Xt)) and torch.equal(both[:, 1:], b.predict(Xt))
    assert torch.equal(a.predict_proba(Xt), torch.sigmoid(a.predict(Xt)))
