"""The RLS kernels (csrc/rls.hip) on the MI355X, entry by entry against the f64 references and rounding bounds of
tests/rls_checks.py (numpy / scipy; tests/test_rls_checks_host.py shows what those bounds reject): the Grams straight from the f32
rows at every tile edge of rls_gram_rows32_kernel, the raw targets' products riding along, rows outside every class that hold
Inf / NaN, the X'Y sweep, the NT route, the one-class entry, the whitening fold, the solves (block substitution and explicit
inverse) by their backward error against scipy's Cholesky on the same systems, and the predictions.  Row counts are tiny on
purpose: the edges are in D and in len mod 32.  Every test prints its largest error / bound ratio (profiles/rls_kernels.md)."""
import ctypes

import numpy as np
import pytest

from tests import rls_checks as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i64s(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def _even(n):
    return (n + 1) // 2 * 2


def _batch(D, C, i=0, seed=0):
    return rc.Batch(D, rc.class_lengths(C, k=3 * i + 1 if C < 32 else 0), seed=1000 * D + C + seed)


def _idx_pad(be, b):
    """The padded row-id array from odx_rls_pad_index (and that it is the one stated in numpy)."""
    idx_pad = be.rls_pad_index(dev(b.run), b.seg_off, b.lengths, b.npad)[0]
    assert np.array_equal(idx_pad.cpu().numpy(), b.idx_pad)
    return idx_pad


def _report(family, **kv):
    print("rls_kernels %s %s" % (family, " ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kv.items())))


def _prefill(rng, C, D):
    D1 = D + 1
    return rng.standard_normal((C, D1, _even(D1)))


def _check_gram_block(b, G1, G0, what):
    """The D x D lower triangles against gram_ref; the bias row, the bias column and the pad column untouched.  Returns the ratio."""
    D, worst = b.D, 0.0
    for c in range(b.C):
        ref, bound = rc.gram_ref(b.X, b.rows[c])
        r = rc.tril_ratio(G1[c, :D, :D], G0[c, :D, :D], ref, bound)
        assert r <= 1.0, (what, "class", c, "len", b.lengths[c], r)
        worst = max(worst, r)
        assert np.array_equal(G1[c, D, :], G0[c, D, :]), (what, "bias row written", c)
        assert np.array_equal(G1[c, :, D:], G0[c, :, D:]), (what, "bias / pad columns written", c)
    return worst


def _raw_call(be, F, b, idx_pad, Yraw, G, O5):
    from odx import hip
    D, D1 = b.D, b.D + 1
    ld = _even(D1)
    hip.check(be.lib.odx_rls_gram_raw_batched_f64(_p(F.X), F.ld, D, _p(idx_pad), b.npad, _i64s(b.seg_off), _i64s(b.lengths), b.C, _p(Yraw),
                                                  Yraw.stride(0), _p(G), ld, D1 * ld, _p(O5), O5.stride(1), be._stream()),
              "odx_rls_gram_raw_batched_f64")


def _check_o5(b, O5, what):
    D, worst = b.D, 0.0
    for c in range(b.C):
        ref, bound = rc.o5_ref(b.X, b.Yraw, b.rows[c])
        r = rc.ratio(O5[c, :, :D], ref, bound)                    # (a cell left unwritten is still NaN: ratio = inf)
        assert r <= 1.0, (what, "class", c, "len", b.lengths[c], r)
        worst = max(worst, r)
        assert np.all(np.isnan(O5[c, :, D:])), (what, "O5 written past column D", c)
    return worst


@pytest.mark.parametrize("C", rc.GRAM_CS)
@pytest.mark.parametrize("D", rc.GRAM_DS)
def test_grams_from_rows(be, D, C):
    """odx_rls_gram_batched_f64 without targets (rls_gram_begin): G += X_c' X_c into a pre-filled G, twice (bit-identical)."""
    b = _batch(D, C, rc.GRAM_DS.index(D))
    F = be.row_matrix(dev(b.X))
    assert be.rls_rows_form(F)
    idx_pad = _idx_pad(be, b)
    G0 = _prefill(np.random.default_rng(D + C), C, D)
    Gd, Gd2 = dev(G0), dev(G0)
    be.rls_gram_begin(F, idx_pad, b.seg_off, b.lengths, Gd)
    be.rls_gram_begin(F, idx_pad, b.seg_off, b.lengths, Gd2)
    assert torch.equal(Gd, Gd2)
    _report("gram_rows", D=D, C=C, ratio=_check_gram_block(b, Gd.cpu().numpy(), G0, "gram"))


@pytest.mark.parametrize("C", rc.GRAM_CS)
@pytest.mark.parametrize("D", rc.GRAM_DS)
def test_grams_with_raw_target_products(be, D, C):
    """odx_rls_gram_raw_batched_f64: the heavy-first tile order's Grams again, and O5 = [Y 1]' X written into a NaN-filled buffer —
    every cell [0, D) of every class, exact zeros for a class of no rows."""
    b = _batch(D, C, rc.GRAM_DS.index(D))
    F = be.row_matrix(dev(b.X))
    idx_pad, Yraw = _idx_pad(be, b), dev(b.Yraw)
    G0 = _prefill(np.random.default_rng(D + C), C, D)
    out = []
    for _ in range(2):
        Gd = dev(G0)
        O5 = torch.full((C, 5, _even(D + 1)), float("nan"), dtype=torch.float64, device="cuda")
        _raw_call(be, F, b, idx_pad, Yraw, Gd, O5)
        out.append((Gd, O5))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1][:, :, :D], out[1][1][:, :, :D])
    rg = _check_gram_block(b, out[0][0].cpu().numpy(), G0, "gram+raw")
    O5h = out[0][1].cpu().numpy()
    for c in range(C):
        if b.lengths[c] == 0:
            assert np.all(O5h[c, :, :D] == 0.0), c
    _report("gram_raw", D=D, C=C, gram_ratio=rg, o5_ratio=_check_o5(b, O5h, "o5"))


@pytest.mark.parametrize("D", rc.GRAM_DS)
def test_rows_outside_every_class_are_never_used(be, D):
    """Row 0 and a few others belong to no class and hold NaN / Inf in X and in Yraw; most class lengths are no multiple of 32, so
    the last k-tile of a class has positions without a row (whose stand-in operand is row 0).  G and O5 stay finite and inside the
    same bounds.  (Before this test the kernel zeroed those positions by multiplying with 0.f: 0 x NaN.)"""
    b = _batch(D, 32, seed=7).poison()
    assert not np.isfinite(b.X[0]).any() and len(b.unused) > 3
    F = be.row_matrix(dev(b.X))
    idx_pad, Yraw = _idx_pad(be, b), dev(b.Yraw)
    G0 = _prefill(np.random.default_rng(D), b.C, D)
    Gd = dev(G0)
    be.rls_gram_begin(F, idx_pad, b.seg_off, b.lengths, Gd)
    r0 = _check_gram_block(b, Gd.cpu().numpy(), G0, "gram, poisoned rows")
    Gd = dev(G0)
    O5 = torch.full((b.C, 5, _even(D + 1)), float("nan"), dtype=torch.float64, device="cuda")
    _raw_call(be, F, b, idx_pad, Yraw, Gd, O5)
    r1 = _check_gram_block(b, Gd.cpu().numpy(), G0, "gram+raw, poisoned rows")
    r2 = _check_o5(b, O5.cpu().numpy(), "o5, poisoned rows")
    # the X'Y sweep and the whole single call over the same rows
    r3 = _check_targets_call(be, b, F, idx_pad, "odx_rls_gram_batched_f64", np.random.default_rng(D + 1))
    _report("outside_rows", D=D, gram_ratio=max(r0, r1), o5_ratio=r2, xty_ratio=r3)


def _check_targets_call(be, b, F, idx_pad, entry, rng):
    """odx_rls_gram_batched_f64 with targets (Grams + X'Y + bias row) or odx_rls_xty_batched_f64 (X'Y + bias row only) into a
    pre-filled G and a zero XtY: XtY (4 x D1) and the bias row against xty_ref, the D x D block against gram_ref or untouched."""
    from odx import hip
    D, D1, C = b.D, b.D + 1, b.C
    ld = _even(D1)
    G0 = _prefill(rng, C, D)
    Gd, XtY, Yt = dev(G0), torch.zeros((C, 4, ld), dtype=torch.float64, device="cuda"), dev(b.Yt)
    ws = be._workspace("rls_gram_batched", be.lib.odx_rls_gram_batched_workspace_bytes(b.npad, D))
    fn = getattr(be.lib, entry)
    hip.check(fn(_p(F.X), F.ld, D, _p(idx_pad), b.npad, _i64s(b.seg_off), _i64s(b.lengths), C, _p(Yt), Yt.stride(0), _p(Gd), ld, D1 * ld,
                 _p(XtY), ld, 4 * ld, _p(ws), ws.numel(), be._stream()), entry)
    G1, X1 = Gd.cpu().numpy(), XtY.cpu().numpy()
    worst = 0.0
    for c in range(C):
        R5, bound = rc.xty_ref(b.X, b.yt_of(c), b.rows[c], D)
        r = max(rc.ratio(X1[c, :, :D1], R5[:4], bound[:4]), rc.added_ratio(G1[c, D, :D1], G0[c, D, :D1], R5[4], bound[4]))
        assert np.array_equal(G1[c, :, D1:], G0[c, :, D1:]) and np.all(X1[c, :, D1:] == 0.0), (entry, "pad columns written", c)
        assert np.array_equal(G1[c, :D, D], G0[c, :D, D]), (entry, "bias column written", c)
        if entry == "odx_rls_xty_batched_f64":
            assert np.array_equal(G1[c, :D, :D], G0[c, :D, :D]), (entry, "Gram block written", c)
        else:
            ref, gb = rc.gram_ref(b.X, b.rows[c], D)
            r = max(r, rc.tril_ratio(G1[c, :D, :D], G0[c, :D, :D], ref, gb))
        assert r <= 1.0, (entry, "class", c, "len", b.lengths[c], r)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("C", rc.GRAM_CS)
@pytest.mark.parametrize("D", rc.GRAM_DS)
def test_xty_sweep_and_the_single_call(be, D, C):
    b = _batch(D, C, rc.GRAM_DS.index(D), seed=3)
    F = be.row_matrix(dev(b.X))
    idx_pad = _idx_pad(be, b)
    rng = np.random.default_rng(D * C)
    r0 = _check_targets_call(be, b, F, idx_pad, "odx_rls_xty_batched_f64", rng)
    r1 = _check_targets_call(be, b, F, idx_pad, "odx_rls_gram_batched_f64", rng)
    _report("xty", D=D, C=C, sweep_ratio=r0, single_call_ratio=r1)


@pytest.mark.parametrize("C", rc.GRAM_CS)
@pytest.mark.parametrize("D,forced", [(d, False) for d in rc.NT_DS] + [(72, True)])
def test_nt_route_of_the_single_call(be, D, C, forced):
    """D % 8 != 0 (and, at D = 72, the hook rls_force_nt_gram): transposed f64 copy + NT GEMM, against the same outside references as
    the rows route."""
    import odx
    b = _batch(D, C, 2, seed=5)
    F = be.row_matrix(dev(b.X))
    idx_pad = _idx_pad(be, b)
    try:
        odx.options.library_hook("rls_force_nt_gram", 1 if forced else 0)
        assert not be.rls_rows_form(F)
        r = _check_targets_call(be, b, F, idx_pad, "odx_rls_gram_batched_f64", np.random.default_rng(D + C))
    finally:
        odx.options.library_hook("rls_force_nt_gram", 0)
    _report("nt_route", D=D, C=C, forced=forced, ratio=r)


@pytest.mark.parametrize("nc", rc.ONE_CLASS_NCS)
@pytest.mark.parametrize("D", [70, 72])
def test_one_class_gram(be, D, nc):
    """odx_rls_gram_f64: the whole (D + 1) x (D + 1) lower triangle and Yt [X 1] of one class."""
    b = rc.Batch(D, [nc], seed=D + nc)
    F = be.row_matrix(dev(b.X))
    D1 = D + 1
    ld = _even(D1)
    G0 = _prefill(np.random.default_rng(nc), 1, D)[0]
    Gd, XtY = dev(G0), torch.zeros((4, ld), dtype=torch.float64, device="cuda")
    be.rls_gram(F, dev(b.rows[0]), dev(b.Yt), Gd, XtY)
    G1, X1 = Gd.cpu().numpy(), XtY.cpu().numpy()
    ref, gb = rc.gram_ref(b.X, b.rows[0], D)
    R5, bound = rc.xty_ref(b.X, b.yt_of(0), b.rows[0], D)
    r = max(rc.tril_ratio(G1[:D, :D], G0[:D, :D], ref, gb), rc.added_ratio(G1[D, :D1], G0[D, :D1], R5[4], bound[4]),
            rc.ratio(X1[:, :D1], R5[:4], bound[:4]))
    assert r <= 1.0, r
    assert np.array_equal(G1[:, D1:], G0[:, D1:]) and np.all(X1[:, D1:] == 0.0)
    _report("one_class_gram", D=D, nc=nc, ratio=r)


@pytest.mark.parametrize("C", rc.FOLD_CS)
@pytest.mark.parametrize("D", rc.FOLD_DS)
def test_fold_whitened(be, D, C):
    """odx_rls_fold_whitened_f64 on the kernel's own O5: judged alone, on the absolute sums (the means are far above the spread)."""
    from odx import hip
    L = rc.class_lengths(C, k=1) if C > 1 else [33]
    if C > 1:
        L[1] = 1                                                   # (L[0] = 1 already at k = 1; L[-1] = 0)
    b = rc.Batch(D, L, seed=D + C)
    assert 0 in b.lengths or C == 1
    F = be.row_matrix(dev(b.X))
    idx_pad = _idx_pad(be, b)
    D1 = D + 1
    ld = _even(D1)
    G = torch.zeros((C, D1, ld), dtype=torch.float64, device="cuda")
    O5 = torch.full((C, 5, ld), float("nan"), dtype=torch.float64, device="cuda")
    _raw_call(be, F, b, idx_pad, dev(b.Yraw), G, O5)
    Gram = G.clone()
    stats = rc.stats_of(np.random.default_rng(D), C)
    cnt = np.array(b.lengths, dtype=np.float64)
    XtY = torch.full((C, 4, ld), float("nan"), dtype=torch.float64, device="cuda")
    sd, cd = dev(stats), dev(cnt)
    hip.check(be.lib.odx_rls_fold_whitened_f64(_p(O5), O5.stride(1), D, C, _p(sd), _p(cd), _p(G), ld, D1 * ld, _p(XtY), ld, 4 * ld,
                                               be._stream()), "odx_rls_fold_whitened_f64")
    O5h, G1, X1, G0 = O5.cpu().numpy(), G.cpu().numpy(), XtY.cpu().numpy(), Gram.cpu().numpy()
    worst = 0.0
    for c in range(C):
        xy, bias, bound = rc.fold_ref(O5h[c, :, :D], stats[c], cnt[c])
        r = rc.ratio(X1[c, :, :D1], xy, bound)
        assert r <= 1.0, (c, b.lengths[c], r)
        worst = max(worst, r)
        assert np.array_equal(G1[c, D, :D1], bias), c             # 0 + the ones row, the row count: exact
        assert np.array_equal(G1[c, :D, :], G0[c, :D, :]) and np.all(G1[c, D, D1:] == 0.0) and np.all(np.isnan(X1[c, :, D1:])), c
    _report("fold", D=D, C=C, ratio=worst)


def _systems(D, C, regime=None):
    rng = np.random.default_rng(7 * D + C)
    D1 = D + 1
    ld = _even(D1)
    G, B = np.zeros((C, D1, ld)), np.zeros((C, 4, ld))
    for c in range(C):
        G[c], B[c] = rc.solve_system(rng, D, (D + c) % 3 if regime is None else regime)
    return G, B


def _solve_batched(be, G, B, D, lam):
    from odx import hip
    C, D1 = G.shape[0], D + 1
    ld = _even(D1)
    Gd, Bd = dev(G), dev(B)
    W = torch.full((C, 4, ld), float("nan"), dtype=torch.float64, device="cuda")
    info = torch.full((C,), -7, dtype=torch.int32, device="cuda")
    ws = be._workspace("rls_solve_batched", be.lib.odx_rls_solve_batched_workspace_bytes(D, C))
    hip.check(be.lib.odx_rls_solve_batched_f64(_p(Gd), ld, D1 * ld, D, C, float(lam), _p(Bd), ld, 4 * ld, _p(W), ld, 4 * ld, _p(info),
                                               _p(ws), ws.numel(), be._stream()), "odx_rls_solve_batched_f64")
    return W.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("C", rc.SOLVE_CS)
@pytest.mark.parametrize("D", rc.SOLVE_DS)
def test_solves_by_backward_error(be, D, C):
    """odx_rls_solve_batched_f64 (block substitution; with rls_force_inverse_solve the explicit inverse) and, for C = 1,
    odx_rls_solve_f64: the normwise backward error of every weight vector against 16 x the largest one scipy's cho_factor /
    cho_solve reaches on the same systems (floor D1 u).  The classes cycle through n < D, n ~ D, n >> D rows."""
    import odx
    D1 = D + 1
    G, B = _systems(D, C)
    for lam in rc.SOLVE_LAMS:
        A = [rc.sym_from_lower(G[c], D1, lam) for c in range(C)]
        ref = [rc.reference_solve(A[c], B[c, :, :D1]) for c in range(C)]
        ref_eta = max(rc.solve_eta(A[c], ref[c][q], B[c, q, :D1]) for c in range(C) for q in range(4))
        bar = rc.solve_bar(D1, [ref_eta])
        got = {}
        try:
            for route in ("substitute", "inverse"):
                odx.options.library_hook("rls_force_inverse_solve", 1 if route == "inverse" else 0)
                W, info = _solve_batched(be, G, B, D, lam)
                assert np.all(info == 0), (route, info)
                got[route] = max(rc.solve_eta(A[c], W[c, q, :D1], B[c, q, :D1]) for c in range(C) for q in range(4))
                if C == 1:
                    W1, info1 = be.rls_solve(dev(G[0]), D, lam, dev(B[0]))
                    assert int(info1.item()) == 0
                    W1 = W1.cpu().numpy()
                    got["single/" + route] = max(rc.solve_eta(A[0], W1[q, :D1], B[0, q, :D1]) for q in range(4))
        finally:
            odx.options.library_hook("rls_force_inverse_solve", 0)
        _report("solve", D=D, C=C, lam=lam, scipy_eta=ref_eta, bar=bar, **{k + "_eta": v for k, v in got.items()})
        for route, eta in got.items():
            assert eta <= bar, (route, lam, eta, bar, ref_eta)


@pytest.mark.parametrize("D", [127, 300])
def test_a_singular_class_does_not_touch_its_neighbour(be, D):
    """A class of all-zero rows with lam = 0 (first pivot 0) beside a good one: info names the first only, and the good class's
    weights are, bit for bit, those it gets beside another good class."""
    import odx
    D1 = D + 1
    G, B = _systems(D, 2, regime=2)                                # two good classes (n >> D rows: definite without lam) ...
    Gs, Bs = G.copy(), B.copy()
    Gs[0] = 0.0
    Gs[0, D, D] = 40.0                                             # ... and [0 1]'[0 1] of forty zero rows in the first's place
    Bs[0] = 0.0
    try:
        for route in ("substitute", "inverse"):
            odx.options.library_hook("rls_force_inverse_solve", 1 if route == "inverse" else 0)
            Wg, ig = _solve_batched(be, G, B, D, 0.0)
            Ws, isg = _solve_batched(be, Gs, Bs, D, 0.0)
            assert ig[0] == 0 and ig[1] == 0 and isg[0] != 0 and isg[1] == 0, (route, ig, isg)
            assert np.array_equal(Wg[1, :, :D1], Ws[1, :, :D1]) and np.all(np.isfinite(Ws[1, :, :D1])), route
    finally:
        odx.options.library_hook("rls_force_inverse_solve", 0)


@pytest.mark.parametrize("D", rc.PREDICT_DS)
def test_predictions(be, D):
    """odx_rls_predict_rows_batched_f64 and odx_rls_predict_rows_f64 (with row ids and, idx == NULL, over all rows) into NaN-filled
    buffers: the listed rows within the bound, nothing behind them written."""
    lengths = list(rc.PREDICT_LENGTHS) + [4, 0, 33, 0]
    b = rc.Batch(D, lengths, seed=D)
    rng = np.random.default_rng(D + 1)
    F = be.row_matrix(dev(b.X))
    ldw = _even(D + 1)
    W = rng.standard_normal((b.C, 4, ldw))
    Wd = dev(W)
    total = len(b.run)
    starts = [int(v) for v in np.concatenate(([0], np.cumsum(lengths)[:-1]))]
    full = torch.full((total + 3, 4), float("nan"), dtype=torch.float64, device="cuda")
    be.rls_predict_rows_batched(F, dev(b.run), starts, Wd, full[:total])
    got = full.cpu().numpy()
    assert np.all(np.isnan(got[total:]))
    worst = 0.0
    for c in range(b.C):
        P, bound = rc.predict_ref(b.X, W[c], b.rows[c], D)
        r = rc.ratio(got[starts[c]:starts[c] + lengths[c]], P, bound)
        one = torch.full((lengths[c] + 2, 4), float("nan"), dtype=torch.float64, device="cuda")
        be.rls_predict_rows(F, dev(b.rows[c]), Wd[c], out=one[:lengths[c]])
        oneh = one.cpu().numpy()
        assert np.all(np.isnan(oneh[lengths[c]:]))
        r = max(r, rc.ratio(oneh[:lengths[c]], P, bound))
        assert r <= 1.0, (c, lengths[c], r)
        worst = max(worst, r)
    allrows = torch.full((b.nX + 2, 4), float("nan"), dtype=torch.float64, device="cuda")
    be.rls_predict_rows(F, None, Wd[2], out=allrows[:b.nX])
    P, bound = rc.predict_ref(b.X, W[2], np.arange(b.nX), D)
    ah = allrows.cpu().numpy()
    r = rc.ratio(ah[:b.nX], P, bound)
    assert r <= 1.0 and np.all(np.isnan(ah[b.nX:])), r
    _report("predict", D=D, ratio=max(worst, r))
