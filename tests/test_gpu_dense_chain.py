"""The f64 factorisation chain (csrc/dense_f64.hip) and the CG updates (csrc/cg.hip) on the MI355X against the references and bars of
tests/dense_checks.py (numpy / scipy; tests/test_dense_checks_host.py shows what those bars reject) — on BOTH routes the two rules
of the chain choose between: helper streams (chain_helpers, automatic from 4096 centres on) and the A factor's products on the
split-f16 tile core (precond, automatic from 4096 centres on), forced here at the smallest sizes where each can go wrong, a few
outer panels.  Two cheap tests sit at the threshold itself.  Helper streams only move launches to other streams: their results must
be the very bits of the in-order run.  Every test prints `dense_chain <family> M=.. route=.. ratio=..` (profiles/dense_chain.md)."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import dense_checks as dc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROUTES = [("f64", 0), ("f64", 1), ("split", 0), ("split", 1)]
FACTORS = ("LTi", "LTit", "LAi", "LAit")
SIGMA, LAM, EPS = 9.0, 1e-4, 1e-5


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


@contextlib.contextmanager
def route(be, precond="auto", helpers=-1, release=None):
    """The chain's two rules set for the block; behind it they are what they were, and a block that (possibly) ran on helper streams
    waits for its work and releases them (odx_release_helper_streams)."""
    import odx
    with odx.options.override(precond=precond, chain_helpers=helpers):
        try:
            yield
        finally:
            if helpers != 0 if release is None else release:
                torch.cuda.synchronize()
                be.release_helper_streams()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _report(family, **kv):
    print("dense_chain %s %s" % (family, " ".join("%s=%s" % (k, ("%.3g" % v) if isinstance(v, float) else v) for k, v in kv.items())))


def _bits_equal(a, b):
    """Bit for bit, NaN included (torch.equal calls NaN unequal to itself)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _nan_bytes(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")           # every f64 / f32 word a NaN


# ---------------------------------------------------------------------------------------------------------------- potrf + trtri
def _potrf(be, Ah, poison=False):
    from odx import hip
    M, ld = Ah.shape
    dA = dev(Ah)
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    nb = be.lib.odx_potrf_workspace_bytes(M)
    ws = _nan_bytes(nb) if poison else torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    hip.check(be.lib.odx_potrf_f64(_p(dA), ld, M, _p(info), _p(ws), ws.numel(), be._stream()), "odx_potrf_f64")
    return dA, int(info.item())


def _trtri(be, dL, M, poison=False):
    from odx import hip
    ld = dL.shape[1]
    fill = float("nan") if poison else 0.0
    Li = torch.full((M, ld), fill, dtype=torch.float64, device="cuda")
    Lit = torch.full((M, ld), fill, dtype=torch.float64, device="cuda")
    nb = be.lib.odx_trtri_workspace_bytes(M)
    ws = _nan_bytes(nb) if poison else torch.zeros(max(nb, 16), dtype=torch.uint8, device="cuda")
    hip.check(be.lib.odx_trtri_f64(_p(dL), ld, M, _p(Li), _p(Lit), ld, _p(ws), ws.numel(), be._stream()), "odx_trtri_f64")
    return Li, Lit


_HOST = {}


def _host_case(kind, M):
    """(A, chol bar, scipy's chol figure): host data only, computed once per problem and shared by the helper settings."""
    if (kind, M) not in _HOST:
        A = dc.problem(kind, M)
        _HOST[(kind, M)] = (A,) + dc.chol_bar(A)
    return _HOST[(kind, M)]


@pytest.mark.parametrize("helpers", [0, 1])
@pytest.mark.parametrize("kind", ["well", "kernel"])
@pytest.mark.parametrize("M", dc.ALL_M)
def test_potrf_trtri_against_scipy(be, M, kind, helpers):
    """odx_potrf_f64 + odx_trtri_f64: backward errors under 16 x scipy's on the same matrix (never below (M + 1) u), exact zeros above
    the diagonal, Li / Lit bitwise transposes — and the bits of that run again with NaN in everything the entries must not read: A's
    strict upper triangle, the pad column of an odd M, the whole workspace, Li / Lit before the call."""
    A, cbar, cref = _host_case(kind, M)
    with route(be, helpers=helpers):
        dL, info = _potrf(be, dc.padded_lower(A))
        Li, Lit = _trtri(be, dL, M)
        dLn, infon = _potrf(be, dc.padded_lower(A, fill=np.nan), poison=True)
        Lin, Litn = _trtri(be, dLn, M, poison=True)                    # (dLn still holds NaN above its diagonal blocks)
    assert info == 0 and infon == 0
    L, X, Xt = (t[:, :M].cpu().numpy() for t in (dL, Li, Lit))
    assert not np.any(np.triu(L, 1)) and not np.any(np.triu(X, 1)) and not np.any(np.tril(Xt, -1))
    ti, tj = np.tril_indices(M)
    assert np.array_equal(dLn[:, :M].cpu().numpy()[ti, tj].view(np.uint64), L[ti, tj].view(np.uint64)), "potrf read what it must not"
    assert _bits_equal(Lin[:, :M], Li[:, :M]) and _bits_equal(Litn[:, :M], Lit[:, :M]), "trtri read what it must not"
    assert dc.transposes(X, Xt)
    ceta = dc.chol_eta(A, L)
    ibar, iref = dc.inv_bar(L)
    ieta = dc.inv_eta(L, X)
    _report("potrf", M=M, kind=kind, route="helpers%d" % helpers, ratio=ceta / cbar, eta=ceta, scipy=cref)
    _report("trtri", M=M, kind=kind, route="helpers%d" % helpers, ratio=ieta / ibar, eta=ieta, scipy=iref)
    assert ceta <= cbar and ieta <= ibar, (ceta, cbar, ieta, ibar)


@pytest.mark.parametrize("helpers", [0, 1])
def test_potrf_reports_the_first_bad_pivot(be, helpers):
    """A non-positive pivot deep in the third outer panel (index 1300 of 1537 -> 1301), and of two in different panels the smaller."""
    M = 1537
    A = dc.spd_well(M)
    one, two = A.copy(), A.copy()
    one[1300, 1300] = -1.0
    two[1300, 1300], two[700, 700] = -1.0, -1.0
    with route(be, helpers=helpers):
        got = [_potrf(be, dc.padded_lower(a))[1] for a in (one, two, A)]
    assert got == [1301, 701, 0], got


# ---------------------------------------------------------------------------------------------------------------- preconditioner
_PC = {}


def _pc_case(M, D):
    """Per (M, D), once, host data only: centres, K, S = T T'/M + lam I from scipy's factor, and their bars."""
    if (M, D) not in _PC:
        Z = dc.centres(M, D)
        K = dc.kmm(Z, SIGMA, EPS)
        Lk = dc.ref_chol(K)
        S = Lk.T @ Lk / M + LAM * np.eye(M)
        _PC[(M, D)] = {"Z": Z, "K": K, "S": S, "tbar": dc.precond_bar(K, dc.ref_inv(Lk)), "abar": dc.precond_bar(S)}
    return _PC[(M, D)]


@pytest.mark.parametrize("precond,helpers", ROUTES)
@pytest.mark.parametrize("M,D", dc.PRECOND_CASES)
def test_precond_against_scipy_on_every_route(be, M, D, precond, helpers):
    """odx_falkon_precond_f64: L_T^-1 K L_T^-T = I under 16 x scipy's figure on the same K and bitwise transposes on every route; the A
    factor the same against T T'/M + lam I of the chain's own T (dense_checks.precond_a_eta) on the f64 route, the project's split bars on the split route (T then the f64 route's bits).
    A second call into a NaN-filled `out=` and workspace gives the same bits, and the products of an odd M stay finite."""
    c = _pc_case(M, D)
    ld = (M + 1) // 2 * 2
    Zf = be.features(torch.from_numpy(c["Z"]))
    with route(be, precond, helpers):
        P = be.precond(Zf, SIGMA, LAM, EPS)
        be.check_precond(P)
        clean = torch.stack([getattr(P, f)[:, :M] for f in FACTORS])
        be._workspace("precond", be.lib.odx_falkon_precond_workspace_bytes(M, D)).fill_(0xFF)
        out = torch.full((4, M, ld), float("nan"), dtype=torch.float64, device="cuda")
        Pn = be.precond(Zf, SIGMA, LAM, EPS, out=out)
        be.check_precond(Pn)
    for k, f in enumerate(FACTORS):
        assert _bits_equal(getattr(Pn, f)[:, :M], clean[k]), (f, "depends on what out= / the workspace held")
    assert torch.equal(clean[0].t(), clean[1]) and torch.equal(clean[2].t(), clean[3])
    if M % 2:
        x = np.random.default_rng(M).standard_normal(M)
        for k, f in enumerate(FACTORS):
            got = be.trmv(Pn, f, dev(x)).cpu().numpy()
            ref = clean[k].cpu().numpy() @ x
            bound = 2.0 * (M + 1) * dc.U * (np.abs(clean[k].cpu().numpy()) @ np.abs(x))
            assert dc.ratio(got, ref, bound) <= 1.0, (f, "the pad column went into a sum")
    tbar, tref = c["tbar"]
    teta = dc.precond_eta(c["K"], clean[0].cpu().numpy())
    tag = "%s/helpers%d" % (precond, helpers)
    _report("precond_T", M=M, D=D, route=tag, ratio=teta / tbar, eta=teta, scipy=tref)
    assert teta <= tbar, (teta, tbar)
    if precond == "f64":
        abar, aref = c["abar"]
        aeta = dc.precond_a_eta(clean[0].cpu().numpy(), clean[2].cpu().numpy(), LAM)
        _report("precond_A", M=M, D=D, route=tag, ratio=aeta / abar, eta=aeta, scipy=aref)
        assert aeta <= abar, (aeta, abar)
    else:
        with route(be, "f64", 0):
            P0 = be.precond(Zf, SIGMA, LAM, EPS)
        assert _bits_equal(clean[0], P0.LTi[:, :M]) and _bits_equal(clean[1], P0.LTit[:, :M])
        assert not torch.equal(clean[2], P0.LAi[:, :M])
        resid, rel = dc.split_figures(c["S"], clean[2].cpu().numpy(), P0.LAi[:, :M].cpu().numpy())
        _report("precond_A_split", M=M, D=D, route=tag, ratio=max(resid / dc.SPLIT_RESID, rel / dc.SPLIT_REL), resid=resid, rel=rel)
        assert resid < dc.SPLIT_RESID and rel < dc.SPLIT_REL, (resid, rel)


def _stack(P):
    return torch.stack([getattr(P, f)[:, :P.M] for f in FACTORS])


def _centres_dev(be, M, D, seed=0):
    return be.features(torch.from_numpy(dc.centres(M, D, seed)))


@pytest.mark.parametrize("precond", ["f64", "split"])
@pytest.mark.parametrize("M", dc.HELPER_M)
def test_helper_streams_change_no_bit_single_and_path(be, M, precond):
    """The launches are the same, only their streams differ: chain_helpers = 1 gives the bits of chain_helpers = 0.  A difference
    would be a race (a missing fork / join, a packed slot reused too early) or an order-dependent sum — never a tolerance."""
    Zf = _centres_dev(be, M, 64)
    lams = [1e-3, 1e-4, 1e-6]
    res = []
    for helpers in (0, 1):
        with route(be, precond, helpers):
            P = be.precond(Zf, SIGMA, LAM, EPS)
            Ps = be.precond_path(Zf, SIGMA, lams, EPS)
            res.append((_stack(P), [_stack(m) for m in Ps], [int(m.info.item()) for m in Ps] + [int(P.info.item())]))
    (s0, p0, i0), (s1, p1, i1) = res
    assert i0 == [0] * 4 and i1 == [0] * 4
    assert _bits_equal(s0, s1), ("single", float((s0 - s1).abs().max()))
    for l in range(3):
        assert _bits_equal(p0[l], p1[l]), ("path member", l, float((p0[l] - p1[l]).abs().max()))
    assert _bits_equal(p1[1], s1)                           # (lam of member 1 is the single call's: the members are that call's bits)
    _report("helpers_single_path", M=M, route=precond, ratio=0.0)


@pytest.mark.parametrize("precond", ["f64", "split"])
@pytest.mark.parametrize("Ms", [(1537, 640, 2600, 129), (2049, 2049), (1025,)])
def test_helper_streams_change_no_bit_batched(be, Ms, precond):
    Zfs = [_centres_dev(be, M, 36, seed=i) for i, M in enumerate(Ms)]
    res = []
    for helpers in (0, 1):
        with route(be, precond, helpers):
            Ps = be.precond_batched(Zfs, SIGMA, LAM, EPS)
            res.append([_stack(P) for P in Ps])
            assert all(int(P.info.item()) == 0 for P in Ps)
    for b, (a0, a1) in enumerate(zip(*res)):
        assert _bits_equal(a0, a1), ("class", b, Ms[b], float((a0 - a1).abs().max()))
    _report("helpers_batched", M="/".join(str(m) for m in Ms), route=precond, ratio=0.0)


def test_batched_and_path_members_equal_the_single_call_on_the_concurrent_route(be):
    """(split, helpers 1) — the route of the headline: class b of a ragged batch and member l of a path are the single call's bits; a
    class whose Cholesky fails reports it alone."""
    Ms, D = (1537, 640, 129), 36
    Zfs = [_centres_dev(be, M, D, seed=i) for i, M in enumerate(Ms)]
    lams = [1e-3, LAM]
    with route(be, "split", 1):
        Pb = be.precond_batched(Zfs, SIGMA, LAM, EPS)
        for Zf, P in zip(Zfs, Pb):
            P1 = be.precond(Zf, SIGMA, LAM, EPS)
            assert int(P.info.item()) == 0 and int(P1.info.item()) == 0
            assert _bits_equal(_stack(P), _stack(P1)), (P.M, float((_stack(P) - _stack(P1)).abs().max()))
        Pp = be.precond_path(Zfs[0], SIGMA, lams, EPS)
        for lam, P in zip(lams, Pp):
            assert _bits_equal(_stack(P), _stack(be.precond(Zfs[0], SIGMA, lam, EPS))), lam
        bad = be.features(torch.zeros((700, D)))                                   # K_MM = all ones: singular without jitter
        Pbad = be.precond_batched([Zfs[1], bad, Zfs[2]], SIGMA, 0.0, 0.0)
        infos = [int(P.info.item()) for P in Pbad]
    assert infos[0] == 0 and infos[2] == 0 and infos[1] != 0, infos
    _report("members_concurrent", M="/".join(str(m) for m in Ms), route="split/helpers1", ratio=0.0)


@pytest.mark.parametrize("M", [4095, 4096])
def test_automatic_rule_switches_both_routes_at_4096(be, M):
    """Default options: below 4096 centres the bits of (f64, helpers 0); from 4096 on those of (split, helpers 1), which differ from
    (f64, helpers 0) in the A factor and not in the T factor.  Device comparisons only."""
    Zf = _centres_dev(be, M, 32)
    with route(be, "auto", -1, release=True):
        auto = _stack(be.precond(Zf, SIGMA, LAM, EPS))
    with route(be, "f64", 0):
        plain = _stack(be.precond(Zf, SIGMA, LAM, EPS))
    if M < 4096:
        assert _bits_equal(auto, plain)
    else:
        with route(be, "split", 1):
            forced = _stack(be.precond(Zf, SIGMA, LAM, EPS))
        assert _bits_equal(auto, forced)
        assert _bits_equal(auto[0], plain[0]) and _bits_equal(auto[1], plain[1])
        assert not torch.equal(auto[2], plain[2]) and torch.equal(auto[2].t(), auto[3])
    _report("automatic_rule", M=M, route="auto", ratio=0.0)


def test_default_route_above_the_threshold_against_scipy(be):
    """M = 4100, D = 64 on the options as shipped (split, helpers): the T factor under its scipy bar, the A factor under the project's
    four split bars (its defining identity, close to and not equal to the f64 route's A factor, T the f64 route's bits).  The one
    test with a few seconds of host linear algebra."""
    M, D = 4100, 64
    Z = dc.centres(M, D)
    K = dc.kmm(Z, SIGMA, EPS)
    Zf = be.features(torch.from_numpy(Z))
    with route(be, "auto", -1, release=True):
        P = be.precond(Zf, SIGMA, LAM, EPS)
        be.check_precond(P)
        auto = _stack(P)
    with route(be, "f64", 0):
        plain = _stack(be.precond(Zf, SIGMA, LAM, EPS))
    assert torch.equal(auto[0].t(), auto[1]) and torch.equal(auto[2].t(), auto[3])
    assert _bits_equal(auto[0], plain[0]) and _bits_equal(auto[1], plain[1])
    assert not torch.equal(auto[2], plain[2])
    Lk = dc.ref_chol(K)
    tbar, tref = dc.precond_bar(K, dc.ref_inv(Lk))
    teta = dc.precond_eta(K, auto[0].cpu().numpy())
    _report("precond_T", M=M, D=D, route="auto", ratio=teta / tbar, eta=teta, scipy=tref)
    resid, rel = dc.split_figures(Lk.T @ Lk / M + LAM * np.eye(M), auto[2].cpu().numpy(), plain[2].cpu().numpy())
    _report("precond_A_split", M=M, D=D, route="auto", ratio=max(resid / dc.SPLIT_RESID, rel / dc.SPLIT_REL), resid=resid, rel=rel)
    assert teta <= tbar and resid < dc.SPLIT_RESID and rel < dc.SPLIT_REL, (teta, tbar, resid, rel)


# ---------------------------------------------------------------------------------------------------------------- cg.hip
def _cg_dev(*arrays):
    return [dev(np.asarray(a, dtype=np.float64)) for a in arrays]


def _np(**tensors):
    return {k: v.cpu().numpy() for k, v in tensors.items()}


@pytest.mark.parametrize("M", dc.CG_MS)
def test_cg_init_step_finish_residual(be, M):
    """odx_cg_init / _step (full_grad 0 and 1) / _finish / _residual entry by entry inside the bounds derived from the formats."""
    X, R, P, AP, B = dc.cg_vectors(M)
    eps, worst = 1e-7, 0.0
    b, x, r, p, st = _cg_dev(B, np.full(M, np.nan), np.full(M, np.nan), np.full(M, np.nan), np.full(4, np.nan))
    be.cg_init(b, x, r, p, st)
    ref, bound = dc.cg_init_ref(B)
    worst = max(worst, dc.cg_ratio(_np(X=x, R=r, P=p, state=st), ref, bound))
    state = np.array([float(R @ R) * 1.3, 0.25, 0.0, 0.5])
    for full in (0, 1):
        x, r, p, ap, st = _cg_dev(X, R, P, AP, state)
        be.cg_step(x, r, p, ap, st, eps, full)
        ref, bound = dc.cg_step_ref(X, R, P, AP, state, eps, full)
        worst = max(worst, dc.cg_ratio(_np(X=x, R=r, state=st), ref, bound))
        assert torch.equal(p, dev(P)) and torch.equal(ap, dev(AP))
    r, p, st = _cg_dev(R, P, state)
    be.cg_finish(r, p, st, eps, 1e-9)
    ref, bound = dc.cg_finish_ref(R, P, state, eps, 1e-9)
    worst = max(worst, dc.cg_ratio(_np(P=p, state=st), ref, bound))
    assert torch.equal(r, dev(R))
    b, ax, ap, st, r = _cg_dev(B, X, AP, state, np.full(M, np.nan))
    be.cg_residual(b, ax, ap, st, r)
    ref, bound = dc.cg_residual_ref(B, X, AP, state, np.full(M, np.nan))
    worst = max(worst, dc.cg_ratio(_np(R=r), ref, bound))
    _report("cg_updates", M=M, route="single", ratio=worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("M", dc.CG_MS)
def test_cg_finish_compares_strictly_and_a_raised_flag_freezes_everything(be, M):
    """sqrt |R . R| against tol just below, just above and exactly equal (25 = 3^2 + 4^2 sums exactly in any order; `<` is strict): the
    flag and whether P moved.  With the flag up, step, finish, residual and scores_axpy leave every output and state word as it was."""
    R = np.zeros(M)
    R[0], R[M - 1] = (3.0, 4.0) if M > 1 else (5.0, 5.0)
    P = np.linspace(1.0, 2.0, M)
    state = np.array([50.0, 50.0, 0.0, 0.1])
    for tol, flag in ((np.nextafter(5.0, 6.0), 1.0), (5.0, 0.0), (np.nextafter(5.0, 4.0), 0.0)):
        r, p, st = _cg_dev(R, P, state)
        be.cg_finish(r, p, st, 0.0, tol)
        ref, bound = dc.cg_finish_ref(R, P, state, 0.0, tol)
        got = _np(P=p, state=st)
        assert got["state"][2] == flag == ref["state"][2], (tol, got["state"])
        assert np.array_equal(got["P"], P) == (flag == 1.0), (tol, "P moved" if flag else "P did not move")
        assert dc.cg_ratio(got, ref, bound) <= 1.0
    X, _, _, AP, B = dc.cg_vectors(M)
    up = np.array([50.0, 25.0, 1.0, 0.1])
    x, r, p, ap, b, st, s = _cg_dev(X, R, P, AP, B, up, X)
    before = [t.clone() for t in (x, r, p, ap, b, st, s)]
    be.cg_step(x, r, p, ap, st, 1e-7, 0)
    be.cg_finish(r, p, st, 1e-7, 1e-30)
    be.cg_residual(b, x, ap, st, r)
    be.cg_scores_axpy(st, ap, s)
    for t, t0 in zip((x, r, p, ap, b, st, s), before):
        assert _bits_equal(t, t0)
    _report("cg_flag", M=M, route="single", ratio=0.0)


@pytest.mark.parametrize("n", dc.SCORE_NS)
def test_cg_scores_and_axpby(be, n):
    """odx_cg_scores_axpy_f64, odx_cg_scores_store_f32 into a strided column (ldo = 3, neighbours untouched, bitwise the rounding of
    S) and odx_axpby_f64 — with b = 0 a NaN-filled y is overwritten, not multiplied."""
    rng = np.random.default_rng(n)
    t, S, y = rng.standard_normal(n) * 3.0, rng.standard_normal(n) * 1e3, rng.standard_normal(n)
    state = np.array([1.0, 1.0, 0.0, -0.37])
    st, td, Sd = _cg_dev(state, t, S)
    be.cg_scores_axpy(st, td, Sd)
    ref, bound = dc.scores_axpy_ref(state, t, S)
    worst = dc.cg_ratio(_np(S=Sd), ref, bound)
    out = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    be.cg_scores_store(Sd, out[:, 1:2])
    o = out.cpu().numpy()
    assert np.array_equal(o[:, 1], dc.scores_store_ref(Sd.cpu().numpy())) and np.all(np.isnan(o[:, [0, 2]]))
    xd, yd = _cg_dev(t, y)
    be.axpby(-1.5, xd, 0.75, yd)
    ref, bound = dc.axpby_ref(-1.5, t, 0.75, y)
    worst = max(worst, dc.cg_ratio(_np(y=yd), ref, bound))
    yn = dev(np.full(n, np.nan))
    be.axpby(-1.5, xd, 0.0, yn)
    ref, bound = dc.axpby_ref(-1.5, t, 0.0, np.full(n, np.nan))
    worst = max(worst, dc.cg_ratio(_np(y=yn), ref, bound))
    _report("cg_scores_axpby", M=n, route="single", ratio=worst)
    assert worst <= 1.0, worst


# (1025, 2, 640) crosses a bracket of the K_nM sweep (M <= 1024 | 1025 .. 2048: csrc/knm_pass.hip pick_cfg), and the lock-step loop takes
# the classes of ONE pass configuration per call (include/odx.h: callers fall back otherwise, as odx/falkon.py does).  Its classes go
# through the loop configuration by configuration; the two batches behind it hold the same sizes as three classes of one call.
@pytest.mark.parametrize("Ms", [(1025, 2, 640), (1024, 2, 640), (1025, 1026, 2048)])
def test_batched_cg_updates_through_the_lockstep_loop(be, Ms):
    """The batched forms of the CG kernels (one workgroup per class), reached through odx_falkon_cg_batched_f64 on tiny blocks, maxiter
    3: the class with a zero right-hand side gets alpha exactly 0, the others their single-class odx_falkon_cg_f64 bits.  A batch
    the library's contract refuses whole (classes from two pass configurations) is refused, and runs as the fewest calls the
    contract allows: the classes in order, each joining the first call it may share."""
    from odx.solver import SolverOptions
    rng = np.random.default_rng(sum(Ms))
    D, opt, ns = 24, SolverOptions(check_pivots=False), (300, 257, 411)
    Fs, Zfs, ys = [], [], []
    for n, M in zip(ns, Ms):
        Fs.append(be.features(torch.from_numpy((rng.standard_normal((n, D)) * (20.0 / np.sqrt(D))).astype(np.float32))))
        Zfs.append(be.features(torch.from_numpy((rng.standard_normal((M, D)) * (20.0 / np.sqrt(D))).astype(np.float32))))
        ys.append(be.vec(np.where(rng.random(n) < 0.3, 1.0, -1.0)))
    ys[1] = be.vec(np.zeros(ns[1]))

    def lockstep(idx):
        Ps = be.precond_batched([Zfs[i] for i in idx], SIGMA, LAM, opt.pc_epsilon)
        b0s = torch.zeros((len(idx), (max(Ms[i] for i in idx) + 1) // 2 * 2), dtype=torch.float64, device="cuda")
        Ks = [be.knm_rhs(Fs[i], Zfs[i], SIGMA, ys[i] * (1.0 / ns[i]), rhs_out=b0s[r, :Ms[i]])[0] for r, i in enumerate(idx)]
        return Ks, Ps, b0s, be.cg_solve_batched(Ks, Ps, b0s, [ns[i] for i in idx], LAM, 3, opt)

    calls = []
    for i in range(3):
        for call in calls:
            if be.cg_batched_supported([ns[j] for j in call + [i]], [Ms[j] for j in call + [i]]):
                call.append(i)
                break
        else:
            calls.append([i])
    if len(calls) > 1:
        assert lockstep([0, 1, 2])[3] is None
    peak = {}
    for idx in calls:
        Ks, Ps, b0s, alphas = lockstep(idx)
        assert alphas is not None, idx
        for r, (i, K, P) in enumerate(zip(idx, Ks, Ps)):
            single = be.cg_solve(K, P, b0s[r, :K.M].clone(), K.n, LAM, 3, opt)
            assert torch.isfinite(single).all() and _bits_equal(alphas[r, :K.M], single), (i, Ms[i])
            peak[i] = float(alphas[r].abs().max())
    assert peak[1] == 0.0 and peak[0] > 0.0 and peak[2] > 0.0, peak
    _report("cg_batched", M="/".join(str(m) for m in Ms), route="lockstep:" + "+".join(str(len(c)) for c in calls), ratio=0.0)
