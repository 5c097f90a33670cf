"""A PARTIAL inverse of T on the MI355X (csrc/dense_f64.hip: odx_trtri_partial_f64, odx_tri_blocked_mv_f64, the class-batched chain
with a stop level).  The stop level is passed explicitly, so matrices of a few hundred rows have unmerged levels: a ragged second
block (300, 641, 1300), a second block of ONE row (129, 257, 1025), M an exact multiple of the block (512), odd block ends.  With
"levels of s >= stop rows are not run", M = 1300 leaves the levels 256 / 512 / 1024 unmerged under stop 256 and 512 / 1024 under 512.

  - the stored form, bit for bit: diagonal blocks = the full call's, blocks beside them = the factor's own, the other triangle zero;
  - the blocked product against scipy's solve_triangular on a HOST Cholesky factor of the same K_MM + eps M I: normwise error at most
    16 x the error of the fully merged odx_trmv_f64 route on the same problem against the same reference (the margin
    tests/dense_checks.py gives the chain).  Every case prints `partial_t_inverse mv ...` with both figures (profiles/build_phase.md);
  - one LockstepClassJob with the stop level forced through the library's option, against oracle/falkon_ref."""
import ctypes

import numpy as np
import pytest

from tests import dense_checks as dc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = [(129, 128), (257, 128), (300, 128), (641, 128), (512, 256), (1025, 256), (1300, 256), (1300, 512)]


@pytest.fixture(scope="module")
def be():
    import odx
    return odx.get_backend()


def _p(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _nan_bytes(nbytes):
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device="cuda")


_CASE = {}


def _case(be, M):
    """Per M, once: K (host), the DEVICE factor of it with NaN wherever the chain must not read (above the diagonal blocks, the pad
    column), and the full inverse pair made from that factor."""
    if M not in _CASE:
        from odx import hip
        K = dc.spd_kernel(M)[1]
        dL = torch.from_numpy(dc.padded_lower(K, fill=np.nan)).cuda()
        ld = dL.shape[1]
        info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        ws = _nan_bytes(be.lib.odx_potrf_workspace_bytes(M))
        hip.check(be.lib.odx_potrf_f64(_p(dL), ld, M, _p(info), _p(ws), ws.numel(), be._stream()), "odx_potrf_f64")
        assert int(info.item()) == 0
        _CASE[M] = (K, dL) + _inverse(be, dL, M, 0)
    return _CASE[M]


def _inverse(be, dL, M, stop):
    from odx import hip
    ld = dL.shape[1]
    Li = torch.full((M, ld), float("nan"), dtype=torch.float64, device="cuda")
    Lit = torch.full((M, ld), float("nan"), dtype=torch.float64, device="cuda")
    ws = _nan_bytes(be.lib.odx_trtri_workspace_bytes(M))
    if stop:
        hip.check(be.lib.odx_trtri_partial_f64(_p(dL), ld, M, stop, _p(Li), _p(Lit), ld, _p(ws), ws.numel(), be._stream()),
                  "odx_trtri_partial_f64")
    else:
        hip.check(be.lib.odx_trtri_f64(_p(dL), ld, M, _p(Li), _p(Lit), ld, _p(ws), ws.numel(), be._stream()), "odx_trtri_f64")
    return Li, Lit


def _bounds(M, stop):
    return list(range(0, M, stop)) + [M]


@pytest.mark.parametrize("M,stop", CASES)
def test_partial_inverse_is_the_full_calls_blocks_and_the_factors(be, M, stop):
    K, dL, Li_f, Lit_f = _case(be, M)
    Li, Lit = _inverse(be, dL, M, stop)
    b = _bounds(M, stop)
    assert len(b) >= 3
    for k in range(len(b) - 1):
        r0, r1 = b[k], b[k + 1]
        # the diagonal block: what the full call has there (final after level stop / 2), in both orientations
        assert _bits_equal(Li[r0:r1, r0:r1], Li_f[r0:r1, r0:r1]), ("Li diagonal block", k)
        assert _bits_equal(Lit[r0:r1, r0:r1], Lit_f[r0:r1, r0:r1]), ("Lit diagonal block", k)
        if r0:
            # beside it: the factor's own block, and its transpose
            assert _bits_equal(Li[r0:r1, :r0], dL[r0:r1, :r0]), ("Li block row", k)
            assert _bits_equal(Lit[:r0, r0:r1], dL[r0:r1, :r0].t()), ("Lit block column", k)
        # the other triangle of the M x M matrix: zero; a pad column: never written
        assert not torch.any(Li[r0:r1, r1:M]) and not torch.any(Lit[r0:r1, :r0])
    assert not torch.any(torch.triu(Li[:, :M], 1)) and not torch.any(torch.tril(Lit[:, :M], -1))
    assert bool(torch.isnan(Li[:, M:]).all()) and bool(torch.isnan(Lit[:, M:]).all())
    # stop at or beyond M: nothing is left unmerged, the full call's bits
    top = 128
    while top < M:
        top *= 2
    Li_t, Lit_t = _inverse(be, dL, M, top)
    assert _bits_equal(Li_t[:, :M], Li_f[:, :M]) and _bits_equal(Lit_t[:, :M], Lit_f[:, :M])


def _blocked_mv(be, Tri, M, uplo, bounds, x, alpha, beta, z, poison=True):
    from odx import hip
    y = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    nb = be.lib.odx_tri_blocked_mv_workspace_bytes(M)
    ws = _nan_bytes(nb) if poison else torch.zeros(nb, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_int64 * len(bounds))(*bounds)
    hip.check(be.lib.odx_tri_blocked_mv_f64(_p(Tri), Tri.shape[1], M, uplo, arr, len(bounds) - 1, _p(x), alpha, beta, _p(z), _p(y),
                                            _p(ws), ws.numel(), be._stream()), "odx_tri_blocked_mv_f64")
    return y


def _merged_mv(be, Tri, M, uplo, x, alpha, beta, z):
    from odx import hip
    y = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
    hip.check(be.lib.odx_trmv_f64(_p(Tri), Tri.shape[1], M, uplo, _p(x), alpha, beta, _p(z), _p(y), be._stream()), "odx_trmv_f64")
    return y


@pytest.mark.parametrize("uplo", [0, 1])
@pytest.mark.parametrize("M,stop", CASES)
def test_blocked_product_against_host_substitution(be, M, stop, uplo):
    import scipy.linalg as sla
    K, dL, Li_f, Lit_f = _case(be, M)
    Li, Lit = _inverse(be, dL, M, stop)
    rng = np.random.default_rng(900 + M + stop + uplo)
    xh, zh = rng.standard_normal(M), rng.standard_normal(M)
    alpha, beta = 1.0 / 3.0, 1e-5
    Lh = dc.ref_chol(K)                                               # the HOST factor of the same matrix
    ref = alpha * sla.solve_triangular(Lh, xh, lower=True, trans="T" if uplo else "N", check_finite=False) + beta * zh
    x, z = torch.from_numpy(xh).cuda(), torch.from_numpy(zh).cuda()
    part, full = (Lit, Lit_f) if uplo else (Li, Li_f)
    got = _blocked_mv(be, part, M, uplo, _bounds(M, stop), x, alpha, beta, z).cpu().numpy()
    merged = _merged_mv(be, full, M, uplo, x, alpha, beta, z).cpu().numpy()
    e_blocked = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    e_merged = float(np.linalg.norm(merged - ref) / np.linalg.norm(ref))
    print("partial_t_inverse mv M=%d stop=%d uplo=%d blocks=%d blocked=%.3e merged=%.3e ratio=%.3g"
          % (M, stop, uplo, len(_bounds(M, stop)) - 1, e_blocked, e_merged, e_blocked / e_merged if e_merged else float("inf")))
    assert np.all(np.isfinite(got)) and e_blocked <= 16.0 * e_merged, (e_blocked, e_merged)
    # beta == 0 takes no z; one block is odx_trmv_f64 itself, bit for bit
    y0 = _blocked_mv(be, part, M, uplo, _bounds(M, stop), x, alpha, 0.0, None)
    y1 = _blocked_mv(be, part, M, uplo, _bounds(M, stop), x, alpha, 0.0, torch.full_like(z, float("nan")))
    assert _bits_equal(y0, y1)
    one = _blocked_mv(be, full, M, uplo, [0, M], x, alpha, beta, z)
    assert _bits_equal(one, torch.from_numpy(merged).cuda())


def test_batched_chain_with_a_stop_level_keeps_every_other_factor(be):
    """backend.precond_batched(t_stop=...): classes of 600 and 300 centres in one chain, stop 256.  LAi / LAit and the diagonal blocks
    of LTi / LTit are the merged call's bits; a class with rows beyond the stop level carries its boundaries, one without does not."""
    Zs = [be.features(torch.from_numpy(dc.centres(M, 36))) for M in (600, 300)]
    full = be.precond_batched(Zs, 9.0, 1e-4, 1e-5, ws_key="precond_partial_test")
    torch.cuda.synchronize()
    part = be.precond_batched(Zs, 9.0, 1e-4, 1e-5, ws_key="precond_partial_test", t_stop=256)
    torch.cuda.synchronize()
    be.release_helper_streams()
    assert [p.blocks for p in full] == [(), ()] and [p.blocks for p in part] == [(0, 256, 512, 600), (0, 256, 300)]
    for pf, pp in zip(full, part):
        assert _bits_equal(pp.LAi, pf.LAi) and _bits_equal(pp.LAit, pf.LAit)
        for r0, r1 in zip(pp.blocks[:-1], pp.blocks[1:]):
            assert _bits_equal(pp.LTi[r0:r1, r0:r1], pf.LTi[r0:r1, r0:r1]) and _bits_equal(pp.LTit[r0:r1, r0:r1], pf.LTit[r0:r1, r0:r1])
        x = torch.from_numpy(np.random.default_rng(5).standard_normal(pf.M)).cuda()
        for name in ("LTi", "LTit"):
            a, b = be.trmv(pp, name, x).cpu().numpy(), be.trmv(pf, name, x).cpu().numpy()
            assert np.linalg.norm(a - b) <= 1e-8 * np.linalg.norm(b), name          # (the same operator, cond(L) M u << 1e-8; the bar proper is the test above)
    be.release_workspaces()


def test_job_with_a_forced_stop_level(be):
    """One LockstepClassJob, two classes of 600 centres over 5000 rows in one class-batched chain, T's inverse stopped at 256 through
    the library's option: every product with T's inverse is a blocked one, alpha within 1e-4 relative and the scores within 1e-4
    absolute of oracle/falkon_ref.  Alpha's movement against the merged route is printed, not asserted."""
    from odx import options
    from odx.job import LockstepClassJob
    from odx.solver import SolverOptions
    from oracle import falkon_ref as fr
    from tests.synth import blob_problem
    n, D, M, sigma, lam = 5000, 256, 600, 10.0, 1e-5
    X, y, rng = blob_problem(n, D, seed=n + M)
    idx = [np.sort(rng.choice(n, M, replace=False)).astype(np.int64) for _ in range(2)]
    ys = [y.astype(np.float64), -y.astype(np.float64)]
    dev = be.device
    Xd = torch.from_numpy(X).to(dev)
    labels = lambda c: torch.from_numpy(ys[c]).to(dev)        # noqa: E731
    cidx = [torch.from_numpy(i).to(dev) for i in idx]
    got, seen = {}, {}
    plain_trmv = be.trmv

    def recording_trmv(P, name, *a, **kw):
        seen.setdefault((stop, name), set()).add(P.blocks)
        return plain_trmv(P, name, *a, **kw)

    be.trmv = recording_trmv
    try:
        for stop in (256, 0):
            options.library_hook("t_inverse_force_stop", stop)
            alphas = {}
            job = LockstepClassJob(be, Xd, n, M, labels, cidx, sigma, lam, 20, SolverOptions(check_pivots=False), precond_batch=2)
            job.run(be.features(Xd), [0, 1], alphas_out=alphas)
            torch.cuda.synchronize()
            got[stop] = ({c: alphas[c].cpu().numpy() for c in (0, 1)}, job.scores.cpu().numpy().copy())
            job.release()
    finally:
        del be.trmv
        options.library_hook("t_inverse_force_stop", 0)
        be.release_workspaces()
    for name in ("LTi", "LTit"):
        assert seen[(256, name)] == {(0, 256, 512, 600)} and seen[(0, name)] == {()}, seen
    for name in ("LAi", "LAit"):
        assert (256, name) in seen
    X64 = X.astype(np.float64)
    for c in (0, 1):
        ref, Z = fr.falkon_fit(X64, ys[c], idx[c], sigma, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        pref = fr.falkon_predict(X64, Z, ref, sigma)[:, 0]
        for stop in (256, 0):
            rel = np.linalg.norm(got[stop][0][c] - ref[:, 0]) / np.linalg.norm(ref[:, 0])
            serr = np.abs(got[stop][1][:, c] - pref).max()
            print("partial_t_inverse job class %d stop=%d: alpha rel err %.3e, scores abs err %.3e" % (c, stop, rel, serr))
            assert rel < 1e-4 and serr < 1e-4, (c, stop, rel, serr)
        d = np.linalg.norm(got[256][0][c] - got[0][0][c]) / np.linalg.norm(got[0][0][c])
        print("partial_t_inverse job class %d: alpha, blocked against merged: relative difference %.3e" % (c, d))
