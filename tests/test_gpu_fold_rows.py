"""The CG's fold step over accumulated scores on the MI355X: one forward and two backward products from one read of a compact
block (odx_knm_fwd_bwd_q_rows[_cols]_t, HipBackend.ktk_rows; include/odx.h) and the schedule that uses it
(solver._cg_run, fold_rows).

Kernel bound.  out1 = K'(K v), out2 = K' s and t_out = K v are checked against f64 products of the decoded block formed by
torch on the device, in the form tests/test_scores_from_cg.py uses for the passes' row products: the largest absolute
difference against 1e-12 of the largest reference entry (that file's constant; every measured figure is printed, and
profiles/fold_rows.md records the worst).

Solver case.  The two-vector rule, and with it the new entry, starts above 4096 columns, and the fold needs n >= 8 M rows:
a fit of 5000 rows and 500 centres never reaches the fold step.  The case below is the smallest that does (33 001 rows,
4100 centres over 4097 distinct rows, the shape of test_scores_from_cg's folded fit); it asserts that the new entry ran."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_distinct_columns import _codes, _mapped, repeated_indices      # noqa: E402

REL = 1e-12      # tests/test_scores_from_cg.py, _check_rows


@pytest.fixture(scope="module")
def be():
    import odx
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return odx.get_backend()


def _poisoned_block(codes, fmt, extra_rows=3):
    """The stored block of `codes` as rows [0, n) of a larger allocation whose further rows hold NaN (bf16) or the largest code
    (u24: the format has no NaN), and the f64 values it encodes, on the device.  Pad columns stay zero, as the builds leave
    them (the passes read them and multiply by zero)."""
    from odx.backend import Knm
    n, M = codes.shape
    ld = (M + 7) // 8 * 8
    full = np.zeros((n + extra_rows, ld), dtype=np.int64)
    full[:n, :M] = codes
    full[n:, :] = (1 << 24) - 1 if fmt == "u24" else 0x7FC0
    K = Knm()
    K.n, K.M, K.ld, K.fmt = n + extra_rows, M, ld, fmt
    if fmt == "u24":
        K.K = torch.from_numpy((full >> 8).astype(np.uint16).view(np.int16)).cuda()
        K.lo = torch.from_numpy((full & 255).astype(np.uint8)).cuda()
        vals = torch.from_numpy(codes.astype(np.float64)).cuda() * 2.0 ** -24
    else:
        K.K = torch.from_numpy(full.astype(np.uint16).view(np.int16)).cuda()
        vals = torch.from_numpy((codes.astype(np.uint32) << 16).view(np.float32)).cuda().double()
    return K.rows(0, n), vals


def _padded(x, pad=64):
    """x in front of `pad` NaN entries: the vector the entry gets, and the whole buffer."""
    big = torch.full((x.numel() + pad,), float("nan"), dtype=torch.float64, device="cuda")
    big[:x.numel()] = x
    return big[:x.numel()], big


def _out(k, pad=64):
    big = torch.full((k + pad,), -7.0, dtype=torch.float64, device="cuda")
    big[:k] = float("nan")
    return big[:k], big


# (n, distinct columns, repeats).  Both configuration classes of the entry (4096 < M <= 8192 and 8192 < M <= ~10 200: the
# two-vector rule's), in each: n = 1 (one row block, the second half of the workgroup has none), n = 3 (fewer rows than
# halves at work on a full grid, not a multiple of a two-row block), a few hundred rows, and more than 1024 rows (a half
# makes several trips); no column count a multiple of 4.
CASES = [(1, 4101, 3), (3, 6001, 5), (1101, 8189, 3), (1, 9997, 5), (3, 8197, 3), (301, 8197, 5), (1301, 9999, 3)]


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,Md,extra", CASES)
def test_rows_pass_against_f64_products(be, fmt, n, Md, extra, mapped):
    from odx import hip
    from odx.cols import column_map
    rng = np.random.default_rng(n * 13 + Md + extra + mapped)
    K, vals = _poisoned_block(_codes(rng, n, Md, fmt), fmt)
    Mv = Md
    if mapped:
        idx = repeated_indices(Md, extra, rng)
        cmap = column_map(torch.from_numpy(idx))
        assert (cmap.Mv, cmap.Md) == (Md + extra, Md) and cmap.col_of[0] == cmap.col_of[-1] == 0      # a repeat at 0 and M - 1
        K = _mapped(K, cmap)
        Mv = cmap.Mv
        vals = vals[:, cmap.col_of.long().cuda()]                    # the full block with the repeated columns
    assert be.can_ktk_rows(K) and Md % 4 != 0
    v, _ = _padded(torch.from_numpy(rng.standard_normal(Mv)).cuda())
    s, _ = _padded(torch.from_numpy(rng.standard_normal(n)).cuda())
    o1, big1 = _out(Mv)
    o2, big2 = _out(Mv)
    t, bigt = _out(n)
    # the slabs start as NaN: what the reduce reads must have been written by this launch
    ws = be._workspace("ktk", 2 * be._pass_bytes("odx_knm_fwd_bwd2_q", n, Md, hip.KNM_CODE[fmt]))
    ws.fill_(0xFF)
    be.ktk_rows(K, v, s, out1=o1, out2=o2, t_out=t)
    p1, p2 = be.ktk_rows(K, v, s)                                   # without t_out: the same bits
    torch.cuda.synchronize()
    assert torch.equal(p1, o1) and torch.equal(p2, o2)
    want_t = vals @ v
    for name, got, want in (("t_out", t, want_t), ("out1", o1, vals.t() @ want_t), ("out2", o2, vals.t() @ s)):
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print("%s %s n=%d Md=%d Mv=%d: max |%s - f64 reference| = %.3e at scale %.3e (%.3e of it)"
              % (fmt, "mapped" if mapped else "plain", n, Md, Mv, name, err, scale, err / scale))
        assert err <= REL * scale, (name, fmt, n, Md, mapped, err, scale)
    for big, k in ((big1, Mv), (big2, Mv), (bigt, n)):
        assert bool((big[k:] == -7.0).all())                        # nothing written behind the vectors


def test_rows_pass_refusals(be):
    from odx import hip
    rng = np.random.default_rng(5)
    K, _ = _poisoned_block(_codes(rng, 5, 4101, "u24"), "u24")
    v = torch.zeros(4101, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        be.ktk_rows(K, v, None)
    with pytest.raises(ValueError):
        be.ktk_rows(K, v, torch.zeros(4, dtype=torch.float64, device="cuda"))
    narrow, _ = _poisoned_block(_codes(rng, 5, 301, "u24"), "u24")
    assert not be.can_ktk_rows(narrow)
    with pytest.raises(hip.OdxError):
        be.ktk_rows(narrow, torch.zeros(301, dtype=torch.float64, device="cuda"), torch.zeros(5, dtype=torch.float64, device="cuda"))


# ------------------------------------------------------------------------------------------------------------- the fit
@contextlib.contextmanager
def _counted(be, names):
    """Counts of the calls into the named library entries."""
    counts, orig = {k: 0 for k in names}, {k: getattr(be.lib, k) for k in names}

    def wrap(k):
        def call(*a):
            counts[k] += 1
            return orig[k](*a)
        return call
    for k in names:
        setattr(be.lib, k, wrap(k))
    try:
        yield counts
    finally:
        for k in names:
            setattr(be.lib, k, orig[k])


ROWS = ("odx_knm_fwd_bwd_q_rows_t", "odx_knm_fwd_bwd_q_rows_cols_t")
N, D, M, SIGMA, LAM = 33_001, 64, 4100, 10.0, 1e-5


@pytest.fixture(scope="module")
def problem():
    from odx.cols import column_map
    from tests.synth import blob_problem
    X, y, rng = blob_problem(N, D, seed=77)
    # 4097 distinct rows, one of them named four times (at positions 0 and M - 1 among them).  (The reference's rule draws so many
    # repeats at this size that the distinct block falls below 4097 columns, where no two-vector configuration exists.)
    idx = rng.permutation(N)[repeated_indices(M - 3, 3, rng) - 100]
    cmap = column_map(torch.from_numpy(idx))
    assert cmap is not None and 4096 < cmap.Md < M                   # some repeated, and still a two-vector width
    return X, y, idx, cmap


def _fit(be, problem, fold_rows, cg_tolerance=1e-7, maxiter=20, mapped=True):
    """alpha, the f64 scores of the fit, the block, and the number of calls of the new entries."""
    import odx
    from odx import options
    from odx.solver import SolverOptions
    X, y, idx, cmap = problem
    prev = be.fold_rows
    be.fold_rows = fold_rows
    try:
        with options.override(gauss="h2", knm_storage="u24"):
            F = be.features(torch.from_numpy(X))
            Zf = be.rows(F, idx)
            if mapped:
                Zf.cmap = cmap
            S = torch.full((N,), 7.0, dtype=torch.float64, device=be.device)
            Ks = []
            with _counted(be, ROWS) as counts:
                alpha = odx.falkon_fit(be, F, be.vec(y), Zf, SIGMA, LAM, maxiter, SolverOptions(cg_tolerance=cg_tolerance), knm_blocks=Ks,
                                       scores_out=S, phase=lambda name: contextlib.nullcontext())
            torch.cuda.synchronize()
        return alpha, S, Ks[0], sum(counts.values())
    finally:
        be.fold_rows = prev


@pytest.fixture(scope="module")
def fits(be, problem):
    try:
        on, off = _fit(be, problem, True), _fit(be, problem, False)
        plain = _fit(be, problem, True, mapped=False)
        return {"on": on, "off": off, "plain": plain}
    finally:
        be.release_workspaces()
        torch.cuda.empty_cache()


def test_fit_takes_the_new_route_once(fits):
    # 20 iterations, full residual every 10th, the last one needs none: one fold step
    assert fits["on"][3] == 1 and fits["off"][3] == 0 and fits["plain"][3] == 1
    assert fits["on"][2].cmap is not None and fits["plain"][2].cmap is None


def test_fit_against_the_route_switched_off(fits):
    a, b = fits["on"][0].cpu(), fits["off"][0].cpu()
    rel = float((a - b).norm() / b.norm())
    ds = float((fits["on"][1] - fits["off"][1]).abs().max())
    print("alpha, fold over the scores against the two-vector fold: relative 2-norm difference %.3e; scores: max abs %.3e" % (rel, ds))
    assert rel <= 1e-9
    assert ds <= 1e-9 * max(1.0, float(fits["off"][1].abs().max()))


def test_fit_against_the_oracle(be, problem, fits):
    from oracle import falkon_ref as fr
    X, y, idx, _ = problem
    X64 = X.astype(np.float64)
    ref, Z = fr.falkon_fit(X64, y.astype(np.float64), idx, SIGMA, LAM, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
    pref = fr.falkon_predict(X64, Z, ref, SIGMA)[:, 0]
    for name in ("on", "plain"):
        alpha, S = fits[name][0].cpu().numpy(), fits[name][1].cpu().numpy()
        rel = float(np.linalg.norm(alpha - ref[:, 0]) / np.linalg.norm(ref[:, 0]))
        serr = float(np.abs(S - pref).max())
        print("%s: alpha rel err %.3e, scores abs err %.3e" % (name, rel, serr))
        assert rel < 1e-4 and serr < 1e-4, (name, rel, serr)


def test_stop_flag_before_the_fold_freezes_the_scores(be, problem):
    """cg_tolerance 1e3: the flag goes up in the cg_finish of iteration 0.  Every later step is dropped from X and from S alike,
    the fold step of iteration 10 still runs over S, and S is K T^-1 A^-1 X for the X that stopped: K' S, what the fold read,
    is K' (K alpha)."""
    try:
        alpha, S, K, calls = _fit(be, problem, True, cg_tolerance=1e3)
        first, S1, _, calls1 = _fit(be, problem, True, cg_tolerance=1e3, maxiter=1)
        assert calls == 1 and calls1 == 0
        assert torch.equal(alpha, first) and torch.equal(S, S1) and float(S.abs().max()) > 0
        kts, ktka = be.ktk(K, w=S), be.ktk(K, v=alpha)
        torch.cuda.synchronize()
        err, scale = float((kts - ktka).abs().max()), float(ktka.abs().max())
        print("stopped fit: max |K' S - K' K alpha| = %.3e at scale %.3e" % (err, scale))
        assert err <= 1e-9 * scale
    finally:
        be.release_workspaces()
        torch.cuda.empty_cache()
