"""K_nM blocks of the DISTINCT centres only on the MI355X (odx/cols.py; include/odx.h, "Distinct columns"): the passes that fold
v where they load it and write out[j] from column col_of[j] (odx_knm_fwd_bwd_q_cols_t, odx_knm_fwd_bwd2_q_cols_t), the
stand-alone fold / expand (odx_cols_fold_f64, odx_cols_expand_f64), the block knm_rhs builds for centres that carry a map,
and a LockstepClassJob fit with distinct_columns="force" against the f64 oracle on the full, repeated centre list.

Bounds.  u = 2^-53.  The stored entries are exact in f64 and so is the 2^-24 scale.  A row product t_r = sum_j K[r, j] v[j]
of M terms, summed in any order (with or without the fold, which only regroups the sum), is within (M + 3) u (|K| |v|)[r] of
the exact value: M u for the sum, up to three more additions per folded entry.  s_r = t_r + w_r rounds once more, and a
column sum over the n rows adds n u: with A = |K| |v| + |w|, E = (M + 3) u |K| |v|,
    |t_out - exact| <= E,      |out - exact| <= |K|' (E + (n + 2) u A)
for ONE pass.  The checks compare two passes (distinct block against full block), each within that of the exact value, so
they use twice these bounds; nothing in them comes from what a kernel returned."""
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


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def repeated_indices(Md, extra, rng):
    """An index list of M = Md + extra positions over Md distinct centres: the centre at position 0 occurs again at position
    M - 1; with extra >= 3 it occurs 4 times, the other extras are second occurrences of further centres."""
    base = rng.permutation(Md) + 100
    a = int(base[0])
    extras = [int(c) for c in base[1:1 + max(extra - 3, 0)]] + [a] * min(extra, 3)
    mid = np.array(list(base[1:]) + extras[:-1], dtype=np.int64)
    rng.shuffle(mid)
    return np.concatenate(([a], mid, extras[-1:])).astype(np.int64)


def _codes(rng, n, M, fmt):
    """(n, M) random stored codes: 24-bit integers, or bf16 bit patterns of values in [0, 1), with the extreme codes."""
    if fmt == "u24":
        q = rng.integers(0, 1 << 24, (n, M), dtype=np.int64)
        q[0, 0], q[-1, M - 1] = (1 << 24) - 1, 0
        return q
    return (rng.random((n, M)).astype(np.float32).view(np.uint32) >> 16).astype(np.int64)


def _block(codes, fmt):
    """The stored block of `codes` in the library's layout, and the f64 values it encodes."""
    from odx.backend import Knm
    n, M = codes.shape
    ld = (M + 7) // 8 * 8
    full = np.zeros((n, ld), dtype=np.int64)
    full[:, :M] = codes
    K = Knm()
    K.n, K.M, K.ld, K.fmt = n, M, ld, fmt
    if fmt == "u24":
        K.K = torch.from_numpy((full >> 8).astype(np.uint16).view(np.int16)).cuda()
        K.lo = torch.from_numpy((full & 255).astype(np.uint8)).cuda()
        return K, codes.astype(np.float64) * 2.0 ** -24
    K.K = torch.from_numpy(full.astype(np.uint16).view(np.int16)).cuda()
    return K, (codes.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _mapped(K, cmap):
    from odx.backend import Knm
    Km = Knm()
    Km.K, Km.lo, Km.n, Km.M, Km.ld, Km.fmt = K.K, K.lo, K.n, K.M, K.ld, K.fmt
    Km.cmap, Km.Mv = cmap, cmap.Mv
    return Km


def _fold(be, cmap, v):
    _, _, start, pos = cmap.on(be.device)
    out = torch.full((cmap.Md,), float("nan"), dtype=torch.float64, device=be.device)
    be._call("odx_cols_fold_f64", _p(v), cmap.Mv, _p(start), _p(pos), cmap.Md, _p(out))
    return out


def _expand(be, cmap, x):
    col_of = cmap.on(be.device)[1]
    out = torch.full((cmap.Mv,), float("nan"), dtype=torch.float64, device=be.device)
    be._call("odx_cols_expand_f64", _p(x), cmap.Md, _p(col_of), cmap.Mv, _p(out))
    return out


# (n, Md, M - Md): one case per configuration of the one-vector rule (odx_knm_pass_kernel_name: the brackets end at 1024,
# 2048, 4096, 8192, 10240, 12288 and 20440 columns) with n no multiple of its row block (16, 8, 4, 3, 2, 4 rows) and several
# blocks per workgroup; Md never a multiple of 4; M - Md = 1; the staggered kernel's bracket twice (the second: the shape
# the headline's classes are closest to).  Those between 4097 and 10240 columns also have the two two-vector configurations.
CASES = [(333, 1021, 1), (333, 2045, 5), (203, 4091, 8), (202, 8189, 11), (601, 8195, 5), (600, 8195, 5), (203, 12283, 7),
         (131, 20437, 3)]
NAMES = {1021: "knm_passq_kernel<256,1,16", 2045: "knm_passq_stag_kernel<2,8", 4091: "knm_passq_stag_kernel<4,4",
         8189: "knm_passq_kernel<256,8,3", 8195: "knm_passq_stag_kernel<10,2", 12283: "knm_passq_kernel<512,6,4",
         20437: "knm_passq_kernel<1024,5,1"}
NAMES2 = {8189: "knm_passq_kernel<512,4,2,2", 8195: "knm_passq_kernel<512,5,2,2"}


def _setup(be, fmt, n, Md, extra):
    from odx import hip
    from odx.cols import column_map
    rng = np.random.default_rng(n * 7 + Md + extra)
    idx = repeated_indices(Md, extra, rng)
    cmap = column_map(torch.from_numpy(idx))
    assert (cmap.Mv, cmap.Md) == (Md + extra, Md) and Md % 4 != 0
    counts = np.diff(cmap.start.numpy())
    assert counts.max() == (4 if extra >= 3 else 2) and cmap.col_of[0] == cmap.col_of[-1] == 0
    codes = _codes(rng, n, Md, fmt)
    Kd, vals_d = _block(codes, fmt)
    col = cmap.col_of.numpy().astype(np.int64)
    Kf, vals_f = _block(codes[:, col], fmt)
    code = hip.KNM_CODE[fmt]
    assert be.lib.odx_knm_pass_kernel_name(Md, code, 1).decode().startswith(NAMES[Md])
    # (the full block may sit in the next bracket: it is only the reference)
    return rng, cmap, Kd, Kf, vals_f, code


def _bounds(vals, v, w):
    """(bound on t_out, bound on out) of ONE pass over the block `vals` (see the module docstring)."""
    n, M = vals.shape
    kv = np.abs(vals) @ np.abs(v) if v is not None else np.zeros(n)
    E = (M + 3) * U * kv
    A = kv + (np.abs(w) if w is not None else 0.0)
    return E, np.abs(vals).T @ (E + (n + 2) * U * A)


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,Md,extra", CASES)
def test_one_vector_pass(be, fmt, n, Md, extra):
    """out, t_out of the _cols entry: bit for bit expand(plain entry on the same block with fold(v)), and within the f64
    summation bound of the pass over the full block with the repeated columns; with v, w and t_out, and with v null."""
    rng, cmap, Kd, Kf, vals_f, _ = _setup(be, fmt, n, Md, extra)
    M = cmap.Mv
    Km = _mapped(Kd, cmap)
    vh = rng.standard_normal(M)
    wh = rng.standard_normal(n)
    v, w = torch.from_numpy(vh).cuda(), torch.from_numpy(wh).cuda()
    for use_v, use_w, use_t in ((True, True, True), (True, False, False), (False, True, False)):
        vv, ww = (v if use_v else None), (w if use_w else None)
        nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")      # noqa: E731
        out, t = nan(M), (nan(n) if use_t else None)
        be.ktk(Km, v=vv, w=ww, out=out, t_out=t)
        # bit for bit: the existing entry on the same block, its v folded and its out expanded by the stand-alone launches
        out_d, t_d = nan(Md), (nan(n) if use_t else None)
        be.ktk(Kd, v=_fold(be, cmap, vv) if use_v else None, w=ww, out=out_d, t_out=t_d)
        assert torch.equal(out, _expand(be, cmap, out_d)), (use_v, use_w)
        if use_t:
            assert torch.equal(t, t_d)
        # the pass over the full block
        out_f, t_f = nan(M), (nan(n) if use_t else None)
        be.ktk(Kf, v=vv, w=ww, out=out_f, t_out=t_f)
        torch.cuda.synchronize()
        Et, Eo = _bounds(vals_f, vh if use_v else None, wh if use_w else None)
        err = np.abs(out.cpu().numpy() - out_f.cpu().numpy())
        print("n=%d Md=%d M=%d %s v=%d w=%d: max err / bound %.3f" % (n, Md, M, fmt, use_v, use_w, float((err / np.maximum(2 * Eo, 1e-300)).max())))
        assert (err <= 2 * Eo).all(), float((err / np.maximum(2 * Eo, 1e-300)).max())
        if use_t:
            assert (np.abs(t.cpu().numpy() - t_f.cpu().numpy()) <= 2 * Et).all()
        # and against the exact product (f64 numpy: its own sums are within the same bound)
        s = (vals_f @ vh if use_v else 0.0) + (wh if use_w else 0.0)
        assert (np.abs(out.cpu().numpy() - vals_f.T @ s) <= 2 * Eo).all()


@pytest.mark.parametrize("fmt", ["u24", "bf16"])
@pytest.mark.parametrize("n,Md,extra", [c for c in CASES if c[1] in NAMES2])
def test_two_vector_pass(be, fmt, n, Md, extra):
    """Both configurations of the two-vector rule: out, out2 and t_out as in test_one_vector_pass."""
    rng, cmap, Kd, Kf, vals_f, code = _setup(be, fmt, n, Md, extra)
    assert be.lib.odx_knm_pass_kernel_name(Md, code, 2).decode().startswith(NAMES2[Md])
    M = cmap.Mv
    Km = _mapped(Kd, cmap)
    assert be.can_ktk2(Km)
    v1h, v2h = rng.standard_normal(M), rng.standard_normal(M) * 1e-3
    v1, v2 = torch.from_numpy(v1h).cuda(), torch.from_numpy(v2h).cuda()
    nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device="cuda")          # noqa: E731
    o1, o2, t = nan(M), nan(M), nan(n)
    be.ktk2(Km, v1, v2, out1=o1, out2=o2, t_out=t)
    d1, d2, td = nan(Md), nan(Md), nan(n)
    be.ktk2(Kd, _fold(be, cmap, v1), _fold(be, cmap, v2), out1=d1, out2=d2, t_out=td)
    assert torch.equal(o1, _expand(be, cmap, d1)) and torch.equal(o2, _expand(be, cmap, d2)) and torch.equal(t, td)
    f1, f2, tf = nan(M), nan(M), nan(n)
    be.ktk2(Kf, v1, v2, out1=f1, out2=f2, t_out=tf)
    torch.cuda.synchronize()
    for got, full, vh in ((o1, f1, v1h), (o2, f2, v2h)):
        Et, Eo = _bounds(vals_f, vh, None)
        assert (np.abs(got.cpu().numpy() - full.cpu().numpy()) <= 2 * Eo).all()
        assert (np.abs(got.cpu().numpy() - vals_f.T @ (vals_f @ vh)) <= 2 * Eo).all()
    assert (np.abs(t.cpu().numpy() - tf.cpu().numpy()) <= 2 * _bounds(vals_f, v1h, None)[0]).all()


def test_fold_and_expand_entries(be):
    """The stand-alone launches against the map's own host arithmetic (left-to-right sums: bit for bit)."""
    from odx.cols import column_map
    rng = np.random.default_rng(11)
    cmap = column_map(torch.from_numpy(repeated_indices(1021, 9, rng)))
    v = torch.from_numpy(rng.standard_normal(cmap.Mv))
    x = torch.from_numpy(rng.standard_normal(cmap.Md))
    assert torch.equal(_fold(be, cmap, v.cuda()).cpu(), cmap.fold(v))
    assert torch.equal(_expand(be, cmap, x.cuda()).cpu(), cmap.expand(x))


def test_wide_routes_refuse_a_mapped_block(be):
    from odx.cols import column_map
    rng = np.random.default_rng(13)
    cmap = column_map(torch.from_numpy(repeated_indices(301, 2, rng)))
    Km = _mapped(_block(_codes(rng, 9, 301, "u24"), "u24")[0], cmap)
    V = torch.zeros((3, 304), dtype=torch.float64, device="cuda")
    for call in (lambda: be.ktkn(Km, V), lambda: be.kvn(Km, V), lambda: be.ktwn(Km, torch.zeros((2, 10), dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError, match="distinct columns"):
            call()


# ------------------------------------------------------------------------------------------------ the block knm_rhs builds
@pytest.mark.parametrize("fmt", ["u24", "bf16"])
def test_block_contents_and_rhs(be, fmt):
    """knm_rhs on centres that carry a map: the decoded distinct block equals the matching columns of the full block bit for
    bit (same build kernel, same operand rows), K' w comes back M long within the f64 summation bound, knm_mv folds alpha."""
    from odx import options
    from odx.cols import column_map
    from tests.synth import blob_problem
    n, D, Md, extra = 1501, 72, 517, 6
    X, y, rng = blob_problem(n, D, seed=5)
    idx = repeated_indices(Md, extra, rng) - 100
    cmap = column_map(torch.from_numpy(idx))
    with options.override(gauss="h2", knm_storage=fmt):
        F = be.features(torch.from_numpy(X))
        w = torch.from_numpy(rng.standard_normal(n)).cuda()
        Zfull = be.rows(F, idx)
        Kf, bf = be.knm_rhs(F, Zfull, 6.0, w)
        Zmap = be.rows(F, idx)
        Zmap.cmap = cmap
        Kd, bd = be.knm_rhs(F, Zmap, 6.0, w)
    torch.cuda.synchronize()
    assert Kf.fmt == Kd.fmt == fmt and Kf.cmap is None and Kd.cmap is cmap and (Kd.M, Kd.Mv, Kf.M) == (Md, Md + extra, Md + extra)
    full, dist = Kf.dense().cpu(), Kd.dense().cpu()
    assert torch.equal(dist, full[:, cmap.first]) and torch.equal(dist[:, cmap.col_of.long()], full)
    assert tuple(bd.shape) == (Md + extra,)
    vals = full.double().numpy()
    bound = 2 * (n + 2) * U * (np.abs(vals).T @ np.abs(w.cpu().numpy()))
    assert (np.abs(bd.cpu().numpy() - bf.cpu().numpy()) <= bound).all()
    assert (np.abs(bd.cpu().numpy() - vals.T @ w.cpu().numpy()) <= bound).all()
    alpha = torch.from_numpy(rng.standard_normal(Md + extra)).cuda()
    got, want = be.knm_mv(Kd, alpha).cpu().double().numpy()[:, 0], vals @ alpha.cpu().numpy()
    # one f32 rounding of an f64 sum of M terms
    tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2 * (Md + extra + 3) * U * (np.abs(vals) @ np.abs(alpha.cpu().numpy()))
    assert (np.abs(got - want) <= tol).all()
    # f32 storage never takes the map
    with options.override(gauss="h2", knm_storage="f32"):
        K32, b32 = be.knm_rhs(F, Zmap, 6.0, w)
    assert K32.fmt == "f32" and K32.cmap is None and K32.M == Md + extra


# ------------------------------------------------------------------------------------------------ the job
def test_job_with_forced_distinct_columns(be):
    """One LockstepClassJob over two classes, compact storage through an options override, distinct_columns="force": the
    class with repeated centres (the reference's centre rule on test_falkon_fit_alpha_parity's first problem) streams its
    distinct columns, the class without takes the plain path; alpha within 1e-4
    relative and scores within 1e-4 absolute of oracle/falkon_ref on the full repeated list (test_falkon_fit_alpha_parity's
    bars).  The difference to distinct_columns=False is printed, not asserted."""
    from odx import options
    from odx.job import LockstepClassJob
    from odx.solver import SolverOptions
    from oracle import falkon_ref as fr
    from odx.cols import column_map
    from tests.synth import blob_problem, centres
    n, D, M, sigma, lam = 5000, 256, 500, 10.0, 1e-5          # test_falkon_fit_alpha_parity's first problem
    X, y, rng = blob_problem(n, D, seed=n + M)
    rep = np.asarray(centres(y, M, rng), dtype=np.int64)      # the reference's rule: positives drawn with replacement
    Md = column_map(torch.from_numpy(rep)).Md
    assert M - 100 < Md < M
    seen = set(rep.tolist())                                  # the same centres without the repeats, filled up with other rows
    plain = np.array(list(dict.fromkeys(rep.tolist())) + [i for i in range(n) if i not in seen][:M - Md], dtype=np.int64)
    assert len(set(plain.tolist())) == M
    ys = [y.astype(np.float64), y.astype(np.float64)]
    dev = be.device
    Xd = torch.from_numpy(X).to(dev)
    labels = lambda c: torch.from_numpy(ys[c]).to(dev)        # noqa: E731
    cidx = [torch.from_numpy(rep).to(dev), torch.from_numpy(plain).to(dev)]
    got = {}
    try:
        with options.override(knm_storage="u24"):
            for mode in ("force", False, "auto"):
                alphas = {}
                job = LockstepClassJob(be, Xd, n, M, labels, cidx, sigma, lam, 20, SolverOptions(check_pivots=False), distinct_columns=mode)
                job.run(be.features(Xd), [0, 1], alphas_out=alphas)
                torch.cuda.synchronize()
                distinct = [p for k, p in job.trace if k == "distinct"]
                # ("auto": 5000 x 500 entries are far below the 2^27 of the size bound)
                assert distinct == ([(0, Md)] if mode == "force" else []), (mode, distinct)
                got[mode] = ({c: alphas[c].cpu().numpy() for c in (0, 1)}, job.scores.cpu().numpy().copy())
                job.release()
    finally:
        be.release_workspaces()
    X64 = X.astype(np.float64)
    for c, idx in ((0, rep), (1, plain)):
        ref, Z = fr.falkon_fit(X64, ys[c], idx, sigma, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        pref = fr.falkon_predict(X64, Z, ref, sigma)[:, 0]
        for mode in ("force", False):
            rel = np.linalg.norm(got[mode][0][c] - ref[:, 0]) / np.linalg.norm(ref[:, 0])
            serr = np.abs(got[mode][1][:, c] - pref).max()
            print("class %d distinct_columns=%r: alpha rel err %.3e, scores abs err %.3e" % (c, mode, rel, serr))
            assert rel < 1e-4 and serr < 1e-4, (c, mode, rel, serr)
    d = np.linalg.norm(got["force"][0][0] - got[False][0][0]) / np.linalg.norm(got[False][0][0])
    print("alpha, distinct columns against the full block (class 0): relative difference %.3e" % d)
    assert np.array_equal(got["force"][0][1], got[False][0][1])          # the class without repeats: the same launches
    assert np.array_equal(got["auto"][0][0], got[False][0][0])
