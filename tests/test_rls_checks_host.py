"""The checkers of tests/rls_checks.py on the CPU: each accepts numpy's / scipy's own result — summed in ANOTHER order than the
reference, as a kernel does — on every shape tests/test_gpu_rls_kernels.py uses, and rejects the faults a subtly wrong kernel makes:
a row dropped, a neighbouring class's row added, a ragged-tile column zeroed, one entry off by 1e-10 relative, the last k-tile
(len mod 32 rows) dropped, a substitution block skipped."""
import numpy as np
import pytest

from tests import rls_checks as rc


def _chunked(fn, rows, step=32):
    """fn summed k-tile by k-tile (32 rows at a time, last tile first): another order of the same sums."""
    out = None
    for s in reversed(range(0, max(len(rows), 1), step)):
        part = fn(rows[s:s + step])
        out = part if out is None else out + part
    return out


def _batches(Ds, Cs):
    for i, D in enumerate(Ds):
        for C in Cs:
            yield D, C, rc.Batch(D, rc.class_lengths(C, k=3 * i + 1 if C < 32 else 0), seed=100 * D + C)


def test_class_lengths_cover_the_edges():
    L = rc.class_lengths(32)
    assert L[0] == 0 and L[12] == 0 and L[24] == 0 and L[31] == 0 and set(rc.LENGTHS) <= set(L)
    assert all(rc.class_lengths(1, k)[0] > 0 for k in range(40))
    b = rc.Batch(72, L, seed=1)
    assert b.npad % 16 == 0 and all(o % 16 == 0 for o in b.seg_off) and 0 in b.unused and len(b.unused) >= 5
    used = np.concatenate(b.rows)
    assert len(set(used.tolist())) == len(used) and not set(used.tolist()) & set(b.unused.tolist())
    assert np.array_equal(np.sort(b.idx_pad[b.idx_pad >= 0]), np.sort(used))


def test_gram_and_o5_checkers_accept_another_summation_order():
    worst = 0.0
    for D, C, b in _batches(rc.GRAM_DS + rc.NT_DS, rc.GRAM_CS):
        for c, rows in enumerate(b.rows):
            G, bound = rc.gram_ref(b.X, rows)
            X64 = b.X.astype(np.float64)
            alt = _chunked(lambda r: X64[r].T @ X64[r], rows)
            before = np.random.default_rng(c).standard_normal(G.shape)
            worst = max(worst, rc.ratio(alt, G, bound), rc.tril_ratio(before + alt, before, G, bound))
            O5, b5 = rc.o5_ref(b.X, b.Yraw, rows)
            Y5 = np.concatenate([b.Yraw.astype(np.float64), np.ones((b.nX, 1))], axis=1)
            worst = max(worst, rc.ratio(_chunked(lambda r: Y5[r].T @ X64[r], rows), O5, b5))
    assert worst <= 1.0, worst


def test_gram_checker_is_within_an_extended_precision_sum():
    """numpy's f64 product against the 80-bit one: well inside the one-sided half of the bound (where numpy has extended precision)."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        return                                                   # (no extended precision on this platform: nothing to compare with)
    b = rc.Batch(72, [33, 100, 513], seed=5)
    for rows in b.rows:
        G, bound = rc.gram_ref(b.X, rows)
        Xl = b.X[rows].astype(np.longdouble)
        exact = np.einsum("ki,kj->ij", Xl, Xl)
        assert float((np.abs(G - exact) / (bound / 2)).max()) < 0.5


GRAM_FAULTS = ["row_dropped", "neighbour_row_added", "ragged_column_zeroed", "entry_off_1e-10", "last_k_tile_dropped"]


def _faulty_rows(fault, b, c):
    rows = b.rows[c]
    if fault == "row_dropped":
        return rows[:-1]
    if fault == "neighbour_row_added":
        return np.concatenate([rows, b.rows[(c + 1) % b.C][:1]])
    if fault == "last_k_tile_dropped":
        return rows[:len(rows) // 32 * 32]
    return rows


@pytest.mark.parametrize("fault", GRAM_FAULTS)
@pytest.mark.parametrize("D", [8, 72, 136, 1032])
def test_gram_o5_xty_checkers_reject(fault, D):
    b = rc.Batch(D, [33, 65, 100, 17], seed=D)
    X64 = b.X.astype(np.float64)
    Y5 = np.concatenate([b.Yraw.astype(np.float64), np.ones((b.nX, 1))], axis=1)
    for c in range(b.C):
        rows = b.rows[c]
        G, bound = rc.gram_ref(b.X, rows)
        O5, b5 = rc.o5_ref(b.X, b.Yraw, rows)
        R5, br = rc.xty_ref(b.X, b.yt_of(c), rows)
        fr = _faulty_rows(fault, b, c)
        bad_g, bad_o = X64[fr].T @ X64[fr], Y5[fr].T @ X64[fr]
        if fault == "neighbour_row_added":
            yt = np.concatenate([b.yt_of(c), b.yt_of((c + 1) % b.C)[:, :1]], axis=1)
        else:
            yt = b.yt_of(c)[:, :len(fr)]
        bad_r = rc.xty_ref(b.X, yt, fr)[0]
        if fault == "ragged_column_zeroed":
            bad_g[:, D - 1] = 0.0
            bad_g[D - 1, :] = 0.0
            bad_o[:, D - 1] = 0.0
            bad_r[:, D - 1] = 0.0
        if fault == "entry_off_1e-10":
            for a in (bad_g, bad_o, bad_r):
                i = np.unravel_index(np.abs(a).argmax(), a.shape)
                a[i] *= 1.0 + 1e-10
        before = np.random.default_rng(c).standard_normal(G.shape)
        assert rc.ratio(bad_g, G, bound) > 1.0 and rc.tril_ratio(before + bad_g, before, G, bound) > 1.0, (fault, c)
        assert rc.ratio(bad_o, O5, b5) > 1.0, (fault, c)
        assert rc.ratio(bad_r, R5, br) > 1.0, (fault, c)


def test_a_missing_row_exceeds_the_gram_bound_on_every_entry():
    b = rc.Batch(72, [33, 100, 3000], seed=9)
    for rows in b.rows:
        G, bound = rc.gram_ref(b.X, rows)
        bad = rc.gram_ref(b.X, rows[1:])[0]
        assert float((np.abs(bad - G) / bound).min()) > 100.0


def test_checkers_reject_non_finite_results():
    b = rc.Batch(8, [17], seed=2)
    G, bound = rc.gram_ref(b.X, b.rows[0])
    bad = G.copy()
    bad[3, 1] = np.nan
    assert rc.ratio(bad, G, bound) == np.inf and rc.tril_ratio(bad, np.zeros_like(G), G, bound) == np.inf
    assert rc.ratio(np.zeros((8, 8)), *rc.gram_ref(b.X, [])) == 0.0            # an empty class: exact zeros pass,
    assert rc.ratio(np.full((8, 8), 1e-300), *rc.gram_ref(b.X, [])) == np.inf   # nothing else does


def test_xty_checker_accepts_another_summation_order():
    worst = 0.0
    for D, C, b in _batches(rc.GRAM_DS + rc.NT_DS, rc.GRAM_CS):
        X1 = np.concatenate([b.X.astype(np.float64), np.ones((b.nX, 1))], axis=1)
        for c, rows in enumerate(b.rows):
            R5, bound = rc.xty_ref(b.X, b.yt_of(c), rows)
            Y5 = np.concatenate([b.yt_of(c), np.ones((1, len(rows)))], axis=0)
            alt = None
            for s in reversed(range(0, max(len(rows), 1), 32)):
                part = Y5[:, s:s + 32] @ X1[rows[s:s + 32]]
                alt = part if alt is None else alt + part
            worst = max(worst, rc.ratio(alt, R5, bound))
    for nc in rc.ONE_CLASS_NCS:
        b = rc.Batch(72, [nc], seed=nc)
        R5, bound = rc.xty_ref(b.X, b.yt_of(0), b.rows[0])
        X1 = np.concatenate([b.X.astype(np.float64), np.ones((b.nX, 1))], axis=1)
        alt = np.concatenate([b.yt_of(0), np.ones((1, nc))], axis=0)[:, ::-1] @ X1[b.rows[0][::-1]]
        worst = max(worst, rc.ratio(alt, R5, bound))
    assert worst <= 1.0, worst


def _fold_f64(O5, st, cnt):
    """The fold as the kernel states it, in plain f64."""
    D = O5.shape[1]
    v = O5[:4] - st[0][:, None] * O5[4][None, :]
    xy = np.zeros((4, D + 1))
    for j in range(4):
        t = np.zeros(D)
        for i in range(4):
            t = t + v[i] * st[1 + i, j]
        xy[j, :D] = t
    return xy


@pytest.mark.parametrize("D", rc.FOLD_DS)
@pytest.mark.parametrize("C", rc.FOLD_CS)
def test_fold_checker_accepts_f64_and_rejects_a_wrong_entry(D, C):
    L = rc.class_lengths(C, k=1) if C > 1 else [33]
    if C > 1:
        L[1] = 1
    b = rc.Batch(D, L, seed=D + C)
    st = rc.stats_of(np.random.default_rng(D), C)
    for c, rows in enumerate(b.rows):
        O5 = rc.o5_ref(b.X, b.Yraw, rows)[0]
        xy, bias, bound = rc.fold_ref(O5, st[c], len(rows))
        got = _fold_f64(O5, st[c], len(rows))
        assert rc.ratio(got, xy, bound) <= 1.0, c
        assert np.array_equal(bias[:D], O5[4]) and bias[D] == len(rows) and np.all(xy[:, D] == 0.0)
        if len(rows):
            with np.errstate(divide="ignore", invalid="ignore"):
                i = np.unravel_index(np.nan_to_num(np.abs(xy) / bound, posinf=0.0).argmax(), xy.shape)
            bad = got.copy()
            bad[i] *= 1.0 + 1e-10
            assert rc.ratio(bad, xy, bound) > 1.0, c
            swapped = _fold_f64(O5, np.concatenate([st[c][:1], st[c][1:5].T, st[c][5:]]), len(rows))   # T' for T
            assert rc.ratio(swapped, xy, bound) > 1.0, c
            nomean = _fold_f64(O5, np.concatenate([st[c][:1] * (1 + 1e-9), st[c][1:]]), len(rows))    # the mean off by 1e-9
            assert rc.ratio(nomean, xy, bound) > 1.0, c


@pytest.mark.parametrize("D", rc.PREDICT_DS)
def test_predict_checker(D):
    rng = np.random.default_rng(D)
    b = rc.Batch(D, list(rc.PREDICT_LENGTHS), seed=D)
    W = rng.standard_normal((b.C, 4, D + 2))
    for c, rows in enumerate(b.rows):
        P, bound = rc.predict_ref(b.X, W[c], rows)
        X1 = np.concatenate([b.X[rows].astype(np.float64), np.ones((len(rows), 1))], axis=1)
        alt = np.zeros((len(rows), 4))
        for lane in range(64):                                   # a lane's strided columns, then the lanes: the kernels' order
            cols = np.arange(lane, D, 64)
            alt += X1[:, cols] @ W[c][:, cols].T
        alt += W[c][:, D][None, :]
        assert rc.ratio(alt, P, bound) <= 1.0
        if len(rows):
            bad = alt.copy()
            bad[-1, 2] *= 1.0 + 1e-10
            assert rc.ratio(bad, P, bound) > 1.0
            assert rc.ratio(alt - W[c][:, D][None, :], P, bound) > 1.0                      # the bias forgotten
            if D > 1:
                assert rc.ratio(X1[:, :D - 1] @ W[c][:, :D - 1].T + W[c][:, D], P, bound) > 1.0   # the last column forgotten
            other = rc.predict_ref(b.X, W[(c + 1) % b.C], rows)[0]
            assert rc.ratio(other, P, bound) > 1.0                                         # the neighbouring class's weights


def _substitute(A, B, skip=None):
    """Block substitution with the Cholesky factor in 128-row blocks (what rls_substitute_kernel does), optionally with one
    off-diagonal block of the forward sweep skipped."""
    import scipy.linalg as sla
    D1 = A.shape[0]
    L = np.linalg.cholesky(A)
    nb = (D1 + 127) // 128
    y = np.zeros((D1, 4))
    for k in range(nb):
        r = slice(128 * k, min(128 * (k + 1), D1))
        t = B.T[r].copy()
        for j in range(k):
            if skip == (k, j):
                continue
            cj = slice(128 * j, 128 * (j + 1))
            t -= L[r, cj] @ y[cj]
        y[r] = sla.solve_triangular(L[r, r], t, lower=True)
    return sla.solve_triangular(L.T, y, lower=False).T


@pytest.mark.parametrize("D", rc.SOLVE_DS)
def test_solve_eta_accepts_scipy_and_rejects_a_skipped_block(D):
    D1 = D + 1
    rng = np.random.default_rng(D)
    for lam in rc.SOLVE_LAMS:
        etas, systems = [], []
        for regime in range(3):
            G, B = rc.solve_system(rng, D, regime)
            A = rc.sym_from_lower(G, D1, lam)
            assert np.array_equal(A, A.T)
            W = rc.reference_solve(A, B[:, :D1])
            etas += [rc.solve_eta(A, W[q], B[q, :D1]) for q in range(4)]
            systems.append((A, B[:, :D1], W))
        bar = rc.solve_bar(D1, etas)
        assert bar < 1e-12, (D, lam, bar)                        # the reference itself is backward stable: the bar is tight
        for A, B, W in systems:
            own = _substitute(A, B)
            assert max(rc.solve_eta(A, own[q], B[q]) for q in range(4)) <= bar
            if D1 > 128:
                skipped = _substitute(A, B, skip=((D1 + 127) // 128 - 1, 0))
                assert min(rc.solve_eta(A, skipped[q], B[q]) for q in range(4)) > bar
            assert rc.solve_eta(A, np.full(D1, np.nan), B[0]) == np.inf
