"""f64 references, entrywise rounding bounds and the test problems of the RLS kernels (csrc/rls.hip) — plain numpy, no GPU.

Every reference comes with the bound its kernel has to meet ENTRY BY ENTRY, derived from the number formats alone (u = 2^-53,
the unit roundoff of f64) — never from what a kernel returns:

  gram_ref     X_c' X_c            2 len u |X|'|X|                 (f32 x f32 products are exact in f64: only the sums round —
  o5_ref       [Y 1]' X_c          2 len u |[Y 1]|'|X|              len u for the kernel's order, len u for numpy's)
  xty_ref      [Yt; 1] [X 1]       2 (len + 1) u |[Yt; 1]| |[X 1]|  (f32 x f64 products round: one more u)
  fold_ref     ((X'Y - X'1 mu') T)'  8 u (absolute sum of the terms)  (reference in extended precision where numpy has it)
  predict_ref  [X 1] W'            2 (D + 2) u |[X 1]| |W|'
  solve_eta    normwise backward error of a solve; its bar is 16 x what scipy's Cholesky reaches on the same systems
               (solve_bar), never below D1 u.

tests/test_rls_checks_host.py shows on the CPU that every checker accepts numpy's / scipy's own results on the GPU file's shapes and
rejects planted faults of the size a wrong kernel would make; tests/test_gpu_rls_kernels.py holds the kernels to them.
"""
import numpy as np

U = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------- the shapes
# D of the Gram tests and what each isolates in rls_gram_rows32_kernel (128 x 64 tiles, half tiles at j0 == i0 + 64)
GRAM_DS = (8,      # one tile, 120 masked columns
           64,     # tiles_n == 1 (the heavy-first order's tiles_n - 1 divisor)
           72,     # first half tile, ragged by 8
           128,
           136,    # second tile row 8 wide
           200,
           328,
           1032)   # nine tile rows: the 8 * (local / tiles_n) wrap of the XCD-rotated order, tiles_n = 17
GRAM_CS = (1, 3, 32)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100)       # around the 16-row padding and the 32-row k-tile
NT_DS = (70, 129)                                                # D % 8 != 0: transposed f64 copy + NT GEMM
ONE_CLASS_NCS = (1, 17, 513)                                     # odx_rls_gram_f64
FOLD_DS, FOLD_CS = (8, 72, 1032), (1, 32)
SOLVE_DS = (1, 7, 126, 127, 128, 255, 256, 1032)                 # D1 on both sides of the 128-row blocks
SOLVE_CS = (1, 5, 32)
SOLVE_LAMS = (10.0, 1000.0)
PREDICT_DS = (1, 3, 70, 72, 1024, 2048)
PREDICT_LENGTHS = (0, 1, 3, 4, 5, 33)                            # a wave owns four rows of one class


def class_lengths(C, k=0):
    """C class sizes cycling through LENGTHS from position k.  C = 32 (k = 0) has an empty class first (0), in the middle (12, 24)
    and last (31, forced)."""
    L = [LENGTHS[(k + c) % len(LENGTHS)] for c in range(C)]
    if C >= 3:
        L[-1] = 0
    if C == 1 and L[0] == 0:
        L[0] = 33
    return L


class Batch:
    """A class batch as the batched entries take it: X (nX, D) f32 with more rows than any class uses, Yraw (nX, 4) f32 raw targets
    by row id (means far above their spread), row ids a random permutation, class segments padded to 16 with -1, whitened targets
    Yt (4, npad) f64 in the padded order (zero in the padding).  Row 0 and the permutation's tail belong to no class."""

    def __init__(self, D, lengths, seed=0, spare=37):
        rng = np.random.default_rng(seed)
        self.D, self.lengths, self.C = D, [int(v) for v in lengths], len(lengths)
        total = sum(self.lengths)
        self.nX = total + spare + 1
        self.X = (rng.standard_normal((self.nX, D)) * 0.5 + 0.1).astype(np.float32)
        self.Yraw = (rng.standard_normal((self.nX, 4)) * 0.05 + np.array([40.0, -25.0, 3.0, 0.0])).astype(np.float32)
        perm = rng.permutation(self.nX - 1) + 1
        self.unused = np.concatenate(([0], perm[total:]))
        self.rows, self.seg_off, at, used = [], [], 0, 0
        for n in self.lengths:
            self.rows.append(perm[used:used + n].astype(np.int64))
            self.seg_off.append(at)
            used += n
            at += (n + 15) // 16 * 16
        self.npad = at
        self.idx_pad = np.full(self.npad, -1, dtype=np.int64)
        self.Yt = np.zeros((4, max(self.npad, 16)))
        for c, r in enumerate(self.rows):
            self.idx_pad[self.seg_off[c]:self.seg_off[c] + len(r)] = r
            self.Yt[:, self.seg_off[c]:self.seg_off[c] + len(r)] = rng.standard_normal((4, len(r)))
        self.run = np.concatenate(self.rows) if total else np.zeros(0, dtype=np.int64)

    def yt_of(self, c):
        return self.Yt[:, self.seg_off[c]:self.seg_off[c] + self.lengths[c]]

    def poison(self):
        """Inf / NaN in every row that belongs to no class (X and Yraw): a kernel that touches them arithmetically shows it."""
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        for i, r in enumerate(self.unused):
            self.X[r, :] = bad[i % 3]
            self.Yraw[r, :] = bad[(i + 1) % 3]
        return self


def stats_of(rng, C):
    """(C, 9, 4) f64 = [mu; T; T_inv] per class with means far above the spread (the fold's subtraction cancels), cnt (C)."""
    st = np.zeros((C, 9, 4))
    for c in range(C):
        st[c, 0] = np.array([40.0, -25.0, 3.0, 0.0]) + 0.01 * rng.standard_normal(4)
        T = np.triu(rng.standard_normal((4, 4))) + 4.0 * np.eye(4)
        st[c, 1:5] = T * 10.0
        st[c, 5:9] = np.linalg.inv(st[c, 1:5])
    return st


# ---------------------------------------------------------------------------------------------------------------- references
def gram_ref(X, rows, D=None):
    """(G, bound): G = X[rows]' X[rows] in f64 over the first D columns; |kernel - G| <= bound entry by entry for any order of the
    sums (len u for the kernel, len u for this product).  A class of no rows: exact zeros."""
    D = X.shape[1] if D is None else D
    Xr = X[np.asarray(rows, dtype=np.int64), :D].astype(np.float64)
    n = Xr.shape[0]
    A = np.abs(Xr)
    return Xr.T @ Xr, 2.0 * n * U * (A.T @ A)


def o5_ref(X, Yraw, rows, D=None):
    """(O5, bound): [Y 1]' X (5 x D) of the raw f32 targets, bound of gram_ref's form with |[Y 1]|."""
    D = X.shape[1] if D is None else D
    rows = np.asarray(rows, dtype=np.int64)
    Xr = X[rows, :D].astype(np.float64)
    n = Xr.shape[0]
    Y5 = np.concatenate([Yraw[rows, :4].astype(np.float64), np.ones((n, 1))], axis=1)
    return Y5.T @ Xr, 2.0 * n * U * (np.abs(Y5).T @ np.abs(Xr))


def xty_ref(X, Yt, rows, D=None):
    """(R5, bound), both (5, D + 1): rows 0..3 = Yt [X 1] for the whitened f64 targets Yt (4, len) of the rows, row 4 = 1' [X 1] (the
    Gram's bias row: column sums and the row count).  The f32 x f64 products round: 2 (len + 1) u |[Yt; 1]| |[X 1]|."""
    D = X.shape[1] if D is None else D
    rows = np.asarray(rows, dtype=np.int64)
    n = len(rows)
    X1 = np.concatenate([X[rows, :D].astype(np.float64), np.ones((n, 1))], axis=1)
    Y5 = np.concatenate([np.asarray(Yt, dtype=np.float64).reshape(4, n), np.ones((1, n))], axis=0)
    return Y5 @ X1, 2.0 * (n + 1) * U * (np.abs(Y5) @ np.abs(X1))


def _wide():
    return np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64


def fold_ref(O5, stats, cnt):
    """One class: (XtY (4, D + 1), bias (D + 1), bound (4, D + 1)) from the kernel's OWN O5 (5, >= D; D = the columns handed over),
    stats (9, 4) = [mu; T; T_inv] and the row count: XtY[j][d] = sum_i (O5[i][d] - mu_i O5[4][d]) T[i][j], XtY[j][D] = 0, bias =
    (O5[4], cnt).  Evaluated in extended precision; the kernel's eight roundings per entry (product, difference, four multiply-adds,
    and slack) are bounded on the ABSOLUTE sum of the terms — the difference cancels.  The bias row is a copy: exact."""
    w = _wide()
    O5 = np.asarray(O5, dtype=np.float64)
    D = O5.shape[1]
    mu, T = stats[0].astype(w), stats[1:5].astype(w)
    o, ones = O5[:4].astype(w), O5[4].astype(w)
    v = o - mu[:, None] * ones[None, :]                               # (4, D)
    xy = np.zeros((4, D + 1))
    xy[:, :D] = (T.T @ v).astype(np.float64)
    absum = np.abs(stats[1:5]).T @ (np.abs(O5[:4]) + np.abs(stats[0])[:, None] * np.abs(O5[4])[None, :])
    bound = np.zeros((4, D + 1))
    bound[:, :D] = 8.0 * U * absum
    bias = np.concatenate([O5[4], [float(cnt)]])
    return xy, bias, bound


def predict_ref(X, W, rows, D=None):
    """(P (len, 4), bound): [X 1] W' in f64 for W (4, >= D + 1); 2 (D + 2) u |[X 1]| |W|'."""
    D = X.shape[1] if D is None else D
    rows = np.asarray(rows, dtype=np.int64)
    X1 = np.concatenate([X[rows, :D].astype(np.float64), np.ones((len(rows), 1))], axis=1)
    Wd = np.asarray(W, dtype=np.float64)[:, :D + 1]
    return X1 @ Wd.T, 2.0 * (D + 2) * U * (np.abs(X1) @ np.abs(Wd).T)


# ---------------------------------------------------------------------------------------------------------------- checkers
def ratio(got, ref, bound):
    """max over the entries of |got - ref| / bound (0 / 0 = 0, x / 0 = inf; a non-finite entry of got = inf): <= 1 passes."""
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(q.max())


def added_ratio(after, before, ref, bound):
    """The same for a kernel that ADDS its result into a pre-filled buffer: after = fl(before + result).  That sum rounds once
    (u |after| <= u (|before| + |ref|) to first order) and the two subtractions here round again, each on a quantity no larger:
    4 u (|before| + |ref|) on top of the bound covers the three."""
    after, before = np.asarray(after, dtype=np.float64), np.asarray(before, dtype=np.float64)
    if after.size and not np.all(np.isfinite(after)):
        return np.inf
    return ratio(after - before, ref, np.asarray(bound) + 4.0 * U * (np.abs(before) + np.abs(ref)))


def tril_ratio(after, before, ref, bound):
    """added_ratio on the lower triangle (diagonal included) of square blocks."""
    i, j = np.tril_indices(ref.shape[0])
    return added_ratio(after[i, j], before[i, j], ref[i, j], bound[i, j])


def sym_from_lower(G, D1, lam):
    """The matrix a solve sees: the lower triangle of G (D1 x >= D1) mirrored, + lam I."""
    L = np.tril(np.asarray(G, dtype=np.float64)[:D1, :D1])
    return L + np.tril(L, -1).T + lam * np.eye(D1)


def solve_eta(A, w, b):
    """Normwise backward error of w as a solution of A w = b: ||A w - b||_inf / (||A||_inf ||w||_inf + ||b||_inf)."""
    A, w, b = np.asarray(A, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.all(np.isfinite(w)):
        return np.inf
    den = np.abs(A).sum(axis=1).max() * np.abs(w).max() + np.abs(b).max()
    return float(np.abs(A @ w - b).max() / den) if den > 0 else 0.0


def solve_system(rng, D, regime):
    """(G (D1, ld) lower triangle of [X 1]'[X 1] for n random rows — the strict upper part holds junk no solve may read —, B (4, ld)):
    regime 0: n < D (lam carries the conditioning), 1: n ~ D, 2: n >> D."""
    D1 = D + 1
    ld = (D1 + 1) // 2 * 2
    n = (max(1, D // 2), D + 1, 2 * D + 5)[regime]
    X1 = np.concatenate([rng.standard_normal((n, D)) * 0.5 + 0.1, np.ones((n, 1))], axis=1)
    full = X1.T @ X1
    G = np.zeros((D1, ld))
    G[:, :D1] = np.tril(full) + np.triu(rng.standard_normal((D1, D1)) * 7.0, 1)
    B = np.zeros((4, ld))
    B[:, :D1] = rng.standard_normal((4, n)) @ X1
    return G, B


def reference_solve(A, B):
    """scipy's Cholesky solve of A W' = B' (B (4, D1)) -> W (4, D1): the reference whose backward error sets the kernels' bar."""
    import scipy.linalg as sla
    cf = sla.cho_factor(A, lower=True)
    return sla.cho_solve(cf, np.asarray(B).T).T


def solve_bar(D1, ref_etas):
    """The kernels' bar for eta on a family of systems: 16 x the largest eta scipy reaches on them (one digit for a different
    blocking and the explicit inverses of the 128 x 128 diagonal blocks), never below D1 u."""
    return max(16.0 * max(ref_etas), D1 * U)
