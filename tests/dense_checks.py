"""f64 references, bars and test problems of the preconditioner chain (csrc/dense_f64.hip) and of the CG updates (csrc/cg.hip) —
plain numpy / scipy, no GPU.

The chain (two blocked Choleskys, T T'/M, two triangular inverses by pairwise merging) is held to BACKWARD errors, each with a bar
computed from the same matrix by scipy — never from a kernel:

  chol_eta(A, L)      max |A - L L'| / max (|L| |L|')         L lower, strict upper part EXACTLY zero (else inf)
  inv_eta(L, Li)      max(max |Li L - I| / max (|Li| |L|), max |L Li - I| / max (|L| |Li|))       Li lower, exactly
  transposes(Li, Lit) Li' == Lit bit for bit (one dual store writes both)
  precond_eta(K, Li)  max |Li K Li' - I|                       K = K_MM + eps M I in f64 from the f32 centres
  precond_a_eta(LTi, LAi, lam)  the same for the A factor against T T'/M + lam I of the chain's OWN T (its docstring says why)

  bar = max(16 x the figure scipy's cholesky / trtri reaches on the same matrix, (M + 1) u)         u = 2^-53
  (16: the margin this project gives its RLS solves, tests/rls_checks.py — the chain multiplies by explicit inverses of its
  diagonal blocks where LAPACK substitutes, and sums in another order)

(max (|L| |L|') is the largest squared row norm of L — Cauchy-Schwarz puts the maximum of |L| |L|' on its diagonal — so chol_eta
needs one product, not two.)

The A factor on the split-f16 route keeps the bars the project already holds (test_precond_split_path): |Li S Li' - I| < 2e-4,
relative difference to the f64 route < 1e-4 and != 0, T factors bit-identical (SPLIT_RESID, SPLIT_REL).

The CG updates are the seven statements of tests/oracle_backend.py (imported, not copied) with entrywise bounds from the formats:
a sum of M products 2 M u sum |p_i q_i| (M u for either order); the step a = rs / (s + eps) and b from that; then X, R, P, S entry
by entry (cg_*_ref below).  tests/test_dense_checks_host.py shows what every checker accepts and rejects."""
import numpy as np
import scipy.linalg as sla

from tests.rls_checks import U, ratio  # noqa: F401 — ratio is part of this module's interface

NB, NBO = 128, 512                    # inner block and outer panel of potrf_f64; merge levels s = 128, 256, ... < M
SPLIT_RESID, SPLIT_REL = 2e-4, 1e-4

# M of the factorisation tests and what each isolates
SIZES = {
    1: "one entry: the pivot's rsqrt + Newton steps alone",
    127: "one ragged diagonal block (identity padding of one row / column)",
    128: "exactly one diagonal block: no panel solve, no merge level",
    129: "first panel solve and first merge level (s = 128) with a second block of ONE row; odd M: pad column",
    511: "one outer panel, last inner block ragged by one",
    512: "exactly one outer panel: no rank-512 update",
    513: "first rank-512 update (thin part only, one row); first s = 512 merge level, second block of one row",
    640: "second panel of one inner block: rank-512 update 128 wide, no look-ahead",
    1024: "two full panels: the thin update is the whole trailing matrix (mr = 0, no helper launch)",
    1025: "first look-ahead launch on the helper stream, mr = 1",
    1536: "three full panels: second look-ahead launch waits for the first join",
    1537: "first reuse of packed-panel slot 0 (panel 2) while panel 0's helper GEMM is two joins back; s = 512 with a ragged third pair",
    2049: "s = 2048 merge level with a one-row second block; four look-ahead launches",
    2177: "fifth panel: 128 + a last inner block of ONE row",
    2600: "largest: six panels, ragged everything (the size test_precond_split_path ends at)",
}
ALL_M = tuple(SIZES)
BIG_M = (2049, 2177, 2600)            # taken once each where a host test would otherwise repeat them
PRECOND_CASES = ((513, 36), (1025, 64), (1537, 256), (2177, 36), (2600, 64))       # (M, D) of the preconditioner tests
HELPER_M = (1025, 1537, 2600)
CG_MS = (1, 2, 1023, 1024, 1025, 20001)                                             # around the 1024-thread workgroup; many strides
SCORE_NS = (1, 255, 257, 70001)                                                     # around the 256-thread block; past the grid cap


def merge_fallback_reachable(max_m=65536):
    """Smallest M < max_m for which a merge level s >= 512 of trtri_from_diag_f64 does not fit the pack scratch
    (2 szr + 2 nbe s^2 > pk_cap = 2 M roundup(M, 64)) and falls back to the f64 GEMMs — or None.  The arithmetic of that function,
    restated: the packs hold at most 4 nbe s^2 units and nbe = ceil((M - s) / 2s) pairs of 2s rows cover M + s rows at most."""
    for M in range(513, max_m):
        cap = 2 * M * ((M + 63) // 64 * 64)
        s = NB
        while s < M:
            if s >= 512:
                nbe = -(-(M - s) // (2 * s))
                m2l = M - s - (nbe - 1) * 2 * s
                szr = (nbe - 1) * s * s + min(m2l, s) * s
                if 2 * szr + 2 * nbe * s * s > cap:
                    return M, s
            s *= 2
    return None


# ---------------------------------------------------------------------------------------------------------------- problems
def spd_well(M, seed=0):
    """A well-conditioned SPD matrix (cond ~ 30): G G' / (M + 20) + 0.1 I."""
    rng = np.random.default_rng(1000 + M + seed)
    G = rng.standard_normal((M, M + 20))
    return G @ G.T / (M + 20) + 0.1 * np.eye(M)


def centres(M, D, seed=0):
    """(M, D) f32 centres of norm ~ 20 whose second half are near-duplicates of the first (the case test_batched_precond... builds)."""
    rng = np.random.default_rng(7000 + 31 * M + D + seed)
    Z = (rng.standard_normal((M, D)) * (20.0 / np.sqrt(D))).astype(np.float32)
    h = M // 2
    if h:
        Z[h:] = Z[:M - h] + 0.01 * rng.standard_normal((M - h, D)).astype(np.float32)
    return Z


def kmm(Z, sigma, eps):
    """K_MM + eps M I in f64 from f32 centres: exp(-max(0, |z_i|^2 + |z_j|^2 - 2 z_i . z_j) / (2 sigma^2))."""
    Zd = np.asarray(Z, dtype=np.float64)
    sq = (Zd * Zd).sum(axis=1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2.0 * (Zd @ Zd.T), 0.0)
    K = np.exp(d2 * (-0.5 / (sigma * sigma)))
    K = 0.5 * (K + K.T)
    K[np.diag_indices(len(Zd))] = 1.0 + eps * len(Zd)
    return K


def spd_kernel(M, D=36, sigma=9.0, eps=1e-5, seed=0):
    """(Z, K): the real, ill-conditioned case — near-duplicate centres, jitter eps M."""
    Z = centres(M, D, seed)
    return Z, kmm(Z, sigma, eps)


def problem(kind, M):
    return spd_well(M) if kind == "well" else spd_kernel(M)[1]


def padded_lower(A, fill=0.0):
    """(M, ld) with ld = M rounded up to even: the lower triangle of A; the strict upper triangle and the pad column hold `fill`."""
    M = A.shape[0]
    out = np.full((M, (M + 1) // 2 * 2), fill, dtype=np.float64)
    i, j = np.tril_indices(M)
    out[i, j] = A[i, j]
    return out


# ---------------------------------------------------------------------------------------------------------------- references
def ref_chol(A):
    return sla.cholesky(A, lower=True, check_finite=False)


def ref_inv(L):
    Li, info = sla.lapack.dtrtri(L, lower=1)
    assert info == 0
    return np.tril(Li)


def blocked_chol(A, fault=None):
    """The chain's factorisation stated in numpy, summed in ANOTHER order than scipy: outer panels of 512, inner blocks of 128, panel
    solves by the explicit inverse of the diagonal block, the trailing matrix updated once per outer panel.  fault (planted, for the
    host tests): ("skip", p) leaves out panel p's rank-512 update; ("stale", p, q) applies panel p's update from the columns of the
    EARLIER panel q (what a packed slot overwritten too late, or read too early, would feed the GEMM: q = p - 2 shares p's slot)."""
    A = np.tril(A).copy()
    M = A.shape[0]
    for p, K0 in enumerate(range(0, M, NBO)):
        K1 = min(K0 + NBO, M)
        for k0 in range(K0, K1, NB):
            k1 = min(k0 + NB, M)
            L11 = sla.cholesky(A[k0:k1, k0:k1] + np.tril(A[k0:k1, k0:k1], -1).T, lower=True, check_finite=False)
            A[k0:k1, k0:k1] = L11
            if k1 < M:
                X = np.linalg.inv(L11)
                A[k1:, k0:k1] = A[k1:, k0:k1] @ X.T
                if k1 < K1:
                    A[k1:, k1:K1] -= A[k1:, k0:k1] @ A[k1:K1, k0:k1].T
        if K1 < M:
            if fault == ("skip", p):
                continue
            stale = fault is not None and fault[:2] == ("stale", p)
            P = A[K1:, fault[2] * NBO:(fault[2] + 1) * NBO] if stale else A[K1:, K0:K1]
            A[K1:, K1:] -= P @ P.T
    return np.tril(A)


def merge_inv(L, fault=None):
    """L^-1 by the chain's pairwise merging of inverted 128-blocks: [X11 0; X21 X22], X21 = -X22 (L21 X11), s = 128, 256, ...
    fault "skip_last_pair": the ragged last pair of the top level is left unmerged (its X21 stays zero)."""
    M = L.shape[0]
    X = np.zeros((M, M))
    for k0 in range(0, M, NB):
        k1 = min(k0 + NB, M)
        X[k0:k1, k0:k1] = np.linalg.inv(L[k0:k1, k0:k1])
    s = NB
    while s < M:
        starts = [r for r in range(0, M, 2 * s) if r + s < M]
        for r in starts:
            if fault == "skip_last_pair" and 2 * s >= M and r == starts[-1]:
                continue
            m, e = r + s, min(r + 2 * s, M)
            X[m:e, r:m] = -X[m:e, m:e] @ (L[m:e, r:m] @ X[r:m, r:m])
        s *= 2
    return X


# ---------------------------------------------------------------------------------------------------------------- checkers
def _lower_exact(L):
    L = np.asarray(L)
    return bool(np.all(np.isfinite(L))) and not np.any(np.triu(L, 1))


def chol_eta(A, L):
    if not _lower_exact(L):
        return np.inf
    return float(np.abs(A - L @ L.T).max() / (L * L).sum(axis=1).max())


def inv_eta(L, Li):
    if not _lower_exact(Li):
        return np.inf
    eye = np.eye(L.shape[0])
    aL, aX = np.abs(L), np.abs(Li)
    left = np.abs(Li @ L - eye).max() / (aX @ aL).max()
    right = np.abs(L @ Li - eye).max() / (aL @ aX).max()
    return float(max(left, right))


def transposes(Li, Lit):
    Li, Lit = np.ascontiguousarray(Li), np.ascontiguousarray(Lit)
    return Li.shape == Lit.shape[::-1] and np.array_equal(np.ascontiguousarray(Li.T).view(np.uint64), Lit.view(np.uint64))


def precond_eta(K, Li):
    if not _lower_exact(Li):
        return np.inf
    return float(np.abs(Li @ K @ Li.T - np.eye(K.shape[0])).max())


def precond_a_eta(LTi, LAi, lam):
    """max |LAi S LAi' - I| for the A factor, S = T T'/M + lam I the matrix the chain ITSELF factors: T' = L_T is the inverse of the
    LTi it returned, applied by substitution (W = L_T LAi' solves LTi W = LAi'; S never formed): max |W'W / M + lam LAi LAi' - I|.
    Why not S from scipy's factor of K: a Cholesky factor is only BACKWARD stable, so two correct factors of K (scipy's, the
    chain's) differ by cond(K) u, and S built from one of them is not the matrix the other chain factored — measured on the CPU
    with two numpy factorisations (M = 513, cond(K) = 2e3): 2.4e-14 against the foreign S, 7.8e-16 against its own, 2.4e-15 by
    this substitution; scipy's own figure 7.8e-16.  The T factor is held to K by precond_eta; this holds the A factor to that T.
    The bar is precond_bar of S built from scipy's factor (the same matrix up to that difference)."""
    if not _lower_exact(LAi) or not _lower_exact(LTi):
        return np.inf
    M = LAi.shape[0]
    W = sla.solve_triangular(LTi, LAi.T, lower=True, check_finite=False)
    return float(np.abs(W.T @ W / M + lam * (LAi @ LAi.T) - np.eye(M)).max())


def _bar(M, ref):
    return max(16.0 * ref, (M + 1) * U)


def chol_bar(A, L=None):
    """(bar, scipy's own figure) for chol_eta on A."""
    ref = chol_eta(A, ref_chol(A) if L is None else L)
    return _bar(A.shape[0], ref), ref


def inv_bar(L, Li=None):
    """(bar, scipy's own figure) for inv_eta on the factor L handed to the inversion (Li: scipy's inverse of it, if at hand)."""
    ref = inv_eta(L, ref_inv(L) if Li is None else Li)
    return _bar(L.shape[0], ref), ref


def precond_bar(K, Li=None):
    """(bar, scipy's own figure) for precond_eta on K: scipy's Cholesky factor inverted by its trtri (Li, if at hand)."""
    ref = precond_eta(K, ref_inv(ref_chol(K)) if Li is None else Li)
    return _bar(K.shape[0], ref), ref


def split_figures(S, Li_split, Li_f64):
    """(max |Li S Li' - I|, relative Frobenius difference to the f64 route) of an A factor made on the split-f16 route."""
    resid = float(np.abs(Li_split @ S @ Li_split.T - np.eye(S.shape[0])).max())
    return resid, float(np.linalg.norm(Li_split - Li_f64) / np.linalg.norm(Li_f64))


# ---------------------------------------------------------------------------------------------------------------- CG updates
# state = [rs_old, rs_new, stop flag, last step].  Every reference runs the statement of tests/oracle_backend.py on copies and returns
# (values, bounds): dicts of the vectors / state words the kernel may write.  A kernel output passes when |got - ref| <= bound entry
# by entry (cg_ratio <= 1); what the statement leaves alone has bound 0: bit for bit.
def _oracle():
    from tests.oracle_backend import OracleBackend
    return OracleBackend()


def _t(*arrays):
    import torch
    return [torch.from_numpy(np.array(a, dtype=np.float64, copy=True)) for a in arrays]


def dot_bound(p, q):
    """|fl(sum p_i q_i) - reference| for ANY order of the M additions on either side, products fused or not: 2 M u sum |p_i q_i|."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return 2.0 * max(len(p), 1) * U * float(np.abs(p * q).sum())


def _quotient_bound(num, dnum, den, dden):
    """|fl(n' / d') - n / d| for |n' - n| <= dnum, |d' - d| <= dden, the division rounded once on either side (2 u): first order
    in dnum, exact in dden (the denominator may cancel)."""
    lo = abs(den) - dden
    if not lo > 0.0:
        return np.inf
    return dnum / lo + abs(num) * dden / (abs(den) * lo) + 2.0 * U * (abs(num) + dnum) / lo


def cg_init_ref(B):
    B = np.asarray(B, dtype=np.float64)
    b, x, r, p = _t(B, np.ones_like(B), np.ones_like(B), np.ones_like(B))
    st, = _t(np.full(4, 7.0))
    _oracle().cg_init(b, x, r, p, st)
    ds = dot_bound(B, B)
    zero = np.zeros_like(B)
    return ({"X": x.numpy(), "R": r.numpy(), "P": p.numpy(), "state": st.numpy()},
            {"X": zero, "R": zero, "P": zero, "state": np.array([ds, ds, 0.0, 0.0])})


def cg_step_ref(X, R, P, AP, state, cg_eps, full_grad):
    """X += a P, R -= a AP (unless full_grad), state[3] = a with a = state[0] / (P . AP + eps); nothing once the flag is up.
    |da| from dot_bound through the quotient (the sum s + eps rounds once more: u |s + eps| on either side); an updated entry
    x + a p carries |p| da and the roundings of either side (the statement rounds product and sum, the kernel's fused multiply-add once):
    u |a p| + 2 u |x + a p| <= 3 u (|x| + |a p|)."""
    X, R, P, AP, state = (np.asarray(v, dtype=np.float64) for v in (X, R, P, AP, state))
    x, r, p, ap, st = _t(X, R, P, AP, state)
    _oracle().cg_step(x, r, p, ap, st, cg_eps, full_grad)
    vals = {"X": x.numpy(), "R": r.numpy(), "state": st.numpy()}
    zero = np.zeros_like(X)
    if state[2] != 0.0:
        return vals, {"X": zero, "R": zero, "state": np.zeros(4)}
    s = float(P @ AP)
    den = s + cg_eps
    da = _quotient_bound(state[0], 0.0, den, dot_bound(P, AP) + 2.0 * U * abs(den))
    a = abs(state[0] / den)
    bx = np.abs(P) * da + 3.0 * U * (np.abs(X) + a * np.abs(P))
    br = zero if full_grad else np.abs(AP) * da + 3.0 * U * (np.abs(R) + a * np.abs(AP))
    return vals, {"X": bx, "R": br, "state": np.array([0.0, 0.0, 0.0, da])}


def cg_finish_ref(R, P, state, cg_eps, tol):
    """s = R . R; sqrt |s| < tol (STRICT): state[1] = s, flag up, P untouched; else P = b P + R with b = s / (state[0] + eps),
    state[0] = state[1] = s.  The caller keeps sqrt |s| away from tol by more than the sum's bound, or makes the sum exact."""
    R, P, state = (np.asarray(v, dtype=np.float64) for v in (R, P, state))
    r, p, st = _t(R, P, state)
    _oracle().cg_finish(r, p, st, cg_eps, tol)
    vals = {"P": p.numpy(), "state": st.numpy()}
    zero = np.zeros_like(P)
    if state[2] != 0.0:
        return vals, {"P": zero, "state": np.zeros(4)}
    s, ds = float(R @ R), dot_bound(R, R)
    if vals["state"][2] != 0.0:
        return vals, {"P": zero, "state": np.array([0.0, ds, 0.0, 0.0])}
    den = state[0] + cg_eps
    db = _quotient_bound(s, ds, den, 2.0 * U * abs(den))
    bp = np.abs(P) * db + 3.0 * U * (abs(s / den) * np.abs(P) + np.abs(R))
    return vals, {"P": bp, "state": np.array([ds, ds, 0.0, 0.0])}


def cg_residual_ref(B, AX, AP, state, R):
    """R = B - (AX + a AP), a = state[3] taken as given; three roundings in the statement and two in the kernel, each over no more than the absolute sum of the terms (6 u covers them)."""
    B, AX, AP, state, R = (np.asarray(v, dtype=np.float64) for v in (B, AX, AP, state, R))
    b, ax, ap, st, r = _t(B, AX, AP, state, R)
    _oracle().cg_residual(b, ax, ap, st, r)
    if state[2] != 0.0:
        return {"R": r.numpy()}, {"R": np.zeros_like(R)}
    return {"R": r.numpy()}, {"R": 6.0 * U * (np.abs(B) + np.abs(AX) + abs(state[3]) * np.abs(AP))}


def scores_axpy_ref(state, t, S):
    """S += a t, a = state[3]; nothing once the flag is up (the guard of the step: S receives exactly the steps X received)."""
    state, t, S = (np.asarray(v, dtype=np.float64) for v in (state, t, S))
    if state[2] != 0.0:
        return {"S": S.copy()}, {"S": np.zeros_like(S)}
    return {"S": S + state[3] * t}, {"S": 3.0 * U * (np.abs(S) + abs(state[3]) * np.abs(t))}


def scores_store_ref(S):
    """(float) S: one rounding to nearest, the same on every IEEE machine — bit for bit."""
    return np.asarray(S, dtype=np.float64).astype(np.float32)


def axpby_ref(a, x, b, y):
    """y = a x + b y through the oracle's statement; b == 0 ignores y altogether (NaN / Inf in it included).  Three roundings on
    either side over |a x| + |b y|."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if b == 0.0:
        return {"y": a * x}, {"y": 2.0 * U * np.abs(a * x)}
    xt, yt = _t(x, y)
    _oracle().axpby(a, xt, b, yt)
    return {"y": yt.numpy()}, {"y": 6.0 * U * (np.abs(a * x) + np.abs(b * y))}


def cg_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the fields of a reference (ratio(): 0 / 0 = 0, x / 0 = inf, a non-finite entry = inf)."""
    return max(ratio(got[k], ref[k], bound[k]) for k in ref)


def cg_vectors(M, seed=0):
    """(X, R, P, AP, B) of length M with entries of mixed sign and size, P . AP > 0 (AP = a positive diagonal times P plus noise)."""
    rng = np.random.default_rng(500 + M + seed)
    X, R, P, B = (rng.standard_normal(M) * s for s in (3.0, 0.5, 1.0, 2.0))
    AP = (0.5 + rng.random(M)) * P + 0.05 * rng.standard_normal(M)
    return X, R, P, AP, B
