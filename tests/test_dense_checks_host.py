"""The checkers of tests/dense_checks.py on the CPU: each accepts scipy's own result and a numpy blocked Cholesky / pairwise-merge
inverse summed in ANOTHER order — on every size tests/test_gpu_dense_chain.py uses, for both problem kinds — and rejects the faults a
subtly wrong chain makes: a rank-512 update skipped, one taken from an earlier panel's values (a stale packed slot), a ragged merge
pair skipped, a zeroed last row block, a transpose of another rounding, one entry off by 1e-10 relative, a non-zero above the
diagonal.  The CG checkers: sums in reversed order pass; rs_new for rs_old, an R updated under full_grad, a P moved behind the stop
flag and a last element left out at M = 1025 do not."""
import functools

import numpy as np
import pytest

from tests import dense_checks as dc

KINDS = ("well", "kernel")


@functools.lru_cache(maxsize=8)
def _case(kind, M):
    """(A, scipy's L, scipy's Li, chol bar, inv bar, precond bar) — the bars as the GPU file computes them."""
    A = dc.problem(kind, M)
    L = dc.ref_chol(A)
    Li = dc.ref_inv(L)
    return A, L, Li, dc.chol_bar(A, L)[0], dc.inv_bar(L, Li)[0], dc.precond_bar(A, Li)[0]


def test_sizes_cover_the_block_structure():
    assert set(dc.BIG_M) <= set(dc.ALL_M) and set(dc.HELPER_M) <= set(dc.ALL_M) and {m for m, _ in dc.PRECOND_CASES} <= set(dc.ALL_M)
    for edge in (dc.NB, dc.NBO, 2 * dc.NBO, 3 * dc.NBO):
        assert edge in dc.ALL_M and edge + 1 in dc.ALL_M
    assert all(dc.SIZES[m] for m in dc.ALL_M)


def test_merge_level_fallback_is_unreachable_below_65536():
    """trtri_from_diag_f64's `2 szr + 2 nbe s^2 > pk_cap`: the four packs of a level hold at most 4 nbe s^2 <= 2 (M + s) s units, and
    s < M, nbe pairs: never more than 2 M roundup(M, 64) — checked for every M and level, not argued."""
    assert dc.merge_fallback_reachable() is None


# every size for both kinds; the three largest once each (the file stays under a minute)
ACCEPT = [(k, m) for m in dc.ALL_M if m not in dc.BIG_M for k in KINDS] + list(zip(("kernel", "well", "kernel"), dc.BIG_M))


@pytest.mark.parametrize("kind,M", ACCEPT)
def test_checkers_accept_scipy_and_another_summation_order(kind, M):
    A, L, Li, cbar, ibar, pbar = _case(kind, M)
    Lb = dc.blocked_chol(A)
    Xb = dc.merge_inv(L)
    figs = {"chol_scipy": dc.chol_eta(A, L) / cbar, "chol_blocked": dc.chol_eta(A, Lb) / cbar,
            "inv_scipy": dc.inv_eta(L, Li) / ibar, "inv_merged": dc.inv_eta(L, Xb) / ibar,
            "precond_scipy": dc.precond_eta(A, Li) / pbar, "precond_merged": dc.precond_eta(A, Xb) / pbar}
    print("dense_checks accept %s M=%d %s" % (kind, M, " ".join("%s=%.3g" % kv for kv in figs.items())))
    assert max(figs.values()) <= 1.0, figs
    assert dc.transposes(Xb, np.ascontiguousarray(Xb.T))
    if M > dc.NBO:                     # blocking really changed the sums
        assert not np.array_equal(L, Lb)


def _last_block(M):
    return (M - 1) // dc.NB * dc.NB


CHOL_FAULTS = {     # fault -> (M, argument of blocked_chol)
    "update_skipped_first": (513, ("skip", 0)), "update_skipped_last": (1537, ("skip", 2)), "update_skipped_mid": (1537, ("skip", 1)),
    "update_from_previous_panel": (1025, ("stale", 1, 0)), "update_from_slot_sharing_panel": (1537, ("stale", 2, 0)),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fault", sorted(CHOL_FAULTS))
def test_chol_checker_rejects_a_wrong_trailing_update(kind, fault):
    M, arg = CHOL_FAULTS[fault]
    A, _, _, cbar, _, pbar = _case(kind, M)
    Lf = dc.blocked_chol(A, fault=arg)
    assert dc.chol_eta(A, Lf) > cbar
    assert dc.precond_eta(A, dc.merge_inv(Lf)) > pbar


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [129, 513, 1537])
def test_inverse_checkers_reject_a_skipped_ragged_merge_pair(kind, M):
    A, L, _, _, ibar, pbar = _case(kind, M)
    Xf = dc.merge_inv(L, fault="skip_last_pair")
    assert dc.inv_eta(L, Xf) > ibar and dc.precond_eta(A, Xf) > pbar


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [129, 640, 1537])
def test_checkers_reject_entry_level_faults(kind, M):
    A, L, Li, cbar, ibar, pbar = _case(kind, M)
    r0 = _last_block(M)
    # a zeroed last row block
    Lz, Xz = L.copy(), Li.copy()
    Lz[r0:], Xz[r0:] = 0.0, 0.0
    assert dc.chol_eta(A, Lz) > cbar and dc.inv_eta(L, Xz) > ibar and dc.precond_eta(A, Xz) > pbar
    # one entry off by 1e-10 relative: the largest of the last row block
    for X, check in ((L, lambda F: dc.chol_eta(A, F) > cbar), (Li, lambda F: dc.inv_eta(L, F) > ibar and dc.precond_eta(A, F) > pbar)):
        i, j = np.unravel_index(np.argmax(np.abs(X[r0:])), X[r0:].shape)
        F = X.copy()
        F[r0 + i, j] *= 1.0 + 1e-10
        assert check(F), (M, r0 + i, j)
    # a non-zero in the strict upper triangle, however small
    if M > 1:
        Lu, Xu = L.copy(), Li.copy()
        Lu[0, M - 1], Xu[M - 2, M - 1] = 1e-300, -1e-300
        assert dc.chol_eta(A, Lu) == np.inf and dc.inv_eta(L, Xu) == np.inf and dc.precond_eta(A, Xu) == np.inf
    # Lit = the transpose of ANOTHER rounding of Li: one entry one ulp off
    Lit = np.ascontiguousarray(Li.T)
    assert dc.transposes(Li, Lit)
    Lit[0, M - 1] = np.nextafter(Lit[0, M - 1], np.inf)
    assert not dc.transposes(Li, Lit)
    Lit = np.ascontiguousarray(Li.T)
    Lit[M - 1, 0] = -0.0 if Lit[M - 1, 0] == 0.0 and not np.signbit(Lit[M - 1, 0]) else np.nextafter(Lit[M - 1, 0], np.inf)
    assert not dc.transposes(Li, Lit)                    # (bitwise: -0.0 is not +0.0)


@pytest.mark.parametrize("M,D", [(129, 36), (513, 36), (1025, 64)])
def test_a_factor_checker_is_held_to_the_chains_own_t(M, D):
    """precond_a_eta on a numpy chain (blocked Choleskys, merged inverses) whose K differs from the reference's by one rounding per entry:
    under the bar scipy sets on S, and the faults of the other checkers are rejected."""
    lam = 1e-4
    K = dc.kmm(dc.centres(M, D), 9.0, 1e-5)
    T = dc.ref_chol(K).T
    pbar = dc.precond_bar(T @ T.T / M + lam * np.eye(M))[0]
    Kp = np.tril(K * (1.0 + dc.U * np.random.default_rng(M).standard_normal((M, M))))
    Lt = dc.blocked_chol(Kp + np.tril(Kp, -1).T)
    LTi = dc.merge_inv(Lt)
    LAi = dc.merge_inv(dc.blocked_chol(Lt.T @ Lt / M + lam * np.eye(M)))
    fig = dc.precond_a_eta(LTi, LAi, lam)
    print("dense_checks accept precond_A M=%d ratio=%.3g" % (M, fig / pbar))
    assert fig <= pbar
    r0 = _last_block(M)
    i, j = np.unravel_index(np.argmax(np.abs(LAi[r0:])), LAi[r0:].shape)
    F = LAi.copy()
    F[r0 + i, j] *= 1.0 + 1e-10
    assert dc.precond_a_eta(LTi, F, lam) > pbar
    F = LAi.copy()
    F[r0:] = 0.0
    assert dc.precond_a_eta(LTi, F, lam) > pbar
    F = LAi.copy()
    F[0, M - 1] = 1e-300
    assert dc.precond_a_eta(LTi, F, lam) == np.inf
    assert dc.precond_a_eta(LTi, dc.merge_inv(dc.blocked_chol(Lt.T @ Lt / M + 1.001 * lam * np.eye(M))), lam) > pbar     # another lambda


def test_padded_lower_poisons_what_must_not_be_read():
    A = dc.spd_well(129)
    P = dc.padded_lower(A, fill=np.nan)
    assert P.shape == (129, 130) and np.all(np.isnan(P[:, 129])) and np.all(np.isnan(P[np.triu_indices(129, 1)]))
    assert np.array_equal(np.tril(P[:, :129]), np.tril(A))
    Z, K = dc.spd_kernel(129)
    assert Z.dtype == np.float32 and abs(np.linalg.norm(Z, axis=1).mean() - 20.0) < 2.0
    assert np.abs(Z[64:128] - Z[:64]).max() < 0.1 and K[0, 0] == 1.0 + 1e-5 * 129 and np.linalg.cond(K) > 1e3


# ---------------------------------------------------------------------------------------------------------------- CG checkers
def _reversed_sum(p, q):
    s = 0.0
    for v in (p * q)[::-1]:
        s += v
    return s


@pytest.mark.parametrize("M", dc.CG_MS)
def test_cg_checkers_accept_reversed_sums(M):
    X, R, P, AP, B = dc.cg_vectors(M)
    eps = 1e-7
    ref, bound = dc.cg_init_ref(B)
    s = _reversed_sum(B, B)
    assert dc.cg_ratio({"X": 0 * B, "R": B, "P": B, "state": np.array([s, s, 0.0, 0.0])}, ref, bound) <= 1.0
    state = np.array([float(R @ R) * 1.3, 0.25, 0.0, 0.5])
    for full in (0, 1):
        ref, bound = dc.cg_step_ref(X, R, P, AP, state, eps, full)
        a = state[0] / (_reversed_sum(P, AP) + eps)
        got = {"X": X + a * P, "R": R if full else R - a * AP, "state": np.array([state[0], state[1], 0.0, a])}
        assert dc.cg_ratio(got, ref, bound) <= 1.0
    ref, bound = dc.cg_finish_ref(R, P, state, eps, 1e-9)
    s = _reversed_sum(R, R)
    got = {"P": s / (state[0] + eps) * P + R, "state": np.array([s, s, 0.0, state[3]])}
    assert dc.cg_ratio(got, ref, bound) <= 1.0
    ref, bound = dc.cg_residual_ref(B, X, AP, state, R)
    assert dc.cg_ratio({"R": B - state[3] * AP - X}, ref, bound) <= 1.0
    ref, bound = dc.scores_axpy_ref(state, P, X)
    assert dc.cg_ratio({"S": state[3] * P + X}, ref, bound) <= 1.0
    ref, bound = dc.axpby_ref(-1.5, P, 0.75, X)
    assert dc.cg_ratio({"y": 0.75 * X - 1.5 * P}, ref, bound) <= 1.0
    ref, bound = dc.axpby_ref(-1.5, P, 0.0, np.full(M, np.nan))
    assert dc.cg_ratio({"y": -1.5 * P}, ref, bound) <= 1.0 and dc.cg_ratio({"y": -1.5 * P + 0.0 * np.full(M, np.nan)}, ref, bound) == np.inf


@pytest.mark.parametrize("M", [2, 1025, 20001])
def test_cg_checkers_reject_wrong_updates(M):
    X, R, P, AP, B = dc.cg_vectors(M)
    eps = 1e-7
    s = float(P @ AP)
    state = np.array([float(R @ R), float(R @ R) * (1.0 + 1e-9), 0.0, 0.5])
    ref, bound = dc.cg_step_ref(X, R, P, AP, state, eps, 0)
    a_new = state[1] / (s + eps)                          # the step taken with rs_new in place of rs_old (1e-9 apart)
    assert dc.cg_ratio({"X": X + a_new * P, "R": R - a_new * AP, "state": np.array([state[0], state[1], 0.0, a_new])}, ref, bound) > 1.0
    ref, bound = dc.cg_step_ref(X, R, P, AP, state, eps, 1)
    a = state[0] / (s + eps)
    good = {"X": X + a * P, "R": R.copy(), "state": np.array([state[0], state[1], 0.0, a])}
    assert dc.cg_ratio(good, ref, bound) <= 1.0
    assert dc.cg_ratio(dict(good, R=R - a * AP), ref, bound) > 1.0                       # R updated although full_grad is set
    up = np.array([state[0], state[1], 1.0, 0.5])         # flag up: nothing may move, not by one ulp
    ref, bound = dc.cg_finish_ref(R, P, up, eps, 1e-9)
    assert dc.cg_ratio({"P": P, "state": up}, ref, bound) == 0.0
    moved = P.copy()
    moved[M - 1] = np.nextafter(moved[M - 1], np.inf)
    assert dc.cg_ratio({"P": moved, "state": up}, ref, bound) == np.inf
    ref, bound = dc.cg_step_ref(X, R, P, AP, up, eps, 0)
    assert dc.cg_ratio({"X": X + 0.5 * P, "R": R, "state": up}, ref, bound) == np.inf
    ref, bound = dc.scores_axpy_ref(up, P, X)
    assert dc.cg_ratio({"S": X + 0.5 * P}, ref, bound) == np.inf
    # finish raises the flag at the right moment: converged leaves P, not converged moves it
    tol = 2.0 * np.sqrt(float(R @ R))
    ref, bound = dc.cg_finish_ref(R, P, state, eps, tol)
    assert ref["state"][2] == 1.0 and np.array_equal(ref["P"], P)
    b = float(R @ R) / (state[0] + eps)
    assert dc.cg_ratio({"P": b * P + R, "state": ref["state"]}, ref, bound) == np.inf   # P updated after the flag rose


def test_cg_checkers_reject_a_last_element_left_out_at_1025():
    M = 1025
    X, R, P, AP, B = dc.cg_vectors(M)
    eps, state = 1e-7, np.array([3.0, 3.0, 0.0, 0.0])
    ref, bound = dc.cg_init_ref(B)
    s = float(B[:-1] @ B[:-1])
    assert dc.cg_ratio({"X": 0 * B, "R": B, "P": B, "state": np.array([s, s, 0.0, 0.0])}, ref, bound) > 1.0
    ref, bound = dc.cg_step_ref(X, R, P, AP, state, eps, 0)
    a_short = state[0] / (float(P[:-1] @ AP[:-1]) + eps)                   # the sum misses element 1024
    assert dc.cg_ratio({"X": X + a_short * P, "R": R - a_short * AP, "state": np.array([3.0, 3.0, 0.0, a_short])}, ref, bound) > 1.0
    a = state[0] / (float(P @ AP) + eps)
    Xs = X + a * P
    Xs[-1] = X[-1]                                                         # the update misses it
    assert dc.cg_ratio({"X": Xs, "R": R - a * AP, "state": np.array([3.0, 3.0, 0.0, a])}, ref, bound) > 1.0
    ref, bound = dc.cg_finish_ref(R, P, state, eps, 1e-9)
    s = float(R[:-1] @ R[:-1])
    assert dc.cg_ratio({"P": s / (3.0 + eps) * P + R, "state": np.array([s, s, 0.0, 0.0])}, ref, bound) > 1.0
    S = np.arange(M, dtype=np.float64) / 3.0
    out = dc.scores_store_ref(S)
    assert out.dtype == np.float32 and np.array_equal(out.astype(np.float64), np.float32(S).astype(np.float64))


def test_finish_reference_compares_strictly():
    """sqrt |s| == tol exactly is NOT converged (the kernel's `<`): R = (3, 4, 0, ...) sums to 25 exactly in any order."""
    M = 1025
    R = np.zeros(M)
    R[0], R[M - 1] = 3.0, 4.0
    P = np.ones(M)
    state = np.array([50.0, 50.0, 0.0, 0.1])
    for tol, flag in ((np.nextafter(5.0, 6.0), 1.0), (5.0, 0.0), (np.nextafter(5.0, 4.0), 0.0)):
        ref, bound = dc.cg_finish_ref(R, P, state, 0.0, tol)
        assert ref["state"][2] == flag and (np.array_equal(ref["P"], P) == (flag == 1.0))
        assert ref["state"][1] == 25.0 and ref["state"][0] == (50.0 if flag else 25.0)
