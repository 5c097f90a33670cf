"""FALKON fit: host-side driver of the preconditioned conjugate gradient (A4).

Restates what ``InCoreFalkon(...).fit(X, y)`` does at the reference's call site
(src/modules/region-classifier/FALKONWrapper_with_centers_selection_incore.py:56-68) with
falkon's upstream defaults for the f32 regime the reference runs in:
    T = chol(K_MM + eps M I)', A = chol(T T'/M + lam I)'          (preconditioner, f64 here)
    b = A^-T T^-T K_nM' (y / n)                                   (K_nM' (y / n) comes out of the K_nM build)
    CG, maxiter steps, on  beta -> A^-T [ T^-T K_nM' (K_nM T^-1 A^-1 beta) / n + lam A^-1 beta ]
    alpha = T^-1 A^-1 beta
Every array op is a libodx kernel reached through the backend; this file only sequences
them and places the (optional) row-shard all-reduce.  No host synchronisation inside the loop:
step sizes, residual norms and the stop flag stay on the device.
"""
import math
from dataclasses import dataclass

import torch


@dataclass
class SolverOptions:
    """falkon's numeric knobs (upstream FalkonOptions defaults for float32 data)."""
    pc_epsilon: float = 1e-5            # jitter eps: K_MM + eps*M*I
    cg_epsilon: float = 1e-7            # added to both CG denominators
    cg_tolerance: float = 1e-7          # stop when sqrt(||r||^2) < cg_tolerance^2
    cg_full_gradient_every: int = 10    # recompute r = b - A x from scratch every k iterations
    check_pivots: bool = True           # one host sync after the fit to report a failed Cholesky


_DEFERRED = None     # while a deferred_pivot_checks() block is open: the (backend, info) pairs still to be looked at


class deferred_pivot_checks:
    """Fits issued inside the block do not synchronise with the host to look at their Cholesky status; every status is
    checked when the block closes.  Lets the host enqueue several independent fits (on several streams) back to back."""

    def __enter__(self):
        global _DEFERRED
        self._prev, self.items = _DEFERRED, []
        _DEFERRED = self.items
        return self

    def __exit__(self, exc_type, exc, tb):
        global _DEFERRED
        _DEFERRED = self._prev
        if exc_type is None and self.items:
            # one host read for all status words of the block (they are 1-element device tensors)
            vals = torch.cat([info.reshape(-1)[:1] for _, info in self.items]).tolist()
            for (be, info), v in zip(self.items, vals):
                if v != 0:
                    be.check_info(info)          # raises with the backend's message
        return False


def _check_pivots(be, P):
    if _DEFERRED is not None and hasattr(be, "check_info") and hasattr(P, "info"):
        _DEFERRED.append((be, P.info))
    else:
        be.check_precond(P)


class _NoPhase:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _can_fold(be, K, M, rows_per_rank):
    """The two-vector pass exists for this block width and pays for itself: a pass reads 4 n M bytes, the second vector's
    four extra triangular products 16 M^2.  Decided from quantities every rank agrees on (M, the job's rows per rank and the
    storage option), never from the local shard length, so that all ranks issue the same collectives.  A streamed shard
    (K recomputed by every pass, 2 n M D flop) always folds."""
    if not (hasattr(be, "ktk2") and be.can_ktk2(K)):
        return False
    return bool(getattr(K, "fmt", None) == "stream" or rows_per_rank >= 8 * M)


def scores_from_cg(be, K):
    """Whether a fit over the stored block K can hand back the scores K alpha of its rows as a by-product of its CG passes.

    alpha = T^-1 A^-1 x and x = sum_i a_i p_i over the steps taken; the vector pass i multiplies K with is
    v_i = T^-1 A^-1 p_i, so K alpha = sum_i a_i (K v_i), and K v_i is phase 1 of the pass (its t_out): no further read of K
    (backend.knm_mv reads the whole block once more for the same sum).  Needs the backend's t_out passes and n-sized score
    kernels, and a block whose entries are the Gaussian's f32-accurate values (gauss "h2" stored as 24-bit fixed point or
    f32: the blocks LockstepClassJob._score reads with knm_mv); streamed shards, bf16 / f8 blocks and other backends do not
    qualify."""
    return bool(hasattr(be, "cg_scores_axpy") and hasattr(be, "cg_scores_store") and getattr(be, "gauss", None) == "h2"
                and getattr(K, "fmt", None) in ("u24", "f32"))


@dataclass
class _CG:
    """One conjugate-gradient state on the rank that holds it: the operator's pieces (preconditioner P, penalty lam), falkon's
    vectors (right-hand side B, iterate X, residual R, direction Pv, W p in AP, W x in AX where the fold is on), the device
    words `state`, and the state's places in its driver's exchange (see _slots)."""
    P: object
    lam: float
    B: torch.Tensor
    X: torch.Tensor
    R: torch.Tensor
    Pv: torch.Tensor
    AP: torch.Tensor
    AX: torch.Tensor            # None without the fold
    state: torch.Tensor         # (4,): ||r||^2 old and new, the stop flag, the step size
    v: tuple                    # scratch: A^-1 s of the first and of the second vector of a sandwich
    io: list                    # io[k - 1][j] = (where T^-1 A^-1 s goes, where the summed K'K of it is read): vector j of k
    alpha: torch.Tensor = None  # receives T^-1 A^-1 X (None: a new vector); set by _cg_run either way
    tk: torch.Tensor = None     # with `scores`: K v of the current direction over this rank's rows (the passes' t_out)
    scores: torch.Tensor = None


class _Rows:
    """The vectors of L states that share ONE preconditioner and penalty (a multi-output fit) as the rows of (L, Mp) matrices,
    with the driver's exchange matrices `send` / `recv` (_slots: state l sends row j L + l and reads it back): what lets
    _cg_run send a triangular product of all L states through one be.trmvn (one read of the factor)."""

    def __init__(self, be, L, Mp, fold, send, recv):
        def mat():
            return be.zeros(L * Mp).view(L, Mp)
        self.B, self.X, self.R, self.Pv, self.AP, self.U, self.alpha = (mat() for _ in range(7))
        self.AX = mat() if fold else None
        self.v = (mat(), mat() if fold else None)
        self.send, self.recv = send, recv
        self.groups = None              # (set by a driver whose states share T but not A: see _cg_run)


def _slots(TT, CC, M, L=1, l=0):
    """The io of state l of L over a driver's send / receive matrices ((L, Mp), or (2 L, Mp) where the fold is on): row l
    carries the only vector of a one-vector exchange and the direction of a two-vector one, row L + l its iterate."""
    return [[(TT[j * L + l, :M], CC[j * L + l, :M]) for j in range(k)] for k in range(1, TT.shape[0] // L + 1)]


def _cg_state(be, P, lam, b0, M, io, fold, alpha=None, tk=None, scores=None):
    """The CG state of (P, lam) at its start: B = A^-T T^-T b0 (b0 = K' (y / n), summed over shards), X = 0, R = Pv = B."""
    X, R, Pv, AP = (be.zeros(M) for _ in range(4))
    c = _CG(P, lam, be.trmv(P, "LAi", be.trmv(P, "LTi", b0)), X, R, Pv, AP, be.zeros(M) if fold else None, be.zeros(4),
            (be.zeros(M), be.zeros(M) if fold else None), io, alpha, tk, scores)
    be.cg_init(c.B, X, R, Pv, c.state)
    return c


def _pass(be, ph, K, T, C, M, t_out=None, s=None):
    """C[j, :M] = K' (K T[j, :M]) for the one or two rows of T from one read of K.  t_out (receives K T[0, :M] over this
    rank's rows) is passed on only when set: backends without score accumulation do not know the keyword.  s (the fold step
    over accumulated scores, see _cg_run): this rank's rows of K T^-1 A^-1 x; then C[1, :M] = K' s and T[1] is not read."""
    kw = {} if t_out is None else {"t_out": t_out}
    if s is not None:
        with ph("ktk2"):                                 # (the fold's one read of K, whichever kernel makes it)
            be.ktk_rows(K, T[0, :M], s, out1=C[0, :M], out2=C[1, :M], **kw)
    elif T.shape[0] == 2:
        with ph("ktk2"):
            be.ktk2(K, T[0, :M], T[1, :M], out1=C[0, :M], out2=C[1, :M], **kw)
    else:
        with ph("ktk"):
            be.ktk(K, v=T[0, :M], out=C[0, :M], **kw)


def _sum(ar, C):
    """C summed over the row shards in place (an `allreduce` that returns another tensor is copied back)."""
    r = ar(C)
    if r is not C:
        C.copy_(r)


def _fold_rows(be, Ks):
    """Whether the fold step of fits that accumulate scores over the blocks Ks takes K' S from those scores (see _cg_run)."""
    return bool(hasattr(be, "ktk_rows") and Ks and all(be.can_ktk_rows(K) for K in Ks))


def _cg_run(be, cgs, exchange, n, maxiter, opt, can_fold, shared=None, fold_rows=False):
    """falkon's preconditioned CG schedule, for the states `cgs` this rank holds (none on a rank that only passes over its
    rows), all advancing in lock step.  Returns with every c.alpha = T^-1 A^-1 x.

    exchange(k, rows) is the driver's way through K'K: called once every state's k (1 or 2) prepared vectors T^-1 A^-1 s lie
    in c.io[k - 1][j][0], it leaves the products, summed over the row shards, in c.io[k - 1][j][1] — by whatever collectives
    and passes the driver uses, issued by every rank alike.  rows: the passes also write the row products K v of each state's
    first vector to its tk.  can_fold is the driver's decision, identical on every rank, to take the periodic full residual
    R = B - W x (falkon: every cg_full_gradient_every-th step) without a pass of its own: W is linear and
    x_new = x_old + a p, so W x_new = W x_old + a W p, and W x_old comes out of the SAME read of K_nM as this step's W p (a
    two-vector exchange).  Same value up to f64 rounding, and still computed from fresh products, so it keeps removing the
    recursive drift the recomputation exists for.  No host synchronisation: step sizes and stop flags stay on the device.

    fold_rows: the driver's statement that every state accumulates scores (the caller's scores_out, or a buffer the driver
    made for the purpose: the route does not depend on whether scores were asked for) and that its exchange takes a third argument,
    exchange(2, rows, True): the fold step's second product from the scores.  A state's scores are S = sum_i a_i (K v_i) over
    the steps its iterate received (cg_scores_axpy and cg_step drop the same steps), so S = K T^-1 A^-1 x_old over this
    rank's rows: the forward product of the fold's second vector is in memory, and K'K T^-1 A^-1 x_old = K' S.  The exchange
    then leaves K' S (summed over the shards) where it would have left the second vector's product; only A^-1 x_old is
    still formed, for the lam A^-1 x term.  S is a sum of products made fresh from K, not a recursively updated quantity, so
    the residual is still rebuilt from fresh products; the value differs from the two-vector form's by f64 rounding of
    sum_i a_i (K v_i) against K (sum_i a_i v_i).  This iteration's cg_scores_axpy runs behind the pass: it reads S_old.

    shared: the _Rows whose matrices the vectors of ALL states are rows of, state l row l — the driver's statement that they
    share one P and lam and that the backend has trmvn: every triangular product of the L states is then one be.trmvn.
    Without it _cg_run issues one be.trmv per state and product.  A _Rows with `groups` ((P, lam, first row, end row) each:
    the members of a lambda path over statistics, _fit_stats_members) states instead that the states of a group share P and
    lam and that ALL states share T: the products with A's factors are then one be.trmvn per group, the one with T's inverse
    one be.trmvn over all rows (the one with its transpose carries the group's lam: one per group)."""
    acc = any(c.scores is not None for c in cgs)
    sh = shared
    if sh is not None:
        P, lam, L = cgs[0].P, cgs[0].lam, len(cgs)
        groups = sh.groups or [(P, lam, 0, L)]

    def Wn(*pairs, rows=False):
        """W for states that share P: every triangular product of the L states from ONE read of its factor."""
        k = len(pairs)
        for j, (s, _) in enumerate(pairs):
            for Pg, _, a, b in groups:
                be.trmvn(Pg, "LAit", getattr(sh, s)[a:b], out=sh.v[j][a:b])                    # A^-1 s
            be.trmvn(P, "LTit", sh.v[j], out=sh.send[j * L:(j + 1) * L])                       # T^-1 A^-1 s
        exchange(k, rows)
        for j, (_, out) in enumerate(pairs):
            for Pg, lg, a, b in groups:
                be.trmvn(Pg, "LTi", sh.recv[j * L + a:j * L + b], alpha=1.0 / n, beta=lg, Z=sh.v[j][a:b], out=sh.U[a:b])    # T^-T cc / n + lam v
                be.trmvn(Pg, "LAi", sh.U[a:b], out=getattr(sh, out)[a:b])                      # A^-T u

    def W1(*pairs, rows=False, srows=False):
        """c.<out> = W c.<s> for every (s, out) of pairs and every state c, W = A^-T [ T^-T K'K (T^-1 A^-1 .) / n + lam A^-1 . ],
        from one exchange.  Vector kind outer, state inner.  srows (fold_rows): the second vector is the iterate, whose
        K T^-1 A^-1 x the exchange reads from the state's scores — no product with T's inverse, nothing to send."""
        k = len(pairs)
        for j, (s, _) in enumerate(pairs):
            for c in cgs:
                be.trmv(c.P, "LAit", getattr(c, s), out=c.v[j])        # A^-1 s
                if not (srows and j == 1):
                    be.trmv(c.P, "LTit", c.v[j], out=c.io[k - 1][j][0])    # T^-1 A^-1 s
        if srows:
            exchange(k, rows, True)
        else:
            exchange(k, rows)                                          # K' K of each, summed over shards
        for j, (_, out) in enumerate(pairs):
            for c in cgs:
                u = be.trmv(c.P, "LTi", c.io[k - 1][j][1], alpha=1.0 / n, beta=c.lam, z=c.v[j])    # T^-T cc / n + lam v
                be.trmv(c.P, "LAi", u, out=getattr(c, out))            # A^-T u

    W = W1 if sh is None else Wn
    fold_rows = bool(fold_rows and sh is None and all(c.scores is not None for c in cgs))
    tol = opt.cg_tolerance ** 2
    for it in range(maxiter):
        full = (it + 1) % opt.cg_full_gradient_every == 0
        fold = can_fold and full and it != maxiter - 1
        if fold and fold_rows:
            W(("Pv", "AP"), ("X", "AX"), rows=acc, srows=True)         # W p and W x_old, the latter from the scores
        elif fold:
            W(("Pv", "AP"), ("X", "AX"), rows=acc)                     # W p and W x_old
        else:
            W(("Pv", "AP"), rows=acc)
        for c in cgs:
            be.cg_step(c.X, c.R, c.Pv, c.AP, c.state, opt.cg_epsilon, full)
        for c in cgs:
            if c.scores is not None:
                # K alpha = sum_i a_i K v_i (scores_from_cg).  Behind the step (state[3] is its size), in front of cg_finish:
                # a flag raised by THIS iteration's cg_finish must not drop the term of the step X has just received; a flag
                # raised earlier drops it as cg_step dropped the step
                be.cg_scores_axpy(c.state, c.tk, c.scores)
        if it == maxiter - 1:
            break    # the residual / direction update of the last step cannot change the returned X
        if fold:
            for c in cgs:
                be.cg_residual(c.B, c.AX, c.AP, c.state, c.R)          # R = B - (W x_old + a W p) = B - W x_new
        elif full:
            W(("X", "AP"))
            for c in cgs:
                c.R.copy_(c.B)
                be.axpby(-1.0, c.AP, 1.0, c.R)                         # R = B - W x
        for c in cgs:
            be.cg_finish(c.R, c.Pv, c.state, opt.cg_epsilon, tol)
    if sh is not None:
        for Pg, _, a, b in groups:
            be.trmvn(Pg, "LAit", sh.X[a:b], out=sh.U[a:b])
        be.trmvn(P, "LTit", sh.U, out=sh.alpha)                                   # T^-1 A^-1 beta
        for l, c in enumerate(cgs):
            c.alpha = sh.alpha[l, :P.M]
    else:
        for c in cgs:
            c.alpha = be.trmv(c.P, "LTit", be.trmv(c.P, "LAit", c.X), out=c.alpha)    # T^-1 A^-1 beta
    if opt.check_pivots:
        for Pc in ([g[0] for g in groups] if sh is not None else [c.P for c in cgs]):      # (a shared preconditioner: one status word)
            _check_pivots(be, Pc)


def falkon_fit(be, F, y, Zf, sigma, lam, maxiter=20, opt=None, n_total=None, allreduce=None, knm_out=None,
               return_knm=False, phase=None, precond=None, shard=None, owner=None, precond_ready=None, knm_blocks=None,
               scores_out=None):
    """Fit one binary FALKON problem.

    be        backend (odx.backend.HipBackend in the product)
    F         Features of this rank's rows (n_local x D)
    y         f64 device vector of labels for those rows (n_local,)
    Zf        Features of the M Nystroem centres (identical on every rank)
    n_total   number of rows over all shards (default: F.n)
    allreduce callable summing an f64 device vector in place over the row shards
              (odx.dist.RowShard.allreduce); None for a single shard
    shard, owner
              owner-computes mode for row shards (odx.dist.RowShard + a rank id): only `owner`
              holds the preconditioner and the CG state.  Per CG step the owner broadcasts the
              (M,) direction T^-1 A^-1 p, every rank runs its K_nM pass, the partials are
              all-reduced, and the owner alone applies the preconditioner and updates the
              iterate; alpha is broadcast at the end.  Ranks other than the owner pass
              precond=None and never build one.  Without `shard` every rank does everything
              (replicated mode) and only `allreduce` is used.
    phase     optional callable name -> context manager bracketing the launches of one kernel
              ("precond", "knm", "ktk" = the one-vector pass, "ktk2" = the two-vector pass); bench.py hangs
              HIP-event timers on it
    precond   an already computed preconditioner for (Zf, sigma, lam) to reuse
    precond_ready
              optional callable invoked once, right before the preconditioner is first applied
              (after the K_nM build and the right-hand-side pass were issued): lets a preconditioner
              that is still being computed on another stream overlap with them
    knm_blocks
              optional list that receives the K_nM block this fit built (the stored shard its passes
              streamed: the caller can score from it)
    scores_out
              optional (n_local,) f64 device vector: where scores_from_cg(be, K) holds and this rank holds the CG state
              (one shard, or replicated row shards: not the owner mode), it is zeroed and receives K alpha for this rank's
              rows, summed step by step from the passes' row products; otherwise it is left untouched (the caller asks
              scores_from_cg about the block it gets through knm_blocks)
    returns   alpha (M,) f64 device vector (on every rank)
    """
    opt = opt or SolverOptions()
    n = float(F.n if n_total is None else n_total)
    M = Zf.n
    if shard is not None and allreduce is None:
        allreduce = shard.allreduce
    ar = allreduce if allreduce is not None else (lambda v: v)
    ph = phase if phase is not None else (lambda name: _NoPhase())
    owned = shard is None or owner is None or shard.rank == owner   # this rank runs the M-sized algebra
    bcast = (lambda v: shard.broadcast(v, src=owner)) if (shard is not None and owner is not None) else (lambda v: v)

    P = precond
    if owned and P is None:
        with ph("precond"):
            P = be.precond(Zf, sigma, lam, opt.pc_epsilon)
    yn = y * (1.0 / n)
    with ph("knm"):
        K, b0 = be.knm_rhs(F, Zf, sigma, yn, out=knm_out)   # K_nM and this shard's K' (y / n), out of the same launch
    if knm_blocks is not None:
        knm_blocks.append(K)
    # scores as a by-product (see scores_from_cg): every rank that accumulates must hold the step sizes
    acc = scores_out is not None and (shard is None or owner is None) and scores_from_cg(be, K)
    tk = None
    if acc:
        scores_out.zero_()
        tk = torch.empty_like(scores_out)              # K v of the current direction, this rank's rows
    # the periodic full residual folded into the step's pass (see _cg_run): where the pass dominates the second vector's
    # four extra triangular products (wide, tall blocks)
    if shard is not None:
        can_fold = _can_fold(be, K, M, int(n) // shard.world)
    else:
        can_fold = allreduce is None and _can_fold(be, K, M, int(n))

    b0 = ar(b0)                                        # K' (y / n), summed over shards
    one_call = (shard is None and allreduce is None and phase is None and hasattr(be, "cg_solve") and not acc
                and not getattr(P, "blocks", ()))           # (the library loops read T's inverse whole: a partial one goes below)
    if one_call and getattr(K, "fmt", "f32") != "f32":
        # compact-format block: the class-batched library loop with a batch of one (odx_falkon_cg_batched_q_f64), where the
        # block's pass configuration has one and the factors are one contiguous block (and the block holds every column of
        # the centre list: the library loop knows no column map)
        one_call = bool(hasattr(be, "cg_batched_supported") and getattr(P, "block_rows", None) is not None
                        and getattr(K, "cmap", None) is None
                        and be.cg_batched_supported([K.n], [K.M], K.fmt))
    if one_call:
        # one shard, nothing to time per kernel family: the schedule of _cg_run as one library call (odx_falkon_cg_f64)
        if precond_ready is not None:
            precond_ready()
            precond_ready = None           # (waited for: the statement-by-statement schedule below must not wait again)
        if K.fmt != "f32":
            b0s = be.zeros((M + 1) // 2 * 2).view(1, -1)
            b0s[0, :M].copy_(b0)
            got = be.cg_solve_batched([K], [P], b0s, [n], lam, maxiter, opt)
            alpha = None if got is None else got[0, :M].clone()
        else:
            alpha = be.cg_solve(K, P, b0, n, lam, maxiter, opt)
    if one_call and alpha is not None:
        if opt.check_pivots:
            _check_pivots(be, P)
        return (alpha, K) if return_knm else alpha

    # the fold step over the summed row products (_cg_run, fold_rows) is this fit's fold wherever the rank could sum them,
    # asked for or not: the sum is then kept in a buffer of the fit's own, so that scores_out changes nothing in alpha
    fold_rows = bool(can_fold and (shard is None or owner is None) and scores_from_cg(be, K) and _fold_rows(be, [K]))
    if fold_rows and not acc:
        acc, scores_out = True, be.zeros(K.n)
        tk = torch.empty_like(scores_out)

    k, Mp = 2 if can_fold else 1, (M + 1) // 2 * 2     # (rows 16-byte aligned for odd M too)
    TT, CC = be.zeros(k * Mp).view(k, Mp), be.zeros(k * Mp).view(k, Mp)

    def exchange(k, rows, srows=False):
        """The owner's vector(s) to every rank, every rank's pass over its rows, the partials summed.  srows: the second
        product is K' of this rank's rows of the scores (every rank holds the state then: nothing to send for it)."""
        bcast(TT if k == 2 and not srows else TT[0, :M])
        _pass(be, ph, K, TT[:k], CC[:k], M, tk if rows else None, scores_out if srows else None)
        _sum(ar, CC if k == 2 else CC[0, :M])

    alpha = be.zeros(M)
    cgs = []
    if owned:
        if precond_ready is not None:
            precond_ready()
        cgs.append(_cg_state(be, P, lam, b0, M, _slots(TT, CC, M), can_fold, alpha, tk, scores_out if acc else None))
    _cg_run(be, cgs, exchange, n, maxiter, opt, can_fold, fold_rows=fold_rows)
    bcast(alpha)
    return (alpha, K) if return_knm else alpha


def falkon_fit_stats(be, G, b, n, P, lam, maxiter=20, opt=None):
    """Fit one binary FALKON problem from its M x M statistics alone: G = K_nM' W K_nM ((M, ld) f64, both triangles),
    b = K_nM' W y ((>= M,) f64) and n = sum w, for the centres and kernel the preconditioner P was built from.

    The CG touches the rows only through K'K v and K'y, so with G in the place of K'K this is falkon_fit's schedule (_cg_run,
    one state) with an exchange that is ONE be.symv over the 1 or 2 prepared vectors: M^2 doubles read per iteration whatever n
    was.  The periodic full residual always folds (it rides in the same read of G).  Scores from the CG are not offered (there
    are no rows).  The result is falkon_fit's alpha on all the rows the statistics hold, up to f64 rounding.  No host
    synchronisation inside the loop.  Returns alpha (M,) f64."""
    opt = opt or SolverOptions()
    n = float(n)
    if not n > 0.0:
        raise ValueError("falkon_fit_stats: the statistics must hold a positive total weight, got n = %r" % (n,))
    M = P.M
    Mp = (M + 1) // 2 * 2                              # (rows 16-byte aligned for odd M too)
    TT, CC = be.zeros(2 * Mp).view(2, Mp), be.zeros(2 * Mp).view(2, Mp)

    def exchange(k, rows):
        be.symv(G, TT[:k], out=CC[:k])

    alpha = be.zeros(M)
    cgs = [_cg_state(be, P, float(lam), b[:M] / n, M, _slots(TT, CC, M), True, alpha)]
    _cg_run(be, cgs, exchange, n, maxiter, opt, True)
    return alpha


def _fit_stats_members(be, G, B, n, Ps, lams, maxiter, opt):
    """The L x T conjugate-gradient states (penalty l of the preconditioners Ps, right-hand side row t of B) over ONE pair of
    statistics in lock step: state l T + t.  falkon_fit_stats' exchange for all of them: one be.symv over the k L T rows in play
    (ceil(k L T / 8) reads of G; k = 2 at a full-residual iteration, which always folds).  Returns the alphas (L, T, M)."""
    n = float(n)
    if not n > 0.0:
        raise ValueError("the statistics must hold a positive total weight, got n = %r" % (n,))
    L, T, M = len(Ps), B.shape[0], Ps[0].M
    S, Mp = L * T, (M + 1) // 2 * 2                      # (rows 16-byte aligned for odd M too)
    TT, CC = be.zeros(2 * S * Mp).view(2 * S, Mp), be.zeros(2 * S * Mp).view(2 * S, Mp)

    def exchange(k, rows):
        be.symv(G, TT[:k * S], out=CC[:k * S])

    sh = _Rows(be, S, Mp, True, TT, CC)
    B0 = be.zeros(T * Mp).view(T, Mp)                    # row t: K' W Y[:, t] / n
    B0[:, :M] = B[:, :M] / n
    shared = None
    if S > 1 and hasattr(be, "trmvn"):
        shared = sh
        sh.groups = [(Ps[l], lams[l], l * T, (l + 1) * T) for l in range(L)]
        U = be.trmvn(Ps[0], "LTi", B0, out=sh.U[:T])     # T^-T b0 is every member's; B = A_l^-T of it
        for P, _, a, b in sh.groups:
            be.trmvn(P, "LAi", U, out=sh.B[a:b])
    else:
        for l in range(L):
            for t in range(T):
                sh.B[l * T + t, :M].copy_(be.trmv(Ps[l], "LAi", be.trmv(Ps[l], "LTi", B0[t, :M])))
    cgs = []
    for s in range(S):
        c = _CG(P=Ps[s // T], lam=lams[s // T], B=sh.B[s, :M], X=sh.X[s, :M], R=sh.R[s, :M], Pv=sh.Pv[s, :M], AP=sh.AP[s, :M],
                AX=sh.AX[s, :M], state=be.zeros(4), v=(sh.v[0][s, :M], sh.v[1][s, :M]), io=_slots(TT, CC, M, S, s),
                alpha=None if shared is not None else sh.alpha[s, :M])
        be.cg_init(c.B, c.X, c.R, c.Pv, c.state)
        cgs.append(c)
    _cg_run(be, cgs, exchange, n, maxiter, opt, True, shared)
    alphas = be.zeros(S * M).view(L, T, M)
    for s, c in enumerate(cgs):
        alphas[s // T, s % T].copy_(c.alpha)
    return alphas


def falkon_fit_stats_multi(be, G, B, n, P, lam, maxiter=20, opt=None):
    """falkon_fit_stats for the T right-hand sides B ((T, >= M) f64, row t = K_nM' W Y[:, t]) of ONE G: T conjugate-gradient
    states that share the preconditioner P, each following falkon_fit_stats' schedule with its own device-side stop flag.  Per
    iteration ceil(k T / 8) reads of G (be.symv; k = 2 at a full-residual iteration, folded as in falkon_fit_stats, else 1) and
    every triangular product of all T states from one read of its factor per 8 (be.trmvn).  No host synchronisation inside the
    loop.  Returns the alphas (T, M) f64, row t for column t."""
    return _fit_stats_members(be, G, B, n, [P], [float(lam)], maxiter, opt or SolverOptions())[0]


def falkon_fit_stats_path(be, G, B, n, Ps, lams, maxiter=20, opt=None):
    """falkon_fit_stats_multi at every penalty of `lams` from the same statistics: Ps is what be.precond_path returns for them
    (the members share T's factors and own A's).  The L T states advance in lock step: per iteration ceil(k L T / 8) reads of G,
    the products with T's inverse for all L T states at once, those with A_l's factors for the T states of member l.  No row is
    touched, and the host does not synchronise inside the loop.  Returns the alphas (L, T, M) f64, in the order of `lams`."""
    lams = [float(x) for x in lams]
    if not lams or len(Ps) != len(lams) or any(not (math.isfinite(x) and x > 0.0) for x in lams):
        raise ValueError("falkon_fit_stats_path: lams must be a non-empty sequence of finite positive penalties, one per member "
                         "of Ps, got %r" % (lams,))
    return _fit_stats_members(be, G, B, n, list(Ps), lams, maxiter, opt or SolverOptions())


def falkon_fit_path(be, F, y, Zf, sigma, lams, maxiter=20, opt=None, n_total=None, allreduce=None, phase=None, knm_out=None,
                    knm_blocks=None):
    """Fit one binary FALKON problem at every penalty of `lams` from ONE K_nM block.

    Nothing before `+ lam I` depends on lambda: the block, its right-hand side, T, T^-1 and T T'/M are made once
    (be.knm_rhs, be.precond_path), and the L conjugate-gradient states — one per lambda, each following falkon_fit's
    schedule exactly, with its own device-side stop flag — share every read of the block: per iteration one be.ktkn over
    the L directions (phase "ktkn"), and one more over the L iterates for the periodic full residual (its plain form
    R = B - W x; the fold of falkon_fit needs two vectors per member).  No host synchronisation inside the loop.

    A streamed shard (K.fmt "stream") recomputes K inside every ktkn, so there a second ktkn is a second build of K: when
    the backend's ktkn_span(K) (vectors one build serves) holds 2 L, the full-residual iteration sends [directions;
    iterates] through ONE ktkn and forms R_l = B_l - (W x_old + a W p) with be.cg_residual, as falkon_fit folds — one
    build of K per CG iteration whatever L <= span / 2.  Stored blocks, and paths with 2 L > span, keep the plain form.

    One shard, or replicated row shards through `allreduce` (in-place sum of an f64 device tensor: the (M,) right-hand
    side once, the (L, Mp) matrix of partial products once per pass; (2 L, Mp) at a folded iteration).  A backend without ktkn / precond_path is served
    by looping ktk / precond.  Other arguments as falkon_fit.  Returns the alphas, (L, M) f64."""
    opt = opt or SolverOptions()
    lams = [float(x) for x in lams]
    if not lams or any(not (math.isfinite(x) and x > 0.0) for x in lams):
        raise ValueError("falkon_fit_path: lams must be a non-empty sequence of finite positive penalties, got %r" % (lams,))
    L = len(lams)
    n = float(F.n if n_total is None else n_total)
    M = Zf.n
    ar = allreduce if allreduce is not None else (lambda v: v)
    ph = phase if phase is not None else (lambda name: _NoPhase())

    with ph("precond"):
        if hasattr(be, "precond_path"):
            Ps = be.precond_path(Zf, sigma, lams, opt.pc_epsilon)
        else:
            Ps = [be.precond(Zf, sigma, lam, opt.pc_epsilon) for lam in lams]
    with ph("knm"):
        K, b0 = be.knm_rhs(F, Zf, sigma, y * (1.0 / n), out=knm_out)
    if knm_blocks is not None:
        knm_blocks.append(K)
    b0 = ar(b0)                                          # K' (y / n), summed over shards

    return _fit_members(be, K, [(P, lam, b0) for P, lam in zip(Ps, lams)], M, n, maxiter, opt, ar, ph)


def falkon_fit_grid(be, F, y, Zf, sigmas, lams, maxiter=20, opt=None, n_total=None, allreduce=None, phase=None, blocks_at_once=4,
                    knm_blocks=None):
    """Fit one binary FALKON problem at every (sigma, lambda) of a grid: alphas (S, L, M) f64, alphas[s] bit for bit what
    falkon_fit_path(be, F, y, Zf, sigmas[s], lams, ...) returns.

    The contraction X Z' behind a K_nM block does not depend on sigma, so the blocks of a group of `blocks_at_once` widths
    come from ONE contraction where the backend has knm_rhs_sigmas (HipBackend: on the split-f16 wide tile core; it loops
    knm_rhs elsewhere, as this function does for a backend without the method).  Per group: one knm_rhs_sigmas (phase
    "knm"); then, width by width, the preconditioners of the lambda path (be.precond_path), the summed right-hand side and
    the L conjugate-gradient states over that width's block, exactly as falkon_fit_path runs them; a block is dropped before
    the next width's fit starts.  The blocks of a group are resident TOGETHER: blocks_at_once * odx_knm_bytes(n, M, fmt) is
    the caller's to budget (1 = one block at a time, no shared contraction).

    lams as falkon_fit_path; sigmas a non-empty sequence of finite positive widths.  Replicated row shards through
    `allreduce` as there.  knm_blocks (a list) receives every block, which keeps them all alive."""
    opt = opt or SolverOptions()
    sigmas, lams = [float(x) for x in sigmas], [float(x) for x in lams]
    if not sigmas or any(not (math.isfinite(x) and x > 0.0) for x in sigmas):
        raise ValueError("falkon_fit_grid: sigmas must be a non-empty sequence of finite positive widths, got %r" % (sigmas,))
    if not lams or any(not (math.isfinite(x) and x > 0.0) for x in lams):
        raise ValueError("falkon_fit_grid: lams must be a non-empty sequence of finite positive penalties, got %r" % (lams,))
    width = int(blocks_at_once)
    if width < 1:
        raise ValueError("falkon_fit_grid: blocks_at_once must be at least 1, got %r" % (blocks_at_once,))
    S, L = len(sigmas), len(lams)
    n = float(F.n if n_total is None else n_total)
    M = Zf.n
    ar = allreduce if allreduce is not None else (lambda v: v)
    ph = phase if phase is not None else (lambda name: _NoPhase())
    w = y * (1.0 / n)
    alphas = be.zeros(S * L * M).view(S, L, M)
    for s0 in range(0, S, width):
        grp = sigmas[s0:s0 + width]
        with ph("knm"):
            if hasattr(be, "knm_rhs_sigmas"):
                built = list(be.knm_rhs_sigmas(F, Zf, grp, w))
            else:
                built = [be.knm_rhs(F, Zf, sigma, w) for sigma in grp]
        for i, sigma in enumerate(grp):
            K, b0 = built[i]
            built[i] = None                                  # this width's block goes with its fit
            with ph("precond"):
                if hasattr(be, "precond_path"):
                    Ps = be.precond_path(Zf, sigma, lams, opt.pc_epsilon)
                else:
                    Ps = [be.precond(Zf, sigma, lam, opt.pc_epsilon) for lam in lams]
            if knm_blocks is not None:
                knm_blocks.append(K)
            b0 = ar(b0)                                      # K' (y / n), summed over shards
            alphas[s0 + i].copy_(_fit_members(be, K, [(P, lam, b0) for P, lam in zip(Ps, lams)], M, n, maxiter, opt, ar, ph))
            del K, b0, Ps
    return alphas


def _fit_members(be, K, members, M, n, maxiter, opt, ar, ph, B0=None, weights=None):
    """The L conjugate-gradient states (P, lam, b0) of `members` over ONE block K in lock step: the driver falkon_fit_path (one
    P per lambda, one b0) and falkon_fit_multi (one P and lambda, one b0 per label column: B0, the (L, Mp) matrix the b0 are
    rows of) share.  Returns the alphas, (L, M) f64.

    weights (with B0; falkon_fit_cv): (Dw, wrow, tk, scores) — the states are fits with ROW WEIGHTS, state l with row wrow[l]
    of Dw (-1: none), so the exchange is one be.ktkn_rows; tk / scores: None, or the (L, >= n) matrices whose rows receive
    each state's row products K v and accumulate its K alpha (scores_from_cg)."""
    L = len(members)
    Mp = (M + 1) // 2 * 2                                # rows of the shared matrices stay 16-byte aligned
    # the fold of the periodic full residual (see falkon_fit_path): streamed shards whose one build serves 2 L vectors
    can_fold = bool(getattr(K, "fmt", None) == "stream" and hasattr(be, "ktkn") and hasattr(be, "ktkn_span")
                    and hasattr(be, "cg_residual") and 2 * L <= be.ktkn_span(K))
    rows = 2 * L if can_fold else L
    TT = be.zeros(rows * Mp).view(rows, Mp)              # row l: T^-1 A_l^-1 s_l, the vector member l sends through K'K
    CC = be.zeros(rows * Mp).view(rows, Mp)              # row l: K'K of it   (rows L .. 2 L - 1: the iterates of a folded step)

    def exchange(k, rows):
        """One ktkn over the k L rows in play, the partials summed."""
        TTr, CCr = TT[:k * L], CC[:k * L]
        if weights is not None:
            # (stored blocks only: no fold, k = 1.  The full-residual exchange asks for no rows, so a state's tk is never
            # overwritten by K x)
            with ph("ktkn_rows"):
                be.ktkn_rows(K, TTr, weights[0], weights[1], out=CCr, t_out=weights[2] if rows else None)
            return
        with ph("ktkn"):
            if hasattr(be, "ktkn"):
                be.ktkn(K, TTr, out=CCr)
            else:
                for l in range(k * L):
                    be.ktk(K, v=TTr[l, :M], out=CCr[l, :M])
        _sum(ar, CCr)

    shared = None
    if B0 is not None:
        # one preconditioner for all members: their vectors are the rows of common matrices (_Rows), and where the backend has
        # trmvn every triangular product of all of them — B = A^-T T^-T b0 here, the rest in _cg_run — is one read of a factor
        P, lam = members[0][0], members[0][1]
        sh = _Rows(be, L, Mp, can_fold, TT, CC)
        if L > 1 and hasattr(be, "trmvn"):
            shared = sh
            be.trmvn(P, "LAi", be.trmvn(P, "LTi", B0, out=sh.U), out=sh.B)
        else:
            for l in range(L):
                sh.B[l, :M].copy_(be.trmv(P, "LAi", be.trmv(P, "LTi", B0[l, :M])))
        cgs = []
        for l in range(L):
            c = _CG(P=P, lam=lam, B=sh.B[l, :M], X=sh.X[l, :M], R=sh.R[l, :M], Pv=sh.Pv[l, :M], AP=sh.AP[l, :M],
                    AX=sh.AX[l, :M] if can_fold else None, state=be.zeros(4),
                    v=(sh.v[0][l, :M], sh.v[1][l, :M] if can_fold else None), io=_slots(TT, CC, M, L, l))
            if weights is not None and weights[3] is not None:
                c.tk, c.scores = weights[2][l, :K.n], weights[3][l, :K.n]
            be.cg_init(c.B, c.X, c.R, c.Pv, c.state)
            cgs.append(c)
    else:
        cgs = [_cg_state(be, P, lam, b0, M, _slots(TT, CC, M, L, l), can_fold) for l, (P, lam, b0) in enumerate(members)]
    _cg_run(be, cgs, exchange, n, maxiter, opt, can_fold, shared)
    alphas = be.zeros(L * M).view(L, M)
    for l, c in enumerate(cgs):
        alphas[l].copy_(c.alpha)
    return alphas


def falkon_fit_multi(be, F, Y, Zf, sigma, lam, maxiter=20, opt=None, n_total=None, allreduce=None, phase=None, knm_out=None,
                     knm_blocks=None):
    """Fit the T columns of a label matrix from ONE K_nM block and ONE preconditioner (one-vs-rest heads on shared rows and
    centres: what T calls of falkon_fit build T times).

    Y is (n_local, T) f64, a column per output (the layout of the upstream estimator's Y); the alphas come back as (T, M)
    f64, row t for column t.  Nothing but the right-hand side and the CG vectors depends on the column: one be.precond, one
    be.knm_rhs (column 0 keeps the build's fused right-hand side, so T = 1 is falkon_fit's statement-by-statement sequence,
    operation for operation), the right-hand sides K' (Y[:, t] / n) of the other columns from one be.ktwn (phase "ktwn"; a
    backend without it loops ktk(K, w=...)), and T conjugate-gradient states that all point at the same preconditioner,
    each following falkon_fit's schedule with its own device-side stop flag: per iteration one be.ktkn over the T
    directions, and every triangular product of all T states from one read of its factor (be.trmvn, where the backend
    has it).  The periodic full residual as in falkon_fit_path: its plain form on stored blocks, folded into the step's
    build where a streamed shard's ktkn_span holds 2 T.  No host synchronisation inside the loop.

    One shard, or replicated row shards through `allreduce` (in-place sum of an f64 device tensor: the (M,) right-hand
    side of column 0, the (T - 1, Mp) matrix of the others, then the matrix of partial products once per pass).  Other
    arguments as falkon_fit."""
    opt = opt or SolverOptions()
    if Y.dim() != 2 or Y.shape[0] != F.n or Y.shape[1] < 1:
        raise ValueError("falkon_fit_multi: Y must be (n_local, T) with the %d rows of F, got %r" % (F.n, tuple(Y.shape)))
    T = Y.shape[1]
    n = float(F.n if n_total is None else n_total)
    M = Zf.n
    Mp = (M + 1) // 2 * 2
    ar = allreduce if allreduce is not None else (lambda v: v)
    ph = phase if phase is not None else (lambda name: _NoPhase())

    with ph("precond"):
        P = be.precond(Zf, sigma, lam, opt.pc_epsilon)
    with ph("knm"):
        K, b0 = be.knm_rhs(F, Zf, sigma, Y[:, 0] * (1.0 / n), out=knm_out)
    if knm_blocks is not None:
        knm_blocks.append(K)
    B0 = be.zeros(T * Mp).view(T, Mp)                    # row t: K' (Y[:, t] / n), summed over shards
    B0[0, :M].copy_(ar(b0))
    if T > 1:
        nl = F.n
        Wn = be.zeros((T - 1) * ((nl + 1) // 2 * 2)).view(T - 1, -1)      # (rows 16-byte aligned for odd n too)
        Wn[:, :nl].copy_(Y[:, 1:].t())
        Wn.mul_(1.0 / n)
        with ph("ktwn"):
            if hasattr(be, "ktwn"):
                be.ktwn(K, Wn, out=B0[1:])
            else:
                for t in range(T - 1):
                    be.ktk(K, w=Wn[t, :nl], out=B0[t + 1, :M])
        _sum(ar, B0[1:])
    return _fit_members(be, K, [(P, float(lam), B0[t, :M]) for t in range(T)], M, n, maxiter, opt, ar, ph, B0=B0)


def cv_folds(n, folds, seed=0):
    """A balanced random assignment of n rows to `folds` folds: an (n,) int64 host tensor with values in [0, folds), fold
    sizes differing by one at most, drawn from a torch.Generator of its own seeded with `seed` (the global RNG is not
    touched)."""
    n, folds = int(n), int(folds)
    if folds < 2 or n < folds:
        raise ValueError("cv_folds: needs 2 <= folds <= n, got folds = %d, n = %d" % (folds, n))
    g = torch.Generator()
    g.manual_seed(int(seed))
    fold_of = torch.empty(n, dtype=torch.int64)
    fold_of[torch.randperm(n, generator=g)] = torch.arange(n, dtype=torch.int64) % folds
    return fold_of


def falkon_fit_cv(be, F, y, Zf, sigma, lams, fold_of, folds, maxiter=20, opt=None, refit=True, phase=None, knm_out=None,
                  knm_blocks=None):
    """A `folds`-fold cross-validation of the penalties `lams` from ONE K_nM block: per penalty the fits on the rows outside
    each fold, the score of every row by the fit that never saw its fold, and (refit) the fit on all rows.

    The preconditioner depends on the centres, sigma and lambda only, never on the rows, and a fit on the rows outside fold
    f is the full fit with the row weights d_f[i] = (n / n_f) [fold_of[i] != f] (n_f rows outside the fold):
    K' diag(d_f) K / n = K_f' K_f / n_f, right-hand side K' (d_f o y) / n.  So the fold fits and the fit on all rows are
    folds + 1 conjugate-gradient states over one block that share one preconditioner — what falkon_fit_multi drives, with
    the row-weighted pass in the exchange: one be.knm_rhs (its fused right-hand side serves the all-rows state), one
    be.precond_path for all penalties, the weight rows once, the fold states' right-hand sides from one be.ktwn, and per
    penalty one lock-step run whose every iteration is one be.ktkn_rows (phase "ktkn_rows") and one be.trmvn per
    triangular product.  Row i is held out of state fold_of[i], and K alpha = sum_i a_i (K v_i) (scores_from_cg): the
    direction exchange hands out the row products, every state accumulates them, and the held-out scores are gathered —
    no scoring pass.  Where scores_from_cg(be, K) does not hold (bf16 blocks) they come from one dense be.mmv over the
    stacked fold alphas.  No host synchronisation inside the loops.

    fold_of: (n,) integer tensor (device or host), values in [0, folds).  One stored shard: no row shards, and a streamed
    shard is refused (ValueError), as are folds < 2, an empty fold, a fold of all rows and bad `lams`.
    Returns (alphas, heldout): alphas (L, folds + refit, M) f64, the last member the fit on all rows when refit;
    heldout (L, n) f64."""
    opt = opt or SolverOptions()
    lams = [float(x) for x in lams]
    if not lams or any(not (math.isfinite(x) and x > 0.0) for x in lams):
        raise ValueError("falkon_fit_cv: lams must be a non-empty sequence of finite positive penalties, got %r" % (lams,))
    folds = int(folds)
    if folds < 2:
        raise ValueError("falkon_fit_cv: needs at least 2 folds, got %d" % folds)
    if not hasattr(be, "ktkn_rows"):
        raise NotImplementedError("falkon_fit_cv: the backend %r has no row-weighted pass (ktkn_rows); there is no slower route"
                                  % getattr(be, "name", be))
    nl = F.n
    fo = torch.as_tensor(fold_of)
    if fo.dim() != 1 or fo.numel() != nl or fo.dtype.is_floating_point or fo.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError("falkon_fit_cv: fold_of must be an integer tensor of the %d rows of F, got %s %r" % (nl, fo.dtype, tuple(fo.shape)))
    fo_host = fo.to(device="cpu", dtype=torch.int64)
    if nl == 0 or int(fo_host.min()) < 0 or int(fo_host.max()) >= folds:
        raise ValueError("falkon_fit_cv: fold_of must hold values in [0, %d)" % folds)
    counts = torch.bincount(fo_host, minlength=folds)
    if bool((counts == nl).any()):
        raise ValueError("falkon_fit_cv: a fold holds all rows (nothing to fit on)")
    if bool((counts == 0).any()):
        raise ValueError("falkon_fit_cv: fold %d has no rows" % int((counts == 0).nonzero()[0]))
    L, S = len(lams), folds + bool(refit)
    n = float(nl)
    M = Zf.n
    Mp, ldn = (M + 1) // 2 * 2, (nl + 1) // 2 * 2      # (rows 16-byte aligned for odd M and n too)
    ph = phase if phase is not None else (lambda name: _NoPhase())

    with ph("knm"):
        K, b0 = be.knm_rhs(F, Zf, sigma, y * (1.0 / n), out=knm_out)
    if getattr(K, "fmt", None) == "stream":
        raise ValueError("falkon_fit_cv: needs a stored K_nM block (a streamed shard's rows pass in chunks: no row weights)")
    if knm_blocks is not None:
        knm_blocks.append(K)
    with ph("precond"):
        Ps = be.precond_path(Zf, sigma, lams, opt.pc_epsilon)
    # the weight rows d_f, and the right-hand sides K' (d_f o y) / n of the fold states
    fo_dev = fo_host.to(be.device)
    scale = be.vec([n / float(nl - int(c)) for c in counts])
    Dw = be.zeros(folds * ldn).view(folds, ldn)
    Dw[:, :nl] = (fo_dev[None, :] != torch.arange(folds, device=fo_dev.device)[:, None]).to(torch.float64) * scale[:, None]
    Wn = be.zeros(folds * ldn).view(folds, ldn)
    Wn[:, :nl] = Dw[:, :nl] * (y * (1.0 / n))[None, :]
    B0 = be.zeros(S * Mp).view(S, Mp)                    # rows 0 .. folds - 1: the fold states; the last: all rows
    with ph("ktwn"):
        be.ktwn(K, Wn, out=B0[:folds])
    if refit:
        B0[folds, :M].copy_(b0)
    wrow = list(range(folds)) + [-1] * (S - folds)
    acc = scores_from_cg(be, K)
    alphas = be.zeros(L * S * M).view(L, S, M)
    heldout = be.zeros(L * nl).view(L, nl)
    for l, (P, lam) in enumerate(zip(Ps, lams)):
        tk = be.zeros(S * ldn).view(S, ldn) if acc else None
        scores = be.zeros(S * ldn).view(S, ldn) if acc else None
        alphas[l].copy_(_fit_members(be, K, [(P, lam, B0[s, :M]) for s in range(S)], M, n, maxiter, opt, lambda v: v, ph, B0=B0,
                                     weights=(Dw, wrow, tk, scores)))
        if acc:
            heldout[l].copy_(scores[:folds, :nl].gather(0, fo_dev[None, :])[0])       # row i from the state that never saw it
    if not acc:
        V = alphas[:, :folds].reshape(L * folds, M).t().contiguous()
        sc = be.mmv(F, Zf, sigma, V)
        for l in range(L):
            heldout[l].copy_(sc[:, l * folds:(l + 1) * folds].gather(1, fo_dev[:, None].to(sc.device))[:, 0])
    return alphas, heldout


def falkon_fit_lockstep(be, F, ys, Zfs, sigma, lam, maxiter=20, opt=None, n_total=None, shard=None, knm_outs=None,
                        phase=None, precond=None, precond_ready=None, owners=None, knm_blocks=None, scores_out=None):
    """Fit up to `world` binary problems at once over row shards, one owner rank per problem.

    Problem b (labels ys[b], centres Zfs[b]) is owned by rank owners[b] (default: rank b): only that rank holds its
    preconditioner and CG state.  (`owners`: B distinct ranks, the same list on every rank — odx.plan rotates them over
    the ranks when a batch is smaller than the world, so that the preconditioner work stays balanced.)  All problems advance through the same CG schedule in lock step, so one iteration costs every rank
        its own problem's triangular products                      (all ranks busy: no owner-only serial section)
        one all-gather of the B directions T^-1 A^-1 p             ((world, M) f64)
        B passes over its row shard of the B stored K_nM           (HBM-bound, the bulk)
        one reduce-scatter handing each owner the sum of its partials
    instead of, per problem, a broadcast, a pass and an all-reduce with the other ranks idle during the owner's
    algebra (falkon_fit's owner mode).  The arithmetic per problem is exactly falkon_fit's.

    ys, Zfs     lists of B <= world label vectors / centre Features (identical on every rank)
    knm_outs    optional list of B preallocated f32 buffers for the K_nM shards
    knm_blocks  optional list that receives the B K_nM shards built here, in problem order
    precond     this rank's problem's preconditioner (when it owns one), or None to build it here
    scores_out  optional list of B (n_local,) f64 device vectors: with ONE rank (which then holds every CG state) and blocks
                for which scores_from_cg holds, vector b is zeroed and receives K_b alpha_b, summed step by step from the
                passes' row products (see falkon_fit).  With more ranks the step sizes live on the owner only and the
                vectors are left untouched: the caller scores from the stored block (backend.knm_mv)
    returns     list of B alpha vectors (M,) f64, on every rank
    """
    from .dist import RowShard
    opt = opt or SolverOptions()
    shard = shard if shard is not None else RowShard()
    world, rank = shard.world, shard.rank
    B = len(Zfs)
    if B > world or len(ys) != B:
        raise ValueError("falkon_fit_lockstep: %d problems for %d ranks" % (B, world))
    n = float(F.n if n_total is None else n_total)
    M = Zfs[0].n
    if any(z.n != M for z in Zfs):
        raise ValueError("falkon_fit_lockstep: every problem needs the same number of centres")
    ph = phase if phase is not None else (lambda name: _NoPhase())
    owners = list(range(B)) if owners is None else [int(o) for o in owners]
    if len(owners) != B or len(set(owners)) != B or any(not 0 <= o < world for o in owners):
        raise ValueError("falkon_fit_lockstep: owners must be %d distinct ranks below %d, got %r" % (B, world, owners))
    owned = rank in owners
    P = precond
    if owned and P is None:
        with ph("precond"):
            P = be.precond(Zfs[owners.index(rank)], sigma, lam, opt.pc_epsilon)
    Mp = (M + 1) // 2 * 2                             # rows of the exchanged matrices stay 16-byte aligned
    # Tall[k - 1] (world, k Mp): the gathered vectors, row r = the k vectors of the problem rank r owns; CC[k - 1]: this
    # rank's partials, row r = its partials of that problem.  k = 2 (the fold): still one all-gather and one reduce-scatter
    Tall, CC = ([be.zeros(world * Mp).view(world, Mp)] for _ in range(2))
    Ks = []
    for b in range(B):
        with ph("knm"):                               # K_nM shard and this shard's K' (y / n) of problem b in one launch
            Ks.append(be.knm_rhs(F, Zfs[b], sigma, ys[b] * (1.0 / n), out=None if knm_outs is None else knm_outs[b],
                                 rhs_out=CC[0][owners[b], :M])[0])
    if knm_blocks is not None:
        knm_blocks.extend(Ks)
    # scores as a by-product of the passes (scores_from_cg): only where this rank holds the step sizes of every problem
    acc = (scores_out is not None and world == 1 and B > 0 and len(scores_out) == B
           and all(scores_from_cg(be, K) for K in Ks))
    tks = None
    if acc:
        for S in scores_out:
            S.zero_()
        tks = [torch.empty_like(S) for S in scores_out]      # K v of problem b's current direction, this rank's rows
    can_fold = B > 0 and _can_fold(be, Ks[0], M, int(n) // world)
    # the fold step over the summed row products, asked for or not (see falkon_fit)
    fold_rows = bool(can_fold and world == 1 and all(scores_from_cg(be, K) for K in Ks) and _fold_rows(be, Ks))
    if fold_rows and not acc:
        acc, scores_out = True, [be.zeros(K.n) for K in Ks]
        tks = [torch.empty_like(S) for S in scores_out]
    if can_fold:
        Tall.append(be.zeros(world * 2 * Mp).view(world, 2 * Mp))
        CC.append(be.zeros(world * 2 * Mp).view(world, 2 * Mp))
    kmax = len(Tall)
    mine, got = be.zeros(kmax * Mp).view(kmax, Mp), be.zeros(kmax * Mp).view(kmax, Mp)    # what this rank sends / is handed

    def exchange(k, rows, srows=False):
        """One all-gather of every owner's vector(s), B passes over this rank's rows, one reduce-scatter of the partials.
        srows (one rank, scores accumulated): problem b's second product is K' of its scores."""
        Ta, Ca = Tall[k - 1], CC[k - 1]
        shard.gather_rows(mine[:k].view(-1), Ta)
        for b in range(B):
            o = owners[b]
            _pass(be, ph, Ks[b], Ta[o].view(k, Mp), Ca[o].view(k, Mp), M, tks[b] if rows else None,
                  scores_out[b] if srows else None)
        shard.reduce_scatter_rows(Ca, got[:k].view(-1))

    shard.reduce_scatter_rows(CC[0], got[0])         # K' (y / n) of every problem: each owner gets the sum of its row
    abuf = be.zeros(Mp)                              # this rank's problem's alpha (zeros on a rank that owns none)
    cgs = []
    if owned:
        if precond_ready is not None:
            precond_ready()
        b = owners.index(rank)
        cgs.append(_cg_state(be, P, lam, got[0, :M], M, _slots(mine, got, M), can_fold, abuf[:M],
                             tks[b] if acc else None, scores_out[b] if acc else None))
    _cg_run(be, cgs, exchange, n, maxiter, opt, can_fold, fold_rows=fold_rows)
    shard.gather_rows(abuf, Tall[0])
    return [Tall[0][owners[b], :M].clone() for b in range(B)]
