"""Sample-weighted FALKON: the squared loss with a weight per row, solved by falkon's CG over one stored K_nM block.

The objective over the Nystroem model f = K_nM alpha is (1 / n) sum_i w_i (f_i - y_i)^2 + lam alpha' K_MM alpha with n the
number of rows — falkon's convention: the weights do not change n.  Its normal equations are
(K' W K / n + lam K_MM) alpha = K' W y / n, so the fit is solver.falkon_fit's with W inside both products:
    T = chol(K_MM + eps M I)',  A = chol(T diag(w_M) T' / M + lam I)'       w_M: the weights of the centres, as falkon's
                                                                            weighted preconditioner carries them
    b = A^-T T^-T K' (w o y / n)                                            (out of the K_nM build)
    CG, maxiter steps, on  beta -> A^-T [ T^-T K' (w o (K T^-1 A^-1 beta)) / n + lam A^-1 beta ]
    alpha = T^-1 A^-1 beta
Every product with the block is ONE be.ktk_w (odx/weighted_ops.py: one read of the block where a one-read kernel exists);
the schedule is solver._cg_run's and the preconditioner LogisticOps' (T once, A for any weights at the centres).  This file
sequences them.  No host synchronisation inside the loop."""
import dataclasses
import types

import torch

from .solver import SolverOptions, _cg_run, _cg_state, _check_pivots, _slots, scores_from_cg


def falkon_fit_weighted(be, F, y, w, Zf, w_centres, kernel_arg, lam, maxiter=20, opt=None, scores_out=None, knm_blocks=None,
                        allreduce=None, shard=None):
    """Fit one binary FALKON problem with a weight per row, over one stored shard.

    be          backend (odx.backend.HipBackend in the product)
    F, y, w     Features of the n rows, their labels and their weights, (n,) f64 device vectors.  The weights must be finite
                and >= 0 with a positive sum (the estimator checks this; a weight of 0 removes its row)
    Zf, w_centres
                Features of the M centres and their weights, (M,) f64: what the preconditioner's A factor carries
    kernel_arg  a Gaussian's width or a kernel object (falkon._kernel_arg)
    scores_out  optional (n,) f64 device vector: where solver.scores_from_cg(be, K) holds it is zeroed and receives K alpha,
                summed step by step from the passes' UNWEIGHTED row products; otherwise it is left untouched
    knm_blocks  optional list that receives the K_nM block this fit built
    returns     alpha (M,) f64

    A default fit makes 21 weighted passes: 20 steps and the full residual at iteration 10 (the fold of the full residual
    into a step's pass is not used).  Not offered, each a ValueError: row shards (allreduce, shard), a streamed shard
    (knm_storage "stream"), centres that repeat (a column map) and 16-bit rows at native width."""
    opt = opt or SolverOptions()
    if allreduce is not None or shard is not None:
        raise ValueError("falkon_fit_weighted: row shards (allreduce / shard) are not offered: one shard holds all rows")
    n, M = F.n, Zf.n
    if n < 1 or M < 1:
        raise ValueError("falkon_fit_weighted: needs rows and centres, got n = %d, M = %d" % (n, M))
    if getattr(F, "b16", False) or getattr(Zf, "b16", False):
        raise ValueError("falkon_fit_weighted: 16-bit rows at native width (native16) are not offered; pass f32 rows")
    if getattr(be, "knm_storage", None) == "stream":
        raise ValueError("falkon_fit_weighted: knm_storage='stream' stores no K_nM block (a streamed shard's rows pass in "
                         "chunks: no row weights)")
    if getattr(Zf, "cmap", None) is not None:
        raise ValueError("falkon_fit_weighted: not built for centres that repeat (a column map)")
    if y.numel() != n or w.numel() != n or w_centres.numel() != M:
        raise ValueError("falkon_fit_weighted: y and w must hold %d entries and w_centres %d" % (n, M))
    lam = float(lam)
    st = be.precond_logistic_begin(Zf, kernel_arg, opt.pc_epsilon)
    P = be.precond_logistic_step(st, w_centres, lam)
    K, b0 = be.knm_rhs(F, Zf, kernel_arg, w * y * (1.0 / n))          # the block, and K' (w o y / n) from the same launch
    if getattr(K, "fmt", None) == "stream":
        raise ValueError("falkon_fit_weighted: needs a stored K_nM block (a streamed shard's rows pass in chunks: no row weights)")
    if getattr(K, "cmap", None) is not None:
        raise ValueError("falkon_fit_weighted: not built for a block of distinct columns (a column map)")
    if knm_blocks is not None:
        knm_blocks.append(K)
    acc = scores_out is not None and scores_from_cg(be, K)
    tk = None
    if acc:
        scores_out.zero_()
        tk = torch.empty_like(scores_out)              # K v of the current direction, before the weight
    Mp = (M + 1) // 2 * 2                              # (rows 16-byte aligned for odd M too)
    TT, CC = be.zeros(Mp).view(1, Mp), be.zeros(Mp).view(1, Mp)

    def exchange(k, rows):
        be.ktk_w(K, TT[0, :M], w, out=CC[0, :M], t_out=tk if rows else None)

    alpha = be.zeros(M)
    c = _cg_state(be, P, lam, b0, M, _slots(TT, CC, M), False, alpha, tk, scores_out if acc else None)
    _cg_run(be, [c], exchange, float(n), int(maxiter), dataclasses.replace(opt, check_pivots=False), False)
    if opt.check_pivots:
        # one host read for the status words of T's factorisation and of A's
        _check_pivots(be, types.SimpleNamespace(info=torch.stack([i.reshape(-1)[0] for i in (st.info, P.info)]).max().reshape(1)))
    return alpha
