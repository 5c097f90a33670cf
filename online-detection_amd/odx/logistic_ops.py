"""Backend operations of the logistic estimator (odx/logistic.py), mixed into ``backend.HipBackend`` beside ``LeverageOps`` and
``IncrementalOps``: the row-weighted pass of a Newton step's Hessian (``ktk_rw``: odx_knm_fwd_bwd_rw on f32 blocks, ``ktkn_rows``
on compact ones), the loss's row terms (``logistic_rows``: odx_logistic_rows_f64) and the preconditioner whose A factor carries
the loss's second derivatives at the centres (``precond_logistic_begin`` / ``precond_logistic_step``: odx_radial_kmm_f64,
odx_potrf_f64, odx_trtri_f64, odx_gemm_nt_f64).  All HIP through libodx."""
import torch

from . import hip
from .knm_path import _compact, _fblock, _no_map, _p


class LogisticPrecond:
    """What does not change from Newton step to Newton step: L_T = chol_lower(K_MM + eps M I) (`L`, strict upper zero), its
    inverses (`LTi` lower, `LTit` upper), the status word of its factorisation (`info`), and the buffers a step's A factor is
    made in."""
    __slots__ = ("M", "ld", "L", "LTi", "LTit", "info", "B", "C", "A", "fM")


class LogisticOps:
    # Whether ktk_rw sends an f32-format block through odx_knm_fwd_bwd_rw (one read).  False: through ktkn_rows, whose f32
    # route is two ktk calls and two reads.  An attribute, not an option: A/B runs and tests switch it on the backend.
    # profiles/logistic_falkon.md has the figures.
    rw_one_read = True

    def ktk_rw(self, K, v, d, out=None, t_out=None):
        """out = K' (d o (K v)) over a stored block (f64).  v: (M,) f64; d: (n,) f64 row weights, or None (ones).  t_out:
        optional (n,) f64 that receives K v BEFORE the weight; `out` is the same bits with or without it.  An f32-format block:
        ONE read (odx_knm_fwd_bwd_rw).  A compact block: ktkn_rows with one vector — one read up to M = 5084
        (odx_knm_fwd_bwdn_q_rw), two above.  A streamed shard and a block with a column map: ValueError."""
        if K.fmt == "stream":
            raise ValueError("ktk_rw: needs a stored K_nM block (a streamed shard's rows pass in chunks)")
        _no_map("ktk_rw", K)
        n, M = K.n, K.M
        for name, t, size in (("v", v, M), ("d", d, n), ("t_out", t_out, n), ("out", out, M)):
            if t is not None and (t.dtype != torch.float64 or t.dim() != 1 or t.numel() != size or not t.is_contiguous()):
                raise ValueError("ktk_rw: %s must be a contiguous f64 vector of %d" % (name, size))
        if v is None:
            raise ValueError("ktk_rw: needs v")
        if out is None:
            out = torch.empty(M, dtype=torch.float64, device=self.device)
        if _compact(K) or not self.rw_one_read:
            # the vectors as one-row matrices, in place: a 16-byte aligned vector IS such a row (the stride of a single row is
            # never walked), and the solver's vectors all are; any other is staged through a workspace
            def row(key, t, size, load):
                if t is None:
                    return None
                ld = (max(size, 1) + 1) // 2 * 2
                if t.data_ptr() % 16 == 0:
                    return t.as_strided((1, size), (ld, 1))
                r = self._workspace(key, ld * 8)[:ld * 8].view(torch.float64).view(1, ld)
                if load:
                    r[0, :size].copy_(t)
                return r
            O, T = row("ktk_rw_o", out, M, False), row("ktk_rw_t", t_out, n, False)
            self.ktkn_rows(K, row("ktk_rw_v", v, M, True), row("ktk_rw_d", d, n, True), [0 if d is not None else -1], out=O, t_out=T)
            if O.data_ptr() != out.data_ptr():
                out.copy_(O[0, :M])
            if T is not None and T.data_ptr() != t_out.data_ptr():
                t_out.copy_(T[0, :n])
            return out
        ws = self._pass_ws("ktk", "odx_knm_fwd_bwd", K)
        self._call("odx_knm_fwd_bwd_rw", *_fblock(K), n, M, _p(v), _p(d), _p(out), _p(t_out), _p(ws), ws.numel())
        return out

    def logistic_rows(self, t, y, neg_weight, g, w, l=None):
        """The weighted logistic loss's row terms at the scores t for the labels y (+-1), both (n,) f64: g = l', w = l'' and
        l = the loss itself, into whichever of the three (n,) f64 vectors is not None (odx_logistic_rows_f64)."""
        n = t.numel()
        for name, x in (("t", t), ("y", y), ("g", g), ("w", w), ("l", l)):
            if x is not None and (x.dtype != torch.float64 or x.numel() != n or not x.is_contiguous()):
                raise ValueError("logistic_rows: %s must be a contiguous f64 vector of %d" % (name, n))
        if y is None:
            raise ValueError("logistic_rows: needs y")
        self._call("odx_logistic_rows_f64", _p(t), _p(y), n, float(neg_weight), _p(g), _p(w), _p(l))

    def precond_logistic_begin(self, Zf, kernel, eps):
        """The part of the logistic preconditioner no Newton step changes (a LogisticPrecond): L_T = chol_lower(K_MM + eps M I)
        of the centres' f64 kernel matrix and its inverses, all f64 (kmm_f64, odx_potrf_f64, odx_trtri_f64: the chain of the
        leverage scores; the split-f16 chain is not used).  kernel: a width or a kernel object (falkon._kernel_arg)."""
        Zf = self.f32(Zf)
        M = Zf.n
        if M < 1:
            raise ValueError("precond_logistic_begin: no centres")
        st = LogisticPrecond()
        st.M, st.ld = M, (M + 1) // 2 * 2
        st.L = self.kmm_f64(Zf, kernel, diag_scale=float(eps) * M)
        st.info = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = self._workspace("lev_potrf", self.lib.odx_potrf_workspace_bytes(M))
        self._call("odx_potrf_f64", _p(st.L), st.ld, M, _p(st.info), _p(ws), ws.numel())
        inv = torch.empty((2, M, st.ld), dtype=torch.float64, device=self.device)
        ws = self._workspace("lev_trtri", self.lib.odx_trtri_workspace_bytes(M))
        self._call("odx_trtri_f64", _p(st.L), st.ld, M, _p(inv[0]), _p(inv[1]), st.ld, _p(ws), ws.numel())
        st.LTi, st.LTit = inv[0], inv[1]
        st.B = torch.zeros((M, st.ld), dtype=torch.float64, device=self.device)
        st.C = torch.empty((M, st.ld), dtype=torch.float64, device=self.device)
        st.A = torch.empty((2, M, st.ld), dtype=torch.float64, device=self.device)
        st.fM = torch.empty(M, dtype=torch.float64, device=self.device)
        return st

    def logistic_centre_scores(self, st, beta):
        """L_T beta (M,) f64: the model's scores at the centres, K_MM alpha up to eps M alpha, for the iterate beta = T alpha
        (odx_trmv_f64; into a buffer of `st`, valid until the next call)."""
        self._call("odx_trmv_f64", _p(st.L), st.ld, st.M, 0, _p(beta), 1.0, 0.0, _p(None), _p(st.fM))
        return st.fM

    def precond_logistic_step(self, st, w_M, lam):
        """The preconditioner of one Newton step (a backend.Precond): T's inverses as they are, and the inverses of
        A = chol_upper(T diag(w_M) T' / M + lam I) for the loss's second derivatives w_M (M,) f64 at the centres.
        T diag(w_M) T' = B B' with B = T diag(sqrt(w_M)), upper triangular: one odx_gemm_nt_f64 over the lower triangle, the
        penalty on the diagonal, odx_potrf_f64, odx_trtri_f64.  The factors live in buffers of `st`: a step's Precond is
        valid until the next call.  Its info is a status word of its own (the factorisation of A)."""
        from .backend import Precond
        M, ld = st.M, st.ld
        if w_M.dtype != torch.float64 or w_M.numel() != M:
            raise ValueError("precond_logistic_step: w_M must hold one f64 weight per centre (%d)" % M)
        torch.mul(st.L[:, :M].t(), torch.sqrt(w_M)[None, :], out=st.B[:, :M])        # (L_T * sqrt(w_M)[:, None]).t()
        flags = hip.GEMM_LOWER_ONLY | hip.GEMM_A_UPPER | hip.GEMM_B_UPPER
        self._call("odx_gemm_nt_f64", _p(st.B), ld, _p(st.B), ld, _p(st.C), ld, M, M, M, 1.0 / M, 0.0, flags)
        st.C.diagonal().add_(float(lam))
        P = Precond()
        P.M, P.ld = M, ld
        P.info = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = self._workspace("lev_potrf", self.lib.odx_potrf_workspace_bytes(M))
        self._call("odx_potrf_f64", _p(st.C), ld, M, _p(P.info), _p(ws), ws.numel())
        ws = self._workspace("lev_trtri", self.lib.odx_trtri_workspace_bytes(M))
        self._call("odx_trtri_f64", _p(st.C), ld, M, _p(st.A[0]), _p(st.A[1]), ld, _p(ws), ws.numel())
        P.LTi, P.LTit, P.LAi, P.LAit = st.LTi, st.LTit, st.A[0], st.A[1]
        P.block_rows = None          # not one (4, M, ld) block: the class-batched library loop does not take it
        return P
