"""Backend operation of the sample-weighted squared-loss fit (odx/weighted.py), mixed into ``backend.HipBackend`` beside
``LogisticOps``: the row-weighted pass ``ktk_w``, out = K' (d o (K v)) from ONE read of a stored block wherever a one-read
kernel exists — odx_knm_fwd_bwd_rw on f32 blocks, odx_knm_fwd_bwd_q_rw (csrc/knm_pass_q_rw.hip) on compact blocks from
``rw_q_min_columns`` columns on, ``ktk_rw``'s NV route (odx_knm_fwd_bwdn_q_rw) below.  All HIP through libodx."""
import torch

from . import hip
from .knm_path import _compact, _fblock, _no_map, _p, _qblock


class WeightedOps:
    # The fewest columns of a compact block from which ktk_w takes odx_knm_fwd_bwd_q_rw; narrower blocks go through ktk_rw.
    # None: the entry is off and every width goes through ktk_rw (above M = 5084: odx_knm_fwdn_q + odx_knm_bwdn_q, two reads).
    # An attribute, not an option: A/B runs and tests switch it on the backend.  5085 is the first width the NV one-read
    # weighted pass does not reach; it moves down only to widths where the new kernel measured faster than the NV pass
    # (profiles/weighted_falkon.md has the rule and the figures).
    rw_q_min_columns = 5085

    def ktk_w(self, K, v, d, out=None, t_out=None):
        """out = K' (d o (K v)) over a stored block (f64).  v: (M,) f64; d: (n,) f64 row weights, or None (ones).  t_out:
        optional (n,) f64 that receives K v BEFORE the weight; `out` is the same bits with or without it.  An f32-format
        block: odx_knm_fwd_bwd_rw.  A compact block of at least rw_q_min_columns columns: odx_knm_fwd_bwd_q_rw, one read at
        every width up to 20440.  A narrower compact block, and every compact block with rw_q_min_columns = None: ktk_rw.
        A streamed shard and a block with a column map: ValueError."""
        if K.fmt == "stream":
            raise ValueError("ktk_w: needs a stored K_nM block (a streamed shard's rows pass in chunks: no row weights)")
        _no_map("ktk_w", K)
        n, M = K.n, K.M
        for name, t, size in (("v", v, M), ("d", d, n), ("t_out", t_out, n), ("out", out, M)):
            if t is not None and (t.dtype != torch.float64 or t.dim() != 1 or t.numel() != size or not t.is_contiguous()):
                raise ValueError("ktk_w: %s must be a contiguous f64 vector of %d" % (name, size))
        if v is None:
            raise ValueError("ktk_w: needs v")
        if out is None:
            out = torch.empty(M, dtype=torch.float64, device=self.device)
        if not _compact(K):
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd", K)
            self._call("odx_knm_fwd_bwd_rw", *_fblock(K), n, M, _p(v), _p(d), _p(out), _p(t_out), _p(ws), ws.numel())
            return out
        if self.rw_q_min_columns is None or M < self.rw_q_min_columns:
            return self.ktk_rw(K, v, d, out=out, t_out=t_out)
        ws = self._pass_ws("ktk", "odx_knm_fwd_bwd_q", K, hip.KNM_CODE[K.fmt])          # (that entry's slabs: include/odx.h)
        self._call("odx_knm_fwd_bwd_q_rw", *_qblock(K), n, M, _p(v), _p(d), _p(out), _p(t_out), _p(ws), ws.numel())
        return out
