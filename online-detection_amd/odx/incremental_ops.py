"""Backend operations of the incremental FALKON model (odx/incremental.py), mixed into ``backend.HipBackend`` beside ``PathOps``
and ``LeverageOps``: the M x M statistics of an f32 K_nM block (``knm_gram``: odx_knm_gram_f64; with T right-hand
sides from the same read, ``knm_gram_multi``: odx_knm_gram_rhsn_f64) and the product of up to 8
vectors with them from one read (``symv``: odx_symvn_f64).  All HIP through libodx."""
import torch

from . import hip
from .knm_path import _p


class IncrementalOps:
    def knm_chunk_buffer(self, rows, M):
        """A buffer that holds the f32-format block of up to `rows` rows and M centres (knm_f32's `out`)."""
        return torch.empty(max(16, int(rows) * int(self.lib.odx_knm_ld(M, hip.KNM_F32)) * 4), dtype=torch.uint8, device=self.device)

    def knm_gram(self, K, w=None, y=None, beta=1.0, G=None, b=None):
        """G = beta G + K' diag(w) K and, with y and b, b = beta b + K' (w o y) for the f32-format block K (a Knm, or a row
        sub-block: Knm.rows).  G: (M, ld >= M) f64, symmetric on entry unless beta == 0 (then it is never read); None: a new
        (M, ld) matrix, ld even, and beta = 0.  w, y: (n,) f64 (w None: ones; negative weights are legal).  Returns (G, b); both
        triangles of G hold the same bits."""
        fmt = getattr(K, "fmt", "f32")
        if fmt != "f32":
            raise ValueError("knm_gram: needs an f32-format K_nM block; this one is %r (statistics of compact blocks and "
                             "streamed shards are not offered)" % (fmt,))
        if getattr(K, "cmap", None) is not None:
            raise ValueError("knm_gram: not built for a block of distinct columns (a column map)")
        n, M = K.n, K.M
        if G is None:
            G, beta = torch.empty((M, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device), 0.0
            if y is not None and b is None:
                b = torch.empty(M, dtype=torch.float64, device=self.device)
        elif G.dtype != torch.float64 or G.dim() != 2 or G.shape[0] < M or G.shape[1] < M or (M and G.stride(1) != 1):
            raise ValueError("knm_gram: G must be an f64 matrix of at least %d x %d, rows contiguous" % (M, M))
        if (y is None) != (b is None):
            raise ValueError("knm_gram: y and b are given together or not at all")
        for name, t in (("w", w), ("y", y)):
            if t is not None and (t.dtype != torch.float64 or t.numel() < n or not t.is_contiguous()):
                raise ValueError("knm_gram: %s must be a contiguous f64 vector of at least %d" % (name, n))
        if b is not None and (b.dtype != torch.float64 or b.numel() < M or not b.is_contiguous()):
            raise ValueError("knm_gram: b must be a contiguous f64 vector of at least %d" % M)
        hip.check(self.lib.odx_knm_gram_f64(_p(K.K), K.ld, n, M, _p(w), _p(y), float(beta), _p(G), G.stride(0) if M else 0, _p(b),
                                            self._stream()), "odx_knm_gram_f64")
        return G, b

    def knm_gram_multi(self, K, w=None, Y=None, beta=1.0, G=None, B=None):
        """knm_gram's G, bit for bit, and B[t] = beta B[t] + K' (w o Y[:, t]) for the T columns of Y from the SAME read of the
        block (odx_knm_gram_rhsn_f64).  Y: (n, T) f64, a column per output, rows contiguous and 16-byte aligned with an even
        row stride, 1 <= T <= 1024.  B: (T, >= M) f64, rows contiguous; None (with G None): a new (T, Mp) matrix, Mp = M rounded
        up to even.  G, w, beta as knm_gram takes them.  Returns (G, B)."""
        fmt = getattr(K, "fmt", "f32")
        if fmt != "f32":
            raise ValueError("knm_gram_multi: needs an f32-format K_nM block; this one is %r (statistics of compact blocks and "
                             "streamed shards are not offered)" % (fmt,))
        if getattr(K, "cmap", None) is not None:
            raise ValueError("knm_gram_multi: not built for a block of distinct columns (a column map)")
        n, M = K.n, K.M
        if Y is None or Y.dtype != torch.float64 or Y.dim() != 2 or Y.shape[0] < n or not 1 <= Y.shape[1] <= 1024:
            raise ValueError("knm_gram_multi: Y must be an f64 matrix of at least %d rows and 1 .. 1024 columns" % n)
        T = Y.shape[1]
        if Y.stride(1) != 1 or Y.stride(0) < T or Y.stride(0) % 2 or Y.data_ptr() % 16:
            raise ValueError("knm_gram_multi: the rows of Y must be contiguous and 16-byte aligned (an even row stride)")
        if G is None:
            if B is not None:
                raise ValueError("knm_gram_multi: G and B are given together or not at all")
            G, beta = torch.empty((M, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device), 0.0
            B = torch.empty((T, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        elif G.dtype != torch.float64 or G.dim() != 2 or G.shape[0] < M or G.shape[1] < M or (M and G.stride(1) != 1):
            raise ValueError("knm_gram_multi: G must be an f64 matrix of at least %d x %d, rows contiguous" % (M, M))
        if B is None or B.dtype != torch.float64 or B.dim() != 2 or B.shape[0] != T or B.shape[1] < M or (M and B.stride(1) != 1) \
                or (T > 1 and B.stride(0) < M):
            raise ValueError("knm_gram_multi: B must be a (%d, >= %d) f64 matrix, rows contiguous" % (T, M))
        if w is not None and (w.dtype != torch.float64 or w.numel() < n or not w.is_contiguous()):
            raise ValueError("knm_gram_multi: w must be a contiguous f64 vector of at least %d" % n)
        hip.check(self.lib.odx_knm_gram_rhsn_f64(_p(K.K), K.ld, n, M, _p(w), _p(Y), Y.stride(0), T, float(beta), _p(G),
                                                 G.stride(0) if M else 0, _p(B), B.stride(0) if T > 1 else max(M, B.shape[1]),
                                                 self._stream()), "odx_knm_gram_rhsn_f64")
        return G, B

    def symv(self, G, X, alpha=1.0, out=None):
        """out[q, :M] = alpha * G X[q, :M] for the nv <= 8 rows of X (nv, Mp) from ONE read of the (M, ld) f64 matrix G
        (odx_symvn_f64); more rows go in groups of 8.  G: 16-byte aligned, even row stride; X rows 16-byte aligned; out must not
        overlap X."""
        M = G.shape[0]
        if G.dtype != torch.float64 or G.dim() != 2 or G.shape[1] < M or (M and (G.stride(1) != 1 or G.stride(0) % 2 or G.data_ptr() % 16)):
            raise ValueError("symv: G must be a 16-byte aligned (M, >= M) f64 matrix with an even row stride")
        if X.dtype != torch.float64 or X.dim() != 2 or X.shape[1] < M or (X.numel() and X.stride(1) != 1):
            raise ValueError("symv: X must be an (nv, >= %d) f64 matrix, rows contiguous" % M)
        nv = X.shape[0]
        if out is None:
            out = torch.zeros((nv, X.shape[1]), dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.dim() != 2 or out.shape[0] != nv or out.shape[1] < M or (out.numel() and out.stride(1) != 1):
            raise ValueError("symv: out must be an (%d, >= %d) f64 matrix, rows contiguous" % (nv, M))
        if nv and M and (X.data_ptr() % 16 or (nv > 1 and X.stride(0) % 2)):
            raise ValueError("symv: the rows of X must be 16-byte aligned")
        if nv and M:
            x0, o0 = X.data_ptr(), out.data_ptr()
            x1, o1 = x0 + 8 * ((nv - 1) * X.stride(0) + M), o0 + 8 * ((nv - 1) * out.stride(0) + M)
            if not (x1 <= o0 or o1 <= x0):
                raise ValueError("symv: out must not overlap X")
        for l in range(0, nv, 8):
            g = min(8, nv - l)
            hip.check(self.lib.odx_symvn_f64(_p(G), G.stride(0) if M else 0, M, g, _p(X[l]), X.stride(0) if g > 1 else 0, float(alpha), _p(out[l]),
                                             out.stride(0), self._stream()), "odx_symvn_f64")
        return out
