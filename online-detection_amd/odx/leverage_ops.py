"""Backend operations of the ridge leverage scores (odx/leverage.py), mixed into ``backend.HipBackend`` beside ``PathOps``:
the f64 matrix of a dictionary (``kmm_f64``: odx_radial_kmm_f64), its inverse Cholesky factor (``chol_inverse``: odx_potrf_f64,
odx_trtri_f64) and the row quadratic form of an f32 K_nM block against that factor (``row_quad``: odx_knm_rowquad_f64).  All
HIP through libodx."""
import torch

from . import hip
from .knm_path import _p


class LeverageOps:
    def _tile_route(self, n, M, D, kernel):
        """The tile core (128 / 256) the Gaussian build of an (n, M) block runs on when that is not what the options pin and
        not the direct-difference build; 0 otherwise (nothing to pin: direct, pinned already, another contraction, a Matern
        kernel — the wide core at every shape)."""
        from . import options as _options
        if self.gauss != "h2" or n <= 0 or M <= 0 or hip.radial_of(kernel)[1] or _options.current().h2_tile:
            return 0
        if self.direct_small(n, M, D):
            return 0
        return int(self.lib.odx_gauss_h2_tile(n, M))

    def knm_f32(self, F, Zf, kernel, route_rows=None, out=None):
        """knm() in f32 format whatever the storage option says, built by the route a block of route_rows rows takes (direct
        differences or a tile core: both are chosen by shape): a chunk of rows gets the entries the whole block has.  out: knm's
        (a preallocated buffer for the block)."""
        from . import options as _options
        saved = self.knm_storage
        self.knm_storage = "f32"
        try:
            tile = self._tile_route(F.n if route_rows is None else int(route_rows), Zf.n, F.D, kernel)
            if tile:
                with _options.override(h2_tile=tile):
                    return self.knm(F, Zf, kernel, out=out)
            return self.knm(F, Zf, kernel, out=out)
        finally:
            self.knm_storage = saved

    def share_split(self, F, Zf, kernel):
        """Before the rows of F are cut into chunks (rows()): give F and Zf their packed f16 split now, where the block is built
        on a tile core, so that every chunk carries the split of all rows (its scale is a maximum over the matrix)."""
        saved = self.knm_storage
        self.knm_storage = "f32"
        try:
            if self.gauss == "h2" and F.n > 0 and Zf.n > 0 and (hip.radial_of(kernel)[1] or not self.direct_small(F.n, Zf.n, F.D)):
                self.pack(F), self.pack(Zf)
        finally:
            self.knm_storage = saved

    def kmm_f64(self, Zf, kernel, diag=None, diag_scale=0.0):
        """The f64 kernel matrix of the centres Zf plus diag_scale * diag on the diagonal (diag None: plus diag_scale), as an
        (M, ld) f64 tensor, ld even: the lower triangle is the matrix, what lies above it is not (the factorisation never
        reads it).  kernel: a width or a kernel object, as the estimators hand it down (falkon._kernel_arg)."""
        Zf = self.f32(Zf)
        M, D = Zf.n, Zf.D
        sigma, kind = hip.radial_of(kernel)
        ld = (M + 1) // 2 * 2
        A = torch.empty((M, ld), dtype=torch.float64, device=self.device)
        if M == 0:
            return A
        ldz = (D + 1) // 2 * 2
        Zd = torch.zeros((M, ldz), dtype=torch.float64, device=self.device)
        zsq = torch.empty(M, dtype=torch.float64, device=self.device)
        hip.check(self.lib.odx_convert_f32_f64(_p(Zf.X), Zf.ld, _p(Zd), ldz, M, D, self._stream()), "odx_convert_f32_f64")
        if diag is not None:
            diag = torch.as_tensor(diag, dtype=torch.float64, device=self.device).contiguous()
            if diag.shape != (M,):
                raise ValueError("kmm_f64: diag must hold one value per centre (%d), got shape %s" % (M, tuple(diag.shape)))
        hip.check(self.lib.odx_radial_kmm_f64(_p(Zd), ldz, M, D, sigma, kind, _p(diag), float(diag_scale), _p(A), ld, _p(zsq),
                                              self._stream()), "odx_radial_kmm_f64")
        return A

    def chol_inverse(self, A):
        """(Li, info): Li = L^-1 (lower, (M, ld) f64) of the Cholesky factor L of the symmetric matrix whose lower triangle A
        (M, ld; ld even) holds; A is left as it was.  A non-positive pivot raises (check_info: one host synchronisation)."""
        M = A.shape[0]
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        if M == 0:
            return A.clone(), info
        if A.dtype != torch.float64 or A.dim() != 2 or A.shape[1] < M or A.stride(1) != 1 or A.stride(0) % 2 or A.data_ptr() % 16:
            raise ValueError("chol_inverse: A must be a 16-byte aligned (M, >= M) f64 matrix with an even row stride")
        ld = A.stride(0)
        L = torch.empty((M, ld), dtype=torch.float64, device=self.device)
        L[:, :A.shape[1]] = A
        ws = self._workspace("lev_potrf", self.lib.odx_potrf_workspace_bytes(M))
        hip.check(self.lib.odx_potrf_f64(_p(L), ld, M, _p(info), _p(ws), ws.numel(), self._stream()), "odx_potrf_f64")
        self.check_info(info)
        out = torch.empty((2, M, ld), dtype=torch.float64, device=self.device)
        ws = self._workspace("lev_trtri", self.lib.odx_trtri_workspace_bytes(M))
        hip.check(self.lib.odx_trtri_f64(_p(L), ld, M, _p(out[0]), _p(out[1]), ld, _p(ws), ws.numel(), self._stream()),
                  "odx_trtri_f64")
        return out[0], info

    def row_quad(self, K, Li, out=None):
        """q (n,) f64, q[r] = |Li k_r|^2 for the rows k_r of the f32-format block K (a Knm, or a row sub-block: Knm.rows) and
        the lower-triangular Li (M, ld) f64.  Bit for bit the same for a row whatever the other rows of the call."""
        fmt = getattr(K, "fmt", "f32")
        if fmt != "f32":
            raise ValueError("row_quad: needs an f32-format K_nM block; this one is %r (leverage scores on compact blocks and "
                             "streamed shards are not offered)" % (fmt,))
        if getattr(K, "cmap", None) is not None:
            raise ValueError("row_quad: not built for a block of distinct columns (a column map)")
        n, M = K.n, K.M
        if Li.dtype != torch.float64 or Li.dim() != 2 or Li.shape[0] < M or Li.shape[1] < M or (M and Li.stride(1) != 1):
            raise ValueError("row_quad: Li must be an f64 matrix of at least %d x %d, rows contiguous" % (M, M))
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
            raise ValueError("row_quad: out must be a contiguous f64 vector of at least %d" % n)
        hip.check(self.lib.odx_knm_rowquad_f64(_p(K.K), K.ld, n, M, _p(Li), Li.stride(0) if M else 0, _p(out), self._stream()),
                  "odx_knm_rowquad_f64")
        return out[:n]
