"""Backend operations of fits that share one K_nM block: a lambda path (solver.falkon_fit_path: L penalties) and a
multi-output fit (solver.falkon_fit_multi: T label columns, which share the preconditioner too).

``PathOps`` is mixed into ``backend.HipBackend``.  It adds the pass over several vectors from one read of the block
(``ktkn``: odx_knm_fwd_bwdn_q for groups of 3 .. 8 vectors, the existing one- and two-vector passes for the rest; where the
one-read pass does not exist — above M = 5084 — groups of up to 8 from TWO reads, ``kvn``: odx_knm_fwdn_q, then
odx_knm_bwdn_q, when ``wide_pass_min`` is set; on a streamed shard odx_gauss_ktk_stream_h2n, up to 16 vectors from one BUILD
of K), the preconditioners of a lambda path
(``precond_path``: odx_falkon_precond_path_f64), the right-hand sides of several label columns from one read of the block
(``ktwn``: odx_knm_bwdn_q) and the triangular products of several vectors from one read of a factor (``trmvn``:
odx_trmvn_f64), all HIP through libodx.
"""
import ctypes

import torch

from . import hip

_CODE = {"u24": hip.KNM_U24, "bf16": hip.KNM_BF16}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _aligned_rows(*ts):
    return all(t.stride(0) % 2 == 0 and t.data_ptr() % 16 == 0 for t in ts)


class PathOps:
    """ktkn / ktkn_width / ktkn_span / kvn / precond_path of HipBackend.  On a streamed shard (KnmStream) ktkn makes ONE build
    of K per group of ktkn_span = 16 vectors; ktkn_width keeps meaning vectors per READ of the block or ring (2 there)."""

    # The smallest group of vectors that ktkn sends through the two-read route (odx_knm_fwdn_q + odx_knm_bwdn_q, up to 8
    # vectors per two reads) on a compact block whose one-read width is 2 or 1; None: never (pairs and singles as before).
    # An attribute, not an option: A/B runs and tests switch it on the backend.  profiles/wide_pass.md has the figures
    # behind the value.
    wide_pass_min = None
    WIDE_PASS_MAX = 8           # vectors per call of odx_knm_fwdn_q / odx_knm_bwdn_q

    def _ktkn_bytes(self, K, nv):
        return self.lib.odx_knm_fwd_bwdn_q_workspace_bytes(max(K.n, 1), K.M, _CODE[K.fmt], nv)

    def ktkn_width(self, K):
        """The largest number of vectors ONE read of K serves: 8 or 4 where the NV-vector pass over a compact block has a
        configuration (the vectors sit in LDS as f64: 8 up to M = 2524, 4 up to M = 5084), else 2 where the two-vector pass
        exists, else 1.  f32 blocks (small, not HBM-bound) and streamed shards are served by ktk / ktk2 only."""
        if K.fmt in _CODE:
            for nv in (8, 4):
                if self._ktkn_bytes(K, nv) >= 0:
                    return nv
        return 2 if self.can_ktk2(K) else 1

    def ktkn_span(self, K):
        """The number of vectors ONE build-or-read of K serves in ktkn.  Stored blocks: ktkn_width(K), a read of the block.
        Streamed shards: 16 (odx_gauss_ktk_stream_h2n builds each chunk of rows once and reads it back, while it is
        resident in the Infinity Cache, once per group of vectors): a path of 8 can fold its full residual into the same build."""
        return hip.STREAM_MAX_VECTORS if K.fmt == "stream" else self.ktkn_width(K)

    def _ktkn_stream(self, K, V, out, l, g):
        """Rows [l, l + g) of V through one build of the streamed shard (odx_gauss_ktk_stream_h2n).  The ring: the caller's
        buffer when it is large enough for this entry (a buffer sized for ktk / ktk2 may not be), else the backend's."""
        F, Zf = K.F, K.Zf
        nbytes = int(self.lib.odx_gauss_ktk_stream_h2n_workspace_bytes(max(K.n, 1), K.M, F.D, g))
        if nbytes < 0:
            raise hip.OdxError("odx_gauss_ktk_stream_h2n: M = %d is outside the supported range (M <= 20440)" % K.M)
        ws = K.ring if K.ring is not None and K.ring.numel() >= nbytes else self._workspace("ktkn_stream", nbytes)
        hip.check(self.lib.odx_gauss_ktk_stream_h2n(_p(F.P), F.P.stride(0), _p(F.meta), _p(F.sq), K.n, _p(Zf.P), Zf.P.stride(0),
                                                    _p(Zf.meta), _p(Zf.sq), K.M, F.D, K.sigma, g, _p(V[l]), V.stride(0), _p(out[l]),
                                                    out.stride(0), _p(ws), ws.numel(), self._stream()), "odx_gauss_ktk_stream_h2n")

    def _ktkn_plan(self, K, L):
        """The calls ktkn makes for L vectors over a stored block, in order: (kind, first vector, count) with kind "nv"
        (odx_knm_fwd_bwdn_q: one read), "wide" (odx_knm_fwdn_q + odx_knm_bwdn_q: two reads), "pair" (ktk2: one read) or
        "single" (one ktk per vector: one read each).  Uses ktkn_width, can_ktk2 and wide_pass_min only."""
        width = self.ktkn_width(K)
        plan, l = [], 0
        wmin = self.wide_pass_min
        if wmin is not None and width <= 2 and K.fmt in _CODE:
            while L - l >= max(int(wmin), 1):
                g = min(self.WIDE_PASS_MAX, L - l)
                plan.append(("wide", l, g))
                l += g
        while l < L:
            g = min(width, L - l)
            plan.append(("nv" if g >= 3 else "pair" if g == 2 and self.can_ktk2(K) else "single", l, g))
            l += g
        return plan

    def ktkn_reads(self, K, L):
        """The number of reads of the block ktkn(K, V) makes for L vectors (on a streamed shard: the number of BUILDS of K;
        a single vector there goes through ktk, one build)."""
        if K.fmt == "stream":
            return -(-L // self.ktkn_span(K))
        return sum({"nv": 1, "wide": 2, "pair": 1, "single": g}[kind] for kind, _, g in self._ktkn_plan(K, L))

    def kvn(self, K, V, out=None):
        """out[l] = K V[l] (the row products, f64) for the L >= 1 rows of V ((L, >= M) f64) over a compact stored block: groups
        of up to 8 rows from ONE read each (odx_knm_fwdn_q, every M <= 20440).  out: (L, >= roundup(n, 2)) f64; cells [n:]
        of a row are not written.  Rows of V and out must be 16-byte aligned.  f32 blocks and streamed shards: ValueError
        (the entry is not built for them)."""
        if K.fmt not in _CODE:
            raise ValueError("kvn: compact stored blocks only (u24 / bf16), got %r" % (K.fmt,))
        L, M, n = V.shape[0], K.M, K.n
        if out is None:
            out = torch.zeros((L, (n + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        for t, cols in ((V, M), (out, n)):
            if t.dim() != 2 or t.shape[0] != L or t.shape[1] < cols or t.dtype != torch.float64 or t.stride(1) != 1:
                raise ValueError("kvn: V must be a (L, >= M) and out a (L, >= n) f64 matrix with contiguous rows")
        if not _aligned_rows(V, out):
            raise ValueError("kvn: rows of V and out must be 16-byte aligned (even leading dimension)")
        for l in range(0, L if n > 0 else 0, self.WIDE_PASS_MAX):
            g = min(self.WIDE_PASS_MAX, L - l)
            if self.lib.odx_knm_fwdn_q_workspace_bytes(max(n, 1), M, _CODE[K.fmt], g) < 0:
                raise hip.OdxError("odx_knm_fwdn_q: M = %d is outside the supported range (M <= 20440)" % M)
            hip.check(self.lib.odx_knm_fwdn_q(_p(K.K), K.ld, _p(K.lo) if K.lo is not None else None, K.ld, _CODE[K.fmt], n, M, g,
                                              _p(V[l]), V.stride(0), _p(out[l]), out.stride(0), None, 0, self._stream()),
                      "odx_knm_fwdn_q")
        return out

    def _ktkn_wide(self, K, V, out, l, g):
        """Rows [l, l + g) of V, g <= 8, from two reads of the block: T = K V (odx_knm_fwdn_q), out = K' T (odx_knm_bwdn_q).
        T has a workspace of its own: "ktk" holds the backward kernel's slabs."""
        n, M = K.n, K.M
        ldt = (max(n, 1) + 1) // 2 * 2
        T = self._workspace("ktkn_t", g * ldt * 8)[:g * ldt * 8].view(torch.float64).view(g, ldt)
        self.kvn(K, V[l:l + g], out=T)
        nbytes = self.lib.odx_knm_bwdn_q_workspace_bytes(max(n, 1), M, _CODE[K.fmt], g)
        if nbytes < 0:
            raise hip.OdxError("odx_knm_bwdn_q: M = %d is outside the supported range (M <= 20440)" % M)
        ws = self._workspace("ktk", nbytes)
        hip.check(self.lib.odx_knm_bwdn_q(_p(K.K), K.ld, _p(K.lo) if K.lo is not None else None, K.ld, _CODE[K.fmt], n, M, g,
                                          _p(T), ldt, _p(out[l]), out.stride(0), _p(ws), ws.numel(), self._stream()),
                  "odx_knm_bwdn_q")

    def ktkn(self, K, V, out=None):
        """out[l] = K' (K V[l]) for the L >= 1 rows of V ((L, ld) f64), with as few reads of K as its width allows: groups of
        ktkn_width(K) rows, a group of 3 .. 8 by odx_knm_fwd_bwdn_q, of 2 by ktk2 (two ktk where the block has no two-vector
        pass), of 1 by ktk.  Where one read serves two vectors at most (M > 5084) and wide_pass_min is set, groups of
        wide_pass_min or more rows go in chunks of up to 8 through TWO reads each (odx_knm_fwdn_q, then odx_knm_bwdn_q);
        what remains below wide_pass_min keeps the pairs and singles.  ktkn_reads(K, L) counts the reads.  A streamed shard:
        groups of ktkn_span(K) = 16 rows, each from ONE build of K (odx_gauss_ktk_stream_h2n; a single row goes through
        ktk).  Columns [0, K.M) of V / out are used; rows must be 16-byte aligned for groups of 3 or more (on a streamed
        shard: of 2 or more)."""
        L, M = V.shape[0], K.M
        if out is None:
            out = torch.zeros((L, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        for t in (V, out):
            if t.dim() != 2 or t.shape[0] != L or t.shape[1] < M or t.dtype != torch.float64 or t.stride(1) != 1:
                raise ValueError("ktkn: V and out must be (L, >= M) f64 matrices with contiguous rows")
        if K.fmt == "stream":
            span = self.ktkn_span(K)
            for l in range(0, L, span):
                g = min(span, L - l)
                if g == 1:
                    self.ktk(K, v=V[l, :M], out=out[l, :M])
                    continue
                if V.stride(0) % 2 or out.stride(0) % 2 or V[l].data_ptr() % 16 or out[l].data_ptr() % 16:
                    raise ValueError("ktkn: rows of V and out must be 16-byte aligned (even leading dimension)")
                self._ktkn_stream(K, V, out, l, g)
            return out
        for kind, l, g in self._ktkn_plan(K, L):
            if kind in ("nv", "wide"):
                if V.stride(0) % 2 or out.stride(0) % 2 or V[l].data_ptr() % 16 or out[l].data_ptr() % 16:
                    raise ValueError("ktkn: rows of V and out must be 16-byte aligned (even leading dimension)")
            if kind == "wide":
                self._ktkn_wide(K, V, out, l, g)
            elif kind == "nv":
                ws = self._workspace("ktk", self._ktkn_bytes(K, g))
                hip.check(self.lib.odx_knm_fwd_bwdn_q(_p(K.K), K.ld, _p(K.lo) if K.lo is not None else None, K.ld, _CODE[K.fmt], K.n, M, g,
                                                      _p(V[l]), V.stride(0), _p(out[l]), out.stride(0), _p(ws), ws.numel(),
                                                      self._stream()), "odx_knm_fwd_bwdn_q")
            elif kind == "pair":
                self.ktk2(K, V[l, :M], V[l + 1, :M], out1=out[l, :M], out2=out[l + 1, :M])
            else:
                for j in range(l, l + g):
                    self.ktk(K, v=V[j, :M], out=out[j, :M])
        return out

    def ktwn(self, K, W, out=None):
        """out[t] = K' W[t] for the T >= 1 rows of W ((T, >= K.n) f64): the right-hand sides of T label columns.  A compact
        stored block: groups of up to 8 rows from ONE read each (odx_knm_bwdn_q, every M the compact passes serve); a group
        of one goes through ktk(K, w=...).  f32 blocks (small, not HBM-bound: ktkn's decision) loop ktk(K, w=...), and so do
        streamed shards — there every row is one recompute of K: a build-once entry for several weight vectors is NOT
        built.  Rows of W and out must be 16-byte aligned for groups of 2 or more."""
        T, M, n = W.shape[0], K.M, K.n
        if out is None:
            out = torch.zeros((T, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        for t, cols in ((W, n), (out, M)):
            if t.dim() != 2 or t.shape[0] != T or t.shape[1] < cols or t.dtype != torch.float64 or t.stride(1) != 1:
                raise ValueError("ktwn: W must be a (T, >= n) and out a (T, >= M) f64 matrix with contiguous rows")
        for l in range(0, T, 8 if K.fmt in _CODE else 1):
            g = min(8, T - l) if K.fmt in _CODE else 1
            if g == 1:
                self.ktk(K, w=W[l, :n], out=out[l, :M])
                continue
            if W.stride(0) % 2 or out.stride(0) % 2 or W[l].data_ptr() % 16 or out[l].data_ptr() % 16:
                raise ValueError("ktwn: rows of W and out must be 16-byte aligned (even leading dimension)")
            nbytes = self.lib.odx_knm_bwdn_q_workspace_bytes(max(n, 1), M, _CODE[K.fmt], g)
            if nbytes < 0:
                raise hip.OdxError("odx_knm_bwdn_q: M = %d is outside the supported range (M <= 20440)" % M)
            ws = self._workspace("ktk", nbytes)
            hip.check(self.lib.odx_knm_bwdn_q(_p(K.K), K.ld, _p(K.lo) if K.lo is not None else None, K.ld, _CODE[K.fmt], n, M, g,
                                              _p(W[l]), W.stride(0), _p(out[l]), out.stride(0), _p(ws), ws.numel(), self._stream()),
                      "odx_knm_bwdn_q")
        return out

    def trmvn(self, P, name, X, alpha=1.0, beta=0.0, Z=None, out=None):
        """out[t] = alpha * P.<name> X[t] + beta * Z[t] over the rows of (T, >= P.M) f64 matrices: groups of up to 8 rows from
        ONE read of the factor each (odx_trmvn_f64); one row goes through trmv.  out may be Z, not X."""
        T, M = X.shape[0], P.M
        if out is None:
            out = torch.zeros((T, P.ld), dtype=torch.float64, device=self.device)
        for t in (X, out) + (() if Z is None else (Z,)):
            if t.dim() != 2 or t.shape[0] != T or t.shape[1] < M or t.dtype != torch.float64 or t.stride(1) != 1:
                raise ValueError("trmvn: X, Z and out must be (T, >= M) f64 matrices with contiguous rows")
        if beta != 0.0 and Z is None:
            raise ValueError("trmvn: beta needs Z")
        for l in range(0, T, 8):
            g = min(8, T - l)
            if g == 1:
                self.trmv(P, name, X[l], alpha=alpha, beta=beta, z=None if Z is None else Z[l], out=out[l])
                continue
            if X.stride(0) % 2 or X[l].data_ptr() % 16:
                raise ValueError("trmvn: rows of X must be 16-byte aligned (even leading dimension)")
            hip.check(self.lib.odx_trmvn_f64(_p(getattr(P, name)), P.ld, M, self._TRI[name], g, _p(X[l]), X.stride(0), float(alpha),
                                             float(beta), None if Z is None else _p(Z[l]), 0 if Z is None else Z.stride(0), _p(out[l]),
                                             out.stride(0), self._stream()), "odx_trmvn_f64")
        return out

    def precond_path(self, Zf, sigma, lams, eps, out=None, ws_key="precond"):
        """One Precond per value of `lams` for the same centres.  The members share LTi / LTit (they do not depend on
        lambda) and own their LAi / LAit; member l equals precond(Zf, sigma, lams[l], eps) bit for bit.  `out`: optional
        (2 + 2 L, M, ld) f64 tensor.  A member's info is its word of one (L,) tensor."""
        from .backend import Precond
        lams = [float(x) for x in lams]
        L, M, D = len(lams), Zf.n, Zf.D
        if not 1 <= L <= self.MAX_CLASS_BATCH:
            raise ValueError("precond_path: 1..%d lambdas per call, got %d" % (self.MAX_CLASS_BATCH, L))
        ld = (M + 1) // 2 * 2
        shape = (2 + 2 * L, M, ld)
        mats = out if out is not None else torch.empty(shape, dtype=torch.float64, device=self.device)
        if mats.dtype != torch.float64 or tuple(mats.shape) != shape or not mats.is_contiguous():
            raise ValueError("precond_path: out must be a contiguous %r f64 tensor" % (shape,))
        info = torch.zeros(L, dtype=torch.int32, device=self.device)
        ws = self._workspace(ws_key, self.lib.odx_falkon_precond_path_workspace_bytes(M, D, L))
        hip.check(self.lib.odx_falkon_precond_path_f64(_p(Zf.X), Zf.ld, M, D, float(sigma), (ctypes.c_double * L)(*lams), L, float(eps),
                                                       _p(mats[0]), _p(mats[1]), _p(mats[2]), ld, _p(info), _p(ws), ws.numel(),
                                                       self._stream()), "odx_falkon_precond_path_f64")
        members = []
        for l in range(L):
            P = Precond()
            P.M, P.ld = M, ld
            P.LTi, P.LTit, P.LAi, P.LAit = mats[0], mats[1], mats[2 + 2 * l], mats[3 + 2 * l]
            P.block_rows = None          # not one (4, M, ld) block: the class-batched library loop does not take it
            P.info = info[l:l + 1]
            members.append(P)
        return members
