"""Backend operations over one K_nM block: the passes of the CG (``ktk``, ``ktk2``), the scoring pass (``knm_mv``) and what fits
that share one block are driven by: a lambda path (solver.falkon_fit_path: L penalties) and a multi-output fit
(solver.falkon_fit_multi: T label columns, which share the preconditioner too).

``PathOps`` is mixed into ``backend.HipBackend``.  It holds every wrapper of a pass over a stored block or a streamed shard,
all HIP through libodx: one vector (``ktk``: odx_knm_fwd_bwd[_q]_t, odx_gauss_ktk_stream_h2), two (``ktk2``:
odx_knm_fwd_bwd2[_q]_t), one vector and an n-long row vector (``ktk_rows``: odx_knm_fwd_bwd_q_rows[_cols]_t, the CG's fold step
over accumulated scores), several from one read of the block (``ktkn``: odx_knm_fwd_bwdn_q for groups of 3 .. 8 vectors, ktk2 and
ktk for the rest; where the one-read pass does not exist — above M = 5084 — groups of up to 8 from TWO reads, ``kvn``:
odx_knm_fwdn_q, then odx_knm_bwdn_q, when ``wide_pass_min`` is set; on a streamed shard odx_gauss_ktk_stream_h2n, up to 16
vectors from one BUILD of K), the right-hand sides of several label columns from one read of the block (``ktwn``:
odx_knm_bwdn_q) and the scores K alpha (``knm_mv``: odx_knm_mv); beside them the preconditioners of a lambda path
(``precond_path``: odx_falkon_precond_path_f64) and the triangular products of several vectors from one read of a factor
(``trmvn``: odx_trmvn_f64).  A compact block that carries a column map (``Knm.cmap``: the distinct columns of a centre list with
repeats, odx/cols.py) goes through ``ktk`` / ``ktk2`` / ``knm_mv`` with vectors of the list's length (odx_knm_fwd_bwd[2]_q_cols_t,
odx_cols_fold_f64); the several-vector wrappers refuse it.

What every wrapper repeats is stated once, in the helpers below: the arguments a block is passed as (``_qblock``,
``_fblock``), the workspace of an entry (``_pass_bytes``, ``_pass_ws``), the checks of a matrix of row vectors
(``_check_matrix``, ``_check_aligned``), the groups of rows (``_groups``) and the call itself (``_call``).
"""
import ctypes

import torch

from . import hip


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _compact(K):
    """Whether K is a stored block in a compact format (u24 / bf16): what the _q entries take."""
    return K.fmt in hip.KNM_CODE and K.fmt != "f32"


def _qblock(K):
    """The five arguments a compact-format entry (and odx_knm_mv, for every stored format) takes a block as."""
    return _p(K.K), K.ld, _p(K.lo), K.ld, hip.KNM_CODE[K.fmt]


def _mapped(K):
    """The ColumnMap of a block of distinct columns (backend.Knm.cmap), or None."""
    return getattr(K, "cmap", None)


def _vlen(K):
    """The length of the vectors a pass over K takes and returns: the centre list's, K.M without a column map."""
    return K.Mv if _mapped(K) is not None else K.M


def _cols(K, device):
    """The four trailing arguments of a _cols entry: Mv, col_of, start, pos."""
    _, col_of, start, pos = K.cmap.on(device)
    return K.Mv, _p(col_of), _p(start), _p(pos)


def _no_map(who, K):
    if _mapped(K) is not None:
        raise ValueError("%s: not built for a block of distinct columns (a column map): ktk, ktk2 and knm_mv serve it" % who)


def _fblock(K):
    """The two arguments an f32 entry takes a block as."""
    return _p(K.K), K.ld


def _groups(L, width):
    """(first, count) of the groups of up to `width` consecutive rows of L."""
    for l in range(0, L, width):
        yield l, min(width, L - l)


def _check_matrix(who, name, t, rows, cols):
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] < cols or t.dtype != torch.float64 or t.stride(1) != 1:
        raise ValueError("%s: %s must be a (%d, >= %d) f64 matrix with contiguous rows" % (who, name, rows, cols))


def _check_aligned(who, **ts):
    """Every row of the matrices starts on 16 bytes (an aligned first row and an even leading dimension)."""
    if not all(t.stride(0) % 2 == 0 and t.data_ptr() % 16 == 0 for t in ts.values()):
        raise ValueError("%s: rows of %s must be 16-byte aligned (even leading dimension)" % (who, " and ".join(ts)))


class PathOps:
    """The passes over a K_nM block of HipBackend (ktk / ktk2 / ktkn / kvn / ktwn / knm_mv), trmvn and precond_path.  On a
    streamed shard (KnmStream) ktkn makes ONE build of K per group of ktkn_span = 16 vectors; ktkn_width keeps meaning vectors
    per READ of the block or ring (2 there)."""

    # The smallest group of vectors that ktkn sends through the two-read route (odx_knm_fwdn_q + odx_knm_bwdn_q, up to 8
    # vectors per two reads) on a compact block whose one-read width is 2 or 1; None: never (pairs and singles as before).
    # An attribute, not an option: A/B runs and tests switch it on the backend.  profiles/wide_pass.md has the figures
    # behind the value.
    wide_pass_min = None
    WIDE_PASS_MAX = 8           # vectors per call of odx_knm_fwdn_q / odx_knm_bwdn_q

    # ------------------------------------------------------------------ plumbing
    def _call(self, entry, *args):
        hip.check(getattr(self.lib, entry)(*args, self._stream()), entry)

    def _pass_bytes(self, entry, n, M, *more):
        """What <entry>_workspace_bytes(n, M, *more) says; OdxError where the entry has no kernel for M."""
        nbytes = int(getattr(self.lib, entry + "_workspace_bytes")(n, M, *more))
        if nbytes < 0:
            raise hip.OdxError("%s: M = %d is outside the supported range" % (entry, M))
        return nbytes

    def _pass_ws(self, key, entry, K, *more):
        """The workspace `key`, large enough for `entry` over the block K."""
        return self._workspace(key, self._pass_bytes(entry, max(K.n, 1), K.M, *more))

    def _stream_bytes(self, n, M, D):
        return self._pass_bytes("odx_gauss_ktk_stream_h2", n, M, D)

    # ------------------------------------------------------------------ one and two vectors
    def _ktk_stream(self, K, v, v2, w, out, out2):
        """out = K' (K v + w) [, out2 = K' (K v2)] with K recomputed chunk by chunk (odx_gauss_ktk_stream_h2)."""
        F, Zf = K.F, K.Zf
        nbytes = self._stream_bytes(max(K.n, 1), K.M, F.D)
        ws = K.ring if K.ring is not None else self._workspace("ktk_stream", nbytes)
        self._call("odx_gauss_ktk_stream_h2", _p(F.P), F.P.stride(0), _p(F.meta), _p(F.sq), K.n, _p(Zf.P), Zf.P.stride(0), _p(Zf.meta),
                   _p(Zf.sq), K.M, F.D, K.sigma, _p(v), _p(v2), _p(w), _p(out), _p(out2), _p(ws), ws.numel())

    def _check_t_out(self, K, v, t_out):
        if K.fmt == "stream":
            raise ValueError("ktk: t_out needs a stored K_nM block (a streamed shard's rows pass in chunks)")
        if v is None:
            raise ValueError("ktk: t_out is the row product K v: it needs v")
        if t_out.dtype != torch.float64 or t_out.numel() != K.n or not t_out.is_contiguous():
            raise ValueError("ktk: t_out must be a contiguous f64 vector of the block's %d rows" % K.n)

    def ktk(self, K, v=None, w=None, out=None, t_out=None):
        """out = K' (K v + w) over this shard (f64).  t_out: optional (n,) f64 that receives the row products K v (before w
        is added), a by-product of the same read of K (odx_knm_fwd_bwd[_q]_t); `out` is bitwise the same with or without it."""
        if out is None:
            out = torch.empty(_vlen(K), dtype=torch.float64, device=self.device)
        if t_out is not None:
            self._check_t_out(K, v, t_out)
        if K.fmt == "stream":
            self._ktk_stream(K, v, None, w, out, None)
            return out
        # (the _t entries with a null t_out ARE the plain entries: one function in C)
        if _compact(K) and _mapped(K) is not None:
            # distinct columns: v and out have the centre list's length, the block and its workspace K.M columns
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd_q", K, hip.KNM_CODE[K.fmt])
            self._call("odx_knm_fwd_bwd_q_cols_t", *_qblock(K), K.n, K.M, _p(v), _p(w), _p(out), _p(t_out), _p(ws), ws.numel(),
                       *_cols(K, self.device))
        elif _compact(K):
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd_q", K, hip.KNM_CODE[K.fmt])
            self._call("odx_knm_fwd_bwd_q_t", *_qblock(K), K.n, K.M, _p(v), _p(w), _p(out), _p(t_out), _p(ws), ws.numel())
        else:
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd", K)
            self._call("odx_knm_fwd_bwd_t", *_fblock(K), K.n, K.M, _p(v), _p(w), _p(out), _p(t_out), _p(ws), ws.numel())
        return out

    def _ktk2_bytes(self, K):
        if _compact(K):
            return self.lib.odx_knm_fwd_bwd2_q_workspace_bytes(max(K.n, 1), K.M, hip.KNM_CODE[K.fmt])
        return self.lib.odx_knm_fwd_bwd2_workspace_bytes(max(K.n, 1), K.M)

    def can_ktk2(self, K):
        """Whether the two-vector pass exists at this block's width (both vectors must fit in LDS: M <= 10 000).  A streamed
        shard always has one: each chunk is built once and read for both vectors while it is resident.  A block of distinct
        columns answers as the full block of its centre list would (every class of a job then decides alike)."""
        if _mapped(K) is not None and self.lib.odx_knm_fwd_bwd2_q_workspace_bytes(max(K.n, 1), K.Mv, hip.KNM_CODE[K.fmt]) < 0:
            return False
        return K.fmt == "stream" or self._ktk2_bytes(K) >= 0

    def ktk2(self, K, v1, v2, out1=None, out2=None, t_out=None):
        """out1 = K' (K v1), out2 = K' (K v2) over this shard from ONE read of K (odx_knm_fwd_bwd2[_q]).  t_out: optional
        (n,) f64 that receives the row products K v1 (odx_knm_fwd_bwd2[_q]_t)."""
        if t_out is not None:
            self._check_t_out(K, v1, t_out)
        if out1 is None:
            out1 = torch.empty(_vlen(K), dtype=torch.float64, device=self.device)
        if out2 is None:
            out2 = torch.empty(_vlen(K), dtype=torch.float64, device=self.device)
        if K.fmt == "stream":
            self._ktk_stream(K, v1, v2, None, out1, out2)
            return out1, out2
        vecs = (_p(v1), _p(v2), _p(out1), _p(out2), _p(t_out))
        if _compact(K) and _mapped(K) is not None:
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd2_q", K, hip.KNM_CODE[K.fmt])
            self._call("odx_knm_fwd_bwd2_q_cols_t", *_qblock(K), K.n, K.M, *vecs, _p(ws), ws.numel(), *_cols(K, self.device))
        elif _compact(K):
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd2_q", K, hip.KNM_CODE[K.fmt])
            self._call("odx_knm_fwd_bwd2_q_t", *_qblock(K), K.n, K.M, *vecs, _p(ws), ws.numel())
        else:
            ws = self._pass_ws("ktk", "odx_knm_fwd_bwd2", K)
            self._call("odx_knm_fwd_bwd2_t", *_fblock(K), K.n, K.M, *vecs, _p(ws), ws.numel())
        return out1, out2

    # Whether the CG's fold step takes K' S from the accumulated row products (ktk_rows) where it can.  An attribute, not an
    # option: A/B runs and tests switch it on the backend.  profiles/fold_rows.md has the figures.
    fold_rows = True

    def can_ktk_rows(self, K):
        """Whether ktk_rows serves this block: a compact stored block at the widths of the two-vector pass (a block of distinct
        columns answers as the full block of its centre list would, as can_ktk2 does), and the route is on (fold_rows)."""
        return bool(self.fold_rows and K.fmt != "stream" and _compact(K) and self.can_ktk2(K))

    def ktk_rows(self, K, v, s, out1=None, out2=None, t_out=None):
        """out1 = K' (K v), out2 = K' s over this shard from ONE read of K, s an (n,) f64 vector of row values the caller holds
        (odx_knm_fwd_bwd_q_rows[_cols]_t): the fold step of the CG with s = the accumulated row products K T^-1 A^-1 x.  s is
        not added into K v.  t_out: optional (n,) f64 that receives K v."""
        if not _compact(K):
            raise ValueError("ktk_rows: compact stored blocks only (u24 / bf16), got %r" % (K.fmt,))
        if s is None or s.dtype != torch.float64 or s.numel() != K.n or not s.is_contiguous():
            raise ValueError("ktk_rows: s must be a contiguous f64 vector of the block's %d rows" % K.n)
        if t_out is not None:
            self._check_t_out(K, v, t_out)
        if out1 is None:
            out1 = torch.empty(_vlen(K), dtype=torch.float64, device=self.device)
        if out2 is None:
            out2 = torch.empty(_vlen(K), dtype=torch.float64, device=self.device)
        # (a slab pair per half of a workgroup: twice the two-vector pass's workspace, include/odx.h)
        ws = self._workspace("ktk", 2 * self._pass_bytes("odx_knm_fwd_bwd2_q", max(K.n, 1), K.M, hip.KNM_CODE[K.fmt]))
        vecs = (_p(v), _p(s), _p(out1), _p(out2), _p(t_out))
        if _mapped(K) is not None:
            self._call("odx_knm_fwd_bwd_q_rows_cols_t", *_qblock(K), K.n, K.M, *vecs, _p(ws), ws.numel(), *_cols(K, self.device))
        else:
            self._call("odx_knm_fwd_bwd_q_rows_t", *_qblock(K), K.n, K.M, *vecs, _p(ws), ws.numel())
        return out1, out2

    # ------------------------------------------------------------------ several vectors
    def _ktkn_bytes(self, K, nv):
        return self.lib.odx_knm_fwd_bwdn_q_workspace_bytes(max(K.n, 1), K.M, hip.KNM_CODE[K.fmt], nv)

    def ktkn_width(self, K):
        """The largest number of vectors ONE read of K serves: 8 or 4 where the NV-vector pass over a compact block has a
        configuration (the vectors sit in LDS as f64: 8 up to M = 2524, 4 up to M = 5084), else 2 where the two-vector pass
        exists, else 1.  f32 blocks (small, not HBM-bound) and streamed shards are served by ktk / ktk2 only."""
        if _compact(K):
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
        nbytes = self._pass_bytes("odx_gauss_ktk_stream_h2n", max(K.n, 1), K.M, F.D, g)
        ws = K.ring if K.ring is not None and K.ring.numel() >= nbytes else self._workspace("ktkn_stream", nbytes)
        self._call("odx_gauss_ktk_stream_h2n", _p(F.P), F.P.stride(0), _p(F.meta), _p(F.sq), K.n, _p(Zf.P), Zf.P.stride(0), _p(Zf.meta),
                   _p(Zf.sq), K.M, F.D, K.sigma, g, _p(V[l]), V.stride(0), _p(out[l]), out.stride(0), _p(ws), ws.numel())

    def _ktkn_plan(self, K, L):
        """The calls ktkn makes for L vectors over a stored block, in order: (kind, first vector, count) with kind "nv"
        (odx_knm_fwd_bwdn_q: one read), "wide" (odx_knm_fwdn_q + odx_knm_bwdn_q: two reads), "pair" (ktk2: one read) or
        "single" (one ktk per vector: one read each).  Uses ktkn_width, can_ktk2 and wide_pass_min only."""
        width = self.ktkn_width(K)
        plan, l = [], 0
        wmin = self.wide_pass_min
        if wmin is not None and width <= 2 and _compact(K):
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

    def _nv_call(self, entry, key, K, g, A, B):
        """One of the three NV-vector entries over a compact block: g rows from A[0] on in, g rows from B[0] on out, its
        slabs in the workspace `key` (None: the entry needs none and is only asked whether it serves M)."""
        nbytes = self._pass_bytes(entry, max(K.n, 1), K.M, hip.KNM_CODE[K.fmt], g)
        ws = self._workspace(key, nbytes) if key else None
        self._call(entry, *_qblock(K), K.n, K.M, g, _p(A[0]), A.stride(0), _p(B[0]), B.stride(0), _p(ws), ws.numel() if key else 0)

    def kvn(self, K, V, out=None):
        """out[l] = K V[l] (the row products, f64) for the L >= 1 rows of V ((L, >= M) f64) over a compact stored block: groups
        of up to 8 rows from ONE read each (odx_knm_fwdn_q, every M <= 20440).  out: (L, >= roundup(n, 2)) f64; cells [n:]
        of a row are not written.  Rows of V and out must be 16-byte aligned.  f32 blocks and streamed shards: ValueError
        (the entry is not built for them)."""
        if not _compact(K):
            raise ValueError("kvn: compact stored blocks only (u24 / bf16), got %r" % (K.fmt,))
        _no_map("kvn", K)
        L, M, n = V.shape[0], K.M, K.n
        if out is None:
            out = torch.zeros((L, (n + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        _check_matrix("kvn", "V", V, L, M)
        _check_matrix("kvn", "out", out, L, n)
        _check_aligned("kvn", V=V, out=out)
        for l, g in _groups(L if n > 0 else 0, self.WIDE_PASS_MAX):
            self._nv_call("odx_knm_fwdn_q", None, K, g, V[l:], out[l:])
        return out

    def _ktkn_wide(self, K, V, out, l, g):
        """Rows [l, l + g) of V, g <= 8, from two reads of the block: T = K V (odx_knm_fwdn_q), out = K' T (odx_knm_bwdn_q).
        T has a workspace of its own: "ktk" holds the backward kernel's slabs."""
        ldt = (max(K.n, 1) + 1) // 2 * 2
        T = self._workspace("ktkn_t", g * ldt * 8)[:g * ldt * 8].view(torch.float64).view(g, ldt)
        self.kvn(K, V[l:l + g], out=T)
        self._nv_call("odx_knm_bwdn_q", "ktk", K, g, T, out[l:])

    def ktkn(self, K, V, out=None):
        """out[l] = K' (K V[l]) for the L >= 1 rows of V ((L, ld) f64), with as few reads of K as its width allows: groups of
        ktkn_width(K) rows, a group of 3 .. 8 by odx_knm_fwd_bwdn_q, of 2 by ktk2 (two ktk where the block has no two-vector
        pass), of 1 by ktk.  Where one read serves two vectors at most (M > 5084) and wide_pass_min is set, groups of
        wide_pass_min or more rows go in chunks of up to 8 through TWO reads each (odx_knm_fwdn_q, then odx_knm_bwdn_q);
        what remains below wide_pass_min keeps the pairs and singles.  ktkn_reads(K, L) counts the reads.  A streamed shard:
        groups of ktkn_span(K) = 16 rows, each from ONE build of K (odx_gauss_ktk_stream_h2n; a single row goes through
        ktk).  Columns [0, K.M) of V / out are used; rows must be 16-byte aligned for groups of 3 or more (on a streamed
        shard: of 2 or more)."""
        _no_map("ktkn", K)
        L, M = V.shape[0], K.M
        if out is None:
            out = torch.zeros((L, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        _check_matrix("ktkn", "V", V, L, M)
        _check_matrix("ktkn", "out", out, L, M)
        if K.fmt == "stream":
            for l, g in _groups(L, self.ktkn_span(K)):
                if g == 1:
                    self.ktk(K, v=V[l, :M], out=out[l, :M])
                    continue
                _check_aligned("ktkn", V=V, out=out)
                self._ktkn_stream(K, V, out, l, g)
            return out
        for kind, l, g in self._ktkn_plan(K, L):
            if kind in ("nv", "wide"):
                _check_aligned("ktkn", V=V, out=out)
            if kind == "wide":
                self._ktkn_wide(K, V, out, l, g)
            elif kind == "nv":
                self._nv_call("odx_knm_fwd_bwdn_q", "ktk", K, g, V[l:], out[l:])
            elif kind == "pair":
                self.ktk2(K, V[l, :M], V[l + 1, :M], out1=out[l, :M], out2=out[l + 1, :M])
            else:
                for j in range(l, l + g):
                    self.ktk(K, v=V[j, :M], out=out[j, :M])
        return out

    # ------------------------------------------------------------------ several vectors with row weights
    def _ktkn_rows_plan(self, K, L):
        """The calls ktkn_rows makes for L vectors over a stored block, in order: (kind, first vector, count) with kind "nv"
        (odx_knm_fwd_bwdn_q_rw: one read), "wide" (odx_knm_fwdn_q + odx_knm_bwdn_q: two reads) or "single" (two ktk per
        vector: two reads each)."""
        if not _compact(K):
            return [("single", l, 1) for l in range(L)]
        code = hip.KNM_CODE[K.fmt]
        if self.lib.odx_knm_fwd_bwdn_q_rw_workspace_bytes(max(K.n, 1), K.M, code, 1) >= 0:
            return [("nv", l, g) for l, g in _groups(L, self.ktkn_width(K))]
        return [("wide", l, g) for l, g in _groups(L, self.WIDE_PASS_MAX)]

    def ktkn_rows_reads(self, K, L):
        """The number of reads of the block ktkn_rows(K, V, ...) makes for L vectors."""
        return sum({"nv": 1, "wide": 2, "single": 2 * g}[kind] for kind, _, g in self._ktkn_rows_plan(K, L))

    def ktkn_rows(self, K, V, Dw, wrow, out=None, t_out=None):
        """out[l] = K' (Dw[wrow[l]] o (K V[l])) for the L >= 1 rows of V ((L, >= M) f64): the pass of CG states that are fits
        with row weights over one block (solver.falkon_fit_cv: the folds of a cross-validation).  Dw: (G, >= n) f64, a row
        of n row weights each; wrow: L ints, the row of Dw vector l uses, -1 = no weights.  t_out: optional (L, >= n) f64
        that receives the row products K V[l] as they are BEFORE the weight; `out` is the same bits with or without it.
        A compact block within the NV pass's widths: groups of ktkn_width(K) rows, groups of 1 and 2 included, from ONE read
        each (odx_knm_fwd_bwdn_q_rw).  A wider compact block (up to M = 20440): groups of up to 8 from TWO reads each,
        whatever wide_pass_min says (T = K V by odx_knm_fwdn_q, T o Dw, then odx_knm_bwdn_q).  f32 blocks (small, not
        HBM-bound): per vector ktk(K, v, t_out=t), then ktk(K, w=d o t).  ktkn_rows_reads(K, L) counts the reads.  Rows of V,
        out and Dw must be 16-byte aligned on compact blocks, and those of t_out on the wide route.  A streamed shard
        (its rows pass in chunks) and a block with a column map: ValueError."""
        if K.fmt == "stream":
            raise ValueError("ktkn_rows: needs a stored K_nM block (a streamed shard's rows pass in chunks)")
        _no_map("ktkn_rows", K)
        L, M, n = V.shape[0], K.M, K.n
        wrow = [int(w) for w in wrow]
        G = Dw.shape[0] if Dw is not None else 0
        if len(wrow) != L or any(not -1 <= w < G for w in wrow):
            raise ValueError("ktkn_rows: wrow must name, for each of the %d vectors, one of the %d rows of Dw or -1, got %r" % (L, G, wrow))
        if out is None:
            out = torch.zeros((L, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        _check_matrix("ktkn_rows", "V", V, L, M)
        _check_matrix("ktkn_rows", "out", out, L, M)
        if G:
            _check_matrix("ktkn_rows", "Dw", Dw, G, n)
        if t_out is not None:
            _check_matrix("ktkn_rows", "t_out", t_out, L, n)
        for kind, l, g in self._ktkn_rows_plan(K, L):
            if kind == "single":
                t = t_out[l, :n] if t_out is not None else self._workspace("ktkn_t", max(n, 1) * 8)[:n * 8].view(torch.float64)
                self.ktk(K, v=V[l, :M], out=out[l, :M], t_out=t)
                w = t if wrow[l] < 0 else t * Dw[wrow[l], :n]
                self.ktk(K, w=w, out=out[l, :M])
                continue
            _check_aligned("ktkn_rows", V=V, out=out, **({"Dw": Dw} if G else {}))
            if kind == "nv":
                nbytes = self._pass_bytes("odx_knm_fwd_bwdn_q_rw", max(n, 1), M, hip.KNM_CODE[K.fmt], g)
                ws = self._workspace("ktk", nbytes)
                self._call("odx_knm_fwd_bwdn_q_rw", *_qblock(K), n, M, g, _p(V[l]), V.stride(0), _p(Dw if G else None),
                           Dw.stride(0) if G else 0, (ctypes.c_int32 * g)(*wrow[l:l + g]), _p(out[l]), out.stride(0),
                           _p(None if t_out is None else t_out[l]), 0 if t_out is None else t_out.stride(0), _p(ws), ws.numel())
                continue
            # two reads: T = K V (it is t_out), W = T o Dw in the "ktkn_t" workspace, out = K' W
            ldt = (max(n, 1) + 1) // 2 * 2
            W = self._workspace("ktkn_t", g * ldt * 8)[:g * ldt * 8].view(torch.float64).view(g, ldt)
            if t_out is not None:
                _check_aligned("ktkn_rows", t_out=t_out)
                T = t_out[l:l + g]
            else:
                T = W
            self.kvn(K, V[l:l + g], out=T)
            for j in range(g):
                if wrow[l + j] >= 0:
                    torch.mul(T[j, :n], Dw[wrow[l + j], :n], out=W[j, :n])
                elif T is not W:
                    W[j, :n].copy_(T[j, :n])
            self._nv_call("odx_knm_bwdn_q", "ktk", K, g, W, out[l:])
        return out

    def ktwn(self, K, W, out=None):
        """out[t] = K' W[t] for the T >= 1 rows of W ((T, >= K.n) f64): the right-hand sides of T label columns.  A compact
        stored block: groups of up to 8 rows from ONE read each (odx_knm_bwdn_q, every M the compact passes serve); a group
        of one goes through ktk(K, w=...).  f32 blocks (small, not HBM-bound: ktkn's decision) loop ktk(K, w=...), and so do
        streamed shards — there every row is one recompute of K: a build-once entry for several weight vectors is NOT
        built.  Rows of W and out must be 16-byte aligned for groups of 2 or more."""
        _no_map("ktwn", K)
        T, M, n = W.shape[0], K.M, K.n
        if out is None:
            out = torch.zeros((T, (M + 1) // 2 * 2), dtype=torch.float64, device=self.device)
        _check_matrix("ktwn", "W", W, T, n)
        _check_matrix("ktwn", "out", out, T, M)
        for l, g in _groups(T, self.WIDE_PASS_MAX if _compact(K) else 1):
            if g == 1:
                self.ktk(K, w=W[l, :n], out=out[l, :M])
                continue
            _check_aligned("ktwn", W=W, out=out)
            self._nv_call("odx_knm_bwdn_q", "ktk", K, g, W[l:], out[l:])
        return out

    def trmvn(self, P, name, X, alpha=1.0, beta=0.0, Z=None, out=None):
        """out[t] = alpha * P.<name> X[t] + beta * Z[t] over the rows of (T, >= P.M) f64 matrices: groups of up to 8 rows from
        ONE read of the factor each (odx_trmvn_f64); one row goes through trmv.  out may be Z, not X."""
        T, M = X.shape[0], P.M
        from .backend import require_merged
        require_merged(P, "trmvn")
        if out is None:
            out = torch.zeros((T, P.ld), dtype=torch.float64, device=self.device)
        for nm, t in (("X", X), ("out", out)) + (() if Z is None else (("Z", Z),)):
            _check_matrix("trmvn", nm, t, T, M)
        if beta != 0.0 and Z is None:
            raise ValueError("trmvn: beta needs Z")
        for l, g in _groups(T, 8):
            if g == 1:
                self.trmv(P, name, X[l], alpha=alpha, beta=beta, z=None if Z is None else Z[l], out=out[l])
                continue
            _check_aligned("trmvn", X=X)
            self._call("odx_trmvn_f64", _p(getattr(P, name)), P.ld, M, self._TRI[name], g, _p(X[l]), X.stride(0), float(alpha),
                       float(beta), _p(None if Z is None else Z[l]), 0 if Z is None else Z.stride(0), _p(out[l]), out.stride(0))
        return out

    # ------------------------------------------------------------------ scoring
    def knm_mv(self, K, alpha, out=None, summed=None):
        """(n, 1) f32 = K alpha over a stored K_nM block, from one read of it (odx_knm_mv; f64 sums); `out` may be a
        strided column such as scores[:, c:c + 1].  summed: the caller already holds K alpha as an (n,) f64 vector — the fit
        that produced alpha summed it from its passes' row products (solver.falkon_fit(scores_out=...)) — and the block is
        not read again: the sum is rounded once into `out` (odx_cg_scores_store_f32)."""
        if K.fmt not in hip.KNM_CODE:
            raise ValueError("knm_mv: needs a stored K_nM block, got %r (a streamed shard is scored by mmv)" % (K.fmt,))
        if summed is not None:
            if summed.numel() != K.n:
                raise ValueError("knm_mv: summed has %d entries but the block has %d rows" % (summed.numel(), K.n))
            if out is None:
                out = torch.empty((K.n, 1), dtype=torch.float32, device=self.device)
            return self.cg_scores_store(summed, out)
        alpha = alpha.to(device=self.device, dtype=torch.float64).contiguous()
        if alpha.numel() != _vlen(K):
            raise ValueError("knm_mv: alpha has %d entries but the block has %d columns" % (alpha.numel(), _vlen(K)))
        if _mapped(K) is not None:
            # distinct columns: K_full alpha = K fold(alpha)
            _, start, pos = _cols(K, self.device)[1:]
            folded = torch.empty(K.M, dtype=torch.float64, device=self.device)
            self._call("odx_cols_fold_f64", _p(alpha), K.Mv, start, pos, K.M, _p(folded))
            alpha = folded
        if out is None:
            out = torch.empty((K.n, 1), dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or out.shape[0] != K.n or (out.dim() == 2 and out.shape[1] != 1):
            raise ValueError("knm_mv: out must be an (n,) or (n, 1) f32 tensor")
        self._call("odx_knm_mv", *_qblock(K), K.n, K.M, _p(alpha), _p(out), out.stride(0))
        return out

    def precond_path(self, Zf, sigma, lams, eps, out=None, ws_key="precond"):
        """One Precond per value of `lams` for the same centres.  The members share LTi / LTit (they do not depend on
        lambda) and own their LAi / LAit; member l equals precond(Zf, sigma, lams[l], eps) bit for bit.  `out`: optional
        (2 + 2 L, M, ld) f64 tensor.  A member's info is its word of one (L,) tensor."""
        from .backend import Precond
        Zf = self.f32(Zf)                    # (16-bit centres: the chain takes their f32 form, as precond does)
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
        sigma, kind = hip.radial_of(sigma)
        if kind:             # a Matern kernel object: K_MM is that kernel's, the chain behind it the same
            hip.check(self.lib.odx_falkon_precond_path_radial_f64(_p(Zf.X), Zf.ld, M, D, sigma, kind, (ctypes.c_double * L)(*lams), L,
                                                                  float(eps), _p(mats[0]), _p(mats[1]), _p(mats[2]), ld, _p(info), _p(ws),
                                                                  ws.numel(), self._stream()), "odx_falkon_precond_path_radial_f64")
        else:
            hip.check(self.lib.odx_falkon_precond_path_f64(_p(Zf.X), Zf.ld, M, D, sigma, (ctypes.c_double * L)(*lams), L, float(eps),
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
