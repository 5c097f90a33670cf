"""The big-n job of SURVEY §8e's first row as a schedule: C one-vs-rest FALKON fits + score-all over rows sharded on the
ranks of one node, classes advancing in lock-step batches of `world`, preconditioners built ahead on side streams.

This is what `bench.py` times; it lives in the package so that its CONTROL FLOW — which rank owns which class of a batch,
how the owned classes are grouped into class-batched preconditioner chains (the group size must be the same on every rank:
the centres of a group's classes are assembled with collectives), which collectives every rank issues in which order —
runs under gloo on CPU ranks with the tests' oracle backend at world sizes no single-GPU box can host
(tests/test_dist_gloo.py: 8 ranks, 30 classes -> batches of 8, 8, 8, 6 and preconditioner groups of 1 + 3).

How many classes advance together (b, a divisor of the world size) and how many classes one chain builds per rank (g) come
from a memory plan (odx/plan.py): b K_nM shards and 2 x g sets of factors per rank must fit the GPU's HBM beside the rows.
With b < world the owners of consecutive batches rotate through the ranks (a ROUND of world / b batches gives every rank
one class), and the chain groups are counted in rounds.

The reference has no counterpart (single process, class-by-class loop: OnlineRegionClassifier_incore.py:96-155); the
arithmetic per class is odx.solver.falkon_fit_lockstep's, i.e. falkon_fit's.
"""
import contextlib

import torch

from . import cols as _cols
from . import plan as _plan
from . import solver
from .dist import RowShard


class _Side:
    """A side stream with an event, or (CPU tensors) nothing: work is then simply done in program order."""

    def __init__(self, device, be=None, cus=0, index=0):
        self.cuda = torch.device(device).type == "cuda"
        self.stream = None
        if self.cuda and cus > 0 and be is not None and hasattr(be, "masked_stream"):
            # confined to `cus` compute units (spread over the XCDs): the factorisation chains then pack their workgroups on
            # those instead of holding one slot on many CUs, each of which takes no Gaussian workgroup meanwhile
            self.stream = be.masked_stream(cus)
        elif self.cuda:
            # a stream measured to sit on a hardware queue of its own (odx/streams.py): the chain must not queue behind the
            # builds and passes of the main stream
            from . import streams as _streams
            own = _streams.distinct(index + 1, device)
            self.stream = own[index] if len(own) > index else torch.cuda.Stream(device=device)

    def after_current(self):
        if self.cuda:
            self.stream.wait_stream(torch.cuda.current_stream())

    def __enter__(self):
        self._ctx = torch.cuda.stream(self.stream) if self.cuda else contextlib.nullcontext()
        return self._ctx.__enter__()

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)

    def mark(self):
        """An event after everything queued on the side stream so far (None on the CPU)."""
        if not self.cuda:
            return None
        ev = torch.cuda.Event()
        ev.record(self.stream)
        return ev


def t_inverse_stop(M, unmerged, force=0):
    """THE rule for who gets a partial inverse of T (backend.precond_batched's t_stop; 0 = fully merged).  Only a lock-step job
    asks, only for more than 8192 centres, and only the top `unmerged` (1 or 2) merge levels of 4096 rows and more stay
    unmerged: at M = 10 000, 1 -> 8192 (blocks 8192 | 1808), 2 -> 4096 (4096 | 4096 | 1808).  No problem of 8192 centres or
    fewer changes.  force > 0 (the library's test hook "t_inverse_force_stop"): that level for every size with rows beyond it."""
    M, unmerged, force = int(M), int(unmerged), int(force)
    if force > 0:
        return force if M > force else 0
    if unmerged <= 0 or M <= 8192:
        return 0
    top = 128
    while 2 * top < M:
        top *= 2                          # the last merge level: the largest 128 2^k below M
    return max(top >> (unmerged - 1), 4096)


def _wait(ev):
    if ev is not None:
        torch.cuda.current_stream().wait_event(ev)


class _OnStream:
    """`inner` (a phase timer or nothing) entered on `stream`, joined to the current stream on both sides: the launches of the
    block run on `stream` in the order the current stream would have given them."""

    def __init__(self, stream, inner):
        self.stream, self.inner = stream, inner

    def __enter__(self):
        self.cur = torch.cuda.current_stream()
        self.stream.wait_stream(self.cur)
        self.ctx = torch.cuda.stream(self.stream)
        self.ctx.__enter__()
        return self.inner.__enter__()

    def __exit__(self, *exc):
        r = self.inner.__exit__(*exc)
        self.ctx.__exit__(*exc)
        self.cur.wait_stream(self.stream)
        return r


precond_groups = _plan.precond_groups       # (kept under its old name: tests and tools import it from here)


class LockstepClassJob:
    """C binary problems on the same (sharded) rows X: labels(c) -> this rank's f64 label vector, centre_idx[c] -> global
    row ids of class c's Nystroem centres (identical on every rank)."""

    def __init__(self, be, X, n_total, M, labels, centre_idx, sigma, lam, maxiter=20, opt=None, shard=None,
                 precond_batch=0, precond_depth=2, precond_after_fit=False, classes=None, precond_cus=0, batch=0,
                 hbm_bytes=None, exchange="lockstep", gauss_on_complement=False, precond_lookahead=1, precond_cus_full_only=False,
                 score_from_knm=True, scores_from_cg=True, distinct_columns="auto"):
        """precond_batch: classes per rank and preconditioner chain (g; 0 = planned, 1 = one chain per class on `precond_depth`
        side streams); batch: classes per lock-step batch (b, a divisor of the world size; 0 = planned); hbm_bytes: the
        memory the plan may count on per rank (default: the device's, 288 GB without one).
        exchange: "lockstep" — batches of b classes, one owner rank per class, per CG iteration one all-gather of the
        directions and one reduce-scatter of the partials (what bench.py times); "allreduce" — the north star's literal form:
        classes one at a time, EVERY rank builds every class's preconditioner and runs every M-sized product, per CG iteration
        ONE all-reduce of the (M,) partial (solver.falkon_fit's replicated mode).  Same arithmetic per class either way.
        score_from_knm: score a class from the K_nM shard its fit has just stored (one read of it, backend.knm_mv) where
        that shard holds the f32-accurate entries (see _score); False: always recompute K(X, Z) alpha (backend.mmv).
        scores_from_cg: where this rank holds the CG state of a class (one rank, or exchange "allreduce") and that shard
        qualifies (solver.scores_from_cg), sum the scores from the row products of the CG's own passes and hand the sum to
        knm_mv, which then does not read the shard again; with score_from_knm off, or on several lock-step ranks, it has no effect.
        distinct_columns: the centre rule draws with replacement, so a class's K_nM block repeats some columns.  "auto": a
        class with repeated centres whose shard is stored compact (u24 / bf16) and has at least 2^27 entries per rank (the
        size bound of the automatic compact-storage rule) builds and streams its DISTINCT columns only (odx/cols.py; every
        M-vector, the preconditioner, alpha and the scores keep their meaning, only f64 summation order moves); "force": the
        same without the size bound (tests); False: never.  f32-stored and streamed shards never do."""
        # gauss_on_complement (with precond_cus = k > 0; an experiment, round-5 review item 1a): the K_nM builds and the scoring run
        # on a stream confined to the OTHER total - k compute units, so that chain and Gaussian workgroups never share a CU.
        # precond_lookahead = L: chain groups in flight ahead of the group being fitted (L + 1 factor blocks; 1 = round 2-5's
        # schedule).  precond_cus = k > 0 confines the chains to k compute units; with precond_cus_full_only the ramp groups
        # (fewer than g classes: the ones the first fits wait for) keep the whole chip and only the full-size groups — which have
        # L groups' worth of fits to finish in — are confined: their f64 work then runs beside the HBM-bound passes, which lose
        # little to it, instead of beside the MFMA-bound builds, which lose all of it.
        if exchange not in ("lockstep", "allreduce"):
            raise ValueError("LockstepClassJob: exchange must be 'lockstep' or 'allreduce', got %r" % (exchange,))
        self.exchange = exchange
        self.score_from_knm = bool(score_from_knm)
        self.scores_from_cg = bool(scores_from_cg) and self.score_from_knm
        if distinct_columns not in ("auto", False, "force"):
            raise ValueError("LockstepClassJob: distinct_columns must be 'auto', False or 'force', got %r" % (distinct_columns,))
        self.distinct_columns = distinct_columns
        if exchange == "allreduce":
            batch = 1                             # one stored K_nM shard in flight; the plan's b = 1 line is this mode's memory
        self.be, self.X, self.N, self.M = be, X, int(n_total), int(M)
        self.labels, self.cidx = labels, centre_idx
        self.sigma, self.lam, self.maxiter = sigma, lam, maxiter
        self.opt = opt or solver.SolverOptions(check_pivots=False)
        self.shard = shard if shard is not None else RowShard()
        self.world, self.rank = self.shard.world, self.shard.rank
        self.lo, self.hi = self.shard.bounds(self.N)
        self.n_loc = self.hi - self.lo
        dev = X.device
        self.C = len(centre_idx) if classes is None else int(classes)
        self.ldk = (self.M + 3) // 4 * 4
        # The plan (the same on every rank: derived from N, D, M, C, world and the budget only): b K_nM shards — one per
        # class of the batch in flight, in the backend's storage format — and 2 x g sets of factors per rank.
        D = int(X.shape[1]) if X.dim() == 2 else 0
        self.plan = _plan.plan_lockstep(
            self.N, D, self.M, self.C, self.world, batch=batch, chain=precond_batch,
            hbm_bytes=hbm_bytes if hbm_bytes is not None else (_plan.device_hbm_bytes(dev) if dev.type == "cuda" else _plan.HBM_BYTES_MI355X),
            knm_format=(be.knm_format if hasattr(be, "knm_format") else None),
            knm_bytes=(be.knm_bytes if hasattr(be, "knm_bytes") else None), gauss=getattr(be, "gauss", "h2"),
            lookahead=max(1, int(precond_lookahead)), chain_sides=2 if (precond_cus_full_only and precond_cus > 0) else 1)
        if not self.plan.feasible:
            raise MemoryError("LockstepClassJob: this job does not fit %d rank(s): %s" % (self.world, self.plan.summary()))
        self.b, self.G = self.plan.b, self.plan.g
        self.R = self.world // self.b                   # batches per round (every rank owns one class per round)
        # (streamed shards, knm_storage "stream": each buffer is the ring of a class's streamed passes, not a block)
        kbytes = (be.knm_bytes(self.n_loc, self.M, D) if self.plan.knm_format == "stream" else be.knm_bytes(self.n_loc, self.M)) \
            if hasattr(be, "knm_bytes") else self.n_loc * self.ldk * 4
        self.kbufs = [torch.empty(max(kbytes, 16), dtype=torch.uint8, device=dev) for _ in range(self.b)]
        self.scores = torch.empty((self.n_loc, self.C), dtype=torch.float32, device=dev)
        # the f64 sum of a class's scores while its CG runs (scores_from_cg); rounded once into its column of `scores`
        self.sbuf = (torch.empty(self.n_loc, dtype=torch.float64, device=dev)
                     if self.scores_from_cg and (self.shard.world == 1 or exchange == "allreduce") and hasattr(be, "cg_scores_axpy")
                     else None)
        self.depth = precond_depth if precond_depth > 0 else 2
        self.after_fit = bool(precond_after_fit)
        self.ld_p = (self.M + 1) // 2 * 2
        self.nslot = self.depth + 1
        self.sides = [_Side(dev, be, precond_cus, index=k) for k in range(self.nslot)] if self.G == 1 else []
        self.lookahead = max(1, int(precond_lookahead))
        self.precond_cus, self.full_only = int(precond_cus), bool(precond_cus_full_only and precond_cus > 0)
        grouped = self.G > 1 or exchange == "allreduce"
        # gside: the chains' side stream (confined when precond_cus > 0 and not full_only); cside: the confined stream of the
        # full-size groups under full_only
        self.gside = _Side(dev, be, 0 if self.full_only else precond_cus) if grouped else None
        self.cside = _Side(dev, be, precond_cus, index=1) if (grouped and self.full_only) else None
        self._cplans = {}        # class -> the centre-assembly plan of gather_centres (world > 1)
        self._cmaps = {}         # class -> the column map of its repeated centres (distinct_columns), where it has one
        self.gauss_stream = (be.masked_stream(precond_cus, complement=True)
                             if gauss_on_complement and precond_cus > 0 and dev.type == "cuda" and hasattr(be, "masked_stream") else None)
        self.pbuf, self.pgroup = [], []
        self.trace = []          # (kind, payload) records of the schedule this rank executed (tests read it)
        if self.world > 1 and not getattr(self.shard, "emulated", False):
            # who owns which centre row: host arithmetic on the job's inputs (like the memory plan), made for every class NOW —
            # its one device-to-host read per class must not land inside a step
            for idx in self.cidx[:self.C]:
                if torch.is_tensor(idx):
                    self._centre_plan(idx)
        if (distinct_columns and hasattr(be, "knm_format") and be.knm_format(self.n_loc, self.M) in ("u24", "bf16")
                and (distinct_columns == "force" or self.n_loc * self.M >= 2 ** 27)):
            # which centres of a class repeat: host arithmetic on the job's inputs, like the ownership plan above, and the
            # map's copy to the device — made for every class NOW, nothing of it waits for the GPU inside a step
            for idx in self.cidx[:self.C]:
                if torch.is_tensor(idx):
                    cmap = _cols.column_map(idx)
                    if cmap is not None:
                        cmap.on(dev)
                        self._cmaps[self._idx_key(idx)] = cmap
        if self.G > 1 and hasattr(be, "precond_batched") and hasattr(be, "lib") and dev.type == "cuda":
            # the two factor blocks and the chain's scratch at their final size now, not inside the first step that needs them
            # (a warm-up on a few classes runs smaller chains: the 22 GB scratch of a 6-class chain was first allocated in the
            # timed region)
            while len(self.pgroup) < self.lookahead + 1:
                self.pgroup.append(torch.empty((self.G, 4, self.M, self.ld_p), dtype=torch.float64, device=dev))
            for side in (self.gside, self.cside):
                if side is not None:
                    with side:
                        be._workspace("precond_group", be.lib.odx_falkon_precond_batched_workspace_bytes(self.M, D, self.G))

    def _t_stop(self):
        """The stop level of T's inverse for this job's class-batched chains (t_inverse_stop, from the library's options)."""
        lib = getattr(self.be, "lib", None)
        if lib is None or not hasattr(lib, "odx_get_option"):
            return 0
        import ctypes
        got = {}
        for name in ("t_inverse_unmerged", "t_inverse_force_stop"):
            v = ctypes.c_int(0)
            if lib.odx_get_option(name.encode(), ctypes.byref(v)) != 0:
                raise RuntimeError("odx_get_option(%s) failed" % name)
            got[name] = v.value
        return t_inverse_stop(self.M, got["t_inverse_unmerged"], got["t_inverse_force_stop"])

    def release(self):
        self.kbufs, self.pbuf, self.pgroup, self.scores, self.sbuf = [], [], [], None, None

    # ------------------------------------------------------------------ pieces
    @staticmethod
    def _idx_key(idx):
        return (idx.data_ptr(), int(idx.numel()))

    def _with_map(self, Zf, idx):
        """The centres' Features, carrying the class's column map where it has one (backend.knm_rhs then stores the distinct
        columns only; the preconditioner is built from all M centres either way)."""
        cmap = self._cmaps.get(self._idx_key(idx)) if self._cmaps else None
        if cmap is not None:
            Zf.cmap = cmap
        return Zf

    def _centre_plan(self, idx):
        """Who owns which centre row (every row of X has exactly one owner rank): per class, once, from the job's inputs —
        `mine` = local row ids of the centres this rank owns (in idx order), `cmax` = the largest count any rank owns (every
        rank contributes a block of that many rows), `slot` = for centre p its row in the gathered (world x cmax) block."""
        key = (idx.data_ptr(), int(idx.numel()))
        plan = self._cplans.get(key)
        if plan is None:
            from .dist import shard_bounds
            ih = idx.detach().cpu().to(torch.int64)
            los = torch.tensor([shard_bounds(self.N, self.world, r)[0] for r in range(self.world)], dtype=torch.int64)
            owner = torch.bucketize(ih, los, right=True) - 1
            counts = torch.bincount(owner, minlength=self.world)
            cmax = max(int(counts.max()), 1)
            order = torch.argsort(owner, stable=True)                       # positions grouped by owner, idx order inside
            starts = torch.cumsum(counts, 0) - counts
            within = torch.empty_like(ih)
            within[order] = torch.arange(ih.numel(), dtype=torch.int64) - starts[owner[order]]
            mine = ih[owner == self.rank] - self.lo
            dev = self.X.device
            plan = (mine.to(dev), cmax, (owner * cmax + within).to(dev), int(counts[self.rank]))
            self._cplans[key] = plan
        return plan

    def gather_centres(self, idx):
        """Z = X_global[idx].  Every centre row lives on exactly one rank: each rank contributes the rows it owns (padded to
        the largest count over the ranks), ONE all-gather assembles them, a row gather puts them in idx order — (W - 1) / W
        of the (M x D) block per rank on a ring, where the zero-padded all-reduce this replaces moved twice that and had
        every rank write and sum a full block (round-5 review, weak 10)."""
        # no boolean-mask indexing on device tensors here: it would make the host wait for the GPU (nonzero), and the ~1500
        # launches of the next preconditioner are then enqueued while the main stream has nothing to run (33 ms per class,
        # measured); the ownership plan is host arithmetic on the job's inputs, made once per class
        be, X = self.be, self.X
        if self.world == 1:
            return self._with_map(be.features(X.index_select(0, idx)), idx)
        if getattr(self.shard, "emulated", False):
            # one rank of an emulated world: the (folded) indices all point at this rank's rows; the real rank would own M / W
            # of them and receive the rest — the gather runs locally, the collective is counted at its real size
            Z = X.index_select(0, idx - self.lo)
            self.shard._count("centre_gather", Z)
            return self._with_map(be.features(Z), idx)
        mine, cmax, slot, n_mine = self._centre_plan(idx)
        blk = torch.zeros((cmax, X.shape[1]), dtype=X.dtype, device=X.device)
        if n_mine:
            torch.index_select(X, 0, mine, out=blk[:n_mine])
        allb = torch.empty((self.world, cmax, X.shape[1]), dtype=X.dtype, device=X.device)
        self.shard.gather_blocks(blk, allb)
        return self._with_map(be.features(allb.view(self.world * cmax, X.shape[1]).index_select(0, slot)), idx)

    def _score(self, ph, F, Z, K, alpha, c, summed=False):
        """scores[:, c] = K(X, Z) alpha.  summed: the fit has left K alpha in self.sbuf (f64, summed from the row products
        of its CG passes: solver.scores_from_cg) — backend.knm_mv then rounds that sum into the column, no read of K.  Otherwise from the
        stored shard K the fit has just streamed when its entries are the Gaussian's f32-accurate values (gauss "h2", stored as 24-bit fixed point or f32): one HBM-bound read of it, timed with the passes
        ("ktk"), instead of a second 2 n M D contraction.  bf16 / f8 shards are ~1e-3 off, so their scores (and those of a
        backend without knm_mv) are recomputed by the contraction.  The next batch's build overwrites K only after this
        launch, in stream order."""
        be = self.be
        if summed:
            # (outside the "ktk" timer: an n-sized rounding, not a read of the block)
            be.knm_mv(K, alpha, out=self.scores[:, c:c + 1], summed=self.sbuf)
        elif (self.score_from_knm and K is not None and hasattr(be, "knm_mv") and getattr(be, "gauss", None) == "h2"
                and getattr(K, "fmt", None) in ("u24", "f32")):
            with ph("ktk"):
                be.knm_mv(K, alpha, out=self.scores[:, c:c + 1])
        else:
            with ph("mmv"):
                be.mmv(F, Z, self.sigma, alpha, None, out=self.scores[:, c:c + 1])

    def _prepare(self, batch, owners, slot, ph, infos):
        """Per-class mode (G == 1): centres of the batch's classes (one all-reduce each, main stream) and, on the slot's side
        stream, the preconditioner of the class this rank owns in the batch."""
        be, dev = self.be, self.X.device
        while len(self.pbuf) < self.nslot:
            self.pbuf.append(torch.empty((4, self.M, self.ld_p), dtype=torch.float64, device=dev))
        Zs = [self.gather_centres(self.cidx[c]) for c in batch]
        P, ev = None, None
        if self.rank in owners:
            pos = owners.index(self.rank)
            side = self.sides[slot]
            side.after_current()          # the slot's last reader is done, the centres exist
            with side:
                with ph("precond"):
                    kw = {"out": self.pbuf[slot], "ws_key": "precond%d" % slot} if hasattr(be, "precond_batched") else {}
                    P = be.precond(Zs[pos], self.sigma, self.lam, self.opt.pc_epsilon, **kw)
                ev = side.mark()
            if infos is not None and hasattr(P, "info"):
                infos.append(P.info)
            self.trace.append(("precond", (batch[pos],)))
        return Zs, P, ev

    def _prepare_group(self, group, slot, ph, infos):
        """Class-batched mode: centres of every class of the group's batches (main stream) and, on the side stream, the
        preconditioners of the classes this rank owns among them (at most one per round, g per group), all by one batched
        call.  group: [(classes, owners)] of the group's batches.  One (Zs, P, event) per batch."""
        be, dev = self.be, self.X.device
        Zs_all = [[self.gather_centres(self.cidx[c]) for c in batch] for batch, _ in group]
        own = [(k, owners.index(self.rank)) for k, (_, owners) in enumerate(group) if self.rank in owners]
        Ps, ev = {}, None
        if own:
            confined = self.cside is not None and len(own) >= self.G        # (full_only: a full-size group)
            side = self.cside if confined else self.gside
            if self.precond_cus > 0 and hasattr(be, "set_helper_cus"):
                # the library's helper streams of a chain are created — with the mask current at that moment — when a caller
                # stream first needs them: confined for the confined stream's chains, the whole chip for the others
                be.set_helper_cus(self.precond_cus if (confined or not self.full_only) else 0)
            side.after_current()          # the slot's last readers were issued, the centres exist
            with side:
                with ph("precond"):
                    zf = [Zs_all[k][pos] for k, pos in own]
                    if hasattr(be, "precond_batched"):
                        while len(self.pgroup) < self.lookahead + 1:
                            self.pgroup.append(torch.empty((self.G, 4, self.M, self.ld_p), dtype=torch.float64, device=dev))
                        plist = be.precond_batched(zf, self.sigma, self.lam, self.opt.pc_epsilon,
                                                   out=self.pgroup[slot][:len(own)], ws_key="precond_group", t_stop=self._t_stop())
                    else:                 # a backend without the batched chain (tests' oracle backend): one after the other
                        plist = [be.precond(z, self.sigma, self.lam, self.opt.pc_epsilon) for z in zf]
                ev = side.mark()
            Ps = dict(zip((k for k, _ in own), plist))
            if infos is not None:
                infos.extend(p.info for p in plist if hasattr(p, "info"))
            self.trace.append(("precond", tuple(group[k][0][pos] for k, pos in own)))
        return [(Zs_all[k], Ps.get(k), ev) for k in range(len(group))]

    def _run_replicated(self, F, classes, ph, phases, infos, alphas_out):
        """exchange = "allreduce": the classes one after the other; every rank builds every preconditioner (class-batched
        chains over groups of 1, 2, 3, g classes, one group ahead on the side stream) and runs the whole M-sized algebra of
        every class; per CG iteration one all-reduce of the (M,) partial of its K_nM pass (two vectors on the folded one)."""
        be, dev = self.be, self.X.device
        groups = precond_groups(len(classes), max(self.G, 1))

        def prepare(gi):
            cls = [classes[k] for k in groups[gi]]
            Zs = [self.gather_centres(self.cidx[c]) for c in cls]
            self.gside.after_current()
            with self.gside:
                with ph("precond"):
                    if hasattr(be, "precond_batched") and len(cls) > 1:
                        g = max(self.G, len(cls))
                        while len(self.pgroup) < 2:
                            self.pgroup.append(torch.empty((g, 4, self.M, self.ld_p), dtype=torch.float64, device=dev))
                        plist = be.precond_batched(Zs, self.sigma, self.lam, self.opt.pc_epsilon,
                                                   out=self.pgroup[gi % 2][:len(cls)], ws_key="precond_group", t_stop=self._t_stop())
                    else:
                        plist = [be.precond(z, self.sigma, self.lam, self.opt.pc_epsilon) for z in Zs]
                ev = self.gside.mark()
            if infos is not None:
                infos.extend(p.info for p in plist if hasattr(p, "info"))
            self.trace.append(("precond", tuple(cls)))
            return {c: (z, p, ev) for c, z, p in zip(cls, Zs, plist)}

        ready = prepare(0) if groups else {}
        first_of = {grp[0]: gi for gi, grp in enumerate(groups)}
        out = None
        for k, c in enumerate(classes):
            gi = first_of.get(k)
            if gi is not None and gi + 1 < len(groups):
                ready.update(prepare(gi + 1))
            Z, P, ev = ready.pop(c)
            self.trace.append(("fit", (c,)))
            Ks = []
            alpha = solver.falkon_fit(be, F, self.labels(c), Z, self.sigma, self.lam, self.maxiter, self.opt, n_total=self.N,
                                      shard=self.shard, owner=None, knm_out=self.kbufs[0],
                                      phase=(lambda name: phases[name]) if phases is not None else None,
                                      precond=P, precond_ready=(lambda ev=ev: _wait(ev)), knm_blocks=Ks, scores_out=self.sbuf)
            self.trace.extend(("distinct", (c, K.M)) for K in Ks if getattr(K, "cmap", None) is not None)
            if alphas_out is not None:
                alphas_out[c] = alpha
            self._score(ph, F, Z, Ks[0] if Ks else None, alpha, c,
                        summed=self.sbuf is not None and bool(Ks) and solver.scores_from_cg(be, Ks[0]))
            out = (alpha, Z)
        if hasattr(be, "release_helper_streams"):
            be.release_helper_streams()
        return out

    # ------------------------------------------------------------------ the schedule
    def run(self, F, classes=None, phases=None, infos=None, alphas_out=None):
        """Fit and score `classes` (default: all).  F: Features of this rank's rows.  phases: name -> context manager
        (bench.py's HIP-event timers) or None; infos: list collecting the Cholesky status words; alphas_out: optional dict
        that receives class -> alpha (M,) f64 of every fitted class.  Returns (alpha, Zf) of the last class."""
        be, world, rank = self.be, self.world, self.rank
        classes = list(range(self.C)) if classes is None else list(classes)
        base = (lambda name: phases[name]) if phases is not None else (lambda name: contextlib.nullcontext())
        if self.gauss_stream is not None:
            ph = lambda name: _OnStream(self.gauss_stream, base(name)) if name in ("knm", "mmv") else base(name)      # noqa: E731
        else:
            ph = base
        if self.exchange == "allreduce":
            return self._run_replicated(F, classes, ph, phases, infos, alphas_out)
        sched = _plan.lockstep_batches(classes, world, self.b)          # [(classes of the batch, their owner ranks)]
        out = None
        if self.G > 1:
            # chain groups are counted in ROUNDS (R = world / b consecutive batches: one class per rank): sizes 1, 2, 3, then g
            n_rounds = (len(sched) + self.R - 1) // self.R
            groups = [[bi for r in grp for bi in range(r * self.R, min((r + 1) * self.R, len(sched)))]
                      for grp in precond_groups(n_rounds, self.G)]
            first_of = {grp[0]: gi for gi, grp in enumerate(groups)}
            L, nb = self.lookahead, self.lookahead + 1
            ready = {}
            for g0 in range(min(L, len(groups))):          # the first L groups are issued before the first fit
                ready.update(zip(groups[g0], self._prepare_group([sched[bi] for bi in groups[g0]], g0 % nb, ph, infos)))
        else:
            ready = {bi: self._prepare(*sched[bi], bi % self.nslot, ph, infos) for bi in range(min(self.depth, len(sched)))}
        for bi, (batch, owners) in enumerate(sched):
            if self.G > 1:
                gi = first_of.get(bi)
                if gi is not None and gi + L < len(groups):          # L groups ahead, on the side stream(s); block (gi + L) % nb was
                    # group gi - 1's: its fits are queued in front of this point
                    ready.update(zip(groups[gi + L], self._prepare_group([sched[k] for k in groups[gi + L]], (gi + L) % nb, ph, infos)))
            elif not self.after_fit and bi + self.depth < len(sched):
                ready[bi + self.depth] = self._prepare(*sched[bi + self.depth], (bi + self.depth) % self.nslot, ph, infos)
            Zs, P, ev = ready.pop(bi)
            ys = [self.labels(c) for c in batch]
            mine = rank in owners
            self.trace.append(("fit", tuple(batch)))
            Ks = []
            alphas = solver.falkon_fit_lockstep(be, F, ys, Zs, self.sigma, self.lam, self.maxiter, self.opt, n_total=self.N,
                                                shard=self.shard, knm_outs=self.kbufs[:len(batch)],
                                                phase=ph if (phases is not None or self.gauss_stream is not None) else None,
                                                precond=P if mine else None,
                                                precond_ready=(lambda: _wait(ev)) if mine else None, owners=owners, knm_blocks=Ks,
                                                scores_out=[self.sbuf] if (self.sbuf is not None and len(batch) == 1) else None)
            if self.G == 1 and self.after_fit and bi + self.depth < len(sched):
                # issued behind this batch's CG in stream order: the factorisations then run beside the MFMA-bound scoring
                # of this batch and K_nM build of the next, and the HBM-bound passes keep the chip to themselves
                ready[bi + self.depth] = self._prepare(*sched[bi + self.depth], (bi + self.depth) % self.nslot, ph, infos)
            self.trace.extend(("distinct", (c, K.M)) for c, K in zip(batch, Ks) if getattr(K, "cmap", None) is not None)
            if alphas_out is not None:
                alphas_out.update((c, alphas[pos]) for pos, c in enumerate(batch))
            summed = self.sbuf is not None and len(batch) == 1 and len(Ks) == 1 and solver.scores_from_cg(be, Ks[0])
            for pos, c in enumerate(batch):
                self._score(ph, F, Zs[pos], Ks[pos] if pos < len(Ks) else None, alphas[pos], c, summed=summed)
            out = (alphas[-1], Zs[-1])
        if hasattr(be, "release_helper_streams"):
            # the chains' internal helper streams go when the step is queued (their work completes first; the next step's first
            # chain makes them again): left alive and idle they slow every later small launch of the process
            be.release_helper_streams()
        return out
