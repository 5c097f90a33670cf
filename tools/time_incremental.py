#!/usr/bin/env python3
"""Timings of the incremental fit (profiles/incremental_fit.md), one process, HIP-event times:

  (a) odx_knm_gram_f64 alone against the composition the library offered before it for the same matrix — a transposed copy of
      the block, odx_convert_f32_f64 of K', odx_gemm_nt_f64 — alternating.  The GEMM with ODX_GEMM_LOWER_ONLY leaves the tiles
      above the diagonal unwritten (half of what odx_knm_gram_f64 delivers); without the flag it writes both triangles; a
      transposed copy of the result stands for the mirror pass that would complete the lower tiles
  (b) odx_symvn_f64 at nv = 1 and 2 against a device-to-device copy of the same number of bytes
  (c) partial_fit of a batch of new rows onto a model that has seen many, against InCoreFalkon.fit on all rows with the same
      centres, and the break-even batch size

With --outputs T[,T...] (profiles/incremental_multi.md), instead of the parts above:

  (d) odx_knm_gram_rhsn_f64 alone at nt = 1, 8, 32 and 64 against odx_knm_gram_f64 with one y on the same 1 GiB f32 chunk
      (M = 2048 and M = 8192), alternating
  (e) per T: partial_fit (solve=False) of one batch of 2e5 rows, D = 1024, M = 2048 into a model of T outputs against T
      one-output models fed the same batch, and solve() likewise
  (f) per T: solve_path with 8 penalties against 8 calls of solve(penalty)

Usage: python tools/time_incremental.py [--part a|b|c|d|e|f] [--reps R] [--outputs T[,T...]]
Prints one JSON line per measurement: median, min and max of the repetitions in ms."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "online-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402

import odx              # noqa: E402
from odx import hip     # noqa: E402
from odx.knm_path import _p   # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def report(what, **kw):
    for k, v in list(kw.items()):
        if isinstance(v, list):
            kw[k] = stats(v)
    print(json.dumps(dict(what=what, **kw)), flush=True)


def alternate(fns, reps):
    """reps rounds over the functions, so that drift of clocks and temperature hits all alike."""
    out = [[] for _ in fns]
    for f in fns:
        timed(f, 0)
    for _ in range(reps):
        for i, f in enumerate(fns):
            out[i] += timed(f, 1, warm=0)
    return out


def part_a(be, reps):
    from odx.backend import Knm
    for n, M in ((16384, 2000), (4096, 10000)):
        K = Knm()
        K.n, K.M, K.ld = n, M, (M + 3) // 4 * 4
        K.K = torch.rand((n, K.ld), dtype=torch.float32, device="cuda")
        w = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.randn(n, dtype=torch.float64, device="cuda")
        ldg = (M + 1) // 2 * 2
        G = torch.zeros((M, ldg), dtype=torch.float64, device="cuda")
        b = torch.zeros(M, dtype=torch.float64, device="cuda")
        ldt = (n + 1) // 2 * 2
        Kt = torch.zeros((M, n), dtype=torch.float32, device="cuda")
        Kt64 = torch.zeros((M, ldt), dtype=torch.float64, device="cuda")
        G2 = torch.zeros((M, ldg), dtype=torch.float64, device="cuda")
        s = be._stream()

        def gram():
            be.knm_gram(K, beta=0.0, G=G)

        def gram_wy():
            be.knm_gram(K, w=w, y=y, beta=1.0, G=G, b=b)

        def composed():
            hip.check(be.lib.odx_convert_f32_f64(_p(Kt), n, _p(Kt64), ldt, M, n, s), "odx_convert_f32_f64")
            hip.check(be.lib.odx_gemm_nt_f64(_p(Kt64), ldt, _p(Kt64), ldt, _p(G2), ldg, M, M, n, 1.0, 0.0, hip.GEMM_LOWER_ONLY, s),
                      "odx_gemm_nt_f64")

        def composed_t():
            Kt.copy_(K.K[:, :M].t())
            composed()

        def composed_full():
            Kt.copy_(K.K[:, :M].t())
            hip.check(be.lib.odx_convert_f32_f64(_p(Kt), n, _p(Kt64), ldt, M, n, s), "odx_convert_f32_f64")
            hip.check(be.lib.odx_gemm_nt_f64(_p(Kt64), ldt, _p(Kt64), ldt, _p(G2), ldg, M, M, n, 1.0, 0.0, 0, s), "odx_gemm_nt_f64")

        Gt = torch.zeros((M, M), dtype=torch.float64, device="cuda")

        def composed_mirror():
            # the lower-tile composition plus a mirror pass.  The library has no mirror kernel: one transposed copy of the whole
            # matrix by torch stands for it (it moves twice the bytes a copy of one triangle would, and its result still has
            # to be merged into G: the figure is an estimate of such a pass, not the time of a route that exists)
            composed_t()
            Gt.copy_(G2[:, :M].t())

        Kt.copy_(K.K[:, :M].t())
        tg, tw, tc, tt, tf, tm = alternate([gram, gram_wy, composed, composed_t, composed_full, composed_mirror], reps)
        composed()
        # both routes compute the tiles on and below the diagonal: n M (M + 1) multiply-adds
        flop = 2.0 * n * M * (M + 1) / 2.0
        gram()                                                   # (G holds the weighted sums of the last round: K'K again)
        low = torch.tril(G[:, :M])
        diff = float((low - torch.tril(G2[:, :M])).abs().max() / low.abs().max())
        report("gram", n=n, M=M, knm_gram=tg, knm_gram_w_y_beta1=tw, convert_gemm_lower=tc, transpose_convert_gemm_lower=tt,
               transpose_convert_gemm_both_triangles=tf, transpose_convert_gemm_lower_plus_transposed_copy=tm,
               knm_gram_tflops=round(flop / (np.median(tg) * 1e-3) / 1e12, 2),
               convert_gemm_tflops=round(flop / (np.median(tc) * 1e-3) / 1e12, 2), max_rel_diff=diff)
        del K, G, G2, Kt, Kt64, Gt


def part_b(be, reps):
    for M in (2000, 10000):
        ld = (M + 1) // 2 * 2
        G = torch.randn((M, ld), dtype=torch.float64, device="cuda")
        C = torch.empty_like(G)
        X = torch.randn((2, ld), dtype=torch.float64, device="cuda")
        Y = torch.zeros((2, ld), dtype=torch.float64, device="cuda")

        def copy():
            C.copy_(G)

        def symv1():
            be.symv(G, X[:1], out=Y[:1])

        def symv2():
            be.symv(G, X, out=Y)

        tc, t1, t2 = alternate([copy, symv1, symv2], reps)
        nbytes = M * ld * 8.0
        rate = lambda t: nbytes / (np.median(t) * 1e-3) / 1e12       # noqa: E731
        # the copy moves the bytes twice (a read and a write); the product reads them once
        report("symvn", M=M, matrix_MB=round(nbytes / 1e6, 1), copy=tc, symv_nv1=t1, symv_nv2=t2,
               copy_TBps_read_plus_write=round(2 * rate(tc), 3), symv_nv1_TBps=round(rate(t1), 3), symv_nv2_TBps=round(rate(t2), 3),
               nv1_fraction_of_copy_rate=round(rate(t1) / (2 * rate(tc)), 3), nv2_fraction_of_copy_rate=round(rate(t2) / (2 * rate(tc)), 3))


def part_c(be, reps):
    from tests.synth import blob_problem
    n0, nb, M, D, sigma, lam = 20000, 512, 2000, 1024, 15.0, 1e-5
    X, y, _ = blob_problem(n0 + nb, D, seed=11)
    Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()[:, None]
    torch.manual_seed(0)
    Z = Xt[torch.randperm(n0)[:M].cuda()].contiguous()

    class Fixed:
        def select(self, Xs, Ys):
            return Z

    est = odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, centres=Z)
    est.partial_fit(Xt[:n0], Yt[:n0])

    def inc():
        est.partial_fit(Xt[n0:], Yt[n0:])
        torch.cuda.synchronize()

    def undo():
        est.remove(Xt[n0:], Yt[n0:], solve=False)

    def inc_nosolve():
        est.partial_fit(Xt[n0:], Yt[n0:], solve=False)

    def solve():
        est.solve()
        torch.cuda.synchronize()

    full = odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma), penalty=lam, M=M, center_selection=Fixed())

    def refit():
        full.fit(Xt, Yt)
        torch.cuda.synchronize()

    t_inc, t_add, t_solve, t_full = [], [], [], []
    inc(), undo(), refit()
    for _ in range(reps):
        t_inc += timed(inc, 1, warm=0)
        undo()
        t_add += timed(inc_nosolve, 1, warm=0)
        undo()
        t_solve += timed(solve, 1, warm=0)
        t_full += timed(refit, 1, warm=0)
    est.partial_fit(Xt[n0:], Yt[n0:])
    rel = float((est.alpha_ - full.alpha_).norm() / full.alpha_.norm())
    # partial_fit(batch) = solve + (add 512 rows) * batch / 512; the full fit grows by its K_nM work per row: taken from a
    # second size
    def refit_small():
        full.fit(Xt[:n0 // 2], Yt[:n0 // 2])
        torch.cuda.synchronize()
    t_half = timed(refit_small, reps, warm=1)
    per_row_inc = np.median(t_add) / nb
    per_row_full = (np.median(t_full) - np.median(t_half)) / (n0 + nb - n0 // 2)
    # rows r of a new batch from which a full refit on n0 + r rows is cheaper than partial_fit of r rows
    den = per_row_inc - per_row_full
    breakeven = None if den <= 0 else int(max(0.0, (np.median(t_full) - nb * per_row_full - np.median(t_solve)) / den))
    report("partial_fit", n_seen=n0, batch=nb, M=M, D=D, partial_fit=t_inc, add_rows_only=t_add, solve_only=t_solve,
           full_fit_all_rows=t_full, full_fit_half_rows=t_half, alpha_rel_diff=rel,
           add_us_per_row=round(1e3 * per_row_inc, 3), full_fit_us_per_row=round(1e3 * per_row_full, 3),
           breakeven_batch_rows=breakeven)


def part_d(be, reps):
    from odx.backend import Knm
    for M in (2048, 8192):
        K = Knm()
        K.M, K.ld = M, M
        K.n = n = (1 << 30) // (4 * M)                           # a 1 GiB f32 chunk
        K.K = torch.rand((n, M), dtype=torch.float32, device="cuda")
        w = torch.randn(n, dtype=torch.float64, device="cuda")
        Y = torch.randn((n, 64), dtype=torch.float64, device="cuda")
        y = Y[:, 0].contiguous()
        G = torch.zeros((M, M), dtype=torch.float64, device="cuda")
        b = torch.zeros(M, dtype=torch.float64, device="cuda")
        B = torch.zeros((64, M), dtype=torch.float64, device="cuda")
        nts = (1, 8, 32, 64)

        def one():
            be.knm_gram(K, w=w, y=y, beta=1.0, G=G, b=b)

        def multi(nt):
            return lambda: be.knm_gram_multi(K, w=w, Y=Y[:, :nt], beta=1.0, G=G, B=B[:nt])

        ts = alternate([one] + [multi(nt) for nt in nts], reps)
        tiles_m = (M + 127) // 128
        base = float(np.median(ts[0]))
        report("gram_rhsn", n=n, M=M, knm_gram_one_y=ts[0], expected_extra_percent=round(100.0 * tiles_m / (tiles_m * (tiles_m + 1)), 2),
               **{"rhsn_nt%d" % nt: t for nt, t in zip(nts, ts[1:])},
               **{"extra_percent_nt%d" % nt: round(100.0 * (float(np.median(t)) / base - 1.0), 2) for nt, t in zip(nts, ts[1:])})
        del K, G, B, Y, w


def _batch_problem(T, n=200000, D=1024, M=2048):
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    X = torch.randn((n, D), dtype=torch.float32, device="cuda", generator=g)
    Y = torch.where(torch.randn((n, T), dtype=torch.float64, device="cuda", generator=g) > 0, 1.0, -1.0)
    return X, Y, X[:M].contiguous()


def part_e(be, reps, T):
    sigma, lam = 30.0, 1e-5
    X, Y, Z = _batch_problem(T)
    multi = odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, centres=Z, outputs=T)
    ones = [odx.IncrementalFalkon(odx.GaussianKernel(sigma), lam, centres=Z) for _ in range(T)]

    def add_multi():
        multi.partial_fit(X, Y, decay=0.0, solve=False)
        torch.cuda.synchronize()

    def add_ones():
        for t, m in enumerate(ones):
            m.partial_fit(X, Y[:, t:t + 1], decay=0.0, solve=False)
        torch.cuda.synchronize()

    def solve_multi():
        multi.solve()
        torch.cuda.synchronize()

    def solve_ones():
        for m in ones:
            m.solve()
        torch.cuda.synchronize()

    ta, tb = alternate([add_multi, add_ones], reps)
    tc, td = alternate([solve_multi, solve_ones], reps)
    diff = max(float((multi.alpha_[:, t] - ones[t].alpha_[:, 0]).norm() / ones[t].alpha_.norm()) for t in range(T))
    report("partial_fit_outputs", T=T, rows=X.shape[0], D=X.shape[1], M=Z.shape[0], add_outputs_T=ta, add_T_one_output_models=tb,
           solve_outputs_T=tc, solve_T_one_output_models=td, add_speedup=round(float(np.median(tb) / np.median(ta)), 2),
           solve_speedup=round(float(np.median(td) / np.median(tc)), 2), max_alpha_rel_diff=diff)


def part_f(be, reps, T):
    sigma = 30.0
    pens = [10.0 ** -k for k in (2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5)]
    X, Y, Z = _batch_problem(T, n=50000)
    est = odx.IncrementalFalkon(odx.GaussianKernel(sigma), pens[0], centres=Z, outputs=T).partial_fit(X, Y, solve=False)

    def path():
        est.solve_path(pens)
        torch.cuda.synchronize()

    def loop():
        for p in pens:
            est.solve(penalty=p)
        torch.cuda.synchronize()

    tp, tl = alternate([path, loop], reps)
    report("solve_path", T=T, M=Z.shape[0], penalties=len(pens), solve_path=tp, solve_per_penalty=tl,
           speedup=round(float(np.median(tl) / np.median(tp)), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--outputs", default=None, help="T[,T...]: time the multi-output route (parts d, e, f) at these widths")
    a = ap.parse_args()
    be = odx.get_backend()
    if a.outputs is not None:
        part = a.part or "def"
        if "d" in part:
            part_d(be, a.reps)
        for T in [int(t) for t in a.outputs.split(",")]:
            if "e" in part:
                part_e(be, max(5, a.reps // 4), T)
            if "f" in part:
                part_f(be, max(5, a.reps // 4), T)
        return
    a.part = a.part or "abc"
    if "a" in a.part:
        part_a(be, a.reps)
    if "b" in a.part:
        part_b(be, a.reps)
    if "c" in a.part:
        part_c(be, max(5, a.reps // 3))


if __name__ == "__main__":
    main()
