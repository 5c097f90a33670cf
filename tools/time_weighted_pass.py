#!/usr/bin/env python3
"""Times behind profiles/weighted_falkon.md, one process, HIP events.

Part A — the row-weighted product out = K' (d o (K v)) over a 24-bit block, three routes alternating round by round so that
clock drift hits them alike:
  q_rw      one read   (odx_knm_fwd_bwd_q_rw: HipBackend.ktk_w with rw_q_min_columns = 1)
  ktk_rw    what the parent offers (HipBackend.ktk_rw: one read up to M = 5084 — odx_knm_fwd_bwdn_q_rw —, above it
            odx_knm_fwdn_q + odx_knm_bwdn_q, two reads)
  plain     the unweighted pass of the same block (odx_knm_fwd_bwd_q_t: HipBackend.ktk), the ceiling
A timed round is `inner` calls back to back; the figures are per call.  Beside median, min and max every route reports its
run-to-run spread, the 10th to 90th percentile width of its rounds, and the routing rule's verdict: q_rw wins a width when
its median is below ktk_rw's by more than three times the larger of the two spreads.  The results of the two weighted
routes are compared at the sizes timed.

Part B — one odx.falkon_fit_weighted (the new entry on, then off) beside odx.falkon_fit on the same rows and centres.

Usage: python tools/time_weighted_pass.py [--reps R] [--shapes n,M ...] [--fit n,M,D] [--tag TEXT]
Prints one JSON line per measurement."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "online-detection_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402

import odx              # noqa: E402
from time_multi import random_u24_block, report, timed      # noqa: E402


def spread(ts):
    return float(np.percentile(ts, 90) - np.percentile(ts, 10))


def part_a(be, n, M, reps, tag, inner=5):
    K = random_u24_block(n, M)
    K.K[:, M:] = 0          # (the pad as the builds leave it: the older passes read it)
    K.lo[:, M:] = 0
    v = torch.randn(M, dtype=torch.float64, device="cuda")
    d = torch.rand(n, dtype=torch.float64, device="cuda")
    t = torch.empty(n, dtype=torch.float64, device="cuda")
    o1, o2, o3 = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(3))

    def q_rw():
        be.rw_q_min_columns = 1
        for _ in range(inner):
            be.ktk_w(K, v, d, out=o1, t_out=t)

    def ktk_rw():
        for _ in range(inner):
            be.ktk_rw(K, v, d, out=o2, t_out=t)

    def plain():
        for _ in range(inner):
            be.ktk(K, v=v, out=o3, t_out=t)

    routes = {"q_rw": q_rw, "ktk_rw": ktk_rw, "plain": plain}
    times = {k: [] for k in routes}
    old = be.rw_q_min_columns
    try:
        for f in routes.values():
            timed(f, 0)
        for _ in range(reps):
            for k, f in routes.items():
                times[k] += [x / inner for x in timed(f, 1, warm=0)]
    finally:
        be.rw_q_min_columns = old
    diff = float((o1 - o2).abs().max() / o2.abs().max())
    gb = n * K.ld * 3 / 1e9
    reads = {"q_rw": 1, "ktk_rw": 1 if M <= 5084 else 2, "plain": 1}
    for k, ts in times.items():
        report(k, tag=tag, n=n, M=M, block_GB=round(gb, 3), time=ts, spread_ms=round(spread(ts), 4), reads=reads[k],
               TB_per_s=round(reads[k] * gb / float(np.median(ts)), 3))
    new, ref = float(np.median(times["q_rw"])), float(np.median(times["ktk_rw"]))
    margin = 3.0 * max(spread(times["q_rw"]), spread(times["ktk_rw"]))
    report("q_rw_vs_ktk_rw", tag=tag, n=n, M=M, ratio_of_medians=round(new / ref, 4), gain_ms=round(ref - new, 4),
           three_spreads_ms=round(margin, 4), q_rw_wins=bool(ref - new > margin), max_rel_diff=diff,
           q_rw_over_plain=round(new / float(np.median(times["plain"])), 4))


def part_b(be, n, M, D, reps, tag):
    from tests.synth import blob_problem
    X, y, rng = blob_problem(n, D, seed=77)
    idx = torch.from_numpy(np.sort(rng.choice(n, M, replace=False)))
    w = np.where(y > 0, 9.0, 1.0) * rng.uniform(0.5, 1.5, n)
    F = be.features(torch.from_numpy(X).cuda())
    Zf = be.rows(F, idx)
    yv, wv = be.vec(y.astype(np.float64)), be.vec(w)
    wz = wv[idx.cuda()].contiguous()
    sigma, lam = 15.0, 1e-4
    fmts = []

    def weighted(minimum):
        def run():
            old, be.rw_q_min_columns = be.rw_q_min_columns, minimum
            try:
                Ks = []
                a = odx.falkon_fit_weighted(be, F, yv, wv, Zf, wz, sigma, lam, 20, knm_blocks=Ks)
                fmts.append(Ks[0].fmt)
                return a
            finally:
                be.rw_q_min_columns = old
        return run

    def squared():
        return odx.falkon_fit(be, F, yv, Zf, sigma, lam, 20)

    routes = {"weighted_fit_q_rw": weighted(5085), "weighted_fit_entry_off": weighted(None), "falkon_fit": squared}
    times = {k: [] for k in routes}
    for f in routes.values():
        timed(f, 0)
    for _ in range(reps):
        for k, f in routes.items():
            times[k] += timed(f, 1, warm=0)
    a1, a2 = routes["weighted_fit_q_rw"](), routes["weighted_fit_entry_off"]()
    for k, ts in times.items():
        report(k, tag=tag, n=n, M=M, D=D, fmt=fmts[0], cg_iterations=20, time=ts, spread_ms=round(spread(ts), 4))
    report("weighted_fit_alpha", tag=tag, n=n, M=M, D=D, rel_diff_entry_on_off=float((a1 - a2).norm() / a2.norm()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--shapes", nargs="*", default=["200000,5200", "200000,8192", "100000,10000", "100000,12288", "50000,20000",
                                                     "500000,2000", "200000,5000"])
    ap.add_argument("--fit", default="200000,8192,256")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    be = odx.get_backend()
    for s in a.shapes:
        n, M = (int(x) for x in s.split(","))
        part_a(be, n, M, a.reps, a.tag)
        torch.cuda.empty_cache()
    if a.fit:
        n, M, D = (int(x) for x in a.fit.split(","))
        part_b(be, n, M, D, max(5, a.reps // 3), a.tag)


if __name__ == "__main__":
    main()
