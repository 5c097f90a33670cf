#!/usr/bin/env python3
"""Stand-alone times of the three passes the CG makes over one compact block (profiles/fold_rows.md), one process, HIP-event
times, the three alternating so that clock drift hits them alike:

  ktk       one vector, with t_out                  (odx_knm_fwd_bwd_q_t)
  ktk2      two vectors, with t_out                 (odx_knm_fwd_bwd2_q_t: the fold step without accumulated scores)
  ktk_rows  one vector and an n-long s, with t_out  (odx_knm_fwd_bwd_q_rows_t: the fold step over accumulated scores)

Usage: python tools/time_fold_rows.py [--n N] [--M M] [--reps R] [--tag TEXT]
Prints one JSON line per pass: median, min and max in ms and block bytes per median time."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    be = odx.get_backend()
    n, M = a.n, a.M
    K = random_u24_block(n, M)
    gb = n * K.ld * 3 / 1e9
    v1, v2 = (torch.randn(M, dtype=torch.float64, device="cuda") for _ in range(2))
    s, t = torch.randn(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    o1, o2 = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(2))
    runs = {"ktk": lambda: be.ktk(K, v=v1, out=o1, t_out=t)}
    if be.can_ktk2(K):
        runs["ktk2"] = lambda: be.ktk2(K, v1, v2, out1=o1, out2=o2, t_out=t)
    if be.can_ktk_rows(K):
        runs["ktk_rows"] = lambda: be.ktk_rows(K, v1, s, out1=o1, out2=o2, t_out=t)
    times = {k: [] for k in runs}
    for fn in runs.values():
        timed(fn, 0)
    for _ in range(a.reps):
        for k, fn in runs.items():
            times[k] += timed(fn, 1, warm=0)
    for k, ts in times.items():
        report(k, tag=a.tag, n=n, M=M, block_GB=round(gb, 2), time=ts, TBps=round(gb / float(np.median(ts)), 3))


if __name__ == "__main__":
    main()
