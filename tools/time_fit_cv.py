#!/usr/bin/env python3
"""Timings of the K-fold cross-validation of one penalty (profiles/cross_validation.md): ONE arm per process, HIP-event times
around whole calls, on the HBM-bound block of tests/test_gpu_falkon_multi.py::test_multi_on_an_hbm_bound_block (2e5 x 2000,
D = 256, 24-bit storage), five folds plus the fit on all rows = 6 conjugate-gradient states.

  --arm cv       odx.falkon_fit_cv: one block, one preconditioner, one 8-wide row-weighted read per iteration
  --arm singles  what there was before it: six odx.falkon_fit calls (the five training subsets, then all rows) and the scores
                 of every fold's held-out rows by be.mmv.  The row subsets are gathered BEFORE the timed window
  --arm multi    odx.falkon_fit_multi with six label columns: the same number of passes as --arm cv without row weights
                 and without the row products handed out, so the difference to cv is what those cost

Usage: python tools/time_fit_cv.py --arm cv|singles|multi [--n N] [--M M] [--D D] [--folds F] [--reps R]
Prints one JSON line: median, min and max of the repetitions in ms, and the reads of the block the arm's passes make."""
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
from tests.synth import blob_problem, centres      # noqa: E402


def timed(fn, reps, warm=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", required=True, choices=["cv", "singles", "multi"])
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--M", type=int, default=2000)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fit_cv: needs the GPU (a time taken elsewhere says nothing)")
    be = odx.get_backend()
    be.gauss, be.knm_storage = "h2", "u24"
    sigma, lam, iters = 10.0, 1e-5, 20
    X, y, rng = blob_problem(a.n, a.D, seed=77)
    idx = centres(y, a.M, rng)
    fold_of = odx.cv_folds(a.n, a.folds, seed=0)
    Xt = torch.from_numpy(X).cuda()
    F = be.features(Xt)
    Zf = be.rows(F, idx)
    yv = be.vec(y)
    S = a.folds + 1
    info = {}
    if a.arm == "cv":
        blocks = []
        odx.falkon_fit_cv(be, F, yv, Zf, sigma, [lam], fold_of, a.folds, iters, knm_blocks=blocks)
        K = blocks.pop()
        info = dict(fmt=K.fmt, ktkn_width=be.ktkn_width(K), reads_per_exchange=be.ktkn_rows_reads(K, S),
                    exchanges=iters + sum(1 for it in range(iters - 1) if (it + 1) % 10 == 0), reads_right_hand_sides=1)
        del K

        def fn():
            odx.falkon_fit_cv(be, F, yv, Zf, sigma, [lam], fold_of, a.folds, iters)
    elif a.arm == "multi":
        Y = yv[:, None].repeat(1, S).contiguous()
        g = torch.Generator(device="cuda").manual_seed(1)
        Y[:, 1:] *= torch.where(torch.rand((a.n, S - 1), generator=g, device="cuda") > 0.1, 1.0, -1.0).double()      # other labellings
        blocks = []
        odx.falkon_fit_multi(be, F, Y, Zf, sigma, lam, iters, knm_blocks=blocks)
        K = blocks.pop()
        info = dict(fmt=K.fmt, ktkn_width=be.ktkn_width(K), reads_per_exchange=be.ktkn_reads(K, S),
                    exchanges=iters + sum(1 for it in range(iters - 1) if (it + 1) % 10 == 0), reads_right_hand_sides=1)
        del K

        def fn():
            odx.falkon_fit_multi(be, F, Y, Zf, sigma, lam, iters)
    else:
        fo = fold_of.cuda()
        parts = []
        for f in range(a.folds):
            tr, te = (fo != f).nonzero()[:, 0], (fo == f).nonzero()[:, 0]
            parts.append((be.features(Xt[tr]), yv[tr].contiguous(), be.features(Xt[te])))
        info = dict(fits=S, builds=S, preconditioners=S, scoring_contractions=a.folds)

        def fn():
            for Ftr, ytr, Fte in parts:
                be.mmv(Fte, Zf, sigma, odx.falkon_fit(be, Ftr, ytr, Zf, sigma, lam, iters))
            odx.falkon_fit(be, F, yv, Zf, sigma, lam, iters)
    t = timed(fn, a.reps)
    print(json.dumps(dict(arm=a.arm, n=a.n, M=a.M, D=a.D, folds=a.folds, states=S, iterations=iters,
                          median_ms=round(float(np.median(t)), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3), reps=a.reps, **info)),
          flush=True)


if __name__ == "__main__":
    main()
