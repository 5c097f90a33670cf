#!/usr/bin/env python3
"""Timings of the shared-centre scoring route (profiles/mmv_shared.md), one process per shape, the two arms alternating,
HIP-event times:

  A  HipBackend.mmv with shared_mmv_min = None: one evaluation of K(X, Z) per column (odx_gauss_mmv_h2)
  B  the same call with the route forced (shared_mmv_min = 2): one evaluation per group of up to 8 columns (odx_gauss_mmvn_h2)

over T = 2, 4, 8, 16 columns of a dense V.

Usage: python tools/time_mmv_shared.py [--n N] [--M M] [--D D] [--tile 0|128|256] [--reps R] [--T 2,4,8,16]
Prints one JSON line per T: median, min and max of the repetitions in ms for both arms, and whether the results are equal."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "online-detection_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch            # noqa: E402

import odx              # noqa: E402
from time_multi import alternate, report      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=10000)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", default="2,4,8,16")
    a = ap.parse_args()
    be = odx.get_backend()
    be.gauss = "h2"
    be.pin_gauss_tile(a.tile)
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((a.n, a.D), generator=g, device="cuda", dtype=torch.float32)
    X *= 20.0 / X.norm(dim=1).mean()
    F = be.features(X)
    Zf = be.rows(F, torch.randperm(a.n)[:a.M])
    sigma = 10.0 if a.D <= 256 else 25.0
    for T in [int(t) for t in a.T.split(",")]:
        V = torch.randn((a.M, T), generator=g, device="cuda", dtype=torch.float64)
        out = torch.empty((a.n, T), dtype=torch.float32, device="cuda")

        def run(smin):
            be.shared_mmv_min = smin
            be.mmv(F, Zf, sigma, V, None, out=out)
        run(None)
        ref = out.clone()
        run(2)
        same = bool(torch.equal(ref, out))
        ta, tb = alternate(lambda: run(None), lambda: run(2), a.reps)
        report("mmv_shared", n=a.n, M=a.M, D=a.D, tile=a.tile, T=T, equal=same, per_column=ta, shared=tb)
    be.shared_mmv_min = None
    be.pin_gauss_tile(0)


if __name__ == "__main__":
    main()
