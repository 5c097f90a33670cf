#!/usr/bin/env python3
"""Timings of the two-read route of HipBackend.ktkn above M = 5084 (profiles/wide_pass.md), one process, alternating A / B,
HIP-event times:

  (a) odx_knm_fwdn_q (HipBackend.kvn) alone over nv = 2, 4, 8 vectors on a u24 block, with block bytes per time
  (b) ktkn over L = 3 .. 8 vectors with the route on (wide_pass_min = 3) and off (None: pairs and singles)
  (c) falkon_fit_multi at T = 8, route on and off
  (d) falkon_fit_path at L = 8, route on and off

Usage: python tools/time_wide_pass.py [--part a|b|c|d] [--n N] [--M M] [--D D] [--reps R]
Prints one JSON line per measurement: median, min and max of the repetitions in ms.  One part and shape per process is the
intended use (each under its own time limit)."""
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
from time_multi import alternate, random_u24_block, report, timed      # noqa: E402


def part_a(be, n, M, reps):
    K = random_u24_block(n, M)
    gb = n * K.ld * 3 / 1e9
    for nv in (2, 4, 8):
        V = torch.randn((nv, (M + 1) // 2 * 2), dtype=torch.float64, device="cuda")
        out = torch.zeros((nv, (n + 1) // 2 * 2), dtype=torch.float64, device="cuda")
        t = timed(lambda: be.kvn(K, V, out=out), reps)
        report("fwdn_q", n=n, M=M, nv=nv, block_GB=round(gb, 2), time=t, TBps=round(gb / float(np.median(t)), 3))


def part_b(be, n, M, reps):
    K = random_u24_block(n, M)
    ld = (M + 1) // 2 * 2
    for L in range(3, 9):
        V = torch.randn((L, ld), dtype=torch.float64, device="cuda")
        out = torch.zeros((L, ld), dtype=torch.float64, device="cuda")

        def run(wmin):
            be.wide_pass_min = wmin
            be.ktkn(K, V, out=out)
        be.wide_pass_min = 3
        ron = be.ktkn_reads(K, L)
        be.wide_pass_min = None
        roff = be.ktkn_reads(K, L)
        ta, tb = alternate(lambda: run(3), lambda: run(None), reps)
        report("ktkn", n=n, M=M, L=L, reads_on=ron, reads_off=roff, route_on=ta, route_off=tb)


def _problem(be, n, M, D, T):
    be.gauss, be.knm_storage = "h2", "u24"
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, D), generator=g, device="cuda", dtype=torch.float32)
    X *= 20.0 / X.norm(dim=1).mean()
    Y = torch.where(torch.randn((n, T), generator=g, device="cuda") > 0.8, 1.0, -1.0).double()
    F = be.features(X)
    Zf = be.rows(F, torch.randperm(n)[:M])
    return F, Y, Zf, (10.0 if D <= 256 else 25.0)


def part_c(be, n, M, D, reps):
    F, Y, Zf, sigma = _problem(be, n, M, D, 8)

    def run(wmin):
        be.wide_pass_min = wmin
        return odx.falkon_fit_multi(be, F, Y, Zf, sigma, 1e-5, 20)
    ta, tb = alternate(lambda: run(3), lambda: run(None), reps)
    report("fit_multi", n=n, M=M, D=D, T=8, route_on=ta, route_off=tb)


def part_d(be, n, M, D, reps):
    F, Y, Zf, sigma = _problem(be, n, M, D, 1)
    y = Y[:, 0].contiguous()
    lams = [float(x) for x in np.logspace(-7, -3, 8)]

    def run(wmin):
        be.wide_pass_min = wmin
        return odx.falkon_fit_path(be, F, y, Zf, sigma, lams, 20)
    ta, tb = alternate(lambda: run(3), lambda: run(None), reps)
    report("fit_path", n=n, M=M, D=D, L=8, route_on=ta, route_off=tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab")
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--M", type=int, default=6000)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    be = odx.get_backend()
    if "a" in a.part:
        part_a(be, a.n, a.M, a.reps)
    if "b" in a.part:
        part_b(be, a.n, a.M, a.reps)
    if "c" in a.part:
        part_c(be, a.n, a.M, a.D, a.reps)
    if "d" in a.part:
        part_d(be, a.n, a.M, a.D, a.reps)


if __name__ == "__main__":
    main()
