#!/usr/bin/env python3
"""Timings of the multi-output fit (profiles/falkon_multi.md), one process, alternating A / B, HIP-event times:

  (a) odx_knm_bwdn_q over nv weight vectors against nv ktk(K, w=...) calls on the same u24 block
  (b) odx_trmvn_f64 over 8 vectors against 8 odx_trmv_f64 on the same factor, both uplo
  (c) falkon_fit_multi at T = 8 against 8 falkon_fit calls, with the split by phase

Usage: python tools/time_multi.py [--part a|b|c] [--n N] [--M M] [--D D] [--reps R] [--T T]
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


def report(what, **kw):
    for k, v in list(kw.items()):
        if isinstance(v, list):
            kw[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    print(json.dumps(dict(what=what, **kw)), flush=True)


def alternate(fa, fb, reps):
    """reps rounds of (A, B), so that drift of clocks and temperature hits both alike."""
    ta, tb = [], []
    timed(fa, 0), timed(fb, 0)
    for _ in range(reps):
        ta += timed(fa, 1, warm=0)
        tb += timed(fb, 1, warm=0)
    return ta, tb


def random_u24_block(n, M):
    """A u24 block with random entries, made on the device (its values do not matter for the time)."""
    from odx.backend import Knm
    K = Knm()
    K.n, K.M, K.ld, K.fmt = n, M, (M + 7) // 8 * 8, "u24"
    K.K = torch.randint(-32768, 32767, (n, K.ld), dtype=torch.int16, device="cuda")
    K.lo = torch.randint(0, 255, (n, K.ld), dtype=torch.uint8, device="cuda")
    return K


def part_a(be, n, M, reps):
    K = random_u24_block(n, M)
    ldw = (n + 1) // 2 * 2
    for nv in (2, 4, 8):
        W = torch.randn((nv, ldw), dtype=torch.float64, device="cuda")
        out = torch.zeros((nv, (M + 1) // 2 * 2), dtype=torch.float64, device="cuda")

        def grouped():
            be.ktwn(K, W, out=out)

        def loop():
            for q in range(nv):
                be.ktk(K, w=W[q, :n], out=out[q, :M])
        tg, tl = alternate(grouped, loop, reps)
        gb = n * K.ld * 3 / 1e9
        report("bwdn_q", n=n, M=M, nv=nv, block_GB=round(gb, 2), grouped=tg, loop=tl,
               grouped_TBps=round(gb / float(np.median(tg)), 3), loop_TBps=round(nv * gb / float(np.median(tl)), 3))


def part_b(be, M, reps):
    from odx.backend import Precond
    ld = (M + 1) // 2 * 2
    P = Precond()
    P.M, P.ld = M, ld
    P.LTi = torch.randn((M, ld), dtype=torch.float64, device="cuda")
    P.LTit = torch.randn((M, ld), dtype=torch.float64, device="cuda")
    X = torch.randn((8, ld), dtype=torch.float64, device="cuda")
    Z = torch.randn((8, ld), dtype=torch.float64, device="cuda")
    out = torch.zeros((8, ld), dtype=torch.float64, device="cuda")
    for name in ("LTi", "LTit"):
        def grouped():
            be.trmvn(P, name, X, alpha=0.5, beta=2.0, Z=Z, out=out)

        def loop():
            for q in range(8):
                be.trmv(P, name, X[q], alpha=0.5, beta=2.0, z=Z[q], out=out[q])
        tg, tl = alternate(grouped, loop, reps)
        report("trmvn", M=M, uplo=be._TRI[name], nv=8, factor_MB=round(M * M * 4 / 1e6, 1), grouped=tg, loop=tl)


class Phases:
    """HIP-event timers per phase name (solver's `phase` hook); triangular products and the rest are what remains."""

    def __init__(self):
        self.ev = {}

    def __call__(self, name):
        outer = self

        class _Ctx:
            def __enter__(self):
                self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                self.a.record()

            def __exit__(self, *exc):
                self.b.record()
                outer.ev.setdefault(name, []).append((self.a, self.b))
                return False
        return _Ctx()

    def totals(self):
        torch.cuda.synchronize()
        return {k: round(sum(a.elapsed_time(b) for a, b in v), 3) for k, v in self.ev.items()}


def part_c(be, n, M, D, T, reps):
    be.gauss, be.knm_storage = "h2", "u24"
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((n, D), generator=g, device="cuda", dtype=torch.float32)
    X *= 20.0 / X.norm(dim=1).mean()
    Y = torch.where(torch.randn((n, T), generator=g, device="cuda") > 0.8, 1.0, -1.0).double()
    F = be.features(X)
    Zf = be.rows(F, torch.randperm(n)[:M])
    sigma, lam = (10.0 if D <= 256 else 25.0), 1e-5

    def multi(ph=None):
        return odx.falkon_fit_multi(be, F, Y, Zf, sigma, lam, 20, phase=ph)

    def singles(ph=None):
        return [odx.falkon_fit(be, F, Y[:, t].contiguous(), Zf, sigma, lam, 20, phase=ph) for t in range(T)]
    tm, ts = alternate(multi, singles, reps)
    report("fit", n=n, M=M, D=D, T=T, multi=tm, singles=ts)
    for what, fn in (("multi", multi), ("singles", singles)):
        ph = Phases()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(ph)
        b.record()
        tot = ph.totals()
        whole = a.elapsed_time(b)
        tot["triangular_and_vector_ops"] = round(whole - sum(tot.values()), 3)
        report("fit_split", run=what, n=n, M=M, D=D, T=T, whole_ms=round(whole, 3), **tot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc")
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--M", type=int, default=2000)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--T", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    be = odx.get_backend()
    if "a" in a.part:
        part_a(be, a.n, a.M, a.reps)
    if "b" in a.part:
        part_b(be, a.M, a.reps)
    if "c" in a.part:
        part_c(be, a.n, a.M, a.D, a.T, a.reps)


if __name__ == "__main__":
    main()
