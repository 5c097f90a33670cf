#!/usr/bin/env python3
"""Timings behind profiles/leverage_scores.md, on the GPU (device events around the calls, warmed up, fused and composed forms
alternating in one process):

  * odx_knm_rowquad_f64 at (n, M): device time, n M^2 flop per second, and its rate as a fraction of gemm_nt_kernel<double>'s
    at the same m, n, k with ODX_GEMM_B_LOWER (the same n M^2 flop, the product stored);
  * the composition of the existing entries it replaces: odx_convert_f32_f64 + odx_gemm_nt_f64 (B_LOWER) + square-and-sum
    (no exported entry sums squares of f64 rows: torch's (T * T).sum(1) stands for it, two more launches);
  * the wall time of one LeverageSelector.select at --select-n rows of --select-d features.

    python tools/time_leverage.py [--shapes 8192x512,65536x2048] [--reps 7] [--select-n 100000] [--select-d 1024]
                                  [--select-lam 1e-4] [--select-sigma 25] [--select-cap 4096] [--out FILE]
Prints one JSON line per measurement (and appends them to --out)."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "online-detection_amd"))
import torch  # noqa: E402

import odx  # noqa: E402
from odx import hip  # noqa: E402


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def time_shape(be, n, M, reps, out):
    lib, s = be.lib, be._stream()
    g = torch.Generator(device="cuda")
    g.manual_seed(n + M)
    ldk = (M + 3) // 4 * 4
    K = torch.rand((n, ldk), generator=g, device="cuda", dtype=torch.float32)
    Li = torch.tril(torch.randn((M, M), generator=g, device="cuda", dtype=torch.float64)) / M ** 0.5
    q = torch.empty(n, dtype=torch.float64, device="cuda")
    Kd = torch.empty((n, M), dtype=torch.float64, device="cuda")
    T = torch.empty((n, M), dtype=torch.float64, device="cuda")

    def fused():
        hip.check(lib.odx_knm_rowquad_f64(_p(K), ldk, n, M, _p(Li), M, _p(q), s), "odx_knm_rowquad_f64")

    def gemm():
        hip.check(lib.odx_gemm_nt_f64(_p(Kd), M, _p(Li), M, _p(T), M, n, M, M, 1.0, 0.0, hip.GEMM_B_LOWER, s), "odx_gemm_nt_f64")

    def composed():
        hip.check(lib.odx_convert_f32_f64(_p(K), ldk, _p(Kd), M, n, M, s), "odx_convert_f32_f64")
        gemm()
        return (T * T).sum(1)

    for _ in range(2):
        fused(), composed()
    torch.cuda.synchronize()
    q2 = composed()
    rel = float(((q - q2).abs() / q2.abs().clamp_min(1e-300)).max())
    tf, tc, tg = [], [], []
    for _ in range(reps):          # alternating: what else runs on the host moves all three alike
        tf.append(_timed(fused))
        tc.append(_timed(composed))
        tg.append(_timed(gemm))
    flop = float(n) * M * M
    mf, mc, mg = min(tf), min(tc), min(tg)
    emit({"what": "rowquad", "n": n, "M": M, "reps": reps, "fused_ms": mf, "fused_ms_all": tf, "fused_tflops": flop / mf * 1e-9,
          "gemm_b_lower_ms": mg, "gemm_tflops": flop / mg * 1e-9, "fused_over_gemm_rate": mg / mf,
          "composed_ms": mc, "composed_ms_all": tc, "composed_over_fused": mc / mf, "max_rel_diff_fused_vs_composed": rel}, out)


def time_select(be, n, D, lam, sigma, cap, out):
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    # blobs around 5 means, centred, mean norm 20 (the shape of tests/synth.blob_problem, made on the device)
    X = 0.7 * torch.randn((n, D), generator=g, device="cuda") + 0.6 * torch.randn((5, D), generator=g, device="cuda")[
        torch.randint(0, 5, (n,), generator=g, device="cuda")]
    X -= X.mean(0)
    X *= 20.0 / X.norm(dim=1).mean()
    sel = odx.LeverageSelector(odx.GaussianKernel(sigma), lam, cap, seed=0)
    walls = []
    for _ in range(2):             # the first call loads code objects and fills the allocator; the second is the figure
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sel.select(X, None)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    emit({"what": "select", "n": n, "D": D, "lam": lam, "sigma": sigma, "cap": cap, "wall_s_first": walls[0], "wall_s": walls[1],
          "centres": int(sel.indices_.numel()), "d_eff_estimate": sel.d_eff_,
          "levels": [[lv[0], lv[1], lv[2], lv[3], lv[4]] for lv in sel.levels_]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x512,65536x2048")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--select-n", type=int, default=100000)
    ap.add_argument("--select-d", type=int, default=1024)
    ap.add_argument("--select-lam", type=float, default=1e-4)
    ap.add_argument("--select-sigma", type=float, default=25.0)
    ap.add_argument("--select-cap", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = odx.get_backend()
    for shape in [s for s in a.shapes.split(",") if s]:
        n, M = (int(v) for v in shape.split("x"))
        time_shape(be, n, M, a.reps, a.out)
    if a.select_n > 0:
        time_select(be, a.select_n, a.select_d, a.select_lam, a.select_sigma, a.select_cap, a.out)


if __name__ == "__main__":
    main()
