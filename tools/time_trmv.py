#!/usr/bin/env python3
"""The CG's triangular products alone (development aid): odx_trmv_f64 with a lower and an upper M x M factor, M = 1e4 (400 MB per
product): microseconds per launch and TB/s, and the product against numpy at M = 700.  Then the same bytes as a BLOCKED product
(odx_tri_blocked_mv_f64, the form a partial inverse of T is multiplied in) with one and two levels unmerged: 3 and 5 launches."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "online-detection_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import odx  # noqa: E402
from odx import hip  # noqa: E402
from odx.backend import _p  # noqa: E402

be = odx.get_backend()
for M in (700, 10000):
    ld = (M + 1) // 2 * 2
    g = torch.Generator(device="cuda").manual_seed(M)
    A = torch.randn((M, ld), generator=g, device="cuda", dtype=torch.float64)
    x = torch.randn(M, generator=g, device="cuda", dtype=torch.float64)
    y = torch.empty(M, device="cuda", dtype=torch.float64)
    for uplo, name in ((0, "lower"), (1, "upper")):
        def run():
            hip.check(be.lib.odx_trmv_f64(_p(A), ld, M, uplo, _p(x), 1.0, 0.0, None, _p(y), be._stream()), "odx_trmv_f64")
        run()
        torch.cuda.synchronize()
        if M == 700:
            a = A.cpu().numpy()[:, :M]
            want = (np.triu(a) if uplo else np.tril(a)) @ x.cpu().numpy()
            print(name, "max rel err", float(np.abs(y.cpu().numpy() - want).max() / np.abs(want).max()))
            continue
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(200):
                run()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / 200)
        print("M = %d %s: %.1f us per product, %.2f TB/s" % (M, name, best * 1e6, M * (M + 1) / 2 * 8 / best / 1e12))

M = 10000
ws = torch.empty(be.lib.odx_tri_blocked_mv_workspace_bytes(M), dtype=torch.uint8, device="cuda")
for bounds in ((0, 8192, M), (0, 4096, 8192, M)):
    arr = (ctypes.c_int64 * len(bounds))(*bounds)
    for uplo, name in ((0, "lower"), (1, "upper")):
        def run():
            hip.check(be.lib.odx_tri_blocked_mv_f64(_p(A), ld, M, uplo, arr, len(bounds) - 1, _p(x), 1.0, 0.0, None, _p(y), _p(ws),
                                                    ws.numel(), be._stream()), "odx_tri_blocked_mv_f64")
        run()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(200):
                run()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / 200)
        print("M = %d %s, blocks %s: %.1f us per product (%d launches), %.2f TB/s"
              % (M, name, bounds, best * 1e6, 2 * len(bounds) - 3, M * (M + 1) / 2 * 8 / best / 1e12))
