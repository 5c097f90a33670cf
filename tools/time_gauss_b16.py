#!/usr/bin/env python3
"""Timings of the Gaussian kernels on rows that are 16-bit already (profiles/b16_features.md), one process per shape, the two
arms alternating on the SAME bf16 / f16 rows, HIP-event times:

  A  HipBackend.native16 = False: the rows are converted to f32, packed as two-term f16 splits, and the split kernels run
     (odx_gauss_knm_h2_store / odx_gauss_mmv_h2 / odx_gauss_mmvn_h2: three MFMAs per product block and 32 features)
  B  HipBackend.native16 = True: the kernels read the 16-bit rows as they are (odx_gauss_knm_b16_store / odx_gauss_mmv_b16 /
     odx_gauss_mmvn_b16: two MFMAs per product block and 64 features, nothing packed)

per phase: `prepare` (features() of both matrices plus whatever the first Gaussian call adds: A converts and packs, B takes
the norms), `build` (K_nM in u24 with the fused right-hand side), `score1` (one column, the per-column kernel), `score8`
(eight dense columns, the shared-centre kernel).  Before timing, the two arms' results are compared on the same inputs.

Usage: python tools/time_gauss_b16.py [--n N] [--M M] [--D D] [--dtype bf16|f16] [--tile 0|128|256] [--reps R]
Prints one JSON line per phase: median, min and max of the repetitions in ms for both arms, and B's median over A's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "online-detection_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402

import odx              # noqa: E402
from time_multi import alternate, report      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=10000)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    be = odx.get_backend()
    be.gauss, be.knm_storage = "h2", "u24"
    be.pin_gauss_tile(a.tile)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn((a.n, a.D), generator=g, device="cuda", dtype=torch.float32)
    X *= 20.0 / X.norm(dim=1).mean()
    X16 = X.to(dt)
    del X
    Z16 = X16[torch.randperm(a.n, device="cuda")[:a.M]].contiguous()
    sigma = 10.0 if a.D <= 256 else 25.0
    w = torch.randn(a.n, generator=g, device="cuda", dtype=torch.float64) / a.n
    V1 = torch.randn((a.M, 1), generator=g, device="cuda", dtype=torch.float64)
    V8 = torch.randn((a.M, 8), generator=g, device="cuda", dtype=torch.float64)
    kbuf = torch.empty(be.knm_bytes(a.n, a.M) + 16, dtype=torch.uint8, device="cuda")
    out1 = torch.empty((a.n, 1), dtype=torch.float32, device="cuda")
    out8 = torch.empty((a.n, 8), dtype=torch.float32, device="cuda")
    shape = dict(n=a.n, M=a.M, D=a.D, dtype=a.dtype, tile=a.tile)

    def prepare(native):
        be.native16 = native
        F, Zf = be.features(X16), be.features(Z16)
        if not native:
            be.pack(F), be.pack(Zf)
        return F, Zf

    ops = {}
    for native in (False, True):
        F, Zf = prepare(native)
        assert F.b16 == native and (F.P is None) == native
        ops[native] = dict(F=F, Zf=Zf,
                           build=lambda F=F, Zf=Zf: be.knm_rhs(F, Zf, sigma, w, out=kbuf),
                           score1=lambda F=F, Zf=Zf: be.mmv(F, Zf, sigma, V1, None, out=out1),
                           score8=lambda F=F, Zf=Zf: be.mmv(F, Zf, sigma, V8, None, out=out8))
    # the two arms on the same inputs: the stored blocks (their first rows), K' w and the scores
    rows = min(a.n, 4096)
    res = {}
    for native in (False, True):
        K, b = ops[native]["build"]()
        assert K.fmt == "u24"
        ops[native]["score1"](), ops[native]["score8"]()
        res[native] = (K.rows(0, rows).dense().clone(), b.clone(), out1.clone(), out8.clone())
    (Ka, ba, s1a, s8a), (Kb, bb, s1b, s8b) = res[False], res[True]
    print(json.dumps(dict(what="b16_agreement", **shape, K_max_abs=float((Ka - Kb).abs().max()),
                          ktw_max_rel=float((ba - bb).abs().max() / ba.abs().max()),
                          score1_max_abs=float((s1a - s1b).abs().max()), score1_scale=float(s1a.abs().max()),
                          score8_max_abs=float((s8a - s8b).abs().max()), score8_scale=float(s8a.abs().max()))), flush=True)
    del res, Ka, Kb
    for phase in ("build", "score1", "score8"):
        ta, tb = alternate(ops[False][phase], ops[True][phase], a.reps)
        report("b16_" + phase, **shape, split=ta, native=tb, native_over_split=round(float(np.median(tb) / np.median(ta)), 4))
    ops.clear()
    del F, Zf
    ta, tb = alternate(lambda: prepare(False), lambda: prepare(True), a.reps)
    report("b16_prepare", **shape, split=ta, native=tb, native_over_split=round(float(np.median(tb) / np.median(ta)), 4))
    be.native16 = False
    be.pin_gauss_tile(0)


if __name__ == "__main__":
    main()
