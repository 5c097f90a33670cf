"""Time the NV-vector pass of a lambda path (HipBackend.ktkn, odx_knm_fwd_bwdn_q) and odx.falkon_fit_path against L calls
of odx.falkon_fit, in one process.  HIP events, warm-up, median of --reps (>= 20 for the passes).

  pass   K'(K V) for NV vectors over a random 24-bit block of n x M (no build needed): ms, effective bytes/s of the block
         read once, and the ratio to NV single-vector passes over the same block
  fit    falkon_fit_path with L penalties on n x M, D features (24-bit storage) against L falkon_fit calls, same inputs

Prints one JSON line per measurement (and appends them to --out when given).
    python tools/time_path_pass.py pass --n 500000 --M 2000 --nv 1 2 4 8
    python tools/time_path_pass.py fit --n 500000 --M 2000 --D 256 --L 4 8
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "online-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def _random_block(be, n, M):
    from odx.backend import Knm
    K = Knm()
    K.n, K.M, K.fmt = n, M, "u24"
    K.ld = ld = int(be.lib.odx_knm_ld(M, 1))
    K.K = torch.randint(-32768, 32767, (n, ld), dtype=torch.int16, device=be.device)
    K.lo = torch.randint(0, 255, (n, ld), dtype=torch.uint8, device=be.device)
    if ld > M:
        K.K[:, M:] = 0
        K.lo[:, M:] = 0
    return K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pass", "fit"])
    ap.add_argument("--n", type=float, default=5e5)
    ap.add_argument("--M", type=float, default=2000)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--nv", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--L", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-single-fits", action="store_true", help="fit: time the path only (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import odx
    n, M = int(a.n), int(a.M)
    be = odx.get_backend()
    lines = []

    def emit(d):
        d.update(n=n, M=M)
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    if a.what == "pass":
        K = _random_block(be, n, M)
        block_bytes = 3 * n * K.ld
        Mp = (M + 1) // 2 * 2
        V = torch.randn((max(a.nv), Mp), dtype=torch.float64, device=be.device) * 1e-3
        out = torch.zeros_like(V)
        o1 = torch.empty(M, dtype=torch.float64, device=be.device)
        single, lo, hi = _time(lambda: be.ktk(K, v=V[0, :M], out=o1), a.reps)
        emit({"what": "pass", "nv": 1, "ms": single, "ms_min": lo, "ms_max": hi, "TBps": block_bytes / single / 1e9,
              "kernel": be.lib.odx_knm_pass_kernel_name(M, 1, 1).decode(), "width": be.ktkn_width(K)})
        for nv in a.nv:
            if nv == 1:
                continue
            reads = -(-nv // be.ktkn_width(K)) if nv > 2 or be.can_ktk2(K) else nv
            ms, lo, hi = _time(lambda: be.ktkn(K, V[:nv], out=out[:nv]), a.reps)
            emit({"what": "pass", "nv": nv, "ms": ms, "ms_min": lo, "ms_max": hi, "reads_of_K": reads,
                  "TBps_per_read": reads * block_bytes / ms / 1e9, "vs_nv_single_passes": ms / (nv * single)})
    else:
        import bench
        from odx.solver import SolverOptions
        be.gauss, be.knm_storage = "h2", "u24"
        X = bench.synth_rows(0, n, a.D, 30, 1234, be.device)
        idx = torch.from_numpy(bench.centre_indices(n, 30, M, 1234)[0]).to(be.device)
        F = be.features(X)
        Zf = be.rows(F, idx)
        y = torch.where((torch.arange(n, device=be.device) % 30) == 0, 1.0, -1.0).to(torch.float64)
        opt = SolverOptions(check_pivots=False)
        grid = [1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 3e-6, 3e-4]

        def wall(fn, reps):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts), ts

        for L in a.L:
            lams = grid[:L]
            path_ms, allp = wall(lambda: odx.falkon_fit_path(be, F, y, Zf, a.sigma, lams, 20, opt), max(3, a.reps // 4))
            d = {"what": "fit", "L": L, "D": a.D, "path_ms": path_ms, "path_ms_all": allp, "width": None}
            if not a.no_single_fits:
                single_ms, alls = wall(lambda: [odx.falkon_fit(be, F, y, Zf, a.sigma, lam, 20, opt) for lam in lams], max(3, a.reps // 4))
                d.update(single_fits_ms=single_ms, single_fits_ms_all=alls, path_vs_single_fits=path_ms / single_ms)
                al = odx.falkon_fit_path(be, F, y, Zf, a.sigma, lams, 20, opt)
                rel = [float((al[l] - s).norm() / s.norm()) for l, s in
                       enumerate(odx.falkon_fit(be, F, y, Zf, a.sigma, lam, 20, opt) for lam in lams)]
                d.update(alpha_rel_diff_max=max(rel))
            emit(d)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
