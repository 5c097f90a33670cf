"""Time one streamed CG pass (knm_storage "stream", odx_gauss_ktk_stream_h2) at a given (n, D, M), in one process, beside
the two things it is measured against:

  build      the stand-alone stored build gauss_knm_h2w256_kernel (odx_gauss_knm_h2_store, 24-bit) of the same shape — of
             min(n, --build-rows) rows, scaled to n when the whole block would not fit (config 5: 300 GB)
  compose    the same product from two Gaussian contractions: u = K v + w (gauss_mmv_h2, rows x centres), then K' u (the
             contraction with the roles swapped) — every entry computed twice
  stream     one streamed pass out = K'(K v + w) (each entry computed once, read back from the ring)
  job        (unless --no-job) the streamed passes inside a LockstepClassJob fitting --classes classes, where the
             preconditioner chains on the side streams share the chip and the Infinity Cache: ms per pass from HIP events
             around every pass ("ktk" phase; the fold's two-vector passes included)

  --nv N,..  instead of all of the above but the build: ktkn of N vectors on the streamed shard (odx_gauss_ktk_stream_h2n: one
             build of K, the vectors in groups over the resident chunk) beside the composition it replaces, ceil(N / 2) calls
             of the streamed ktk2 (a ktk for the odd one), alternating in one process, HIP events around each
  --fit L,.. instead: odx.falkon_fit_path of L penalties (decades down from 1e-3) under "stream", seconds per fit

Prints one JSON line per measurement (and writes them to --out when given).
    python tools/time_stream_pass.py --n 1000000 --D 1024 --M 10000
    python tools/time_stream_pass.py --n 5000000 --D 1024 --M 20000 --classes 1
    python tools/time_stream_pass.py --n 1000000 --D 1024 --M 10000 --nv 4,8,16 --out profiles/stream_path.jsonl
    python tools/time_stream_pass.py --n 1000000 --D 1024 --M 10000 --fit 4,8
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


def _time(fn, reps):
    """Median ms of `reps` calls of fn, each bracketed by HIP events on the current stream."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


class _Timer:
    """A phase context for LockstepClassJob.run: HIP events around every entry, summed at the end."""

    def __init__(self):
        self.pairs = []

    def __call__(self):
        return self

    def __enter__(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.pairs.append([e, None])
        return self

    def __exit__(self, *exc):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.pairs[-1][1] = e
        return False

    def ms(self):
        return [a.elapsed_time(b) for a, b in self.pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--M", type=float, default=1e4)
    ap.add_argument("--sigma", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build-rows", type=float, default=1e6)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--no-job", action="store_true")
    ap.add_argument("--no-compose", action="store_true")
    ap.add_argument("--nv", default="", help="comma-separated vector counts: time ktkn on the streamed shard beside ktk2 / ktk calls")
    ap.add_argument("--fit", default="", help="comma-separated path lengths: time falkon_fit_path under knm_storage 'stream'")
    ap.add_argument("--tag", default=None, help="copied into every line (which tree was measured)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import odx
    from odx import options
    n, D, M, C = int(a.n), a.D, int(a.M), 30
    be = odx.get_backend()
    dev = be.device
    lines = []

    def emit(d):
        d.update(n=n, D=D, M=M)
        if a.tag:
            d["tag"] = a.tag
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    X = bench.synth_rows(0, n, D, C, 1234, dev)
    cidx = [torch.from_numpy(i).to(dev) for i in bench.centre_indices(n, C, M, 1234)]
    F = be.features(X)
    Zf = be.rows(F, cidx[0])
    be.pack(F), be.pack(Zf)
    g = torch.Generator(device="cpu").manual_seed(0)
    v = torch.randn(M, generator=g, dtype=torch.float64).to(dev) * 1e-3
    w = torch.randn(n, generator=g, dtype=torch.float64).to(dev) / n
    R = int(be.lib.odx_gauss_ktk_stream_h2_rows(M, D))
    ring_bytes = int(be.lib.odx_gauss_ktk_stream_h2_workspace_bytes(n, M, D))
    emit({"what": "ring", "rows": R, "chunks": (n + R - 1) // R, "workspace_bytes": ring_bytes})

    def finish():
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if a.fit:
        y = torch.where((torch.arange(n, device=dev) % C) == 0, 1.0, -1.0).to(torch.float64)
        with options.override(knm_storage="stream"):
            for L in [int(x) for x in a.fit.split(",")]:
                lams = [10.0 ** (-3 - 0.5 * i) for i in range(L)]

                def fit():
                    odx.falkon_fit_path(be, F, y, Zf, a.sigma, lams, 20)
                fit()                                            # warm-up: workspaces, kernel load
                torch.cuda.synchronize()
                ms, every = _time(fit, a.reps)
                emit({"what": "fit_path", "L": L, "s": ms / 1e3, "s_all": [x / 1e3 for x in every]})
        finish()
        return

    # stand-alone stored build of the same shape (scaled from a row slice when the block does not fit)
    rows = min(n, int(a.build_rows))
    Fs = F if rows == n else be.rows(F, torch.arange(rows, device=dev))
    be.pack(Fs)
    holder = {}

    def build():
        holder["K"] = None
        holder["K"] = be._knm_store(Fs, Zf, a.sigma, "u24", None, None, None)[0]
    build_ms, all_build = _time(build, a.reps)
    holder.clear()
    del Fs
    torch.cuda.empty_cache()
    emit({"what": "build", "ms": build_ms * n / rows, "rows_timed": rows, "ms_timed": all_build})

    if a.nv:
        Mp = (M + 1) // 2 * 2
        with options.override(knm_storage="stream"):
            S, _ = be.knm_rhs(F, Zf, a.sigma, w)
            Rn = int(be.lib.odx_gauss_ktk_stream_h2n_rows(M, D))
            for nv in [int(x) for x in a.nv.split(",")]:
                V = torch.randn((nv, Mp), generator=g, dtype=torch.float64).to(dev) * 1e-3
                O, O2 = torch.zeros_like(V), torch.zeros_like(V)

                def parent():
                    for q in range(0, nv - 1, 2):
                        be.ktk2(S, V[q, :M], V[q + 1, :M], out1=O2[q, :M], out2=O2[q + 1, :M])
                    if nv % 2:
                        be.ktk(S, v=V[nv - 1, :M], out=O2[nv - 1, :M])

                def new():
                    be.ktkn(S, V, out=O)
                parent(), new()                                  # warm-up
                torch.cuda.synchronize()
                tp, tn = [], []
                for _ in range(a.reps):                          # alternating: drift hits both alike
                    tp.append(_time(parent, 1)[0])
                    tn.append(_time(new, 1)[0])
                mp, mn = statistics.median(tp), statistics.median(tn)
                err = float((O - O2).abs().max() / O2.abs().max())
                emit({"what": "ktkn_stream", "nv": nv, "rows": Rn, "chunks": (n + Rn - 1) // Rn, "ms": mn, "ms_all": tn,
                      "parent_ms": mp, "parent_ms_all": tp, "vs_parent": mn / mp, "vs_build": mn / (build_ms * n / rows),
                      "max_rel_diff": err})
        finish()
        return

    with options.override(knm_storage="stream"):
        S, _ = be.knm_rhs(F, Zf, a.sigma, w)
        out = torch.empty(M, dtype=torch.float64, device=dev)
        stream_ms, all_stream = _time(lambda: be.ktk(S, v=v, w=w, out=out), a.reps)
        o1, o2 = torch.empty_like(out), torch.empty_like(out)
        two_ms, _ = _time(lambda: be.ktk2(S, v, v, out1=o1, out2=o2), max(1, a.reps // 2))
    emit({"what": "stream", "ms": stream_ms, "ms_all": all_stream, "ms_two_vectors": two_ms,
          "vs_build": stream_ms / (build_ms * n / rows)})

    if not a.no_compose:
        u = torch.empty((n, 1), dtype=torch.float32, device=dev)
        c = torch.empty((M, 1), dtype=torch.float32, device=dev)

        def compose():
            be.mmv(F, Zf, a.sigma, v, out=u)                  # K v (+ w: a vector add, not timed separately)
            be.mmv(Zf, F, a.sigma, u[:, 0].double() + w, out=c)
        comp_ms, all_comp = _time(compose, max(1, a.reps // 2))
        emit({"what": "compose", "ms": comp_ms, "ms_all": all_comp, "stream_vs_compose": stream_ms / comp_ms})
        del u, c
    be.release_workspaces()
    torch.cuda.empty_cache()

    if not a.no_job:
        from odx.job import LockstepClassJob
        from odx.solver import SolverOptions
        row_ids = torch.arange(n, device=dev)
        labels = lambda k: torch.where((row_ids % C) == k, 1.0, -1.0).to(torch.float64)       # noqa: E731
        with options.override(knm_storage="stream"):
            job = LockstepClassJob(be, X, n, M, labels, cidx[:a.classes], a.sigma, 1e-5, 20, SolverOptions(check_pivots=False),
                                   classes=a.classes)
            timers = {k: _Timer() for k in ("precond", "knm", "ktk", "ktk2", "mmv")}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            job.run(F, list(range(a.classes)), phases={k: t for k, t in timers.items()})
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        passes = timers["ktk"].ms() + timers["ktk2"].ms()
        emit({"what": "job", "classes": a.classes, "s_per_class": wall / a.classes, "passes": len(passes) + len(timers["knm"].ms()),
              "ms_per_pass_median": statistics.median(passes), "ms_knm_rhs_pass": statistics.median(timers["knm"].ms()),
              "ms_two_vector_pass": statistics.median(timers["ktk2"].ms()) if timers["ktk2"].ms() else None,
              "ms_score_mmv": statistics.median(timers["mmv"].ms()) if timers["mmv"].ms() else None})
    finish()


if __name__ == "__main__":
    main()
