#!/usr/bin/env python3
"""Times behind profiles/logistic_falkon.md, one process, HIP events.

Part A — the row-weighted product out = K' (d o (K v)) over an f32-format block, two routes alternating round by round so that
clock drift hits them alike:
  rw        one read   (odx_knm_fwd_bwd_rw: HipBackend.ktk_rw)
  two_call  two reads  (ktk(v, t_out), then ktk(w = d o t): ktkn_rows' "single" route, what the parent offers)
(a timed round is 10 calls back to back; the figures are per call) and their results compared at the sizes timed.

Part B — one LogisticFalkon.fit (schedule A) beside InCoreFalkon.fit at 20 iterations on the same rows and centres, the
logistic fit split into build, preconditioner steps, passes and row kernels by timers around the backend's methods.

Usage: python tools/time_logistic.py [--reps R] [--shapes n,M ...] [--fit n,M,D] [--tag TEXT]
Prints one JSON line per measurement."""
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
from time_multi import report, timed      # noqa: E402

SCHEDULE_A = [(1e-1, 3), (1e-2, 3), (1e-3, 3), (1e-4, 8), (1e-4, 8), (1e-4, 8)]


def random_f32_block(n, M):
    """An f32-format block with random entries in [0, 1), made on the device; columns [M, ld) zero."""
    from odx.backend import Knm
    K = Knm()
    K.n, K.M, K.ld, K.fmt = n, M, (M + 3) // 4 * 4, "f32"
    K.K = torch.rand((n, K.ld), dtype=torch.float32, device="cuda")
    K.K[:, M:] = 0.0
    return K


def part_a(be, n, M, reps, tag, inner=10):
    K = random_f32_block(n, M)
    v = torch.randn(M, dtype=torch.float64, device="cuda")
    d = torch.rand(n, dtype=torch.float64, device="cuda")
    t = torch.empty(n, dtype=torch.float64, device="cuda")
    o1, o2 = (torch.empty(M, dtype=torch.float64, device="cuda") for _ in range(2))

    def rw():
        for _ in range(inner):
            be.ktk_rw(K, v, d, out=o1, t_out=t)

    def two_call():
        for _ in range(inner):
            be.ktk(K, v=v, out=o2, t_out=t)
            be.ktk(K, w=d * t, out=o2)

    times = {"rw": [], "two_call": []}
    timed(rw, 0), timed(two_call, 0)
    for _ in range(reps):
        times["rw"] += [x / inner for x in timed(rw, 1, warm=0)]
        times["two_call"] += [x / inner for x in timed(two_call, 1, warm=0)]
    diff = float((o1 - o2).abs().max() / o2.abs().max())
    gb = n * K.ld * 4 / 1e9
    for k, ts in times.items():
        report(k, tag=tag, n=n, M=M, block_GB=round(gb, 3), time=ts, reads=1 if k == "rw" else 2)
    report("rw_vs_two_call", tag=tag, n=n, M=M, ratio_of_medians=round(float(np.median(times["rw"]) / np.median(times["two_call"])), 4),
           max_rel_diff=diff)


class _Timers:
    """HIP-event timers around methods of the backend, by group."""

    def __init__(self, be, groups):
        self.be, self.events, self.saved = be, {g: [] for g in groups}, {}
        for g, names in groups.items():
            for nm in names:
                self.saved[nm] = getattr(be, nm)
                setattr(be, nm, self._wrap(g, self.saved[nm]))

    def _wrap(self, g, fn):
        def call(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            self.events[g].append((e0, e1))
            return r
        return call

    def close(self):
        torch.cuda.synchronize()
        for nm in self.saved:
            delattr(self.be, nm)
        return {g: round(sum(a.elapsed_time(b) for a, b in ev), 3) for g, ev in self.events.items()}


def part_b(be, n, M, D, reps, tag):
    sys.path.insert(0, ROOT)
    from tests.synth import blob_problem
    X, y, rng = blob_problem(n, D, seed=77)
    idx = torch.from_numpy(np.sort(rng.choice(n, M, replace=False)))
    Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(y.astype(np.float64))

    class Pick:
        def select(self, Xs, Ys):
            i = idx.to(Xs.device)
            return Xs[i], (None if Ys is None else Ys[i])

    def logistic():
        return odx.LogisticFalkon(odx.GaussianKernel(15.0), [p for p, _ in SCHEDULE_A], [m for _, m in SCHEDULE_A],
                                  loss=odx.LogisticLoss(0.25), center_selection=Pick()).fit(Xt, yt)

    def squared():
        return odx.InCoreFalkon(odx.GaussianKernel(15.0), 1e-4, M, center_selection=Pick(), maxiter=20).fit(Xt, yt)

    tl, ts = [], []
    timed(logistic, 0), timed(squared, 0)
    for _ in range(reps):
        tl += timed(logistic, 1, warm=0)
        ts += timed(squared, 1, warm=0)
    report("logistic_fit", tag=tag, n=n, M=M, D=D, schedule="A", cg_iterations=sum(m for _, m in SCHEDULE_A), time=tl)
    report("incore_fit", tag=tag, n=n, M=M, D=D, cg_iterations=20, time=ts)
    tm = _Timers(be, {"build": ["knm_rhs"], "precond": ["precond_logistic_begin", "precond_logistic_step", "logistic_centre_scores"],
                      "passes": ["ktk_rw", "ktk"], "row_kernels": ["logistic_rows", "cg_scores_axpy"],
                      "triangular_and_cg": ["trmv", "cg_init", "cg_step", "cg_finish", "axpby"]})
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    logistic()
    e1.record()
    split = tm.close()
    report("logistic_fit_split_ms", tag=tag, n=n, M=M, D=D, whole=round(e0.elapsed_time(e1), 3), **split)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--shapes", nargs="*", default=["20000,2000", "65536,2000", "20000,5000", "26843,5000"])
    ap.add_argument("--fit", default="20000,2000,1024")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    be = odx.get_backend()
    for s in a.shapes:
        n, M = (int(x) for x in s.split(","))
        part_a(be, n, M, a.reps, a.tag)
    if a.fit:
        n, M, D = (int(x) for x in a.fit.split(","))
        part_b(be, n, M, D, max(5, a.reps // 3), a.tag)


if __name__ == "__main__":
    main()
