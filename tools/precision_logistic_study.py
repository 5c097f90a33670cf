"""CPU study: how the accuracy of the K_nM entries moves a logistic FALKON fit (odx/logistic.py, profiles/logistic_falkon.md).

The fit is tests/logistic_ref.py in numpy f64 throughout; only the block it iterates on changes:
  f64        the kernel evaluated in f64 (the reference of every other column)
  eval32     the kernel EVALUATED in f32 (what tests/oracle_backend.py does; stands in for the tile cores' entry error)
  f32        the f64 entries rounded to f32 (the f32 storage format)
  u24        the f64 entries rounded to 24-bit fixed point on [0, 1] (the compact storage format)
Columns: the relative distance of alpha and the largest absolute distance of the scores K alpha from the f64 column, and
whether the objective fell at every step.  Problems: tests/synth.blob_problem on the three shapes of
tests/test_gpu_incremental.py::SHAPES plus (2000, 256, 256) at sigma 10 and 25; schedules A, B, C; neg_weight 1 and 0.25.
Usage: python tools/precision_logistic_study.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))
from oracle import falkon_ref as fr  # noqa: E402
from tests import logistic_ref as lr  # noqa: E402
from tests.synth import blob_problem  # noqa: E402

SHAPES = [(777, 129, 36, 5.0), (1500, 257, 70, 5.0), (3000, 300, 1024, 15.0), (2000, 256, 256, 10.0), (2000, 256, 256, 25.0)]
SCHEDULES = {
    "A": [(1e-1, 3), (1e-2, 3), (1e-3, 3), (1e-4, 8), (1e-4, 8), (1e-4, 8)],
    "B": [(1e-2, 3), (1e-3, 3), (1e-4, 5), (1e-5, 8), (1e-5, 8)],
    "C": [(1e-3, 4), (1e-5, 4), (1e-6, 10), (1e-6, 10)],
}


def blocks(X, Z, sigma):
    K64 = fr.gaussian_kernel(X.astype(np.float64), Z.astype(np.float64), sigma, np.float64)
    return {"eval32": fr.gaussian_kernel(X, Z, sigma, np.float32).astype(np.float64),
            "f32": K64.astype(np.float32).astype(np.float64),
            "u24": np.minimum(np.rint(K64 * 16777216.0), 16777215.0) / 16777216.0}, K64


if __name__ == "__main__":
    print("%-22s %-3s %-5s | %-8s %-21s | %s" % ("n, M, D, sigma", "sch", "negw", "block", "alpha rel / score abs", "objective falls; max |f|"))
    worst = {}
    for n, M, D, sigma in SHAPES:
        X, y, rng = blob_problem(n, D, seed=500 + n)
        y = y.astype(np.float64)
        idx = np.sort(rng.choice(n, M, replace=False))
        Z = X[idx]
        variants, K64 = blocks(X, Z, sigma)
        for name, sched in SCHEDULES.items():
            pens, its = [p for p, _ in sched], [m for _, m in sched]
            for nw in (1.0, 0.25):
                obj = []
                ref = lr.logistic_fit(X, y, Z, y[idx], sigma, pens, its, nw, objective_out=obj)
                falls = all(b <= a for a, b in zip(obj, obj[1:]))
                fref = K64 @ ref
                for fmt, K in variants.items():
                    a = lr.logistic_fit(X, y, Z, y[idx], sigma, pens, its, nw, knm=K)
                    rel = float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
                    sc = float(np.abs(K @ a - fref).max())
                    worst[fmt] = (max(worst.get(fmt, (0, 0))[0], rel), max(worst.get(fmt, (0, 0))[1], sc))
                    print("%-22s %-3s %-5g | %-8s %.2e / %.2e   | %s; %.1f" % ("%d, %d, %d, %g" % (n, M, D, sigma), name, nw, fmt, rel, sc,
                                                                             falls, float(np.abs(fref).max())))
    for fmt, (rel, sc) in worst.items():
        print("worst %-7s alpha rel %.2e, score abs %.2e" % (fmt, rel, sc))
