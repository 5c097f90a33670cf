#!/usr/bin/env python3
"""Timings of the (sigma, lambda) grid (profiles/sigma_grid.md), one process per shape, the two arms alternating, HIP-event
times:

  build   odx_gauss_knm_h2_store_sigmas for S = 1 .. 4 widths (HipBackend.knm_rhs_sigmas, one contraction) against S calls of
          odx_gauss_knm_h2_store (HipBackend.knm_rhs), u24 blocks with the fused right-hand side, preallocated buffers
  score   odx_gauss_mmvn_h2_sigmas at T = 8, 16, 32 columns with 1, 2 and 4 distinct widths (HipBackend.mmv_sigmas) against
          odx_gauss_mmvn_h2 on the same operands (HipBackend.mmv, one width): the cost of the exps per column
  grid    a 4 x 4 grid: odx.falkon_fit_grid + one mmv_sigmas over the 16 alphas on held-out rows (what odx.predict_grid calls)
          against four odx.falkon_fit_path + four dense mmv of 4 columns (what odx.predict_path calls), rows and centres
          shared by both arms

Usage: python tools/time_sigma_grid.py [--part build|score|grid|all] [--n N] [--M M] [--D D] [--reps R]
Prints one JSON line per measurement: median, min and max of the repetitions in ms for both arms, and whether the two arms'
results are bit for bit equal."""
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

WIDTHS = [5.0, 10.0, 15.0, 25.0]
LAMS = [1e-3, 1e-4, 1e-5, 1e-6]


def part_build(be, F, Zf, y, a):
    n, M = F.n, Zf.n
    w = y / n
    nbytes = be.knm_bytes(n, M)
    bufs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(4)]
    shipped, be.sigma_grid_min_features = be.sigma_grid_min_features, 0          # the entry itself, whatever the routing rule says
    for S in (1, 2, 3, 4):
        sig = WIDTHS[:S]

        def loop():
            return [be.knm_rhs(F, Zf, s, w, out=bufs[i]) for i, s in enumerate(sig)]

        def entry():                          # (the call knm_rhs_sigmas makes for a group of two or more widths)
            return be._knm_store_sigmas(F, Zf, sig, "u24", w, bufs[:S])
        ref = [(K.K.clone(), K.lo.clone(), b.clone()) for K, b in loop()]
        got = entry()
        same = all(torch.equal(K.K, r[0]) and torch.equal(K.lo, r[1]) and torch.equal(b, r[2]) for (K, b), r in zip(got, ref))
        del ref, got
        ta, tb = alternate(loop, entry, a.reps)
        report("sigma_grid_build", n=n, M=M, D=F.D, fmt="u24", S=S, equal=same, single_builds=ta, one_contraction=tb)
    be.sigma_grid_min_features = shipped


def part_score(be, F, Zf, a, g):
    n, M = F.n, Zf.n
    for T in (8, 16, 32):
        V = torch.randn((M, T), generator=g, device="cuda", dtype=torch.float64)
        out = torch.empty((n, T), dtype=torch.float32, device="cuda")
        be.mmv(F, Zf, WIDTHS[1], V, None, out=out)
        ref = out.clone()
        for distinct in (1, 2, 4):
            sig = [WIDTHS[(1 + c) % distinct if distinct > 1 else 1] for c in range(T)]
            be.mmv_sigmas(F, Zf, sig, V, out=out)
            same = bool(torch.equal(out, ref)) if distinct == 1 else None
            ta, tb = alternate(lambda: be.mmv(F, Zf, WIDTHS[1], V, None, out=out), lambda: be.mmv_sigmas(F, Zf, sig, V, out=out), a.reps)
            report("sigma_grid_score", n=n, M=M, D=F.D, T=T, distinct=distinct, equal=same, one_width=ta, width_per_column=tb)


def part_grid(be, F, Zf, y, Fval, a):
    S, L = len(WIDTHS), len(LAMS)
    cols = [WIDTHS[s] for s in range(S) for _ in range(L)]
    res = {}

    def loop():
        alphas = [odx.falkon_fit_path(be, F, y, Zf, s, LAMS, 20) for s in WIDTHS]
        scores = [be.mmv(Fval, Zf, s, al.t().contiguous(), None) for s, al in zip(WIDTHS, alphas)]
        res["loop"] = (torch.stack(alphas), torch.cat(scores, dim=1))

    def grid():
        alphas = odx.falkon_fit_grid(be, F, y, Zf, WIDTHS, LAMS, 20)
        scores = be.mmv_sigmas(Fval, Zf, cols, alphas.reshape(S * L, -1).t().contiguous())
        res["grid"] = (alphas, scores)
    loop(), grid()
    same_alpha = bool(torch.equal(res["loop"][0], res["grid"][0]))
    # (the loop arm scores 4 columns per call, the grid arm 16: the tile core and the groups are chosen per call, so the scores
    # are compared to f32 rounding, not bit for bit)
    diff = float((res["loop"][1] - res["grid"][1]).abs().max())
    shipped = be.sigma_grid_min_features
    for least in (shipped, 0):                # the routing as shipped, then with the shared contraction forced
        be.sigma_grid_min_features = least
        ta, tb = alternate(loop, grid, a.reps)
        report("sigma_grid_whole", n=F.n, M=Zf.n, D=F.D, n_val=Fval.n, sigmas=S, lams=L, fmt=be.knm_format(F.n, Zf.n),
               min_features=least, shared_contraction=bool(least is not None and F.D >= least), alphas_equal=same_alpha,
               max_score_diff=diff, four_paths=ta, one_grid=tb)
    be.sigma_grid_min_features = shipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=("build", "score", "grid", "all"))
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--M", type=int, default=2000)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    be = odx.get_backend()
    be.gauss, be.knm_storage = "h2", "u24"
    g = torch.Generator(device="cuda").manual_seed(1)
    n_val = a.n // 10
    from tests.synth import blob_problem, centres       # the generator of the suite's fits (tests/test_gpu_falkon_path.py)
    Xh, yh, rng = blob_problem(a.n + n_val, a.D, seed=77)
    idx = centres(yh[:a.n], a.M, rng)
    X = torch.from_numpy(Xh).cuda()
    y = be.vec(yh[:a.n])
    F, Fval = be.features(X[:a.n]), be.features(X[a.n:])
    Zf = be.rows(F, idx)
    if a.part in ("build", "all"):
        part_build(be, F, Zf, y, a)
    if a.part in ("score", "all"):
        part_score(be, F, Zf, a, g)
    if a.part in ("grid", "all"):
        part_grid(be, F, Zf, y, Fval, a)


if __name__ == "__main__":
    main()
