"""A lambda path over streamed shards without a GPU: solver.falkon_fit_path on an oracle backend whose K_nM is never stored
and whose ktkn makes one counted build per group of ktkn_span rows.  With 2 L <= span the periodic full residual is folded
into the step's ktkn (one build per CG iteration); otherwise, and on stored blocks, the plain form stays."""
import threading

import numpy as np
import pytest
import torch

import odx
from oracle import falkon_ref as fr
from tests.oracle_backend import OracleBackend
from tests.test_falkon_path_host import LAMS, CountingBackend, _problem
from tests.test_knm_stream_host import StreamOracleBackend


class StreamPathBackend(StreamOracleBackend):
    """StreamOracleBackend with the multi-vector pass of a streamed shard: ONE build of K per group of ktkn_span rows."""
    span = 16

    def __init__(self):
        super().__init__()
        self.ktkn_rows = []              # rows of every ktkn call

    def ktkn_span(self, K):
        return self.span

    def ktkn(self, K, V, out=None):
        assert K.fmt == "stream"
        L, M = V.shape[0], K.M
        self.ktkn_rows.append(L)
        if out is None:
            out = torch.zeros((L, V.shape[1]), dtype=torch.float64)
        for l in range(0, L, self.span):
            self.passes += 1
            blk = self._build(K)         # one build serves the whole group
            for j in range(l, min(l + self.span, L)):
                OracleBackend.ktk(self, blk, v=V[j, :M], out=out[j, :M])
        return out


def _path(be, X, y, idx, lams, maxiter=20, sigma=10.0, **kw):
    F = be.features(torch.from_numpy(X))
    return odx.falkon_fit_path(be, F, be.vec(y), be.rows(F, idx), sigma, lams, maxiter, **kw)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_one_build_per_iteration_and_the_oracle_alphas():
    """L = 3, 20 iterations, full residual every 10: 1 build for the right-hand side + 20, the full residual at iteration 10
    folded into that iteration's ktkn (6 rows); the alphas against oracle.falkon_ref.falkon_fit at 1e-6 relative, the bound
    test_path_rows_equal_the_oracle_at_every_lambda holds the plain form to.  The folded form against the plain form on this
    problem is printed (f64 rounding that 20 steps on an ill-conditioned system do not contract)."""
    X, y, idx = _problem()
    lams = LAMS[:3]
    be = StreamPathBackend()
    alphas = _path(be, X, y, idx, lams)
    print("builds %d, ktkn rows %r" % (be.builds, be.ktkn_rows))
    plain = _path(OracleBackend(np.float64), X, y, idx, lams)
    for l, lam in enumerate(lams):
        ref, _ = fr.falkon_fit(X.astype(np.float64), y, idx, 10.0, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        rel = _rel(alphas[l].numpy(), ref[:, 0])
        print("lam %g: alpha rel err to the oracle %.2e, folded against plain %.2e" % (lam, rel, _rel(alphas[l].numpy(), plain[l].numpy())))
        assert rel < 1e-6, (lam, rel)
    assert be.builds == 21 and be.passes == 21
    assert be.ktkn_rows == [3] * 9 + [6] + [3] * 10


def test_a_path_wider_than_half_the_span_keeps_the_plain_form():
    """L = 9 with span 16: 2 L > span, so the full residual is a ktkn of its own: 1 + 20 + 1 builds."""
    X, y, idx = _problem(seed=36)
    lams = list(np.logspace(-7, -3, 9))
    be = StreamPathBackend()
    alphas = _path(be, X, y, idx, lams)
    assert be.ktkn_rows == [9] * 21 and be.builds == 22
    plain = _path(OracleBackend(np.float64), X, y, idx, lams)
    for l in range(9):
        assert _rel(alphas[l].numpy(), plain[l].numpy()) <= 1e-12, l      # the same operations on the same entries


def test_a_narrow_span_splits_the_groups():
    """L = 3 with span 2: no fold, every ktkn is two builds (2 + 1 rows)."""
    X, y, idx = _problem(seed=37)
    be = StreamPathBackend()
    be.span = 2
    _path(be, X, y, idx, LAMS[:3], maxiter=12)
    assert be.ktkn_rows == [3] * 13 and be.builds == 1 + 2 * 13


def test_a_path_of_one():
    """L = 1: the fold sends [p; x] (2 rows) through one ktkn; 21 builds; the alpha of falkon_fit on the same backend class
    (which folds with ktk2) to f64 rounding, and the oracle's to 1e-6."""
    from odx import solver
    X, y, idx = _problem(seed=38)
    be = StreamPathBackend()
    alpha = _path(be, X, y, idx, [1e-5])
    assert tuple(alpha.shape) == (1, len(idx))
    assert be.builds == 21 and be.ktkn_rows == [1] * 9 + [2] + [1] * 10
    one = StreamOracleBackend()
    F = one.features(torch.from_numpy(X))
    a1 = solver.falkon_fit(one, F, one.vec(y), one.rows(F, idx), 10.0, 1e-5, maxiter=20)
    assert _rel(alpha[0].numpy(), a1.numpy()) <= 1e-12
    ref, _ = fr.falkon_fit(X.astype(np.float64), y, idx, 10.0, 1e-5, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
    assert _rel(alpha[0].numpy(), ref[:, 0]) < 1e-6


@pytest.mark.parametrize("maxiter,builds", [(5, 6), (9, 10), (10, 11), (11, 12)])
def test_maxiter_around_the_full_residual_period(maxiter, builds):
    """Below the period no full residual exists; at maxiter = 10 the full step is the last one and is skipped, as in
    falkon_fit; at 11 it is folded.  Always 1 + maxiter builds."""
    X, y, idx = _problem(seed=39)
    be = StreamPathBackend()
    alphas = _path(be, X, y, idx, LAMS[:3], maxiter=maxiter)
    assert be.builds == builds
    assert be.ktkn_rows == ([3] * 9 + [6] + [3] if maxiter == 11 else [3] * maxiter)
    plain = _path(OracleBackend(np.float64), X, y, idx, LAMS[:3], maxiter=maxiter)
    for l in range(3):
        rel = _rel(alphas[l].numpy(), plain[l].numpy())
        print("maxiter %d member %d: folded against plain %.2e" % (maxiter, l, rel))
        if maxiter <= 10:
            assert rel <= 1e-12, (l, rel)        # no fold took place: the same operations


def test_replicated_row_shards_give_the_one_shard_alphas():
    """Two halves of the rows, each a streamed shard driven by its own thread, with an allreduce stub summing in place:
    the (2 L, Mp) matrix of the folded iteration is reduced ONCE; the alphas of the one-shard streamed path to f64 rounding
    (test_falkon_path_host's 1e-9: the partial products are added in another order)."""
    X, y, idx = _problem(seed=34)
    n, lams = len(X), LAMS[:3]
    be = StreamPathBackend()
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    whole = odx.falkon_fit_path(be, F, be.vec(y), Zf, 10.0, lams, 20)
    barrier, slots, shapes, bes = threading.Barrier(2), [None, None], [[], []], [None, None]

    def make_allreduce(rank):
        def allreduce(v):
            shapes[rank].append(tuple(v.shape))
            slots[rank] = v
            barrier.wait()
            total = slots[0] + slots[1]
            barrier.wait()
            v.copy_(total)
            return v
        return allreduce

    out, errs = [None, None], []

    def run(rank):
        try:
            rows = torch.arange(rank * (n // 2), n // 2 if rank == 0 else n)
            b = bes[rank] = StreamPathBackend()
            Fr = b.features(torch.from_numpy(X)[rows])
            out[rank] = odx.falkon_fit_path(b, Fr, b.vec(y)[rows], Zf, 10.0, lams, 20, n_total=n, allreduce=make_allreduce(rank))
        except Exception as e:      # noqa: BLE001 — reported below; the other thread must not wait for ever
            errs.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errs, errs
    Mp = (len(idx) + 1) // 2 * 2
    assert shapes[0] == [(len(idx),)] + [(3, Mp)] * 9 + [(6, Mp)] + [(3, Mp)] * 10
    assert bes[0].builds == 21 and bes[1].builds == 21
    for r in range(2):
        for l in range(3):
            rel = _rel(out[r][l].numpy(), whole[l].numpy())
            assert rel < 1e-9, (r, l, rel)
    assert torch.equal(out[0], out[1])


class SpanCountingBackend(CountingBackend):
    """A stored-block backend that also answers ktkn_span."""

    def ktkn_span(self, K):
        return 16


@pytest.mark.parametrize("maxiter", [10, 11, 20])
def test_stored_blocks_keep_the_plain_form(maxiter):
    """The pass count of test_one_build_and_the_passes_of_one_fit_per_member, on a stored-block backend with ktkn_span."""
    X, y, idx = _problem(seed=32)
    one = CountingBackend(np.float64)
    F = one.features(torch.from_numpy(X))
    a1 = odx.falkon_fit(one, F, one.vec(y), one.rows(F, idx), 10.0, LAMS[1], maxiter)
    be = SpanCountingBackend(np.float64)
    alphas = _path(be, X, y, idx, LAMS, maxiter=maxiter)
    assert be.calls["knm_rhs"] == 1 and be.calls["ktk"] == len(LAMS) * one.calls["ktk"] and be.calls["ktk2"] == 0
    assert torch.equal(alphas[1], a1)
