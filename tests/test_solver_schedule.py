"""The launch sequence of odx/solver.py, pinned: what falkon_fit, falkon_fit_path and falkon_fit_lockstep ask of the backend
and of the row shard, call by call, against a recording made with the solver.py of the commit before the three drivers
were put on one schedule (_cg_run).  No GPU, no floating-point value: names, flags and byte counts only, so the fixture
tests/golden/solver_schedule.json is the same on any machine.

A recording proxy around the tests' oracle backends logs every backend method the solver calls — trmv with its factor,
cg_step with its `full` flag, ktk / ktk2 with whether a t_out was passed — every phase entered and left, and every
collective of an EmulatedShard with its byte count.  One backend method is left out: `zeros`, the allocator.  Where a
buffer is allocated is not part of the schedule (falkon_fit now hands its pass a preallocated out=, which the log does
not record either), and allocations have no order among the launches that a result could depend on.

Re-record (only against a solver.py whose sequence is the reference, e.g. that of an earlier commit):
    git show <commit>:online-detection_amd/odx/solver.py > /tmp/solver_ref.py
    PYTHONPATH=online-detection_amd python -m tests.test_solver_schedule --record /tmp/solver_ref.py
"""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from odx import solver as odx_solver
from odx.dist import EmulatedShard
from tests.oracle_backend import OracleBackend
from tests.test_scores_from_cg_host import CgScoresOracleBackend
from tests.test_stream_path_host import StreamPathBackend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_schedule.json")
MAXITERS = (1, 10, 11, 20)
LAMS = [1e-5, 1e-4, 1e-3]


class Recorder:
    """Proxy of a backend: every method called through it is logged, in order; attributes it does not have stay missing
    (the solver's hasattr fallbacks see the backend as it is)."""

    def __init__(self, be, log):
        self._be, self._log = be, log

    def __getattr__(self, name):
        a = getattr(self._be, name)
        if not callable(a) or name == "zeros":
            return a

        def call(*args, **kw):
            entry = name
            if name == "trmv":
                entry += ":" + args[1]
            elif name == "cg_step":
                entry += ":full=%d" % bool(args[6])
            elif name in ("ktk", "ktk2") and "t_out" in kw:
                entry += ":t_out"
            self._log.append(entry)
            return a(*args, **kw)
        return call


class LoggedShard(EmulatedShard):
    def __init__(self, world, rank, log):
        super().__init__(world, rank)
        self._log = log

    def _count(self, kind, t):
        super()._count(kind, t)
        self._log.append("%s:%d" % (kind, int(t.numel()) * int(t.element_size())))


class _Phase:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def __enter__(self):
        self.log.append("phase+" + self.name)

    def __exit__(self, *exc):
        self.log.append("phase-" + self.name)
        return False


class StoredPathBackend(OracleBackend):
    """The oracle backend with the lambda path's two entries on a stored block: ktkn (one read of K for all rows) and
    precond_path."""
    fold = False

    def precond_path(self, Zf, sigma, lams, eps):
        return [self.precond(Zf, sigma, lam, eps) for lam in lams]

    def ktkn(self, K, V, out=None):
        for l in range(V.shape[0]):
            OracleBackend.ktk(self, K, v=V[l, :K.M], out=out[l, :K.M])
        return out


def _problem(n=600, D=12, M=41, seed=5):          # M odd: the padded rows (Mp = 42) show in the byte counts
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    y = np.where(X[:, 0] + 0.3 * rng.standard_normal(n) > 0, 1.0, -1.0)
    return X, y, rng.choice(n, M, replace=False)


def _oracle(fold):
    be = OracleBackend(np.float64)
    be.fold = fold
    return be


def _span(span):
    be = StreamPathBackend()
    be.span = span
    return be


def _fit(sv, be, log, maxiter, world=None, rank=0, owner=None, replicated=False, scores=False):
    X, y, idx = _problem()
    rec = Recorder(be, log)
    F = be.features(X)
    kw = {}
    if replicated:
        kw = {"allreduce": LoggedShard(world, rank, log).allreduce, "n_total": world * F.n}
    elif world is not None:
        kw = {"shard": LoggedShard(world, rank, log), "owner": owner, "n_total": world * F.n}
    S = torch.full((F.n,), 7.0, dtype=torch.float64) if scores else None
    alpha = sv.falkon_fit(rec, F, be.vec(y), be.rows(F, idx), 4.0, 1e-3, maxiter, phase=lambda name: _Phase(log, name),
                          scores_out=S, **kw)
    return [alpha] + ([S] if scores else [])


def _path(sv, be, log, maxiter):
    X, y, idx = _problem()
    F = be.features(torch.from_numpy(X))
    return [sv.falkon_fit_path(Recorder(be, log), F, be.vec(y), be.rows(F, idx), 4.0, LAMS, maxiter,
                               phase=lambda name: _Phase(log, name))]


def _lockstep(sv, be, log, maxiter, world, rank, B, scores=False):
    X, y, idx = _problem()
    F = be.features(X)
    rng = np.random.default_rng(9)
    ys = [be.vec(y if b == 0 else np.where(X[:, b] > 0, 1.0, -1.0)) for b in range(B)]
    Zfs = [be.rows(F, idx if b == 0 else rng.choice(F.n, len(idx), replace=False)) for b in range(B)]
    S = [torch.full((F.n,), 7.0, dtype=torch.float64) for _ in range(B)] if scores else None
    alphas = sv.falkon_fit_lockstep(Recorder(be, log), F, ys, Zfs, 4.0, 1e-3, maxiter, n_total=world * F.n,
                                    shard=LoggedShard(world, rank, log), phase=lambda name: _Phase(log, name), scores_out=S)
    return list(alphas) + (S or [])


# name -> (sv, log, maxiter) -> the tensors the fit produced
SCENARIOS = {
    "fit/one_shard/fold_off": lambda sv, log, k: _fit(sv, _oracle(False), log, k),
    "fit/one_shard/fold_on": lambda sv, log, k: _fit(sv, _oracle(True), log, k),
    "fit/scores/fold_on": lambda sv, log, k: _fit(sv, CgScoresOracleBackend(fold=True), log, k, scores=True),
    "fit/scores/fold_off": lambda sv, log, k: _fit(sv, CgScoresOracleBackend(fold=False), log, k, scores=True),
    "fit/replicated_allreduce": lambda sv, log, k: _fit(sv, _oracle(True), log, k, world=2, replicated=True),
    "fit/owner_mode/owner/fold_on": lambda sv, log, k: _fit(sv, _oracle(True), log, k, world=2, rank=0, owner=0),
    "fit/owner_mode/owner/fold_off": lambda sv, log, k: _fit(sv, _oracle(False), log, k, world=2, rank=0, owner=0),
    "fit/owner_mode/non_owner/fold_on": lambda sv, log, k: _fit(sv, _oracle(True), log, k, world=2, rank=1, owner=0),
    "fit/owner_mode/non_owner/fold_off": lambda sv, log, k: _fit(sv, _oracle(False), log, k, world=2, rank=1, owner=0),
    "fit/streamed_shard": lambda sv, log, k: _fit(sv, _span(16), log, k),
    "path/stored_L3": lambda sv, log, k: _path(sv, StoredPathBackend(np.float64), log, k),
    "path/streamed_2L_le_span": lambda sv, log, k: _path(sv, _span(16), log, k),
    "path/streamed_2L_gt_span": lambda sv, log, k: _path(sv, _span(4), log, k),
    "path/no_ktkn": lambda sv, log, k: _path(sv, _oracle(True), log, k),
    "lockstep/world1_B1_scores/fold_on": lambda sv, log, k: _lockstep(sv, CgScoresOracleBackend(fold=True), log, k, 1, 0, 1, True),
    "lockstep/world1_B1_scores/fold_off": lambda sv, log, k: _lockstep(sv, CgScoresOracleBackend(fold=False), log, k, 1, 0, 1, True),
    "lockstep/world4_B3/owning/fold_on": lambda sv, log, k: _lockstep(sv, _oracle(True), log, k, 4, 1, 3),
    "lockstep/world4_B3/owning/fold_off": lambda sv, log, k: _lockstep(sv, _oracle(False), log, k, 4, 1, 3),
    "lockstep/world4_B3/non_owning/fold_on": lambda sv, log, k: _lockstep(sv, _oracle(True), log, k, 4, 3, 3),
    "lockstep/world4_B3/non_owning/fold_off": lambda sv, log, k: _lockstep(sv, _oracle(False), log, k, 4, 3, 3),
}
CASES = ["%s/maxiter%d" % (name, k) for name in SCENARIOS for k in MAXITERS]


def run_case(sv, case):
    """(log, tensors) of one case under the solver module `sv`."""
    name, k = case.rsplit("/maxiter", 1)
    log = []
    return log, SCENARIOS[name](sv, log, int(k))


def load_solver(path, name="odx._solver_under_record"):
    """A solver.py from elsewhere, imported as a member of the odx package (its relative imports resolve)."""
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_launch_sequence_is_the_recorded_one(case, golden):
    log, _ = run_case(odx_solver, case)
    want = golden[case]
    for i, (a, b) in enumerate(zip(log, want)):
        assert a == b, "%s: entry %d is %r, recorded %r (after %r)" % (case, i, a, b, log[max(0, i - 5):i])
    assert len(log) == len(want), "%s: %d entries, recorded %d" % (case, len(log), len(want))


def test_the_cases_exercise_what_they_name(golden):
    """The recording itself: folds where a case says fold, none where it says not; t_out only with scores; collectives on
    ranks without a CG state."""
    def count(case, entry):
        return sum(e == entry for e in golden[case])
    assert count("fit/one_shard/fold_on/maxiter11", "ktk2") == 1 and count("fit/one_shard/fold_on/maxiter10", "ktk2") == 0
    assert count("fit/one_shard/fold_off/maxiter20", "ktk2") == 0 and count("fit/one_shard/fold_off/maxiter20", "ktk") == 21
    assert count("fit/scores/fold_on/maxiter20", "ktk:t_out") == 19 and count("fit/scores/fold_on/maxiter20", "ktk2:t_out") == 1
    assert count("fit/scores/fold_off/maxiter20", "ktk:t_out") == 20 and count("fit/scores/fold_off/maxiter20", "ktk") == 1
    assert not any("t_out" in e for e in golden["fit/one_shard/fold_on/maxiter20"])
    assert count("fit/owner_mode/non_owner/fold_on/maxiter20", "trmv:LAit") == 0
    assert sum(e.startswith("broadcast:") for e in golden["fit/owner_mode/non_owner/fold_on/maxiter20"]) == 21
    assert count("path/streamed_2L_le_span/maxiter20", "cg_residual") == 3 and count("path/streamed_2L_gt_span/maxiter20", "cg_residual") == 0
    assert count("path/stored_L3/maxiter20", "ktkn") == 21 and count("path/no_ktkn/maxiter20", "ktk") == 63
    assert count("lockstep/world4_B3/non_owning/fold_on/maxiter20", "ktk") == 57 and count("lockstep/world4_B3/non_owning/fold_on/maxiter20", "ktk2") == 3
    assert count("lockstep/world4_B3/non_owning/fold_on/maxiter20", "cg_step:full=0") == 0
    assert count("lockstep/world1_B1_scores/fold_on/maxiter20", "cg_scores_axpy") == 20


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python -m tests.test_solver_schedule --record PATH_TO_A_SOLVER_PY")
    ref = load_solver(sys.argv[2])
    with open(GOLDEN, "w") as f:
        json.dump({case: run_case(ref, case)[0] for case in CASES}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("recorded %d cases from %s into %s" % (len(CASES), sys.argv[2], GOLDEN))
