"""Distinct columns without a GPU: the column map (odx/cols.py), the calls the wrappers make for a block that carries one
(pinned against the recording fake library of tests/test_knm_calls_host.py; tests/golden/knm_cols_calls.json holds the
log, `PYTHONPATH=online-detection_amd:. python tests/test_distinct_columns_host.py` writes it anew), and which classes of a
LockstepClassJob get a map."""
import json
import os

import numpy as np
import pytest
import torch

from odx import hip
from odx.cols import column_map
from tests.test_knm_calls_host import F32, Rec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knm_cols_calls.json")


# ------------------------------------------------------------------------------------------------------------- the map
def _check_map(idx):
    idx = np.asarray(idx, dtype=np.int64)
    m = column_map(torch.from_numpy(idx))
    M = len(idx)
    distinct = list(dict.fromkeys(idx.tolist()))              # order of first occurrence
    assert (m.Mv, m.Md) == (M, len(distinct))
    assert m.col_of.dtype == m.start.dtype == m.pos.dtype == torch.int32
    assert tuple(m.col_of.shape) == (M,) and tuple(m.start.shape) == (m.Md + 1,) and tuple(m.pos.shape) == (M,)
    assert idx[m.first.numpy()].tolist() == distinct and (np.diff(m.first.numpy()) > 0).all()
    assert [distinct[d] for d in m.col_of.tolist()] == idx.tolist()
    start, pos = m.start.tolist(), m.pos.tolist()
    assert start[0] == 0 and start[-1] == M and sorted(pos) == list(range(M))
    for d in range(m.Md):
        mine = pos[start[d]:start[d + 1]]
        assert mine == sorted(mine) and mine == [j for j in range(M) if idx[j] == distinct[d]] and mine[0] == int(m.first[d])
    return m


def test_map_of_repeated_centres():
    # 7 twice, 3 three times, 9 four times; repeats at positions 0 and M - 1
    m = _check_map([9, 7, 3, 9, 5, 7, 3, 9, 8, 3, 9])
    assert np.diff(m.start.numpy()).tolist() == [4, 2, 3, 1, 1]
    assert m.col_of.tolist() == [0, 1, 2, 0, 3, 1, 2, 0, 4, 2, 0]
    _check_map([4, 4])
    _check_map([1, 2, 3, 1])
    _check_map([1, 2, 3, 3])
    rng = np.random.default_rng(0)
    _check_map(rng.integers(0, 300, 400))                     # drawn with replacement


def test_no_repeats_no_map():
    assert column_map(torch.tensor([5, 1, 9, 0])) is None
    assert column_map(torch.arange(1000)) is None
    assert column_map(torch.tensor([7])) is None


def test_fold_and_expand_of_the_map():
    m = column_map(torch.tensor([9, 7, 3, 9, 5, 7, 3, 9, 8, 3, 9]))
    v = torch.arange(1, 12, dtype=torch.float64)
    f = m.fold(v)
    assert f.tolist() == [1 + 4 + 8 + 11, 2 + 6, 3 + 7 + 10, 5, 9]
    assert m.expand(f).tolist() == [f[d].item() for d in m.col_of.tolist()]
    # left to right: ((a + b) + c) + d, not another grouping
    w = torch.tensor([1e16, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1e16, 0.0, 0.0, 1.0], dtype=torch.float64)
    assert m.fold(w)[0].item() == ((1e16 + 1.0) + -1e16) + 1.0
    # the device copies are made once
    assert m.on("cpu") is m.on("cpu") and [t.dtype for t in m.on("cpu")] == [torch.int64] + [torch.int32] * 3


# ------------------------------------------------------------------------------------------------------- wrapper calls
N, M = 10, 21
IDX = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6]      # 21 positions over 9 distinct centres, 3 four times
CASES = {}


def case(name, **kw):
    def add(fn):
        assert name not in CASES
        CASES[name] = (fn, kw)
        return fn
    return add


def _mapped_block(r, fmt, rows=None):
    """A compact block of the 9 distinct columns of IDX with its map; the map's tensors are named, so the log says which
    of them each pointer is."""
    cmap = column_map(torch.tensor(IDX))
    K = r.block(fmt, N, cmap.Md, rows=rows)
    K.cmap, K.Mv = cmap, cmap.Mv
    for name, t in zip(("first", "col_of", "start", "pos"), cmap.on("cpu")):
        r.t("map." + name, t)
    return K


for _fmt in ("u24", "bf16"):
    for _how in ("v", "w", "vw", "t_out"):
        @case("ktk-cols-%s-%s" % (_fmt, _how))
        def _(r, fmt=_fmt, how=_how):
            return r.be.ktk(_mapped_block(r, fmt), v=r.vec("v", M) if how != "w" else None, w=r.vec("w", N) if how in ("w", "vw") else None,
                            out=r.vec("out", M), t_out=r.vec("t", N) if how == "t_out" else None)

    @case("ktk-cols-%s-out-none" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk(_mapped_block(r, fmt), v=r.vec("v", M))

    @case("ktk-cols-%s-row-range" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk(_mapped_block(r, fmt, rows=(3, 8)), v=r.vec("v", M), out=r.vec("out", M), t_out=r.vec("t", 5))

    for _t in (False, True):
        @case("ktk2-cols-%s%s" % (_fmt, "-t_out" if _t else ""))
        def _(r, fmt=_fmt, t=_t):
            return r.be.ktk2(_mapped_block(r, fmt), r.vec("v1", M), r.vec("v2", M), out1=r.vec("o1", M), out2=r.vec("o2", M),
                             t_out=r.vec("t", N) if t else None)

    @case("ktk2-cols-%s-out-none" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.ktk2(_mapped_block(r, fmt), r.vec("v1", M), r.vec("v2", M))

    @case("knm_mv-cols-%s" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.knm_mv(_mapped_block(r, fmt), r.vec("alpha", M), out=r.mat("S", N, 7, dtype=F32)[:, 3:4])

    @case("knm_mv-cols-%s-summed" % _fmt)
    def _(r, fmt=_fmt):
        return r.be.knm_mv(_mapped_block(r, fmt), None, summed=r.vec("sum", N))


def _run(name):
    fn, kw = CASES[name]
    r = Rec(**kw)
    return r.result(fn(r))


_golden = None


def _load():
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)
    return _golden


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_are_the_recorded_ones(name):
    assert name in _load()["calls"], "no recorded calls for this case"
    assert json.loads(json.dumps(_run(name))) == _load()["calls"][name]


def test_the_fixture_has_no_other_cases():
    assert sorted(_load()["calls"]) == sorted(CASES)


def test_what_the_recorded_calls_say():
    """The golden log read once by hand: the _cols entry with the block's 9 columns, vectors of the list's 21 positions, the
    workspace of the 9-column block, and the map's three vectors behind Mv."""
    got = _run("ktk-cols-u24-t_out")
    (call,) = got["calls"]
    assert call[0] == "odx_knm_fwd_bwd_q_cols_t" and len(call) - 1 == len(hip.SIGNATURES["odx_knm_fwd_bwd_q_cols_t"][1])
    assert call[6:8] == [N, 9] and call[8] == ["v", 0] and call[10] == ["out", 0] and call[11] == ["t", 0]
    assert call[14:] == [M, ["map.col_of", 0], ["map.start", 0], ["map.pos", 0], None]
    assert got["workspaces"] == [["ktk", 64 + 16 * (1 * N + 2 * 9 + 3 * hip.KNM_U24)]]
    two = _run("ktk2-cols-bf16-t_out")["calls"][0]
    assert two[0] == "odx_knm_fwd_bwd2_q_cols_t" and two[15:] == [M, ["map.col_of", 0], ["map.start", 0], ["map.pos", 0], None]
    mv = _run("knm_mv-cols-u24")["calls"]
    assert [c[0] for c in mv] == ["odx_cols_fold_f64", "odx_knm_mv"] and mv[0][1:6] == [["alpha", 0], M, ["map.start", 0], ["map.pos", 0], 9]
    assert mv[1][7] == 9 and mv[1][8] == mv[0][6]               # the folded vector is what odx_knm_mv multiplies with
    assert [c[0] for c in _run("knm_mv-cols-u24-summed")["calls"]] == ["odx_cg_scores_store_f32"]


def test_refusals():
    for fn in (lambda r: r.be.ktkn(_mapped_block(r, "u24"), r.mat("V", 3, M, 24)),
               lambda r: r.be.kvn(_mapped_block(r, "u24"), r.mat("V", 3, M, 24)),
               lambda r: r.be.ktwn(_mapped_block(r, "u24"), r.mat("W", 3, N, 12)),
               lambda r: r.be.knm_mv(_mapped_block(r, "u24"), r.vec("alpha", 9))):          # alpha has the LIST's length
        r = Rec()
        with pytest.raises(ValueError):
            fn(r)
        assert r.calls == []
    # the two-vector pass of a mapped block exists where the full block's would: every class of a job decides alike
    r = Rec()
    assert r.be.can_ktk2(_mapped_block(r, "u24"))
    r = Rec(unsupported=["odx_knm_fwd_bwd2_q_workspace_bytes"])
    assert not r.be.can_ktk2(_mapped_block(r, "u24"))


# ------------------------------------------------------------------------------------------------------------- the job
class _FormatBackend:
    """What LockstepClassJob's constructor asks of a backend, with a storage format to answer with."""

    def __init__(self, fmt):
        self.fmt = fmt

    def knm_format(self, n, M):
        return self.fmt

    def knm_bytes(self, n, M, D=None):
        return n * M * 3


def _job(fmt, mode, n=600, M=40, **kw):
    from odx.job import LockstepClassJob
    X = torch.zeros((n, 8))
    rep = torch.arange(M)
    rep[-1] = rep[0]
    cidx = [rep, torch.arange(M), rep.clone()]
    return LockstepClassJob(_FormatBackend(fmt), X, n, M, lambda c: None, cidx, 6.0, 1e-4, distinct_columns=mode, **kw), cidx


def test_which_classes_get_a_map():
    job, cidx = _job("u24", "force")
    assert sorted(job._cmaps) == sorted({job._idx_key(cidx[0]), job._idx_key(cidx[2])})      # the class without repeats: none
    assert job._cmaps[job._idx_key(cidx[0])].Md == 39
    for fmt in ("f32", "stream"):
        assert _job(fmt, "force")[0]._cmaps == {}
    assert _job("bf16", "force")[0]._cmaps != {}
    assert _job("u24", False)[0]._cmaps == {} and _job("u24", "auto")[0]._cmaps == {}       # 600 x 40 entries: below the bound
    big = 2 ** 27 // 40
    assert _job("u24", "auto", n=big + 1)[0]._cmaps != {} and _job("u24", "auto", n=big - 1)[0]._cmaps == {}
    with pytest.raises(ValueError):
        _job("u24", True)


def test_a_backend_without_compact_storage_never_gets_a_map():
    """The oracle backend of the CPU suite (no knm_format): a job with repeated centres runs as before under every setting."""
    from odx.job import LockstepClassJob
    from tests.oracle_backend import OracleBackend
    rng = np.random.default_rng(3)
    n, D, M = 300, 8, 30
    X = rng.standard_normal((n, D)).astype(np.float32)
    idx = rng.integers(0, n, M)
    assert len(set(idx.tolist())) < M
    row_ids = torch.arange(n)
    out = []
    for mode in ("auto", "force", False):
        be = OracleBackend()
        alphas = {}
        job = LockstepClassJob(be, torch.from_numpy(X), n, M, lambda c: torch.where((row_ids % 3) == c, 1.0, -1.0).double(),
                               [torch.from_numpy(idx)], 6.0, 1e-3, 20, distinct_columns=mode)
        job.run(be.features(job.X), alphas_out=alphas)
        assert job._cmaps == {} and not [t for t in job.trace if t[0] == "distinct"]
        out.append(alphas[0].numpy().copy())
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({"calls": {name: _run(name) for name in sorted(CASES)}}, f, separators=(",", ":"), sort_keys=True)
