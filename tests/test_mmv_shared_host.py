"""Host logic of the shared-centre scoring route on the numpy oracle backend: odx.predict_path makes ONE dense mmv for the
members of a path, predict of a multi-output model passes no ranges, and GaussianKernel.mmv without `dense` still looks for
the block structure of its weights (the heads' path).  No GPU."""
import copy

import numpy as np
import pytest
import torch

import odx
from tests.oracle_backend import OracleBackend
from tests.synth import blob_problem, centres

LAMS = [1e-5, 1e-4, 1e-3]


class CountingBackend(OracleBackend):
    """The oracle backend recording every mmv call: the number of columns and the ranges it was given."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.mmv_calls = []

    def mmv(self, F, Zf, sigma, V, ranges=None, out=None, max_range=None):
        V2 = torch.as_tensor(V)
        self.mmv_calls.append((1 if V2.dim() == 1 else int(V2.shape[1]), None if ranges is None else ranges.clone()))
        return super().mmv(F, Zf, sigma, V, ranges, out, max_range)


@pytest.fixture
def be():
    b = CountingBackend(np.float64)
    odx.set_backend(b)
    yield b
    odx.set_backend(None)


def _template(idx, sigma=6.0, cls=None):
    from odx.wrappers import CenterSelector
    return (cls or odx.InCoreFalkon)(kernel=odx.GaussianKernel(sigma=sigma), penalty=1e-3, M=len(idx), maxiter=10,
                                     center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))


def _path(cls=None):
    X, y, rng = blob_problem(400, 16, seed=8)
    idx = centres(y, 40, rng)
    Xt = torch.from_numpy(X)
    return _template(idx, cls=cls).fit_path(Xt, torch.from_numpy(y), LAMS), Xt


def test_predict_path_is_one_mmv_and_the_members_predict_columns(be):
    models, Xt = _path()
    cols = [m.predict(Xt[:70]) for m in models]
    be.mmv_calls.clear()
    got = odx.predict_path(models, Xt[:70])
    assert len(be.mmv_calls) == 1 and be.mmv_calls[0][0] == len(LAMS) and be.mmv_calls[0][1] is None
    assert got.dtype == torch.float32 and tuple(got.shape) == (70, len(LAMS))
    assert torch.equal(got, torch.cat(cols, dim=1))
    # members given as a generator, and in another order
    assert torch.equal(odx.predict_path((m for m in reversed(models)), Xt[:70]), torch.cat(cols[::-1], dim=1))


def test_predict_path_accepts_equal_views_of_the_centres(be):
    models, Xt = _path()
    other = copy.copy(models[1])
    other.__dict__.pop("_zf", None)
    other.ny_points_ = models[0].ny_points_[:]          # another tensor object: same storage, shape and strides
    assert other.ny_points_ is not models[0].ny_points_
    assert torch.equal(odx.predict_path([models[0], other], Xt[:9]), odx.predict_path(models[:2], Xt[:9]))


def test_predict_path_of_a_host_model_returns_host_scores(be):
    models, Xt = _path(cls=odx.Falkon)
    got = odx.predict_path(models, Xt[:20])
    assert got.device.type == "cpu" and torch.equal(got[:, 2:3], models[2].predict(Xt[:20]))


def test_predict_path_refuses_what_does_not_share_centres_sigma_or_shape(be):
    models, Xt = _path()
    with pytest.raises(ValueError):
        odx.predict_path([], Xt)
    moved = copy.copy(models[1])
    moved.ny_points_ = models[0].ny_points_.clone()     # equal values, another tensor
    with pytest.raises(ValueError, match="ny_points_"):
        odx.predict_path([models[0], moved], Xt)
    fewer = copy.copy(models[1])
    fewer.ny_points_ = models[0].ny_points_[:-1]
    fewer.alpha_ = models[1].alpha_[:-1]
    with pytest.raises(ValueError, match="ny_points_"):
        odx.predict_path([models[0], fewer], Xt)
    wider = copy.copy(models[1])
    wider.kernel = odx.GaussianKernel(sigma=7.0)
    with pytest.raises(ValueError, match="sigma"):
        odx.predict_path([models[0], wider], Xt)
    two = copy.copy(models[1])
    two.alpha_ = torch.cat([models[1].alpha_, models[2].alpha_], dim=1)
    with pytest.raises(ValueError, match=r"\(M, 1\)"):
        odx.predict_path([models[0], two], Xt)
    flat = copy.copy(models[1])
    flat.alpha_ = models[1].alpha_[:, 0]
    with pytest.raises(ValueError, match=r"\(M, 1\)"):
        odx.predict_path([models[0], flat], Xt)
    with pytest.raises(RuntimeError):
        odx.predict_path([models[0], _template([0, 1])], Xt)


def test_predict_of_a_multi_output_model_passes_no_ranges(be):
    X, y, rng = blob_problem(300, 16, seed=9)
    idx = centres(y, 30, rng)
    g = np.random.default_rng(5)
    Y = np.stack([y.astype(np.float64), np.where(X @ g.standard_normal(16) > 0, 1.0, -1.0)], 1)
    Xt = torch.from_numpy(X)
    m = _template(idx).fit_multi(Xt, torch.from_numpy(Y))
    assert tuple(m.alpha_.shape) == (30, 2)
    m.alpha_[0, 1] = 0.0          # block_ranges would now start column 1 at row 1: predict does not ask it
    be.mmv_calls.clear()
    p = m.predict(Xt[:40])
    assert tuple(p.shape) == (40, 2)
    assert be.mmv_calls == [(2, None)]
    # one output: one column, no ranges, as before
    one = _template(idx).fit(Xt, torch.from_numpy(y))
    be.mmv_calls.clear()
    one.predict(Xt[:40])
    assert be.mmv_calls == [(1, None)]


def test_kernel_mmv_without_dense_still_finds_the_blocks(be):
    X, _, rng = blob_problem(50, 8, seed=3)
    Z = torch.from_numpy(X[:12])
    V = torch.zeros((12, 3), dtype=torch.float64)
    V[0:5, 0] = torch.from_numpy(rng.standard_normal(5))
    V[5:12, 2] = torch.from_numpy(rng.standard_normal(7))
    k = odx.GaussianKernel(sigma=5.0)
    a = k.mmv(torch.from_numpy(X), Z, V)
    assert len(be.mmv_calls) == 1 and be.mmv_calls[0][1].tolist() == [[0, 5], [0, 0], [5, 12]]
    b = k.mmv(torch.from_numpy(X), Z, V, dense=True)
    assert be.mmv_calls[1] == (3, None)
    assert torch.equal(a, b)          # (the oracle backend multiplies densely either way)
    k.mmv(torch.from_numpy(X), Z, V[:, 0])
    assert be.mmv_calls[2] == (1, None)
