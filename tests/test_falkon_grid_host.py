"""Host logic of the (sigma, lambda) grid (odx.solver.falkon_fit_grid, _FalkonBase.fit_grid, odx.predict_grid) on the numpy
oracle backend: every row of the grid is falkon_fit_path's at its sigma, operation for operation.  No GPU."""
import numpy as np
import pytest
import torch

import odx
from oracle import falkon_ref as fr
from tests.oracle_backend import OracleBackend
from tests.synth import blob_problem, centres
from tests.test_falkon_path_host import LAMS

SIGMAS = [6.0, 10.0, 15.0]


class CountingBackend(OracleBackend):
    """The oracle backend (no knm_rhs_sigmas: the grid loops knm_rhs) with a counter of its builds."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.builds = []

    def knm_rhs(self, F, Zf, sigma, w, **kw):
        self.builds.append(float(sigma))
        return super().knm_rhs(F, Zf, sigma, w, **kw)


@pytest.fixture(scope="module")
def problem():
    """n = 1500, D = 48, M = 150; the grid fitted once (blocks_at_once = 4, the default) and shared by the tests below."""
    X, y, rng = blob_problem(1500, 48, seed=31)
    idx = centres(y, 150, rng)
    be = CountingBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    grid = odx.falkon_fit_grid(be, F, be.vec(y), Zf, SIGMAS, LAMS, 20)
    assert be.builds == SIGMAS                      # one block per width, in order
    return X, y, idx, be, F, Zf, grid


def test_grid_rows_equal_the_path_at_every_sigma(problem):
    X, y, idx, be, F, Zf, grid = problem
    assert tuple(grid.shape) == (len(SIGMAS), len(LAMS), len(idx)) and grid.dtype == torch.float64
    for s, sigma in enumerate(SIGMAS):
        path = odx.falkon_fit_path(be, F, be.vec(y), Zf, sigma, LAMS, 20)
        assert torch.equal(grid[s], path), sigma


def test_grid_rows_equal_the_oracle(problem):
    """Against oracle.falkon_ref.falkon_fit at every (sigma, lambda): 1e-6 relative, the bar of test_falkon_path_host.py."""
    X, y, idx, _, _, _, grid = problem
    for s, sigma in enumerate(SIGMAS):
        for l, lam in enumerate(LAMS):
            ref, _ = fr.falkon_fit(X.astype(np.float64), y, idx, sigma, lam, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
            rel = np.linalg.norm(grid[s, l].numpy() - ref[:, 0]) / np.linalg.norm(ref[:, 0])
            print("sigma %g lam %g: alpha rel err %.2e" % (sigma, lam, rel))
            assert rel < 1e-6, (sigma, lam, rel)


@pytest.mark.parametrize("width", [1, 2, 4])
def test_groups_of_any_width_give_the_same_alphas(problem, width):
    _, y, _, _, F, Zf, grid = problem
    be = CountingBackend(np.float64)
    again = odx.falkon_fit_grid(be, F, be.vec(y), Zf, SIGMAS, LAMS, 20, blocks_at_once=width)
    assert be.builds == SIGMAS and torch.equal(again, grid)


class GroupBackend(OracleBackend):
    """A backend WITH knm_rhs_sigmas: the grid must hand it groups of blocks_at_once widths and never call knm_rhs."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = []

    def knm_rhs_sigmas(self, F, Zf, sigmas, w, outs=None):
        self.groups.append(list(sigmas))
        return [OracleBackend.knm_rhs(self, F, Zf, s, w) for s in sigmas]

    def knm_rhs(self, *a, **kw):
        raise AssertionError("falkon_fit_grid called knm_rhs on a backend that has knm_rhs_sigmas")


def test_a_backend_with_knm_rhs_sigmas_gets_the_groups(problem):
    _, y, _, _, F, Zf, grid = problem
    be = GroupBackend(np.float64)
    blocks = []
    got = odx.falkon_fit_grid(be, F, be.vec(y), Zf, SIGMAS, LAMS, 20, blocks_at_once=2, knm_blocks=blocks)
    assert be.groups == [SIGMAS[:2], SIGMAS[2:]] and len(blocks) == len(SIGMAS)
    assert torch.equal(got, grid)


@pytest.mark.parametrize("sigmas", [[], [0.0], [10.0, -1.0], [float("nan")], [float("inf"), 10.0]])
def test_bad_sigmas_are_refused(sigmas):
    X, y, rng = blob_problem(300, 16, seed=35)
    idx = centres(y, 30, rng)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    with pytest.raises(ValueError, match="sigmas"):
        odx.falkon_fit_grid(be, F, be.vec(y), be.rows(F, idx), sigmas, [1e-4], 5)


def test_bad_penalties_and_widths_of_groups_are_refused():
    X, y, rng = blob_problem(300, 16, seed=35)
    idx = centres(y, 30, rng)
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    for lams in ([], [0.0], [1e-5, float("nan")]):
        with pytest.raises(ValueError, match="lams"):
            odx.falkon_fit_grid(be, F, be.vec(y), be.rows(F, idx), [10.0], lams, 5)
    with pytest.raises(ValueError, match="blocks_at_once"):
        odx.falkon_fit_grid(be, F, be.vec(y), be.rows(F, idx), [10.0], [1e-4], 5, blocks_at_once=0)


def test_estimator_fit_grid_and_predict_grid():
    from odx.wrappers import CenterSelector
    X, y, rng = blob_problem(600, 24, seed=8)
    idx = centres(y, 60, rng)
    sigmas, lams = [4.0, 6.0], LAMS[1:3]
    odx.set_backend(OracleBackend(np.float64))
    try:
        mk = lambda sigma: odx.InCoreFalkon(kernel=odx.GaussianKernel(sigma=sigma), penalty=1e-3, M=len(idx), maxiter=20,    # noqa: E731
                                            center_selection=CenterSelector(idx), options=odx.FalkonOptions(keops_active="no"))
        Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
        m = mk(9.0)
        grid = m.fit_grid(Xt, yt, sigmas, lams)
        assert m.alpha_ is None and m.penalty == 1e-3 and m.kernel.sigma == 9.0          # the template is left alone
        assert len(grid) == len(sigmas) and all(len(row) == len(lams) for row in grid)
        flat = [e for row in grid for e in row]
        for s, sigma in enumerate(sigmas):
            path = mk(sigma).fit_path(Xt, yt, lams)
            for l, lam in enumerate(lams):
                e = grid[s][l]
                assert type(e) is type(m) and e.kernel.sigma == sigma and e.penalty == lam and e.M == 60
                assert e.ny_points_ is flat[0].ny_points_ and tuple(e.alpha_.shape) == (60, 1)
                assert torch.equal(e.alpha_, path[l].alpha_), (sigma, lam)
        scores = odx.predict_grid(flat, Xt[:50])
        assert tuple(scores.shape) == (50, len(flat)) and scores.dtype == torch.float32
        for t, e in enumerate(flat):
            assert torch.equal(scores[:, t], e.predict(Xt[:50])[:, 0]), t
        with pytest.raises(ValueError, match="sigma"):                                    # predict_path keeps refusing mixed widths
            odx.predict_path(flat, Xt[:50])
        other = mk(4.0).fit(Xt, yt)                                                       # the same centres in a tensor of its own
        with pytest.raises(ValueError, match="ny_points_"):
            odx.predict_grid([flat[0], other], Xt[:50])
        with pytest.raises(ValueError):
            odx.predict_grid([], Xt[:50])
    finally:
        odx.set_backend(None)
