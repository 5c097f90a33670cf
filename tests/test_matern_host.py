"""odx.MaternKernel without a GPU: the constructor rules, the kind codes against include/odx.h, the f64 statement of the
kernels (tests/matern_ref.py) against direct differences, and the solver on the numpy oracle backend carrying the kernel
object untouched — every fit equals oracle.falkon_ref.falkon_fit with its gaussian_kernel replaced by radial_kernel."""
import math
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

import odx
from oracle import falkon_ref as fr
from tests.matern_ref import direct_kernel, radial_kernel
from tests.oracle_backend import OracleBackend
from tests.synth import blob_problem, centres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUS = [1.5, 2.5]


def _header_kinds():
    text = open(os.path.join(ROOT, "include", "odx.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+ODX_KERNEL_(\w+)\s+(\d+)", text)}


def test_constructor_rules():
    k = odx.MaternKernel(5, 1.5)
    assert k.sigma == 5.0 and k.nu == 1.5 and k.kernel_name == "matern" and isinstance(k.sigma, float)
    assert odx.MaternKernel(7.5, 2.5, opt=None).nu == 2.5
    assert odx.falkon.kernels.MaternKernel is odx.MaternKernel
    with pytest.raises(NotImplementedError, match="slope"):
        odx.MaternKernel(5.0, 0.5)
    for bad in (1.0, 2.0, 3.5, 0.0, -1.5, float("nan")):
        with pytest.raises(ValueError):
            odx.MaternKernel(5.0, bad)
    assert callable(k.mmv)
    k2 = pickle.loads(pickle.dumps(k))
    assert (k2.sigma, k2.nu, k2.kind) == (k.sigma, k.nu, k.kind)


def test_kinds_are_the_headers():
    kinds = _header_kinds()
    assert kinds == {"GAUSS": 0, "MATERN32": 1, "MATERN52": 2}
    assert odx.GaussianKernel(3.0).kind == kinds["GAUSS"]
    assert odx.MaternKernel(3.0, 1.5).kind == kinds["MATERN32"]
    assert odx.MaternKernel(3.0, 2.5).kind == kinds["MATERN52"]
    assert odx.MaternKernel(3.0, float("inf")).kind == kinds["GAUSS"]
    assert (odx.hip.KERNEL_GAUSS, odx.hip.KERNEL_MATERN32, odx.hip.KERNEL_MATERN52) == (0, 1, 2)
    assert odx.hip.radial_of(4) == (4.0, 0) and odx.hip.radial_of(odx.MaternKernel(4, 2.5)) == (4.0, 2)
    assert odx.hip.radial_of(odx.MaternKernel(4, float("inf"))) == (4.0, 0)


def test_no_float_and_what_travels():
    """The object has no __float__: a wrapper that was not taught the kinds fails at its own float(sigma).  A Gaussian
    estimator hands down the float it always did; a Matern one the object; nu = inf is the Gaussian's float."""
    k = odx.MaternKernel(5.0, 2.5)
    assert not hasattr(k, "__float__")
    with pytest.raises(TypeError):
        float(k)
    arg = odx.falkon._kernel_arg
    assert arg(k) is k
    g = arg(odx.GaussianKernel(5))
    assert type(g) is float and g == 5.0
    assert type(arg(odx.MaternKernel(5, float("inf")))) is float
    assert arg(types.SimpleNamespace(sigma=3)) == 3           # (a foreign kernel object with a sigma: as ever)


def test_wrappers_that_were_not_taught_the_kind_raise_type_error():
    from odx import backend
    k = odx.MaternKernel(5.0, 1.5)
    rows = types.SimpleNamespace(n=4, D=3, P=None)
    with pytest.raises(TypeError):
        backend.KnmStream(rows, rows, k)                       # the streamed shard
    me = types.SimpleNamespace(f32=lambda F: F, device=torch.device("cpu"))
    with pytest.raises(TypeError):
        backend.HipBackend.knm_rhs_sigmas(me, rows, rows, [k], None)
    with pytest.raises(TypeError):
        backend.HipBackend.mmv_sigmas(me, rows, rows, [k], torch.zeros(4, 1))
    # fit_batch / BatchFit key their chains by what precond_batched gets: the object, not its sigma
    est = odx.InCoreFalkon(kernel=k, penalty=1e-3, M=4)
    assert odx.falkon.BatchFit._key(types.SimpleNamespace(), est)[0] is k


@pytest.mark.parametrize("nu", NUS + [float("inf")])
def test_radial_kernel_against_direct_differences(nu):
    rng = np.random.default_rng(5)
    X, Z = rng.standard_normal((7, 3)) * 2.0, rng.standard_normal((5, 3)) * 2.0
    Z[2] = X[4]                                                # a centre that is a row
    for sigma in (0.7, 3.0):
        k = odx.MaternKernel(sigma, nu)
        got = radial_kernel(X, Z, k, np.float64)
        want = direct_kernel(X, Z, sigma, nu)
        assert got.shape == (7, 5) and got.dtype == np.float64
        # the Gram formula's own rounding: d^2 off by ~|x|^2 eps, and the Matern kernels take its square root
        assert np.abs(got - want).max() < 1e-6, np.abs(got - want).max()
        assert np.abs(np.delete(got, 2, axis=1) - np.delete(want, 2, axis=1)).max() < 1e-13
        assert np.all(got > 0) and np.all(got <= 1)
        kxx = radial_kernel(X, X, k, np.float64)
        assert np.abs(np.diag(kxx) - 1.0).max() < 1e-6         # k(x, x) = 1 (d^2 clamped at 0, up to the Gram rounding)
        assert radial_kernel(X[:1] * 0, X[:1] * 0, k, np.float64)[0, 0] == 1.0


def test_nu_inf_is_the_gaussian_and_a_number_falls_back():
    rng = np.random.default_rng(6)
    X, Z = rng.standard_normal((7, 3)), rng.standard_normal((5, 3))
    ref = fr.gaussian_kernel(X, Z, 2.0, np.float64)
    assert np.array_equal(radial_kernel(X, Z, odx.MaternKernel(2.0, float("inf")), np.float64), ref)
    assert np.array_equal(radial_kernel(X, Z, 2.0, np.float64), ref)
    assert radial_kernel(X.astype(np.float32), Z.astype(np.float32), odx.MaternKernel(2.0, 1.5)).dtype == np.float32


def _problem(seed=41):
    # a small, well conditioned problem: the backend multiplies by explicit inverses where the oracle solves triangular
    # systems, which differ by cond(T) eps
    X, y, rng = blob_problem(600, 36, seed=seed)
    return X, y, centres(y, 60, rng)


class _Sel:
    """A MyCenterSelector-style selector: the rows of a fixed index list."""

    def __init__(self, idx):
        self.idx = torch.as_tensor(idx)

    def select(self, Xs, Y):
        return Xs[self.idx]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("nu", NUS)
def test_solver_carries_the_kernel_object_untouched(monkeypatch, nu):
    """solver.falkon_fit / falkon_fit_path / falkon_fit_multi on the oracle backend with a Matern object equal
    falkon_ref.falkon_fit under the monkeypatch at 1e-10 relative; the Gaussian of the same width is another answer."""
    monkeypatch.setattr(fr, "gaussian_kernel", radial_kernel)
    X, y, idx = _problem()
    Xd = X.astype(np.float64)
    k = odx.MaternKernel(5.0, nu)
    lams = [1e-2, 1e-3, 3e-3]
    kw = dict(maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
    refs = [fr.falkon_fit(Xd, y.astype(np.float64), idx, k, lam, **kw)[0][:, 0] for lam in lams]
    gauss = fr.falkon_fit(Xd, y.astype(np.float64), idx, 5.0, lams[1], **kw)[0][:, 0]
    assert _rel(gauss, refs[1]) > 1e-2                          # the patched oracle did compute another kernel
    be = OracleBackend(np.float64)
    F = be.features(torch.from_numpy(X))
    Zf = be.rows(F, idx)
    one = odx.falkon_fit(be, F, be.vec(y), Zf, k, lams[1], 20).numpy()
    print("nu %g: falkon_fit rel %.2e" % (nu, _rel(one, refs[1])))
    assert _rel(one, refs[1]) < 1e-10
    path = odx.falkon_fit_path(be, F, be.vec(y), Zf, k, lams, 20).numpy()
    for l in range(len(lams)):
        print("nu %g lam %g: falkon_fit_path rel %.2e" % (nu, lams[l], _rel(path[l], refs[l])))
        assert _rel(path[l], refs[l]) < 1e-10
    Y = np.stack([y, -y, np.where(np.arange(len(y)) % 3 == 0, 1.0, -1.0)], axis=1).astype(np.float64)
    multi = odx.falkon_fit_multi(be, F, be.vec(Y), Zf, k, lams[1], 20).numpy()
    refm = fr.falkon_fit(Xd, Y, idx, k, lams[1], **kw)[0]
    for t in range(3):
        print("nu %g column %d: falkon_fit_multi rel %.2e" % (nu, t, _rel(multi[t], refm[:, t])))
        assert _rel(multi[t], refm[:, t]) < 1e-10
    # the independent oracle sees the Matern kernel through the same patch
    dense = fr.dense_nystrom_krr(Xd, y, Xd[idx], k, lams[1], jitter=1e-5 * len(idx))
    assert np.all(np.isfinite(dense))


@pytest.mark.parametrize("nu", NUS)
def test_estimators_on_the_oracle_backend(monkeypatch, nu):
    """InCoreFalkon(kernel=MaternKernel) through fit / predict / fit_path / predict_path on the oracle backend; fit_grid and
    predict_grid refuse; predict_path wants one kernel function; the estimator pickles with its kernel."""
    monkeypatch.setattr(fr, "gaussian_kernel", radial_kernel)
    X, y, idx = _problem(seed=42)
    Xd = X.astype(np.float64)
    be = OracleBackend(np.float64)
    old = odx.backend._BACKEND
    odx.set_backend(be)
    try:
        k = odx.MaternKernel(5.0, nu)
        est = odx.InCoreFalkon(kernel=k, penalty=1e-3, M=len(idx), center_selection=_Sel(idx), maxiter=20,
                               options=odx.FalkonOptions(pc_epsilon_32=1e-5, cg_epsilon_32=1e-7))
        est.fit(torch.from_numpy(X), torch.from_numpy(y))
        ref, Z = fr.falkon_fit(Xd, y.astype(np.float64), idx, k, 1e-3, maxiter=20, dtype=np.float64, pc_eps=1e-5, cg_epsilon=1e-7)
        assert _rel(est.alpha_.numpy()[:, 0], ref[:, 0]) < 1e-10
        pref = fr.falkon_predict(Xd, Z, ref, k)
        assert np.abs(est.predict(torch.from_numpy(X)).numpy() - pref).max() < 1e-5      # (the backend returns f32 scores)
        members = est.fit_path(torch.from_numpy(X), torch.from_numpy(y), [1e-2, 1e-3])
        assert all(m.kernel is k for m in members)
        assert _rel(members[1].alpha_.numpy()[:, 0], ref[:, 0]) < 1e-10
        both = odx.predict_path(members, torch.from_numpy(X))
        assert torch.equal(both[:, 1:2], members[1].predict(torch.from_numpy(X)))
        back = pickle.loads(pickle.dumps(est))
        assert back.kernel.kind == k.kind and back.kernel.nu == nu and torch.equal(back.alpha_, est.alpha_)
        with pytest.raises(NotImplementedError):
            est.fit_grid(torch.from_numpy(X), torch.from_numpy(y), [4.0, 5.0], [1e-3])
        with pytest.raises(NotImplementedError):
            odx.predict_grid(members, torch.from_numpy(X))
        import copy
        other = copy.copy(members[0])
        other.kernel = odx.GaussianKernel(5.0)
        with pytest.raises(ValueError, match="kernel function"):
            odx.predict_path([members[0], other], torch.from_numpy(X))
        other.kernel = odx.MaternKernel(5.0, 4.0 - nu)
        with pytest.raises(ValueError, match="kernel function"):
            odx.predict_path([members[0], other], torch.from_numpy(X))
        assert math.isfinite(float(both.abs().max()))
    finally:
        odx.set_backend(old)
