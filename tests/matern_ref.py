"""The f64 statement of the radial kernels of odx.MaternKernel — TEST ORACLE ONLY.

``radial_kernel`` has the signature of ``oracle.falkon_ref.gaussian_kernel`` with a kernel object (``.sigma``, ``.nu``)
where that takes a number, and falls back to it for a number.  A test runs the WHOLE f64 oracle on a Matern kernel by
``monkeypatch.setattr(falkon_ref, "gaussian_kernel", radial_kernel)``: Preconditioner, falkon_fit, falkon_predict,
dense_nystrom_krr and tests/oracle_backend.py all look the function up in that module and hand their sigma through
untouched.

With d^2 = max(0, |x|^2 + |z|^2 - 2 x.z) (the Gram formula and the clamp of gaussian_kernel) and u = sqrt(2 nu d^2) / sigma:
    nu = 3/2   k = (1 + u) exp(-u)
    nu = 5/2   k = (1 + u + u^2 / 3) exp(-u)
    nu = inf   the Gaussian exp(-d^2 / (2 sigma^2))
"""
import numpy as np

from oracle import falkon_ref

_gaussian_kernel = falkon_ref.gaussian_kernel          # the function itself: the name in the module may be patched to radial_kernel


def radial_kernel(X1, X2, kernel_or_sigma, dtype=None):
    nu = getattr(kernel_or_sigma, "nu", None)
    if nu is None:
        return _gaussian_kernel(X1, X2, kernel_or_sigma, dtype)
    sigma = float(kernel_or_sigma.sigma)
    if np.isinf(nu):
        return _gaussian_kernel(X1, X2, sigma, dtype)
    if nu not in (1.5, 2.5):
        raise ValueError("radial_kernel: nu = %r" % (nu,))
    dtype = np.dtype(dtype or X1.dtype)
    X1 = np.asarray(X1, dtype=dtype)
    X2 = np.asarray(X2, dtype=dtype)
    sq1 = np.sum(X1 * X1, axis=1, dtype=dtype)[:, None]
    sq2 = np.sum(X2 * X2, axis=1, dtype=dtype)[None, :]
    D2 = X1 @ X2.T
    D2 *= dtype.type(-2.0)
    D2 += sq1
    D2 += sq2
    np.maximum(D2, 0, out=D2)
    U = np.sqrt(D2 * dtype.type(2.0 * nu)) / dtype.type(sigma)
    P = 1 + U if nu == 1.5 else 1 + U + U * U / dtype.type(3.0)
    return (P * np.exp(-U)).astype(dtype, copy=False)


def direct_kernel(X1, X2, sigma, nu):
    """The same kernels from the differences themselves (f64, no Gram formula): what radial_kernel is checked against."""
    X1, X2 = np.asarray(X1, dtype=np.float64), np.asarray(X2, dtype=np.float64)
    r = np.sqrt(((X1[:, None, :] - X2[None, :, :]) ** 2).sum(-1))
    if np.isinf(nu):
        return np.exp(-r * r / (2.0 * sigma * sigma))
    u = np.sqrt(2.0 * nu) * r / sigma
    return ((1 + u) if nu == 1.5 else (1 + u + u * u / 3.0)) * np.exp(-u)
