"""odx — MI355X-native hot path of hsp-iit/online-detection (FALKON classifiers, RLS box
regressors, scoring) behind the reference's Python module API.  See DESIGN.md."""
from . import hip  # noqa: F401  (ctypes binding; loading is lazy)
from . import options  # noqa: F401  (the one options table: odx.options.current() / set() / override())
from .backend import get_backend, set_backend  # noqa: F401
from .solver import SolverOptions, cv_folds, falkon_fit, falkon_fit_cv, falkon_fit_grid, falkon_fit_lockstep, falkon_fit_multi, falkon_fit_path, falkon_fit_stats, falkon_fit_stats_multi, falkon_fit_stats_path  # noqa: F401
from .falkon import Falkon, FalkonOptions, GaussianKernel, InCoreFalkon, MaternKernel, predict_grid, predict_path  # noqa: F401
from .leverage import LeverageSelector, leverage_scores  # noqa: F401
from .incremental import IncrementalFalkon  # noqa: F401
from .logistic import LogisticFalkon, LogisticLoss, falkon_fit_logistic  # noqa: F401
from .weighted import falkon_fit_weighted  # noqa: F401

__all__ = ["hip", "options", "get_backend", "set_backend", "SolverOptions", "falkon_fit", "falkon_fit_lockstep", "falkon_fit_path", "falkon_fit_multi", "falkon_fit_grid", "falkon_fit_cv", "falkon_fit_stats", "falkon_fit_stats_multi", "falkon_fit_stats_path", "cv_folds", "Falkon", "InCoreFalkon",
           "GaussianKernel", "MaternKernel", "FalkonOptions", "predict_path", "predict_grid", "leverage_scores", "LeverageSelector", "IncrementalFalkon", "LogisticFalkon", "LogisticLoss",
           "falkon_fit_logistic", "falkon_fit_weighted"]
