"""CPU tests (-m "not gpu") of the log Chebyshev-scalarised expected improvement's C ABI (include/moe_hip.h:
moe_log_ei_chebyshev_constrained_mcmc, its _multistart and _suggest) and its Python names: the three symbols are declared, exported
and in _lib.SIGNATURES with moe_ei_chebyshev_mcmc*'s argument lists plus (constraint_gps, num_constraints, thresholds) behind the
objectives, the api and module names are callable, the class carries the plain class's method names, and the feasible incumbent
computes what it says."""
import ctypes as C
import os

import numpy as np
import pytest

from cornell_moe_amd import _lib, build as moe_build

NEW = ("moe_log_ei_chebyshev_constrained_mcmc", "moe_log_ei_chebyshev_constrained_mcmc_multistart",
       "moe_log_ei_chebyshev_constrained_mcmc_suggest")
TWINS = ("moe_ei_chebyshev_mcmc", "moe_ei_chebyshev_mcmc_multistart", "moe_ei_chebyshev_mcmc_suggest")


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_the_three_symbols_are_declared_and_exported(lib):
    import cornell_moe_amd
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(cornell_moe_amd.__file__))), "include", "moe_hip.h")).read()
    for name, twin in zip(NEW, TWINS):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and ("int %s(" % name) in header, name
        res, args = _lib.SIGNATURES[name]
        tres, targs = _lib.SIGNATURES[twin]
        # (objective_gps, num_objectives | constraint_gps, num_constraints, thresholds | num_mcmc, scalarisations, best_so_far, ...)
        assert res == tres and list(args[:2]) == list(targs[:2]) and list(args[2:5]) == [_lib._GPA, C.c_int, _lib.dp], name
        assert list(args[5:]) == list(targs[2:]), name


def test_the_python_names_are_there():
    from cornell_moe_amd import api, expected_scalarised_improvement as esi
    for name in ("log_ei_chebyshev_constrained_ensemble", "log_ei_chebyshev_constrained_multistart",
                 "log_ei_chebyshev_constrained_suggest"):
        assert callable(getattr(api, name))
    for name in ("LogChebyshevExpectedImprovementMCMC", "multistart_log_chebyshev_expected_improvement_optimization",
                 "feasible_chebyshev_best_so_far"):
        assert callable(getattr(esi, name))
    for name in ("dim", "problem_size", "get_current_point", "set_current_point", "current_point", "evaluate_at_point_list",
                 "compute_objective_function", "compute_grad_objective_function", "compute_hessian_objective_function", "scalarisation",
                 "best_so_far"):
        assert hasattr(esi.ChebyshevExpectedImprovementMCMC, name)
        assert hasattr(esi.LogChebyshevExpectedImprovementMCMC, name), name
    assert hasattr(esi.LogChebyshevExpectedImprovementMCMC, "num_constraints")


def test_the_incumbent_of_the_feasible_observations():
    from cornell_moe_amd import expected_scalarised_improvement as esi
    a, b = esi.chebyshev_scalarisation([0.5, 0.5], [0.0, 0.0], [1.0, 1.0])
    y = np.array([[0.2, 0.4], [0.6, 0.1], [0.9, 0.8], [np.nan, 0.0]])  # scalarised: 0.2, 0.3, 0.45, not finite
    c = np.array([[0.5], [-0.1], [-0.2], [-1.0]])
    assert esi.feasible_chebyshev_best_so_far(y, c, [0.0], a, b) == 0.3            # row 0 is infeasible, row 3 not finite
    assert esi.feasible_chebyshev_best_so_far(y, c, [1.0], a, b) == 0.2            # every row feasible
    assert esi.feasible_chebyshev_best_so_far(y, None, None, a, b) == esi.chebyshev_best_so_far(y, a, b) == 0.2
    assert esi.feasible_chebyshev_best_so_far(y, c, [-5.0], a, b) == 0.45          # none feasible: the finite cap, never +inf
    with pytest.raises(ValueError):
        esi.feasible_chebyshev_best_so_far(y, c[:2], [0.0], a, b)
    with pytest.raises(ValueError):
        esi.feasible_chebyshev_best_so_far(y[3:], c[3:], [-5.0], a, b)


def test_shapes_that_do_not_fit_are_refused_on_the_host():
    from cornell_moe_amd import api
    with pytest.raises(api.BoundsException):
        api._log_ei_chebyshev_call([], None, None, np.zeros(4), 0.0, 1)
