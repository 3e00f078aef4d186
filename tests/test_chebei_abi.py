"""CPU tests (-m "not gpu") of the Chebyshev-scalarised expected improvement's C ABI (include/moe_hip.h: moe_ei_chebyshev_mcmc, its
_multistart and _suggest) and its Python names: the three symbols are declared, exported and in _lib.SIGNATURES with
moe_ehvi3_mcmc*'s argument lists but for the objective's own arguments, the api and module names are callable, the class carries
the method names of ExpectedHypervolumeImprovement3MCMC, and the module's helpers compute what they say."""
import ctypes as C
import os

import numpy as np
import pytest

from cornell_moe_amd import _lib, build as moe_build

NEW = ("moe_ei_chebyshev_mcmc", "moe_ei_chebyshev_mcmc_multistart", "moe_ei_chebyshev_mcmc_suggest")
TWINS = ("moe_ehvi3_mcmc", "moe_ehvi3_mcmc_multistart", "moe_ehvi3_mcmc_suggest")


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
        # (objective_gps, num_objectives, num_mcmc, scalarisations, best_so_far) in the place of (gps, gps2, gps3, num_mcmc,
        # reference_point, front, num_front); everything behind is the twin's
        assert res == tres and list(args[:5]) == [_lib._GPA, C.c_int, C.c_int, _lib.dp, _lib.dp] and list(args[5:]) == list(targs[7:]), name


def test_the_python_names_are_there():
    from cornell_moe_amd import api, expected_hypervolume_improvement as ehvi, expected_scalarised_improvement as esi
    for name in ("ei_chebyshev_ensemble", "ei_chebyshev_multistart", "ei_chebyshev_suggest"):
        assert callable(getattr(api, name))
    for name in ("chebyshev_scalarisation", "chebyshev_best_so_far", "sample_simplex_weights", "ChebyshevExpectedImprovementMCMC",
                 "multistart_chebyshev_expected_improvement_optimization"):
        assert callable(getattr(esi, name))
    for name in ("dim", "problem_size", "get_current_point", "set_current_point", "current_point", "evaluate_at_point_list",
                 "compute_objective_function", "compute_grad_objective_function", "compute_hessian_objective_function"):
        assert hasattr(ehvi.ExpectedHypervolumeImprovement3MCMC, name)
        assert hasattr(esi.ChebyshevExpectedImprovementMCMC, name), name


def test_the_scalarisation_the_incumbent_and_the_weights():
    from cornell_moe_amd import expected_scalarised_improvement as esi
    a, b = esi.chebyshev_scalarisation([0.2, 0.3, 0.5], [-1.0, 0.0, 2.0], [1.0, 2.0, 4.0])
    assert np.array_equal(a, np.array([0.2, 0.3, 0.5]) / 2.0) and np.array_equal(b, -a * np.array([-1.0, 0.0, 2.0]))
    # the ideal point scalarises to 0, the nadir point to the largest weight
    assert np.max(a * np.array([-1.0, 0.0, 2.0]) + b) == 0.0 and np.max(a * np.array([1.0, 2.0, 4.0]) + b) == 0.5
    for bad in (([0.5, 0.0], [0, 0], [1, 1]), ([0.5, 0.5], [0, 1], [1, 1]), ([0.5, np.nan], [0, 0], [1, 1]), ([1.0], [0, 0], [1, 1])):
        with pytest.raises(ValueError):
            esi.chebyshev_scalarisation(*bad)
    y = np.array([[0.0, 1.0, 3.0], [1.0, 0.5, 2.5], [np.nan, 0.0, 2.0]])
    g = np.max(a[None, :] * y[:2] + b[None, :], axis=1)
    assert esi.chebyshev_best_so_far(y, a, b) == float(np.min(g))
    with pytest.raises(ValueError):
        esi.chebyshev_best_so_far(y[2:], a, b)
    w = esi.sample_simplex_weights(5, 4, 3)
    assert w.shape == (5, 4) and np.all(w > 0.0) and np.allclose(np.sum(w, axis=1), 1.0)
    assert np.array_equal(w, esi.sample_simplex_weights(5, 4, 3)) and not np.array_equal(w, esi.sample_simplex_weights(5, 4, 4))


def test_shapes_that_do_not_fit_are_refused_on_the_host():
    from cornell_moe_amd import api
    with pytest.raises(api.BoundsException):
        api._ei_chebyshev_call([], np.zeros(4), 0.0, 1)
