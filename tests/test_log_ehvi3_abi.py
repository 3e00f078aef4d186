"""CPU tests (-m "not gpu") of the three-objective log expected hypervolume improvement's C ABI (include/moe_hip.h:
moe_log_ehvi3_constrained_mcmc, its _multistart and _suggest): the three symbols are declared, exported and in _lib.SIGNATURES with
their moe_ehvi3_constrained_mcmc* twins' signatures, the api and module names are callable, and every refusal that needs no handle
returns the code and the payload of its twin, in that function's order (tests/test_cehvi_abi.py's M = 3 list), before a handle or a
device is touched."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from cornell_moe_amd import _lib, build as moe_build

dp, ip = _lib.dp, _lib.ip

NEW = ("moe_log_ehvi3_constrained_mcmc", "moe_log_ehvi3_constrained_mcmc_multistart", "moe_log_ehvi3_constrained_mcmc_suggest")
STEM = NEW[0]
M = 3


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_the_three_symbols_are_declared_and_exported(lib):
    import cornell_moe_amd
    from cornell_moe_amd import api, expected_hypervolume_improvement as ehvi, log_expected_hypervolume_improvement as lehvi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(cornell_moe_amd.__file__))), "include", "moe_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and ("int %s(" % name) in header, name
        twin = name.replace("moe_log_ehvi3", "moe_ehvi3")
        assert twin in _lib.SIGNATURES and _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]
    for name in ("log_ehvi3_constrained_ensemble", "log_ehvi3_constrained_multistart", "log_ehvi3_constrained_suggest",
                 "_log_ehvi3_constrained_call"):
        assert callable(getattr(api, name))
    for name in ("LogExpectedHypervolumeImprovement3MCMC", "multistart_log_expected_hypervolume_improvement_3_optimization"):
        assert callable(getattr(lehvi, name))
    for name in ("dim", "problem_size", "reference_point", "front", "get_current_point", "set_current_point", "current_point",
                 "evaluate_at_point_list", "compute_expected_hypervolume_improvement", "compute_objective_function",
                 "compute_grad_expected_hypervolume_improvement", "compute_grad_objective_function",
                 "compute_hessian_objective_function"):
        assert hasattr(ehvi.ExpectedHypervolumeImprovementMCMC, name)
        assert hasattr(lehvi.LogExpectedHypervolumeImprovement3MCMC, name), name
    assert "are not built" not in lehvi.__doc__.split("Derivative observations")[0]


def test_other_numbers_of_ensembles_are_refused_naming_three_objectives():
    from cornell_moe_amd import api, log_expected_hypervolume_improvement as lehvi
    for n in (2, 4):
        with pytest.raises(ValueError) as e:
            lehvi.LogExpectedHypervolumeImprovement3MCMC([object()] * n, (1.0,) * n)
        assert "three objectives" in str(e.value) and str(n) in str(e.value)
        with pytest.raises(ValueError) as e:
            lehvi.multistart_log_expected_hypervolume_improvement_3_optimization([object()] * n, (1.0,) * n, [[0, 1]] * 2,
                                                                                 (4, 2, 1, 0, 0.7, 1.0, 0.5, 1e-8), 4)
        assert "three objectives" in str(e.value)
        with pytest.raises(api.BoundsException) as e:
            api._log_ehvi3_constrained_call([object()] * n, None, None, (1.0,) * n, None)
        assert "three objectives" in str(e.value)
    # the two-objective names still refuse three ensembles
    with pytest.raises(ValueError) as e:
        lehvi.LogExpectedHypervolumeImprovementMCMC([object()] * 3, (1.0, 1.0, 1.0))
    assert "two objectives" in str(e.value)


def _front(F):
    # the canonical order: w ascending; u descending with it, so that no point is <= another
    return np.array([(1.0 - 0.1 * i, 0.5, 0.1 * i) for i in range(max(F, 1))], dtype=np.float64)


def _args(d=2, E=1, K=1, F=2, C_=3, p=0, q=1, steps=3, domain=0):
    """valid arguments that need no handle: the arrays of handles hold NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    return dict(gps=[(C.c_void_p * max(E, 1))() for _ in range(M)], cons=(C.c_void_p * max(E * max(K, 1), 1))(), K=K,
                tau=np.full(max(K, 1), 0.25), E=E, ref=np.array([200.0, 2.0, 3.0]), front=_front(F), F=F,
                pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25), C=C_,
                out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _head(a, g):
    gps = tuple(g("gps" if r == 0 else "gps%d" % (r + 1), a["gps"][r]) for r in range(M))
    return gps + (g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), a["E"], g("ref", _p(a["ref"])), g("front", _p(a["front"])),
                  a["F"])


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return getattr(lib, STEM)(*(_head(a, g) + (g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], 1,
                                               g("ei", _p(a["out"])), g("grad", _p(a["out"])), None, C.byref(err))))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return getattr(lib, STEM + "_multistart")(*(_head(a, g) + (
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None, None, None, None,
        C.byref(err))))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return getattr(lib, STEM + "_suggest")(*(_head(a, g) + (
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])), g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    Emax, Fmax = 341, 192
    for call in (_eval, _ascent, _suggest):
        # num_mcmc first, even with everything else wrong
        for E in (0, Emax + 1):
            a = _args(C_=0, p=65, F=Fmax + 1, K=9)
            a["E"] = E
            assert call(lib, a, err, gps=True, pts=True, cons=True) == B and _payload(err) == (float(E), 1.0, float(Emax)), call.__name__
        # then NULL arrays, before the constraints' checks
        for name in ("gps", "gps2", "gps3", "ref", "pts", "front"):
            assert call(lib, _args(C_=0, p=65, K=9), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # then num_constraints outside 0 .. 8, before the product limit and the NULL arrays of K > 0
        for K in (-1, 9):
            a = _args(C_=0, p=65, F=Fmax + 1, E=Emax, K=K)
            assert call(lib, a, err, cons=True, tau=True) == B and _payload(err) == (float(K), 0.0, 8.0), (call.__name__, K)
        # then E (3 + K) > 1024: payload (num_mcmc, 1, 1024 // (3 + K))
        for E, K in ((1025 // 6, 3), (1024 // 11 + 1, 8), (Emax, 1)):
            if E * (M + K) <= 1024:
                continue
            a = _args(C_=0, p=65, F=Fmax + 1, E=E, K=K)
            a["tau"][0] = math.nan
            assert call(lib, a, err, cons=True) == B and _payload(err) == (float(E), 1.0, float(1024 // (M + K))), (call.__name__, E, K)
        a = _args(C_=0, E=205, K=2)  # 205 (3 + 2) = 1025 exactly
        assert call(lib, a, err) == B and _payload(err) == (205.0, 1.0, 204.0)
        a = _args(E=204, K=2)  # 1020: accepted as far as the NULL handle
        assert call(lib, a, err) == R and b"NULL GP handle" in err.message
        # then constraint_gps or thresholds NULL with K > 0, before the thresholds' values and the front
        for name in ("cons", "tau"):
            a = _args(C_=0, p=65, F=Fmax + 1, K=2)
            assert call(lib, a, err, **{name: True}) == R and b"constraint_gps and thresholds" in err.message, (call.__name__, name)
        # then a threshold that is not finite: payload (the value, k, 0)
        for k, bad in ((0, math.nan), (1, math.inf), (2, -math.inf)):
            a = _args(C_=0, p=65, F=Fmax + 1, K=3)
            a["tau"][k] = bad
            assert call(lib, a, err) == V and b"thresholds" in err.message and _payload(err)[1:] == (float(k), 0.0), (call.__name__, k)
            assert math.isnan(_payload(err)[0]) if math.isnan(bad) else _payload(err)[0] == bad
        # then num_front, the reference point, the front (the canonical order), num_points, the pending points
        for F in (-1, Fmax + 1):
            a = _args(C_=0, p=65)
            a["F"] = F
            a["ref"][0] = math.nan
            assert call(lib, a, err) == B and _payload(err) == (float(F), 0.0, float(Fmax)), call.__name__
        a = _args(C_=0, p=65)
        a["ref"][2] = math.inf
        a["front"][1, 0] = math.nan
        assert call(lib, a, err) == V and b"reference_point" in err.message and _payload(err)[1:] == (2.0, 0.0)
        a = _args(C_=0, p=65, F=3)
        a["front"][2] = a["front"][1]
        assert call(lib, a, err) == V and b"front" in err.message and b"canonical" in err.message and _payload(err) == (2.0, 0.0, 0.0)
        assert call(lib, _args(C_=0, p=65), err) == B and _payload(err)[:2] == (0.0, 1.0)
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        # everything that needs no handle in order: the NULL handle is next, with and without constraints (K = 0 is accepted)
        for K in (0, 1, 8):
            assert call(lib, _args(p=2, K=K), err) == R and b"NULL GP handle" in err.message, (call.__name__, K)
        assert call(lib, _args(K=0, F=0), err, cons=True, tau=True, front=True, pend=True) == R and b"NULL GP handle" in err.message
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0, K=9), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        assert call(lib, _args(steps=0, domain=1), err) == B and b"max_num_steps" in err.message
        # a simplex domain is refused under the log form's name
        assert call(lib, _args(domain=1), err) == V and b"log expected hypervolume improvement" in err.message
    for p, q, hi in ((0, 0, 65.0), (3, 63, 62.0)):
        assert _suggest(lib, _args(p=p, q=q), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
