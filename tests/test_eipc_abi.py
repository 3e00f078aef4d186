"""CPU tests (-m "not gpu") of the C ABI and the Python layer of the log expected improvement per unit cost (csrc/logeipc1.hip:
moe_log_ei_per_cost_mcmc, moe_log_ei_per_cost_mcmc_multistart, moe_log_ei_per_cost_mcmc_suggest), without a device: the three
symbols are declared, exported and described with their moe_log_ei_constrained_mcmc* twin's argument list plus (cost_gps,
cost_exponent) behind thresholds; the Python names exist; the host refuses what it can; and the library's refusals that need no
handle arrive in the header's order with their payloads."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from cornell_moe_amd import _lib, build as moe_build

dp, ip = _lib.dp, _lib.ip
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moe_hip.h")

NEW = ("moe_log_ei_per_cost_mcmc", "moe_log_ei_per_cost_mcmc_multistart", "moe_log_ei_per_cost_mcmc_suggest")
TWIN = ("moe_log_ei_constrained_mcmc", "moe_log_ei_constrained_mcmc_multistart", "moe_log_ei_constrained_mcmc_suggest")
AFTER_THRESHOLDS = 5  # gps, num_mcmc, constraint_gps, num_constraints, thresholds


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def _declared_types(text, name):
    """the parameter types of a declaration in the header, names dropped"""
    params = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S).group(1)
    return [re.sub(r"\s*\w+$", "", " ".join(q.split())) for q in params.split(",")]


def test_the_symbols_are_exported_with_the_twins_lists_plus_the_cost(lib):
    import cornell_moe_amd
    from cornell_moe_amd import api, expected_improvement_per_cost as epc, log_expected_improvement as lei
    with open(HEADER) as fh:
        text = fh.read()
    for new, twin in zip(NEW, TWIN):
        assert hasattr(lib, new) and new in _lib.SIGNATURES
        want = _declared_types(text, twin)
        want[AFTER_THRESHOLDS:AFTER_THRESHOLDS] = ["const moe_gp_t* const*", "double"]
        assert _declared_types(text, new) == want
        sig = list(_lib.SIGNATURES[twin][1])
        sig[AFTER_THRESHOLDS:AFTER_THRESHOLDS] = [_lib._GPA, C.c_double]
        assert _lib.SIGNATURES[new][0] is _lib.SIGNATURES[twin][0] and list(_lib.SIGNATURES[new][1]) == sig
        assert len(sig) == len(want)
    for name in ("log_ei_per_cost_ensemble", "log_ei_per_cost_multistart", "log_ei_per_cost_suggest", "_ei_per_cost_members"):
        assert callable(getattr(api, name))
    for name in ("LogExpectedImprovementPerCostMCMC", "multistart_log_expected_improvement_per_cost_optimization", "predicted_cost",
                 "cost_cooling_exponent"):
        assert callable(getattr(epc, name))
    assert cornell_moe_amd.expected_improvement_per_cost is epc
    twin_names = {n for n in dir(lei.LogExpectedImprovementMCMC) if not n.startswith("_")}
    mine = {n for n in dir(epc.LogExpectedImprovementPerCostMCMC) if not n.startswith("_")}
    assert twin_names <= mine and {"cost_exponent", "num_constraints"} <= mine


def test_the_cost_cooling_exponent():
    from cornell_moe_amd.expected_improvement_per_cost import cost_cooling_exponent as f
    assert f(10.0, 110.0, 10.0) == 1.0 and f(110.0, 110.0, 10.0) == 0.0 and f(60.0, 110.0, 10.0) == 0.5
    assert f(0.0, 110.0, 10.0) == 1.0 and f(500.0, 110.0, 10.0) == 0.0 and f(25.0, 100.0) == 0.75
    with pytest.raises(ValueError):
        f(0.0, 10.0, 10.0)


def _args(d=2, E=1, K=1, C_=3, p=0, q=1, steps=3, domain=0, alpha=1.0):
    """valid arguments that need no handle: the arrays of handles hold NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    return dict(gps=(C.c_void_p * max(E, 1))(), E=E, cons=(C.c_void_p * max(E * max(K, 1), 1))(), K=K, tau=np.zeros(max(K, 1)),
                cost=(C.c_void_p * max(E, 1))(), alpha=alpha, best=np.zeros(max(E, 1)), pend=np.full((max(p, 1), d), 0.5), p=p,
                pts=np.full((max(C_, 1), d), 0.25), C=C_, out=np.zeros(max(C_, 1) * (d + 1) + 64),
                bounds=np.array([[0.0, 1.0]] * d), q=q, gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain),
                iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0), found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_per_cost_mcmc(g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])),
                                        g("cost", a["cost"]), a["alpha"], g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"],
                                        g("pts", _p(a["pts"])), a["C"], 1, g("ei", _p(a["out"])), g("grad", _p(a["out"])), None,
                                        C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_per_cost_mcmc_multistart(
        g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), g("cost", a["cost"]), a["alpha"],
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"],
        g("pts", _p(a["pts"])), a["C"], ascent, g("point", _p(a["out"])), g("value", C.byref(a["val"])),
        g("found", C.byref(a["found"])), None, None, None, None, None, None, C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_per_cost_mcmc_suggest(
        g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), g("cost", a["cost"]), a["alpha"],
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"],
        g("pts", _p(a["pts"])), a["C"], ascent, a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])),
        g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    """the log constrained expected improvement's ladder with the cost's rungs: cost_gps among the NULL arrays, the product limit
    over 2 + K, the exponent behind best_so_far"""
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    for call in (_eval, _ascent, _suggest):
        # num_mcmc first, even with everything else wrong
        for E in (0, 1025):
            a = _args(C_=0, p=65, K=9, alpha=math.nan)
            a["E"] = E
            assert call(lib, a, err, gps=True, cost=True, pts=True) == B and _payload(err) == (float(E), 1.0, 1024.0), call.__name__
        # then NULL arrays, cost_gps among them, before the constraints' own checks, the exponent and the counts
        for name in ("gps", "cost", "best", "pts"):
            a = _args(C_=0, p=65, K=9, alpha=-1.0)
            assert call(lib, a, err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # then num_constraints outside 0 .. 8, before the exponent
        for K in (-1, 9):
            a = _args(C_=0, p=65, K=K, alpha=math.nan)
            assert call(lib, a, err, cons=True) == B and _payload(err) == (float(K), 0.0, 8.0), call.__name__
        # then the product limit: 1024 GPs in all, 2 + K per member
        for E, K, most in ((257, 2, 256.0), (513, 0, 512.0), (103, 8, 102.0)):
            a = _args(C_=0, p=65, E=E, K=K, alpha=math.nan)
            assert call(lib, a, err, cons=True) == B and _payload(err) == (float(E), 1.0, most) and b"2 + num_constraints" in err.message
        # (the twin's limit of 341 members at K = 2 is no longer reached: 256 pass this rung and end at the next)
        assert call(lib, _args(C_=0, p=65, E=256, K=2), err, cons=True) == R and b"constraint_gps and thresholds" in err.message
        # then constraint_gps and thresholds with K > 0
        for name in ("cons", "tau"):
            assert call(lib, _args(C_=0, p=65, alpha=-1.0), err, **{name: True}) == R and b"constraint_gps and thresholds" in err.message
        # then a threshold that is not finite, then best_so_far, both before the exponent
        a = _args(C_=0, p=65, K=3, alpha=math.nan)
        a["tau"][2] = math.inf
        a["best"][0] = math.nan
        assert call(lib, a, err) == V and b"thresholds" in err.message and _payload(err)[1:] == (2.0, 0.0), call.__name__
        for bad in (math.nan, -math.inf):
            a = _args(C_=0, p=65, E=2, alpha=math.nan)
            a["best"][1] = bad
            assert call(lib, a, err) == V and b"best_so_far" in err.message and _payload(err)[1:] == (1.0, 0.0), call.__name__
        # then the exponent: NaN, negative and +infinity are refused with payload (the value, 0, 0); 0 and +infinity's neighbours pass
        for bad in (math.nan, -1.0, math.inf, -math.inf, -1e-300):
            a = _args(C_=0, p=65, alpha=bad)
            a["best"][0] = math.inf
            assert call(lib, a, err) == V and b"cost_exponent" in err.message, (call.__name__, bad)
            got = _payload(err)
            assert (math.isnan(got[0]) if math.isnan(bad) else got[0] == bad) and got[1:] == (0.0, 0.0)
        # then num_points, before num_being_sampled
        for good in (0.0, 1.0, 1e300):
            assert call(lib, _args(C_=0, p=65, alpha=good), err) == B and _payload(err)[:2] == (0.0, 1.0)
        # then num_being_sampled outside 0 .. 64, then points_being_sampled NULL with num_being_sampled > 0
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        # everything that needs no handle in order: the NULL handle is next, with and without constraints
        for K in (0, 1, 8):
            assert call(lib, _args(p=2, K=K), err) == R and b"NULL GP handle" in err.message, (call.__name__, K)
        assert call(lib, _args(p=0, K=0), err, pend=True, cons=True, tau=True) == R and b"NULL GP handle" in err.message
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0, K=9), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        assert call(lib, _args(steps=0, domain=1), err) == B and _payload(err)[:2] == (0.0, 1.0) and b"max_num_steps" in err.message
        assert call(lib, _args(domain=1), err) == V and _payload(err)[0] == 1.0
        assert b"the log expected improvement per unit cost" in err.message
    for p, q, hi in ((0, 0, 65.0), (3, 63, 62.0)):
        assert _suggest(lib, _args(p=p, q=q, steps=0, domain=1), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)


class _NoDevice(object):
    """stands in for a DeviceGP in the checks api.py makes before the library is called: a NULL handle in dim 2"""
    _h, d = C.c_void_p(None), 2


def test_the_python_layer_checks_its_arguments(lib):
    from cornell_moe_amd import api
    g = _NoDevice()
    pts, box, gd = np.full((3, 2), 0.25), np.array([[0.0, 1.0]] * 2), (1, 3, 1, 0, 0.7, 0.1, 0.5, 1e-8)

    def calls(gps, cons, tau, cost, alpha, best):
        yield lambda: api.log_ei_per_cost_ensemble(gps, cons, tau, cost, alpha, pts, best, want_grad=True, want_log_factors=True)
        yield lambda: api.log_ei_per_cost_multistart(gps, cons, tau, cost, alpha, gd, box, best, pts)
        yield lambda: api.log_ei_per_cost_suggest(gps, cons, tau, cost, alpha, gd, box, best, pts, 2)

    # a cost ensemble of another length, or none
    for gps, cost, best in (([g], [g, g], [0.0]), ([g, g], [g], [0.0, 0.0]), ([g], [], [0.0]), ([g], None, [0.0])):
        for call in calls(gps, None, None, cost, 1.0, best):
            with pytest.raises(api.BoundsException, match="one cost GP"):
                call()
    # a bad exponent, on the host
    for bad in (math.nan, -1.0, math.inf):
        for call in calls([g], None, None, [g], bad, [0.0]):
            with pytest.raises(api.InvalidValueException, match="cost_exponent"):
                call()
    # the twin's own host checks stand in front
    for call in calls([g], [[g]], None, [g], 1.0, [0.0]):
        with pytest.raises(api.BoundsException, match="one threshold"):
            call()
    # valid shapes reach the library, which ends at the NULL handle
    for cons, tau in ((None, None), ([[g]], [0.3])):
        for call in calls([g], cons, tau, [g], 0.0, [0.0]):
            with pytest.raises(api.OptimalLearningException, match="NULL GP handle"):
                call()
    with pytest.raises(api.BoundsException, match="num_constraints"):
        api.log_ei_per_cost_ensemble([g], [[g]] * 9, [0.0] * 9, [g], 1.0, pts, [0.0])
