"""CPU tests (-m "not gpu") of the log constrained expected improvement: tests/logcei1_reference.py, the restatement
tests/test_gpu_logcei1.py checks the device against, is itself checked here -- its scalars against mpmath at 150 digits, float64
against long double on every case and shift, exp(value) against tests/cei1_reference.py -- and the inputs are QUALIFIED: the
pending points move a checked candidate's value in every case that has some, and on the stall problems the plain form and its
gradient are exactly 0 in float64 at every start while the log form climbs.  A case that breaks a condition fails; none is
skipped.  Then the C ABI's refusals in the header's order, without a device, and the Python layer's argument checks."""
import ctypes as C
import math
import os
import re

import mpmath as mp  # (the outside truth of the scalars: a machine without it fails here, it does not skip)
import numpy as np
import pytest

import cei1_reference as cr
import logcei1_reference as lr
import ms_restatement as ms
from cornell_moe_amd import _lib, build as moe_build

LD = lr.LD
dp, ip = _lib.dp, _lib.ip
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moe_hip.h")

CASE_SHIFTS = [(c, s) for c in lr.CASES for s in lr.SHIFTS] + [(c, s) for c in lr.WIDE_CASES for s in lr.WIDE_SHIFTS]
ALL_CASES = lr.CASES + lr.WIDE_CASES
IDS = ["%s-b%g-t%g" % (c.name, s[0], s[1]) for c, s in CASE_SHIFTS]

SCALAR_POINTS = list(np.linspace(-12.0, 12.0, 97)) + [-20.0, -38.5, -50.0, -100.0, -1e3, -1e5, -1e8, -1e12, -3e15, 20.0, 40.0, 100.0]


def test_the_scalars_agree_with_mpmath():
    """long double against 150 digits, relative to max(1, |true|): log h, Phi / h, phi / h, log Phi, phi / Phi"""
    mp.mp.dps = 150
    worst = dict(log_h=0.0, lam=0.0, kap=0.0, log_cdf=0.0, ratio=0.0)

    def err(got, true):
        return float(abs(mp.mpf(repr(float(got))) + mp.mpf(repr(float(got - LD(float(got))))) - true) / max(1, abs(true)))

    for x in SCALAR_POINTS:
        c = mp.mpf(float(x))
        P, p = mp.ncdf(c), mp.npdf(c)
        h = c * P + p
        got = lr.log_h_parts(x, LD) + lr.log_cdf_parts(x, LD)
        true = (mp.log(h), P / h, p / h, mp.log(P), p / P)
        for key, g, t in zip(("log_h", "lam", "kap", "log_cdf", "ratio"), got, true):
            worst[key] = max(worst[key], err(g, t))
            assert np.isfinite(g), (key, x)
    print("long double - mpmath, relative to max(1, |true|): " + " ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1e-14


def test_the_scalars_are_continuous_across_the_switch():
    """both sides of the restatement's switch at -3 and of the device's at -6 and 0: long double to the bound of the comparison with
    mpmath, float64 (the direct form cancels a digit and a half at -3) to the bound its restatement has to keep against long double"""
    for T, tol in ((LD, 1e-14), (np.float64, 2.5e-11)):
        for at in (lr.FRACTION_BELOW, -6.0, 0.0):
            lo, hi = np.nextafter(at, -np.inf), at
            for f in (lr.log_h_parts, lr.log_cdf_parts):
                for a, b in zip(f(lo, T), f(hi, T)):
                    assert abs(float(a - b)) <= tol * max(1.0, abs(float(b))), (T, at, f.__name__)


@pytest.mark.parametrize("case,shift", CASE_SHIFTS, ids=IDS)
def test_float64_agrees_with_long_double(case, shift):
    p, want = lr.expected(case, shift, LD)
    _, got = lr.expected(case, shift, np.float64)
    worst_v = worst_g = worst_f = 0.0
    low_c, low_v, big_g = 0.0, 0.0, 0.0
    for i in p.checked:
        w, g = want[i], got[i]
        assert np.isfinite(float(g.value)) and np.all(np.isfinite(g.grad.astype(np.float64)))
        worst_v = max(worst_v, abs(float(g.value - w.value)) / max(1.0, abs(float(w.value))))
        gmax = float(np.max(np.abs(w.grad)))
        worst_g = max(worst_g, float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / max(1.0, gmax))
        worst_f = max(worst_f, max(abs(float(a - b)) / max(1.0, abs(float(b)))
                                   for ra, rb in zip(g.log_factors, w.log_factors) for a, b in zip(ra, rb)))
        low_c = min([low_c] + [a for row in w.args for a in row])
        low_v, big_g = min(low_v, float(w.value)), max(big_g, gmax)
    print("%s %s: float64 - long double, value %.2e grad %.2e log factors %.2e (relative); lowest c or z %.1f, lowest value %.1f, "
          "largest |grad| %.3g" % (case.name, shift, worst_v, worst_g, worst_f, low_c, low_v, big_g))
    assert worst_v <= 2.5e-11 and worst_g <= 2.5e-11 and worst_f <= 2.5e-11


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_exp_of_the_value_is_the_plain_form(case):
    """shift (0, 0), long double: exp(value) is tests/cei1_reference.py's value, the log factors the logs of its factors"""
    p, want = lr.expected(case, lr.SHIFTS[0], LD)
    _, plain = cr.expected(case, LD)
    worst = 0.0
    for i in p.checked:
        A, v = plain[i].value, want[i].value
        assert float(A) > 0
        worst = max(worst, abs(float(np.exp(v) - A)) / (max(1.0, abs(float(np.log(A)))) * min(1.0, float(A))))
        assert [float(b) for b in want[i].bprime] == [float(b) for b in plain[i].bprime]
    print("%s: exp(value) - plain value %.2e (relative to max(1, |log|) times the value)" % (case.name, worst))
    assert worst <= 1e-15


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c.p], ids=[c.name for c in ALL_CASES if c.p])
def test_the_pending_points_move_the_value(case):
    p0 = lr.make_problem(case)
    bare = cr.ensemble(p0, LD, pending=p0.pending[:0])
    for shift in (lr.WIDE_SHIFTS if case in lr.WIDE_CASES else lr.SHIFTS):
        p, want = lr.expected(case, shift, LD)
        without = lr.relimited(bare, p.best, p.thresholds)
        moved = max(abs(float(lr.evaluate(without, p.points[i]).value - want[i].value)) for i in p.checked)
        print("%s %s: the pending points move a checked value by %.3g" % (case.name, shift, moved))
        assert moved >= 1e-5, (case.name, shift)


def _regime_errors(T_got, near):
    p, limits, want = lr.regime_expected(LD, near)
    _, _, got = lr.regime_expected(T_got, near)
    e_v = [abs(float(g.value - w.value)) / max(1.0, abs(float(w.value))) for g, w in zip(got, want)]
    e_g = [float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / max(1.0, float(np.max(np.abs(w.grad)))) for g, w in zip(got, want)]
    return want, e_v, e_g


def test_the_scalar_regimes_are_reached_and_qualified():
    """every candidate's c and z inside its interval in long double, float64 within 2.5e-11 of long double at every candidate"""
    want, e_v, e_g = _regime_errors(np.float64, lr.REGIME_NEAR)
    n = len(lr.REGIMES)
    for i, w in enumerate(want):
        c, z = w.args[0]
        (clo, chi), (zlo, zhi) = lr.REGIMES[i], lr.REGIMES[(i + 3) % n]
        print("candidate %d: c %.6g z %.6g value %.6g, float64 - long double value %.2e grad %.2e" % (i, c, z, float(w.value), e_v[i], e_g[i]))
        assert clo < c < chi and zlo < z < zhi, (i, c, z)
    assert max(e_v) <= 2.5e-11 and max(e_g) <= 2.5e-11
    assert e_v[1] <= 2.5e-12 and e_g[1] <= 2.5e-12  # (the candidate beside a sampled point: a tenth, logcei1_reference.REGIME_NEAR)
    # a small sigma alone does not carry c below -1e4 within that bound: the ladder of distances to the sampled point.  With
    # |b' - mu| at most 0.5, c < -1e4 needs sigma < 5e-5, the point within 1e-5: that rung and the next part by far more than 2.5e-11.
    ladder = {}
    for near in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
        _, v, g = _regime_errors(np.float64, near)
        p, _, _ = lr.regime_expected(LD, near)
        m = lr.ensemble(p, LD)[0]
        sigma = float(np.sqrt(lr.moments(m.models[0], m.bases[0], p.points[1])[1]))
        ladder[near] = (sigma, v[1], g[1])
        print("candidate 1 at %.0e from a sampled point: sigma %.3g, float64 - long double value %.2e grad %.2e" % (near, sigma, v[1], g[1]))
    assert ladder[1e-4][0] > 5e-5 > ladder[1e-6][0]
    for near in (1e-5, 1e-6):  # (the rungs around and below sigma = 5e-5)
        assert ladder[near][1] > 2.5e-11 and ladder[near][2] > 2.5e-11, near


def test_gradient_agrees_with_central_differences():
    """long double, the ensemble case at the deepest shift: relative to the gradient's size"""
    case, shift = cr.case(cr.ENSEMBLE), lr.SHIFTS[2]
    p, want = lr.expected(case, shift, LD)
    _, members = lr.shifted(case, shift, LD)
    h, worst = 1e-6, 0.0
    for i in p.checked[:2]:
        x = p.points[i]
        for j in range(len(x)):
            hi, lo = x.copy(), x.copy()
            hi[j] += h
            lo[j] -= h
            fd = (lr.evaluate(members, hi).value - lr.evaluate(members, lo).value) / LD(hi[j] - lo[j])
            worst = max(worst, abs(float(fd - want[i].grad[j])) / max(1.0, float(np.max(np.abs(want[i].grad)))))
    print("gradient - central differences %.2e (relative)" % worst)
    assert worst <= 1e-6


def test_one_member_without_constraints_is_its_own_log():
    """E = 1, K = 0: the value is the member's l and the gradient its gradient, exactly"""
    case = cr.case("e1_k1_d3_n20_p3")
    for T in (LD, np.float64):
        _, members = lr.shifted(case, lr.SHIFTS[1], T, constraints=False)
        for x in lr.make_problem(case).points:
            got = lr.evaluate(members, x)
            vals, grads, _ = lr.member_logs(members[0], x)
            assert len(vals) == 1 and got.value == vals[0] and np.array_equal(got.grad, grads[0])


@pytest.mark.parametrize("name", lr.STALL_CASES)
def test_the_plain_form_stalls_and_the_log_form_climbs(name):
    p, members = lr.stall(name, np.float64)
    starts = lr.stall_starts(p.points.shape[1])
    low = 0.0
    for x in starts:
        plain = cr.evaluate(members, x)
        assert float(plain.value) == 0.0 and not np.any(plain.grad), (name, x)
        low = min([low] + [row[0] for row in lr.evaluate(members, x).args])
    start_values = np.array([float(lr.evaluate(members, x).value) for x in starts])
    assert np.all(np.isfinite(start_values))
    bounds = np.array([[0.0, 1.0]] * starts.shape[1])
    _, best, found = ms.multistart_best(lambda X: np.array([float(lr.evaluate(members, x).value) for x in X]),
                                        lambda X: np.array([lr.evaluate(members, x).grad for x in X], dtype=np.float64),
                                        lr.STALL_GD, bounds, starts)
    print("%s: lowest c %.0f, best start value %.6g, after the ascent %.6g (gain %.3g)"
          % (name, low, start_values.max(), best, best - start_values.max()))
    assert found and best >= start_values.max() + lr.STALL_GAIN


# ---- the C ABI without a device ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


NEW = ("moe_log_ei_constrained_mcmc", "moe_log_ei_constrained_mcmc_multistart", "moe_log_ei_constrained_mcmc_suggest")
OLD = ("moe_ei_constrained_mcmc", "moe_ei_constrained_mcmc_multistart", "moe_ei_constrained_mcmc_suggest")


def _declared_types(text, name):
    """the parameter types of a declaration in the header, names dropped"""
    params = re.search(r"\bint %s\(([^;]*?)\);" % name, text, re.S).group(1)
    return [re.sub(r"\s*\w+$", "", " ".join(q.split())) for q in params.split(",")]


def test_the_new_symbols_are_exported_with_the_constrained_signatures(lib):
    import cornell_moe_amd
    from cornell_moe_amd import api, expected_improvement_constrained as eic, log_expected_improvement as lei
    with open(HEADER) as fh:
        text = fh.read()
    for new, old in zip(NEW, OLD):
        assert hasattr(lib, new) and new in _lib.SIGNATURES
        assert _declared_types(text, new) == _declared_types(text, old)
        assert _lib.SIGNATURES[new][0] is _lib.SIGNATURES[old][0] and list(_lib.SIGNATURES[new][1]) == list(_lib.SIGNATURES[old][1])
        assert len(_lib.SIGNATURES[new][1]) == len(_declared_types(text, new))
    for name in ("log_ei_constrained_ensemble", "log_ei_constrained_multistart", "log_ei_constrained_suggest"):
        assert callable(getattr(api, name))
    for name in ("LogExpectedImprovementMCMC", "multistart_log_expected_improvement_optimization"):
        assert callable(getattr(lei, name))
    assert lei.best_feasible_value is eic.best_feasible_value
    assert cornell_moe_amd.log_expected_improvement is lei


def _args(d=2, E=1, K=1, C_=3, p=0, q=1, steps=3, domain=0):
    """valid arguments that need no handle: the arrays of handles hold NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    return dict(gps=(C.c_void_p * max(E, 1))(), E=E, cons=(C.c_void_p * max(E * max(K, 1), 1))(), K=K, tau=np.zeros(max(K, 1)),
                best=np.zeros(max(E, 1)), pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25), C=C_,
                out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_constrained_mcmc(g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])),
                                           g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"],
                                           1, g("ei", _p(a["out"])), g("grad", _p(a["out"])), None, C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_constrained_mcmc_multistart(
        g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), g("gd", C.byref(a["gd"])),
        g("bounds", _p(a["bounds"])), g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None, None, None, None,
        C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_constrained_mcmc_suggest(
        g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), g("gd", C.byref(a["gd"])),
        g("bounds", _p(a["bounds"])), g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])), g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    """the constrained expected improvement's ladder, rung for rung, under the new objective's name"""
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    for call in (_eval, _ascent, _suggest):
        # num_mcmc first, even with everything else wrong
        for E in (0, 1025):
            a = _args(C_=0, p=65, K=9)
            a["E"] = E
            assert call(lib, a, err, gps=True, pts=True) == B and _payload(err) == (float(E), 1.0, 1024.0), call.__name__
        # then NULL arrays, before the constraints' own checks and the counts
        for name in ("gps", "best", "pts"):
            assert call(lib, _args(C_=0, p=65, K=9), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # then num_constraints outside 0 .. 8
        for K in (-1, 9):
            assert call(lib, _args(C_=0, p=65, K=K), err, cons=True) == B and _payload(err) == (float(K), 0.0, 8.0), call.__name__
        # then the product limit: 1024 GPs in all
        a = _args(C_=0, p=65, E=342, K=2)
        assert call(lib, a, err, cons=True) == B and _payload(err) == (342.0, 1.0, 341.0) and b"1 + num_constraints" in err.message
        # then constraint_gps and thresholds with K > 0 (neither is asked for with K = 0)
        for name in ("cons", "tau"):
            assert call(lib, _args(C_=0, p=65), err, **{name: True}) == R and b"constraint_gps and thresholds" in err.message
        # then a threshold that is not finite
        for bad in (math.nan, math.inf, -math.inf):
            a = _args(C_=0, p=65, K=3)
            a["tau"][2] = bad
            a["best"][0] = math.nan
            assert call(lib, a, err) == V and b"thresholds" in err.message and _payload(err)[1:] == (2.0, 0.0), call.__name__
        # then best_so_far: NaN and -infinity are refused, +infinity is "no feasible observation yet"
        for bad in (math.nan, -math.inf):
            a = _args(C_=0, p=65, E=2)
            a["best"][1] = bad
            assert call(lib, a, err) == V and b"best_so_far" in err.message and _payload(err)[1:] == (1.0, 0.0), call.__name__
        a = _args(C_=0, p=65)
        a["best"][0] = math.inf
        # then num_points, before num_being_sampled
        assert call(lib, a, err) == B and _payload(err)[:2] == (0.0, 1.0)
        # then num_being_sampled outside 0 .. 64
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        # then points_being_sampled NULL with num_being_sampled > 0
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        # everything that needs no handle in order: the NULL handle is next, with and without constraints
        for K in (0, 1, 8):
            assert call(lib, _args(p=2, K=K), err) == R and b"NULL GP handle" in err.message, (call.__name__, K)
        assert call(lib, _args(p=0, K=0), err, pend=True, cons=True, tau=True) == R and b"NULL GP handle" in err.message
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0, K=9), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # max_num_steps < 1 after the pending checks and before the domain type; not asked for without the ascent
        assert call(lib, _args(steps=0, domain=1, p=65), err) == B and _payload(err) == (65.0, 0.0, 64.0)
        assert call(lib, _args(steps=0, domain=1), err) == B and _payload(err)[:2] == (0.0, 1.0) and b"max_num_steps" in err.message
        assert call(lib, _args(steps=0, domain=1), err, ascent=0) == V and b"tensor-product" in err.message
        assert call(lib, _args(domain=1), err) == V and _payload(err)[0] == 1.0
        assert b"the log constrained expected improvement" in err.message
    # the batch: num_to_sample directly after num_being_sampled, before the NULL pending array, the steps and the domain
    for p, q, hi in ((0, 0, 65.0), (0, 66, 65.0), (3, 63, 62.0), (64, 2, 1.0)):
        assert _suggest(lib, _args(p=p, q=q, steps=0, domain=1), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
    assert _suggest(lib, _args(p=65, q=0), err) == B and _payload(err) == (65.0, 0.0, 64.0)


class _NoDevice(object):
    """stands in for a DeviceGP in the checks api.py makes before the library is called: a NULL handle in dim 2"""
    _h, d = C.c_void_p(None), 2


def test_the_python_layer_checks_its_arguments(lib):
    from cornell_moe_amd import api
    g = _NoDevice()
    pts, box, gd = np.full((3, 2), 0.25), np.array([[0.0, 1.0]] * 2), (1, 3, 1, 0, 0.7, 0.1, 0.5, 1e-8)

    def calls(gps, cons, tau, best):
        yield lambda: api.log_ei_constrained_ensemble(gps, cons, tau, pts, best, want_grad=True, want_log_factors=True)
        yield lambda: api.log_ei_constrained_multistart(gps, cons, tau, gd, box, best, pts)
        yield lambda: api.log_ei_constrained_suggest(gps, cons, tau, gd, box, best, pts, 2)

    for gps, cons, tau, best, what in (([], None, None, [], "one best value"), ([g], None, None, [0.0, 0.0], "one best value"),
                                       ([g], [[g]], None, [0.0], "one threshold"), ([g], None, [0.0], [0.0], "one threshold"),
                                       ([g, g], [[g]], [0.0], [0.0, 0.0], "one constraint GP")):
        for call in calls(gps, cons, tau, best):
            with pytest.raises(api.BoundsException, match=what):
                call()
    # constraint_gps = None / thresholds = None is K = 0: the call reaches the library, which ends at the NULL handle
    for cons, tau in ((None, None), ([[g]], [0.3])):
        for call in calls([g], cons, tau, [0.0]):
            with pytest.raises(api.OptimalLearningException, match="NULL GP handle"):
                call()
    # the library's own refusals arrive as the constrained expected improvement's exceptions
    with pytest.raises(api.InvalidValueException, match="best_so_far"):
        api.log_ei_constrained_ensemble([g], None, None, pts, [-math.inf])
    with pytest.raises(api.BoundsException, match="num_constraints"):
        api.log_ei_constrained_ensemble([g], [[g]] * 9, [0.0] * 9, pts, [0.0])
