"""CPU tests (-m "not gpu") of the constrained expected improvement: tests/cei1_reference.py, the restatement
tests/test_gpu_cei1.py checks the device against, is itself checked here -- float64 against long double, the gradient against
central differences of the long-double value, K = 0 against tests/ei1_reference.py -- and every case is QUALIFIED: at its checked
candidates the feasibility factors are neither 0 nor 1, the value and the gradient are far above the device test's tolerance, and
dropping the constraints or the pending points moves the value by far more than that tolerance, so that a device which returned
zeros, ignored the constraints or ignored P could not pass.  A case that breaks a condition fails; none is skipped.  Then the C
ABI's refusals in the header's order, without a device, and best_feasible_value."""
import ctypes as C
import math

import numpy as np
import pytest

import cei1_reference as cr
import ei1_reference as er
import kg1_pending_reference as kp
import kg1_reference as kr
from cornell_moe_amd import _lib, build as moe_build

LD = cr.LD
dp, ip = _lib.dp, _lib.ip

CASES = cr.CASES + cr.WIDE_CASES


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_float64_agrees_with_long_double(case):
    p, want = cr.expected(case, LD)
    _, got = cr.expected(case, np.float64)
    worst_v = worst_g = worst_f = 0.0
    for w, g in zip(want, got):
        worst_v = max(worst_v, abs(float(g.value - w.value)) / w.scale)
        worst_g = max(worst_g, float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / w.scale)
        worst_f = max(worst_f, max(abs(float(a - b)) for ra, rb in zip(g.factors, w.factors) for a, b in zip(ra, rb)) / w.scale)
    print("%s: float64 - long double, value %.2e grad %.2e factors %.2e (scale)" % (case.name, worst_v, worst_g, worst_f))
    assert worst_v <= 2.5e-11 and worst_g <= 2.5e-11 and worst_f <= 2.5e-11


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_gradient_agrees_with_central_differences(case):
    p, want = cr.expected(case, LD)
    members = cr.ensemble(p, LD)
    h = 1e-6
    worst = 0.0
    for i in p.checked[:3]:
        x = p.points[i]
        for j in range(len(x)):
            hi, lo = x.copy(), x.copy()
            hi[j] += h
            lo[j] -= h
            fd = (cr.evaluate(members, hi).value - cr.evaluate(members, lo).value) / LD(hi[j] - lo[j])
            worst = max(worst, abs(float(fd - want[i].grad[j])))
    print("%s: gradient - central differences %.2e" % (case.name, worst))
    assert worst <= 1e-7


@pytest.mark.parametrize("T", (LD, np.float64), ids=("long_double", "float64"))
def test_without_constraints_it_is_ei1_reference_exactly(T):
    p = cr.make_problem(cr.case(cr.ENSEMBLE))
    members = cr.ensemble(p, T, constraints=False)
    bases = [kr.Model(g[0].cov_type, g[0].hyper, g[0].X, g[0].y, g[0].noise, T) for g in p.gps]
    models = [kp.PendingModel(b, p.pending) for b in bases]
    for x in p.points:
        got = cr.evaluate(members, x)
        res = [er.evaluate_model(mm, m, p.pending, x, b) for mm, m, b in zip(models, bases, p.best)]
        value, grad = T(0), np.zeros(len(x), dtype=T)
        for r in res:
            value, grad = value + r.value, grad + r.grad
        assert got.value == value / T(len(res)) and np.array_equal(got.grad, grad / T(len(res)))
        assert [row[0] for row in got.factors] == [r.value for r in res]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_every_case_is_qualified(case):
    p, want = cr.expected(case, LD)
    assert len(p.checked) >= 3
    free = cr.ensemble(p, LD, constraints=False)
    bare = cr.ensemble(p, LD, pending=p.pending[:0])
    for i in p.checked:
        w, x = want[i], p.points[i]
        F = [float(f) for row in w.factors for f in row[1:]]
        assert len(F) == case.E * case.K and all(0.02 <= f <= 0.98 for f in F), (case.name, i, F)
        assert float(w.value) >= 1e-3 * w.scale, (case.name, i)
        assert float(np.max(np.abs(w.grad))) >= 1e-2, (case.name, i)
        assert abs(float(cr.evaluate(free, x).value - w.value)) >= 1e-3 * w.scale, (case.name, i)
        if case.p:
            assert abs(float(cr.evaluate(bare, x).value - w.value)) >= 1e-5 * w.scale, (case.name, i)


def test_the_wide_case_stages_unequal_members_at_a_wide_padded_dimension():
    from test_ei1_reference import padded_dim
    c = cr.WIDE
    assert c.E == 3 and c.K == 2 and c.p == 3 and c.C == 6 and padded_dim(c.d) == 24 and c.d % 8
    assert all(sorted(row) == [20, 300, 600] for row in c.n) and len({row for row in c.n}) == 3
    assert all(len({row[r] for row in c.n}) == 3 for r in range(3))  # (every role sees every row count)
    # the believed-feasible rule takes both branches among the members: some pending point lowers an incumbent, another member's stays
    for T in (LD, np.float64):
        members = cr.ensemble(cr.make_problem(c), T)
        assert any(m.mask.any() and float(m.bprime) < m.best - 1e-3 for m in members)
        assert any(not m.mask.any() and float(m.bprime) == m.best for m in members)
        for m in members:
            assert min(abs(float(v) - t) for base, t in zip(m.bases[1:], m.taus) for v in cr.mean_at(base, m.P)) >= 1e-3


def test_both_branches_of_the_incumbent_rule_bind():
    """under member 0 pending point 0 is believed feasible and lowers the incumbent; under member 1 it is believed infeasible and the
    incumbent stays, although the believed objective value lies below it"""
    for T in (LD, np.float64):
        p = cr.make_problem(cr.case(cr.MIXED))
        m0, m1 = cr.ensemble(p, T)
        assert m0.mask[0] and float(m0.bprime) < p.best[0] - 1e-3
        assert not m1.mask.any() and float(m1.bprime) == p.best[1]
        assert float(min(cr.mean_at(m1.bases[0], m1.P))) < p.best[1] - 1e-3
        # the margins of the beliefs are far above any rounding
        for m in (m0, m1):
            assert min(abs(float(v) - p.thresholds[0]) for v in cr.mean_at(m.bases[1], m.P)) >= 1e-3


def test_a_member_without_a_feasible_observation():
    for T in (LD, np.float64):
        p = cr.make_problem(cr.case(cr.INF))
        m0, m1 = cr.ensemble(p, T)
        assert math.isinf(p.best[0]) and np.isinf(m0.bprime) and not m0.mask.any() and math.isfinite(m0.scale)
        vals, grads = m0.factors(p.points[0])
        assert vals[0] == 1 and not np.any(grads[0])  # the member's acquisition is its probability of feasibility
        a, _, _ = m0.evaluate(p.points[0])
        assert a == vals[1]
        q = cr.make_problem(cr.case(cr.INF_FEASIBLE))
        n0 = cr.ensemble(q, T)[0]
        assert math.isinf(q.best[0]) and n0.mask[0] and np.isfinite(n0.bprime)
        assert min(abs(float(v) - q.thresholds[0]) for m in (m0, n0) for v in cr.mean_at(m.bases[1], m.P)) >= 1e-3


def test_best_feasible_value():
    from cornell_moe_amd import expected_improvement_constrained as eic
    y = np.array([3.0, 1.0, 2.0, 0.5])
    c = np.array([[0.1, 0.0], [0.3, 0.0], [0.2, -1.0], [0.0, 0.5]])
    assert eic.best_feasible_value(y, c, [0.25, 0.1]) == 2.0       # rows 0 and 2 are feasible
    assert eic.best_feasible_value(y, c, [0.3, 0.5]) == 0.5        # all are: the bound itself is feasible
    assert eic.best_feasible_value(y, c, [-1.0, 0.0]) == math.inf  # none is
    assert eic.best_feasible_value(y, c[:, 0], [0.05]) == 0.5      # one constraint as a vector
    assert eic.best_feasible_value(y.reshape(-1, 1), np.zeros((4, 0)), []) == 0.5  # no constraints
    with pytest.raises(ValueError):
        eic.best_feasible_value(y, c, [0.0])


# ---- the C ABI without a device ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


NEW = ("moe_ei_constrained_mcmc", "moe_ei_constrained_mcmc_multistart", "moe_ei_constrained_mcmc_suggest")


def test_the_new_symbols_are_exported(lib):
    import cornell_moe_amd
    from cornell_moe_amd import api, expected_improvement_constrained as eic
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("ei_constrained_ensemble", "ei_constrained_multistart", "ei_constrained_suggest"):
        assert callable(getattr(api, name))
    for name in ("ConstrainedExpectedImprovementMCMC", "multistart_constrained_expected_improvement_optimization", "best_feasible_value"):
        assert callable(getattr(eic, name))
    assert cornell_moe_amd.expected_improvement_constrained is eic


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
    return lib.moe_ei_constrained_mcmc(g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])),
                                       g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], 1,
                                       g("ei", _p(a["out"])), g("grad", _p(a["out"])), None, C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_constrained_mcmc_multistart(
        g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), g("gd", C.byref(a["gd"])),
        g("bounds", _p(a["bounds"])), g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None, None, None, None,
        C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_constrained_mcmc_suggest(
        g("gps", a["gps"]), a["E"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), g("gd", C.byref(a["gd"])),
        g("bounds", _p(a["bounds"])), g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])), g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
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
        assert call(lib, _args(domain=1), err) == V and _payload(err)[0] == 1.0 and b"constrained expected improvement" in err.message
    # the batch: num_to_sample directly after num_being_sampled, before the NULL pending array, the steps and the domain
    for p, q, hi in ((0, 0, 65.0), (0, 66, 65.0), (3, 63, 62.0), (64, 2, 1.0)):
        assert _suggest(lib, _args(p=p, q=q, steps=0, domain=1), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
    assert _suggest(lib, _args(p=65, q=0), err) == B and _payload(err) == (65.0, 0.0, 64.0)
