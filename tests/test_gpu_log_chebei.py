"""The log Chebyshev-scalarised expected improvement, constrained too, on the device (csrc/logchebei1.hip:
moe_log_ei_chebyshev_constrained_mcmc, _multistart, _suggest) against the long-double restatement of tests/log_chebei_reference.py,
on the cases log_chebei_reference.CASES, BELIEVED and MANY, which tests/test_log_chebei_reference.py qualifies on the CPU.

Tolerances: the value, LA_e and every log F differ from long double by at most max(1e-10, 4 ld_diff), an absolute difference of a
log; the gradient by the same bound relative to its largest entry.  Everything else is bit for bit: value-only against value +
gradient, a candidate alone against itself in a batch and across the pass boundary, the value against the log-sum-exp of the group
values formed on the host (with one member; with more within a few units in the last place, _is_host_rule), ensemble-wide
launches on against off, the ascent against a host-driven loop over the evaluator, the greedy batch with three weight vectors
against calls of the ascent fed their predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md
section 5.28 records those of the first run."""
import numpy as np
import pytest

import chebei_reference as ch
import log_chebei_reference as lc
import test_gpu_cei1 as tc
from cornell_moe_amd import _lib, api, expected_scalarised_improvement as esi

pytestmark = pytest.mark.gpu

LD = lc.LD
_Launches, _host_loop, _same_run = tc._Launches, tc._host_loop, tc._same_run
MS, _ascent_inputs = tc.MS, tc._ascent_inputs


class _Device(object):
    """the GPs of a problem on the device: objs[j] [E], objective j; cons[k] [E], constraint k"""

    def __init__(self, p):
        G = p.M + p.K
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in row[:G]] for row in p.gps]
        self.objs = [[row[j] for row in self.all] for j in range(p.M)]
        self.cons = [[row[p.M + k] for row in self.all] for k in range(p.K)]
        self.tau = list(p.taus)

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", scal=None, best=None, **kw):
    pending = p.pending if isinstance(pending, str) else pending
    return api.log_ei_chebyshev_constrained_ensemble(D.objs, D.cons or None, D.tau or None, p.scal if scal is None else scal,
                                                     p.best if best is None else best, points, points_being_sampled=pending, **kw)


def _ascent(D, p, gd, bounds, starts, scal=None, best=None, **kw):
    return api.log_ei_chebyshev_constrained_multistart(D.objs, D.cons or None, D.tau or None, p.scal if scal is None else scal,
                                                       p.best if best is None else best, gd, bounds, starts, **kw)


def _errors(value, grad, factors, want, members=None):
    """(value, gradient, group values): absolute differences of logs; the gradient relative to its largest entry"""
    e_v = max(abs(value[i] - float(w.value)) for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / float(np.max(np.abs(w.grad))) for i, w in enumerate(want))
    idx = range(factors.shape[0]) if members is None else members
    e_f = max(abs(factors[e, r, i] - float(v)) for i, w in enumerate(want) for e, row in zip(idx, w.log_factors) for r, v in enumerate(row))
    return e_v, e_g, e_f


def _is_host_rule(value, factors):
    """the value is the documented rule over the call's own group values.  With one member the rule is a sum: bit for bit.  With more
    it takes exp and log, which the device's and the host's libraries each round within a unit in the last place and not alike
    (tests/test_gpu_log_ehvi3.py's finding and rule): the weights are at most 1 and W at most E, so the two values lie within a few
    units in the last place of the larger of 1 and |value|"""
    host = lc.host_value(factors)
    if factors.shape[0] == 1:
        return np.array_equal(value, host)
    return bool(np.all(np.abs(value - host) <= 8.0 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(host))))


# ---- 1. value, gradient and the group values against long double; the bits of one call ----
@pytest.mark.parametrize("case", lc.ALL_CASES, ids=[c.name for c in lc.ALL_CASES])
def test_against_the_long_double_restatement(case):
    p, want = lc.expected(case, LD)
    D = _Device(p)
    C_, d = p.points.shape
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_factors=True))
    value, grad, factors = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and factors.shape == (case.E, 1 + case.K, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(factors))
    assert np.all(np.max(np.abs(grad), axis=1) > 0.0)
    bound = max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, e_f = _errors(value, grad, factors, want)
    print("%s: value error %.3g, gradient error %.3g, group values' error %.3g (bound %.3g); values %.6g .. %.6g" % (
        case.name, e_v, e_g, e_f, bound, value.min(), value.max()))
    assert e_v <= bound and e_g <= bound and e_f <= bound, (case.name, e_v, e_g, e_f)
    # the call's value is the log-sum-exp of its own group values formed on the host; with E = 1 their sum, bit for bit
    assert _is_host_rule(value, factors)
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], factors[:, :, i]), (case.name, i)
    if len(p.pending):
        assert not np.array_equal(_eval(D, p, p.points, pending=None, want_grad=False), value)  # (the pending points are not ignored)
    D.close()


# ---- 2. the exact-zero regime: what the log form is there for ----
@pytest.mark.parametrize("name", [lc.STALL, lc.STALL_FAR_CASE])
def test_where_the_plain_form_is_exactly_zero_the_log_form_has_a_gradient(name):
    p = lc.make_problem(lc.case(name))
    D = _Device(p)
    plain, plain_grad = api.ei_chebyshev_ensemble(D.objs, p.scal, p.best, p.points)
    assert not np.any(plain) and not np.any(plain_grad)  # exact zeros at all 8 candidates: what the case is there for
    value, grad, factors = _eval(D, p, p.points, want_factors=True)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.max(np.abs(grad), axis=1) > 0.0)
    assert np.all(factors[:, 0, :] < -745.0)  # (below the smallest float64's log: no plain value could carry it)
    if p.K:
        assert np.all(factors[:, 1, :] < -400.0)  # the constraint 40 deviations from feasible
    print("%s: LA %.6g .. %.6g, gradient's largest entries %s" % (name, factors[:, 0, :].min(), factors[:, 0, :].max(),
                                                               np.max(np.abs(grad), axis=1)))
    D.close()


def test_twelve_starts_in_the_exact_zero_regime_all_climb():
    p = lc.make_problem(lc.case(lc.STALL))
    D = _Device(p)
    starts, _, bounds = _ascent_inputs(3, 1e-10)
    gd = lc.STALL_GD  # (the step size that the objective's curvature allows: log_chebei_reference.py says why)
    plain = api.ei_chebyshev_multistart(D.objs, p.scal, p.best, gd, bounds, starts)
    assert not np.any(plain["start_values"]) and not np.any(plain["end_values"])
    assert np.array_equal(plain["end_points"], starts[plain["kept_index"]])  # the plain form moves none
    got = _ascent(D, p, gd, bounds, starts)
    kept = got["kept_index"]
    gain = got["end_values"] - got["start_values"][kept]
    print("log form: every start's gain %s" % gain)
    assert len(kept) == MS["starts"] and np.all(gain > 0.0) and got["found"]
    D.close()


def test_a_floored_objective_above_the_incumbent_is_finite():
    """candidate 0 lies on a noise-free observation whose scalarised value is ABOVE the incumbent: sigma is the floor, ell about
    1e-29, LA about -1e28.  The value's bound there is the resolution of float64, 64 eps |LA| (the sum of M terms z^2 / 2, each a
    few roundings); the other candidates keep 1e-10.  At candidate 0 grad mu and grad var of the floored objective are 0 (the
    observation's own point), so the gradient is asserted finite, not non-zero."""
    p, want = lc.expected(lc.FLOOR_ABOVE, LD)
    D = _Device(p)
    value, grad, factors = _eval(D, p, p.points, want_factors=True)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(factors))
    assert value[0] < -1e27 and np.all(value[1:] > -10.0)
    errs = [abs(value[i] - float(w.value)) / max(1.0, abs(float(w.value))) for i, w in enumerate(want)]
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / float(np.max(np.abs(w.grad))) for i, w in enumerate(want) if i)
    print("%s: value %.6g at the floored candidate, relative error %.3g; elsewhere %.3g; gradient error %.3g; |grad| at the floored "
          "candidate %.3g" % (p.name, value[0], errs[0], max(errs[1:]), e_g, float(np.max(np.abs(grad[0])))))
    assert errs[0] <= 64 * np.finfo(np.float64).eps and max(errs[1:]) <= 1e-10 and e_g <= 1e-10
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value) and np.array_equal(value, factors[0, 0])
    starts, gd, bounds = _ascent_inputs(3, 1e-10)
    got = _ascent(D, p, gd, bounds, np.vstack([p.points[:1], starts[:5]]))  # an ascent that screens the floored point
    assert got["found"] and np.all(np.isfinite(got["start_values"])) and np.all(np.isfinite(got["end_values"]))
    D.close()


# ---- 3. across the pass boundary ----
_N8 = lc.Case("log_m3_e1_k1_d2_n8_p2_two_passes", 44, 3, 1, 1, 2, ((8, 8, 8, 8),), 2, 4100, "plain", lc.TAUS[1], 0.0, 0.0, 0.0)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    p = lc.make_problem(_N8)
    checked = (0, per_pass - 1, per_pass, _N8.C - 1)
    ref = lc.ensemble(p.gps, p.M, p.taus, p.pending, LD)
    D = _Device(p)
    value, grad, factors = _eval(D, p, p.points, want_factors=True)
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    assert _is_host_rule(value, factors) and np.all(np.isfinite(value))
    for i in checked:
        v1, g1 = _eval(D, p, p.points[i:i + 1])
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
    want = [lc.evaluate(ref, p.points[i], p.scal, p.best) for i in checked]
    idx = list(checked)
    e_v, e_g, e_f = _errors(value[idx], grad[idx], factors[:, :, idx], want)
    print("%s: value error %.3g, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
    assert e_v <= 1e-10 and e_g <= 1e-10 and e_f <= 1e-10
    D.close()


# ---- 4. the believed-and-feasible rule ----
def test_a_pending_point_joins_the_incumbent_only_where_the_member_believes_it_feasible():
    p, want = lc.expected(lc.BELIEVED, LD)
    D = _Device(p)
    value, grad, factors = _eval(D, p, p.points, want_factors=True)
    bound = max(1e-10, 4.0 * lc.BELIEVED.ld_diff)
    e_v, e_g, e_f = _errors(value, grad, factors, want)
    assert e_v <= bound and e_g <= bound and e_f <= bound
    # member 0's incumbent is NOT its lowest believed outcome (which it believes infeasible); without the constraint it is
    open_ = api.log_ei_chebyshev_constrained_ensemble(D.objs, None, None, p.scal, p.best, p.points, points_being_sampled=p.pending,
                                                      want_grad=False, want_factors=True)[1]
    assert not np.array_equal(open_[0, 0], factors[0, 0]) and np.array_equal(open_[1, 0], factors[1, 0])
    print("believed rule: errors %.3g %.3g %.3g; member 0's LA moves by %.3g where the mask is dropped" % (
        e_v, e_g, e_f, float(np.max(np.abs(open_[0, 0] - factors[0, 0])))))
    D.close()


# ---- 5. the ascent against the host-driven loop ----
@pytest.mark.parametrize("tolerance", [1e-10, 0.3], ids=["tight", "loose"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(tolerance):
    p = lc.make_problem(lc.case(lc.BATCH_K2))  # M = 4, K = 2
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], tolerance)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    for on in (True, False):
        with _Launches(on):
            got = _ascent(D, p, gd, bounds, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("tolerance %g: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"]
    if tolerance > 1e-3:
        assert int(want["steps_taken"].min()) < MS["steps"] * MS["restarts"]  # (masked steps occurred)
    else:
        assert want["value"] >= want["start_values"].max()
    D.close()


# ---- 6. a greedy batch with a weight vector per point ----
@pytest.mark.parametrize("name", [lc.ENSEMBLE, lc.BATCH_K2], ids=["k0", "k2"])
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit(name):
    p = lc.make_problem(lc.case(name))
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 3
    w = esi.sample_simplex_weights(q, p.M, 5)
    scal = np.array([ch.scalarisation(w[t], [ch.IDEAL] * p.M, [ch.NADIR] * p.M) for t in range(q)])
    best = np.array([ch.observed_best([row[:p.M] for row in p.gps], scal[t]) for t in range(q)])
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = _ascent(D, p, gd, bounds, starts, scal=scal[t], best=best[t], points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ei_chebyshev_constrained_suggest(D.objs, D.cons or None, D.tau or None, scal, best, gd, bounds, starts, q,
                                                           points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    print("%s: greedy values %s" % (name, want_values))
    D.close()


# ---- 7. the limits ----
def test_1024_gps_run_and_a_65th_member_of_sixteen_is_refused():
    members = (0, 31, 63)
    p, want = lc.expected(lc.MANY, LD, members)
    D = _Device(p)
    value, factors = _eval(D, p, p.points, want_grad=False, want_factors=True)
    assert factors.shape == (64, 9, lc.MANY.C) and _is_host_rule(value, factors)
    worst = max(abs(factors[e, r, i] - float(v)) for i, w in enumerate(want) for e, row in zip(members, w.log_factors)
                for r, v in enumerate(row))
    print("%s: members %s within %.3g of long double; values %s" % (p.name, members, worst, value))
    assert worst <= 1e-10
    objs = [list(col) + [col[0]] for col in D.objs]  # 65 members: refused before a handle is looked at
    cons = [list(col) + [col[0]] for col in D.cons]
    with pytest.raises(api.BoundsException):
        api.log_ei_chebyshev_constrained_ensemble(objs, cons, D.tau, p.scal, list(p.best) + [p.best[0]], p.points, want_grad=False)
    D.close()


def test_a_65th_pending_point_and_derivative_observations_are_refused():
    p = lc.make_problem(lc.case("log_m2_e1_k0_d3_n20_p0"))
    D = _Device(p)
    rng = np.random.default_rng(3)
    pend = rng.uniform(0, 1, size=(65, 3))
    v64 = _eval(D, p, p.points[:2], pending=pend[:64], want_grad=False)
    assert np.all(np.isfinite(v64))
    with pytest.raises(api.BoundsException):
        _eval(D, p, p.points[:2], pending=pend, want_grad=False)
    starts, gd, bounds = _ascent_inputs(3, 1e-10)
    scal, best = np.tile(p.scal, (2, 1)), np.tile(p.best, (2, 1))
    with pytest.raises(api.BoundsException):
        api.log_ei_chebyshev_constrained_suggest(D.objs, None, None, scal, best, gd, bounds, starts, 2, points_being_sampled=pend[:64])
    g = p.gps[0][0]
    yd = np.hstack([np.asarray(g.y).reshape(-1, 1), np.zeros((len(g.X), 1))])
    deriv = api.DeviceGP(g.hyper, g.X, yd, [1e-2, 1e-2], [0], cov_type=g.cov_type)  # (one observed derivative)
    with pytest.raises(api.InvalidValueException):
        api.log_ei_chebyshev_constrained_ensemble([[deriv], D.objs[1]], None, None, p.scal, p.best, p.points[:2], want_grad=False)
    deriv.close()
    D.close()


# ---- 8. the wrapper ----
def test_the_wrapper_and_the_optimisation_run_end_to_end():
    p = lc.make_problem(lc.case(lc.BATCH_K2))
    D = _Device(p)

    class _Observed(object):  # a model object that keeps its observed values beside its device GP
        def __init__(self, dev, y):
            self._dev, self._y = dev, np.asarray(y, dtype=np.float64)

    objective_models = [[_Observed(D.all[0][j], p.gps[0][j].y)] for j in range(p.M)]
    constraint_models = [[_Observed(D.all[0][p.M + k], p.gps[0][p.M + k].y)] for k in range(p.K)]
    w = [0.1, 0.2, 0.3, 0.4]
    ideal, nadir = [ch.IDEAL] * 4, [ch.NADIR] * 4
    a, b = esi.chebyshev_scalarisation(w, ideal, nadir)
    y = np.stack([np.asarray(g.y, dtype=np.float64).ravel() for g in p.gps[0][:p.M]], axis=1)
    cy = np.stack([np.asarray(g.y, dtype=np.float64).ravel() for g in p.gps[0][p.M:]], axis=1)
    best = esi.feasible_chebyshev_best_so_far(y, cy, p.taus, a, b)
    feasible = np.all(cy <= np.asarray(p.taus)[None, :], axis=1)
    assert 0 < feasible.sum() < len(feasible) and best == esi.chebyshev_best_so_far(y[feasible], a, b) >= esi.chebyshev_best_so_far(y, a, b)
    obj = esi.LogChebyshevExpectedImprovementMCMC(objective_models, w, ideal, nadir, points_being_sampled=p.pending,
                                                  constraint_models=constraint_models, thresholds=p.taus)
    assert obj.best_so_far[0] == best and obj.num_constraints == 2
    direct = api.log_ei_chebyshev_constrained_ensemble(D.objs, D.cons, D.tau, np.concatenate([a, b]), [best], p.points,
                                                       points_being_sampled=p.pending)
    v, g = obj.evaluate_at_point_list(p.points, want_grad=True)
    assert np.array_equal(v, direct[0]) and np.array_equal(g, direct[1])
    obj.set_current_point(p.points[2:3])
    assert obj.compute_objective_function() == v[2] and np.array_equal(obj.compute_grad_objective_function()[0], g[2])
    gd = (8, 6, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    bounds = np.array([[0.0, 1.0]] * 3)
    weights = esi.sample_simplex_weights(2, 4, 11)
    pts, vals, found = esi.multistart_log_chebyshev_expected_improvement_optimization(
        objective_models, ideal, nadir, bounds, gd, 8, num_to_sample=2, weights=weights, seed=11, constraint_models=constraint_models,
        thresholds=p.taus)
    assert np.all(found) and np.all(pts >= 0.0) and np.all(pts <= 1.0) and np.all(np.isfinite(vals))
    scal0 = np.concatenate(esi.chebyshev_scalarisation(weights[0], ideal, nadir))
    best0 = esi.feasible_chebyshev_best_so_far(y, cy, p.taus, *ch.split(scal0))
    first = api.log_ei_chebyshev_constrained_multistart(D.objs, D.cons, D.tau, scal0, [best0], gd, bounds, api.latin_hypercube(11, bounds, 8))
    assert np.array_equal(pts[0], first["point"]) and vals[0] == first["value"]
    D.close()
