"""The Chebyshev-scalarised expected improvement on the device (csrc/chebei1.hip: moe_ei_chebyshev_mcmc,
moe_ei_chebyshev_mcmc_multistart, moe_ei_chebyshev_mcmc_suggest) against the long-double restatement of tests/chebei_reference.py,
on the cases chebei_reference.CASES, BELIEVED and MANY, which tests/test_chebei_reference.py checks on the CPU (the definition, an
independent evaluation of the integral, the analytic limit, central differences, the branches of the believed rule, each case
reaching what it is there for).

Tolerances: |value - want| and |A_e - want| <= max(1e-10, 4 ld_diff) scale, the gradient likewise as tests/test_gpu_ehvi3.py applies
it.  Everything else is bit for bit: value-only against value + gradient, a candidate alone against itself in a batch and across
the pass boundary, the value against the mean of the members' values formed on the host, ensemble-wide launches on against off,
the ascent against a host-driven loop over the evaluator, the greedy batch with three weight vectors against calls of the ascent
fed their predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.27 records those of
the first run."""
import numpy as np
import pytest

import chebei_reference as ch
import test_gpu_cei1 as tc
from cornell_moe_amd import _lib, api, expected_scalarised_improvement as esi

pytestmark = pytest.mark.gpu

LD = ch.LD
_Launches, _host_loop, _same_run = tc._Launches, tc._host_loop, tc._same_run
MS, _ascent_inputs = tc.MS, tc._ascent_inputs


class _Device(object):
    """the GPs of a problem on the device: objs[j] [E], objective j"""

    def __init__(self, p):
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in row] for row in p.gps]
        self.objs = [[row[j] for row in self.all] for j in range(p.M)]

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", scal=None, best=None, **kw):
    pending = p.pending if isinstance(pending, str) else pending
    return api.ei_chebyshev_ensemble(D.objs, p.scal[0] if scal is None else scal, p.best[0] if best is None else best, points,
                                     points_being_sampled=pending, **kw)


def _errors(value, grad, members, want):
    e_v = max(abs(value[i] - float(w.value)) / w.scale for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / min(w.scale, max(1.0, float(np.max(np.abs(w.grad)))))
              for i, w in enumerate(want))
    e_m = max(abs(members[e, i] - float(a)) / w.scale for i, w in enumerate(want) for e, a in enumerate(w.members))
    return e_v, e_g, e_m


def _host_mean(members):
    """the documented rule on the host: the members added in member order, divided once"""
    E, n = members.shape
    out = np.zeros(n)
    for i in range(n):
        total = float(members[0, i])
        for e in range(1, E):
            total = total + float(members[e, i])
        out[i] = total / float(E)
    return out


# ---- 1. value, gradient and the members' values against long double; the bits of one call ----
@pytest.mark.parametrize("case", ch.ALL_CASES, ids=[c.name for c in ch.ALL_CASES])
def test_against_the_long_double_restatement(case):
    p, want = ch.expected(case, LD)
    D = _Device(p)
    C_, d = p.points.shape
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_member_values=True))
    value, grad, members = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and members.shape == (case.E, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(members >= 0.0) and np.all(value >= 0.0)
    bound = max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, e_m = _errors(value, grad, members, want)
    print("%s: value error %.3g scale, gradient error %.3g, members' error %.3g scale (bound %.3g)" % (case.name, e_v, e_g, e_m, bound))
    assert e_v <= bound and e_g <= bound and e_m <= bound, (case.name, e_v, e_g, e_m)
    # the call's value is the mean of its own members' values formed on the host, bit for bit
    assert np.array_equal(value, _host_mean(members))
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, m1 = _eval(D, p, p.points[i:i + 1], want_member_values=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(m1[:, 0], members[:, i]), (case.name, i)
    if case.kind == "below":
        assert not np.any(value) and not np.any(grad) and not np.any(members)  # exact zeros, zero coefficients
    elif len(p.pending):
        assert not np.array_equal(_eval(D, p, p.points, pending=None, want_grad=False), value)  # (the pending points are not ignored)
    D.close()


# ---- 2. across the pass boundary ----
_N8 = ch.Case("m3_e1_d2_n8_p2_two_passes", 44, 3, 1, 2, ((8, 8, 8),), 2, 4100, "plain", 0.0)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    p = ch.make_problem(_N8)
    checked = (0, per_pass - 1, per_pass, _N8.C - 1)
    ref_members = ch.ensemble(p, LD)
    sc = ch.scales_of(p)
    D = _Device(p)
    for pending in (p.pending, None):
        value, grad, members = _eval(D, p, p.points, pending=pending, want_member_values=True)
        assert np.array_equal(_eval(D, p, p.points, pending=pending, want_grad=False), value)
        assert np.array_equal(value, _host_mean(members)) and np.all(value >= 0.0) and float(np.max(value)) > 1e-4
        for i in checked:
            v1, g1 = _eval(D, p, p.points[i:i + 1], pending=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            want = [ch.evaluate(ref_members, p.points[i], p.scal[0], p.best[0], sc) for i in checked]
            idx = list(checked)
            e_v, e_g, e_m = _errors(value[idx], grad[idx], members[:, idx], want)
            print("%s: value error %.3g scale, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= 1e-10 and e_g <= 1e-10 and e_m <= 1e-10
    D.close()


# ---- 3. the ascent against the host-driven loop ----
# (the loose tolerance is tests/test_gpu_cei1.py's: starts stop inside a round, so that masked steps occur)
@pytest.mark.parametrize("tolerance", [1e-10, 0.3], ids=["tight", "loose"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(tolerance):
    p = ch.make_problem(ch.case(ch.ENSEMBLE))  # E = 3, M = 3
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], tolerance)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    plain = api.ei_chebyshev_multistart(D.objs, p.scal[0], p.best[0], gd, bounds, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.ei_chebyshev_multistart(D.objs, p.scal[0], p.best[0], gd, bounds, starts, want_path=True, points_being_sampled=pending)
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
    none = api.ei_chebyshev_multistart(D.objs, p.scal[0], p.best[0], gd, bounds, starts, gradient_ascent=False, points_being_sampled=pending)
    best = int(np.argmax(want["start_values"]))
    assert np.array_equal(none["point"], starts[best]) and none["value"] == want["start_values"][best] and none["found"]
    D.close()


# ---- 4. a greedy batch with a weight vector per point ----
def _three_rounds(p):
    """three scalarisations and every member's observed incumbents under each"""
    w = esi.sample_simplex_weights(3, p.M, 5)
    scal = np.array([ch.scalarisation(w[t], [ch.IDEAL] * p.M, [ch.NADIR] * p.M) for t in range(3)])
    best = np.array([ch.observed_best(p.gps, scal[t]) for t in range(3)])
    return scal, best


def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    p = ch.make_problem(ch.case(ch.ENSEMBLE))
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 3
    scal, best = _three_rounds(p)
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.ei_chebyshev_multistart(D.objs, scal[t], best[t], gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.ei_chebyshev_suggest(D.objs, scal, best, gd, bounds, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    # the weights matter: round 1 under round 0's scalarisation is another call
    same = api.ei_chebyshev_multistart(D.objs, scal[0], best[0], gd, bounds, starts,
                                       points_being_sampled=np.vstack([pending, want_points[0][None, :]]))
    assert same["value"] != want_values[1]
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) >= 1e-3
    D.close()


# ---- 5. the limits ----
def test_1024_gps_run_and_129_members_of_eight_are_refused():
    members = (0, 63, 127)
    p, want = ch.expected(ch.MANY, LD, members)
    D = _Device(p)
    value, vals = _eval(D, p, p.points, want_grad=False, want_member_values=True)
    assert vals.shape == (128, ch.MANY.C) and np.array_equal(value, _host_mean(vals)) and float(np.min(vals)) >= 0.0
    worst = max(abs(vals[e, i] - float(a)) / w.scale for i, w in enumerate(want) for e, a in zip(members, w.members))
    print("%s: members %s within %.3g scale of long double; values %s" % (p.name, members, worst, value))
    assert worst <= 1e-10 and float(np.max(value)) > 1e-5
    objs = [list(col) + [col[0]] for col in D.objs]  # 129 members: refused before a handle is looked at
    with pytest.raises(api.BoundsException):
        api.ei_chebyshev_ensemble(objs, p.scal[0], list(p.best[0]) + [p.best[0][0]], p.points, want_grad=False)
    D.close()


def test_a_65th_pending_point_and_derivative_observations_are_refused():
    p = ch.make_problem(ch.case("m2_e1_d3_n20_p0"))
    D = _Device(p)
    rng = np.random.default_rng(3)
    pend = rng.uniform(0, 1, size=(65, 3))
    v64 = _eval(D, p, p.points[:2], pending=pend[:64], want_grad=False)
    assert np.all(np.isfinite(v64)) and np.all(v64 >= 0.0)
    with pytest.raises(api.BoundsException):
        _eval(D, p, p.points[:2], pending=pend, want_grad=False)
    starts, gd, bounds = _ascent_inputs(3, 1e-10)
    scal, best = np.tile(p.scal[0], (2, 1)), np.tile(p.best[0], (2, 1))
    with pytest.raises(api.BoundsException):
        api.ei_chebyshev_suggest(D.objs, scal, best, gd, bounds, starts, 2, points_being_sampled=pend[:64])
    g = p.gps[0][0]
    yd = np.hstack([np.asarray(g.y).reshape(-1, 1), np.zeros((len(g.X), 1))])
    deriv = api.DeviceGP(g.hyper, g.X, yd, [1e-2, 1e-2], [0], cov_type=g.cov_type)  # (one observed derivative)
    with pytest.raises(api.InvalidValueException):
        api.ei_chebyshev_ensemble([[deriv], D.objs[1]], p.scal[0], p.best[0], p.points[:2], want_grad=False)
    deriv.close()
    D.close()


# ---- 6. the wrapper ----
def test_the_wrapper_and_the_optimisation_run_end_to_end():
    p = ch.make_problem(ch.case("m3_e1_d3_n20_p2"))
    D = _Device(p)
    models = [[g] for g in D.all[0]]  # M ensembles of one member each
    outcomes = np.stack([np.asarray(g.y, dtype=np.float64).ravel() for g in p.gps[0]], axis=1)
    w = [0.2, 0.3, 0.5]
    ideal, nadir = [ch.IDEAL] * 3, [ch.NADIR] * 3
    a, b = esi.chebyshev_scalarisation(w, ideal, nadir)
    best = esi.chebyshev_best_so_far(outcomes, a, b)
    obj = esi.ChebyshevExpectedImprovementMCMC(models, w, ideal, nadir, best_so_far=best, points_being_sampled=p.pending)
    direct = api.ei_chebyshev_ensemble(D.objs, np.concatenate([a, b]), [best], p.points, points_being_sampled=p.pending)
    v, g = obj.evaluate_at_point_list(p.points, want_grad=True)
    assert np.array_equal(v, direct[0]) and np.array_equal(g, direct[1])
    obj.set_current_point(p.points[2:3])
    assert obj.compute_objective_function() == v[2] and np.array_equal(obj.compute_grad_objective_function()[0], g[2])
    # the whole suggestion: inside the bounds, and its first pick is api.ei_chebyshev_multistart's
    gd = (8, 6, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    bounds = np.array([[0.0, 1.0]] * 3)
    weights = esi.sample_simplex_weights(2, 3, 11)
    # (the models here are device GPs, which keep no observed values: the incumbents are computed from the problem's and passed on)
    scal = [np.concatenate(esi.chebyshev_scalarisation(weights[t], ideal, nadir)) for t in range(2)]
    bests = [[esi.chebyshev_best_so_far(outcomes, *ch.split(scal[t]))] for t in range(2)]
    starts = api.latin_hypercube(11, bounds, 8)
    batch = api.ei_chebyshev_suggest(D.objs, np.array(scal), np.array(bests), gd, bounds, starts, 2)
    first = api.ei_chebyshev_multistart(D.objs, scal[0], bests[0], gd, bounds, starts)
    assert np.all(batch["found"]) and np.all(batch["points"] >= 0.0) and np.all(batch["points"] <= 1.0)
    assert np.array_equal(batch["points"][0], first["point"]) and batch["values"][0] == first["value"]

    class _Observed(object):  # a model object that keeps its observed values beside its device GP
        def __init__(self, dev, y):
            self._dev, self._y = dev, np.asarray(y, dtype=np.float64)

    wrapped = [[_Observed(D.all[0][j], p.gps[0][j].y)] for j in range(3)]
    pts, vals, found = esi.multistart_chebyshev_expected_improvement_optimization(wrapped, ideal, nadir, bounds, gd, 8, num_to_sample=2,
                                                                                  weights=weights, seed=11)
    assert np.array_equal(pts, batch["points"]) and np.array_equal(vals, batch["values"]) and np.all(found)
    D.close()
