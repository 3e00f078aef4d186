"""The log three-objective expected hypervolume improvement on the device (csrc/logehvi3.hip: moe_log_ehvi3_constrained_mcmc,
moe_log_ehvi3_constrained_mcmc_multistart, moe_log_ehvi3_constrained_mcmc_suggest) against the long-double restatement of
tests/log_ehvi3_reference.py on its case-shifts, which tests/test_log_ehvi3_reference.py qualifies on the CPU.

Tolerances: the other log forms' -- |value - want| <= 1e-10 max(1, |want|), |grad - want|_inf <= 1e-10 max(1, |want|_inf), every log
factor like the value; exp(value) against the plain M = 3 constrained form within 1e-9 absolute.  Everything else is bit for bit:
value-only against value + gradient, a candidate alone against itself among eight and across the pass boundary, the ascent against
a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch against calls of the ascent fed their
predecessors' points, the value against the documented rule over factors_out with one member (with more, within the few units in
the last place by which the host's exp and log part from the device's).  Every test prints the worst figures it saw (pytest -s);
DESIGN.md section 5.26 records those of the first run."""
import math

import numpy as np
import pytest

import cehvi_reference as ch
import ehvi3_reference as h3
import log_ehvi3_reference as l3
import test_gpu_cei1 as tc
from cornell_moe_amd import _lib, api

pytestmark = pytest.mark.gpu

LD = l3.LD
BOUND = 1e-10
_Launches, _host_loop, _same_run = tc._Launches, tc._host_loop, tc._same_run

IDS = ["%s-r%g-t%g" % (c.name, s[0], s[1]) for c, s in l3.CASE_SHIFTS]


class _Device(object):
    """the GPs of a problem on the device: objs [3][E], cons [K][E] (None without constraints)"""

    def __init__(self, p, K=None):
        K = len(p.gps[0]) - 3 if K is None else K
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in row[:3 + K]] for row in p.gps]
        self.objs = [[row[r] for row in self.all] for r in range(3)]
        self.cons = [[row[3 + k] for row in self.all] for k in range(K)] if K else None
        self.tau = list(p.taus[:K]) if K else None

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", **kw):
    pending = p.pending if isinstance(pending, str) else pending
    front = p.front if len(p.front) else None
    return api.log_ehvi3_constrained_ensemble(D.objs, D.cons, D.tau, p.ref, front, points, points_being_sampled=pending, **kw)


def _rule_holds(value, logs):
    """the value is the documented rule over the call's own log factors.  With one member the rule is a sum: bit for bit.  With more
    it takes exp and log, which the device's and the host's libraries each round within a unit in the last place and not alike: the
    weights are at most 1 and W at most E, so the two values lie within a few units of the larger of 1 and |value|"""
    host = l3.host_value(logs)
    if logs.shape[0] == 1:
        return np.array_equal(value, host)
    return bool(np.all(np.abs(value - host) <= 8.0 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(host))))


def _errors(value, grad, logs, want):
    """the worst relative errors of candidates' values, gradients and log factors against Results"""
    e_v = max(abs(value[i] - float(w.value)) / max(1.0, abs(float(w.value))) for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(w.grad)))) for i, w in enumerate(want))
    e_f = max(abs(logs[e, r, i] - float(f)) / max(1.0, abs(float(f))) for i, w in enumerate(want) for e, row in enumerate(w.log_factors)
              for r, f in enumerate(row))
    return e_v, e_g, e_f


# ---- 1. value, gradient and log factors against long double; the bits of one call ----
@pytest.mark.parametrize("case,shift", l3.CASE_SHIFTS, ids=IDS)
def test_against_the_long_double_restatement(case, shift):
    p, members, want = l3.expected(case, shift, LD)
    D = _Device(p)
    C_, d = p.points.shape
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    assert value.shape == (C_,) and grad.shape == (C_, d) and logs.shape == (case.E, 1 + case.K, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(logs))
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    print("%s %s: boxes %s; value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds 1e-10); lowest value "
          "%.1f, largest |grad| %.3g" % (case.name, shift, [len(m.table) for m in members], e_v, e_g, e_f, float(value.min()),
                                          float(np.max(np.abs(grad)))))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND, (case.name, shift, e_v, e_g, e_f)
    # the value is the documented rule over the call's own log factors, formed on the host
    assert _rule_holds(value, logs)
    # the value alone: the same bits (want_grad 0 against 1); a candidate alone carries the bits it has among the eight
    v_only, f_only = _eval(D, p, p.points, want_grad=False, want_log_factors=True)
    assert np.array_equal(v_only, value) and np.array_equal(f_only, logs)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_log_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], logs[:, :, i]), (case.name, i)
    if case.p:
        assert not np.array_equal(_eval(D, p, p.points, pending=None, want_grad=False), value)
    D.close()


# ---- 2. against the plain form ----
@pytest.mark.parametrize("case", l3.CASES, ids=[c.name for c in l3.CASES])
def test_exp_of_the_value_is_the_plain_value(case):
    p, _, _ = l3.expected(case, l3.SHIFTS[0], LD)
    D = _Device(p)
    value = _eval(D, p, p.points, want_grad=False)
    A = api.ehvi_constrained_ensemble(D.objs, D.cons, D.tau, p.ref, p.front if len(p.front) else None, p.points,
                                      points_being_sampled=p.pending, want_grad=False)
    worst = float(np.max(np.abs(np.exp(value) - A)))
    print("%s: |exp(value) - plain value| at most %.3g (bound 1e-9 absolute); plain values %.3g .. %.3g" % (case.name, worst, A.min(), A.max()))
    assert worst <= 1e-9 and np.all(A > 0.0)
    D.close()


# ---- 3. no front, no pending point, one member, no constraint: one box ----
def test_with_an_empty_front_the_value_is_the_sum_of_three_log_psi():
    c = l3.case("log3_e3_k0_d3_n20_26_33_p3_f0")
    p0, _ = l3.shifted(c, l3.SHIFTS[0], LD)
    p = p0._replace(gps=p0.gps[:1], pending=p0.pending[:0])
    members = ch.ensemble(p, LD)
    D = _Device(p)
    worst = 0.0
    for s in l3.SHIFTS:
        q = l3.shifted_problem(p, None, s)
        value, logs = _eval(D, q, q.points, pending=None, want_grad=False, want_log_factors=True)
        assert np.array_equal(value, logs[0, 0])  # E = 1, K = 0: LL_0 bit for bit
        for i, x in enumerate(q.points):
            e, _ = l3.edge_logs([(m[0], m[1]) for m in l3.member_moments(members[0], x)], np.zeros((0, 3)), q.ref, LD)
            total = (e[0, 0, 1] + e[1, 0, 1]) + e[2, 0, 1]
            worst = max(worst, abs(value[i] - float(total)) / max(1.0, abs(float(total))))
    print("F = 0, p = 0, E = 1, K = 0: |value - (lambda_1(r1) + lambda_2(r2) + lambda_3(r3))| at most %.3g relative" % worst)
    assert worst <= BOUND
    D.close()


# ---- 4. the stall ----
@pytest.mark.parametrize("kind", l3.STALL_KINDS)
def test_the_plain_form_stalls_and_the_log_form_climbs(kind):
    """The reference point 60 below the observations in one objective, in all three, or one constraint 40 deviations from feasible:
    the plain M = 3 form is 0 at every start and moves none; the log form is finite, climbs from every start and has a gradient"""
    p = l3.stall_problem(kind)
    D = _Device(p)
    d = p.points.shape[1]
    starts, bounds = l3.stall_starts(d), np.array([[0.0, 1.0]] * d)
    front = p.front if len(p.front) else None
    plain = api.ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, front, l3.STALL_GD, bounds, starts,
                                            points_being_sampled=p.pending)
    assert np.all(plain["start_values"] == 0.0) and plain["value"] == 0.0
    assert np.array_equal(plain["end_points"], starts[plain["kept_index"]])  # no start moved
    got = api.log_ehvi3_constrained_multistart(D.objs, D.cons, D.tau, p.ref, front, l3.STALL_GD, bounds, starts,
                                               points_being_sampled=p.pending)
    climbs = got["end_values"] - got["start_values"][got["kept_index"]]
    _, grad = api.log_ehvi3_constrained_ensemble(D.objs, D.cons, D.tau, p.ref, front, starts, points_being_sampled=p.pending)
    print("stall (%s): the plain form's start values are all 0 and no start moves; the log form's start values %.6g .. %.6g, climbs "
          "per start %s, smallest |grad|_inf %.3g" % (kind, got["start_values"].min(), got["start_values"].max(),
                                                      np.round(climbs, 3).tolist(), float(np.min(np.max(np.abs(grad), axis=1)))))
    assert np.all(np.isfinite(got["start_values"])) and got["found"] and len(climbs) == len(starts) == 12
    assert np.all(climbs > 0.0) and got["value"] == got["end_values"].max()
    assert np.all(np.isfinite(grad)) and np.all(np.max(np.abs(grad), axis=1) > 0.0)
    D.close()


# ---- 5. boxes of weight 0 ----
@pytest.mark.parametrize("case", l3.EDGE_CASES, ids=[c.name for c in l3.EDGE_CASES])
def test_boxes_of_weight_zero_are_skipped(case):
    """a slab of zero thickness (two points share w exactly) and a strip whose u edges are an ulp apart: finite, no NaN, equal to
    the restatement"""
    for shift in l3.SHIFTS:
        p, members, want = l3.expected(case, shift, LD)
        D = _Device(p)
        value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(logs))
        e_v, e_g, e_f = _errors(value, grad, logs, want)
        print("%s %s: value error %.3g, gradient error %.3g, log factor error %.3g; boxes the long-double restatement skipped: %s" % (
            case.name, shift, e_v, e_g, e_f, sorted(set(w.skipped for w in want))))
        assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
        if case.name == l3.TIE.name:
            assert all(w.skipped == 3 for w in want)
        D.close()


# ---- 6. order and bits ----
def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    C_ = per_pass + 4
    assert per_pass == 4096
    c = ch.Case("m3_e1_k1_d2_n8_p2_f5_two_passes", 45, 3, 1, 1, 2, ch._grid(1, 4, 8), 2, 5, (0.0,), C_, None, 0.0)
    p0 = ch.make_problem(c)
    p = l3.shifted_problem(p0, None, l3.SHIFTS[1])
    checked = (0, per_pass - 1, per_pass, C_ - 1)
    members = l3.reshifted(ch.ensemble(p0, LD), p.ref, p.front, p.taus)
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    v_only, f_only = _eval(D, p, p.points, want_grad=False, want_log_factors=True)
    assert np.array_equal(v_only, value) and np.array_equal(f_only, logs)
    assert np.array_equal(value, logs[0, 0] + logs[0, 1])
    for i in checked:
        v1, g1 = _eval(D, p, p.points[i:i + 1])
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
    want = [l3.evaluate(members, p.points[i]) for i in checked]
    idx = list(checked)
    e_v, e_g, e_f = _errors(value[idx], grad[idx], logs[:, :, idx], want)
    print("%s: value error %.3g, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    D.close()


MS = dict(tc.MS, starts=12, steps=4, restarts=2)
ASCENT_CASE = "log3_e3_k1_d3_n20_26_33_p3_f22"


def _ascent_inputs(d, tolerance):
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], d))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    return starts, gd, np.array([[0.0, 1.0]] * d)


@pytest.mark.parametrize("shift", (l3.SHIFTS[0], l3.SHIFTS[2]), ids=["shift0", "shift8"])
@pytest.mark.parametrize("constraints", [True, False], ids=["k1", "k0"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(constraints, shift):
    p, _ = l3.shifted(l3.case(ASCENT_CASE), shift, np.float64)  # E = 3, K = 1, 276 boxes
    D = _Device(p, K=None if constraints else 0)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    for on in (True, False):
        with _Launches(on):
            got = api.log_ehvi3_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, want_path=True,
                                                       points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("shift %s, K = %d: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        shift, 1 if constraints else 0, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"],
        want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"] and np.isfinite(want["value"])
    assert want["value"] >= want["start_values"].max()
    assert float(np.max(np.abs(want["end_points"] - starts[want["kept_index"]]))) > 1e-3  # (the starts moved)
    D.close()


def test_the_batch_of_two_is_two_ascents_the_second_fed_the_firsts_pick():
    p, _ = l3.shifted(l3.case(ASCENT_CASE), l3.SHIFTS[1], np.float64)
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 2
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.log_ehvi3_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ehvi3_constrained_suggest(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, q,
                                                    points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gap = float(np.max(np.abs(want_points[1] - want_points[0])))
    print("greedy log values %s, the picks %.3g apart" % (want_values, gap))
    assert np.all(np.isfinite(want_values)) and gap >= 1e-3
    D.close()


# ---- 7. the believed-feasibility mask through the log form ----
def test_the_mask_rule_decides_which_believed_outcomes_join():
    """cehvi_reference.BELIEVED3: a pending point believed infeasible by one member joins only the other member's front.  Every
    member's L_e agrees with the restatement under the member's OWN mask and parts from the restatement under the other member's."""
    p = ch.make_problem(ch.BELIEVED3)
    members = l3.reshifted(ch.ensemble(p, LD), p.ref, p.front, p.taus)
    want = [l3.evaluate(members, x) for x in p.points]
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    masks = [list(m.mask) for m in members]
    assert masks[0] != masks[1] and not all(masks[1])
    moved = []
    for e in range(2):
        alt = l3.remasked(members[e], masks[1 - e])
        L = [float(l3.member_logs(alt, x)[0][0]) for x in p.points]
        own = max(abs(logs[e, 0, i] - float(w.log_factors[e][0])) / max(1.0, abs(float(w.log_factors[e][0]))) for i, w in enumerate(want))
        assert own <= BOUND, (e, own)
        moved.append(max(abs(logs[e, 0, i] - L[i]) / max(1.0, abs(L[i])) for i in range(len(L))))
    print("BELIEVED3: masks %s; errors %.3g %.3g %.3g; each member's log hypervolume term against the restatement under the OTHER "
          "member's mask: %s" % (masks, e_v, e_g, e_f, moved))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    assert max(moved) >= 1e-3
    D.close()


def test_eight_pending_points_under_a_mask_that_differs_per_member():
    """cehvi_reference.MASKED[3] with every eighth of its pending points: E = 5, p = 8, every member's own mask row and its own front
    and table; the members' L_e one by one"""
    p = ch.masked_problem(3)
    p = p._replace(pending=np.ascontiguousarray(p.pending[::8]))
    assert len(p.pending) == 8
    members = l3.reshifted(ch.ensemble(p, LD), p.ref, p.front, p.taus)
    masks = [tuple(bool(b) for b in m.mask) for m in members]
    assert len(set(masks)) >= 3 and any(not all(m) for m in masks) and any(any(m) for m in masks)
    want = [l3.evaluate(members, x) for x in p.points]
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    assert _rule_holds(value, logs)
    per_member = [max(abs(logs[e, 0, i] - float(w.log_factors[e][0])) / max(1.0, abs(float(w.log_factors[e][0]))) for i, w in enumerate(want))
                  for e in range(5)]
    ones = [l3.remasked(m, [True] * 8) for m in members]
    apart = [max(abs(logs[e, 0, i] - float(l3.member_logs(ones[e], x)[0][0])) for i, x in enumerate(p.points)) for e in range(5)]
    print("%s, p = 8: masks %s; boxes %s; value error %.3g, gradient error %.3g, log factor error %.3g; L_e per member %s; against the "
          "all-ones mask per member %s" % (p.name, [sum(m) for m in masks], [len(m.table) for m in members], e_v, e_g, e_f, per_member,
                                           np.round(apart, 4).tolist()))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND and max(per_member) <= BOUND
    assert max(apart) > 1e-3
    D.close()


# ---- 8. the limits, once ----
def test_the_full_front_with_sixty_four_pending_points():
    """ehvi3_reference.FULL: F = 192 and 64 pending points, E = 2, C = 4, K = 0 -- member 0's front takes all 64 believed outcomes
    (256 points, 33 153 boxes), member 1's stays the caller's (18 721 boxes)"""
    f = h3.make_problem(h3.FULL)
    p = ch.Problem(f.name, 3, f.gps, [], f.ref, f.front, f.points, f.pending, f.checked)
    members = l3.reshifted(ch.ensemble(p, LD), p.ref, p.front, p.taus)
    assert [len(m.table) for m in members] == [33153, 18721]
    want = [l3.evaluate(members, x) for x in p.points]
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    print("%s: value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds 1e-10); values %s" % (
        p.name, e_v, e_g, e_f, value.tolist()))
    assert _rule_holds(value, logs)
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    D.close()


# ---- 9. the wrapper ----
def test_the_wrapper_and_the_optimisation_run_end_to_end():
    import wrappers_mirror as cw
    from cornell_moe_amd import expected_hypervolume_improvement_constrained as cehvi, log_expected_hypervolume_improvement as lehvi
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(10, dim))
    centres = [(0.25, 0.25), (0.75, 0.75), (0.25, 0.75)]
    ys = [np.sum((X - np.array(c)) ** 2, axis=1) * 4.0 - 1.0 for c in centres]
    con = np.sum((X - 0.5) ** 2, axis=1)  # feasible inside the disc of radius 0.4 about the centre
    tau = [0.16]
    hypers = np.array([[1.0, 0.5, 0.5], [1.4, 0.45, 0.6], [0.8, 0.6, 0.5]])
    ensembles = []
    for vals in ys + [con]:
        hd = cw.HistoricalData(dim=dim, num_derivatives=0)
        hd.append_sample_points([cw.SamplePoint(X[i], [vals[i]], noise) for i in range(X.shape[0])])
        ensembles.append(cw.GaussianProcessMCMC(hypers, np.full((num_mcmc, 1), noise), hd, []).member_models())
    objective_models, constraint_models = ensembles[:3], ensembles[3:]
    ref = (2.0, 2.0, 2.0)
    cand = rng.uniform(size=(7, dim))
    gd, bounds = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8), [[0.0, 1.0]] * dim
    starts = api.latin_hypercube(31, bounds, 16)
    objs = [cehvi._device_members(m) for m in objective_models]
    for cm, tt in ((constraint_models, tau), (None, None)):
        front = cehvi.feasible_pareto_front(np.stack(ys, axis=1), con[:, None] if cm else np.zeros((len(con), 0)), tt or [], ref)
        obj = lehvi.LogExpectedHypervolumeImprovement3MCMC(objective_models, ref, constraint_models=cm, thresholds=tt)
        assert obj.problem_size == dim and np.array_equal(obj.front, front) and obj.num_constraints == (1 if cm else 0)
        cons = [cehvi._device_members(m) for m in cm] if cm else None
        want_v, want_g = api.log_ehvi3_constrained_ensemble(objs, cons, tt, ref, front, cand)
        assert np.array_equal(obj.evaluate_at_point_list(cand), want_v) and np.all(np.isfinite(want_v))
        obj.set_current_point(cand[3])
        assert obj.compute_expected_hypervolume_improvement() == want_v[3]
        assert np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
        plain = cehvi.ConstrainedExpectedHypervolumeImprovementMCMC(objective_models, cm, tt, ref).evaluate_at_point_list(cand)
        assert np.max(np.abs(np.exp(want_v) - plain)) <= 1e-9
        points, values, found = lehvi.multistart_log_expected_hypervolume_improvement_3_optimization(
            objective_models, ref, bounds, gd, 16, num_to_sample=2, constraint_models=cm, thresholds=tt, seed=31)
        assert points.shape == (2, dim) and values.shape == (2,) and np.all(found) and np.all(np.isfinite(values))
        first = api.log_ehvi3_constrained_multistart(objs, cons, tt, ref, front, gd, bounds, starts)
        assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
        print("K = %d: a batch of 2 at %s, log values %s" % (1 if cm else 0, np.round(points, 3).tolist(), [float(v) for v in values]))
    for n in (2, 4):
        with pytest.raises(ValueError) as e:
            lehvi.LogExpectedHypervolumeImprovement3MCMC(ensembles[:n], (2.0,) * n)
        assert "three objectives" in str(e.value)
    with pytest.raises(api.BoundsException):
        api.log_ehvi3_constrained_ensemble(objs[:2], None, None, (2.0, 2.0), None, cand)
