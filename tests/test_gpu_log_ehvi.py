"""The log expected hypervolume improvement on the device (csrc/logehvi1.hip: moe_log_ehvi_constrained_mcmc,
moe_log_ehvi_constrained_mcmc_multistart, moe_log_ehvi_constrained_mcmc_suggest) against the long-double restatement of
tests/log_ehvi_reference.py on its case-shifts, whose inputs tests/test_log_ehvi_reference.py qualifies on the CPU (float64 within
2.5e-11 of long double, the constructions, the stall).

Tolerances: tests/test_gpu_logcei1.py's, over the same chains -- |value - want| <= 1e-10 max(1, |want|), |grad - want|_inf <= 1e-10
max(1, |want|_inf), every log factor like the value.  Against the plain forms the bound is the sum of the two forms' bounds.
Everything else is bit for bit: value-only against value + gradient, a candidate alone against itself in a batch and across the pass
boundary, ensemble-wide launches on against off, an empty pending list against none, the value against the documented rule over
factors_out, the ascent against a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch against calls of
the ascent fed their predecessors' points.  log_ehvi_reference.EDGE_CASES add E = 2 with K = 2 and K = 8 (distinct thresholds), the
constraint role's floor, the log-strip kernel's lane branches (four sweeps, weights that underflow, the rho = 1 strip at lane 0 of
the second sweep and as the last strip; tests/test_log_ehvi_reference.py counts the branches on a replay of the lane order) and a
member whose weight underflows in the member log-sum-exp.  Every test prints the worst figures it saw (pytest -s); DESIGN.md
section 5.25 records those of the first run."""
import ctypes as C
import math

import numpy as np
import pytest

import cehvi_reference as ch
import log_ehvi_reference as lh
import test_gpu_cei1 as tc
from cornell_moe_amd import _lib, api

pytestmark = pytest.mark.gpu

LD = lh.LD
dp = _lib.dp
BOUND = 1e-10
_Launches, _host_loop, _same_run = tc._Launches, tc._host_loop, tc._same_run

IDS = ["%s-r%g-t%g" % (c.name, s[0], s[1]) for c, s in lh.CASE_SHIFTS]


class _Device(object):
    """the GPs of a problem on the device: objs [2][E], cons [K][E] (None without constraints)"""

    def __init__(self, p, K=None):
        K = len(p.gps[0]) - 2 if K is None else K
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in row[:2 + K]] for row in p.gps]
        self.objs = [[row[r] for row in self.all] for r in range(2)]
        self.cons = [[row[2 + k] for row in self.all] for k in range(K)] if K else None
        self.tau = list(p.taus[:K]) if K else None

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", **kw):
    pending = p.pending if isinstance(pending, str) else pending
    return api.log_ehvi_constrained_ensemble(D.objs, D.cons, D.tau, p.ref, p.front, points, points_being_sampled=pending, **kw)


def _raw_eval(D, p, points, pending):
    """moe_log_ehvi_constrained_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array"""
    stem, pre, E, d, K, keep = api._log_ehvi_constrained_call(D.objs, D.cons, D.tau, p.ref, p.front)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    value, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(getattr(_lib.load(), stem)(*(pre + (pend.ctypes.data_as(dp), pend.shape[0] - 1, pts.ctypes.data_as(dp), len(pts), 1,
                                                   value.ctypes.data_as(dp), grad.ctypes.data_as(dp), None, C.byref(err)))), err)
    return value, grad


def _errors(value, grad, logs, want):
    """the worst relative errors of candidates' values, gradients and log factors against Results"""
    e_v = max(abs(value[i] - float(w.value)) / max(1.0, abs(float(w.value))) for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(w.grad)))) for i, w in enumerate(want))
    e_f = max(abs(logs[e, r, i] - float(f)) / max(1.0, abs(float(f))) for i, w in enumerate(want) for e, row in enumerate(w.log_factors)
              for r, f in enumerate(row))
    return e_v, e_g, e_f


# ---- 1. value, gradient and log factors against long double; 2. the bits of one call ----
@pytest.mark.parametrize("case,shift", lh.CASE_SHIFTS, ids=IDS)
def test_against_the_long_double_restatement(case, shift):
    p, _, want = lh.expected(case, shift, LD)
    D = _Device(p)
    C_, d = p.points.shape
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_log_factors=True))
    value, grad, logs = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and logs.shape == (case.E, 1 + case.K, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(logs))
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    low = min(a for w in want for a in w.args)
    print("%s %s: value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds 1e-10); lowest z %.1f, lowest value "
          "%.1f, largest |grad| %.3g" % (case.name, shift, e_v, e_g, e_f, low, float(value.min()), float(np.max(np.abs(grad)))))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND, (case.name, shift, e_v, e_g, e_f)
    # the value is the documented rule over the call's own log factors, formed on the host
    assert np.array_equal(value, lh.host_value(logs))
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_log_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], logs[:, :, i]), (case.name, i)
    # no pending point through the symbol's pending arguments against None
    raw = _raw_eval(D, p, p.points, p.pending[:0])
    none = _eval(D, p, p.points, pending=None)
    assert np.array_equal(raw[0], none[0]) and np.array_equal(raw[1], none[1])
    if case.p:
        assert not np.array_equal(none[0], value)
    D.close()


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    C_ = per_pass + 4
    assert per_pass == 4096
    c = ch.Case("m2_e1_k1_d2_n8_p2_f5_two_passes", 44, 2, 1, 1, 2, ch._grid(1, 3, 8), 2, 5, (0.0,), C_, None, 0.0)
    p0 = ch.make_problem(c)
    s = lh.SHIFTS[1]
    p = p0._replace(ref=tuple(r - s[0] for r in p0.ref), front=np.ascontiguousarray(p0.front - s[0]))
    checked = (0, per_pass - 1, per_pass, C_ - 1)
    members = lh.reshifted(ch.ensemble(p0, LD), p.ref, p.front, p.taus)
    D = _Device(p)
    for pending in (p.pending, None):
        value, grad, logs = _eval(D, p, p.points, pending=pending, want_log_factors=True)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
        v_only, f_only = _eval(D, p, p.points, pending=pending, want_grad=False, want_log_factors=True)
        assert np.array_equal(v_only, value) and np.array_equal(f_only, logs)
        assert np.array_equal(value, logs[0, 0] + logs[0, 1])
        for i in checked:
            v1, g1 = _eval(D, p, p.points[i:i + 1], pending=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            want = [lh.evaluate(members, p.points[i]) for i in checked]
            idx = list(checked)
            e_v, e_g, e_f = _errors(value[idx], grad[idx], logs[:, :, idx], want)
            print("%s: value error %.3g, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    D.close()


def test_two_members_with_two_constraints_cross_the_pass_boundary():
    """E = 2, K = 2, distinct thresholds: the second pass holds 4 candidates where the first held 4096, so every [e][k] block of the
    per-pass arrays is strided by a pass size that is not the call's number of candidates"""
    per_pass = _lib.load().moe_ei1_pass_size(8)
    C_ = per_pass + 4
    assert per_pass == 4096
    c = ch.Case("m2_e2_k2_d2_n8_p2_f5_two_passes", 44, 2, 2, 2, 2, ch._grid(2, 4, 8), 2, 5, ch.EDGE_TAUS[2], C_, None, 0.0)
    p0 = ch.make_problem(c)
    s = lh.SHIFTS[1]
    p = p0._replace(ref=tuple(r - s[0] for r in p0.ref), front=np.ascontiguousarray(p0.front - s[0]))
    checked = (0, per_pass - 1, per_pass, C_ - 1)
    members = lh.reshifted(ch.ensemble(p0, LD), p.ref, p.front, p.taus)
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and logs.shape == (2, 3, C_)
    v_only, f_only = _eval(D, p, p.points, want_grad=False, want_log_factors=True)
    assert np.array_equal(v_only, value) and np.array_equal(f_only, logs)
    idx = list(checked)
    assert np.array_equal(value[idx], lh.host_value(logs[:, :, idx]))
    for i in checked:
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_log_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], logs[:, :, i]), i
    want = [lh.evaluate(members, p.points[i]) for i in checked]
    e_v, e_g, e_f = _errors(value[idx], grad[idx], logs[:, :, idx], want)
    print("%s: value error %.3g, gradient error %.3g, log factor error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g, e_f))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    D.close()


def test_on_a_noise_free_constraints_sampled_point_the_log_feasibility_is_exactly_zero():
    """log_ehvi_reference.CFLOOR: candidate 0 on a sampled point of the noise-free GP of constraint 1, observed 0.2 below tau_1:
    logehvi1_feas_kernel's own floor, log F_1 = 0 and a gradient that the factor does not move"""
    for shift in lh.CFLOOR_SHIFTS:
        p, _, want = lh.expected(lh.CFLOOR, shift, LD)
        D = _Device(p)
        value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
        assert logs[0, 1, 0] == 0.0 and np.all(logs[0, 1, 1:] < 0.0) and np.all(np.isfinite(grad))
        assert value[0] == logs[0, 0, 0] + 0.0 + logs[0, 2, 0]
        e_v, e_g, e_f = _errors(value[:1], grad[:1], logs[:, :, :1], want[:1])
        print("the constraint floor %s: at the floored candidate value error %.3g, gradient error %.3g, log factor error %.3g" % (
            shift, e_v, e_g, e_f))
        assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
        D.close()


# ---- 3. no front, no constraints, one member: the sum of two log expected improvements ----
def test_with_an_empty_front_the_value_is_the_sum_of_two_log_expected_improvements():
    p, _, _ = lh.expected(lh.case("log_e1_k0_d3_n20_p3_f0"), lh.SHIFTS[0], LD)
    D = _Device(p)
    worst, same = 0.0, True
    for s in (0.0, 3.0, 8.0):
        ref = tuple(r - s for r in p.ref)
        value = api.log_ehvi_constrained_ensemble(D.objs, None, None, ref, None, p.points, want_grad=False)
        l1 = api.log_ei_constrained_ensemble(D.objs[0], None, None, p.points, [ref[0]], want_grad=False)
        l2 = api.log_ei_constrained_ensemble(D.objs[1], None, None, p.points, [ref[1]], want_grad=False)
        total = l1 + l2
        worst = max(worst, float(np.max(np.abs(value - total) / np.maximum(1.0, np.abs(total)))))
        same = same and np.array_equal(value, total)
    print("F = 0, K = 0, E = 1: |value - (log EI_1 + log EI_2)| at most %.3g relative (bound 2e-10); bit equality observed: %s" % (worst, same))
    assert worst <= 2.0 * BOUND
    D.close()


# ---- 4. against the plain forms ----
@pytest.mark.parametrize("case", lh.ALL_CASES, ids=[c.name for c in lh.ALL_CASES])
def test_exp_of_the_value_is_the_plain_value(case):
    p, members, _ = lh.expected(case, lh.SHIFTS[0], LD)
    D = _Device(p)
    value = _eval(D, p, p.points, want_grad=False)
    if case.K:
        A = api.ehvi_constrained_ensemble(D.objs, D.cons, D.tau, p.ref, p.front, p.points, points_being_sampled=p.pending, want_grad=False)
    else:
        A = api.ehvi_ensemble(D.objs[0], D.objs[1], p.ref, p.front, p.points, points_being_sampled=p.pending, want_grad=False)
    scale = max(m.scale for m in members)
    worst = 0.0
    for i in range(len(p.points)):
        bound = BOUND * scale + BOUND * A[i] * max(1.0, abs(math.log(A[i])) if A[i] > 0 else 1.0)
        worst = max(worst, abs(math.exp(value[i]) - A[i]) / bound)
    print("%s: |exp(value) - plain value| at most %.3g of the sum of the two bounds" % (case.name, worst))
    assert worst <= 1.0
    D.close()


# ---- 5. the believed-feasibility mask through the log form ----
def test_the_mask_rule_decides_which_believed_outcomes_join():
    """cehvi_reference.BELIEVED2: member 0's front takes pending point 0 (a front point leaves), member 1 believes point 1
    infeasible and does not take it (it would have joined), point 2 is dominated under both.  Each decision is shown through the
    member's log hypervolume term: it agrees with the restatement under the rule within the bound and parts from the restatement
    whose front is formed WITHOUT the point (member 0, point 0) or WITH it (member 1, point 1) by far more; leaving point 2 out of
    the offers moves nothing."""
    case = lh.BELIEVED2
    p, members, want = lh.expected(case, lh.SHIFTS[0], LD)
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    assert [list(m.mask) for m in members] == [[True, True, True], [True, False, True]]
    other = {"member 0 without point 0": (0, [False, True, True]), "member 1 with point 1": (1, [True, True, True]),
             "member 0 without point 2": (0, [True, True, False]), "member 1 without point 2": (1, [True, False, False])}
    moved = {}
    for name, (e, mask) in other.items():
        alt = lh.remasked(members[e], mask)
        L = [float(lh.member_logs(alt, x)[0][0]) for x in p.points]
        moved[name] = max(abs(logs[e, 0, i] - L[i]) / max(1.0, abs(L[i])) for i in range(len(L)))
    print("BELIEVED2: errors %.3g %.3g %.3g; the log hypervolume term against the restatement under other decisions: %s" % (
        e_v, e_g, e_f, moved))
    assert moved["member 0 without point 0"] >= 1e-3 and moved["member 1 with point 1"] >= 1e-3
    assert moved["member 0 without point 2"] <= BOUND and moved["member 1 without point 2"] <= BOUND
    # on the device alone: without constraints every point is offered -- member 0's bits stay, member 1's term moves
    free = api.log_ehvi_constrained_ensemble(D.objs, None, None, p.ref, p.front, p.points, points_being_sampled=p.pending,
                                             want_grad=False, want_log_factors=True)[1]
    assert np.array_equal(free[0, 0], logs[0, 0]) and float(np.max(np.abs(free[1, 0] - logs[1, 0]))) >= 1e-3
    D.close()


def test_sixty_four_pending_points_under_a_mask_that_differs_per_member():
    """cehvi_reference.MASKED[2] through the log form: E = 5, p = 64, every member's own mask row of 64 words and its own front of
    130 to 160 points (three sweeps of strips)"""
    p, _ = ch.expected(ch.MASKED[2], LD)
    members = ch.ensemble(p, LD)
    want = [lh.evaluate(members, x) for x in p.points]
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    assert np.array_equal(value, lh.host_value(logs))
    ones = [ch.remasked(m, [True] * len(p.pending), p.front) for m in members]
    apart = [max(abs(logs[e, 0, i] - float(lh.member_logs(ones[e], x)[0][0])) for i, x in enumerate(p.points)) for e in range(5)]
    print("%s: value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds 1e-10); the log hypervolume term against "
          "the restatement under the all-ones mask, per member: %s" % (p.name, e_v, e_g, e_f, np.round(apart, 4).tolist()))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    assert min(apart) > 1e-3
    D.close()


# ---- 6. the stall ----
@pytest.mark.parametrize("kind", lh.STALL_FRONTS)
def test_the_plain_form_stalls_and_the_log_form_climbs(kind):
    p, _ = lh.stall(kind, np.float64)
    D = _Device(p)
    d = p.points.shape[1]
    starts, bounds = lh.stall_starts(d), np.array([[0.0, 1.0]] * d)
    front = p.front if len(p.front) else None
    plain = api.ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, front, lh.STALL_GD, bounds, starts,
                                            points_being_sampled=p.pending)
    assert np.all(plain["start_values"] == 0.0) and plain["value"] == 0.0
    assert np.array_equal(plain["end_points"], starts[plain["kept_index"]])  # no start moved
    got = api.log_ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, front, lh.STALL_GD, bounds, starts,
                                              points_being_sampled=p.pending)
    climbs = got["end_values"] - got["start_values"][got["kept_index"]]
    print("stall (%s front): the plain form's start values are all 0 and no start moves; the log form's start values %.6g .. %.6g, "
          "climbs per start %s" % (kind, got["start_values"].min(), got["start_values"].max(), np.round(climbs, 3).tolist()))
    assert np.all(np.isfinite(got["start_values"])) and got["found"] and len(climbs) == len(starts)
    assert np.all(climbs > 0.0) and got["value"] == got["end_values"].max()
    assert float(np.max(np.abs(got["end_points"] - starts[got["kept_index"]]))) > 1e-3
    D.close()


# ---- 7. the ascent against the host-driven loop; greedy batches ----
MS = dict(tc.MS, starts=12, steps=4, restarts=2)


def _ascent_inputs(d, tolerance):
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], d))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    return starts, gd, np.array([[0.0, 1.0]] * d)


@pytest.mark.parametrize("shift", (lh.SHIFTS[0], lh.SHIFTS[2]), ids=["shift0", "shift8"])
@pytest.mark.parametrize("constraints", [True, False], ids=["k1", "k0"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(constraints, shift):
    p, _ = lh.shifted(lh.case(ch.ENSEMBLE2), shift, np.float64)  # E = 3, K = 1, rows 20 / 130 / 300
    D = _Device(p, K=None if constraints else 0)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    plain = api.log_ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.log_ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, want_path=True,
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


def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    p, _ = lh.shifted(lh.case(ch.ENSEMBLE2), lh.SHIFTS[1], np.float64)
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.log_ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ehvi_constrained_suggest(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, q,
                                                   points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert np.all(np.isfinite(want_values)) and min(gaps) >= 1e-3
    D.close()


def test_the_batch_of_two_members_with_two_constraints_is_the_ascent_fed_its_predecessor():
    """cehvi_reference.MIXED2: E = 2, K = 2, d = 13, rows that differ per role and member, through the log form's hand-over"""
    p, _ = lh.shifted(ch.MIXED2, lh.SHIFTS[1], np.float64)
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 2
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.log_ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ehvi_constrained_suggest(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, q,
                                                   points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gap = float(np.max(np.abs(want_points[1] - want_points[0])))
    print("E = 2, K = 2: greedy log values %s, the picks %.3g apart" % (want_values, gap))
    assert np.all(np.isfinite(want_values)) and gap >= 1e-3
    D.close()


def test_a_belief_that_changes_along_the_batch_is_worked_out_anew_for_every_pick():
    """cehvi_reference.changing_problem (M = 2) through the log form: tests/test_gpu_cehvi.py's test of the same name"""
    p, starts = ch.changing_problem(2)
    D = _Device(p)
    _, gd, bounds = _ascent_inputs(3, 1e-10)
    q, tau = ch.CHANGING_Q[2], p.taus[0]
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([p.pending] + [x[None, :] for x in want_points])
        res = api.log_ehvi_constrained_multistart(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ehvi_constrained_suggest(D.objs, D.cons, D.tau, p.ref, p.front, gd, bounds, starts, q,
                                                   points_being_sampled=p.pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    every = np.vstack([p.pending] + [x[None, :] for x in want_points])
    mu0, mu1 = D.cons[0][0].mean(every), D.cons[0][1].mean(every)
    belief = [bool(m <= tau) for m in mu1]
    true_gap, stale_gap = [], []
    for t, v in enumerate(want_values):
        fed = every[:1 + t]
        members = ch.ensemble(p, LD, pending=fed)
        stale = [ch.remasked(m, [m.mask[0]] * len(fed), p.front) for m in members]
        a, b = lh.evaluate(members, every[1 + t]), lh.evaluate(stale, every[1 + t])
        true_gap.append(abs(v - float(a.value)) / max(1.0, abs(float(a.value))))
        stale_gap.append(abs(v - float(b.value)) / max(1.0, abs(float(a.value))))
    print("member 1's constraint means at the pending point and the %d picks %s (tau = 0): believed feasible %s; member 0's %s; log "
          "values %s; against the restatement %s, against the one under the first point's belief %s" % (
              q, np.round(mu1, 4).tolist(), belief, np.round(mu0, 3).tolist(), want_values, true_gap, stale_gap))
    assert np.all(np.abs(mu1 - tau) >= ch.MARGIN) and np.all(mu0 <= tau - ch.MARGIN)
    assert len(set(belief)) == 2 and any(belief[j] != belief[t] for t in range(1, q + 1) for j in range(t))
    assert max(true_gap) <= BOUND and max(stale_gap[1:]) > 1e-3
    D.close()


# ---- 7b. a member whose weight underflows ----
def test_a_hopeless_member_leaves_the_other_members_bits_less_log_two():
    """log_ehvi_reference.HOPELESS: LL_1 lies more than 800 below LL_0 at every candidate (tests/test_log_ehvi_reference.py), so
    w_1 = exp(LL_1 - m) is exactly 0 in the member log-sum-exp: W = 1 + 0, the gradient (1 g_0 + 0 g_1) / 1.  Member 0's log factors
    and the gradient are those of the call on member 0's GPs alone, and the value is that call's less log 2 under the documented
    rule m + log W - log E, bit for bit."""
    p, _, want = lh.expected(lh.HOPELESS, lh.SHIFTS[0], LD)
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
    assert np.all(np.isfinite(logs)) and np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    LL = logs[:, 0] + logs[:, 1]
    assert np.all(LL[1] - LL[0] < lh.HOPELESS_GAP)
    assert np.array_equal(value, lh.host_value(logs))
    alone = api.log_ehvi_constrained_ensemble([D.objs[0][:1], D.objs[1][:1]], [D.cons[0][:1]], D.tau, p.ref, p.front, p.points,
                                              points_being_sampled=p.pending, want_log_factors=True)
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    print("hopeless: LL_1 - LL_0 on the device %s; errors %.3g %.3g %.3g; value - (member 0 alone - log 2) %s" % (
        np.round(LL[1] - LL[0], 1).tolist(), e_v, e_g, e_f, (value - (alone[0] - math.log(2.0))).tolist()))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    assert np.array_equal(logs[0], alone[2][0]) and np.array_equal(grad, alone[1])
    assert np.array_equal(value, alone[0] - math.log(2.0))
    D.close()


# ---- 8. the wrapper ----
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
    objective_models, constraint_models = ensembles[:2], ensembles[3:]
    ref = (2.0, 2.0)
    cand = rng.uniform(size=(7, dim))
    gd, bounds = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8), [[0.0, 1.0]] * dim
    starts = api.latin_hypercube(31, bounds, 16)
    objs = [cehvi._device_members(m) for m in objective_models]
    for cm, tt in ((constraint_models, tau), (None, None)):
        front = cehvi.feasible_pareto_front(np.stack(ys[:2], axis=1), con[:, None] if cm else np.zeros((len(con), 0)), tt or [], ref)
        obj = lehvi.LogExpectedHypervolumeImprovementMCMC(objective_models, ref, constraint_models=cm, thresholds=tt)
        assert obj.problem_size == dim and np.array_equal(obj.front, front) and obj.num_constraints == (1 if cm else 0)
        cons = [cehvi._device_members(m) for m in cm] if cm else None
        want_v, want_g = api.log_ehvi_constrained_ensemble(objs, cons, tt, ref, front, cand)
        assert np.array_equal(obj.evaluate_at_point_list(cand), want_v) and np.all(np.isfinite(want_v))
        obj.set_current_point(cand[3])
        assert obj.compute_expected_hypervolume_improvement() == want_v[3]
        assert np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
        plain = cehvi.ConstrainedExpectedHypervolumeImprovementMCMC(objective_models, cm, tt, ref).evaluate_at_point_list(cand)
        assert np.max(np.abs(np.exp(want_v) - plain)) <= 1e-9
        points, values, found = lehvi.multistart_log_expected_hypervolume_improvement_optimization(
            objective_models, ref, bounds, gd, 16, num_to_sample=2, constraint_models=cm, thresholds=tt, seed=31)
        assert points.shape == (2, dim) and values.shape == (2,) and np.all(found) and np.all(np.isfinite(values))
        first = api.log_ehvi_constrained_multistart(objs, cons, tt, ref, front, gd, bounds, starts)
        assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
        print("K = %d: a batch of 2 at %s, log values %s" % (1 if cm else 0, np.round(points, 3).tolist(), [float(v) for v in values]))
    with pytest.raises(ValueError) as e:
        lehvi.LogExpectedHypervolumeImprovementMCMC(ensembles[:3], (2.0, 2.0, 2.0))
    assert "two objectives" in str(e.value)
    with pytest.raises(ValueError):
        lehvi.multistart_log_expected_hypervolume_improvement_optimization(ensembles[:3], (2.0, 2.0, 2.0), bounds, gd, 16)
    with pytest.raises(api.BoundsException):
        api.log_ehvi_constrained_ensemble([cehvi._device_members(m) for m in ensembles[:3]], None, None, (2.0, 2.0, 2.0), None, cand)
