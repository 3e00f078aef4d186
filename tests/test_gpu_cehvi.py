"""The constrained expected hypervolume improvement on the device (csrc/cehvi1.hip: moe_ehvi_constrained_mcmc*,
moe_ehvi3_constrained_mcmc*) against the long-double restatement of tests/cehvi_reference.py, on the cases cehvi_reference.ALL_CASES,
whose inputs tests/test_cehvi_reference.py qualifies on the CPU (at the checked candidates, at least 7 of 8, the value above 1e-3
scale, the gradient above 1e-2, the constraints, the front and the pending points each moving the value by far more than the bound
here: a device that returned zeros, ignored the constraints, the front or P fails).

Tolerances: |value - want|, |H_e - want|, |F_{e,k} - want| <= max(1e-10, 4 ld_diff) scale, the gradient likewise as
tests/test_gpu_ehvi.py applies it -- 1e-10 is tests/test_gpu_ei1.py's bound for the same chains, ld_diff the case's recorded
float64-against-long-double difference of the restatement.  Everything else is bit for bit: the value against the documented rule
formed on the host from factors_out, value-only against value + gradient, a candidate alone against itself in a batch and across the
pass boundary, ensemble-wide launches on against off, K = 0 against the unconstrained entry points in all three call shapes, an
empty front with K = 1 against moe_ei_constrained_mcmc's factors, the ascent against a host-driven loop over the evaluator, the
greedy batch against calls of the ascent fed their predecessors' points.  cehvi_reference.EDGE_CASES and the constructions behind
them add what the first cases could not tell apart: E >= 2 with K >= 2 together (every [e][k] stride, distinct thresholds, across
the pass boundary and through a batch), a belief that changes along a batch (against the restatement under a stale mask word), 64
pending points under masks that differ per member, the constraint roles' variance floors, and E (M + K) = 1024 run once for the
plain and the log form over the same handles.  Every test prints the worst figures it saw (pytest -s)."""
import numpy as np
import pytest

import cehvi_reference as ch
import ehvi3_reference as h3
import ehvi_reference as hr
import kg1_reference as kr
import test_gpu_cei1 as tc
from cornell_moe_amd import _lib, api, expected_hypervolume_improvement_constrained as cehvi

pytestmark = pytest.mark.gpu

LD = ch.LD
_Launches, _host_loop, _same_run = tc._Launches, tc._host_loop, tc._same_run

CASES = ch.ALL_CASES


class _Device(object):
    """the GPs of a problem on the device: objs [M][E], cons [K][E]"""

    def __init__(self, p):
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in row] for row in p.gps]
        K = len(p.gps[0]) - p.M
        self.objs = [[row[r] for row in self.all] for r in range(p.M)]
        self.cons = [[row[p.M + k] for row in self.all] for k in range(K)]

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", front="problem", taus="problem", **kw):
    pending = p.pending if isinstance(pending, str) else pending
    front = p.front if isinstance(front, str) else front
    taus = p.taus if isinstance(taus, str) else taus
    return api.ehvi_constrained_ensemble(D.objs, D.cons, taus, p.ref, front, points, points_being_sampled=pending, **kw)


def _twin_eval(D, p, points, pending, **kw):
    if p.M == 2:
        return api.ehvi_ensemble(D.objs[0], D.objs[1], p.ref, p.front, points, points_being_sampled=pending, **kw)
    return api.ehvi3_ensemble(D.objs[0], D.objs[1], D.objs[2], p.ref, p.front, points, points_being_sampled=pending, **kw)


def _twin_multistart(D, p, gd, bounds, starts, **kw):
    if p.M == 2:
        return api.ehvi_multistart(D.objs[0], D.objs[1], p.ref, p.front, gd, bounds, starts, **kw)
    return api.ehvi3_multistart(D.objs[0], D.objs[1], D.objs[2], p.ref, p.front, gd, bounds, starts, **kw)


def _twin_suggest(D, p, gd, bounds, starts, q, **kw):
    if p.M == 2:
        return api.ehvi_suggest(D.objs[0], D.objs[1], p.ref, p.front, gd, bounds, starts, q, **kw)
    return api.ehvi3_suggest(D.objs[0], D.objs[1], D.objs[2], p.ref, p.front, gd, bounds, starts, q, **kw)


def _errors(value, grad, factors, want, idx):
    """the worst errors over the candidates idx (positions in value / grad / factors and in want alike)"""
    e_v = max(abs(value[i] - float(want[i].value)) / want[i].scale for i in idx)
    e_g = max(float(np.max(np.abs(grad[i] - want[i].grad.astype(np.float64)))) /
              min(want[i].scale, max(1.0, float(np.max(np.abs(want[i].grad))))) for i in idx)
    e_f = max(abs(factors[e, k, i] - float(f)) / want[i].scale for i in idx for e, row in enumerate(want[i].factors)
              for k, f in enumerate(row))
    return e_v, e_g, e_f


# ---- 1. value, gradient and the factors against long double; the host reproduction; the bits of one call ----
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_against_the_long_double_restatement(case):
    p, want = ch.expected(case, LD)
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
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(factors >= 0.0) and np.all(factors[:, 1:] <= 1.0)
    bound = max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, e_f = _errors(value, grad, factors, want, p.checked)
    a_v, a_g, a_f = _errors(value, grad, factors, want, range(C_))
    print("%s: value error %.3g scale, gradient error %.3g, factors' error %.3g scale at the checked candidates (all candidates: "
          "%.3g, %.3g, %.3g; bound %.3g)" % (case.name, e_v, e_g, e_f, a_v, a_g, a_f, bound))
    assert e_v <= bound and e_g <= bound and e_f <= bound, (case.name, e_v, e_g, e_f)
    assert a_v <= bound and a_g <= bound and a_f <= bound, (case.name, a_v, a_g, a_f)
    # the call's value is the documented rule formed on the host from its own factors, bit for bit
    assert np.array_equal(value, ch.host_value(factors))
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], factors[:, :, i]), (case.name, i)
    # neither the pending points, nor the front, nor the constraints are ignored
    assert not np.array_equal(_eval(D, p, p.points, pending=None, want_grad=False), value)
    if case.F:
        assert not np.array_equal(_eval(D, p, p.points, front=None, want_grad=False), value)
    assert not np.array_equal(_twin_eval(D, p, p.points, p.pending, want_grad=False), value)
    D.close()


# ---- 2. K = 0: the unconstrained entry points, all three call shapes ----
@pytest.mark.parametrize("M", (2, 3))
def test_without_constraints_it_is_the_unconstrained_call_bit_for_bit(M):
    p = ch.make_problem(ch.BELIEVED[M])
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    for pending in (p.pending, None):
        v, g, f = api.ehvi_constrained_ensemble(D.objs, None, None, p.ref, p.front, p.points, points_being_sampled=pending,
                                                want_factors=True)
        tv, tg, tm = _twin_eval(D, p, p.points, pending, want_member_values=True)
        assert np.array_equal(v, tv) and np.array_equal(g, tg) and f.shape == (2, 1, len(p.points)) and np.array_equal(f[:, 0], tm)
        got = api.ehvi_constrained_multistart(D.objs, [], [], p.ref, p.front, gd, bounds, starts, want_path=True,
                                              points_being_sampled=pending)
        _same_run(got, _twin_multistart(D, p, gd, bounds, starts, want_path=True, points_being_sampled=pending))
        got = api.ehvi_constrained_suggest(D.objs, None, None, p.ref, p.front, gd, bounds, starts, 2, points_being_sampled=pending)
        twin = _twin_suggest(D, p, gd, bounds, starts, 2, points_being_sampled=pending)
        for key in ("points", "values", "found"):
            assert np.array_equal(got[key], twin[key]), key
    D.close()


# ---- 3. an empty front and K = 1: (EI_1 EI_2) F from moe_ei_constrained_mcmc's factors ----
def test_with_an_empty_front_a_member_is_the_product_of_two_improvements_and_the_feasibility():
    p = ch.make_problem(ch.BELIEVED[2])  # E = 2, K = 1
    D = _Device(p)
    v, g, f = _eval(D, p, p.points, pending=None, front=None, want_factors=True)
    E = len(p.gps)
    _, _, f1 = api.ei_constrained_ensemble(D.objs[0], D.cons, p.taus, p.points, [p.ref[0]] * E, want_factors=True)
    _, _, f2 = api.ei_constrained_ensemble(D.objs[1], D.cons, p.taus, p.points, [p.ref[1]] * E, want_factors=True)
    assert np.array_equal(f1[:, 1], f2[:, 1]) and np.array_equal(f[:, 1], f1[:, 1])  # the feasibility factor
    assert np.array_equal(f[:, 0], f1[:, 0] * f2[:, 0])                               # H_e = EI_1 EI_2, the product rounded once
    members = (f1[:, 0] * f2[:, 0]) * f1[:, 1]
    assert np.array_equal(v, ch.host_value(f)) and np.array_equal(v, (members[0] + members[1]) / 2.0)
    print("F = 0, K = 1: member values %s" % members[:, :3].tolist())
    assert float(np.min(members)) > 1e-6
    D.close()


# ---- 4. across the pass boundary ----
def _across_the_pass_boundary(M, E, K, taus):
    per_pass = _lib.load().moe_ei1_pass_size(8)
    C_ = per_pass + 4
    assert per_pass == 4096
    c = ch.Case("m%d_e%d_k%d_d2_n8_p2_f5_two_passes" % (M, E, K), 44, M, E, K, 2, ch._grid(E, M + K, 8), 2, 5, taus, C_, None, 0.0)
    p = ch.make_problem(c)
    checked = (0, per_pass - 1, per_pass, C_ - 1)
    ref_members = ch.ensemble(p, LD)
    D = _Device(p)
    for pending in (p.pending, None):
        value, grad, factors = _eval(D, p, p.points, pending=pending, want_factors=True)
        v_only, f_only = _eval(D, p, p.points, pending=pending, want_grad=False, want_factors=True)
        assert np.array_equal(v_only, value) and np.array_equal(f_only, factors)
        assert np.array_equal(value, ch.host_value(factors)) and np.all(value >= 0.0)
        for i in checked:
            v1, g1, f1 = _eval(D, p, p.points[i:i + 1], pending=pending, want_factors=True)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], factors[:, :, i]), i
            assert _eval(D, p, p.points[i:i + 1], pending=pending, want_grad=False)[0] == value[i]
        if pending is not None:
            want = {i: ch.evaluate(ref_members, p.points[i]) for i in checked}
            e_v, e_g, e_f = _errors(value, grad, factors, want, checked)
            print("%s: value error %.3g scale, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= 1e-10 and e_g <= 1e-10 and e_f <= 1e-10
    D.close()


@pytest.mark.parametrize("M", (2, 3))
def test_a_candidate_carries_its_bits_across_the_pass_boundary_and_want_grad(M):
    _across_the_pass_boundary(M, 1, 1, (0.0,))


@pytest.mark.parametrize("M", (2, 3))
def test_two_members_with_two_constraints_cross_the_pass_boundary(M):
    """the second pass holds 4 candidates where the first held 4096: every [e][k] block of the per-pass arrays is strided by a pass
    size that is not the call's number of candidates"""
    _across_the_pass_boundary(M, 2, 2, ch.EDGE_TAUS[2])


# ---- 5. the ascent against the host-driven loop ----
MS = dict(tc.MS, starts=12, steps=4, restarts=2)


def _ascent_inputs(d, tolerance):
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], d))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    return starts, gd, np.array([[0.0, 1.0]] * d)


@pytest.mark.parametrize("tolerance", [1e-10, 0.3], ids=["tight", "loose"])
@pytest.mark.parametrize("M", (2, 3))
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(M, tolerance):
    p = ch.make_problem(ch.case(ch.ENSEMBLE2 if M == 2 else ch.ENSEMBLE3))  # E = 3, K = 1, rows 20 / 130 / 300
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], tolerance)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    kw = dict(points_being_sampled=pending)
    plain = api.ehvi_constrained_multistart(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    free = _twin_multistart(D, p, gd, bounds, starts, **kw)
    assert not np.array_equal(free["start_values"], want["start_values"])  # (nor are the constraints)
    for on in (True, False):
        with _Launches(on):
            got = api.ehvi_constrained_multistart(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, want_path=True, **kw)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("M = %d, tolerance %g: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        M, tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"]
    if tolerance < 1e-3:
        assert want["value"] >= want["start_values"].max()
        assert float(np.max(np.abs(want["end_points"] - starts[want["kept_index"]]))) > 1e-3  # (the starts moved)
    D.close()


# ---- 6. greedy batches, a pick believed infeasible by one member ----
def _split_problem(M):
    """E = 2, K = 1, tau = 0: the constraint GP of member 0 observes values about -0.6 (it believes every point feasible), that of
    member 1 values about +0.6 (it believes every point infeasible, with a probability of feasibility that is small and not 0)"""
    p = ch.make_problem(ch.BELIEVED[M])
    rng = np.random.default_rng(5)
    gps = []
    for e, row in enumerate(p.gps):
        con = row[M]
        level = -0.6 if e == 0 else 0.6
        y = level + 0.05 * rng.normal(size=np.asarray(con.y).shape)
        gps.append(list(row[:M]) + [ch.GP(con.cov_type, con.hyper, con.X, y, con.noise, ())])
    return p._replace(gps=gps)


@pytest.mark.parametrize("M", (2, 3))
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit(M):
    p = _split_problem(M)
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.points[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.ehvi_constrained_multistart(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.ehvi_constrained_suggest(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    # on the host, from the members' own means at the picks: member 0 believes every pick feasible, member 1 believes every pick
    # infeasible, each by a margin no rounding crosses
    picks = np.array(want_points)
    mu0, mu1 = D.cons[0][0].mean(picks), D.cons[0][1].mean(picks)
    print("M = %d: greedy values %s; the constraint means at the picks: member 0 %s, member 1 %s (tau = 0)" % (
        M, want_values, mu0.tolist(), mu1.tolist()))
    assert np.all(mu0 <= p.taus[0] - 0.05) and np.all(mu1 >= p.taus[0] + 0.05)
    # the constraints decide what the batch does: the unconstrained batch on the objective GPs alone picks other points
    free = _twin_suggest(D, p, gd, bounds, starts, q, points_being_sampled=pending)
    assert not np.array_equal(free["points"], picks)
    gaps = [float(np.min(np.max(np.abs(picks[:t] - picks[t]), axis=1))) for t in range(1, q)]
    assert min(gaps) >= 1e-3, gaps  # (no pick repeats an earlier one)
    D.close()


@pytest.mark.parametrize("M", (2, 3))
def test_the_batch_of_two_members_with_two_constraints_is_the_ascent_fed_its_predecessor(M):
    """cehvi_reference.MIXED: E = 2, K = 2, d = 13, rows that differ per role and member -- the hand-over between the rounds of a
    batch (the appended pending row, the constraint means [e][k] the beliefs are taken from) at strides that do not collapse"""
    p = ch.make_problem(ch.MIXED[M])
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 2
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.ehvi_constrained_multistart(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.ehvi_constrained_suggest(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gap = float(np.max(np.abs(want_points[1] - want_points[0])))
    print("M = %d, E = 2, K = 2: greedy values %s, the picks %.3g apart" % (M, want_values, gap))
    assert want_values[0] > 0.0 and want_values[1] > 0.0 and gap >= 1e-3
    D.close()


@pytest.mark.parametrize("M", (2, 3))
def test_a_belief_that_changes_along_the_batch_is_worked_out_anew_for_every_pick(M):
    """cehvi_reference.changing_problem: member 1's constraint mean falls through tau at x_0 = 0.5, the pending point lies on the
    infeasible side and the starts on both.  The batch is the ascent fed its predecessors bit for bit; member 1's beliefs along
    pending point and picks, from its own means, are not constant; and every pick's value is the restatement's under the beliefs of
    ALL the points before it, while the restatement that gives every point the FIRST point's belief (a mask word never worked out
    again) lies more than 1e-3 away at a later pick."""
    p, starts = ch.changing_problem(M)
    D = _Device(p)
    _, gd, bounds = _ascent_inputs(3, 1e-10)
    q, tau = ch.CHANGING_Q[M], p.taus[0]
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([p.pending] + [x[None, :] for x in want_points])
        res = api.ehvi_constrained_multistart(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.ehvi_constrained_suggest(D.objs, D.cons, p.taus, p.ref, p.front, gd, bounds, starts, q, points_being_sampled=p.pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    every = np.vstack([p.pending] + [x[None, :] for x in want_points])
    mu0, mu1 = D.cons[0][0].mean(every), D.cons[0][1].mean(every)
    belief = [bool(m <= tau) for m in mu1]
    true_gap, stale_gap = _gaps_to_the_restatement(p, every, want_values)
    print("M = %d: member 1's constraint means at the pending point and the %d picks %s (tau = 0): believed feasible %s; member 0's %s; "
          "values %s; against the restatement %s scale, against the one under the first point's belief %s" % (
              M, q, np.round(mu1, 4).tolist(), belief, np.round(mu0, 3).tolist(), want_values, true_gap, stale_gap))
    assert np.all(np.abs(mu1 - tau) >= ch.MARGIN) and np.all(mu0 <= tau - ch.MARGIN)
    assert len(set(belief)) == 2 and any(belief[j] != belief[t] for t in range(1, q + 1) for j in range(t))
    assert max(true_gap) <= 1e-10 and max(stale_gap[1:]) > 1e-3
    D.close()


def _gaps_to_the_restatement(p, every, values):
    """pick t's value against the restatement conditioned on the points before it, in units of scale: under the believed-feasible
    rule, and with the first point's belief given to every point (member by member)"""
    true_gap, stale_gap = [], []
    for t, v in enumerate(values):
        fed = every[:1 + t]
        members = ch.ensemble(p, LD, pending=fed)
        stale = [ch.remasked(m, [m.mask[0]] * len(fed), p.front) for m in members]
        a, b = ch.evaluate(members, every[1 + t]), ch.evaluate(stale, every[1 + t])
        true_gap.append(abs(v - float(a.value)) / a.scale)
        stale_gap.append(abs(v - float(b.value)) / a.scale)
    return true_gap, stale_gap


# ---- 6b. the constraint roles' floors ----
@pytest.mark.parametrize("M", (2, 3))
def test_on_a_noise_free_constraints_sampled_points_the_feasibility_is_exactly_one_and_zero(M):
    """cehvi_reference.FLOOR: candidates 0 and 1 on sampled points of the noise-free GP of constraint 1, observed 0.2 below and above
    its threshold (tests/test_cehvi_reference.py: the float64 variance there lies under 150 eps^2).  cehvi_feas_kernel's own two
    floors: F under DBL_MIN is exactly 1 and exactly 0, its gradient under 150 eps^2 exactly 0."""
    case = ch.FLOOR[M]
    p, want = ch.expected(case, LD)
    D = _Device(p)
    value, grad, factors = _eval(D, p, p.points, want_factors=True)
    print("M = %d: F_1 at the two sampled points %r, %r; values %r, %r; F_1 elsewhere %s" % (
        M, factors[0, 1, 0], factors[0, 1, 1], value[0], value[1], np.round(factors[0, 1, 2:], 4).tolist()))
    assert factors[0, 1, 0] == 1.0 and factors[0, 1, 1] == 0.0
    assert value[1] == 0.0 and not np.any(grad[1]) and np.all(np.isfinite(grad)) and np.all(np.isfinite(factors))
    # candidate 0 is the product without F_1, and its gradient that of the other factors: against the restatement
    assert value[0] == factors[0, 0, 0] * 1.0 * factors[0, 2, 0] and value[0] > 0.0
    bound = max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, e_f = _errors(value, grad, factors, want, (0, 1))
    print("M = %d: at the two floored candidates value error %.3g scale, gradient error %.3g, factors' error %.3g scale" % (M, e_v, e_g, e_f))
    assert e_v <= bound and e_g <= bound and e_f <= bound
    assert np.all(factors[0, 1, 2:] > 0.0) and np.all(factors[0, 1, 2:] < 1.0)  # (elsewhere the same GP's factor is a probability)
    D.close()


# ---- 7. the believed-feasible rule through the members' values ----
@pytest.mark.parametrize("M", (2, 3))
def test_a_believed_infeasible_point_does_not_shrink_the_members_region(M):
    """tests/test_cehvi_reference.py asserts the construction (margins of 0.05 at every decision); here member 1's hypervolume term
    is the restatement's, which holds pending point 1 back, and NOT the unconstrained call's, which offers it"""
    case = ch.BELIEVED[M]
    p, want = ch.expected(case, LD)
    D = _Device(p)
    v, g, f = _eval(D, p, p.points, want_factors=True)
    tv, tg, tm = _twin_eval(D, p, p.points, p.pending, want_member_values=True)
    bound = max(1e-10, 4.0 * case.ld_diff)
    err = [max(abs(f[e, 0, i] - float(w.factors[e][0])) / w.scale for i, w in enumerate(want)) for e in range(2)]
    gap = [float(np.max(np.abs(f[e, 0] - tm[e]))) for e in range(2)]
    print("M = %d: H_e against the restatement %s scale (bound %.3g); against the unconstrained call's members %s" % (M, err, bound, gap))
    assert max(err) <= bound
    assert np.array_equal(f[0, 0], tm[0])  # member 0 believes all three feasible: the unconstrained member's bits
    assert gap[1] >= 1e-3                  # member 1 holds pending point 1 back: its region stays larger
    assert np.all(f[1, 0] >= tm[1] - 1e-12)
    D.close()


# ---- 7b. sixty-four pending points under a mixed mask ----
@pytest.mark.parametrize("M", (2, 3))
def test_sixty_four_pending_points_under_a_mask_that_differs_per_member(M):
    """cehvi_reference.MASKED (tests/test_cehvi_reference.py qualifies it): cehvi_believed_kernel over 5 x 64 threads with mask rows
    of 64 words; in every member offered outcomes evict front points past index 64 behind skipped ones, and skipped outcomes would
    have joined and dominated later ones.  A member whose mask were all ones gives the other restatement, 1e-3 scale away."""
    case = ch.MASKED[M]
    p, want = ch.expected(case, LD)
    D = _Device(p)
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_factors=True))
    value, grad, factors = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    bound = max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, e_f = _errors(value, grad, factors, want, range(case.C))
    assert e_v <= bound and e_g <= bound and e_f <= bound, (e_v, e_g, e_f)
    assert np.array_equal(value, ch.host_value(factors))
    ones = [ch.remasked(m, [True] * len(p.pending), p.front) for m in ch.ensemble(p, LD)]
    apart = [max(abs(factors[e, 0, i] - float(ones[e].evaluate(x)[2][0])) for i, x in enumerate(p.points)) / want[0].scale for e in range(case.E)]
    print("%s: value error %.3g scale, gradient error %.3g, factors' error %.3g scale (bound %.3g); H_e against the restatement under "
          "the all-ones mask, per member: %s scale" % (case.name, e_v, e_g, e_f, bound, np.round(apart, 5).tolist()))
    assert min(apart) > 1e-3
    D.close()


# ---- 8. behaviour ----
@pytest.mark.parametrize("M", (2, 3))
def test_a_threshold_far_below_every_mean_gives_exactly_zero(M):
    p = ch.make_problem(ch.case(ch.ENSEMBLE2 if M == 2 else ch.ENSEMBLE3))
    D = _Device(p)
    low = min(float(np.min(g.y)) for row in p.gps for g in row) - 100.0
    v, g, f = _eval(D, p, p.points, taus=[low], want_factors=True)
    assert np.all(v == 0.0) and np.all(g == 0.0) and np.all(np.isfinite(f)) and np.all(f[:, 1] == 0.0) and np.any(f[:, 0] > 0.0)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    res = api.ehvi_constrained_multistart(D.objs, D.cons, [low], p.ref, p.front, gd, bounds, starts, points_being_sampled=p.pending)
    assert np.all(res["start_values"] == 0.0) and np.all(np.isfinite(res["end_points"])) and res["value"] == 0.0
    D.close()


def test_a_pending_point_listed_twice_in_a_noise_free_constraint_gp_is_singular():
    """tests/test_gpu_ehvi.py's construction with the noise-free GP as the constraint of the second member: flat index 1 * 3 + 2"""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    objs = [[api.DeviceGP(hyper, X, y, [1e-5]) for _ in range(2)] for _ in range(2)]
    cons = [[api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]]
    ref, front, tau = (1.0, 1.0), [(-0.5, 0.5), (0.5, -0.5)], [0.0]
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.ehvi_constrained_ensemble(objs, cons, tau, ref, front, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (5, 3) and "pending point 3" in str(e.value)
            with pytest.raises(api.SingularMatrixException) as e:
                api.ehvi_constrained_multistart(objs, cons, tau, ref, front, gd, [[0, 1], [0, 1]], starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (5, 3)
    ok = api.ehvi_constrained_ensemble(objs, cons, tau, ref, front, starts, want_grad=False, points_being_sampled=pending[:3])
    assert np.all(np.isfinite(ok))  # (the handles still answer)
    # the handle checks count the GPs flat across roles: a constraint handle equal to an objective handle, a derivative-observing
    # constraint GP
    with pytest.raises(api.InvalidValueException) as e:
        api.ehvi_constrained_ensemble(objs, [objs[0]], tau, ref, front, starts)
    assert "listed twice" in str(e.value)
    deriv = api.DeviceGP([1.3, 0.4, 0.4], X, 0.3 * rng.normal(size=(6, 2)), [1e-2, 1e-2], [0])
    with pytest.raises(api.InvalidValueException) as e:
        api.ehvi_constrained_ensemble(objs, [[cons[0][0], deriv]], tau, ref, front, starts)
    assert "derivative" in str(e.value)
    deriv.close()
    for g in objs[0] + objs[1] + cons[0]:
        g.close()


# ---- 8b. E (M + K) = 1024 exactly, the plain and the log form over the same handles ----
def test_1024_gps_at_the_limit_and_one_member_more_is_refused():
    """E = 128, M = 2, K = 6: pointer tables of 1024 entries, feasibility blocks [128][6], factors_out [128][7][C]"""
    import time
    import log_ehvi_reference as lh
    t0 = time.perf_counter()
    c = ch.LIMIT
    p, want = ch.expected(c, LD)
    want_log = [lh.evaluate(ch.ensemble(p, LD), x) for x in p.points]
    t1 = time.perf_counter()
    D = _Device(p)
    t2 = time.perf_counter()
    assert len(D.objs[0]) == 128 and len(D.cons) == 6 and sum(len(row) for row in D.all) == 1024
    value, grad, factors = _eval(D, p, p.points, want_factors=True)
    assert factors.shape == (128, 7, c.C) and np.all(np.isfinite(grad))
    bound = max(1e-10, 4.0 * c.ld_diff)
    e_v, e_g, e_f = _errors(value, grad, factors, want, range(c.C))
    e_3 = max(abs(factors[e, k, i] - float(want[i].factors[e][k])) / want[i].scale for i in range(c.C) for e in ch.LIMIT_MEMBERS
              for k in range(7))
    assert e_v <= bound and e_g <= bound and e_f <= bound and e_3 <= bound, (e_v, e_g, e_f, e_3)
    assert np.array_equal(value, ch.host_value(factors))
    lv, lg, logs = api.log_ehvi_constrained_ensemble(D.objs, D.cons, p.taus, p.ref, p.front, p.points, points_being_sampled=p.pending,
                                                     want_log_factors=True)
    assert logs.shape == (128, 7, c.C) and np.all(np.isfinite(lv)) and np.all(np.isfinite(lg)) and np.all(np.isfinite(logs))
    l_v = max(abs(lv[i] - float(w.value)) / max(1.0, abs(float(w.value))) for i, w in enumerate(want_log))
    l_g = max(float(np.max(np.abs(lg[i] - w.grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(w.grad)))) for i, w in enumerate(want_log))
    l_f = max(abs(logs[e, r, i] - float(f)) / max(1.0, abs(float(f))) for i, w in enumerate(want_log) for e, row in enumerate(w.log_factors)
              for r, f in enumerate(row))
    l_3 = max(abs(logs[e, r, i] - float(w.log_factors[e][r])) / max(1.0, abs(float(w.log_factors[e][r]))) for i, w in enumerate(want_log)
              for e in ch.LIMIT_MEMBERS for r in range(7))
    assert l_v <= 1e-10 and l_g <= 1e-10 and l_f <= 1e-10 and l_3 <= 1e-10, (l_v, l_g, l_f, l_3)
    assert np.array_equal(lv, lh.host_value(logs))
    t3 = time.perf_counter()
    # one member more: E (M + K) = 1032
    g = p.gps[0]
    extra = [api.DeviceGP(x.hyper * 1.01, x.X, x.y, x.noise, [], cov_type=x.cov_type) for x in g]
    objs = [D.objs[r] + [extra[r]] for r in range(2)]
    cons = [D.cons[k] + [extra[2 + k]] for k in range(6)]
    for call in (api.ehvi_constrained_ensemble, api.log_ehvi_constrained_ensemble):
        with pytest.raises(api.BoundsException) as e:
            call(objs, cons, p.taus, p.ref, p.front, p.points)
        assert (e.value.value, e.value.min, e.value.max) == (129, 1, 128), str(e.value)
    for x in extra:
        x.close()
    D.close()
    t4 = time.perf_counter()
    print("E = 128, K = 6: plain value error %.3g scale, gradient %.3g, factors %.3g (members 0, 63, 127: %.3g; bound %.3g); log value "
          "error %.3g, gradient %.3g, log factors %.3g (members 0, 63, 127: %.3g; bound 1e-10); wall time %.2f s: the long-double "
          "restatements %.2f (less when another test built them), 1024 handles built in %.2f, the device calls %.2f, E = 129 and the "
          "handles closed in %.2f" % (e_v, e_g, e_f, e_3, bound, l_v, l_g, l_f, l_3, t4 - t0, t1 - t0, t2 - t1, t3 - t2, t4 - t3))


# ---- 9. the wrapper, on competing objectives inside a disc ----
@pytest.mark.parametrize("M", (2, 3))
def test_the_wrapper_and_the_optimisation_run_end_to_end(M):
    import wrappers_mirror as cw
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(10, dim))
    centres = [(0.25, 0.25), (0.75, 0.75), (0.25, 0.75)][:M]
    ys = [np.sum((X - np.array(c)) ** 2, axis=1) * 4.0 - 1.0 for c in centres]
    con = np.sum((X - 0.5) ** 2, axis=1)  # feasible inside the disc of radius 0.4 about the centre
    tau = [0.16]
    hypers = np.array([[1.0, 0.5, 0.5], [1.4, 0.45, 0.6], [0.8, 0.6, 0.5]])
    ensembles = []
    for vals in ys + [con]:
        hd = cw.HistoricalData(dim=dim, num_derivatives=0)
        hd.append_sample_points([cw.SamplePoint(X[i], [vals[i]], noise) for i in range(X.shape[0])])
        ensembles.append(cw.GaussianProcessMCMC(hypers, np.full((num_mcmc, 1), noise), hd, []).member_models())
    objective_models, constraint_models = ensembles[:M], ensembles[M:]
    ref = (2.0,) * M
    front = cehvi.feasible_pareto_front(np.stack(ys, axis=1), con[:, None], tau, ref)
    assert int(np.sum(con <= tau[0])) >= 2 and int(np.sum(con > tau[0])) >= 2 and len(front) >= 1
    obj = cehvi.ConstrainedExpectedHypervolumeImprovementMCMC(objective_models, constraint_models, tau, ref)
    assert obj.problem_size == dim and np.array_equal(obj.front, front) and obj.num_objectives == M and obj.num_constraints == 1
    objs = [cehvi._device_members(m) for m in objective_models]
    cons = [cehvi._device_members(m) for m in constraint_models]
    cand = rng.uniform(size=(7, dim))
    want_v, want_g = api.ehvi_constrained_ensemble(objs, cons, tau, ref, front, cand)
    assert np.array_equal(obj.evaluate_at_point_list(cand), want_v) and float(np.max(want_v)) > 0.0
    obj.set_current_point(cand[3])
    assert obj.compute_objective_function() == want_v[3] and np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
    gd = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    bounds = [[0.0, 1.0]] * dim
    points, values, found = cehvi.multistart_constrained_expected_hypervolume_improvement_optimization(
        objective_models, constraint_models, tau, ref, bounds, gd, num_multistarts=16, num_to_sample=3, seed=31)
    assert points.shape == (3, dim) and values.shape == (3,) and np.all(found)
    assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values)) and values[0] > 0.0
    starts = api.latin_hypercube(31, bounds, 16)
    first = api.ehvi_constrained_multistart(objs, cons, tau, ref, front, gd, bounds, starts)
    assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
    # the first pick against the restatement
    gps = [[ch.GP(kr.MATERN, hypers[e], X, y.reshape(-1, 1), [noise], ()) for y in ys + [con]] for e in range(num_mcmc)]
    members = [ch.Member(row, M, tau, ref, front, np.zeros((0, dim)), LD) for row in gps]
    res = ch.evaluate(members, points[0])
    inside = float(np.sum((points[0] - 0.5) ** 2))
    print("M = %d, 10 points, 3 members: a batch of 3 at %s, values %s; the first pick's constraint value %.3f (tau %.2f); its value "
          "%.6g against the restatement's %.6g" % (M, np.round(points, 3).tolist(), [float(v) for v in values], inside, tau[0],
                                                   values[0], float(res.value)))
    assert abs(values[0] - float(res.value)) <= 1e-10 * res.scale
