"""What tests/test_gpu_chebei.py and tests/test_gpu_log_chebei.py leave out of csrc/chebei1.hip and csrc/logchebei1.hip, against the
long-double restatements of tests/chebei_reference.py and tests/log_chebei_reference.py on their EDGE_CASES, which
tests/test_chebei_reference.py and tests/test_log_chebei_reference.py qualify on the CPU (float64 against long double, and each
case reaching what it is there for):

1. M = 6 and M = 7 in both forms, K = 3 and K = 5, an odd dimension under two members; the plain form also with the incumbent
   above every objective, the one regime in which its last, partly filled sweep adds anything but zeros;
2. the log form with the incumbent far above every objective, where the rate is exactly 0 and ell is the cap;
3. ensembles that mix a member of exact zeros (plain form) or of weight exactly 0 (log form) with a live one, in either order;
4. 64 pending points whose deciding ones sit at indices 40, 62 and 63, and greedy batches that fill extension rows 62 and 63;
5. the believed-and-feasible rule inside a greedy batch, a pick believed infeasible by one member among the pending points;
6. handles with a history: calls of other shapes and roles before a call, against the same call on fresh handles.

Tolerances are those two files': max(1e-10, 4 ld_diff) against long double (in units of scale for the plain form; absolute for
logs and relative to the largest entry for the log form's gradient), ld_diff the recorded figure of the Case; everything else bit
for bit, but the host log-sum-exp with E >= 2 (_is_host_rule).  Parts 1, 2 and 4 run those files'
test_against_the_long_double_restatement on the new cases.  Every test prints the worst figures it saw (pytest -s); DESIGN.md
section 5.29 records those of the first run."""
import numpy as np
import pytest

import chebei_reference as ch
import log_chebei_reference as lc
import test_gpu_chebei as tp
import test_gpu_log_chebei as tl
from cornell_moe_amd import api, expected_scalarised_improvement as esi

pytestmark = pytest.mark.gpu

LD = ch.LD
_Launches, _ascent_inputs = tp._Launches, tp._ascent_inputs


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. M = 6 and M = 7 ----
# (the two `above` cases: under an observed incumbent the plain form's last, partly filled sweep holds panels without a width and
#  adds exact zeros, so that a wrong last sweep would pass; with the incumbent above every s_j + 8 tau_j it carries 0.98 of the value)
@pytest.mark.parametrize("name", [ch.M6, ch.M7, ch.M6_ABOVE, ch.M7_ABOVE])
def test_six_and_seven_objectives_against_long_double(name):
    tp.test_against_the_long_double_restatement(ch.case(name))


@pytest.mark.parametrize("case", lc.M67, ids=_ids(lc.M67))
def test_the_log_of_six_and_seven_objectives_against_long_double(case):
    tl.test_against_the_long_double_restatement(case)


# ---- 2. the log form with the incumbent far above: the cap binds ----
@pytest.mark.parametrize("case", lc.ABOVE, ids=_ids(lc.ABOVE))
def test_the_log_form_where_the_rate_is_exactly_zero(case):
    tl.test_against_the_long_double_restatement(case)
    p = lc.make_problem(case)
    D = tl._Device(p)
    value, factors = tl._eval(D, p, p.points, want_grad=False, want_factors=True)
    plain, members = api.ei_chebyshev_ensemble(D.objs, p.scal, p.best, p.points, want_grad=False, want_member_values=True)
    print("%s: LA %.6g .. %.6g, the plain form's member values %.6g .. %.6g" % (case.name, factors.min(), factors.max(), members.min(),
                                                                              members.max()))
    assert np.array_equal(value, factors[0, 0]) and np.all(members > 0.0) and np.array_equal(plain, members[0])
    # (log of the plain form: both restatements' bounds, as tests/test_log_chebei_reference.py holds them together)
    assert float(np.max(np.abs(np.exp(factors[0, 0]) / members[0] - 1.0))) <= 1e-9
    D.close()


# ---- 3. mixed ensembles ----
def test_a_member_of_exact_zeros_beside_a_live_one():
    case = ch.case(ch.MIXED)
    tp.test_against_the_long_double_restatement(case)  # (value == _host_mean(members) bit for bit among it)
    p = ch.make_problem(case)
    D = tp._Device(p)
    for on in (True, False):
        with _Launches(on):
            value, grad, members = tp._eval(D, p, p.points, want_member_values=True)
            alone = [api.ei_chebyshev_ensemble([[col[e]] for col in D.objs], p.scal[0], [p.best[0][e]], p.points) for e in (0, 1)]
        assert not np.any(members[0]) and np.all(members[1] > 0.0)
        assert not np.any(alone[0][0]) and not np.any(alone[0][1])  # member 0 alone: exact zeros, a zero gradient
        # its share of the sums is an exact zero: the ensemble's value and gradient are member 1's, halved
        assert np.array_equal(members[1], alone[1][0]) and np.array_equal(value, members[1] / 2.0)
        assert np.array_equal(grad, alone[1][1] / 2.0) and np.all(np.max(np.abs(grad), axis=1) > 0.0)
    print("%s: values %s are member 1's halved, bit for bit, and so is the gradient" % (case.name, value))
    D.close()


@pytest.mark.parametrize("case", lc.MIXED, ids=_ids(lc.MIXED))
def test_a_member_of_weight_exactly_zero_beside_a_live_one(case):
    p, want = lc.expected(case, LD)
    dead = lc.stalled_member(case)
    live = 1 - dead
    D = tl._Device(p)
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(tl._eval(D, p, p.points, want_factors=True))
    value, grad, factors = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(factors))
    assert np.all(np.max(np.abs(grad), axis=1) > 0.0)
    # the stalled member's LA, of order -1e6, is held to its own recorded figure, everything else to the figure without it
    bound, bound_dead = max(1e-10, 4.0 * lc.MIXED_LIVE[case.name]), max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, _ = tl._errors(value, grad, factors, want)
    e_dead = max(abs(factors[dead, 0, i] - float(w.log_factors[dead][0])) for i, w in enumerate(want))
    e_f = max(abs(factors[e, r, i] - float(v)) for i, w in enumerate(want) for e, row in enumerate(w.log_factors) for r, v in enumerate(row)
              if (e, r) != (dead, 0))
    print("%s: value error %.3g, gradient error %.3g, group values' error %.3g (bound %.3g); the stalled member's LA %.6g .. %.6g, error "
          "%.3g (bound %.3g)" % (case.name, e_v, e_g, e_f, bound, factors[dead, 0].min(), factors[dead, 0].max(), e_dead, bound_dead))
    assert e_v <= bound and e_g <= bound and e_f <= bound and e_dead <= bound_dead
    # the weight exp(LL - m) of the stalled member is exactly 0: the value is the live member's LL - log 2
    LL = factors[:, 0, :].copy()
    for r in range(1, 1 + case.K):
        LL = LL + factors[:, r, :]
    assert np.all(LL[dead] - LL[live] < -745.0) and tl._is_host_rule(value, factors)
    assert np.all(np.abs(value - (LL[live] - np.log(2.0))) <= 8.0 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(value)))
    # ... and the gradient the live member's own, which a call with that member alone returns
    g_live = api.log_ei_chebyshev_constrained_ensemble([[col[live]] for col in D.objs], [[col[live]] for col in D.cons] or None,
                                                       D.tau or None, p.scal, [p.best[live]], p.points)[1]
    assert np.array_equal(grad, g_live)
    assert np.array_equal(tl._eval(D, p, p.points, want_grad=False), value)
    for i in (0, len(p.points) - 1):
        v1, g1, f1 = tl._eval(D, p, p.points[i:i + 1], want_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], factors[:, :, i])
    D.close()


# ---- 4. sixty-four pending points ----
def test_sixty_four_pending_points_with_the_incumbents_at_points_40_and_63():
    case = ch.case(ch.P64)
    tp.test_against_the_long_double_restatement(case)
    p = ch.make_problem(case)
    D = tp._Device(p)
    value, members = tp._eval(D, p, p.points, want_grad=False, want_member_values=True)
    short, short_members = tp._eval(D, p, p.points, pending=p.pending[:63], want_grad=False, want_member_values=True)
    assert np.all(short != value) and np.all(short_members[0] != members[0])  # point 63 is member 0's incumbent
    keep = [i for i in range(64) if i != ch.P64_SLOTS[1][2]]
    _, less = tp._eval(D, p, p.points, pending=p.pending[keep], want_grad=False, want_member_values=True)
    assert np.all(less[1] != members[1])  # point 40 is member 1's
    print("%s: member 0's values %s, without point 63 %s; member 1's %s, without point 40 %s" % (
        case.name, members[0], short_members[0], members[1], less[1]))
    D.close()


def test_the_log_form_at_sixty_four_pending_points_with_point_62_believed_infeasible():
    case = lc.P64
    tl.test_against_the_long_double_restatement(case)
    p = lc.make_problem(case)
    D = tl._Device(p)
    value, factors = tl._eval(D, p, p.points, want_grad=False, want_factors=True)
    short, short_factors = tl._eval(D, p, p.points, pending=p.pending[:63], want_grad=False, want_factors=True)
    assert np.all(short != value) and np.all(short_factors[0, 0] != factors[0, 0])  # point 63 is member 0's incumbent
    # member 0's incumbent is NOT its lowest believed outcome, point 62, which it believes infeasible; without the constraint it is
    open_ = api.log_ei_chebyshev_constrained_ensemble(D.objs, None, None, p.scal, p.best, p.points, points_being_sampled=p.pending,
                                                      want_grad=False, want_factors=True)[1]
    assert not np.array_equal(open_[0, 0], factors[0, 0]) and np.array_equal(open_[1, 0], factors[1, 0])
    print("%s: member 0's LA %s, without point 63 %s, with the mask dropped %s" % (case.name, factors[0, 0], short_factors[0, 0],
                                                                                   open_[0, 0]))
    D.close()


def _batch_is_the_chain(ascent, suggest, scal, best, gd, bounds, starts, pending, q):
    """suggest(...) is q calls of ascent(...), each fed its predecessors' points, bit for bit, launches on and off"""
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = ascent(scal[t], best[t], gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = suggest(scal, best, gd, bounds, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    return np.array(want_points), want_values


def _three_weighted_rounds(gps, M):
    w = esi.sample_simplex_weights(3, M, 5)
    scal = np.array([ch.scalarisation(w[t], [ch.IDEAL] * M, [ch.NADIR] * M) for t in range(3)])
    return scal, np.array([ch.observed_best([row[:M] for row in gps], scal[t]) for t in range(3)])


def test_a_batch_that_fills_extension_rows_62_and_63():
    p = ch.make_problem(ch.case(ch.P64))  # M = 3, E = 2
    D = tp._Device(p)
    starts, gd, bounds = _ascent_inputs(3, 1e-10)
    scal, best = _three_weighted_rounds(p.gps, p.M)
    points, values = _batch_is_the_chain(lambda *a, **k: api.ei_chebyshev_multistart(D.objs, *a, **k),
                                         lambda *a, **k: api.ei_chebyshev_suggest(D.objs, *a, **k), scal, best, gd, bounds, starts,
                                         p.pending[:62], 3)
    print("plain form, p = 62, q = 3: greedy values %s" % values)
    assert len(np.unique(points, axis=0)) == 3
    with pytest.raises(api.BoundsException):
        api.ei_chebyshev_suggest(D.objs, scal, best, gd, bounds, starts, 3, points_being_sampled=p.pending[:63])
    D.close()


def test_a_log_batch_that_fills_extension_rows_62_and_63():
    p = lc.make_problem(lc.P64)  # M = 3, E = 2, K = 1
    D = tl._Device(p)
    starts, gd, bounds = _ascent_inputs(3, 1e-10)
    scal, best = _three_weighted_rounds(p.gps, p.M)
    points, values = _batch_is_the_chain(
        lambda *a, **k: api.log_ei_chebyshev_constrained_multistart(D.objs, D.cons, D.tau, *a, **k),
        lambda *a, **k: api.log_ei_chebyshev_constrained_suggest(D.objs, D.cons, D.tau, *a, **k), scal, best, gd, bounds, starts,
        p.pending[:62], 3)
    print("log form, p = 62, q = 3, K = 1: greedy values %s" % values)
    assert len(np.unique(points, axis=0)) == 3
    with pytest.raises(api.BoundsException):
        api.log_ei_chebyshev_constrained_suggest(D.objs, D.cons, D.tau, scal, best, gd, bounds, starts, 3,
                                                 points_being_sampled=p.pending[:63])
    D.close()


# ---- 5. the believed-and-feasible rule inside a batch ----
def test_a_pick_one_member_believes_infeasible_inside_a_batch():
    case = lc.HALF  # M = 2, E = 2, K = 1, p = 2
    p = lc.make_problem(case)
    D = tl._Device(p)
    starts, gd, bounds = _ascent_inputs(3, 1e-10)
    scal, best = lc.batch_rounds(p, 3)
    points, values = _batch_is_the_chain(
        lambda *a, **k: api.log_ei_chebyshev_constrained_multistart(D.objs, D.cons, D.tau, *a, **k),
        lambda *a, **k: api.log_ei_chebyshev_constrained_suggest(D.objs, D.cons, D.tau, *a, **k), scal, best, gd, bounds, starts,
        p.pending, 3)
    # round 2's pending points in the order the batch appended them: the problem's two, then picks 0 and 1
    fed = np.ascontiguousarray(np.vstack([p.pending, points[:2]]))
    refs = {T: lc.ensemble(p.gps, p.M, p.taus, fed, T) for T in (np.float64, LD)}
    masks = [list(m.mask) for m in refs[np.float64]]
    means = [float(v) for v in refs[np.float64][0].constraint_means[0]]
    sa, sb = ch.split(scal[2])
    outcomes = [[float(v) for v in ch.scalarised_outcomes(sa, sb, m.outcomes, np.float64)] for m in refs[np.float64]]
    print("half: picks %s, values %s; member 0 believes %s of (pending, picks 0 and 1) feasible (constraint means %s), member 1 %s"
          % (points.tolist(), values, masks[0], means, masks[1]))
    # not vacuous: member 0 believes a pick infeasible that member 1 believes feasible, clear of rounding, every believed outcome lies
    # below the incumbents, and member 0's lowest believed outcome is one that it believes infeasible -- the mask decides its incumbent
    assert not all(masks[0][2:]) and all(masks[1]) and min(abs(v) for v in means) > 1e-6
    assert max(max(o) for o in outcomes) < lc.HIGH_BEST and not masks[0][int(np.argmin(outcomes[0]))]
    x = starts[:1]  # one fixed candidate: the first start, whose value the round's ascent reports
    want = {T: lc.evaluate(refs[T], x[0], scal[2], best[2]) for T in refs}
    own = max(abs(float(a - LD(b))) for hv, lv in zip(want[LD].log_factors, want[np.float64].log_factors) for a, b in zip(hv, lv))
    bound = max(1e-10, 4.0 * max(case.ld_diff, own))  # (the case's recorded figure and this evaluation's own)
    value, grad, factors = tl._eval(D, p, x, pending=fed, scal=scal[2], best=best[2], want_factors=True)
    e_v, e_g, e_f = tl._errors(value, grad, factors, [want[LD]])
    print("half: round 2 at the first start: value error %.3g, gradient error %.3g, group values' error %.3g (bound %.3g)" % (
        e_v, e_g, e_f, bound))
    assert e_v <= bound and e_g <= bound and e_f <= bound
    # the batch's own round 2 saw the same: its ascent, fed the picks in that order, reports this value for the first start
    round2 = tl._ascent(D, p, gd, bounds, starts, scal=scal[2], best=best[2], points_being_sampled=fed)
    assert round2["start_values"][0] == value[0] and np.array_equal(round2["point"], points[2]) and round2["value"] == values[2]
    # ... and with the mask dropped member 0's LA is another, member 1's the same bits
    open_ = api.log_ei_chebyshev_constrained_ensemble(D.objs, None, None, scal[2], best[2], x, points_being_sampled=fed, want_grad=False,
                                                      want_factors=True)[1]
    assert open_[0, 0, 0] != factors[0, 0, 0] and open_[1, 0, 0] == factors[1, 0, 0]
    D.close()


# ---- 6. handles with a history ----
def _history_calls(h, gps, points, pending):
    """the five calls over the 16 handles h (gps: what they hold, for the incumbents); every result as a tuple of arrays"""
    def scal_best(rows, M):
        w = np.arange(1.0, M + 1.0)
        s = ch.scalarisation(w / w.sum(), [ch.IDEAL] * M, [ch.NADIR] * M)
        return s, ch.observed_best([[gps[i] for i in row[:M]] for row in rows], s)

    def log_call(rows, M, taus, C_, p):
        s, b = scal_best(rows, M)
        objs = [[h[row[j]] for row in rows] for j in range(M)]
        cons = [[h[row[M + k]] for row in rows] for k in range(len(taus))]
        return api.log_ei_chebyshev_constrained_ensemble(objs, cons, list(taus), s, b, points[:C_], points_being_sampled=pending[:p],
                                                         want_factors=True)

    def plain_call(rows, M, C_, want_grad):
        s, b = scal_best(rows, M)
        out = api.ei_chebyshev_ensemble([[h[row[j]] for row in rows] for j in range(M)], s, b, points[:C_], want_grad=want_grad)
        return out if want_grad else (out,)

    return [
        lambda: log_call([list(range(16))], 8, lc.TAUS[8], 8, 2),
        lambda: plain_call([[0, 1]], 2, 1, True),
        lambda: log_call([[5, 6, 7, 8], [9, 10, 11, 12]], 3, lc.TAUS[1], 5, 4),  # other roles; GP 5 comes first
        lambda: plain_call([list(range(6)), list(range(6, 12))], 6, 3, False),
        lambda: log_call([list(range(16))], 8, lc.TAUS[8], 8, 2),
    ]


def test_handles_with_a_history_answer_as_fresh_ones_do():
    p = lc.make_problem(lc.case("log_m8_e2_k8_d3_n20_p2"))
    gps = p.gps[0]  # 16 GPs, n = 20, d = 3
    rng = np.random.default_rng(61)
    points, pending = rng.uniform(0.1, 0.9, size=(8, 3)), rng.uniform(0, 1, size=(4, 3))

    def make():
        return [api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in gps]

    used = make()
    results = [call() for call in _history_calls(used, gps, points, pending)]
    for k in range(5):
        fresh = make()
        want = _history_calls(fresh, gps, points, pending)[k]()
        assert len(want) == len(results[k]) and all(np.array_equal(a, b) for a, b in zip(results[k], want)), "call %d" % (k + 1)
        assert all(np.all(np.isfinite(a)) for a in want)
        for g in fresh:
            g.close()
    assert all(np.array_equal(a, b) for a, b in zip(results[0], results[4]))
    print("five calls over 16 handles: each bit-equal to the same call on fresh handles; values %s" % [r[0].tolist() for r in results])
    # a handle in two roles is refused: an objective's as a constraint, and as a second objective, in either form
    s = ch.scalarisation([0.5, 0.5], [ch.IDEAL] * 2, [ch.NADIR] * 2)
    with pytest.raises(api.InvalidValueException):
        api.log_ei_chebyshev_constrained_ensemble([[used[0]], [used[1]]], [[used[0]]], [0.0], s, [0.3], points[:2], want_grad=False)
    with pytest.raises(api.InvalidValueException):
        api.log_ei_chebyshev_constrained_ensemble([[used[0]], [used[0]]], None, None, s, [0.3], points[:2], want_grad=False)
    with pytest.raises(api.InvalidValueException):
        api.ei_chebyshev_ensemble([[used[0]], [used[0]]], s, [0.3], points[:2], want_grad=False)
    # ... and the handles still answer
    again = _history_calls(used, gps, points, pending)[1]()
    assert all(np.array_equal(a, b) for a, b in zip(again, results[1]))
    for g in used:
        g.close()
