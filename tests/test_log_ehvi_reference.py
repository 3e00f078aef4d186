"""CPU tests (-m "not gpu") of tests/log_ehvi_reference.py, the restatement tests/test_gpu_log_ehvi.py checks the device against: the
member's log strip sum and its four coefficients in long double against mpmath at 60 digits (the gradient by mpmath.diff of the log
of the plain strip sum; bound 1e-13 relative to max(1, |.|)), every case-shift qualified with float64 within 2.5e-11 of long double
(a quarter of the GPU bound, the margin tests/test_logcei1_reference.py keeps), exp of the value at shift 0 against
tests/cehvi_reference.py's plain value, the three constructions (1025 strips, the rho = 1 strip, the floor) and the stall problem;
the edge cases: E = 2 with K >= 2 against cehvi_reference.swapped, the constraint role's floor, the hopeless member, the limit and
mixed-mask problems in logs, and the COUNTS of lane_replay, a float64 replay of logehvi1_strip_kernel's lane order, per case."""
import math

import mpmath as mp  # (the outside truth: a machine without it fails here, it does not skip)
import numpy as np
import pytest

import cehvi_reference as ch
import cei1_reference as cr
import ei1_reference as er
import log_ehvi_reference as lh

LD = lh.LD
QUALIFY = 2.5e-11
PIN = 1e-13


def _mp_log_strips(mu1, v1, mu2, v2, front, ref):
    """(log S, its four derivatives) of the plain strip sum at 60 digits"""
    def log_S(mu1, v1, mu2, v2):
        s1, s2 = mp.sqrt(v1), mp.sqrt(v2)

        def psi(t, mu, s):
            z = (t - mu) / s
            return (t - mu) * mp.ncdf(z) + s * mp.npdf(z)
        F = len(front)
        u = [f[0] for f in front] + [ref[0]]
        v = [ref[1]] + [f[1] for f in front]
        total, prev = mp.mpf(0), mp.mpf(0)
        for i in range(F + 1):
            b = psi(mp.mpf(u[i]), mu1, s1)
            total += (b - prev) * psi(mp.mpf(v[i]), mu2, s2)
            prev = b
        return mp.log(total)
    a = [mp.mpf(x) for x in (mu1, v1, mu2, v2)]
    return log_S(*a), [mp.diff(lambda t, k=k: log_S(*[t if j == k else a[j] for j in range(4)]), a[k]) for k in range(4)]


@pytest.mark.parametrize("F,trials", [(0, 3), (2, 3), (65, 3), (300, 1)])
def test_the_member_agrees_with_mpmath(F, trials):
    mp.mp.dps = 60
    rng = np.random.default_rng(1 + F)
    worst = {}
    for shift in (0.0, 3.0, 8.0, 20.0):
        for _ in range(trials):
            uu = np.sort(rng.uniform(-1, 1.4, F))
            vv = np.sort(rng.uniform(-1, 1.3, F))[::-1]
            front = [(float(uu[i] - shift), float(vv[i] - shift)) for i in range(F)]
            ref = (1.5 - shift, 1.4 - shift)
            mu1, mu2 = (float(x) for x in rng.normal(0, 0.3, 2))
            v1, v2 = (float(x) for x in rng.uniform(0.01, 0.5, 2))
            true_L, true_c = _mp_log_strips(mu1, v1, mu2, v2, front, ref)
            for T in (np.float64, LD):
                L, c, low, _ = lh.log_strips(mu1, v1, mu2, v2, np.array(front).reshape(-1, 2), ref, T)
                assert np.isfinite(L) and all(np.isfinite(x) for x in c)
                e_v = abs(float(mp.mpf(float(L)) - true_L)) / max(1.0, abs(float(true_L)))
                top = max(1.0, max(abs(float(x)) for x in true_c))
                e_c = max(abs(float(mp.mpf(float(c[k])) - true_c[k])) for k in range(4)) / top
                key = (shift, T.__name__)
                worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0, 0.0)), (e_v, e_c, -low)))
    for key in sorted(worst):
        print("F = %d, shift %g, %s: L error %.2e, coefficients' error %.2e (relative to max(1, |true|)); lowest z %.1f" % (
            (F,) + key + worst[key][:2] + (-worst[key][2],)))
    # long double, what the device is checked against, is pinned; float64 (logcei1_reference's scalars take Phi directly down to -3,
    # 1e-16 absolute on a Phi of 1e-3) only has to stay inside the qualification margin
    for key, w in worst.items():
        assert max(w[:2]) <= (PIN if key[1] == "longdouble" else QUALIFY), (key, w)


def _differences(want, got):
    e_v = max(abs(float(w.value) - float(g.value)) / max(1.0, abs(float(w.value))) for w, g in zip(want, got))
    e_g = max(float(np.max(np.abs(w.grad - g.grad))) / max(1.0, float(np.max(np.abs(w.grad)))) for w, g in zip(want, got))
    e_f = max(abs(float(a) - float(b)) / max(1.0, abs(float(a))) for w, g in zip(want, got)
              for ra, rb in zip(w.log_factors, g.log_factors) for a, b in zip(ra, rb))
    return e_v, e_g, e_f


@pytest.mark.parametrize("case,shift", lh.CASE_SHIFTS, ids=["%s-r%g-t%g" % (c.name, s[0], s[1]) for c, s in lh.CASE_SHIFTS])
def test_every_case_shift_qualifies(case, shift):
    p, members, want = lh.expected(case, shift, LD)
    _, members64, got = lh.expected(case, shift, np.float64)
    for w in want + got:
        assert np.isfinite(w.value) and np.all(np.isfinite(w.grad)) and all(np.isfinite(f) for row in w.log_factors for f in row)
    e_v, e_g, e_f = _differences(want, got)
    low = min(a for w in want for a in w.args)
    print("%s %s: float64 - long double value %.3g, gradient %.3g, log factors %.3g (relative, bound %.3g); lowest z %.1f, lowest "
          "value %.1f, front sizes %s, strips skipped in float64 %d" % (case.name, shift, e_v, e_g, e_f, QUALIFY, low,
                                                                         min(float(w.value) for w in want),
                                                                         [len(m.front) for m in members], sum(g.skipped for g in got)))
    assert e_v <= QUALIFY and e_g <= QUALIFY and e_f <= QUALIFY
    # the same join decisions in both arithmetics
    assert [len(m.front) for m in members] == [len(m.front) for m in members64]
    assert [list(m.mask) for m in members] == [list(m.mask) for m in members64]
    # the gradient is no zero and the pending points are not ignored
    assert all(float(np.max(np.abs(w.grad))) > 0.0 for w in want)
    if shift[0] > 0:
        assert low < -6.0 or case.name == lh.FLOOR.name  # (the shift reaches the fraction's regime)


@pytest.mark.parametrize("case", lh.ALL_CASES, ids=[c.name for c in lh.ALL_CASES])
def test_exp_of_the_value_is_the_plain_value_at_shift_zero(case):
    p, members, want = lh.expected(case, lh.SHIFTS[0], LD)
    worst = 0.0
    for x, w in zip(p.points, want):
        plain = ch.evaluate(members, x)  # (the same members under cehvi_reference's plain rule)
        A = float(plain.value)
        bound = 1e-10 * plain.scale + 1e-10 * A * max(1.0, abs(math.log(A)) if A > 0 else 1.0)
        worst = max(worst, abs(math.exp(float(w.value)) - A) / bound)
    print("%s: |exp(value) - plain value| at most %.3g of the sum of the two bounds" % (case.name, worst))
    assert worst <= 1.0


def test_the_full_front_takes_every_pending_point_without_evicting():
    p, members, want = lh.expected(lh.FULL, lh.SHIFTS[0], LD)
    for T in (LD, np.float64):
        m = lh.expected(lh.FULL, lh.SHIFTS[0], T)[1][0]
        assert len(p.front) == 960 and len(p.pending) == 64 and [tuple(x) for x in m.log] == [("joined", 0)] * 64
        assert len(m.front) == 1024  # 1025 strips
    margin = ch.join_margin(p.front, members[0].offered, p.ref, 2)
    print("full front: 1024 points, the smallest distance of a join decision from flipping %.3g" % margin)
    assert margin >= 1e-7
    for shift in lh.SHIFTS[1:]:
        assert len(lh.expected(lh.FULL, shift, LD)[1][0].front) == 960  # (the lowered reference point leaves the outcomes outside)


def test_the_ulp_front_has_a_strip_of_weight_zero_in_float64():
    p, _, got = lh.expected(lh.ULP, lh.SHIFTS[0], np.float64)
    assert p.front[1, 0] == np.nextafter(p.front[0, 0], 1.0) and p.front[1, 0] > p.front[0, 0]
    skipped = [g.skipped for g in got]
    print("rho = 1: strips skipped in float64 per candidate %s" % skipped)
    assert max(skipped) >= 1


def test_the_floor_candidates_lie_under_the_floor():
    p, members, _ = lh.expected(lh.FLOOR, lh.SHIFTS[0], np.float64)
    m = members[0]
    var = [float(cr.moments(m.models[0], m.bases[0], x)[1]) for x in p.points]
    print("floor: float64 variances of objective 1 at the candidates %s against the floor %.3g" % (var, er.MIN_VAR_GRAD_EI))
    assert var[0] < 1e-12 and var[1] < 1e-12 and min(var[2:]) > 1e-6


MIXED_SHIFTS = [(c, s) for c in lh.MIXED for s in lh.SHIFTS]


@pytest.mark.parametrize("case,shift", MIXED_SHIFTS, ids=["%s-r%g-t%g" % (c.name, s[0], s[1]) for c, s in MIXED_SHIFTS])
def test_members_and_constraints_together_are_told_apart(case, shift):
    """E = 2 with K >= 2.  At shift 0 every exchange of cehvi_reference.swapped (two constraint GPs within a member, the members'
    GPs of one constraint, two thresholds) moves the log value and its gradient by at least 1e-6 relative, 10^4 times the GPU bound,
    at every checked candidate -- no [e][k] order but the documented one passes the device test.  Under a lowered reference point
    or lowered thresholds one member's weight exp(LL_e - m) falls to 1e-7 and below (to exactly 0 under (8, 2) at some candidates),
    and an exchange within that member cannot move the VALUE by 1e-6 whatever the seed (each of the twenty-one seeds tried fails there); what
    the device test compares there entry by entry is log_factors [e][k], and the condition is that those entries tell (e, k) apart:
    the two members' log F of one constraint lie 1e-3 relative apart at every checked candidate, and with K = 2 any two of the
    four lie 1e-4 apart (the transposed order [k][e] exchanges (0, 1) with (1, 0))."""
    assert case in lh.ALL_CASES and case in ch.EDGE_CASES and case.E == 2 and case.K >= 2
    p, members = lh.shifted(case, shift, np.float64)
    got = {i: lh.evaluate(members, p.points[i]) for i in p.checked}
    logs = np.array([[[float(f) for f in row[1:]] for row in got[i].log_factors] for i in p.checked])  # [checked][E][K]
    rel = lambda a, b: np.abs(a - b) / np.maximum(1.0, np.maximum(np.abs(a), np.abs(b)))
    members_apart = float(np.min(rel(logs[:, 0], logs[:, 1])))
    flat = logs.reshape(len(p.checked), -1)
    pairs_apart = min(float(np.min(rel(flat[:, a], flat[:, b]))) for a in range(flat.shape[1]) for b in range(a))
    print("%s %s: the members' log feasibility factors lie at least %.3g relative apart, any two of them %.3g" % (
        case.name, shift, members_apart, pairs_apart))
    assert members_apart >= ch.FACTORS_APART and (case.K > 2 or pairs_apart >= 0.1 * ch.FACTORS_APART)  # (10^6 times the GPU bound)
    if shift != lh.SHIFTS[0]:
        return
    worst = {}
    for what, q in ch.swapped(p):
        alt = lh.reshifted(ch.ensemble(q, np.float64), q.ref, q.front, q.taus)
        moved_v = moved_g = np.inf
        for i in p.checked:
            w = lh.evaluate(alt, p.points[i])
            moved_v = min(moved_v, abs(float(w.value - got[i].value)) / max(1.0, abs(float(got[i].value))))
            moved_g = min(moved_g, float(np.max(np.abs(w.grad - got[i].grad))) / max(1.0, float(np.max(np.abs(got[i].grad)))))
        worst[what] = min(moved_v, moved_g)
        assert moved_v >= ch.SWAP_MOVES and moved_g >= ch.SWAP_MOVES, (case.name, shift, what, moved_v, moved_g)
    print("%s %s: the exchange that moves value or gradient least, %s: %.3g relative at its weakest checked candidate" % (
        case.name, shift, min(worst, key=worst.get), min(worst.values())))
    assert len(worst) == (4 * case.K if case.K > 2 else 5)


def test_the_constraint_floor_candidate_lies_under_the_floor_on_the_feasible_side():
    c = lh.CFLOOR
    assert lh.shifts_of(c) == lh.CFLOOR_SHIFTS and all(s[1] == 0.0 for s in lh.CFLOOR_SHIFTS) and c.E == 1 and c.K == 2
    for shift in lh.CFLOOR_SHIFTS:
        for T in (np.float64, LD):
            p, members, want = lh.expected(c, shift, T)
            m = members[0]
            con = p.gps[0][2]
            row = ch.FLOOR_ROWS[2][0]
            assert float(con.noise[0]) == 0.0 and np.array_equal(p.points[0], con.X[row]) and float(con.y[row, 0]) == p.taus[0] - ch.FLOOR_GAP
            var = [float(cr.moments(m.models[2], m.bases[2], x)[1]) for x in p.points]
            assert var[0] < (er.MIN_VAR_GRAD_EI if T is np.float64 else 1e-16) and min(var[1:]) > 1e-6
            assert float(want[0].log_factors[0][1]) == 0.0 and all(float(w.log_factors[0][1]) < 0.0 for w in want[1:])
    # the other side is the one that does not qualify: log F_1 of order -1e28
    p2 = ch.make_problem(ch.FLOOR2)
    m2 = ch.ensemble(p2, np.float64)[0]
    low = float(lh.member_logs(m2, p2.points[1])[0][1])
    print("the constraint floor: float64 variance %.3g at candidate 0; log F_1 on the infeasible side %.3g" % (var[0], low))
    assert low < -1e27


@pytest.mark.parametrize("shift", lh.SHIFTS, ids=["r%g-t%g" % s for s in lh.SHIFTS])
def test_the_hopeless_members_weight_underflows(shift):
    for T in (np.float64, LD):
        p, members, want = lh.expected(lh.HOPELESS, shift, T)
        gaps = []
        for w in want:
            LL = [float(sum(row[1:], row[0])) for row in w.log_factors]
            gaps.append(LL[1] - LL[0])
            assert LL[1] - LL[0] < lh.HOPELESS_GAP and math.exp(LL[1] - LL[0]) == 0.0 and all(np.isfinite(f) for row in w.log_factors for f in row)
            # the value is member 0's total less log 2 and the gradient member 0's own
            assert abs(float(w.value) - (LL[0] - math.log(2.0))) <= 1e-15 * max(1.0, abs(LL[0]))
    print("hopeless %s: LL_1 - LL_0 per candidate %s" % (shift, np.round(gaps, 1).tolist()))


def test_the_limit_case_qualifies_in_logs():
    c = ch.LIMIT
    p, _ = ch.expected(c, LD)
    want = [lh.evaluate(ch.ensemble(p, LD), x) for x in p.points]
    got = [lh.evaluate(ch.ensemble(p, np.float64), x) for x in p.points]
    e_v, e_g, e_f = _differences(want, got)
    print("%s: float64 - long double value %.3g, gradient %.3g, log factors %.3g (relative, bound %.3g)" % (c.name, e_v, e_g, e_f, QUALIFY))
    assert e_v <= QUALIFY and e_g <= QUALIFY and e_f <= QUALIFY
    for w in want:
        LL = [float(sum(row[1:], row[0])) for row in w.log_factors]
        assert len(set(LL)) == c.E and all(np.isfinite(LL)) and float(np.max(np.abs(w.grad))) > 1e-3


def test_the_mixed_mask_problem_qualifies_in_logs():
    p, _ = ch.expected(ch.MASKED[2], LD)
    want = [lh.evaluate(ch.ensemble(p, LD), x) for x in p.points]
    got = [lh.evaluate(ch.ensemble(p, np.float64), x) for x in p.points]
    e_v, e_g, e_f = _differences(want, got)
    print("%s: float64 - long double value %.3g, gradient %.3g, log factors %.3g (relative, bound %.3g)" % (p.name, e_v, e_g, e_f, QUALIFY))
    assert e_v <= QUALIFY and e_g <= QUALIFY and e_f <= QUALIFY


# ---- the log-strip kernel's branches, counted on a replay of its lane order ----
def _replays(case, shift):
    """[candidate][member] lane_replay of the float64 members, with the restatement's own L beside"""
    p, members, got = lh.expected(case, shift, np.float64)
    out = []
    for x, g in zip(p.points, got):
        row = [lh.member_replay(m, x) for m in members]
        for r, logs in zip(row, g.log_factors):  # (the replay adds the same terms in another order)
            assert abs(r["L"] - float(logs[0])) <= 1e-12 * max(1.0, abs(float(logs[0]))), (case.name, shift, r["L"], float(logs[0]))
        out.append(row)
    return p, members, got, out


def _total(rows, key):
    return sum(r[key] for row in rows for r in row)


def _show(name, shift, rows):
    keys = ("rho_low", "rho_high", "rho_one", "first", "rescales", "below", "won_low", "won_high", "empty", "zero_weights")
    print("%s %s: %s; in later sweeps (rescales, below) %s; largest spread within a lane %.1f, across a merge %.1f" % (
        name, shift, ", ".join("%s %d" % (k, _total(rows, k)) for k in keys),
        tuple(sum(r["later_sweeps"][q] for row in rows for r in row) for q in (0, 1)),
        max(r["lane_spread"] for row in rows for r in row), max(r["merge_spread"] for row in rows for r in row)))


def test_the_full_front_at_shift_zero_keeps_its_rescales():
    p, members, got, rows = _replays(lh.FULL, lh.SHIFTS[0])
    _show(lh.FULL.name, lh.SHIFTS[0], rows)
    for (r,) in rows:
        assert r["rho_low"] + r["rho_high"] == 1025 and r["rho_one"] == 0 and r["first"] == 64
        assert r["rescales"] >= 1 and r["below"] >= 1 and r["rescales"] + r["below"] == 1025 - 64
        assert r["won_low"] + r["won_high"] == 192 and r["empty"] == 0
        assert r["lane_spread"] < 745.0 and r["zero_weights"] == 0  # (this case never underflows a weight: LANES does)


@pytest.mark.parametrize("shift", lh.SHIFTS, ids=["r%g-t%g" % s for s in lh.SHIFTS])
def test_four_sweeps_take_both_branches_and_shift_eight_underflows_weights(shift):
    p, members, got, rows = _replays(lh.LANES, shift)
    _show(lh.LANES.name, shift, rows)
    assert len(p.front) == 200 and lh.LANES.E == 2 and lh.LANES.K == 1
    X = p.gps[0][0].X
    for i, row in enumerate(lh.LANES_ROWS):
        assert float(np.max(np.abs(p.points[i] - X[row]))) == pytest.approx(lh.LANES_OFFSET) and float(p.gps[0][0].noise[0]) == lh.LANES_NOISE
    assert min(len(m.front) for m in members) >= 192  # (four sweeps each)
    for row in rows:
        for r, m in zip(row, members):
            strips = len(m.front) + 1
            assert r["rho_low"] + r["rho_high"] + r["rho_one"] == strips and r["first"] + r["rescales"] + r["below"] == strips - r["rho_one"]
            assert r["won_low"] + r["won_high"] + r["empty"] == 192
            # both branches of record_take in the second or later sweeps: at shift 0 for every member and candidate (under a
            # lowered reference point a member's strips may fall from the first to the last, and none rescales)
            if shift == lh.SHIFTS[0]:
                assert r["later_sweeps"][0] >= 1 and r["later_sweeps"][1] >= 1, (shift, r)
    for q in (0, 1):
        assert sum(r["later_sweeps"][q] for row in rows for r in row) >= 100
    assert _total(rows, "rho_low") >= 1 and _total(rows, "rho_high") >= 1
    assert _total(rows, "won_low") >= 1 and _total(rows, "won_high") >= 1
    if shift == lh.SHIFTS[2]:
        # candidates 0 and 1, a hundredth from sampled points of GPs that observe with noise 1e-6: weights that are exactly 0
        for row in rows[:2]:
            assert max(r["lane_spread"] for r in row) > 745.0 and max(r["merge_spread"] for r in row) > 745.0
            assert sum(r["zero_weights"] for r in row) >= 2


@pytest.mark.parametrize("shift", lh.SHIFTS, ids=["r%g-t%g" % s for s in lh.SHIFTS])
def test_the_rho_one_strip_at_lane_zero_of_the_second_sweep(shift):
    p, members, got, rows = _replays(lh.ULP64, shift)
    _show(lh.ULP64.name, shift, rows)
    assert len(p.front) == 70 and p.front[64, 0] == np.nextafter(p.front[63, 0], np.inf) and all(len(m.front) == 70 for m in members)
    # lambda_1 at two edges a unit in the last place apart comes out equal (rho = 1, the strip is skipped) or one rounding apart
    # (a strip of weight 1e-16 of its neighbours'), as the candidate's mean and deviation fall: the restatement's count in float64,
    # strip 64 and no other, at least once in every shift
    for row, g in zip(rows, got):
        assert g.skipped == sum(r["rho_one"] for r in row) <= 2
        for r in row:
            assert r["skipped_at"] in ([], [64]) and r["first"] == 64
            assert r["rescales"] + r["below"] == 7 - r["rho_one"]  # (strips 64 .. 70; lane 0 holds strip 0 alone where 64 is skipped)
    assert sum(g.skipped for g in got) >= 1


@pytest.mark.parametrize("shift", lh.SHIFTS, ids=["r%g-t%g" % s for s in lh.SHIFTS])
def test_the_rho_one_strip_as_the_last_strip_leaves_the_second_sweep_empty(shift):
    p, members, got, rows = _replays(lh.ULP_LAST, shift)
    _show(lh.ULP_LAST.name, shift, rows)
    assert len(p.front) == 64 and p.front[63, 0] == np.nextafter(p.ref[0], -np.inf) and all(len(m.front) == 64 for m in members)
    for row, g in zip(rows, got):
        assert g.skipped == sum(r["rho_one"] for r in row) <= 2
        for r in row:
            assert r["skipped_at"] in ([], [64]) and r["first"] == 64 and r["rescales"] + r["below"] == 1 - r["rho_one"] and r["empty"] == 0
    assert sum(g.skipped for g in got) >= 1


@pytest.mark.parametrize("kind", lh.STALL_FRONTS)
def test_the_stall_problem_stalls_the_plain_form_and_not_the_log_form(kind):
    p, members = lh.stall(kind, np.float64)
    starts = lh.stall_starts(p.points.shape[1])
    assert starts.shape == (12, 3) and len(p.taus) == 1 and len(p.front) == (0 if kind == "empty" else 2)
    for r in range(2):
        assert p.ref[r] <= float(np.min(p.gps[0][r].y)) - 60.0
    norms = []
    for x in starts:
        plain = ch.evaluate(members, x)
        assert float(plain.value) == 0.0 and not np.any(plain.grad)
        w = lh.evaluate(members, x)
        assert np.isfinite(w.value) and np.all(np.isfinite(w.grad)) and float(np.max(np.abs(w.grad))) > 0.0
        norms.append(float(np.max(np.abs(w.grad))))
    print("stall (%s front): plain value and gradient 0 at all 12 starts; log gradient norms %.3g .. %.3g" % (kind, min(norms), max(norms)))
