"""CPU tests (-m "not gpu") of the log expected improvement per unit cost: tests/eipc_reference.py, the restatement
tests/test_gpu_eipc.py checks the device against, is itself checked here and its inputs are QUALIFIED before the GPU sees them --
float64 against long double on every case, shift and exponent of eipc_reference.RUNS, the analytic gradient against central
differences, exponent 0 against tests/logcei1_reference.py exactly, one member against the left-to-right sum of its log factors,
the pending points moving a value in every case that has some, and the two-basin problem's condition with its margin.  A case that
breaks a condition fails; none is skipped."""
import numpy as np
import pytest

import eipc_reference as pr
import logcei1_reference as lr
import ms_restatement as ms

LD = pr.LD


@pytest.mark.parametrize("case,shift,alpha", pr.RUNS, ids=pr.RUN_IDS)
def test_float64_agrees_with_long_double(case, shift, alpha):
    """relative to max(1, |long double|): value, gradient (infinity norm) and every log factor within the project's 2.5e-11"""
    p, want = pr.expected(case, shift, alpha, LD)
    _, got = pr.expected(case, shift, alpha, np.float64)
    worst_v = worst_g = worst_f = 0.0
    for w, g in zip(want, got):
        assert np.isfinite(float(g.value)) and np.all(np.isfinite(g.grad.astype(np.float64)))
        assert len(w.log_factors) == case.E and all(len(row) == 1 + case.K for row in w.log_factors)  # (the case's K is K + 1)
        worst_v = max(worst_v, abs(float(g.value - w.value)) / max(1.0, abs(float(w.value))))
        worst_g = max(worst_g, float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / max(1.0, float(np.max(np.abs(w.grad)))))
        worst_f = max(worst_f, max(abs(float(a - b)) / max(1.0, abs(float(b)))
                                   for ra, rb in zip(g.log_factors, w.log_factors) for a, b in zip(ra, rb)))
    print("%s %s alpha %g: float64 - long double, value %.2e grad %.2e log factors %.2e (relative)"
          % (case.name, shift, alpha, worst_v, worst_g, worst_f))
    assert worst_v <= 2.5e-11 and worst_g <= 2.5e-11 and worst_f <= 2.5e-11


@pytest.mark.parametrize("case,shift,alpha", [(pr.ENSEMBLE, pr.DEEPEST, 1.0), (pr.SECOND, lr.SHIFTS[0], 2.0), (pr.DERIV, lr.SHIFTS[0], 0.5)],
                         ids=["ensemble-deepest", "second-a2", "deriv-a0.5"])
def test_gradient_agrees_with_central_differences(case, shift, alpha):
    """long double, relative to the gradient's size"""
    p, members = pr.shifted(case, shift, alpha, LD)
    h, worst = 1e-6, 0.0
    for x in p.points[:2]:
        want = pr.evaluate(members, x)
        for j in range(len(x)):
            hi, lo = x.copy(), x.copy()
            hi[j] += h
            lo[j] -= h
            fd = (pr.evaluate(members, hi).value - pr.evaluate(members, lo).value) / LD(hi[j] - lo[j])
            worst = max(worst, abs(float(fd - want.grad[j])) / max(1.0, float(np.max(np.abs(want.grad)))))
    print("%s alpha %g: gradient - central differences %.2e (relative)" % (case.name, alpha, worst))
    assert worst <= 1e-6


@pytest.mark.parametrize("case", [pr.SECOND, pr.ENSEMBLE, pr.INF, pr.SMALLEST], ids=lambda c: c.name)
def test_exponent_zero_is_the_log_constrained_expected_improvement_exactly(case):
    for T in (LD, np.float64):
        p, members = pr.shifted(case, lr.SHIFTS[0], 0.0, T)
        plain = [m.inner for m in members]
        for x in p.points:
            got, want = pr.evaluate(members, x), lr.evaluate(plain, x)
            assert got.value == want.value and np.array_equal(got.grad, want.grad)
            for row, wrow in zip(got.log_factors, want.log_factors):
                assert row[:-1] == wrow and row[-1] == 0
            assert got.bprime == want.bprime
    # and another exponent is another value
    _, one = pr.shifted(case, lr.SHIFTS[0], 1.0, LD)
    assert all(abs(float(pr.evaluate(one, x).value - lr.evaluate([m.inner for m in one], x).value)) > 1e-3 for x in p.points)


@pytest.mark.parametrize("case", [pr.SMALLEST, pr.SECOND, pr.K8], ids=lambda c: c.name)
def test_one_member_is_the_left_to_right_sum_of_its_log_factors(case):
    for T in (LD, np.float64):
        p, members = pr.shifted(case, lr.SHIFTS[0], 1.0, T)
        for x in p.points:
            got = pr.evaluate(members, x)
            total = got.log_factors[0][0]
            for f in got.log_factors[0][1:]:
                total = total + f
            assert got.value == total


@pytest.mark.parametrize("case", [c for c in pr.CASES if c.p], ids=lambda c: c.name)
def test_the_pending_points_move_the_value(case):
    p0 = pr.make_problem(case)
    bare = pr.ensemble(p0, 1.0, LD, pending=p0.pending[:0])
    for shift in sorted({s for c, s, a in pr.RUNS if c is case}):
        p, want = pr.expected(case, shift, 1.0, LD)
        without = pr.relimited(bare, p.best, p.thresholds)
        moved = max(abs(float(pr.evaluate(without, x).value - w.value)) for x, w in zip(p.points, want))
        cost_moved = max(abs(float(a.logs(x)[0][-1] - w.log_factors[e][-1])) for x, w in zip(p.points, want) for e, a in enumerate(without))
        print("%s %s: the pending points move a value by %.3g, a cost term by %.3g" % (case.name, shift, moved, cost_moved))
        assert moved >= 1e-5, (case.name, shift)


def test_the_cost_gp_takes_no_part_in_the_incumbent():
    """the believed-feasible incumbent is the one of the objective and constraint GPs alone, whatever the cost GP believes"""
    p, members = pr.members_of(pr.INF, LD)
    assert np.isinf(float(members[0].bprime)) and np.isfinite(float(members[1].bprime))
    assert float(members[1].bprime) <= p.best[1]


def test_the_two_basin_problem_has_its_margin():
    """at alpha = 1 the restatement's own best start lies in the cheap half, its value exceeds its mirror image's by a difference of
    the order 2 (1 - 2 x0), half of which is the margin of tests/test_gpu_eipc.py; the restatement's ascent (float64, the
    host-driven loop the device is compared with) ends in the cheap half with that margin; at alpha = 0 the mirror images agree"""
    tb = pr.two_basin()
    margin, s, diff = pr.two_basin_margin()
    x0 = tb.starts[s][0]
    rough = 2.0 * (1.0 - 2.0 * x0)
    print("two basins: best start %d at x0 = %.4f, value - mirrored value = %.6g (2 (1 - 2 x0) = %.4g), margin %.6g" % (s, x0, diff, rough, margin))
    assert x0 < 0.5 and 0.5 * rough <= diff <= 2.0 * rough and margin == 0.5 * diff
    one, zero = pr.ensemble(tb.problem, 1.0, np.float64), pr.ensemble(tb.problem, 0.0, LD)
    point, value, found = ms.multistart_best(lambda X: np.array([float(pr.evaluate(one, x).value) for x in X]),
                                             lambda X: np.array([pr.evaluate(one, x).grad for x in X], dtype=np.float64),
                                             tb.gd, tb.bounds, tb.starts)
    long_one = pr.ensemble(tb.problem, 1.0, LD)
    gap = float(pr.evaluate(long_one, point).value - pr.evaluate(long_one, pr.mirrored(point)).value)
    print("two basins: the ascent ends at %s, value %.9g, value - mirrored value = %.6g" % (point, value, gap))
    assert found and point[0] < 0.5 and gap >= margin
    for x in list(tb.starts) + [point]:
        a, b = pr.evaluate(zero, x).value, pr.evaluate(zero, pr.mirrored(x)).value
        assert abs(float(a - b)) <= 1e-10 * max(1.0, abs(float(a)))
