"""CPU tests (-m "not gpu") of the three-objective expected hypervolume improvement: tests/ehvi3_reference.py, the restatement
tests/test_gpu_ehvi3.py checks the device against, is itself checked here -- the closed form against the DEFINITION (the mean gain
of hypervolume_3 over seeded normal draws), the empty front against the product of three analytic expected improvements, a front
flat in the third objective against the two-objective strip sum of tests/ehvi_reference.py, float64 against long double, the
gradient against central differences of the long-double value, hypervolume_3 against inclusion-exclusion, every branch of the
believed-front rule, the table's box counts -- and the C ABI's refusals in the header's order, which need no device.  Sections 7 to
10 qualify the cases that reach the limits (the full member of 256 points and 33 153 boxes, random fronts of 192 points, the
believed-front rule past 64 points, 341 members): each reaches the branch it is there for, in float64 and in long double alike, with
1e-3 between the coordinates that decide it."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import ehvi3_reference as h3
import ehvi_reference as hr
import ei1_reference as er
import kg1_reference as kr
from cornell_moe_amd import _lib, build as moe_build, expected_hypervolume_improvement as ehvi

LD = h3.LD
dp, ip = _lib.dp, _lib.ip

CASES = h3.CASES + [h3.BELIEVED] + h3.LIMIT_CASES
# (the gradient's formula does not know E: the 341 members are left to float64 against long double)
FD_CASES = [c for c in CASES if c.E <= 3]


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. the closed form against the definition ----
def _gain_by_volume(front, ref, y):
    """hypervolume_3(front u {y}) - hypervolume_3(front) for draws y [n][3] as a volume: the part of [y, r] inside the
    non-dominated region, box by box of the table"""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 3)
    n = len(f)
    edge = [np.concatenate([[-np.inf], f[:, k], [ref[k]]]) for k in range(3)]
    out = np.zeros(len(y))
    for left, right, height, slab in h3.box_table(f):
        du = np.maximum(edge[0][right] - np.maximum(edge[0][left], y[:, 0]), 0.0)
        dv = np.maximum(edge[1][height] - y[:, 1], 0.0)
        dw = np.maximum(edge[2][slab + 1] - np.maximum(edge[2][slab], y[:, 2]), 0.0)
        out += du * dv * dw
    assert n == 0 or len(h3.box_table(f)) <= (n + 1) * (n + 2) // 2
    return out


# (mu_k, sigma_k) of the three objectives: ahead of the fronts, beside them, and behind them with deviations wide enough that a gain
# is still drawn often
MOMENTS = [((0.1, 0.5), (-0.2, 0.4), (0.0, 0.5)), ((-0.6, 0.3), (0.5, 0.8), (0.3, 0.6)), ((0.5, 0.6), (0.4, 0.7), (0.4, 0.7))]


@pytest.mark.parametrize("F", (0, 1, 20, 160))
def test_the_closed_form_is_the_expected_gain_in_hypervolume(F):
    rng = np.random.default_rng(300 + F)
    ref = h3.REF
    front = h3.random_front(rng, F, 0.1)
    assert len(front) == F
    table = h3.box_table(front)
    hv0 = ehvi.hypervolume_3(front, ref)
    draws = 40000 if F < 100 else 20000
    for mom in MOMENTS:
        y = np.stack([mu + s * rng.normal(size=draws) for mu, s in mom], axis=1)
        gain = _gain_by_volume(front, ref, y)
        # the volume form IS the module's hypervolume difference, draw by draw
        for j in range(100 if F < 100 else 12):
            by_definition = ehvi.hypervolume_3(np.vstack([front, y[j:j + 1]]), ref) - hv0
            assert abs(by_definition - gain[j]) <= 1e-11, (F, j, by_definition, gain[j])
        mean, se = float(np.mean(gain)), float(np.std(gain, ddof=1)) / math.sqrt(len(gain))
        for T in (LD, np.float64):
            closed = float(h3.box_sum([(mu, s * s) for mu, s in mom], front, ref, T, table)[0])
            assert abs(closed - mean) <= 5.0 * se, (F, mom, closed, mean, se)
        print("F = %d (%d boxes), mu %s: closed form %.6f, %d draws %.6f +- %.6f" % (
            F, len(table), [m[0] for m in mom], closed, draws, mean, se))
        assert mean > 10 * se  # (the comparison is not vacuous)


@pytest.mark.parametrize("T", (LD, np.float64), ids=("long_double", "float64"))
def test_with_an_empty_front_a_member_is_the_product_of_three_expected_improvements(T):
    p = h3.make_problem(h3.case("e1_d3_n20_p3_f1"))
    none = p.pending[:0]
    m = h3.Member(p.gps[0], p.ref, np.zeros((0, 3)), none, T)
    bases = [kr.Model(g.cov_type, g.hyper, g.X, g.y, g.noise, T) for g in p.gps[0]]
    for x in p.points:
        a, grad, _ = m.evaluate(x)
        e = [er.evaluate_model(b, b, none, x, r) for b, r in zip(bases, p.ref)]
        assert a == (e[0].value * e[1].value) * e[2].value and a > 0
        product_rule = (e[1].value * e[2].value) * e[0].grad + (e[0].value * e[2].value) * e[1].grad + (e[0].value * e[1].value) * e[2].grad
        assert float(np.max(np.abs(grad - product_rule))) <= 1e-14 * max(1.0, float(np.max(np.abs(grad))))


@pytest.mark.parametrize("T", (LD, np.float64), ids=("long_double", "float64"))
def test_a_front_flat_in_the_third_objective_is_the_two_objective_strip_sum(T):
    """all w_i = w*: psi_3(w*) psi_1(r1) psi_2(r2) + (psi_3(r3) - psi_3(w*)) (the strip sum over the projected front)"""
    p = h3.make_problem(h3.case(h3.FLAT))
    w_star = float(p.front[0, 2])
    assert np.all(p.front[:, 2] == w_star) and len(p.front) == 12
    m = h3.Member(p.gps[0], p.ref, p.front, p.pending, T)
    assert len(m.table) == 91 and len(set(m.table[:, 3])) == 13
    for x in p.points:
        a, _, _ = m.evaluate(x)
        mo = [h3.cr.moments(mm, b, x) for mm, b in zip(m.models, m.bases)]
        p1, p2 = h3.psi(p.ref[0], mo[0][0], mo[0][1], T)[0], h3.psi(p.ref[1], mo[1][0], mo[1][1], T)[0]
        p3_star, p3_r = h3.psi(w_star, mo[2][0], mo[2][1], T)[0], h3.psi(p.ref[2], mo[2][0], mo[2][1], T)[0]
        two = hr.strips(mo[0][0], mo[0][1], mo[1][0], mo[1][1], p.front[:, :2], p.ref[:2], T)[0]
        want = p3_star * p1 * p2 + (p3_r - p3_star) * two
        assert abs(float(a - want)) <= (1e-17 if T is LD else 1e-14) * 100, (float(a), float(want))
        assert float(a) > 1e-3


# ---- 2. float64 against long double; 3. the gradient ----
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_float64_agrees_with_long_double(case):
    p, want = h3.expected(case, LD)
    _, got = h3.expected(case, np.float64)
    worst = 0.0
    for w, g in zip(want, got):
        worst = max(worst, abs(float(g.value - w.value)) / w.scale,
                    float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / w.scale,
                    max(abs(float(a - b)) for a, b in zip(g.members, w.members)) / w.scale)
    print("%s: float64 - long double %.2e scale (recorded %.2e)" % (case.name, worst, case.ld_diff))
    assert worst <= case.ld_diff  # (the case table's figure; the device test's bound is max(1e-10, 4 times it))
    assert 4.0 * case.ld_diff <= 1e-10
    # the cases are not vacuous: the value and the gradient stand far above the device test's bound at most candidates
    big = [i for i, w in enumerate(want) if float(w.value) >= 1e-4 * w.scale and float(np.max(np.abs(w.grad))) >= 1e-3]
    assert len(big) >= 3, (case.name, [float(w.value) for w in want])


@pytest.mark.parametrize("case", FD_CASES, ids=_ids(FD_CASES))
def test_gradient_agrees_with_central_differences(case):
    p, want = h3.expected(case, LD)
    members = h3.ensemble(p, LD)
    h = 1e-6
    worst = 0.0
    for i in p.checked[:2]:
        x = p.points[i]
        for j in range(min(len(x), 4)):
            hi, lo = x.copy(), x.copy()
            hi[j] += h
            lo[j] -= h
            fd = (h3.evaluate(members, hi).value - h3.evaluate(members, lo).value) / LD(hi[j] - lo[j])
            worst = max(worst, abs(float(fd - want[i].grad[j])))
    print("%s: gradient - central differences %.2e" % (case.name, worst))
    assert worst <= 1e-7


@pytest.mark.parametrize("case", [c for c in CASES if c.p and c.F], ids=_ids([c for c in CASES if c.p and c.F]))
def test_the_front_and_the_pending_points_move_the_value(case):
    p, want = h3.expected(case, LD)
    empty = h3.ensemble(p, LD, front=np.zeros((0, 3)))
    bare = h3.ensemble(p, LD, pending=p.pending[:0])
    x, w = p.points[0], want[0]
    assert abs(float(h3.evaluate(empty, x).value - w.value)) >= 1e-3 * w.scale
    assert abs(float(h3.evaluate(bare, x).value - w.value)) >= 1e-6 * w.scale


# ---- 4. hypervolume_3 and pareto_front_3 ----
def _inclusion_exclusion(points, ref):
    total = 0.0
    for m in range(1, len(points) + 1):
        for sub in itertools.combinations(points, m):
            corner = np.max(np.array(sub), axis=0)
            total += (-1.0) ** (m + 1) * float(np.prod(np.maximum(np.asarray(ref) - corner, 0.0)))
    return total


def test_hypervolume_3_against_inclusion_exclusion_on_five_points():
    rng = np.random.default_rng(5)
    ref = (1.0, 1.2, 0.9)
    for trial in range(20):
        pts = rng.uniform(-0.5, 1.1, size=(5, 3))
        if trial % 4 == 0:
            pts[1, 2] = pts[0, 2]  # a tie in the third objective
        if trial % 5 == 0:
            pts[3] = pts[2]  # an equal point
        assert abs(ehvi.hypervolume_3(pts, ref) - _inclusion_exclusion(pts, ref)) <= 1e-13, trial
    assert ehvi.hypervolume_3([], ref) == 0.0 and ehvi.hypervolume_3([(0.0, 0.2, -0.1)], ref) == 1.0
    assert ehvi.hypervolume_3([(1.0, 0.0, 0.0)], ref) == 0.0  # on the boundary: nothing


def test_pareto_front_3_is_canonical_and_keeps_one_of_equal_points():
    pts = [(1.0, 3.0, 0.0), (2.0, 2.0, 0.0), (1.0, 3.0, 0.0), (0.5, 0.5, 1.0), (2.0, 2.0, 0.5), (0.0, 5.0, 0.0), (3.0, 3.0, 3.0)]
    f = ehvi.pareto_front_3(pts)
    assert np.array_equal(f, np.array([(0.0, 5.0, 0.0), (1.0, 3.0, 0.0), (2.0, 2.0, 0.0), (0.5, 0.5, 1.0)]))
    assert np.array_equal(ehvi.pareto_front_3(pts, (1.5, 6.0, 2.0)), np.array([(0.0, 5.0, 0.0), (1.0, 3.0, 0.0), (0.5, 0.5, 1.0)]))
    assert ehvi.pareto_front_3([]).shape == (0, 3) and ehvi.pareto_front_3([(1.0, 1.0, 1.0)], (1.0, 2.0, 2.0)).shape == (0, 3)
    assert np.array_equal(h3.canonical(f), f)


# ---- 5. the believed-front rule ----
def test_every_branch_of_the_believed_front_rule_binds():
    # the rule itself on a hand-made front
    front = [(0.0, 3.0, 0.0), (1.0, 2.0, 0.0), (2.0, 1.0, 1.0), (3.0, 0.0, 1.0), (0.5, 0.5, 2.0)]
    outcomes = [(1.5, 1.5, 0.5),    # joins, nobody leaves, ties nobody
                (5.0, 0.0, 0.0),    # outside r
                (1.0, 2.5, 0.5),    # dominated by (1, 2, 0)
                (0.5, 0.5, 0.5),    # (2, 1, 1), (1.5, 1.5, 0.5) and (0.5, 0.5, 2) are >= it: three leave
                (4.0, -1.0, 1.0),   # joins and ties (3, 0, 1) in w
                (math.nan, 0.0, 0.0), (0.0, 0.0, 4.0)]
    for T in (LD, np.float64):
        f, log = h3.believed_front(front, outcomes, (4.5, 4.0, 4.0), T)
        assert log == [("joined", 0, False), ("outside", 0, False), ("dominated", 0, False), ("joined", 3, False), ("joined", 0, True),
                       ("outside", 0, False), ("outside", 0, False)], log
        want = np.array([(0.0, 3.0, 0.0), (1.0, 2.0, 0.0), (0.5, 0.5, 0.5), (3.0, 0.0, 1.0), (4.0, -1.0, 1.0)])
        assert np.array_equal(np.asarray(f, dtype=np.float64), want)
        assert np.array_equal(h3.canonical(f), f)
    # the device case: each branch under some member, with margins a device's last bits cannot cross
    for T in (LD, np.float64):
        p = h3.make_problem(h3.BELIEVED)
        m0, m1 = h3.ensemble(p, T)
        print("believed-front case: caller's front %d points; logs %s and %s" % (len(p.front), m0.log, m1.log))
        assert m0.log[0][0] == "joined" and m0.log[0][1] >= 2     # several front points leave under member 0
        assert m0.log[1][0] == "dominated"
        assert m0.log[2][0] == "outside" and m1.log[2][0] == "outside"
        assert any(what == "joined" and left == 0 for what, left, _ in m0.log + m1.log)
        assert any(what == "joined" and tie for what, _, tie in m1.log)  # an outcome with w = 0 beside the front point at w = 0
        assert all(float(o[2]) == 0.0 for o in m1.outcomes) and any(float(q[2]) == 0.0 for q in p.front)
        # margins: no believed outcome within 1e-3 of a front point's u or v, nor, but for the exact ties, of its w; nor of r
        for m in (m0, m1):
            for o in m.outcomes:
                for q in p.front:
                    assert min(abs(float(o[0]) - q[0]), abs(float(o[1]) - q[1])) >= 1e-3
                    assert float(o[2]) == q[2] or abs(float(o[2]) - q[2]) >= 1e-3
                assert min(abs(float(o[k]) - p.ref[k]) for k in range(3)) >= 1e-3
            for a, b in itertools.combinations(m.outcomes, 2):
                assert max(abs(float(a[k]) - float(b[k])) for k in range(2)) >= 1e-3


# ---- 6. the table ----
def test_the_tables_box_counts():
    for c in h3.CASES:
        p = h3.make_problem(c)
        assert len(p.front) == c.F and np.array_equal(h3.canonical(p.front), p.front), c.name
        t = h3.box_table(p.front)
        assert len(t) <= (c.F + 1) * (c.F + 2) // 2 and np.all(np.diff(t[:, 3]) >= 0) and t[-1, 3] == c.F  # slab-major
        if c.B is not None:
            assert len(t) == c.B, (c.name, len(t))
        for k in range(c.F + 1):  # inside a slab the strips run in ascending u and tile (-infinity, r1]
            rows = t[t[:, 3] == k]
            assert rows[0, 0] == 0 and rows[-1, 1] == c.F + 1 and np.array_equal(rows[1:, 0], rows[:-1, 1]) and rows[0, 2] == c.F + 1
            assert np.array_equal(rows[1:, 2], rows[1:, 0])
    assert {len(h3.box_table(h3.staircase_front(F))) for F in (9, 10, 21, 22)} == {55, 66, 253, 276}
    assert len(h3.box_table(h3.descending_front(70))) == 141 and len(h3.box_table(h3.staircase_front(192))) == 193 * 194 // 2
    assert len(h3.box_table(h3.staircase_front(256))) == 33153


# ---- 7. the full member ----
def _gap(a, b):
    """the smallest distance between a number of a and one of b"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.min(np.abs(a[:, None] - b[None, :])))


def _own_gap(a):
    return float(np.min(np.diff(np.sort(np.asarray(a, dtype=np.float64).ravel()))))


def _full_member_0(m, front):
    """what decides member 0's log -- every outcome above every front point in u and below it in v, the outcomes' own u and v
    apart -- holds with 1e-3 to spare; w decides the order alone"""
    o = np.array([[float(x) for x in row] for row in m.outcomes])
    assert float(np.min(o[:, 0])) - float(np.max(front[:, 0])) >= 1e-3 and float(np.min(front[:, 1])) - float(np.max(o[:, 1])) >= 1e-3
    assert _own_gap(o[:, 0]) >= 1e-3 and _own_gap(o[:, 1]) >= 1e-3
    assert float(np.max(o)) <= min(h3.REF) - 1e-3
    return o


def test_the_full_member_holds_256_points_and_33153_boxes():
    c = h3.FULL
    p = h3.make_problem(c)
    assert len(p.front) == 192 and np.array_equal(h3.canonical(p.front), p.front) and len(h3.box_table(p.front)) == c.B == 193 * 194 // 2
    assert np.array_equal(ehvi.pareto_front_3(p.front, p.ref), p.front)
    assert not np.array_equal(np.sort(p.pending[:, 0]), p.pending[:, 0]) and np.all(p.pending[:, 1] == 0.5)  # on one line, shuffled
    tables = []
    for T in (np.float64, LD):
        m0, m1 = h3.ensemble(p, T)
        assert m0.log == [("joined", 0, False)] * 64 and len(m0.front) == 256 and len(m0.table) == 33153
        o = _full_member_0(m0, p.front)
        # w orders the points and decides nothing else; the device's means agree with these to 1e-10 scale, far inside the gaps
        w_gap = min(_own_gap(o[:, 2]), _gap(o[:, 2], p.front[:, 2]))
        assert w_gap >= 1e-6
        slabs = np.bincount(m0.table[:, 3], minlength=257)
        assert np.array_equal(slabs, np.arange(257) + 1)  # slab k holds k + 1 strips
        inside = 0
        for k in range(1, 257):
            place = h3.staircase(m0.front, k).index(k - 1)
            inside += 1 if 0 < place < k - 1 else 0
        assert inside >= 32
        assert tuple(m0.table[-1]) == (int(m0.table[-2][1]), 257, int(m0.table[-2][1]), 256)  # strip 256 of slab 256
        # member 1: every outcome lies above EVERY front point in all three objectives by 1e-3 or more: dominated, its front the caller's
        o1 = np.array([[float(x) for x in row] for row in m1.outcomes])
        assert m1.log == [("dominated", 0, False)] * 64 and len(m1.front) == 192 and len(m1.table) == c.B
        assert float(np.min(np.min(o1, axis=0) - np.max(p.front, axis=0))) >= 1e-3 and float(np.max(o1)) <= min(h3.REF) - 1e-3
        print("full member, %s: outcomes' smallest gaps %.2e in u, %.2e in v, %.2e in w (order only); %d of 256 slabs insert their "
              "point inside the staircase" % (T.__name__, _own_gap(o[:, 0]), _own_gap(o[:, 1]), w_gap, inside))
        tables.append(m0.table)
    assert np.array_equal(tables[0], tables[1])  # the same order in both arithmetics
    # sensitivity: the table's last box, and its last sweep of 129, each carry at least 100 times the device test's bound
    p, want = h3.expected(c, LD)
    m0 = h3.ensemble(p, LD)[0]
    bound = max(1e-10, 4.0 * c.ld_diff)
    factors = []
    for x in p.points:
        mo = [h3.cr.moments(mm, b, x) for mm, b in zip(m0.models, m0.bases)]
        mom = [(q[0], q[1]) for q in mo]
        whole = h3.box_sum(mom, m0.front, m0.ref, LD, m0.table)[0]
        for cut in (33152, 33024):
            part = h3.box_sum(mom, m0.front, m0.ref, LD, m0.table[:cut])[0]
            factors.append(abs(float(whole - part)) / (bound * m0.scale))
    print("full member: dropping the last box / the last sweep moves member 0's value by %s times the bound" % (
        ["%.3g" % f for f in factors]))
    assert min(factors) >= 100.0


def test_the_full_front_is_reached_through_a_pick_too():
    """the first 63 pending points fed, the value-only batch's first pick on the pending line: whichever start is picked, its outcome
    joins member 0's front as the 256th point, with u and v 1e-3 or more from every other outcome's"""
    p = h3.make_problem(h3.FULL)
    starts = h3.full_starts(p.pending)
    assert np.all(starts[:, 1] == 0.5) and _gap(starts[:, 0], p.pending[:63, 0]) >= 4e-3
    for T in (np.float64, LD):
        for s in starts:
            m0, m1 = h3.ensemble(p, T, pending=np.vstack([p.pending[:63], s[None, :]]))
            assert m0.log == [("joined", 0, False)] * 64 and len(m0.front) == 256 and len(m0.table) == 33153
            _full_member_0(m0, p.front)
            assert m1.log == [("dominated", 0, False)] * 64 and len(m1.front) == 192
            o1 = np.array([float(x) for x in m1.outcomes[63]])
            assert float(np.min(o1 - np.max(p.front, axis=0))) >= 1e-3 and float(np.max(o1)) <= min(h3.REF) - 1e-3


# ---- 8. random fronts of 192 points ----
RANDOM_192 = [c for c in h3.CASES if c.F == 192]


@pytest.mark.parametrize("case", RANDOM_192, ids=_ids(RANDOM_192))
def test_a_random_front_of_192_evicts_staircase_points_past_one_wavefront(case):
    p = h3.make_problem(case)
    f = p.front
    assert len(RANDOM_192) == 2 and len(f) == 192 and len(h3.box_table(f)) == case.B
    evicting, several, high, identity = 0, 0, 0, 0
    before = h3.staircase(f, 64)
    for k in range(65, 193):
        after = h3.staircase(f, k)
        gone = [i for i in before if i not in after]
        evicting += 1 if gone else 0
        several += 1 if len(gone) >= 2 else 0
        high += sum(1 for i in gone if i >= 64)
        identity += 1 if after == sorted(after) else 0
        before = after
    print("%s: %d boxes; of the slabs past 64, %d evict a staircase point, %d evict two or more, %d evictions of a survivor with index "
          ">= 64; %d of them in ascending index order" % (case.name, case.B, evicting, several, high, identity))
    assert evicting >= 10 and several >= 1 and high >= 1
    assert 128 - identity >= 100  # (the u order is not the w order: the ordering step rearranges in nearly every slab past 64)


# ---- 9. the believed-front rule past 64 points ----
def test_the_believed_front_rule_binds_past_64_points():
    c = h3.BELIEVED_WIDE
    p = h3.make_problem(c)
    assert len(p.front) == 192 and np.array_equal(ehvi.pareto_front_3(p.front, p.ref), p.front) and len(h3.box_table(p.front)) == c.B
    assert int(np.sum(p.front[:, 2] < 0.0)) >= 64 and int(np.sum(p.front[:, 2] == 0.0)) == 1
    seen = []
    for T in (np.float64, LD):
        m0, m1 = h3.ensemble(p, T)
        d0, d1 = m0.detail, m1.detail
        role = dict(zip(h3.ROLES, range(6)))
        ranges = lambda d: sorted(set(i // 64 for i in d["left"]))  # noqa: E731
        print("believed-front case past 64 points, %s: member 0 %s, places %s, the ranges that lose points %s; member 1 %s, places %s" % (
            T.__name__, m0.log, [d["place"] for d in d0], [ranges(d) for d in d0], m1.log, [d["place"] for d in d1]))
        # a join at place 0 with the smallest w of all
        j = role["first"]
        assert m0.log[j][0] == "joined" and d0[j]["place"] == 0 and float(m0.outcomes[j][2]) < float(np.min(p.front[:, 2])) - 1e-3
        # a join that evicts nobody, in the middle
        j = role["middle"]
        assert m0.log[j] == ("joined", 0, False) and 64 <= d0[j]["place"] < d0[j]["n"] - 64
        # a join at a place >= 64 whose evictions lie in three of the four index ranges (the lower one cannot lose a point then)
        j = role["sweep"]
        assert m0.log[j][0] == "joined" and d0[j]["place"] >= 64 and d0[j]["n"] >= 193 and ranges(d0[j]) == [1, 2, 3]
        # an outcome dominated only by front points with index >= 128
        j = role["behind"]
        assert m0.log[j][0] == "dominated" and min(d0[j]["dominators"]) >= 128
        # a join at the last place with the largest w
        j = role["last"]
        assert m0.log[j][0] == "joined" and d0[j]["place"] == d0[j]["n"] - m0.log[j][1] == len(m0.front) - 1
        assert float(m0.outcomes[j][2]) > float(np.max(p.front[:, 2])) + 1e-3
        # member 1: w = 0 exactly; an outcome joins beside the kept front point at w = 0, which has index >= 64
        assert all(float(o[2]) == 0.0 for o in m1.outcomes)
        ties = [(log, d) for log, d in zip(m1.log, d1) if log[0] == "joined" and log[2]]
        assert ties and all(d["place"] >= 64 for _, d in ties)
        zero = int(np.flatnonzero(np.asarray(m1.front[:, 2], dtype=np.float64) == 0.0)[0])
        assert zero >= 64 and np.array_equal(np.asarray(m1.front[zero], dtype=np.float64), p.front[p.front[:, 2] == 0.0][0])
        # margins: 1e-3 between an outcome and every caller's point, the reference point and every other outcome of its member, in
        # each objective; the exact ties in w made on purpose excepted
        for m in (m0, m1):
            o = np.array([[float(x) for x in row] for row in m.outcomes])
            for k in range(3):
                exact = k == 2 and m is m1
                assert exact or (_gap(o[:, k], p.front[:, k]) >= 1e-3 and _own_gap(o[:, k]) >= 1e-3), (k, _gap(o[:, k], p.front[:, k]))
                assert p.ref[k] - float(np.max(o[:, k])) >= 1e-3
            if m is m1:
                others = p.front[p.front[:, 2] != 0.0]
                assert np.all(o[:, 2] == 0.0) and float(np.min(np.abs(others[:, 2]))) >= 1e-3
        seen.append((m0.log, m1.log, [d["place"] for d in d0 + d1], [d["left"] for d in d0 + d1]))
    assert seen[0] == seen[1]  # float64 and long double take the same branches


# ---- 10. 341 members ----
def test_no_two_of_the_341_members_agree():
    p, want = h3.expected(h3.MANY, LD)
    assert len(p.gps) == 341 and sum(len(row) for row in p.gps) == 1023 and len(p.front) == 2 and len(p.pending) == 1
    for w in want:
        vals = [float(a) for a in w.members]
        assert len(set(vals)) == 341 and _own_gap(vals) >= 1e-8 * w.scale and min(vals) > 1e-3
    logs = [[m.log for m in h3.ensemble(p, T)] for T in (np.float64, LD)]
    print("341 members: the believed outcome is %s" % sorted(set(log[0][0] for log in logs[1])))
    assert logs[0] == logs[1]  # every member takes the same branch in both arithmetics


# ---- 11. the C ABI without a device ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


NEW = ("moe_ehvi3_mcmc", "moe_ehvi3_mcmc_multistart", "moe_ehvi3_mcmc_suggest")


def test_the_new_symbols_are_exported(lib):
    from cornell_moe_amd import api
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("ehvi3_ensemble", "ehvi3_multistart", "ehvi3_suggest"):
        assert callable(getattr(api, name))
    for name in ("ExpectedHypervolumeImprovement3MCMC", "multistart_expected_hypervolume_improvement_3_optimization", "pareto_front_3",
                 "hypervolume_3"):
        assert callable(getattr(ehvi, name))


def _args(d=2, E=1, F=2, C_=3, p=0, q=1, steps=3, domain=0):
    """valid arguments that need no handle: the arrays of handles hold NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    front = np.array([(0.1 * i, 1.0 - 0.1 * i, 0.01 * i) for i in range(max(F, 1))], dtype=np.float64)
    hs = [(C.c_void_p * max(E, 1))() for _ in range(3)]
    return dict(gps=hs[0], gps2=hs[1], gps3=hs[2], E=E, ref=np.array([200.0, 2.0, 5.0]), front=front, F=F,
                pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25), C=C_,
                out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ehvi3_mcmc(g("gps", a["gps"]), g("gps2", a["gps2"]), g("gps3", a["gps3"]), a["E"], g("ref", _p(a["ref"])),
                              g("front", _p(a["front"])), a["F"], g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], 1,
                              g("ei", _p(a["out"])), g("grad", _p(a["out"])), None, C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ehvi3_mcmc_multistart(
        g("gps", a["gps"]), g("gps2", a["gps2"]), g("gps3", a["gps3"]), a["E"], g("ref", _p(a["ref"])), g("front", _p(a["front"])),
        a["F"], g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])),
        a["C"], ascent, g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None,
        None, None, None, C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ehvi3_mcmc_suggest(
        g("gps", a["gps"]), g("gps2", a["gps2"]), g("gps3", a["gps3"]), a["E"], g("ref", _p(a["ref"])), g("front", _p(a["front"])),
        a["F"], g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])),
        a["C"], ascent, a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])), g("found", a["iout"].ctypes.data_as(ip)),
        C.byref(err))


def _payload(err):
    return tuple(err.payload)


def refusals_in_order(lib):
    """the header's order of errors, argument by argument, on the three entry points (tests/test_gpu_ehvi3.py runs it too)"""
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    for call in (_eval, _ascent, _suggest):
        # num_mcmc first, even with everything else wrong: three GPs per member, 341 members
        for E in (0, 342):
            a = _args(C_=0, p=65, F=193)
            a["E"] = E
            assert call(lib, a, err, gps=True, pts=True) == B and _payload(err) == (float(E), 1.0, 341.0), call.__name__
        # then NULL arrays, before the front's own checks and the counts
        for name in ("gps", "gps2", "gps3", "ref", "pts", "front"):
            assert call(lib, _args(C_=0, p=65), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        a = _args(C_=0, p=65, F=193)
        a["ref"][0] = math.nan
        # then num_front outside 0 .. 192
        for F in (-1, 193):
            a["F"] = F
            assert call(lib, a, err) == B and _payload(err) == (float(F), 0.0, 192.0), call.__name__
        # then a reference point that is not finite
        for r, bad in ((0, math.nan), (1, math.inf), (2, -math.inf)):
            a = _args(C_=0, p=65)
            a["ref"][r] = bad
            a["front"][1, 0] = math.nan
            assert call(lib, a, err) == V and b"reference_point" in err.message and _payload(err)[1:] == (float(r), 0.0), call.__name__
        # then the front (0, 1, 0), (0.1, 0.9, 0.01), (0.2, 0.8, 0.02), (0.3, 0.7, 0.03): not finite, on or outside the reference
        # point, out of the canonical order (w descends; w ties and u descends; w and u tie and v descends), equal to its
        # predecessor, dominated by its predecessor or by a point further back -- payload: the offending index
        for i, point in ((1, (math.nan, 0.5, 0.01)), (2, (0.2, 0.8, math.inf)), (3, (200.0, 0.1, 0.03)), (0, (0.0, 2.0, 0.0)),
                         (0, (0.0, 1.0, 5.0)), (2, (0.2, 0.8, 0.005)), (2, (0.05, 0.95, 0.01)), (2, (0.1, 0.85, 0.01)),
                         (2, (0.1, 0.9, 0.01)), (3, (0.25, 0.85, 0.03)), (3, (0.2, 0.8, 0.03)), (3, (0.15, 0.95, 0.03)),
                         (2, (0.1, 0.95, 0.01))):
            a = _args(C_=0, p=65, F=4)
            a["front"][i] = point
            assert call(lib, a, err) == V and b"front" in err.message and _payload(err) == (float(i), 0.0, 0.0), (call.__name__, i, point)
        # a tie in w alone is in order
        a = _args(p=2, F=4)
        a["front"][2] = (0.2, 0.8, 0.01)
        assert call(lib, a, err) == R and b"NULL GP handle" in err.message
        # then num_points, before num_being_sampled; an empty front needs no array
        assert call(lib, _args(C_=0, p=65), err) == B and _payload(err)[:2] == (0.0, 1.0)
        assert call(lib, _args(C_=0, p=65, F=0), err, front=True) == B and _payload(err)[:2] == (0.0, 1.0)
        # then num_being_sampled outside 0 .. 64
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        # then points_being_sampled NULL with num_being_sampled > 0
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        # everything that needs no handle in order: the NULL handle is next
        for F in (0, 2, 192):
            assert call(lib, _args(p=2, F=F), err) == R and b"NULL GP handle" in err.message, (call.__name__, F)
        assert call(lib, _args(p=0, F=0), err, pend=True, front=True) == R and b"NULL GP handle" in err.message
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0, F=193), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # max_num_steps < 1 after the pending checks and before the domain type; not asked for without the ascent
        assert call(lib, _args(steps=0, domain=1, p=65), err) == B and _payload(err) == (65.0, 0.0, 64.0)
        assert call(lib, _args(steps=0, domain=1), err) == B and _payload(err)[:2] == (0.0, 1.0) and b"max_num_steps" in err.message
        assert call(lib, _args(steps=0, domain=1), err, ascent=0) == V and b"tensor-product" in err.message
        assert call(lib, _args(domain=1), err) == V and _payload(err)[0] == 1.0 and b"expected hypervolume improvement" in err.message
    # the batch: num_to_sample directly after num_being_sampled, before the NULL pending array, the steps and the domain
    for p, q, hi in ((0, 0, 65.0), (0, 66, 65.0), (3, 63, 62.0), (64, 2, 1.0)):
        assert _suggest(lib, _args(p=p, q=q, steps=0, domain=1), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
    assert _suggest(lib, _args(p=65, q=0), err) == B and _payload(err) == (65.0, 0.0, 64.0)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    refusals_in_order(lib)
