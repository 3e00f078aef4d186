"""CPU tests (-m "not gpu") of the constrained expected hypervolume improvement: tests/cehvi_reference.py, the restatement
tests/test_gpu_cehvi.py checks the device against, is itself checked here -- without constraints against tests/ehvi_reference.py and
tests/ehvi3_reference.py term for term, float64 against long double (the measured ld_diff is the case table's), the gradient against
central differences of the long-double value -- and every case is QUALIFIED: at its checked candidates, at least 7 of its 8, the value
and the gradient are far above the device test's tolerance, and dropping the constraints, emptying the front or dropping the pending
points each moves the value by far more than that tolerance, so that a device which returned zeros, ignored the constraints, ignored
the front or ignored P could not pass.  A case that breaks a condition fails; none is skipped.  Then the believed-feasible front rule
with its margins, and feasible_pareto_front on hand-computed inputs.  The edge constructions are qualified in their own terms: E = 2
with K >= 2 against every exchange of cehvi_reference.swapped (10^-6 scale) with the factors told apart, the constraint floors,
the 1024-GP limit case, the changing-belief problem and the two mixed-mask problems of 64 pending points."""
import numpy as np
import pytest

import cehvi_reference as ch
import cei1_reference as cr
import ehvi3_reference as h3
import ei1_reference as er
import ehvi_reference as hr
from cornell_moe_amd import expected_hypervolume_improvement_constrained as cehvi

LD = ch.LD
CASES = ch.ALL_CASES


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. without constraints it is the unconstrained restatement ----
@pytest.mark.parametrize("name", ("m2_e1_k2_d3_n20_p3_f65", "m3_e1_k2_d3_n20_p3_f20"))
def test_without_constraints_it_is_the_unconstrained_restatement(name):
    p = ch.make_problem(ch.case(name))
    bare = ch.ensemble(p, LD, constraints=False)
    mod = hr if p.M == 2 else h3
    twin = [mod.Member(g[:p.M], p.ref, p.front, p.pending, LD) for g in p.gps]
    for x in p.points[:3]:
        a, b = ch.evaluate(bare, x), mod.evaluate(twin, x)
        assert a.value == b.value and [f[0] for f in a.factors] == list(b.members)
        # (the same terms added from 0 and multiplied by 1: a rounding or two of the long double's 1.1e-19)
        assert float(np.max(np.abs(a.grad - b.grad))) <= 1e-17 * max(1.0, float(np.max(np.abs(b.grad))))


# ---- 2. float64 against long double; 3. the gradient ----
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_float64_agrees_with_long_double(case):
    p, want = ch.expected(case, LD)
    _, got = ch.expected(case, np.float64)
    worst = 0.0
    for w, g in zip(want, got):
        worst = max(worst, abs(float(g.value - w.value)) / w.scale,
                    float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / w.scale,
                    max(abs(float(a - b)) for a, b in zip(g.members, w.members)) / w.scale,
                    max(abs(float(a - b)) for fa, fb in zip(g.factors, w.factors) for a, b in zip(fa, fb)) / w.scale)
    print("%s: float64 - long double %.2e scale (recorded %.2e)" % (case.name, worst, case.ld_diff))
    assert worst <= case.ld_diff  # (the case table's figure; the device test's bound is max(1e-10, 4 times it))
    assert 4.0 * case.ld_diff <= 1e-10
    for m64, mld in zip(ch.ensemble(p, np.float64), ch.ensemble(p, LD)):  # (the same beliefs and joins in both arithmetics)
        assert np.array_equal(m64.mask, mld.mask) and [e[0] for e in m64.log] == [e[0] for e in mld.log]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_gradient_agrees_with_central_differences(case):
    p, want = ch.expected(case, LD)
    members = ch.ensemble(p, LD)
    h = 1e-6
    worst = 0.0
    for i in p.checked[:2]:
        x = p.points[i]
        for j in range(min(len(x), 3)):
            hi, lo = x.copy(), x.copy()
            hi[j] += h
            lo[j] -= h
            fd = (ch.evaluate(members, hi).value - ch.evaluate(members, lo).value) / LD(hi[j] - lo[j])
            worst = max(worst, abs(float(fd - want[i].grad[j])))
    print("%s: gradient - central differences %.2e" % (case.name, worst))
    assert worst <= 1e-7


# ---- 4. every case qualified ----
def qualified(case):
    """the candidates of a case at which the conditions hold"""
    p, want = ch.expected(case, LD)
    free = ch.ensemble(p, LD, constraints=False)
    empty = ch.ensemble(p, LD, front=np.zeros((0, p.M)))
    bare = ch.ensemble(p, LD, pending=p.pending[:0])
    ok = []
    for i, (w, x) in enumerate(zip(want, p.points)):
        good = float(w.value) >= 1e-3 * w.scale and float(np.max(np.abs(w.grad))) >= 1e-2
        good = good and abs(float(ch.evaluate(free, x).value - w.value)) >= 1e-3 * w.scale
        if len(p.front):
            good = good and abs(float(ch.evaluate(empty, x).value - w.value)) >= 1e-3 * w.scale
        if len(p.pending):
            good = good and abs(float(ch.evaluate(bare, x).value - w.value)) >= 1e-5 * w.scale
        if good:
            ok.append(i)
    return tuple(ok)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_every_case_is_qualified(case):
    p, want = ch.expected(case, LD)
    assert case.C == 8 and len(p.front) == case.F and len(p.pending) == case.p == 3 and len(p.gps[0]) == case.M + case.K
    ok = qualified(case)
    print("%s: qualified candidates %s" % (case.name, ok))
    assert set(p.checked) <= set(ok), (case.name, ok)
    assert len(p.checked) >= 7
    # every feasibility factor is a probability strictly inside (0, 1) somewhere: none saturates over the whole case
    for k in range(1, case.K + 1):
        assert any(1e-3 < float(w.factors[e][k]) < 1.0 - 1e-3 for w in want for e in range(case.E)), (case.name, k)


def test_the_ensembles_shuffle_their_rows_over_objective_and_constraint_roles():
    for name in (ch.ENSEMBLE2, ch.ENSEMBLE3):
        c = ch.case(name)
        assert c.E == 3 and all(set(row) == {20, 130, 300} for row in c.n)
        for r in range(c.M + c.K):
            assert len({row[r] for row in c.n}) == 3, (name, r)  # (every role sees all three sizes)
    assert any(c.d == 10 for c in ch.CASES)
    assert {(c.M, c.K, c.F) for c in ch.CASES if c.E == 1 and c.d == 3} == (
        {(2, K, F) for K in (1, 2, 8) for F in (0, 2, 65)} | {(3, K, F) for K in (1, 2, 8) for F in (0, 2, 20)})


# ---- 4b. E >= 2 with K >= 2: no [e][k] order but the documented one gives the value ----
MIXED_CASES = [ch.MIXED2, ch.MIXED3, ch.MIXED2_K8]


@pytest.mark.parametrize("case", MIXED_CASES, ids=_ids(MIXED_CASES))
def test_members_and_constraints_together_are_told_apart(case):
    p, want = ch.expected(case, LD)
    assert case.E == 2 and case.K >= 2 and len(set(case.tau)) == case.K and case in ch.EDGE_CASES
    if case.K == 2:
        assert case.d == 13 and case.p == 3 and case.F == (10 if case.M == 2 else 20)
        for r in range(case.M + case.K):
            assert case.n[0][r] != case.n[1][r]                        # (the rows differ per member in every role ...
        assert len(set(case.n[0])) >= 3 and len(set(case.n[1])) >= 3   #  ... and per role within a member)
    got = {i: ch.evaluate(ch.ensemble(p, np.float64), p.points[i]) for i in p.checked}
    worst = {}
    for what, q in ch.swapped(p):
        members = ch.ensemble(q, np.float64)  # (a move of 1e-6 scale needs no long double)
        moved = min(abs(float(ch.evaluate(members, p.points[i]).value - got[i].value)) / want[i].scale for i in p.checked)
        worst[what] = moved
        assert moved >= ch.SWAP_MOVES, (case.name, what, moved)
    assert len(worst) == (4 * case.K if case.K > 2 else 5)
    # the factors F_{e,k} [checked][E][K]: the two members' factors of one constraint lie FACTORS_APART apart at every checked
    # candidate; so does every pair of the E K entries where there are four of them, and where there are sixteen (120 pairs in
    # [0, 1]) every pair does at all checked candidates but at most one -- an entry of factors_out read from another (e, k) fails
    # the device test's entry-by-entry comparison either way
    fac = np.array([[[float(f) for f in row[1:]] for row in want[i].factors] for i in p.checked])
    members_apart = float(np.min(np.abs(fac[:, 0] - fac[:, 1])))
    flat = fac.reshape(len(p.checked), -1)
    close = max(int(np.sum(np.abs(flat[:, a] - flat[:, b]) < ch.FACTORS_APART)) for a in range(flat.shape[1]) for b in range(a))
    print("%s: the exchange that moves the value least, %s, moves it by %.3g scale at its weakest checked candidate; the members' "
          "feasibility factors lie at least %.3g apart; no two factors lie within %.3g of each other at more than %d checked "
          "candidates" % (case.name, min(worst, key=worst.get), min(worst.values()), members_apart, ch.FACTORS_APART, close))
    assert members_apart >= ch.FACTORS_APART
    assert close <= (0 if case.K == 2 else 1)


# ---- 4c. the constraint roles' floors ----
@pytest.mark.parametrize("M", (2, 3))
def test_the_floor_candidates_lie_under_the_constraint_floors(M):
    case = ch.FLOOR[M]
    p = ch.make_problem(case)
    con = p.gps[0][M]
    assert case.E == 1 and case.K == 2 and float(con.noise[0]) == 0.0 and float(p.gps[0][M + 1].noise[0]) > 0.0
    for T in (LD, np.float64):
        m = ch.ensemble(p, T)[0]
        for i, (row, side) in enumerate(zip(ch.FLOOR_ROWS[M], (-1.0, 1.0))):
            assert np.array_equal(p.points[i], con.X[row]) and float(con.y[row, 0]) == case.tau[0] + side * ch.FLOOR_GAP
            mu, var = cr.moments(m.models[M], m.bases[M], p.points[i])[:2]
            print("M = %d, %s: candidate %d, constraint 1: variance %.3g, mean - observation %.3g" % (
                M, T.__name__, i, float(var), float(mu) - float(con.y[row, 0])))
            # (under the gradient's floor in float64, the device's arithmetic; long double's own rounding of alpha - k'K^-1 k
            # leaves 1e-19, a deviation of 3e-10 under a mean 0.2 from tau: F and its gradient saturate in both)
            assert float(var) < (er.MIN_VAR_GRAD_EI if T is np.float64 else 1e-16) and abs(float(mu) - float(con.y[row, 0])) <= 1e-9
            a, g, f, _ = m.evaluate(p.points[i])
            assert float(f[1]) == (1.0 if side < 0 else 0.0) and 1e-3 < float(f[2]) < 1.0 - 1e-3 and float(f[0]) > 1e-3
            if side > 0:
                assert float(a) == 0.0 and not np.any(g)
        assert min(float(cr.moments(m.models[M], m.bases[M], x)[1]) for x in p.points[2:]) > 1e-6
    assert er.MIN_VAR_GRAD_EI == 150.0 * np.finfo(np.float64).eps ** 2


# ---- 4d. E (M + K) = 1024 ----
def test_the_limit_case_has_1024_gps_and_no_two_members_agree():
    c = ch.LIMIT
    p, want = ch.expected(c, LD)
    _, got = ch.expected(c, np.float64)
    assert c.E * (c.M + c.K) == 1024 and sum(len(row) for row in p.gps) == 1024 and len(set(c.tau)) == 6 and c.C == 4
    worst = 0.0
    for w, g in zip(want, got):
        worst = max(worst, abs(float(g.value - w.value)) / w.scale, float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / w.scale,
                    max(abs(float(a - b)) for fa, fb in zip(g.factors, w.factors) for a, b in zip(fa, fb)) / w.scale)
        vals = [float(a) for a in w.members]
        assert len(set(vals)) == c.E and min(vals) > 1e-8 and float(w.value) > 1e-4 and float(np.max(np.abs(w.grad))) > 1e-3
    for k in range(1, c.K + 1):  # (among the members the device test names every constraint's factor is a probability somewhere)
        assert any(1e-3 < float(w.factors[e][k]) < 1.0 - 1e-3 for w in want for e in ch.LIMIT_MEMBERS), k
    print("%s: float64 - long double %.2e scale (recorded %.2e); values %s" % (c.name, worst, c.ld_diff, [float(w.value) for w in want]))
    assert worst <= c.ld_diff and 4.0 * c.ld_diff <= 1e-10


# ---- 5. the believed-feasible front rule ----
@pytest.mark.parametrize("M", (2, 3))
def test_the_believed_feasible_front_rule_binds_with_margins(M):
    c = ch.BELIEVED[M]
    p = ch.make_problem(c)
    origin = tuple([0.0] * M)
    for T in (LD, np.float64):
        m0, m1 = ch.ensemble(p, T)
        # every constraint mean lies at least MARGIN from its threshold: no rounding flips a belief
        for m in (m0, m1):
            gap = min(abs(float(mu) - tau) for mus, tau in zip(m.constraint_means, m.taus) for mu in mus)
            assert gap >= ch.MARGIN, gap
        assert list(m0.mask) == [True, True, True] and list(m1.mask) == [True, False, True]
        # pending point 0 is believed feasible under member 0, joins its front and the origin leaves
        assert m0.log[0][0] == "joined" and m0.log[0][1] == 1
        assert not any(tuple(float(x) for x in q) == origin for q in m0.front)
        assert any(all(float(q[k]) == float(m0.outcomes[0][k]) for k in range(M)) for q in m0.front)
        # pending point 1 is believed infeasible under member 1: it is not offered -- and it WOULD have joined and evicted the origin
        rule = hr.believed_front if M == 2 else h3.believed_front
        _, would = rule(p.front, m1.outcomes, p.ref, T)
        assert would[1][0] == "joined" and would[1][1] >= 1
        assert len(m1.offered) == 2 and any(tuple(float(x) for x in q) == origin for q in m1.front)
        # pending point 2 is believed feasible under both and dominated under both (the last offered outcome of each)
        assert m0.log[2][0] == "dominated" and m1.log[1][0] == "dominated"
        # every outcome lies at least MARGIN from every front point it is compared with and from the reference point, the outcome
        # that is held back included (compared as if it had been offered)
        for m in (m0, m1):
            assert ch.join_margin(p.front, m.offered, p.ref, M) >= ch.MARGIN
            assert ch.join_margin(p.front, m.outcomes, p.ref, M) >= ch.MARGIN
    # the held-back outcome matters: offering it changes member 1's value at the candidates by far more than the device's tolerance
    m1 = ch.ensemble(p, LD)[1]
    mod = hr if M == 2 else h3
    offered_all = mod.Member(p.gps[1][:M], p.ref, p.front, p.pending, LD)
    moved = [abs(float(offered_all.evaluate(x)[0] - m1.evaluate(x)[2][0])) for x in p.points]
    print("M = %d: H under member 1 moves by %s when the believed-infeasible outcome is offered" % (M, ["%.3g" % v for v in moved]))
    assert max(moved) >= 1e-3


@pytest.mark.parametrize("M", (2, 3))
def test_the_changing_belief_problem_crosses_tau_at_the_middle_of_the_first_coordinate(M):
    p, starts = ch.changing_problem(M)
    assert len(p.gps) == 2 and len(p.taus) == 1 and p.taus[0] == 0.0 and p.pending.shape == (1, 3) and p.pending[0, 0] < 0.45
    assert starts.shape == (12, 3) and np.all(starts[:6, 0] < 0.35) and np.all(starts[6:, 0] > 0.65)  # (two clusters)
    con = p.gps[1][M]
    assert float(np.max(np.abs(con.y[:, 0] - ch.CHANGING_SLOPE * (0.5 - con.X[:, 0])))) <= 0.05
    rng = np.random.default_rng(1)
    grid = rng.uniform(0, 1, size=(200, 3))
    for T in (LD, np.float64):
        mu0 = np.asarray(cr.mean_at(cr.base_model(p.gps[0][M], T), grid), dtype=np.float64)
        mu1 = np.asarray(cr.mean_at(cr.base_model(con, T), grid), dtype=np.float64)
        assert np.all(mu0 <= -ch.MARGIN)  # member 0 believes every point feasible
        far = np.abs(grid[:, 0] - 0.5) >= 0.1
        assert np.all(mu1[far & (grid[:, 0] < 0.5)] >= ch.MARGIN) and np.all(mu1[far & (grid[:, 0] > 0.5)] <= -ch.MARGIN)
    assert float(cr.mean_at(cr.base_model(con, LD), p.pending)[0]) >= ch.MARGIN  # (the pending point: believed infeasible)


# ---- 5b. sixty-four pending points under a mixed mask ----
@pytest.mark.parametrize("M", (2, 3))
def test_the_mixed_mask_problem_is_qualified(M):
    c = ch.MASKED[M]
    p, want = ch.expected(c, LD)
    _, got = ch.expected(c, np.float64)
    assert c.E == 5 and c.K == 1 and len(p.pending) == 64 and len(p.front) == (200 if M == 2 else 100)
    assert all(18 <= n <= 22 for row in c.n for n in row)
    worst = 0.0
    for w, g in zip(want, got):
        worst = max(worst, abs(float(g.value - w.value)) / w.scale, float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / w.scale,
                    max(abs(float(a - b)) for fa, fb in zip(g.factors, w.factors) for a, b in zip(fa, fb)) / w.scale)
    assert worst <= c.ld_diff and 4.0 * c.ld_diff <= 1e-10
    masks = {}
    for T in (np.float64, LD):
        members = ch.ensemble(p, T)
        masks[T] = np.array([m.mask for m in members])
        margin = min(abs(float(mu) - p.taus[0]) for m in members for mu in m.constraint_means[0])
        assert margin >= 1e-3                                                        # every belief decided by 1e-3
        assert np.all(masks[T].sum(axis=1) >= 16) and np.all((~masks[T]).sum(axis=1) >= 16)
        disagree = min(int(np.sum(masks[T][a] != masks[T][b])) for a in range(5) for b in range(a))
        assert disagree >= 8                                                         # every two members disagree on 8 points
        joins = [ch.join_margin(p.front, m.offered, p.ref, M) for m in members]
        assert min(joins) >= 1e-6
        effects = [ch.mask_effects(m, p.front) for m in members]
        assert all(len(ev) >= 1 and len(mi) >= 1 for ev, mi in effects), effects
        sizes = [len(m.front) for m in members]
        assert len(set(sizes)) >= 3  # (the members' fronts differ in length)
        if T is LD:
            print("%s: float64 - long double %.2e scale; beliefs decided by %.3g; feasible per member %s; two members disagree on at least "
                  "%d points; join margin %.3g; fronts %s; outcomes that evict past index 64 per member %s, skipped outcomes that would "
                  "have joined and dominate a later offered one %s" % (c.name, worst, margin, masks[T].sum(axis=1).tolist(), disagree,
                                                                       min(joins), sizes, [len(ev) for ev, _ in effects],
                                                                       [len(mi) for _, mi in effects]))
    assert np.array_equal(masks[np.float64], masks[LD])
    # the mask matters to every member: its H_e under the all-ones mask lies more than 1e-3 scale away at some candidate
    members = ch.ensemble(p, LD)
    ones = [ch.remasked(m, [True] * 64, p.front) for m in members]
    for e in range(5):
        gap = max(abs(float(members[e].evaluate(x)[2][0] - ones[e].evaluate(x)[2][0])) for x in p.points) / want[0].scale
        assert gap > 1e-3, (e, gap)


# ---- 6. feasible_pareto_front ----
def test_feasible_pareto_front_on_hand_computed_inputs():
    obj = [(1.0, 3.0), (2.0, 2.0), (3.0, 1.0), (0.5, 0.5), (2.5, 2.5)]
    con = [(0.0,), (0.2,), (-1.0,), (0.3,), (-2.0,)]
    # (0.5, 0.5) dominates everything and is infeasible; (2, 2) is infeasible; (2.5, 2.5) is feasible and not dominated by a feasible one
    f = cehvi.feasible_pareto_front(obj, con, [0.1], (4.0, 4.0))
    assert np.array_equal(f, np.array([(1.0, 3.0), (2.5, 2.5), (3.0, 1.0)]))
    # a point on its threshold is feasible; no constraints: the plain front
    assert np.array_equal(cehvi.feasible_pareto_front(obj, con, [0.2], (4.0, 4.0)), np.array([(1.0, 3.0), (2.0, 2.0), (3.0, 1.0)]))
    assert np.array_equal(cehvi.feasible_pareto_front(obj, np.zeros((5, 0)), [], (4.0, 4.0)), np.array([(0.5, 0.5)]))
    assert cehvi.feasible_pareto_front(obj, con, [-5.0], (4.0, 4.0)).shape == (0, 2)
    # two constraints, three objectives: the canonical order of pareto_front_3
    obj3 = [(1.0, 2.0, 3.0), (3.0, 2.0, 1.0), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)]
    con2 = [(0.0, 0.0), (0.0, 0.0), (1.0, 0.0), (0.0, 0.0)]
    f3 = cehvi.feasible_pareto_front(obj3, con2, [0.5, 0.5], (4.0, 4.0, 4.0))
    assert np.array_equal(f3, np.array([(3.0, 2.0, 1.0), (2.0, 2.0, 2.0), (1.0, 2.0, 3.0)]))
    with pytest.raises(ValueError):
        cehvi.feasible_pareto_front(obj, con[:4], [0.1], (4.0, 4.0))
    with pytest.raises(ValueError):
        cehvi.feasible_pareto_front(obj, con, [0.1, 0.2], (4.0, 4.0))
