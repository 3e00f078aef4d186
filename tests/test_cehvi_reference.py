"""CPU tests (-m "not gpu") of the constrained expected hypervolume improvement: tests/cehvi_reference.py, the restatement
tests/test_gpu_cehvi.py checks the device against, is itself checked here -- without constraints against tests/ehvi_reference.py and
tests/ehvi3_reference.py term for term, float64 against long double (the measured ld_diff is the case table's), the gradient against
central differences of the long-double value -- and every case is QUALIFIED: at its checked candidates, at least 7 of its 8, the value
and the gradient are far above the device test's tolerance, and dropping the constraints, emptying the front or dropping the pending
points each moves the value by far more than that tolerance, so that a device which returned zeros, ignored the constraints, ignored
the front or ignored P could not pass.  A case that breaks a condition fails; none is skipped.  Then the believed-feasible front rule
with its margins, and feasible_pareto_front on hand-computed inputs."""
import numpy as np
import pytest

import cehvi_reference as ch
import ehvi3_reference as h3
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
