"""CPU tests (-m "not gpu") of tests/log_ehvi3_reference.py, the restatement tests/test_gpu_log_ehvi3.py checks the device against:
exp(L) is the plain box sum of tests/ehvi3_reference.py, the six coefficients are the derivatives of L, the float64 replay of
logehvi3_box_kernel's thread order agrees with the order-free restatement, and constructed inputs reach every branch of the kernel's
record rules, which the replay counts."""
import numpy as np
import pytest

import ehvi3_reference as h3
import log_ehvi3_reference as l3

LD = l3.LD
# one case per front size (the box sum does not see the constraints), shift 0
BOX_CASES = [c for c in l3.CASES if c.K == 1] + l3.EDGE_CASES


def _moments(m, x):
    return [(q[0], q[1]) for q in l3.member_moments(m, x)]


@pytest.mark.parametrize("case", BOX_CASES, ids=[c.name for c in BOX_CASES])
def test_exp_of_the_log_box_sum_is_the_plain_box_sum_and_the_coefficients_are_its_derivatives(case):
    """Long double.  Value: 1e-12 relative.  Coefficients: central differences of L with step h = 1e-5 in mu and 1e-5 var in var;
    the truncation error is h^2 |L'''| / 6, of order 1e-10 times a third derivative that reaches 1e3 where sigma is about 0.1, and
    the rounding error 1e-19 |L| / h is far below: the bound is 1e-6 max(1, |coefficient|)."""
    p, members = l3.shifted(case, l3.SHIFTS[0], LD)
    worst_v = worst_c = 0.0
    for m in members:
        for x in p.points[:3]:
            mo = _moments(m, x)
            L, c, skipped = l3.log_boxes(mo, m.front, m.ref, LD, m.table)
            A, _ = h3.box_sum(mo, m.front, m.ref, LD, m.table)
            assert A > 0
            worst_v = max(worst_v, abs(float((np.exp(L) - A) / A)))
            for r in range(3):
                for which in range(2):
                    h = LD(1e-5) * (LD(1) if which == 0 else mo[r][1])
                    up, dn = [list(q) for q in mo], [list(q) for q in mo]
                    up[r][which], dn[r][which] = mo[r][which] + h, mo[r][which] - h
                    fd = (l3.log_boxes(up, m.front, m.ref, LD, m.table)[0] - l3.log_boxes(dn, m.front, m.ref, LD, m.table)[0]) / (2 * h)
                    got = c[2 * r + which]
                    worst_c = max(worst_c, abs(float(got - fd)) / max(1.0, abs(float(got))))
    print("%s: |exp(L) - box_sum| / box_sum at most %.3g; coefficients against central differences at most %.3g" % (
        case.name, worst_v, worst_c))
    assert worst_v <= 1e-12 and worst_c <= 1e-6


@pytest.mark.parametrize("case,shift", [(c, s) for c in BOX_CASES for s in l3.SHIFTS],
                         ids=["%s-r%g" % (c.name, s[0]) for c in BOX_CASES for s in l3.SHIFTS])
def test_the_thread_order_replay_agrees_with_the_restatement_in_float64(case, shift):
    p, members = l3.shifted(case, shift, np.float64)
    worst = worst_c = 0.0
    for m in members:
        for x in p.points[:3]:
            mo = _moments(m, x)
            L, c, skipped = l3.log_boxes(mo, m.front, m.ref, np.float64, m.table)
            r = l3.thread_replay(mo, m.front, m.ref, m.table)
            worst = max(worst, abs(r["L"] - float(L)) / max(1.0, abs(float(L))))
            worst_c = max(worst_c, max(abs(a - float(b)) / max(1.0, abs(float(b))) for a, b in zip(r["c"], c)))
            assert r["w_skipped"] + r["p_one"] == skipped
            assert r["first"] + r["rescales"] + r["below"] == len(m.table) - skipped
    print("%s %s: replay against restatement %.3g (value), %.3g (coefficients)" % (case.name, shift, worst, worst_c))
    assert worst <= 1e-13 and worst_c <= 1e-11


def test_the_cases_tables_reach_the_sweeps_they_are_named_for():
    differ = 0
    for c, shift in l3.CASE_SHIFTS:
        _, members = l3.shifted(c, shift, np.float64)
        B = [len(m.table) for m in members]
        if c.F <= 2:
            assert max(B) < 64, (c.name, B)                      # lanes and whole wavefronts without a box
            differ += len(set(tuple(map(tuple, np.asarray(m.front, dtype=np.float64))) for m in members)) == 3
        elif c.F == 22:
            assert 276 <= min(B) and max(B) < 512, (c.name, B)   # a second sweep in some threads
        else:
            assert min(B) >= 1081, (c.name, B)                   # a second sweep in every wavefront
    print("case-shifts of F <= 2 in which all three members' believed fronts differ: %d of 36" % differ)
    assert differ > 0


# ---- constructed inputs: the moments are given, no GP ----
REF = (1.5, 1.4, 1.3)


def _stair(F):
    return h3.staircase_front(F)


def test_every_branch_of_the_record_rules_is_reached():
    # B < 256: a front of two, six boxes at most -- threads, lanes and whole wavefronts whose record holds no box
    small = l3.thread_replay([(0.1, 0.3), (0.0, 0.2), (-0.1, 0.25)], _stair(2), REF)
    assert small["boxes"] == 6 and small["first"] == 6 and small["rescales"] == small["below"] == 0 and small["later_sweeps"] == 0
    assert small["empty"] > 0 and small["wave_empty"] == 3  # (wavefronts 1 .. 3 hold nothing: every wavefront merge meets an empty record)
    assert small["p_one"] == small["w_one"] == 0
    # B > 256: the staircase of 22, 276 boxes -- threads 0 .. 19 take a second box, above and below their first
    big = l3.thread_replay([(0.1, 0.3), (0.0, 0.2), (-0.1, 0.25)], _stair(22), REF)
    assert big["boxes"] == 276 and big["later_sweeps"] == 20 and big["first"] == 256
    assert big["rescales"] + big["below"] == 20 and big["rescales"] > 0 and big["below"] > 0
    assert big["empty"] == 0 and big["wave_empty"] == 0 and big["won_low"] > 0 and big["won_high"] > 0
    # rho > 1/2: wide posteriors against edges that lie close together
    wide = l3.thread_replay([(0.0, 9.0), (0.0, 9.0), (0.0, 9.0)], _stair(22), REF)
    assert wide["p_high"] > 0 and wide["w_high"] > 0 and wide["p_one"] == 0 and wide["w_one"] == 0
    # and rho <= 1/2 with narrow ones
    assert big["p_low"] > 0 and big["w_low"] > 0
    L = l3.log_boxes([(0.0, 9.0), (0.0, 9.0), (0.0, 9.0)], _stair(22), REF, np.float64)
    assert abs(wide["L"] - float(L[0])) <= 1e-13 * max(1.0, abs(float(L[0]))) and L[2] == 0


def test_the_boxes_of_a_zero_thickness_slab_and_of_equal_edges_are_skipped_and_nothing_more():
    mo = [(-5.0, 0.3), (0.0, 0.2), (-0.1, 0.25)]
    # rho = 1 in W: two points share w exactly; slab 2 has the staircase of the first two points, three boxes
    tie = l3.thread_replay(mo, l3.TIE_FRONT, REF)
    table = h3.box_table(l3.TIE_FRONT)
    in_slab = int(np.sum(table[:, 3] == 2))
    assert in_slab == 3 and tie["w_one"] == 1 and tie["w_skipped"] == 3 and tie["p_one"] == 0
    assert l3.log_boxes(mo, l3.TIE_FRONT, REF, np.float64)[2] == 3 and l3.log_boxes(mo, l3.TIE_FRONT, REF, LD)[2] == 3
    # rho = 1 in P: two neighbouring u edges an ulp apart under a mean that lies 5 below them -- t - mu rounds the ulp away, so the
    # two edges' lambda_1 are the same float64 -- the box between them in slabs 2 and 3
    front = l3.ulp_front()
    assert (front[0, 0] - mo[0][0]) == (front[1, 0] - mo[0][0]) and front[0, 0] < front[1, 0]
    table = h3.box_table(front)
    between = int(np.sum((table[:, 0] == 1) & (table[:, 1] == 2)))
    ulp = l3.thread_replay(mo, front, REF)
    assert between == 2 and ulp["p_one"] == 2 and ulp["w_one"] == 0 and ulp["w_skipped"] == 0
    L64 = l3.log_boxes(mo, front, REF, np.float64)
    assert L64[2] == 2 and np.isfinite(float(L64[0])) and all(np.isfinite(float(c)) for c in L64[1])
    # the skipped boxes carry nothing: the long-double restatement, which may keep them, agrees
    LL = l3.log_boxes(mo, front, REF, LD)
    assert abs(float(LL[0]) - float(L64[0])) <= 1e-13 * max(1.0, abs(float(L64[0])))
    # both at once, and the value is still that of the plain box sum
    for f, skipped in ((l3.TIE_FRONT, 3), (front, 2)):
        A = h3.box_sum(mo, f, REF, LD)[0]
        L = l3.log_boxes(mo, f, REF, np.float64)
        assert L[2] == skipped and abs(float(np.exp(LD(L[0])) - A) / float(A)) <= 1e-12


def test_the_stall_problems_underflow_in_the_plain_form():
    import cehvi_reference as ch
    for kind in l3.STALL_KINDS:
        p = l3.stall_problem(kind)
        members = ch.ensemble(p, np.float64)
        for x in l3.stall_starts():
            assert float(ch.evaluate(members, x).value) == 0.0
            r = l3.evaluate(members, x)
            assert np.isfinite(float(r.value)) and float(np.max(np.abs(r.grad))) > 0.0
