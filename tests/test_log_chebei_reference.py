"""CPU tests (-m "not gpu") that qualify tests/log_chebei_reference.py, the checker of tests/test_gpu_log_chebei.py, and the
refusals of moe_log_ei_chebyshev_constrained_mcmc* that need no handle:

(a) the fixed quadrature (chebei1.hip's breakpoints and the ladder below the incumbent) against an independent evaluation, every
    panel halved under a 32-node rule in long double, on RULE_CASES random cases, M = 2 .. 8, tau_j from 1e-6 to 3, more than a third
    of them with the incumbent below L, some 60, 200 and 1000 deviations below every s_j;
(b) exp(LA) against chebei_reference's value where that is above 1e-200;
(c) the coefficients against central differences of the long-double LA;
(d) K = 0 with E = 1 is LA_0 bit for bit, every branch of the believed-and-feasible rule by hand, the refusals in the header's order.
"""
import ctypes as C
import math

import numpy as np
import pytest

import chebei_reference as ch
import log_chebei_reference as lc
import logcei1_reference as lr
from cornell_moe_amd import _lib, build as moe_build

LD = lc.LD
dp, ip = _lib.dp, _lib.ip
# Looked up for ONE purpose: on a tree without the three entry points this module fails to import, so that none of its tests, which
# qualify the checker of those entry points and call the library only in the refusals, passes where the feature is missing.
ENTRY_POINTS = [_lib.SIGNATURES[name] for name in ("moe_log_ei_chebyshev_constrained_mcmc", "moe_log_ei_chebyshev_constrained_mcmc_multistart",
                                                   "moe_log_ei_chebyshev_constrained_mcmc_suggest")]


def test_the_array_form_of_log_cdf_parts_is_the_scalar_function_bit_for_bit():
    rng = np.random.default_rng(11)
    z = np.concatenate([rng.uniform(-45.0, 9.0, size=300), -np.exp(rng.uniform(0.0, 20.0, size=60)), [0.0, -0.0, -3.0, -38.0, 40.0]])
    for T in (np.float64, LD):
        l, r = lc.log_cdf_parts_many(z.astype(T), T)
        for i, zi in enumerate(z):
            ls, rs = lr.log_cdf_parts(T(zi), T)
            assert l[i] == ls and r[i] == rs, (T, zi)


# ---- (a) the rule against an independent evaluation ----
RULE_CASES = 84
RULE_BOUND = 1e-12


def rule_cases(n=RULE_CASES, seed=5):
    """(a, b, mus, variances, g, kind): the incumbent g in [-1, 1], b_j in [-0.5, 0.5] and every z_j(g) are drawn and mu_j follows
    from s_j = g - z_j tau_j, tau_j log-uniform in [1e-6, 3] and a_j in [0.05, 5] independently per objective.
      deep     z_j = -k u_j, u_j in [1.001, 1.1], k = 60, 200, 1000: g lies k deviations below every s_j (M <= 4 at k = 1000, so
               that |LA| stays below 2.5e6, which long double resolves to 2.3e-13: beyond 9e6 it cannot hold a log to 1e-12)
      belowL   one z_j in [-60, -38.5], the others in [-38, 10]: g below L, where the plain form is exactly 0
      bulk     z_j in [-8, 8];  tail  z_j in [-37, 3];  edge  one z_j in [-38, -37], the others in [-30, 30]: g just above L"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        M = 2 + i % 7
        kind = ("deep", "belowL", "belowL", "bulk", "tail", "edge")[i % 6]
        a = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=M))
        tau = np.exp(rng.uniform(np.log(1e-6), np.log(3.0), size=M))
        b = rng.uniform(-0.5, 0.5, size=M)
        g = rng.uniform(-1, 1)
        if kind == "deep":
            k = (60.0, 200.0, 1000.0)[(i // 6) % 3]
            if k == 1000.0:
                M = min(M, 4)
                a, tau, b = a[:M], tau[:M], b[:M]
            z = -k * rng.uniform(1.001, 1.1, size=M)
        elif kind == "belowL":
            z = rng.uniform(-38.0, 10.0, size=M)
            z[rng.integers(M)] = -rng.uniform(38.5, 60.0)
        elif kind == "bulk":
            z = rng.uniform(-8.0, 8.0, size=M)
        elif kind == "tail":
            z = rng.uniform(-37.0, 3.0, size=M)
        else:
            z = rng.uniform(-30.0, 30.0, size=M)
            z[rng.integers(M)] = -rng.uniform(37.0, 38.0)
        s = g - z * tau
        out.append((a, b, (s - b) / a, (tau / a) ** 2, g, kind))
    return out


def rule_errors(a, b, mus, variances, g):
    """(|LA - independent|, the worst coefficient error) in long double.  A coefficient's error is |difference| / max(scale, 1e-12
    natural).  scale is |c| for mu, whose integrand has one sign.  For var it is the same mean with |z_j| in the place of z_j: the
    integrand changes sign with z_j, the signed mean passes through 0 as the inputs move, and an error relative to |c| has no
    bound there -- a bulk case of rule_cases(168, 11) (z_j(g) = 7.5, tau_j = 1.3e-6) has c = -2.3e6 under an unsigned mean of
    4.3e9, and the 8-node panels' 6e-15 of that scale is 1.1e-11 of |c|, whatever the ladder.  natural is a_j / tau_j and a_j /
    (2 sigma_j tau_j), the coefficient of an objective at the middle of its own transition -- the floor below which a coefficient
    (1e-75 for an objective 45 deviations below g) is noise."""
    LA, c, I = lc.log_value_at_moments(a, b, mus, variances, g, LD)
    RA, rc, rs = lc.refined_log_value(a, b, mus, variances, g, LD)
    s, tau, sg = ch.scalarised_moments(a, b, mus, variances, LD)
    worst = 0.0
    for j in range(len(a)):
        natural = (float(a[j] / tau[j]), float(a[j] / (2 * sg[j] * tau[j])))
        for q in range(2):
            worst = max(worst, abs(float(c[2 * j + q] - rc[2 * j + q])) / max(float(rs[2 * j + q]), 1e-12 * natural[q]))
    L = max(s[j] - 38 * tau[j] for j in range(len(a)))
    return abs(float(LA - RA)), worst, float(LA), bool(LD(g) <= L), s, tau


def test_the_fixed_quadrature_agrees_with_halved_panels_and_a_32_node_rule():
    cases = rule_cases()
    assert len(cases) >= 60 and {len(c[0]) for c in cases} == set(range(2, 9))
    worst_A, worst_c, below, deep = 0.0, 0.0, 0, set()
    for a, b, mus, variances, g, kind in cases:
        eA, ec, LA, is_below, s, tau = rule_errors(a, b, mus, variances, g)
        assert math.isfinite(LA)
        below += is_below
        if is_below:
            assert ch.value_at_moments(a, b, mus, variances, g, np.float64)[0] == 0.0  # the plain form is exactly 0 there
        if kind == "deep":
            depth = min(float((s[j] - g) / tau[j]) for j in range(len(a)))
            deep.add(max(k for k in (0, 60, 200, 1000) if depth >= k))
        worst_A, worst_c = max(worst_A, eA), max(worst_c, ec)
    print("%d cases, %d with the incumbent below L, deep ones from %s deviations: |LA - independent| <= %.3g, coefficients within %.3g"
          % (len(cases), below, sorted(deep), worst_A, worst_c))
    assert 3 * below >= len(cases) and deep == {60, 200, 1000}
    assert worst_A <= RULE_BOUND and worst_c <= RULE_BOUND


# ---- (b) agreement with the plain form ----
def test_where_the_plain_form_is_representable_the_log_form_is_its_log():
    worst, seen = 0.0, 0
    log_ld = max(c.ld_diff for c in lc.ALL_CASES if not c.drop)
    for case in ch.CASES:
        p, want = ch.expected(case, LD)
        if case.E != 1 or case.kind == "below":
            continue
        ms = ch.ensemble(p, LD)
        tol = max(1e-10, 4.0 * max(case.ld_diff, log_ld))  # (both restatements' recorded long-double differences)
        for x, w in zip(p.points, want):
            if not float(w.value) > 1e-200:
                continue
            mo = ms[0].moments(x)
            g = ms[0].incumbent(p.scal[0], p.best[0][0])
            sa, sb = ch.split(p.scal[0])
            LA, _, _ = lc.log_value_at_moments(sa, sb, [m[0] for m in mo], [m[1] for m in mo], g, LD)
            err = abs(float(np.exp(LA) - w.value)) / w.scale
            worst, seen = max(worst, err), seen + 1
            assert err <= tol, (case.name, err)
    print("exp(LA) against the plain form at %d candidates: the worst difference %.3g scale" % (seen, worst))
    assert seen >= 40


# ---- (c) the coefficients against central differences of the long-double LA ----
# chebei_reference's measured 3.1e-11 times 10: the log divides by A
DIFFERENCE_BOUND = 3.1e-10


@pytest.mark.parametrize("M,depth", [(2, 0.0), (3, 0.0), (8, 0.0), (3, 20.0), (4, 60.0)])
def test_the_coefficients_are_the_derivatives_of_the_log(M, depth):
    rng = np.random.default_rng(500 + M)
    a = rng.uniform(0.3, 1.5, size=M)
    b = rng.uniform(-0.2, 0.2, size=M)
    mus = rng.uniform(-0.3, 0.3, size=M)
    var = rng.uniform(0.2, 1.0, size=M) ** 2
    g = float(np.max(a * mus + b)) + 0.1 - depth * float(np.max(a * np.sqrt(var)))
    LA, c, _ = lc.log_value_at_moments(a, b, mus, var, g, LD)
    worst = 0.0
    for j in range(M):
        for k, arr in ((0, mus), (1, var)):
            h = 1e-6
            up, dn = arr.copy(), arr.copy()
            up[j] += h
            dn[j] -= h
            hi = lc.log_value_at_moments(a, b, up if k == 0 else mus, up if k == 1 else var, g, LD)[0]
            lo = lc.log_value_at_moments(a, b, dn if k == 0 else mus, dn if k == 1 else var, g, LD)[0]
            fd = float((hi - lo) / (LD(up[j]) - LD(dn[j])))
            worst = max(worst, abs(fd - float(c[2 * j + k])) / max(1e-3, abs(fd)))  # (test_chebei_reference.py's measure)
    print("M = %d, %g deviations down: LA = %.6g, coefficients against central differences: the worst relative difference %.3g" % (
        M, depth, float(LA), worst))
    assert worst <= DIFFERENCE_BOUND


# ---- (d) one member without constraints; the believed-and-feasible rule; float64 against long double ----
def test_one_member_without_constraints_is_its_own_log_bit_for_bit():
    p = lc.make_problem(lc.case("log_m3_e1_k0_d3_n20_p2"))
    for T in (np.float64, LD):
        ms = lc.ensemble(p.gps, p.M, p.taus, p.pending, T)
        r = lc.evaluate(ms, p.points[1], p.scal, p.best)
        assert r.value == r.log_factors[0][0] and np.array_equal(r.grad, r.members_grad[0])
    v = lc.host_value(np.array([[[float(r.log_factors[0][0])]]]))
    assert v[0] == float(r.log_factors[0][0])


def test_every_branch_of_the_believed_and_feasible_rule():
    c = lc.BELIEVED
    p = lc.make_problem(c)
    a, b = ch.split(p.scal)
    for T in (np.float64, LD):
        ms = lc.ensemble(p.gps, p.M, p.taus, p.pending, T)
        out = [ch.scalarised_outcomes(a, b, m.outcomes, T) for m in ms]
        low = int(np.argmin(out[0]))
        # member 0: its lowest outcome is believed infeasible and does not join; the next one, feasible and lower, does
        assert list(ms[0].mask) == [i != low for i in range(c.p)] and all(ms[1].mask)
        assert ms[0].incumbent(p.scal, p.best[0]) == sorted(out[0])[1] < T(p.best[0])
        # member 1 believes all feasible: its lowest outcome joins
        assert ms[1].incumbent(p.scal, p.best[1]) == min(out[1])
        # none lower: the caller's incumbent stands
        assert ms[1].incumbent(p.scal, float(min(out[1])) - 0.1) == T(float(min(out[1])) - 0.1)
        # the margins are clear of rounding
        assert min(abs(float(m_)) - 0.0 for m in ms for mu in m.constraint_means for m_ in mu) > 0.4
    # by hand: outcomes [M][p] scalarised to 0.5, 0.2, 1.0 under (1, 2 | 0, -1)
    hand = lc.Member.__new__(lc.Member)
    hand.T, hand.outcomes = np.float64, [np.array([0.5, 0.2, 1.0]), np.array([0.5, 0.6, 1.0])]
    scal = np.array([1.0, 2.0, 0.0, -1.0])
    for mask, best, want in (((True, True, True), 0.7, 0.2), ((True, False, True), 0.7, 0.5), ((False, False, True), 0.7, 0.7),
                             ((True, True, True), 0.1, 0.1)):
        hand.mask = np.array(mask)
        assert float(hand.incumbent(scal, best)) == pytest.approx(want)


@pytest.mark.parametrize("case", lc.ALL_CASES, ids=[c.name for c in lc.ALL_CASES])
def test_float64_against_long_double_on_the_cases_of_the_gpu_tests(case):
    worst = lc.ld_difference(case)
    print("%s: float64 against long double %.3g (recorded %.3g)" % (case.name, worst, case.ld_diff))
    assert worst <= 1.05 * case.ld_diff
    _, want = lc.expected(case, LD)
    if case.drop >= lc.STALL_DROP:
        p = lc.make_problem(case)
        ms = ch.ensemble(ch.Problem(p.name, p.M, [row[:p.M] for row in p.gps], [p.scal], [p.best], p.points, p.pending, ()), np.float64)
        for x in p.points:  # the plain form is exactly 0 with zero coefficients
            A, gr = ms[0].evaluate(x, p.scal, p.best[0])
            assert A == 0.0 and not np.any(gr)
        assert all(float(w.log_factors[0][0]) < -745.0 for w in want)
    if case.far:
        assert all(float(w.log_factors[0][1]) < -400.0 for w in want)


@pytest.mark.parametrize("case", lc.EDGE_CASES, ids=[c.name for c in lc.EDGE_CASES])
def test_float64_against_long_double_on_the_edge_cases(case):
    worst = lc.ld_difference(case)
    print("%s: float64 against long double %.3g (recorded %.3g)" % (case.name, worst, case.ld_diff))
    assert worst <= 1.05 * case.ld_diff
    if case.kind.startswith("mixed"):
        live = lc.ld_difference(case, without=lc.stalled_member(case))
        print("%s: without the stalled member's group values %.3g (recorded %.3g)" % (case.name, live, lc.MIXED_LIVE[case.name]))
        assert live <= 1.05 * lc.MIXED_LIVE[case.name]
    _, want = lc.expected(case, LD)
    assert all(np.isfinite(float(w.value)) and np.all(np.isfinite(w.grad.astype(np.float64))) and float(np.max(np.abs(w.grad))) > 0.0
               for w in want)


def _moments_of(member, p, x, T):
    """(s, tau, the offsets d) of a member's objectives at x under the problem's scalarisation and the member's incumbent"""
    a, b = ch.split(p.scal)
    mo = [lc.cr.moments(m, bs, x) for m, bs in zip(member.models[:p.M], member.bases[:p.M])]
    s, tau, _ = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], T)
    return s, tau


def test_the_edge_cases_reach_what_they_are_there_for():
    """the cases of tests/test_gpu_chebei_edges.py, from the restatement alone"""
    # M = 6 and 7: 100 and 114 breakpoints, 792 and 904 nodes; K = 3 and 5 among them, an odd dimension under two members
    for c in lc.M67:
        p = lc.make_problem(c)
        m = lc.ensemble(p.gps, p.M, p.taus, p.pending, np.float64)[0]
        s, tau = _moments_of(m, p, p.points[0], np.float64)
        U, ell, bp, d = lc.log_breakpoints(s, tau, m.incumbent(p.scal, p.best[0]), np.float64)
        assert len(bp) == 14 * c.M + 16 == {6: 100, 7: 114}[c.M] and 8 * (len(bp) - 1) == {6: 792, 7: 904}[c.M]
        assert len(p.taus) == c.K and len(p.gps) == c.E and all(len(row) == c.M + c.K for row in p.gps)
    assert {(c.M, c.E, c.K, c.d) for c in lc.M67} == {(6, 2, 3, 7), (7, 2, 5, 3), (6, 1, 0, 3), (7, 1, 0, 3)}
    # above: at every candidate the rate is exactly 0, in both arithmetics, and ell is the cap; the plain form is positive
    for c in lc.ABOVE:
        p = lc.make_problem(c)
        assert c.E == 1 and c.K == 0 and c.M in (3, 6)
        observed = ch.observed_best([row[:p.M] for row in p.gps], p.scal)
        assert p.best[0] == observed[0] + lc.ABOVE_RAISE
        for T in (np.float64, LD):
            m = lc.ensemble(p.gps, p.M, p.taus, p.pending, T)[0]
            for x in p.points:
                s, tau = _moments_of(m, p, x, T)
                d = lc.offsets(s, tau, p.best[0], T)
                assert lc.decay_rate(d, tau, T) == 0 and lc.decay_length(d, tau, T) == max(tau)
                U, ell, bp, _ = lc.log_breakpoints(s, tau, p.best[0], T)
                assert ell == max(tau) and sum(1 for u in bp if u == T(34.0) * ell) >= 1  # (the ladder stands on the cap)
        plain = ch.ensemble(ch.Problem(p.name, p.M, [row[:p.M] for row in p.gps], [p.scal], [p.best], p.points, p.pending, ()), np.float64)
        assert all(float(plain[0].evaluate(x, p.scal, p.best[0])[0]) > 0.0 for x in p.points)
    # mixed: the stalled member's LL lies more than 745 below the live one's at every candidate, so that its weight is exactly 0,
    # the value is the live member's LL - log 2 and the gradient the live member's
    for c in lc.MIXED:
        p, want = lc.expected(c, np.float64)
        dead = lc.stalled_member(c)
        assert c.E == 2 and c.M == 3 and c.drop == lc.STALL_DROP
        gaps = []
        for w in want:
            LL = [sum(row[1:], row[0]) for row in w.log_factors]
            gaps.append(float(LL[dead] - LL[1 - dead]))
            assert gaps[-1] < -745.0 and np.exp(LL[dead] - LL[1 - dead]) == 0.0
            assert w.value == LL[1 - dead] + np.log(np.float64(1.0)) - np.log(np.float64(2.0))
            assert np.array_equal(w.grad, w.members_grad[1 - dead]) and np.all(np.isfinite(w.members_grad[dead]))
        print("%s: LL of the stalled member below the live one's by %.6g .. %.6g" % (c.name, -max(gaps), -min(gaps)))
    a, b = lc.make_problem(lc.MIXED[0]), lc.make_problem(lc.MIXED[1])
    assert a.best == b.best[::-1] and all(np.array_equal(x.y, y.y) for r, q in zip(a.gps, b.gps[::-1]) for x, y in zip(r, q))
    # p64: the placements, the mask and the margins from the float64 beliefs
    c = lc.P64
    p = lc.make_problem(c)
    sa, sb = ch.split(p.scal)
    assert p.pending.shape == (64, 3) and c.K == 1 and c.E == 2
    for T in (np.float64, LD):
        ms = lc.ensemble(p.gps, p.M, p.taus, p.pending, T)
        out = [[float(v) for v in ch.scalarised_outcomes(sa, sb, m.outcomes, T)] for m in ms]
        o0, o1 = np.argsort(out[0]), np.argsort(out[1])
        assert [int(o0[0]), int(o0[1]), int(o1[0])] == [index for _, _, index in lc.P64_SLOTS] == [62, 63, 40]
        assert list(ms[0].mask) == [i != 62 for i in range(64)] and all(ms[1].mask)
        assert float(ms[0].incumbent(p.scal, p.best[0])) == out[0][63] and float(ms[1].incumbent(p.scal, p.best[1])) == out[1][40]
        assert min(p.best) > max(max(o) for o in out)
        margins = [out[0][o0[1]] - out[0][o0[0]], out[0][o0[2]] - out[0][o0[1]], out[1][o1[1]] - out[1][o1[0]]]
        clear = min(abs(float(v) - p.taus[0]) for m in ms for v in m.constraint_means[0])
        assert min(margins) >= ch.P64_MARGIN and clear > 0.1
    print("p64: outcome margins %s, the constraint means at least %.3g from the threshold" % (margins, clear))
    # half: member 0 believes the region infeasible and the rest feasible, member 1 the whole box feasible, away from the cut;
    # HIGH_BEST lies above everything a member believes anywhere
    c = lc.HALF
    p = lc.make_problem(c)
    k, upper = lc.half_region(c, p.gps, p.pending, p.scal)
    probes = np.random.default_rng(1).uniform(0, 1, size=(400, c.d))
    deep = np.abs(probes[:, k] - 0.5) > 0.25
    inside = (probes[:, k] > 0.5) == upper
    bases = [[lc.cr.base_model(g, np.float64) for g in row] for row in p.gps]
    mean0 = np.array([float(v) for v in lc.cr.mean_at(bases[0][c.M], probes)])
    mean1 = np.array([float(v) for v in lc.cr.mean_at(bases[1][c.M], probes)])
    # (20 observations leave corners of the region where the believed mean falls back towards the other side: nine tenths suffice)
    assert p.taus == (0.0,) and np.mean(mean0[deep & inside] > 1e-3) >= 0.9 and np.all(mean0[deep & ~inside] < -1e-3) and np.all(mean1 < -1e-3)
    scal, best = lc.batch_rounds(p, 3)
    assert np.array_equal(scal[0], p.scal) and best.shape == (3, 2) and np.all(best == lc.HIGH_BEST) and p.best == [lc.HIGH_BEST] * 2
    for t in range(3):
        ta, tb = ch.split(scal[t])
        for row in bases:
            outcomes = [lc.cr.mean_at(bs, probes) for bs in row[:c.M]]
            assert max(float(v) for v in ch.scalarised_outcomes(ta, tb, outcomes, np.float64)) < lc.HIGH_BEST - 0.5
    print("half: member 0 believes x[%d] %s 0.5 infeasible: means %.3g .. %.3g deep inside, %.3g .. %.3g deep outside; member 1's below %.3g"
          % (k, ">" if upper else "<", mean0[deep & inside].min(), mean0[deep & inside].max(), mean0[deep & ~inside].min(),
             mean0[deep & ~inside].max(), mean1.max()))


def test_a_floored_objective_above_the_incumbent_keeps_its_nodes():
    """where ell is far below an ulp of g the ladder g - kappa ell would round to g and leave no node: in offsets LA and its
    coefficients are finite, in both arithmetics alike"""
    for v in (0.0, 1e-24, 1e-20, 1e-18, 1e-12):  # var_0 under s_0 = 1 above g = 0.5: ell = 1.5e-29 .. 2e-12
        out = []
        for T in (np.float64, LD):
            LA, c, I = lc.log_value_at_moments([1.0, 1.0], [0.0, 0.0], [1.0, 0.2], [v, 0.25], 0.5, T)
            assert np.isfinite(LA) and all(np.isfinite(x) for x in c) and I.U > 0 and sum(hi > lo for lo, hi in zip(I.breaks[:-1], I.breaks[1:])) >= 15
            out.append((LA, c))
        assert abs(float(out[0][0] - out[1][0])) <= 64 * np.finfo(np.float64).eps * abs(float(out[1][0]))
        assert all(abs(float(x - y)) <= 1e-10 * abs(float(y)) for x, y in zip(*[o[1] for o in out]))
        # the tangent bound's closed form: LA = log f(g) + log ell up to the curvature's 1 / z^2, the coefficient -a r(g) / tau
        sig = max(np.sqrt(LD(v)), np.sqrt(LD(150)) * LD(np.finfo(np.float64).eps))
        l0, r0 = lr.log_cdf_parts(LD(-0.5) / sig, LD)
        l1, _ = lr.log_cdf_parts(LD(0.3) / LD(0.5), LD)
        closed = l0 + l1 + np.log(I.ell)
        assert abs(float(out[1][0] - closed)) <= max(1e-3, 64 * np.finfo(np.float64).eps * abs(float(closed)))
        assert abs(float(out[1][1][0] + r0 / sig)) <= 1e-6 * float(r0 / sig)
    c = lc.FLOOR_ABOVE
    p, hi = lc.expected(c, LD)
    _, lo = lc.expected(c, np.float64)
    m = lc.ensemble(p.gps, p.M, p.taus, p.pending, np.float64)[0]
    mo = [lc.cr.moments(model, base, p.points[0]) for model, base in zip(m.models, m.bases)]
    a, b = ch.split(p.scal)
    assert float(mo[1][1]) <= 150 * np.finfo(np.float64).eps ** 2 and a[1] * float(mo[1][0]) + b[1] > p.best[0] + 0.1  # floored, above
    for i, (h, l) in enumerate(zip(hi, lo)):
        assert np.isfinite(l.value) and np.all(np.isfinite(l.grad)), i
        assert abs(float(h.value - LD(l.value))) <= max(1e-10, 64 * np.finfo(np.float64).eps * abs(float(h.value))), i
    assert float(hi[0].value) < -1e27 and all(float(h.value) > -10.0 for h in hi[1:])


# ---- the refusals, in the header's order, before a handle is touched ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def _args(M=3, K=2, E=2, d=2, C_=3, p=0, q=1, steps=3, domain=0):
    R, Mp = max(q, 1), max(M, 1)
    a = np.tile(np.concatenate([np.full(Mp, 0.5), np.zeros(Mp)]), (R, 1))
    return dict(gps=(C.c_void_p * max(E * Mp, 1))(), cons=(C.c_void_p * max(E * max(K, 1), 1))(), M=M, K=K, E=E,
                tau=np.zeros(max(K, 1)), scal=np.ascontiguousarray(a), best=np.full((R, max(E, 1)), 0.3),
                pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25), C=C_,
                out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _head(a, g):
    return (g("gps", a["gps"]), a["M"], g("cons", a["cons"]), a["K"], g("tau", _p(a["tau"])), a["E"], g("scal", _p(a["scal"])),
            g("best", _p(a["best"])))


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_chebyshev_constrained_mcmc(*(_head(a, g) + (
        g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], 1, g("ei", _p(a["out"])), g("grad", _p(a["out"])), None,
        C.byref(err))))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_chebyshev_constrained_mcmc_multistart(*(_head(a, g) + (
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None, None, None, None,
        C.byref(err))))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_log_ei_chebyshev_constrained_mcmc_suggest(*(_head(a, g) + (
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])), g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    for call in (_eval, _ascent, _suggest):
        # the number of objectives first, even with everything else wrong
        for M in (1, 9, 0, -1):
            a = _args(M=M, K=9, E=0, C_=0, p=65)
            assert call(lib, a, err, gps=True, pts=True, scal=True) == B and _payload(err) == (float(M), 2.0, 8.0), (call.__name__, M)
        # then the number of constraints
        for K in (-1, 9):
            a = _args(K=K, E=0, C_=0, p=65)
            assert call(lib, a, err, gps=True, pts=True) == B and _payload(err) == (float(K), 0.0, 8.0), (call.__name__, K)
        # then E (M + K) > 1024 (and E < 1): payload (num_mcmc, 1, 1024 // (M + K))
        for M, K, E in ((8, 8, 65), (2, 0, 513), (4, 1, 205), (5, 3, 0)):
            a = _args(M=M, K=K, E=E, C_=0, p=65)
            a["scal"][0, 0] = math.nan
            assert call(lib, a, err, pts=True) == B and _payload(err) == (float(E), 1.0, float(1024 // (M + K))), (call.__name__, M, K, E)
        # the limit itself is accepted as far as the NULL handle
        for M, K, E in ((8, 8, 64), (2, 0, 512), (4, 1, 204)):
            assert call(lib, _args(M=M, K=K, E=E), err) == R and b"NULL GP handle" in err.message, (call.__name__, M, K, E)
        # then NULL arrays; constraint_gps and thresholds only with K > 0
        for name in ("gps", "scal", "best", "pts", "cons", "tau"):
            a = _args(C_=0, p=65)
            a["scal"][0, 0] = -1.0
            assert call(lib, a, err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        assert call(lib, _args(K=0), err, cons=True, tau=True) == R and b"NULL GP handle" in err.message
        # then the scalarisation: payload (the value, its flat index, 0)
        for k, bad in ((0, 0.0), (1, -0.5), (2, math.inf), (0, math.nan), (3, math.nan), (5, -math.inf)):
            a = _args(C_=0, p=65)
            a["scal"][0, k] = bad
            a["tau"][0] = math.nan
            a["best"][0, 0] = math.nan
            assert call(lib, a, err) == V and b"scalarisation" in err.message and _payload(err)[1:] == (float(k), 0.0), (call.__name__, k)
            assert math.isnan(_payload(err)[0]) if math.isnan(bad) else _payload(err)[0] == bad
        # then the thresholds: payload (the value, k, 2)
        for k, bad in ((0, math.nan), (1, math.inf), (1, -math.inf)):
            a = _args(C_=0, p=65)
            a["tau"][k] = bad
            a["best"][0, 0] = math.nan
            assert call(lib, a, err) == V and b"thresholds" in err.message and _payload(err)[1:] == (float(k), 2.0), (call.__name__, k)
        # then the incumbents, +infinity included: payload (the value, its flat index, 1)
        for e, bad in ((0, math.nan), (1, math.inf), (1, -math.inf)):
            a = _args(C_=0, p=65)
            a["best"][0, e] = bad
            assert call(lib, a, err) == V and b"best_so_far" in err.message and _payload(err)[1:] == (float(e), 1.0), (call.__name__, e)
        # then num_points and the pending points: a 65th is refused
        assert call(lib, _args(C_=0, p=65), err) == B and _payload(err)[:2] == (0.0, 1.0)
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        assert call(lib, _args(p=64), err) == R and b"NULL GP handle" in err.message
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        assert call(lib, _args(steps=0, domain=1), err) == B and b"max_num_steps" in err.message
        assert call(lib, _args(domain=1), err) == V and b"Chebyshev" in err.message
    # a batch: picks count as pending points, and every row of the scalarisations and incumbents is checked
    for p, q, hi in ((0, 0, 65.0), (3, 63, 62.0), (64, 2, 1.0)):
        assert _suggest(lib, _args(p=p, q=q), err, pend=(p == 0)) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
    a = _args(q=3)
    a["scal"][2, 1] = 0.0
    assert _suggest(lib, a, err) == V and _payload(err) == (0.0, float(2 * 6 + 1), 0.0)
    a = _args(q=3, E=2)
    a["best"][2, 1] = math.inf
    assert _suggest(lib, a, err) == V and _payload(err) == (math.inf, 5.0, 1.0)
    assert _suggest(lib, _args(q=3, p=2), err) == R and b"NULL GP handle" in err.message
    # the restatement's order is the library's
    assert lc.refusal(9, 9, 0, [], [], []) == ("bounds", "num_objectives") and lc.refusal(3, 9, 0, [], [], []) == ("bounds", "num_constraints")
    assert lc.refusal(8, 8, 65, [], [], []) == ("bounds", "num_mcmc")
    assert lc.refusal(2, 1, 1, [1.0, 0.0, 0.0, 0.0], [math.nan], [math.nan]) == ("invalid", 1)
    assert lc.refusal(2, 1, 1, [1.0, 1.0, 0.0, 0.0], [math.nan], [math.nan]) == ("invalid", 0)
    assert lc.refusal(2, 1, 1, [1.0, 1.0, 0.0, 0.0], [0.0], [math.inf]) == ("invalid", 0)
    assert lc.refusal(2, 1, 1, [1.0, 1.0, 0.0, 0.0], [0.0], [0.0]) is None
