"""CPU tests (-m "not gpu") that qualify tests/chebei_reference.py, the checker of tests/test_gpu_chebei.py, and the refusals of
the three entry points that need no handle.

The restatement is held to the DEFINITION (a Monte-Carlo mean of (g* - max_j (a_j y_j + b_j))^+), to an INDEPENDENT evaluation of
the integral (every panel halved, a 32-node rule, long double: bound 1e-13 of max(1, value)), to the analytic expected improvement
where all objectives but one are irrelevant (the same bound), its coefficients to central differences, its believed-incumbent rule
to every branch by hand, and its float64 form to its long-double form on every case of the GPU tests: the figure recorded there as
ld_diff.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.27 records them."""
import ctypes as C
import math

import numpy as np
import pytest

import chebei_reference as ch
import ei1_reference as er
import kg1_reference as kr
from cornell_moe_amd import _lib, build as moe_build

LD = ch.LD
dp, ip = _lib.dp, _lib.ip


def _random_moments(rng, M):
    """a scalarisation, moments and an incumbent: tau_j from 1e-6 to 3, g* on either side of the s_j"""
    a = 10.0 ** rng.uniform(-1.0, 1.0, size=M)
    b = rng.uniform(-0.5, 0.5, size=M)
    mus = rng.uniform(-1.0, 1.0, size=M)
    sig = 10.0 ** rng.uniform(-6.0, math.log10(3.0), size=M) / a
    s = a * mus + b
    if rng.uniform() < 0.5:  # about the largest s_j, where the value is not tiny
        k = int(np.argmax(s))
        g = float(s[k]) + float(rng.uniform(-2.0, 4.0)) * float(a[k] * sig[k]) + float(rng.uniform(0.0, 0.5))
    else:
        g = float(rng.choice(s)) + float(rng.uniform(-1.0, 1.0)) * float(rng.choice(a * sig)) * 3.0
    return a, b, mus, sig * sig, g


# ---- 0. Phi and phi over arrays are the scalar functions, bit for bit ----
def test_the_array_forms_of_phi_are_the_scalar_functions_bit_for_bit():
    rng = np.random.default_rng(0)
    z = np.concatenate([rng.uniform(-40, 40, 200), rng.uniform(-4, 4, 200), [0.0, -0.0, 2.5 * math.sqrt(2), -2.5 * math.sqrt(2), 38.0, -38.0]])
    for T in (LD, np.float64):
        assert np.array_equal(ch.cdf_many(z, T), np.array([er.normal_cdf(T(v), T) for v in z], dtype=T))
        assert np.array_equal(ch.pdf_many(z, T), np.array([kr.normal_pdf(T(v), T) for v in z], dtype=T))


# ---- 1. the definition ----
@pytest.mark.parametrize("M", [2, 4, 8])
def test_the_integral_is_the_expected_improvement_of_the_scalarisation(M):
    rng = np.random.default_rng(100 + M)
    a = rng.uniform(0.3, 1.5, size=M)
    b = rng.uniform(-0.2, 0.2, size=M)
    mus = rng.uniform(-0.5, 0.5, size=M)
    sig = rng.uniform(0.2, 1.0, size=M)
    g = float(np.max(a * mus + b)) + 0.2
    want, _ = ch.value_at_moments(a, b, mus, sig * sig, g, LD)
    y = mus[None, :] + sig[None, :] * rng.normal(size=(40000, M))
    imp = np.maximum(g - np.max(a[None, :] * y + b[None, :], axis=1), 0.0)
    mean, se = float(np.mean(imp)), float(np.std(imp, ddof=1)) / math.sqrt(len(imp))
    print("M = %d: quadrature %.6g, mean of 4e4 draws %.6g, standard error %.3g: %.2f standard errors apart" % (
        M, float(want), mean, se, abs(mean - float(want)) / se))
    assert float(want) > 1e-3 and abs(mean - float(want)) <= 5.0 * se


# ---- 2. the quadrature against an independent evaluation ----
def test_the_fixed_quadrature_agrees_with_halved_panels_and_a_32_node_rule():
    rng = np.random.default_rng(7)
    worst, positive = 0.0, 0
    for k in range(60):
        M = 2 + k % 7
        a, b, mus, var, g = _random_moments(rng, M)
        got, _ = ch.value_at_moments(a, b, mus, var, g, LD, want_grad=False)
        ref = ch.refined_value(a, b, mus, var, g, LD)
        err = abs(float(got - ref)) / max(1.0, float(ref))
        worst = max(worst, err)
        positive += 1 if float(ref) > 1e-6 else 0
        assert err <= 1e-13, (k, M, float(got), float(ref))
    print("60 random cases, %d with a value above 1e-6: the worst difference %.3g of max(1, value) (bound 1e-13)" % (positive, worst))
    assert positive >= 20


# ---- 3. irrelevant objectives ----
@pytest.mark.parametrize("M", [2, 5, 8])
def test_with_the_other_objectives_irrelevant_it_is_the_analytic_expected_improvement(M):
    rng = np.random.default_rng(300 + M)
    a = rng.uniform(0.5, 2.0, size=M)
    b = rng.uniform(-0.2, 0.2, size=M)
    mus = rng.uniform(-0.5, 0.5, size=M)
    sig = rng.uniform(0.01, 0.05, size=M)
    sig[0] = 0.02
    # objectives 2 .. M lie so low that s_j + 8 tau_j <= s_1 - 38 tau_1
    s1, tau1 = a[0] * mus[0] + b[0], a[0] * sig[0]
    for j in range(1, M):
        b[j] = (s1 - 38.0 * tau1) - 8.0 * a[j] * sig[j] - a[j] * mus[j] - 0.01 * (1 + j)
    worst = 0.0
    for g in (s1 - 2.0 * tau1, s1, s1 + 3.0 * tau1, s1 + 1.0):
        got, _ = ch.value_at_moments(a, b, mus, sig * sig, g, LD, want_grad=False)
        want = LD(a[0]) * ch.analytic_ei(mus[0], sig[0], (LD(g) - LD(b[0])) / LD(a[0]), LD)
        worst = max(worst, abs(float(got - want)) / max(1.0, float(want)))
    print("M = %d: the worst difference from a_1 EI_1 %.3g of max(1, value) (bound 1e-13)" % (M, worst))
    assert worst <= 1e-13


# ---- 4. float64 against long double: ld_diff ----
_QUALIFIED = ch.ALL_CASES + ch.EDGE_CASES


@pytest.mark.parametrize("case", _QUALIFIED, ids=[c.name for c in _QUALIFIED])
def test_float64_against_long_double_on_the_cases_of_the_gpu_tests(case):
    measured = ch.ld_difference(case)
    p, want = ch.expected(case, LD)
    print("%s: ld_diff %.3g (recorded %.3g); values %.3g .. %.3g" % (case.name, measured, case.ld_diff,
                                                                      min(float(w.value) for w in want), max(float(w.value) for w in want)))
    assert measured <= case.ld_diff
    if case.kind == "below":
        assert all(float(w.value) == 0.0 and not np.any(w.grad) for w in want)
    else:
        assert all(float(w.value) > 0.0 for w in want) and max(float(np.max(np.abs(w.grad))) for w in want) > 1e-4


def test_the_many_member_case_in_float64_against_long_double_on_three_members():
    members = (0, 63, 127)
    p, hi = ch.expected(ch.MANY, LD, members)
    _, lo = ch.expected(ch.MANY, np.float64, members)
    worst = max(abs(float(x - LD(y))) / h.scale for h, l in zip(hi, lo) for x, y in zip(h.members, l.members))
    print("%s: members %s, ld_diff %.3g" % (ch.MANY.name, members, worst))
    assert worst <= ch.MANY.ld_diff and len(p.gps) == 128 and p.M == 8


def test_the_cases_reach_what_they_are_there_for():
    # M = 2: 29 panels, 232 nodes; M = 8: 113 panels, 904 nodes
    for M, panels in ((2, 29), (8, 113)):
        L, bp = ch.breakpoints([LD(0.1 * j) for j in range(M)], [LD(1)] * M, LD(0.5), LD)
        assert len(bp) == 14 * M + 2 == panels + 1 and all(x <= y for x, y in zip(bp[:-1], bp[1:]))
    # the floor: candidate 0's objective 1 has variance exactly 0, and at least 14 breakpoints coincide
    p = ch.make_problem(ch.case(ch.FLOOR))
    for T in (LD, np.float64):
        m = ch.Member(p.gps[0], p.pending, T)
        mo = m.moments(p.points[0])
        assert mo[1][1] == 0 and not np.any(mo[1][2]) and not np.any(mo[1][3])
        a, b = ch.split(p.scal[0])
        s, tau, sg = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], T)
        assert float(sg[1]) == math.sqrt(er.MIN_VAR_GRAD_EI)
        L, bp = ch.breakpoints(s, tau, p.best[0][0], T)
        assert sum(1 for x in bp if x == L) >= 14 and T(p.best[0][0]) > L
    # the decades: tau_j spread over more than six decades at every candidate
    p = ch.make_problem(ch.case("m4_e1_d3_n20_decades"))
    m = ch.Member(p.gps[0], p.pending, np.float64)
    a, b = ch.split(p.scal[0])
    for x in p.points:
        mo = m.moments(x)
        s, tau, sg = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], np.float64)
        assert max(tau) / min(tau) > 1e5
    # below: g* <= L everywhere; above: g* beyond every s_j + 8 tau_j
    for name, above in (("m3_e1_d3_n20_below", False), ("m3_e1_d3_n20_above", True)):
        p = ch.make_problem(ch.case(name))
        m = ch.Member(p.gps[0], p.pending, np.float64)
        a, b = ch.split(p.scal[0])
        for x in p.points:
            mo = m.moments(x)
            s, tau, sg = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], np.float64)
            L, bp = ch.breakpoints(s, tau, p.best[0][0], np.float64)
            if above:
                assert all(p.best[0][0] > s[j] + 8.0 * tau[j] for j in range(3))
            else:
                assert p.best[0][0] < L


def test_the_edge_cases_reach_what_they_are_there_for():
    """the cases of tests/test_gpu_chebei_edges.py: M = 6 and 7 with their breakpoint and node counts, n on both sides of 128, a
    member of exact zeros beside a live one, and 64 pending points whose deciding ones sit at the indices P64_SLOTS names"""
    for name, M, breaks, nodes in ((ch.M6, 6, 86, 680), (ch.M7, 7, 100, 792)):
        c = ch.case(name)
        p = ch.make_problem(c)
        assert c.M == M == len(p.gps[0]) and len(p.gps) == c.E and nodes % 64 != 0
        m = ch.Member(p.gps[0], p.pending, np.float64)
        a, b = ch.split(p.scal[0])
        mo = m.moments(p.points[0])
        s, tau, sg = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], np.float64)
        L, bp = ch.breakpoints(s, tau, m.incumbent(p.scal[0], p.best[0][0]), np.float64)
        assert len(bp) == breaks and 8 * (len(bp) - 1) == nodes
    sizes = {len(g.X) for row in ch.make_problem(ch.case(ch.M7)).gps for g in row}
    assert min(sizes) < 128 < max(sizes)
    # the last, partly filled sweep (40 lanes at M = 6, 24 at M = 7): under an observed incumbent every one of its panels is clamped
    # to no width and it adds exact zeros; with g* above every s_j + 8 tau_j all its nodes have a weight and carry most of the value
    for name, live_last in ((ch.M6, False), (ch.M7, False), (ch.M6_ABOVE, True), (ch.M7_ABOVE, True)):
        c = ch.case(name)
        p = ch.make_problem(c)
        a, b = ch.split(p.scal[0])
        m = ch.Member(p.gps[0], p.pending, np.float64)
        shares = []
        for x in p.points:
            mo = m.moments(x)
            s, tau, sg = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], np.float64)
            g = m.incumbent(p.scal[0], p.best[0][0])
            L, bp = ch.breakpoints(s, tau, g, np.float64)
            lo, hi = np.array(bp[:-1]), np.array(bp[1:])
            half, mid = 0.5 * (hi - lo), 0.5 * (lo + hi)
            t = (mid[:, None] + half[:, None] * np.array(ch.GL8_X)[None, :]).ravel()
            wt = (half[:, None] * np.array(ch.GL8_W)[None, :]).ravel()
            first = (len(wt) // 64) * 64
            assert len(wt) - first == {6: 40, 7: 24}[c.M]
            if live_last:
                assert np.all(wt[first:] > 0.0) and all(g > s[j] + 8.0 * tau[j] for j in range(c.M))
                terms = wt * ch.integrand(t, s, tau, np.float64, False)[0]
                shares.append(float(terms[first:].sum() / terms.sum()))
            else:
                assert not np.any(wt[first:])
        if live_last:
            print("%s: the last sweep carries %.3g .. %.3g of the value" % (name, min(shares), max(shares)))
            assert min(shares) > 0.5
    # mixed: member 0's incumbent at or below L at every candidate, exact zeros in both arithmetics; member 1 is live and the
    # ensemble's value is its value halved
    c = ch.case(ch.MIXED)
    for T in (LD, np.float64):
        p, want = ch.expected(c, T)
        ms = ch.ensemble(p, T)
        a, b = ch.split(p.scal[0])
        for x, w in zip(p.points, want):
            mo = ms[0].moments(x)
            s, tau, sg = ch.scalarised_moments(a, b, [q[0] for q in mo], [q[1] for q in mo], T)
            assert T(p.best[0][0]) < ch.breakpoints(s, tau, p.best[0][0], T)[0]
            A0, g0 = ms[0].evaluate(x, p.scal[0], p.best[0][0])
            A1, g1 = ms[1].evaluate(x, p.scal[0], p.best[0][1])
            assert A0 == 0 and not np.any(g0) and A1 > 0 and np.any(g1)
            assert w.members[0] == 0 and w.value == w.members[1] / T(2) and np.array_equal(w.grad, g1 / T(2))
    # p64: the placements and their margins from the float64 outcomes; every incumbent above every outcome
    c = ch.case(ch.P64)
    p = ch.make_problem(c)
    assert p.pending.shape == (64, 3) and c.E == 2 and c.C == 2
    G = ch._float64_outcomes(p.gps, p.pending, p.scal[0])
    margins = []
    for e, rank, index in ch.P64_SLOTS:
        order = np.argsort(G[e])
        assert rank == 0 and int(order[0]) == index
        margins.append(G[e][order[1]] - G[e][order[0]])
        assert p.best[0][e] > max(G[e]) and float(ch.Member(p.gps[e], p.pending, np.float64).incumbent(p.scal[0], p.best[0][e])) == G[e][index]
    assert ch.P64_SLOTS[0][2] == 63 and 32 <= ch.P64_SLOTS[1][2] <= 62
    print("p64: member 0's lowest outcome at point %d, member 1's at point %d, leading their runners-up by %s" % (
        ch.P64_SLOTS[0][2], ch.P64_SLOTS[1][2], margins))
    assert min(margins) >= ch.P64_MARGIN


# ---- 5. the coefficients against central differences ----
@pytest.mark.parametrize("M", [2, 3, 8])
def test_the_coefficients_are_the_derivatives_of_the_value(M):
    rng = np.random.default_rng(500 + M)
    a = rng.uniform(0.3, 1.5, size=M)
    b = rng.uniform(-0.2, 0.2, size=M)
    mus = rng.uniform(-0.3, 0.3, size=M)
    var = rng.uniform(0.2, 1.0, size=M) ** 2
    g = float(np.max(a * mus + b)) + 0.1
    A, c = ch.value_at_moments(a, b, mus, var, g, LD)
    worst, h = 0.0, 1e-6
    for j in range(M):
        for k, arr in ((0, mus), (1, var)):
            up, dn = arr.copy(), arr.copy()
            up[j] += h
            dn[j] -= h
            hi = ch.value_at_moments(a, b, up if k == 0 else mus, up if k == 1 else var, g, LD, want_grad=False)[0]
            lo = ch.value_at_moments(a, b, dn if k == 0 else mus, dn if k == 1 else var, g, LD, want_grad=False)[0]
            fd = float((hi - lo) / LD(2 * h))
            worst = max(worst, abs(fd - float(c[2 * j + k])) / max(1e-3, abs(fd)))
    print("M = %d: A = %.6g, coefficients against central differences: the worst relative difference %.3g" % (M, float(A), worst))
    assert worst <= 1e-7


def test_the_gradient_is_the_derivative_of_the_value_along_x():
    c = ch.case("m3_e1_d3_n20_p2")
    p = ch.make_problem(c)
    m = ch.ensemble(p, LD)
    sc = ch.scales_of(p)
    x = p.points[1]
    r = ch.evaluate(m, x, p.scal[0], p.best[0], sc)
    worst, h = 0.0, 1e-6
    for k in range(len(x)):
        up, dn = x.copy(), x.copy()
        up[k] += h
        dn[k] -= h
        fd = float((ch.evaluate(m, up, p.scal[0], p.best[0], sc, False).value - ch.evaluate(m, dn, p.scal[0], p.best[0], sc, False).value) / LD(2 * h))
        worst = max(worst, abs(fd - float(r.grad[k])))
    print("gradient against central differences along x: %.3g (the gradient's largest entry %.3g)" % (worst, float(np.max(np.abs(r.grad)))))
    assert worst <= 1e-7 * max(1.0, float(np.max(np.abs(r.grad)))) and float(np.max(np.abs(r.grad))) > 1e-3


# ---- 6. the believed rule, every branch by hand ----
def test_every_branch_of_the_believed_rule():
    a, b = np.array([1.0, 2.0]), np.array([0.0, -1.0])
    # outcomes [M][p]: scalarised max(mu_1, 2 mu_2 - 1) = 0.5, 0.2, 1.0
    outcomes = [np.array([0.5, 0.2, 1.0]), np.array([0.5, 0.6, 1.0])]
    assert [float(v) for v in ch.scalarised_outcomes(a, b, outcomes, np.float64)] == [0.5, pytest.approx(0.2), 1.0]
    assert float(ch.incumbent(a, b, outcomes, 0.7, np.float64)) == pytest.approx(0.2)  # an outcome lowers it
    assert float(ch.incumbent(a, b, outcomes, 0.1, np.float64)) == 0.1                  # none does
    assert float(ch.incumbent(a, b, [], 0.7, np.float64)) == 0.7                         # no pending point
    bad = [np.array([np.nan, 0.4]), np.array([0.0, np.inf])]
    assert float(ch.incumbent(a, b, bad, 0.7, np.float64)) == 0.7                        # outcomes that are not finite are left out
    half = [np.array([np.nan, 0.4]), np.array([0.0, 0.2])]
    assert float(ch.incumbent(a, b, half, 0.7, np.float64)) == pytest.approx(0.4)
    # another scalarisation, another pending point: under (1, 2 | 0, -1) point 1 is the smallest, under (3, 0.1 | 0, 0) point 1 still,
    # under (0.1, 3 | 0, 0) point 0
    assert int(np.argmin(ch.scalarised_outcomes([0.1, 3.0], [0.0, 0.0], outcomes, np.float64))) == 0
    assert int(np.argmin(ch.scalarised_outcomes(a, b, outcomes, np.float64))) == 1
    # the three cases of the GPU tests reach their branches under both members
    want = {"believed_one": (True, False), "believed_none": (False, False), "believed_other": (True, True)}
    first = None
    for c in ch.BELIEVED:
        p = ch.make_problem(c)
        for T in (LD, np.float64):
            ms = ch.ensemble(p, T)
            lowered = tuple(bool(m.incumbent(p.scal[0], bst) < T(bst)) for m, bst in zip(ms, p.best[0]))
            assert lowered == want[c.kind], (c.name, lowered)
            sa, sb = ch.split(p.scal[0])
            G = ch.scalarised_outcomes(sa, sb, ms[0].outcomes, T)
            margins = [abs(float(g - T(p.best[0][0]))) for g in G]
            assert min(margins) > 1e-3
            if c.kind == "believed_one":
                first = int(np.argmin(G))
            elif c.kind == "believed_other":
                assert first is not None and int(np.argmin(G)) != first
        # the pending points move the value
        r1 = ch.evaluate(ch.ensemble(p, np.float64), p.points[0], p.scal[0], p.best[0], ch.scales_of(p), False)
        r0 = ch.evaluate(ch.ensemble(p, np.float64, pending=p.pending[:0]), p.points[0], p.scal[0], p.best[0], ch.scales_of(p), False)
        assert abs(float(r1.value - r0.value)) > 1e-6


# ---- 7. the refusals, in the header's order, before a handle is touched ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def _args(M=3, E=2, d=2, C_=3, p=0, q=1, steps=3, domain=0):
    R = max(q, 1)
    a = np.tile(np.concatenate([np.full(M if M > 0 else 1, 0.5), np.zeros(M if M > 0 else 1)]), (R, 1))
    return dict(gps=(C.c_void_p * max(E * max(M, 1), 1))(), M=M, E=E, scal=np.ascontiguousarray(a), best=np.full((R, max(E, 1)), 0.3),
                pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25), C=C_,
                out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _head(a, g):
    return (g("gps", a["gps"]), a["M"], a["E"], g("scal", _p(a["scal"])), g("best", _p(a["best"])))


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_chebyshev_mcmc(*(_head(a, g) + (g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], 1,
                                                     g("ei", _p(a["out"])), g("grad", _p(a["out"])), None, C.byref(err))))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_chebyshev_mcmc_multistart(*(_head(a, g) + (
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None, None, None, None,
        C.byref(err))))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_chebyshev_mcmc_suggest(*(_head(a, g) + (
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
            a = _args(M=M, E=0, C_=0, p=65)
            assert call(lib, a, err, gps=True, pts=True, scal=True) == B and _payload(err) == (float(M), 2.0, 8.0), (call.__name__, M)
        # then E M > 1024 (and E < 1): payload (num_mcmc, 1, 1024 // M)
        for M, E in ((8, 129), (2, 513), (3, 342), (5, 0)):
            a = _args(M=M, E=E, C_=0, p=65)
            a["scal"][0, 0] = math.nan
            assert call(lib, a, err, pts=True) == B and _payload(err) == (float(E), 1.0, float(1024 // M)), (call.__name__, M, E)
        # the limit itself is accepted as far as the NULL handle
        for M, E in ((8, 128), (2, 512), (3, 341)):
            assert call(lib, _args(M=M, E=E), err) == R and b"NULL GP handle" in err.message, (call.__name__, M, E)
        # then NULL arrays
        for name in ("gps", "scal", "best", "pts"):
            a = _args(C_=0, p=65)
            a["scal"][0, 0] = -1.0
            assert call(lib, a, err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # then the scalarisation: payload (the value, its flat index, 0)
        for k, bad in ((0, 0.0), (1, -0.5), (2, math.inf), (0, math.nan), (3, math.nan), (5, -math.inf)):
            a = _args(C_=0, p=65)
            a["scal"][0, k] = bad
            a["best"][0, 0] = math.nan
            assert call(lib, a, err) == V and b"scalarisation" in err.message and _payload(err)[1:] == (float(k), 0.0), (call.__name__, k)
            assert math.isnan(_payload(err)[0]) if math.isnan(bad) else _payload(err)[0] == bad
        # a b_j may be negative or zero
        a = _args()
        a["scal"][0, 3:] = (-2.0, 0.0, 1.0)
        assert call(lib, a, err) == R and b"NULL GP handle" in err.message
        # then the incumbents: payload (the value, its flat index, 1)
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
        # a domain other than tensor product, behind the pending points and before the handles
        assert call(lib, _args(domain=1, p=65), err, pend=True) == B
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
