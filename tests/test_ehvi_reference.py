"""CPU tests (-m "not gpu") of the two-objective expected hypervolume improvement: tests/ehvi_reference.py, the restatement
tests/test_gpu_ehvi.py checks the device against, is itself checked here -- the closed form against the DEFINITION (the mean
hypervolume gain over seeded normal draws, through the module's own pareto_front / hypervolume), the empty front against
tests/ei1_reference.py, float64 against long double, the gradient against central differences of the long-double value -- and every
case is QUALIFIED: at its checked candidates the value and the gradient are far above the device test's tolerance, emptying the front
or dropping the pending points moves the value by far more than that tolerance, and the front dominates some candidates' mean pairs
and not others, so that a device which returned zeros, ignored the front or ignored P could not pass.  A case that breaks a
condition fails; none is skipped.  Then the believed-front rule, the C ABI's refusals in the header's order without a device, and
pareto_front / hypervolume on hand-computed inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import ehvi_reference as hr
import ei1_reference as er
import kg1_reference as kr
from cornell_moe_amd import _lib, build as moe_build, expected_hypervolume_improvement as ehvi

LD = hr.LD
dp, ip = _lib.dp, _lib.ip

CASES = hr.CASES + [hr.BELIEVED] + hr.WIDE_CASES


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. the closed form against the definition ----
def _gain_by_area(front, ref, y):
    """hypervolume(front u {y}) - hypervolume(front) for draws y [n][2] as an area: the part of [y1, r1] x [y2, r2] under the
    staircase h(s) = min(r2, min{v_i : u_i <= s}), segment by segment"""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    edges = np.concatenate([[-np.inf], f[:, 0], [ref[0]]])
    heights = np.concatenate([[ref[1]], f[:, 1]])
    out = np.zeros(len(y))
    for i in range(len(heights)):
        lo = np.maximum(edges[i], y[:, 0])
        width = np.maximum(edges[i + 1] - lo, 0.0)
        out += width * np.maximum(heights[i] - y[:, 1], 0.0)
    return out


# (mu_1, sigma_1, mu_2, sigma_2): ahead of the fronts, beside them, and behind them with deviations wide enough that a gain is still
# drawn often (deep behind a front no draw in 4e5 gains anything and the estimate says nothing)
MOMENTS = [(0.1, 0.5, -0.2, 0.4), (-0.6, 0.3, 0.5, 0.8), (0.5, 0.6, 0.4, 0.7)]


@pytest.mark.parametrize("F", (0, 1, 3, 40))
def test_the_closed_form_is_the_expected_gain_in_hypervolume(F):
    rng = np.random.default_rng(100 + F)
    ref = hr.REF
    front = hr.random_front(rng, F, 0.1)
    hv0 = ehvi.hypervolume(front, ref)
    for mu1, s1, mu2, s2 in MOMENTS:
        y = np.stack([mu1 + s1 * rng.normal(size=400000), mu2 + s2 * rng.normal(size=400000)], axis=1)
        gain = _gain_by_area(front, ref, y)
        # the area form IS the module's hypervolume difference, draw by draw
        for j in range(200):
            by_definition = ehvi.hypervolume(np.vstack([front, y[j:j + 1]]), ref) - hv0
            assert abs(by_definition - gain[j]) <= 1e-12, (F, j)
        mean, se = float(np.mean(gain)), float(np.std(gain, ddof=1)) / math.sqrt(len(gain))
        for T in (LD, np.float64):
            closed = float(hr.strips(mu1, s1 * s1, mu2, s2 * s2, front, ref, T)[0])
            assert abs(closed - mean) <= 5.0 * se, (F, mu1, mu2, closed, mean, se)
        print("F = %d, mu (%.1f, %.1f): closed form %.6f, %d draws %.6f +- %.6f" % (F, mu1, mu2, closed, len(gain), mean, se))
        assert mean > 20 * se  # (the comparison is not vacuous)


@pytest.mark.parametrize("T", (LD, np.float64), ids=("long_double", "float64"))
def test_with_an_empty_front_a_member_is_the_product_of_two_expected_improvements(T):
    c = hr.case("e1_d3_n20_p3_f2")
    p = hr.make_problem(c)
    none = p.pending[:0]
    m = hr.Member(p.gps[0], p.ref, np.zeros((0, 2)), none, T)
    bases = [kr.Model(g.cov_type, g.hyper, g.X, g.y, g.noise, T) for g in p.gps[0]]
    for x in p.points:
        a, grad, _ = m.evaluate(x)
        e1 = er.evaluate_model(bases[0], bases[0], none, x, p.ref[0])
        e2 = er.evaluate_model(bases[1], bases[1], none, x, p.ref[1])
        assert a == e1.value * e2.value
        # (the same terms grouped differently: a handful of roundings at 2.2e-16)
        assert float(np.max(np.abs(grad - (e2.value * e1.grad + e1.value * e2.grad)))) <= 1e-14 * max(1.0, float(np.max(np.abs(grad))))


# ---- 2. float64 against long double; 3. the gradient ----
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_float64_agrees_with_long_double(case):
    p, want = hr.expected(case, LD)
    _, got = hr.expected(case, np.float64)
    worst = 0.0
    for w, g in zip(want, got):
        worst = max(worst, abs(float(g.value - w.value)) / w.scale,
                    float(np.max(np.abs(g.grad.astype(LD) - w.grad))) / w.scale,
                    max(abs(float(a - b)) for a, b in zip(g.members, w.members)) / w.scale)
    print("%s: float64 - long double %.2e scale (recorded %.2e)" % (case.name, worst, case.ld_diff))
    assert worst <= case.ld_diff  # (the case table's figure; the device test's bound is max(1e-10, 4 times it))
    assert 4.0 * case.ld_diff <= 1e-10


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_gradient_agrees_with_central_differences(case):
    p, want = hr.expected(case, LD)
    members = hr.ensemble(p, LD)
    h = 1e-6
    worst = 0.0
    for i in p.checked[:3]:
        x = p.points[i]
        for j in range(len(x)):
            hi, lo = x.copy(), x.copy()
            hi[j] += h
            lo[j] -= h
            fd = (hr.evaluate(members, hi).value - hr.evaluate(members, lo).value) / LD(hi[j] - lo[j])
            worst = max(worst, abs(float(fd - want[i].grad[j])))
    print("%s: gradient - central differences %.2e" % (case.name, worst))
    assert worst <= 1e-7


# ---- 4. every case qualified ----
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_every_case_is_qualified(case):
    p, want = hr.expected(case, LD)
    assert len(p.checked) >= 3 and len(p.front) == case.F and len(p.pending) == case.p
    members = hr.ensemble(p, LD)
    empty = hr.ensemble(p, LD, front=np.zeros((0, 2)))
    bare = hr.ensemble(p, LD, pending=p.pending[:0])
    dominated = []
    for i in p.checked:
        w, x = want[i], p.points[i]
        assert float(w.value) >= 1e-3 * w.scale, (case.name, i)
        assert float(np.max(np.abs(w.grad))) >= 1e-2, (case.name, i)
        if case.F:
            assert abs(float(hr.evaluate(empty, x).value - w.value)) >= 1e-3 * w.scale, (case.name, i)
        if case.p:
            assert abs(float(hr.evaluate(bare, x).value - w.value)) >= 1e-5 * w.scale, (case.name, i)
        dominated += [hr.dominated(m.front, float(mu[0]), float(mu[1])) for m, mu in zip(members, w.means)]
    # (with neither a front nor pending points there is nothing to dominate a candidate)
    if case.F or case.p:
        assert any(dominated) and not all(dominated), (case.name, dominated)


def test_the_wide_cases_reach_every_instantiation_of_the_gradient_kernel():
    from test_ei1_reference import padded_dim
    reached = {}
    for c in hr.CASES + hr.WIDE_CASES:
        reached.setdefault(padded_dim(c.d), set()).add(padded_dim(c.d) - c.d)
    assert set(reached) == {4, 8, 12, 16, 24, 32}
    assert {0, 1, 2, 3, 4} <= set().union(*reached.values())  # (the padded coordinates)
    for c in hr.WIDE_CASES:
        p = hr.make_problem(c)
        assert c.C == 8 and c.p == 3 and c.F >= 65 and len(p.checked) >= 4, c.name
    # past one 256-row stride at a padded dimension other than 4, and three strides in the wide ensemble, one GP below 128 rows
    assert any(c.E == 1 and padded_dim(c.d) == 24 and max(c.n[0]) + c.p > 256 for c in hr.WIDE_CASES)
    w = hr.case(hr.ENSEMBLE_WIDE)
    rows = sorted(n for row in w.n for n in row)
    assert w.E == 3 and padded_dim(w.d) == 24 and rows[0] < 128 and rows[-1] + w.p > 512 and any(256 < n <= 512 for n in rows)
    assert len({row for row in w.n}) == 3 and all(row[0] != row[1] for row in w.n)  # (the chains do not line up)


def test_the_ensemble_compacts_a_front_tail_that_spans_lane_chunks():
    """some member's believed-front log has a join in which at least 2 front points leave and at least 65 points behind them move
    (the device moves the tail 64 lanes at a time)"""
    p = hr.make_problem(hr.case(hr.ENSEMBLE))
    seen = []
    for m in hr.ensemble(p, np.float64):
        for j, (what, left) in enumerate(m.log):
            if what != "joined":
                continue
            before, _ = hr.believed_front(p.front, m.outcomes[:j], p.ref, np.float64)
            a = float(m.outcomes[j][0])
            lower = int(np.sum(before[:, 0] < a))
            seen.append((left, len(before) - lower - left))
    print("%s: (front points that leave, points behind them that move) per join %s" % (hr.ENSEMBLE, seen))
    assert any(left >= 2 and moved >= 65 for left, moved in seen), seen


# ---- 5. the believed-front rule ----
def test_the_three_branches_of_the_believed_front_rule_bind():
    for T in (LD, np.float64):
        p = hr.make_problem(hr.BELIEVED)
        m0, m1 = hr.ensemble(p, T)
        assert m0.log[0][0] == "joined" and m0.log[0][1] >= 1   # a front point leaves under member 0
        assert m1.log[1] == ("dominated", 0)                    # member 1 ignores its outcome of pending point 1
        assert m0.log[2] == ("outside", 0) and m1.log[2] == ("outside", 0)
        a, b = (float(v) for v in m0.outcomes[0])
        after, _ = hr.believed_front(p.front, m0.outcomes[:1], p.ref, T)  # (the front once pending point 0 alone has joined)
        after = np.asarray(after, dtype=np.float64)
        gone = [(u, v) for u, v in p.front if not any(u == fu and v == fv for fu, fv in after)]
        assert len(gone) == m0.log[0][1] and all(u - a >= 1e-3 and v - b >= 1e-3 for u, v in gone)
        assert any(fu == a and fv == b for fu, fv in after) and len(after) == len(p.front) + 1 - len(gone)
        a, b = (float(v) for v in m1.outcomes[1])
        assert any(a - u >= 1e-3 and b - v >= 1e-3 for u, v in p.front)
        assert float(m0.outcomes[2][0]) - p.ref[0] >= 1e-3 and float(m1.outcomes[2][0]) - p.ref[0] >= 1e-3
        # every other decision of the rule has a margin too: no believed outcome within 1e-3 of a front point's coordinates
        for m in (m0, m1):
            for a, b in m.outcomes[:2]:
                assert min(min(abs(float(a) - u), abs(float(b) - v)) for u, v in p.front) >= 1e-3
    # the rule itself on a hand-made front
    front = [(0.0, 3.0), (1.0, 2.0), (2.0, 1.0), (3.0, 0.0)]
    f, log = hr.believed_front(front, [(0.5, 0.5), (2.5, 2.5), (5.0, 0.0), (-1.0, 3.5), (0.5, 0.5)], (4.0, 4.0), np.float64)
    assert log == [("joined", 2), ("dominated", 0), ("outside", 0), ("joined", 0), ("dominated", 0)]
    assert np.array_equal(f, np.array([(-1.0, 3.5), (0.0, 3.0), (0.5, 0.5), (3.0, 0.0)]))


# ---- 7. pareto_front and hypervolume ----
def test_pareto_front_and_hypervolume_on_hand_computed_inputs():
    pts = [(1.0, 3.0), (2.0, 2.0), (3.0, 1.0), (2.5, 2.5), (1.0, 3.0), (2.0, 4.0), (1.0, 3.5), (0.5, 3.0)]
    # (1, 3) twice: one kept -- and then dropped, for (0.5, 3) ties its second objective with a better first; (1, 3.5) ties the first
    assert np.array_equal(ehvi.pareto_front(pts), np.array([(0.5, 3.0), (2.0, 2.0), (3.0, 1.0)]))
    assert np.array_equal(ehvi.pareto_front([(1.0, 3.0), (1.0, 2.0), (2.0, 2.0)]), np.array([(1.0, 2.0)]))
    # points on the reference boundary are not strictly inside
    assert np.array_equal(ehvi.pareto_front(pts, (3.0, 4.0)), np.array([(0.5, 3.0), (2.0, 2.0)]))
    assert ehvi.pareto_front([(1.0, 1.0)], (1.0, 2.0)).shape == (0, 2) and ehvi.pareto_front([]).shape == (0, 2)
    # the staircase (0.5, 3), (2, 2), (3, 1) inside (4, 4): 3.5 * 1 + 2 * 1 + 1 * 1
    assert ehvi.hypervolume(pts, (4.0, 4.0)) == 6.5
    assert ehvi.hypervolume([(1.0, 1.0)], (3.0, 2.0)) == 2.0 and ehvi.hypervolume([], (3.0, 2.0)) == 0.0
    assert ehvi.hypervolume([(3.0, 0.0), (0.0, 2.0)], (3.0, 2.0)) == 0.0  # on the boundary: nothing
    assert ehvi.hypervolume([(1.0, 1.0), (1.0, 1.0), (2.0, 1.5)], (3.0, 2.0)) == 2.0  # a tie and a dominated point add nothing


# ---- 6. the C ABI without a device ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


NEW = ("moe_ehvi_mcmc", "moe_ehvi_mcmc_multistart", "moe_ehvi_mcmc_suggest")


def test_the_new_symbols_are_exported(lib):
    import cornell_moe_amd
    from cornell_moe_amd import api
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name in ("ehvi_ensemble", "ehvi_multistart", "ehvi_suggest"):
        assert callable(getattr(api, name))
    for name in ("ExpectedHypervolumeImprovementMCMC", "multistart_expected_hypervolume_improvement_optimization", "pareto_front",
                 "hypervolume"):
        assert callable(getattr(ehvi, name))
    assert cornell_moe_amd.expected_hypervolume_improvement is ehvi


def _args(d=2, E=1, F=2, C_=3, p=0, q=1, steps=3, domain=0):
    """valid arguments that need no handle: the arrays of handles hold NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    front = np.array([(0.1 * i, 1.0 - 0.1 * i) for i in range(max(F, 1))], dtype=np.float64)
    return dict(gps=(C.c_void_p * max(E, 1))(), gps2=(C.c_void_p * max(E, 1))(), E=E, ref=np.array([200.0, 2.0]), front=front, F=F,
                pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25), C=C_,
                out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ehvi_mcmc(g("gps", a["gps"]), g("gps2", a["gps2"]), a["E"], g("ref", _p(a["ref"])), g("front", _p(a["front"])),
                             a["F"], g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], 1, g("ei", _p(a["out"])),
                             g("grad", _p(a["out"])), None, C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ehvi_mcmc_multistart(
        g("gps", a["gps"]), g("gps2", a["gps2"]), a["E"], g("ref", _p(a["ref"])), g("front", _p(a["front"])), a["F"],
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        g("point", _p(a["out"])), g("value", C.byref(a["val"])), g("found", C.byref(a["found"])), None, None, None, None, None, None,
        C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ehvi_mcmc_suggest(
        g("gps", a["gps"]), g("gps2", a["gps2"]), a["E"], g("ref", _p(a["ref"])), g("front", _p(a["front"])), a["F"],
        g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent,
        a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])), g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    for call in (_eval, _ascent, _suggest):
        # num_mcmc first, even with everything else wrong: two GPs per member, 512 members
        for E in (0, 513):
            a = _args(C_=0, p=65, F=961)
            a["E"] = E
            assert call(lib, a, err, gps=True, pts=True) == B and _payload(err) == (float(E), 1.0, 512.0), call.__name__
        # then NULL arrays, before the front's own checks and the counts
        for name in ("gps", "gps2", "ref", "pts", "front"):
            assert call(lib, _args(C_=0, p=65), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        a = _args(C_=0, p=65, F=961)
        a["ref"][0] = math.nan
        # then num_front outside 0 .. 960
        for F in (-1, 961):
            a["F"] = F
            assert call(lib, a, err) == B and _payload(err) == (float(F), 0.0, 960.0), call.__name__
        # then a reference point that is not finite
        for r, bad in ((0, math.nan), (1, math.inf), (1, -math.inf)):
            a = _args(C_=0, p=65)
            a["ref"][r] = bad
            a["front"][1, 0] = math.nan
            assert call(lib, a, err) == V and b"reference_point" in err.message and _payload(err)[1:] == (float(r), 0.0), call.__name__
        # then the front: not finite, not sorted, dominated, on or outside the reference point -- payload: the offending index
        for i, u, v in ((1, math.nan, 0.5), (2, 0.2, math.inf), (2, 0.05, 0.5), (2, 0.1, 0.5), (2, 0.3, 0.9), (2, 0.3, 0.95),
                        (3, 200.0, 0.1), (0, 0.0, 2.0), (0, 0.0, 3.0)):
            a = _args(C_=0, p=65, F=4)
            a["front"][i] = (u, v)
            assert call(lib, a, err) == V and b"front" in err.message and _payload(err) == (float(i), 0.0, 0.0), (call.__name__, i, u, v)
        # then num_points, before num_being_sampled; an empty front needs no array
        assert call(lib, _args(C_=0, p=65), err) == B and _payload(err)[:2] == (0.0, 1.0)
        assert call(lib, _args(C_=0, p=65, F=0), err, front=True) == B and _payload(err)[:2] == (0.0, 1.0)
        # then num_being_sampled outside 0 .. 64
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        # then points_being_sampled NULL with num_being_sampled > 0
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        # everything that needs no handle in order: the NULL handle is next
        for F in (0, 2, 960):
            assert call(lib, _args(p=2, F=F), err) == R and b"NULL GP handle" in err.message, (call.__name__, F)
        assert call(lib, _args(p=0, F=0), err, pend=True, front=True) == R and b"NULL GP handle" in err.message
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0, F=961), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # max_num_steps < 1 after the pending checks and before the domain type; not asked for without the ascent
        assert call(lib, _args(steps=0, domain=1, p=65), err) == B and _payload(err) == (65.0, 0.0, 64.0)
        assert call(lib, _args(steps=0, domain=1), err) == B and _payload(err)[:2] == (0.0, 1.0) and b"max_num_steps" in err.message
        assert call(lib, _args(steps=0, domain=1), err, ascent=0) == V and b"tensor-product" in err.message
        assert call(lib, _args(domain=1), err) == V and _payload(err)[0] == 1.0 and b"expected hypervolume improvement" in err.message
    # the batch: num_to_sample directly after num_being_sampled, before the NULL pending array, the steps and the domain
    for p, q, hi in ((0, 0, 65.0), (0, 66, 65.0), (3, 63, 62.0), (64, 2, 1.0)):
        assert _suggest(lib, _args(p=p, q=q, steps=0, domain=1), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
    assert _suggest(lib, _args(p=65, q=0), err) == B and _payload(err) == (65.0, 0.0, 64.0)
