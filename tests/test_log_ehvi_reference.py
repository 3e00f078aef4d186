"""CPU tests (-m "not gpu") of tests/log_ehvi_reference.py, the restatement tests/test_gpu_log_ehvi.py checks the device against: the
member's log strip sum and its four coefficients in long double against mpmath at 60 digits (the gradient by mpmath.diff of the log
of the plain strip sum; bound 1e-13 relative to max(1, |.|)), every case-shift qualified with float64 within 2.5e-11 of long double
(a quarter of the GPU bound, the margin tests/test_logcei1_reference.py keeps), exp of the value at shift 0 against
tests/cehvi_reference.py's plain value, the three constructions (1025 strips, the rho = 1 strip, the floor) and the stall problem."""
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
