"""CPU tests (-m "not gpu") of tests/gibbon_reference.py, the checker of tests/test_gpu_gibbon.py: the inputs are qualified (a case
that breaks a condition FAILS), the restatement's gradient is checked against central differences of its value, the formula against
first principles (the variance of a noisy observation given f >= m by quadrature; the batch term 1/2 log |R| against the sum of the
greedy brackets), var0 against tests/ei1_reference.py's variance bit for bit; the three new symbols are exported and refuse bad
arguments in the stated order with the stated payloads before a handle or the device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import ei1_deriv_reference as ed
import ei1_reference as er
import gibbon_reference as gr
from cornell_moe_amd import _lib, build as moe_build
from test_ei1_reference import padded_dim, wide_magnitudes

LD = gr.LD
dp, ip = _lib.dp, _lib.ip


@pytest.mark.parametrize("p", gr.PROBLEMS, ids=lambda p: p.name)
def test_the_inputs_are_well_conditioned(p):
    want, without, shifted = gr.expected(p, LD)
    w64 = gr.expected(p, np.float64)[0]
    every = range(len(p.points))
    e_v = max(abs(float(want[i].value) - float(w64[i].value)) / want[i].scale for i in every)
    e_g = max(float(np.max(np.abs(want[i].grad - w64[i].grad))) / want[i].scale for i in every)
    sig = min(want[i].sigma0 for i in every) / math.sqrt(p.hyper[0])
    g_lo, g_hi = min(want[i].gammas[0] for i in every), max(want[i].gammas[1] for i in every)
    moved = min(abs(float(want[i].value - without[i])) / want[i].scale for i in p.checked)
    by_m = min(abs(float(want[i].value - shifted[i])) / want[i].scale for i in p.checked)
    print("%s (K = %d): float64 against long double %.3g scale in value, %.3g in gradient; min sigma0 / sqrt(alpha) %.3g; gamma from "
          "%.2f to %.2f; P moves the value by >= %.3g scale, the min-values by >= %.3g" % (p.name, len(p.mins), e_v, e_g, sig, g_lo,
                                                                                            g_hi, moved, by_m))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11
    assert -6.0 <= g_lo and g_hi <= 40.0
    assert sig >= 0.05
    assert 0 in p.checked and len(p.checked) >= 2
    if len(p.pending):
        assert moved >= 1e-5  # (a device that ignored P fails a 1e-10 test)
    else:
        assert moved == 0.0 and all(want[i].bracket == 0.0 for i in every)
    assert by_m >= 1e-5  # (and so does one that ignored the min-values)
    if p.name == gr.NOISE_FREE:  # no tolerance rests on a floor
        assert p.noise[0] == 0.0
        for i in every:
            assert float(want[i].var0) >= 1e-4 * p.hyper[0] and float(want[i].varc) >= 1e-4 * p.hyper[0]
    if p.name == gr.NEGATIVE:
        assert g_lo < 0.0


@pytest.mark.parametrize("p", gr.WIDE_PROBLEMS, ids=lambda p: p.name)
def test_the_wide_inputs_are_well_conditioned(p):
    """two candidates, not three, have to carry a value and a gradient of size: a case may check as few as two (the condition
    above), and the 1e-5 movement by the min-values already fails a device whose terms vanish"""
    test_the_inputs_are_well_conditioned(p)
    want = gr.expected(p, LD)[0]
    wide_magnitudes(p.name, [(float(want[i].value) / want[i].scale, want[i].grad) for i in p.checked], p.X.shape[1], 2)


def test_the_wide_cases_reach_every_path():
    names = [p.name for p in gr.WIDE_PROBLEMS]
    assert len(set(names)) == len(names) and not set(names) & {p.name for p in gr.PROBLEMS}
    plain = {padded_dim(p.X.shape[1]) for p in gr.WIDE_PROBLEMS if not len(p.derivs)}
    deriv = {padded_dim(p.X.shape[1]) for p in gr.WIDE_PROBLEMS if len(p.derivs)}
    assert {16, 24} <= plain and 16 in deriv and any(p.X.shape[1] % 4 for p in gr.WIDE_PROBLEMS)
    assert {63, 65} <= {len(p.mins) for p in gr.WIDE_PROBLEMS}
    big = [p for p in gr.WIDE_PROBLEMS if len(p.mins) > 128]
    assert big and all(p.y.size > 256 and p.y.size % 64 and len(p.pending) for p in big)  # (five row trips, the last one partial)
    for p in gr.WIDE_PROBLEMS:
        assert len(p.pending) and np.max(np.abs(p.pending[0] - p.points[0])) <= 0.05
    p = [q for q in gr.WIDE_PROBLEMS if q.name == gr.WIDE_N300][0]
    low = p.X[np.argsort(p.y[:, 0])[:5]]
    assert np.max(np.abs(p.points - low)) <= 0.05
    ep, mins = gr.make_ensemble(er.ENSEMBLE_WIDE)
    assert [len(x) for x in ep.X] == [20, 300, 600] and ep.points.shape[1] == 10 and mins.shape == (3, gr.ENSEMBLE_K)


def test_the_cases_reach_every_path():
    names = [p.name for p in gr.PROBLEMS]
    assert len(set(names)) == len(names) == 16 and names[:12] == [q.name for q in er.PROBLEMS]
    assert {len(p.mins) for p in gr.PROBLEMS} == {1, 63, 64, 65, 1024}
    assert {6, 32} <= {p.X.shape[1] for p in gr.PROBLEMS}
    assert any(len(p.pending) == 0 and p.X.shape[1] == 6 for p in gr.PROBLEMS) and any(len(p.pending) == 0 and p.X.shape[1] == 32 for p in gr.PROBLEMS)
    for p in gr.PROBLEMS:  # candidate 0 lies within 0.05 of pending point 0 (0.09 in the noise-free case: no floor in reach)
        if len(p.pending):
            assert np.max(np.abs(p.pending[0] - p.points[0])) <= (0.09 if p.name == gr.NOISE_FREE else 0.05)
    by_name = {p.name: p for p in gr.PROBLEMS}
    g2, big = by_name[gr.G2], by_name[gr.ROWS141]
    assert len(g2.derivs) == 2 and len(big.X) * (1 + len(big.derivs)) == 132 and len(big.pending) * (1 + len(big.derivs)) == 9
    ep, mins = gr.make_ensemble()
    assert [len(x) for x in ep.X] == [12, 130, 40] and mins.shape == (3, gr.ENSEMBLE_K)


def test_the_wide_ensemble_is_well_conditioned():
    test_the_ensemble_is_well_conditioned(er.ENSEMBLE_WIDE)


def test_the_ensemble_is_well_conditioned(e=er.ENSEMBLE):
    ep, mins = gr.make_ensemble(e)
    want, w64 = gr.ensemble_expected(ep, mins, ep.pending, LD), gr.ensemble_expected(ep, mins, ep.pending, np.float64)
    without = gr.ensemble_expected(ep, mins, ep.pending[:0], LD)
    e_v = max(abs(float(a[0]) - float(b[0])) / a[2] for a, b in zip(want, w64))
    e_g = max(float(np.max(np.abs(a[1] - b[1]))) / a[2] for a, b in zip(want, w64))
    moved = max(abs(float(a[0] - b[0])) / a[2] for a, b in zip(want, without))
    print("ensemble of 3: float64 against long double %.3g / %.3g; P moves the value by %.3g scale" % (e_v, e_g, moved))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11 and moved >= 1e-5
    if e is er.ENSEMBLE_WIDE:
        wide_magnitudes("the wide ensemble", [(float(a[0]) / a[2], a[1]) for a in want], e["d"])


@pytest.mark.parametrize("name", ["n20_d3_A12_p2_fid", "n40_d4_A64_p5_se", "n20_d6_p0", gr.NEGATIVE, gr.G2, gr.NOISE_FREE,
                                  "n10_d13_D0_12_p2"])
def test_the_gradient_is_the_central_difference_of_the_value(name):
    p = [q for q in gr.PROBLEMS + gr.WIDE_PROBLEMS if q.name == name][0]
    base = gr.base_model(p, LD)
    model = gr.conditioned(base, p.pending)
    h, worst = 1e-6, 0.0
    for i in p.checked[:3]:
        grad = gr.evaluate(base, model, p.points[i], p.mins).grad
        for k in range(p.points.shape[1]):
            xp, xm = p.points[i].copy(), p.points[i].copy()
            xp[k] += h
            xm[k] -= h
            fd = (gr.evaluate(base, model, xp, p.mins).value - gr.evaluate(base, model, xm, p.mins).value) / LD(xp[k] - xm[k])
            worst = max(worst, abs(float(fd - grad[k])) / max(1.0, float(np.max(np.abs(grad)))))
    print("%s: gradient against central differences of the long-double value: %.3g (bound 1e-7)" % (name, worst))
    assert worst <= 1e-7


@pytest.mark.parametrize("rho2", [1.0, 0.8])
@pytest.mark.parametrize("gamma", [-2.0, 0.0, 1.5])
def test_one_minus_rho2_q_is_the_variance_of_the_noisy_observation_given_f_above_m(gamma, rho2):
    """f ~ N(mu, s0), y = f + eps, eps ~ N(0, sigma^2) independent of f: Var(y | f >= m) = Var(f | f >= m) + sigma^2, the first term
    by the trapezoid rule on 400001 points of [m, mu + 14 sigma0] (the tail beyond carries < 1e-40 of the mass)"""
    mu, s0 = 0.3, 0.7
    sigma0 = math.sqrt(s0)
    noise = s0 * (1.0 - rho2) / rho2
    m = mu - gamma * sigma0
    f = np.linspace(LD(m), LD(mu + 14.0 * sigma0), 400001)
    w = np.exp(-(f - LD(mu)) ** 2 / (LD(2) * LD(s0)))
    w[0], w[-1] = w[0] / 2, w[-1] / 2
    mass = np.sum(w)
    mean = np.sum(w * f) / mass
    var_f = np.sum(w * (f - mean) ** 2) / mass
    got = float((var_f + LD(noise)) / (LD(s0) + LD(noise)))
    for T in (LD, np.float64):
        _, q = gr.ratio(np.array([gamma]), T)
        want = 1.0 - rho2 * float(q[0])
        assert abs(got - want) <= 1e-6, (gamma, rho2, T, got, want)
    print("gamma %.1f, rho^2 %.1f: Var(y | f >= m) / Var(y) = %.9f by quadrature, 1 - rho^2 q = %.9f" % (gamma, rho2, got, want))


def test_the_greedy_brackets_add_up_to_half_the_log_determinant_of_the_batch_correlation():
    p = [q for q in gr.PROBLEMS if q.name == "n20_d6_p0"][0]
    base = gr.base_model(p, LD)
    picks = p.points[:3].copy()
    picks[1] = picks[0] + 0.04  # (two picks close to each other: a determinant well below 1)
    total = LD(0)
    for t in range(3):
        r = gr.evaluate(base, gr.conditioned(base, picks[:t]), picks[t], p.mins)
        var_c, var_0 = r.varc + LD(base.noise), r.var0 + LD(base.noise)
        inc = (np.log(var_c) - np.log(var_0)) / LD(2)
        assert t == 0 and r.bracket == 0.0 or abs(r.bracket - float(inc)) <= 1e-15 * max(1.0, abs(float(inc)))
        total = total + inc
    k = base.cov(base.X, picks)
    V = base.fwd(k)
    S = base.cov(picks, picks) - V.T @ V + LD(base.noise) * np.eye(3, dtype=LD)
    s = np.sqrt(np.diag(S))
    R = S / s[:, None] / s[None, :]
    det = (R[0, 0] * (R[1, 1] * R[2, 2] - R[1, 2] * R[2, 1]) - R[0, 1] * (R[1, 0] * R[2, 2] - R[1, 2] * R[2, 0])
           + R[0, 2] * (R[1, 0] * R[2, 1] - R[1, 1] * R[2, 0]))
    want = np.log(det) / LD(2)
    print("sum of the greedy brackets %.15g, 1/2 log |R| %.15g" % (float(total), float(want)))
    assert float(want) < -0.05 and abs(float(total - want)) <= 1e-12


@pytest.mark.parametrize("T", [LD, np.float64], ids=["long double", "float64"])
def test_without_pending_points_var0_is_the_variance_of_the_expected_improvement_bit_for_bit(T):
    tiny = T(gr.TINY)
    for p in gr.PROBLEMS:
        base = gr.base_model(p, T)
        ref = ed if len(p.derivs) else er
        for i in (0, len(p.points) - 1):
            r = gr.evaluate(base, base, p.points[i], p.mins)
            ei = ref.evaluate(base, p.pending[:0], p.points[i], 0.0)
            assert float(np.sqrt(max(tiny, r.var0))) == ei.sigma and r.varc == r.var0 and r.bracket == 0.0, (p.name, i)


# ---- the C ABI without a device ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


NEW = ("moe_gibbon_mcmc", "moe_gibbon_mcmc_multistart", "moe_gibbon_mcmc_suggest")


def test_the_new_symbols_are_exported(lib):
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def _args(d=2, E=1, C_=3, p=0, q=1, steps=3, domain=0, K=4):
    """valid arguments that need no handle: the array of handles holds NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    return dict(gps=(C.c_void_p * max(E, 1))(), E=E, mins=np.full((max(E, 1), max(K, 1)), -1.5), K=K, pend=np.full((max(p, 1), d), 0.5), p=p,
                pts=np.full((max(C_, 1), d), 0.25), C=C_, out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
                gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
                found=C.c_int(0))


def _p(x):
    return x.ctypes.data_as(dp)


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_gibbon_mcmc(g("gps", a["gps"]), a["E"], g("mins", _p(a["mins"])), a["K"], g("pend", _p(a["pend"])), a["p"],
                               g("pts", _p(a["pts"])), a["C"], 1, g("ei", _p(a["out"])), g("grad", _p(a["out"])), C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_gibbon_mcmc_multistart(
        g("gps", a["gps"]), a["E"], g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("mins", _p(a["mins"])), a["K"],
        g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent, g("point", _p(a["out"])), g("value", C.byref(a["val"])),
        g("found", C.byref(a["found"])), None, None, None, None, None, None, C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_gibbon_mcmc_suggest(
        g("gps", a["gps"]), a["E"], g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("mins", _p(a["mins"])), a["K"],
        g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent, a["q"], g("point", _p(a["out"])), g("value", _p(a["out"])),
        g("found", a["iout"].ctypes.data_as(ip)), C.byref(err))


def _payload(err):
    return tuple(err.payload)


def test_bad_arguments_are_refused_in_order_before_a_handle_is_touched(lib):
    err = _lib.MoeError()
    B, R, V = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME, _lib.MOE_ERR_INVALID_VALUE
    for call in (_eval, _ascent, _suggest):
        # num_mcmc first, even with everything else wrong
        for E in (0, 1025):
            a = _args(C_=0, p=65, K=0)
            a["E"] = E
            assert call(lib, a, err, gps=True, pts=True) == B and _payload(err) == (float(E), 1.0, 1024.0), call.__name__
        # then NULL arrays, before the counts
        for name in ("gps", "mins", "pts"):
            assert call(lib, _args(C_=0, p=65, K=0), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # then num_min_values outside 1 .. 1024, before num_points
        for K in (0, -3, 1025):
            assert call(lib, _args(C_=0, p=65, K=K), err) == B and _payload(err) == (float(K), 1.0, 1024.0), (call.__name__, K)
        # then a min-value that is not finite: payload (the value, member, index)
        for bad in (np.inf, -np.inf, np.nan):
            a = _args(E=2, C_=0, p=65, K=5)
            a["mins"][1, 3] = bad
            assert call(lib, a, err) == V and _payload(err)[1:] == (1.0, 3.0), (call.__name__, bad)
            assert _payload(err)[0] == bad or (np.isnan(bad) and np.isnan(_payload(err)[0]))
        a = _args(C_=0, p=65, K=1024)
        a["mins"][0, 1023] = np.inf  # (the last of 1024 is read: the count is accepted)
        assert call(lib, a, err) == V and _payload(err)[1:] == (0.0, 1023.0)
        # then num_points, before num_being_sampled
        assert call(lib, _args(C_=0, p=65), err) == B and _payload(err)[:2] == (0.0, 1.0)
        # then num_being_sampled outside 0 .. 64
        for p in (-1, 65):
            assert call(lib, _args(p=p), err, pend=True) == B and _payload(err) == (float(p), 0.0, 64.0), call.__name__
        # then points_being_sampled NULL with num_being_sampled > 0
        assert call(lib, _args(p=2), err, pend=True) == R and b"points_being_sampled" in err.message
        # everything that needs no handle in order: the NULL handle is next
        assert call(lib, _args(p=2), err) == R and b"NULL" in err.message and b"points_being_sampled" not in err.message
        assert call(lib, _args(p=0), err, pend=True) == R and b"points_being_sampled" not in err.message  # (p = 0: NULL is fine)
    assert _eval(lib, _args(), err, ei=True) == R and _eval(lib, _args(), err, grad=True) == R
    for call in (_ascent, _suggest):
        for name in ("gd", "bounds", "point", "value", "found"):
            assert call(lib, _args(C_=0), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
        # max_num_steps < 1 after the pending checks and before the domain type; not asked for without the ascent
        assert call(lib, _args(steps=0, domain=1, p=65), err) == B and _payload(err) == (65.0, 0.0, 64.0)
        assert call(lib, _args(steps=0, domain=1), err) == B and _payload(err)[:2] == (0.0, 1.0) and b"max_num_steps" in err.message
        assert call(lib, _args(steps=0, domain=1), err, ascent=0) == V and b"tensor-product" in err.message
        assert call(lib, _args(domain=1), err) == V and _payload(err)[0] == 1.0
    # the batch: num_to_sample directly after num_being_sampled, before the NULL pending array, the steps and the domain
    for p, q, hi in ((0, 0, 65.0), (0, 66, 65.0), (3, 63, 62.0), (64, 2, 1.0)):
        assert _suggest(lib, _args(p=p, q=q, steps=0, domain=1), err, pend=True) == B and _payload(err) == (float(q), 1.0, hi), (p, q)
    assert _suggest(lib, _args(p=65, q=0), err) == B and _payload(err) == (65.0, 0.0, 64.0)
    assert _suggest(lib, _args(p=3, q=62), err) == R and b"NULL" in err.message  # (p + q - 1 = 64 is accepted: the NULL handle is next)
