"""CPU tests (-m "not gpu") of tests/ei1_reference.py, the checker of tests/test_gpu_ei1.py: the inputs are qualified (a case that
breaks a condition FAILS), the restatement's gradient is checked against central differences and its p = 0 value and gradient
against the plain-C oracle on the committed fixtures; the four new symbols are exported and refuse bad arguments in the stated order
with the stated payloads before a handle or the device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

import ei1_reference as er
from cornell_moe_amd import _lib, build as moe_build
from oracle import orc

LD = er.LD
dp, ip = _lib.dp, _lib.ip


def padded_dim(d):
    """the device's padded dimension (csrc/common.hpp): a multiple of 4 up to 16, of 8 beyond"""
    return 4 * ((d + 3) // 4) if d <= 16 else 8 * ((d + 7) // 8)


def wide_magnitudes(name, results, d, at_least=3):
    """the conditions on the wide cases' inputs beyond tests/ei1_reference.PROBLEMS': `results` are (value / scale, gradient) of the
    checked candidates in long double.  At `at_least` of them the value is >= 1e-3 scale and the gradient's largest entry >= 1e-2 (an
    absolute bound of 1e-10 scale means ten digits there, and a device that returned zeros fails); from d = 10 on, at one of them
    every one of the d gradient coordinates is >= 1e-6 in magnitude (a dropped coordinate exceeds the bound 1e4 times over)."""
    big = [i for i, (v, g) in enumerate(results) if abs(v) >= 1e-3 and float(np.max(np.abs(g))) >= 1e-2]
    smallest = max(float(np.min(np.abs(g))) for v, g in results)
    print("%s: %d of %d checked candidates have |value| >= 1e-3 scale and |gradient| >= 1e-2; the best candidate's smallest gradient "
          "coordinate is %.3g" % (name, len(big), len(results), smallest))
    assert len(big) >= at_least
    if d >= 10:
        assert all(len(g) == d for v, g in results) and smallest >= 1e-6


@pytest.mark.parametrize("p", er.WIDE_PROBLEMS, ids=lambda p: p.name)
def test_the_wide_inputs_are_well_conditioned(p):
    test_the_inputs_are_well_conditioned(p)
    want, _ = er.expected(p, LD)
    wide_magnitudes(p.name, [(float(want[i].value) / want[i].scale, want[i].grad) for i in p.checked], p.X.shape[1],
                    3 if len(p.points) > 3 else 2)
    if len(p.X) >= 256:
        assert p.best == float(np.median(p.y))


@pytest.mark.parametrize("p", er.PROBLEMS, ids=lambda p: p.name)
def test_the_inputs_are_well_conditioned(p):
    want, without = er.expected(p, LD)
    w64, _ = er.expected(p, np.float64)
    e_v = max(abs(float(want[i].value) - float(w64[i].value)) / want[i].scale for i in p.checked)
    e_g = max(float(np.max(np.abs(want[i].grad - w64[i].grad))) / max(1.0, float(np.max(np.abs(want[i].grad)))) for i in p.checked)
    sig = min(want[i].sigma for i in p.checked) / math.sqrt(p.hyper[0])
    moved = max(abs(float(want[i].value - without[i])) / want[i].scale for i in p.checked)
    cs = [want[i].c for i in p.checked]
    print("%s: float64 against long double %.3g scale in value, %.3g in gradient; min sigma / sqrt(alpha) %.3g; P moves EI by %.3g "
          "scale; c from %.2f to %.2f" % (p.name, e_v, e_g, sig, moved, min(cs), max(cs)))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11
    assert sig >= 0.05  # (the gradient divides by sigma)
    if len(p.pending):
        assert moved >= 1e-5  # (a device that ignored P fails a 1e-10 test)
    else:
        assert moved == 0.0
    if p.name == er.BPRIME:
        assert want[p.checked[0]].bprime < p.best - 1e-3 and p.best == float(p.y.max())


def test_the_cases_reach_every_path():
    names = [p.name for p in er.PROBLEMS]
    assert len(set(names)) == len(names) == 12 and er.BPRIME in names
    dims = {p.X.shape[1] for p in er.PROBLEMS}
    assert {6, 32} <= dims  # (the DP = 8 and DP = 32 gradient kernels)
    assert any(len(p.pending) == 0 and p.X.shape[1] == 6 for p in er.PROBLEMS) and any(len(p.pending) == 0 and p.X.shape[1] == 32 for p in er.PROBLEMS)
    assert max(len(p.pending) for p in er.PROBLEMS) == 64 and any(len(p.X) >= 128 for p in er.PROBLEMS)
    for p in er.PROBLEMS:  # candidate 0 lies within 0.05 of pending point 0
        if len(p.pending):
            assert 0 in p.checked and np.max(np.abs(p.pending[0] - p.points[0])) <= 0.05
    e = er.ENSEMBLE
    assert len(e["n"]) == 3 and min(e["n"]) < 128 <= max(e["n"]) and len(set(e["factors"])) == 3


def test_the_wide_cases_reach_every_path():
    names = [p.name for p in er.WIDE_PROBLEMS]
    assert len(set(names)) == len(names) and not set(names) & {p.name for p in er.PROBLEMS}
    for pending in (True, False):  # with and without pending points
        some = [p for p in er.WIDE_PROBLEMS if (len(p.pending) > 0) == pending]
        assert any(padded_dim(p.X.shape[1]) > p.X.shape[1] > 8 for p in some)  # (padded coordinates beyond DP = 8)
        assert any(len(p.X) + len(p.pending) > 256 for p in some)       # (a second trip of the gradient kernel's row loop)
    padded = {padded_dim(p.X.shape[1]) for p in er.WIDE_PROBLEMS}
    assert {12, 16, 24} <= padded
    rows = [len(p.X) for p in er.WIDE_PROBLEMS if len(p.pending)]
    assert any(256 < n <= 512 for n in rows) and any(512 < n <= 1024 for n in rows) and any(n > 1024 for n in rows)  # (K slices 64, 128, 192)
    for p in er.WIDE_PROBLEMS:
        if len(p.pending):
            assert 0 in p.checked and np.max(np.abs(p.pending[0] - p.points[0])) <= 0.05
    e = er.ENSEMBLE_WIDE
    assert e["d"] == 10 and min(e["n"]) < 256 < sorted(e["n"])[1] <= 512 < max(e["n"]) and len(set(e["factors"])) == 3


def test_the_wide_ensemble_is_well_conditioned():
    test_the_ensemble_is_well_conditioned(er.ENSEMBLE_WIDE)


def test_the_ensemble_is_well_conditioned(e=er.ENSEMBLE):
    ep = er.make_ensemble(e)
    want, w64 = er.ensemble_expected(ep, ep.pending, LD), er.ensemble_expected(ep, ep.pending, np.float64)
    without = er.ensemble_expected(ep, ep.pending[:0], LD)
    e_v = max(abs(float(a[0]) - float(b[0])) / a[2] for a, b in zip(want, w64))
    e_g = max(float(np.max(np.abs(a[1] - b[1]))) / max(1.0, float(np.max(np.abs(a[1])))) for a, b in zip(want, w64))
    moved = max(abs(float(a[0] - b[0])) / a[2] for a, b in zip(want, without))
    print("ensemble of 3: float64 against long double %.3g / %.3g; P moves EI by %.3g scale" % (e_v, e_g, moved))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11 and moved >= 1e-5
    if e is er.ENSEMBLE_WIDE:
        wide_magnitudes("the wide ensemble", [(float(a[0]) / a[2], a[1]) for a in want], e["d"])


@pytest.mark.parametrize("name", ["n20_d3_A12_p2_fid", "n40_d4_A64_p5_se", "n20_d6_p0", er.BPRIME, "n20_d13_p3_se"])
def test_the_gradient_is_the_central_difference_of_the_value(name):
    p = [q for q in er.PROBLEMS + er.WIDE_PROBLEMS if q.name == name][0]
    base = er.base_model(p, LD)
    h, worst = 1e-6, 0.0
    for i in p.checked[:3]:
        grad = er.evaluate(base, p.pending, p.points[i], p.best).grad
        for k in range(p.points.shape[1]):
            xp, xm = p.points[i].copy(), p.points[i].copy()
            xp[k] += h
            xm[k] -= h
            fd = (er.evaluate(base, p.pending, xp, p.best).value - er.evaluate(base, p.pending, xm, p.best).value) / LD(xp[k] - xm[k])
            worst = max(worst, abs(float(fd - grad[k])) / max(1.0, float(np.max(np.abs(grad)))))
    print("%s: gradient against central differences of the long-double value: %.3g (bound 1e-7)" % (name, worst))
    assert worst <= 1e-7


def test_without_pending_points_the_restatement_is_the_oracle(golden):
    """the fixture cases without derivative observations (a one-entry noise vector; c6, c8, c10, c11 among them), tests/test_oracle.py's
    bounds: 1e-12 in value and 1e-10 in gradient, relative to the reference's recorded figure"""
    cases, _ = golden
    seen = []
    for c in cases:
        i = c.inp
        if len(i["derivs"]) or len(np.ravel(i["noise"])) != 1:
            continue
        seen.append(c.name if hasattr(c, "name") else len(seen))
        gp = orc.OrcGP(int(i["cov_type"]), float(i["alpha"]), i["lengths"], i["X"], i["y"], i["noise"], [])
        base = er.kr.Model(int(i["cov_type"]), np.concatenate([[float(i["alpha"])], i["lengths"]]), i["X"], i["y"], i["noise"], LD)
        best = float(i["ei_best"])
        none = np.zeros((0, np.shape(i["X"])[1]))
        for pt in i["query"]:
            v, g = gp.ei_analytic(pt, best)
            r = er.evaluate(base, none, pt, best)
            assert abs(float(r.value) - v) <= 1e-12 * max(abs(v), 1e-6)
            assert np.abs(r.grad.astype(np.float64) - g).max() <= 1e-10 * max(np.abs(g).max(), 1e-6)
    print("fixture cases without derivative observations: %s" % seen)
    assert len(seen) >= 4


# ---- the C ABI without a device ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


NEW = ("moe_ei_analytic_mcmc", "moe_ei_analytic_mcmc_multistart", "moe_ei_analytic_mcmc_suggest", "moe_ei1_pass_size")


def test_the_new_symbols_are_exported(lib):
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    # a function of N alone, a multiple of 64 between 64 and 4096, the columns of a pass within 2^24 doubles
    assert lib.moe_ei1_pass_size(8) == 4096 and lib.moe_ei1_pass_size(4096) == 4096 and lib.moe_ei1_pass_size(5000) == 3328
    assert lib.moe_ei1_pass_size(1 << 20) == 64


def _args(d=2, E=1, C_=3, p=0, q=1, steps=3, domain=0):
    """valid arguments that need no handle: the array of handles holds NULL, so a call that passes every earlier check ends at the
    NULL handle (MOE_ERR_RUNTIME)"""
    a = dict(gps=(C.c_void_p * E)(), E=E, best=np.zeros(max(E, 1)), pend=np.full((max(p, 1), d), 0.5), p=p, pts=np.full((max(C_, 1), d), 0.25),
             C=C_, out=np.zeros(max(C_, 1) * (d + 1) + 64), bounds=np.array([[0.0, 1.0]] * d), q=q,
             gd=_lib.GdParams(1, steps, 1, 0, 0.7, 0.1, 0.5, 1e-8, domain), iout=np.zeros(64, dtype=np.int32), val=C.c_double(0.0),
             found=C.c_int(0))
    return a


def _p(x):
    return x.ctypes.data_as(dp)


def _eval(lib, a, err, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_analytic_mcmc(g("gps", a["gps"]), a["E"], g("best", _p(a["best"])), g("pend", _p(a["pend"])), a["p"],
                                    g("pts", _p(a["pts"])), a["C"], 1, g("ei", _p(a["out"])), g("grad", _p(a["out"])), C.byref(err))


def _ascent(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_analytic_mcmc_multistart(
        g("gps", a["gps"]), a["E"], g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("best", _p(a["best"])),
        g("pend", _p(a["pend"])), a["p"], g("pts", _p(a["pts"])), a["C"], ascent, g("point", _p(a["out"])), g("value", C.byref(a["val"])),
        g("found", C.byref(a["found"])), None, None, None, None, None, None, C.byref(err))


def _suggest(lib, a, err, ascent=1, **null):
    g = lambda k, v: None if null.get(k) else v  # noqa: E731
    return lib.moe_ei_analytic_mcmc_suggest(
        g("gps", a["gps"]), a["E"], g("gd", C.byref(a["gd"])), g("bounds", _p(a["bounds"])), g("best", _p(a["best"])),
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
            a = _args(C_=0, p=65)
            a["E"] = E
            assert call(lib, a, err, gps=True, pts=True) == B and _payload(err) == (float(E), 1.0, 1024.0), call.__name__
        # then NULL arrays, before the counts
        for name in ("gps", "best", "pts"):
            assert call(lib, _args(C_=0, p=65), err, **{name: True}) == R and b"NULL argument" in err.message, (call.__name__, name)
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
