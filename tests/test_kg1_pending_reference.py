"""CPU tests of the discretised one-point knowledge gradient with pending points (csrc/kg1_pending.hip: moe_kg_discrete_mcmc_pending,
moe_kg_discrete_mcmc_multistart_pending, moe_kg_discrete_mcmc_suggest): the restatement of tests/kg1_pending_reference.py against
Monte Carlo over a plain conditioned GP, against central differences and against itself under a permutation of P; the refusals that
need no device, in the order include/moe_hip.h documents; and the qualification of the inputs of tests/test_gpu_kg1_pending.py."""
import ctypes as C
import os

import numpy as np
import pytest

import kg1_pending_reference as kp
import kg1_reference as kr
from cornell_moe_amd import _lib, build as moe_build

LD = kr.LD
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moe_hip.h")
SMALL = [c for c in kp.GPU_CASES if c.A <= 129 and c.n <= 40]


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


# ---- the restatement ----
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_the_believed_values_leave_the_intercepts_unchanged_exactly(case):
    """K'^-1 (y' - mean) = [alpha ; 0]: a_A = mu_n(A) of the conditioned model is the base model's, bit for bit in long double (its
    dot products are plain loops, and the pending rows add exact zeros at their end)"""
    p = kp.make_problem(case)
    base, cond = kp.models(p, LD)
    a0, a1 = kr.DiscreteSet(base, p.discrete, case.nf).a, kr.DiscreteSet(cond, p.discrete, case.nf).a
    assert np.array_equal(a0, a1)
    for x in p.points[:3]:
        assert kr.lines(kr.DiscreteSet(cond, p.discrete, case.nf), x)[0][0] == kr.lines(kr.DiscreteSet(base, p.discrete, case.nf), x)[0][0]


def test_the_value_is_the_monte_carlo_knowledge_gradient_of_a_plain_conditioned_gp():
    """1e5 antithetic pairs from a GP with the rows X u P and the observations [y ; mu_n(P)], solved as one plain system in float64
    (no [alpha ; 0], no extension): the long-double value lies within 5 standard errors, plus 1e-10 scale for the float64 solves
    of the plain system (where one line carries the whole minimum the antithetic pairs cancel and the standard error is zero)"""
    case = [c for c in kp.GPU_CASES if c.name == "n20_d3_A12_p2_fid"][0]
    p, want, _ = kp.expected(case)
    f8 = np.float64
    hyper = np.asarray(p.hyper)

    def cov(A, B):
        return kr.covariance(case.cov_type, hyper[0], hyper[1:], A, B, f8)

    mean = kr.Model(case.cov_type, p.hyper, p.X, p.y, p.noise, f8).mean
    yc = p.y.ravel() - mean
    K = cov(p.X, p.X) + p.noise[0] * np.eye(case.n)
    believed = cov(p.pending, p.X) @ np.linalg.solve(K, yc)  # mu_n(P) - mean
    Xc = np.vstack([p.X, p.pending])
    Kc = cov(Xc, Xc) + p.noise[0] * np.eye(case.n + case.p)
    wc = np.linalg.solve(Kc, np.concatenate([yc, believed]))
    rng = np.random.default_rng(123)
    assert max(want[i].num_active for i in p.checked) >= 2
    for i in p.checked:
        x = p.points[i]
        xh = x.copy()
        xh[case.d - case.nf:] = 1.0
        Z = np.vstack([xh[None, :], kr.pad(p.discrete, case.d, case.nf)])
        kz, kx = cov(Xc, Z), cov(Xc, x[None, :])[:, 0]
        sol = np.linalg.solve(Kc, kx)
        s = np.sqrt(hyper[0] - kx @ sol + p.noise[0])
        a = mean + kz.T @ wc
        b = (cov(Z, x[None, :])[:, 0] - kz.T @ sol) / s
        z = rng.standard_normal(100000)
        pair = 0.5 * (np.min(a[None, :] + z[:, None] * b[None, :], axis=1) + np.min(a[None, :] - z[:, None] * b[None, :], axis=1))
        est, se = min(p.best, a[0]) - pair.mean(), pair.std(ddof=1) / np.sqrt(pair.size)
        print("candidate %d (%d lines): long double %.9g, Monte Carlo %.9g +- %.2g" % (i, want[i].num_active, float(want[i].value), est, se))
        assert abs(float(want[i].value) - est) <= 5 * se + 1e-10 * want[i].scale


@pytest.mark.parametrize("name", ["n20_d3_A12_p2_fid", "n40_d4_A64_p5_se"])
def test_the_gradient_is_the_central_difference_of_the_long_double_value(name):
    case = [c for c in kp.GPU_CASES if c.name == name][0]
    p, want, _ = kp.expected(case)
    dset = kr.DiscreteSet(kp.models(p, LD)[1], p.discrete, case.nf)
    h, worst = 1e-6, 0.0
    for i in p.checked[:2]:
        num = np.zeros(case.d)
        for k in range(case.d):
            e = np.zeros(case.d)
            e[k] = h
            num[k] = float((kr.evaluate(dset, p.points[i] + e, p.best, want_grad=False).value -
                            kr.evaluate(dset, p.points[i] - e, p.best, want_grad=False).value) / LD(2 * h))
        g = want[i].grad.astype(np.float64)
        worst = max(worst, float(np.max(np.abs(num - g))) / max(1.0, float(np.max(np.abs(g)))))
    print("%s: gradient vs central differences %.3g (bound 1e-7)" % (name, worst))
    assert worst <= 1e-7


@pytest.mark.parametrize("name", ["n40_d4_A64_p5_se", "n12_d2_A129_p8"])
def test_a_permutation_of_the_pending_points_changes_nothing(name):
    case = [c for c in kp.GPU_CASES if c.name == name][0]
    p, want, _ = kp.expected(case)
    perm = np.random.default_rng(5).permutation(case.p)
    base = kp.models(p, LD)[0]
    dset = kr.DiscreteSet(kp.PendingModel(base, p.pending[perm]), p.discrete, case.nf)
    worst = max(abs(float(kr.evaluate(dset, p.points[i], p.best, want_grad=False).value - want[i].value)) / want[i].scale
                for i in p.checked)
    print("%s: permuted P moves the value by %.3g scale (bound 1e-12)" % (name, worst))
    assert worst <= 1e-12


# ---- the inputs of the GPU tests ----
@pytest.mark.parametrize("case", kp.GPU_CASES, ids=lambda c: c.name)
def test_every_gpu_case_qualifies(case):
    """the float64 restatement within 2.5e-11 scale of long double (value and gradient), every decision margin >= 1e-7 with no
    candidate left out, and P moves at least one checked candidate's value by >= 1e-4 scale"""
    p, want, without = kp.expected(case)
    _, got, _ = kp.expected(case, np.float64)
    e_v = max(abs(float(got[i].value) - float(want[i].value)) / want[i].scale for i in p.checked)
    e_g = max(float(np.max(np.abs(got[i].grad.astype(np.float64) - want[i].grad.astype(np.float64)))) /
              max(1.0, float(np.max(np.abs(want[i].grad)))) for i in p.checked)
    margin = min(min(want[i].margins) for i in p.checked)
    moved = max(abs(float(want[i].value - without[i])) / want[i].scale for i in p.checked)
    print("%s: float64 vs long double value %.3g scale, gradient %.3g; smallest margin %.3g; P moves KG by up to %.3g scale" % (
        case.name, e_v, e_g, margin, moved))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11
    assert margin >= 1e-7
    assert [got[i].num_active for i in p.checked] == [want[i].num_active for i in p.checked]
    assert moved >= 1e-4


def test_the_ensemble_case_qualifies():
    _ensemble_qualifies(kp.ENSEMBLE)


def test_the_wide_ensemble_case_qualifies():
    _ensemble_qualifies(kp.ENSEMBLE_WIDE)


def _ensemble_qualifies(spec):
    ep = kp.make_ensemble(spec)
    want, f8 = kp.ensemble_expected(ep, ep.pending, LD), kp.ensemble_expected(ep, ep.pending, np.float64)
    without = kp.ensemble_expected(ep, ep.pending[:0], LD)
    e_v = max(abs(float(a[0]) - float(b[0])) / b[2] for a, b in zip(f8, want))
    margin = min(w[3] for w in want)
    moved = max(abs(float(a[0] - b[0])) / a[2] for a, b in zip(want, without))
    print("ensemble: float64 vs long double %.3g scale; smallest margin %.3g; P moves the mean by up to %.3g scale" % (e_v, margin, moved))
    assert e_v <= 2.5e-11 and margin >= 1e-7 and moved >= 1e-4


# ---- the ABI without a device ----
def test_the_header_declares_the_symbols_and_the_library_has_them(lib):
    with open(HEADER) as f:
        text = f.read()
    for name in ("moe_kg_discrete_mcmc_pending", "moe_kg_discrete_mcmc_multistart_pending", "moe_kg_discrete_mcmc_suggest"):
        assert ("int %s(" % name) in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "Kriging-believer" in text


def _gd(steps=4, restarts=1, domain_type=0):
    g = _lib.GdParams()
    g.num_multistarts, g.max_num_steps, g.max_num_restarts, g.num_steps_averaged = 4, steps, restarts, 0
    g.gamma, g.pre_mult, g.max_relative_change, g.tolerance, g.domain_type = 0.7, 1.0, 0.5, 1e-10, domain_type
    return g


def test_the_evaluator_refuses_bad_arguments_without_a_device(lib):
    """in the order include/moe_hip.h documents; the handles are NULL and are looked at last"""
    dp, ip = _lib.dp, _lib.ip
    err = _lib.MoeError()
    buf = np.zeros(64 * 8)
    p = buf.ctypes.data_as(dp)
    gps = (C.c_void_p * 2)(None, None)

    def call(E=2, nf=0, counts=(4, 4), C_=2, pend=p, np_=3, disc=p):
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        return lib.moe_kg_discrete_mcmc_pending(gps, E, nf, disc, cnt.ctypes.data_as(ip), p, pend, np_, p, C_, 1, p, p, C.byref(err))

    assert call(E=0, np_=65) == _lib.MOE_ERR_BOUNDS and b"num_mcmc" in err.message
    assert call(disc=None, np_=65) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(counts=(4, 4096), np_=65) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (4096.0, 1.0, 4095.0)
    assert call(C_=0, np_=65) == _lib.MOE_ERR_BOUNDS and b"candidates" in err.message
    assert call(nf=-1, np_=65) == _lib.MOE_ERR_BOUNDS and b"num_fidelity" in err.message
    assert call(np_=65) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (65.0, 0.0, 64.0) and b"num_being_sampled" in err.message
    assert call(np_=-1) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (-1.0, 0.0, 64.0)
    assert call(pend=None) == _lib.MOE_ERR_RUNTIME and b"points_being_sampled is NULL" in err.message
    assert call(pend=None, np_=0) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message  # (no pending point: none is read)
    assert call(np_=64) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message


def test_the_optimiser_and_the_batch_refuse_bad_arguments_without_a_device(lib):
    dp, ip = _lib.dp, _lib.ip
    err = _lib.MoeError()
    buf = np.zeros(64 * 8)
    p = buf.ctypes.data_as(dp)
    gps = (C.c_void_p * 2)(None, None)
    value, found = C.c_double(0.0), C.c_int(0)
    founds = np.zeros(64, dtype=np.int32)
    cnt = np.ascontiguousarray([4, 4], dtype=np.int32)

    def ascent(nf=0, S=3, gd=_gd(), pend=p, np_=3):
        return lib.moe_kg_discrete_mcmc_multistart_pending(gps, 2, nf, C.byref(gd), p, p, cnt.ctypes.data_as(ip), p, pend, np_, p, S, 1,
                                                           p, C.byref(value), C.byref(found), None, None, None, None, None, None,
                                                           C.byref(err))

    def batch(nf=0, S=3, gd=_gd(), pend=p, np_=3, q=1, points=p):
        return lib.moe_kg_discrete_mcmc_suggest(gps, 2, nf, C.byref(gd), p, p, cnt.ctypes.data_as(ip), p, pend, np_, p, S, 1, q, points, p,
                                                founds.ctypes.data_as(ip), C.byref(err))

    for call in (ascent, batch):
        assert call(S=0, nf=-1, np_=65) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 1e9)
        assert call(nf=-1, np_=65) == _lib.MOE_ERR_BOUNDS and b"num_fidelity" in err.message
        assert call(np_=65, gd=_gd(steps=0)) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (65.0, 0.0, 64.0)
        assert call(pend=None, gd=_gd(steps=0)) == _lib.MOE_ERR_RUNTIME and b"points_being_sampled is NULL" in err.message
        assert call(gd=_gd(steps=0, domain_type=1)) == _lib.MOE_ERR_BOUNDS and b"max_num_steps" in err.message
        assert call(gd=_gd(domain_type=1)) == _lib.MOE_ERR_INVALID_VALUE and b"tensor-product" in err.message
        assert call() == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
        assert call(np_=64) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert batch(points=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert batch(q=0, pend=None) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 62.0) and b"num_to_sample" in err.message
    assert batch(np_=64, q=2) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (2.0, 1.0, 1.0)
    assert batch(np_=0, q=66, pend=None) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (66.0, 1.0, 65.0)
    assert batch(np_=64, q=1) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert batch(np_=0, q=65, pend=None) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
