"""CPU tests of the checker of the discretised one-point knowledge gradient (tests/kg1_reference.py) and of the new entry point's
argument checks: the closed form against a fixed antithetic sample, its gradient against central differences of the long-double
value, its lines against the plain-C oracle GP conditioned on a fantasy, the float64 restatement against the long-double one on
every case of tests/test_gpu_kg1.py, and moe_gp_kg_discrete's refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import kg1_reference as kr
import sampling_reference as sr
from cornell_moe_amd import _lib, build as moe_build

SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
LD = kr.LD


def _small(seed, n, d, A, cov_type=MATERN, noise=1e-2, nf=0, C_=3):
    return kr.Case("small%d" % seed, seed, n, d, A, cov_type, noise, nf, C_)


def test_erfc_of_the_checker_matches_the_library():
    for x in (0.0, 1e-3, 0.5, 1.0, 2.0, 2.4999, 2.5, 3.0, 6.0, 12.0, 26.0):
        got, want = float(kr._erfc_nonneg(x, LD)), math.erfc(x)
        assert abs(got - want) <= 4e-16 * want, (x, got, want)
    assert kr._erfc_nonneg(np.inf, LD) == 0
    assert float(kr.normal_cdf_diff(LD(-np.inf), LD(np.inf), LD)) == 1.0


# seeds fixed; pairs (z, -z) are the unit of the standard error
@pytest.mark.parametrize("case", [_small(11, 5, 2, 1), _small(12, 20, 3, 63, nf=1), _small(13, 5, 2, 255, cov_type=SE),
                                  _small(14, 40, 4, 300, nf=1), _small(15, 8, 2, 2000, noise=1e-3)], ids=lambda c: c.name)
def test_value_against_an_antithetic_sample(case):
    p = kr.make_problem(case)
    dset = kr.DiscreteSet(kr.Model(case.cov_type, p.hyper, p.X, p.y, p.noise, LD), p.discrete, case.nf)
    z = np.random.default_rng(424242).normal(size=100000)
    for i in range(case.C):
        want = kr.evaluate(dset, p.points[i], p.best, want_grad=False)
        a, b = want.a.astype(np.float64), want.b.astype(np.float64)
        pair = np.zeros(z.size)
        for lo in range(0, z.size, 20000):
            zz = z[lo:lo + 20000]
            pair[lo:lo + 20000] = 0.5 * ((a[:, None] + b[:, None] * zz[None, :]).min(axis=0) +
                                         (a[:, None] - b[:, None] * zz[None, :]).min(axis=0))
        mc, se = pair.mean(), pair.std(ddof=1) / math.sqrt(pair.size)
        print("%s[%d]: E[min] %.12g, sample %.12g +- %.3g, %d lines on the envelope" % (case.name, i, float(want.emin), mc, se,
                                                                                      want.num_active))
        # (1e-14: the rounding of the double sample itself, where one line takes every draw and the pairs cancel to the last bit)
        assert abs(float(want.emin) - mc) <= 5 * se + 1e-14, (case.name, i, float(want.emin), mc, se)
        assert float(want.emin) <= float(want.a.min()) + 1e-15  # (Jensen: the expected minimum is below the minimum of the intercepts)


GRAD_CASES = [_small(21, 5, 2, 1), _small(22, 20, 3, 63, nf=1), _small(23, 30, 4, 64, cov_type=SE), _small(24, 40, 8, 300, nf=1),
              _small(29, 8, 2, 400, noise=1e-3, C_=8), _small(26, 60, 6, 200)]


@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: c.name)
def test_gradient_against_central_differences(case):
    """on candidates whose decision margins are >= 1e-4, with best_so_far on either side of mu_n(x^)"""
    p = kr.make_problem(case)
    dset = kr.DiscreteSet(kr.Model(case.cov_type, p.hyper, p.X, p.y, p.noise, LD), p.discrete, case.nf)
    checked = 0
    for i in range(case.C):
        x = p.points[i]
        mu = float(kr.lines(dset, x)[0][0])
        for best in (mu - 0.3, mu + 0.3):
            want = kr.evaluate(dset, x, best)
            if min(want.margins) < 1e-4:
                continue
            fd = np.zeros(case.d, dtype=LD)
            for k in range(case.d):
                xp, xm = x.copy(), x.copy()
                xp[k] += 1e-6
                xm[k] -= 1e-6
                up = kr.evaluate(dset, xp, best, want_grad=False)
                dn = kr.evaluate(dset, xm, best, want_grad=False)
                fd[k] = (up.value - dn.value) / (LD(xp[k]) - LD(xm[k]))
            err = float(np.max(np.abs(want.grad - fd))) / max(1.0, float(np.max(np.abs(fd))))
            print("%s[%d] best %+.1f: gradient vs central differences %.3g, %d lines" % (case.name, i, best - mu, err, want.num_active))
            assert err <= 1e-7, (case.name, i, err)
            checked += 1
    assert checked >= 2, (case.name, checked)


@pytest.mark.parametrize("case", [_small(31, 12, 2, 6), _small(32, 25, 3, 6, nf=1), _small(33, 30, 4, 6, cov_type=SE)],
                         ids=lambda c: c.name)
def test_lines_are_the_reference_fantasy(case):
    """The oracle GP with (x, mu_n(x) + s zeta) appended under the GP's noise has the posterior mean a_z + b_z zeta at z.  The oracle
    takes the mean of its observed values as the constant prior mean, so the fantasy leaves that mean alone only where it equals
    it: zeta = (mean - mu_n(x)) / s, one zeta per candidate (asserted away from zero, so that the slope carries weight)."""
    from oracle import orc
    p = kr.make_problem(case)
    model = kr.Model(case.cov_type, p.hyper, p.X, p.y, p.noise, LD)
    dset = kr.DiscreteSet(model, p.discrete, case.nf)
    gp = orc.OrcGP(case.cov_type, p.hyper[0], p.hyper[1:], p.X, p.y, np.array(p.noise), [])
    worst = 0.0
    for i in range(case.C):
        x = p.points[i]
        a, b, s2, rest = kr.lines(dset, x)
        Z = rest[2]
        assert np.max(np.abs(gp.mean(Z) - a.astype(np.float64))) <= 1e-10  # a_z = mu_n(z), constant mean included
        mu_x = float(model.T(model.mean) + model.cov(model.X, x[None, :])[:, 0] @ model.kinvy)
        s = float(np.sqrt(s2))
        zeta = (model.mean - mu_x) / s
        assert abs(zeta) >= 0.05, zeta
        fantasy = orc.OrcGP(case.cov_type, p.hyper[0], p.hyper[1:], np.vstack([p.X, x[None, :]]),
                            np.vstack([p.y, [[mu_x + s * zeta]]]), np.array(p.noise), [])
        assert abs(fantasy.dump()[2] - model.mean) <= 1e-14
        err = float(np.max(np.abs(fantasy.mean(Z) - (a + b * LD(zeta)).astype(np.float64))))
        worst = max(worst, err)
        assert err <= 1e-10, (case.name, i, err)
    print("%s: posterior mean of the fantasised oracle GP vs a + b zeta: %.3g" % (case.name, worst))


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_bad_arguments_are_refused_without_a_device(lib):
    """the limits that need no handle, in the documented order, before the handle is looked at"""
    assert hasattr(lib, "moe_gp_kg_discrete") and "moe_gp_kg_discrete" in _lib.SIGNATURES
    dp = _lib.dp
    err = _lib.MoeError()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(dp)

    def call(nf, A, C_):
        return lib.moe_gp_kg_discrete(None, nf, p, A, p, C_, 0.0, 1, p, p, None, C.byref(err))

    assert call(0, 4, 0) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 1e9)
    assert call(0, 0, 2) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 4095.0)
    assert call(0, 4096, 2) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (4096.0, 1.0, 4095.0) and b"4096 lines" in err.message
    assert call(-1, 4, 2) == _lib.MOE_ERR_BOUNDS and b"num_fidelity" in err.message
    assert call(0, 4095, 2) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert lib.moe_gp_kg_discrete(None, 0, p, 4, p, 2, 0.0, 1, p, p, None, None) == _lib.MOE_ERR_RUNTIME
    assert lib.moe_kg1_pass_size(300, 4095) == 1024 and lib.moe_kg1_pass_size(5, 255) == 4096
    assert lib.moe_kg1_pass_size(10 ** 6, 1) == 64


@pytest.mark.parametrize("case", kr.GPU_CASES, ids=lambda c: c.name)
def test_float64_restatement_on_the_gpu_cases(case):
    """the same formulas in plain float64 stay within 2.5e-11 scale of the long-double value -- a quarter of the bound the device
    is held to -- on every candidate tests/test_gpu_kg1.py checks; the active counts agree wherever the margins are >= 1e-7"""
    p, want = kr.expected(case, LD)
    _, got = kr.expected(case, np.float64)
    worst_v = worst_g = 0.0
    for i in p.checked:
        w, g = want[i], got[i]
        worst_v = max(worst_v, abs(float(g.value) - float(w.value)) / w.scale)
        worst_g = max(worst_g, float(np.max(np.abs(g.grad - w.grad))) / max(1.0, float(np.max(np.abs(w.grad)))))
        if w.margins[0] >= 1e-7:
            assert g.num_active == w.num_active and g.hull == w.hull
    print("%s: float64 vs long double: value %.3g scale, gradient %.3g; lines on the envelope %s; smallest margins %.3g / %.3g" % (
        case.name, worst_v, worst_g, sorted(set(want[i].num_active for i in p.checked)),
        min(want[i].margins[0] for i in p.checked), min(want[i].margins[1] for i in p.checked)))
    assert worst_v <= 2.5e-11
