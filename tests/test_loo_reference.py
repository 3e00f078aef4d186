"""CPU tests (-m "not gpu") of the leave-one-out objective's host restatement (tests/loo_reference.py) and of the new ABI symbols.

  * closed form against brute force ("delete row and column i, predict row i") on the problems of tests/test_gpu_loo.py: value,
    means and variances to 1e-12 relative.  The inputs (noise >= 1e-2, lengths in [0.3, 1], points in the unit cube) keep the
    restatement alone far inside that: it agrees to ~1e-17 in long double.
  * its gradient against central differences of its own value, g = 0, both kernels, to 1e-6 max(1, |.|).
  * the seeds of the sampler test have no decision inside the band the GPU test skips.
  * moe_ll_set_objective / moe_ll_get_objective / moe_ll_loo_predict are declared, bound and exported.
"""
import os
import subprocess

import numpy as np
import pytest

import hyper_mcmc_reference as hm
import loo_reference as R


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1, np.abs(want))))


@pytest.mark.parametrize("case", R.CASES + R.WIDE_CASES + [R.SE_DERIV_CASE], ids=R.case_id)
def test_closed_form_against_brute_force(case):
    r = R.reference(case)
    assert abs(r["value"] - r["bf_value"]) <= 1e-12 * max(1, abs(r["bf_value"]))
    assert _rel(r["mu"], r["bf_mu"]) <= 1e-12
    assert _rel(r["var"], r["bf_var"]) <= 1e-12
    assert np.all(r["var"] > 0)


@pytest.mark.parametrize("case", [c for c in R.CASES + R.WIDE_CASES if c[3] == 0 and c[1] <= 129], ids=R.case_id)
def test_gradient_against_central_differences(case):
    r = R.reference(case)
    h = r["hyper"].astype(np.longdouble)
    for k in range(h.size):
        step = np.longdouble(1e-7) * h[k]
        hp, hm_ = h.copy(), h.copy()
        hp[k] += step
        hm_[k] -= step
        fd = (R.closed_form(r["X"], r["y"], r["derivs"], hp, case[0], want_grad=False)[0]
              - R.closed_form(r["X"], r["y"], r["derivs"], hm_, case[0], want_grad=False)[0]) / (2 * step)
        assert abs(fd - r["grad"][k]) <= 1e-6 * max(1, abs(r["grad"][k])), (k, fd, r["grad"][k])


def test_the_wide_cases_leave_the_gradient_bound_alone():
    """tests/test_gpu_loo.py holds the device's gradient to 10 grad_gap(), a maximum over CASES alone (1.23e-13): the wide cases do
    not enter it, and each one's own float64-vs-long-double gap lies below it, so the bound asks no less of them than of CASES."""
    bound = R.grad_gap()
    assert 1.0e-14 < bound < 1.0e-12
    assert not set(R.WIDE_CASES) & set(R.CASES)
    for case in R.WIDE_CASES:
        r = R.reference(case)
        gap = _rel(r["grad64"].astype(np.longdouble), r["grad"])
        print("%s: float64 vs long double gradient %.3g (CASES: %.3g), largest component %.3g" % (
            R.case_id(case), gap, bound, float(np.max(np.abs(r["grad"])))))
        assert gap < bound, (case, gap, bound)
        assert np.max(np.abs(r["grad"])) > 1.0   # (a gradient that carries weight in every comparison)
    assert R.grad_gap() == bound


def test_singular_matrix_is_minus_infinity():
    X, y, derivs, hyper = R.make_problem((R.MATERN, 5, 3, 0))
    hyper[0, -1] = -2.0 * hyper[0, 0]   # a negative diagonal: the first pivot fails
    assert R.closed_form(X, y, derivs, hyper[0], R.MATERN)[0] == -np.inf


@pytest.mark.parametrize("case", R.MCMC_CASES, ids=lambda c: "g%d" % c[3])
def test_sampler_seeds_have_no_decision_inside_the_band(case):
    pb = R.mcmc_problem(case)
    want = hm.run_chain(pb["p0"], *pb["tables"], pb["table"], pb["lnpost"])
    assert np.all(np.isfinite(want["lnprob0"]))
    assert want["margin"].min() > 1e-8
    assert 0 < want["accepted"].sum() < want["accepted"].size   # both outcomes occur


def test_loo_symbols_declared_and_exported():
    from cornell_moe_amd import _lib
    L = _lib.load()
    names = ("moe_ll_set_objective", "moe_ll_get_objective", "moe_ll_loo_predict")
    for name in names:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    assert (_lib.LL_LOG_MARGINAL, _lib.LL_LEAVE_ONE_OUT) == (0, 1)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "moe_hip.h")).read()
    for name in names + ("#define MOE_LL_LOG_MARGINAL 0", "#define MOE_LL_LEAVE_ONE_OUT 1"):
        assert name in header
    lib = os.path.join(root, "cornell_moe_amd", "lib", "libmoe_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in names:
        assert name in exported


def test_objective_of_a_null_handle_and_bad_arguments():
    from cornell_moe_amd import _lib
    L = _lib.load()
    err = _lib.MoeError()
    assert L.moe_ll_get_objective(None) == _lib.LL_LOG_MARGINAL
    rc = L.moe_ll_set_objective(None, 1, err)
    assert rc != _lib.MOE_OK and err.code == rc
    rc = L.moe_ll_loo_predict(None, None, None, None, err)
    assert rc != _lib.MOE_OK and err.code == rc


def test_boundary_accepts_both_objectives_and_refuses_others():
    from cornell_moe_amd import GPP, api
    assert GPP._check_objective(GPP.LogLikelihoodTypes.log_marginal_likelihood) == 0
    assert GPP._check_objective(GPP.LogLikelihoodTypes.leave_one_out_log_likelihood) == 1
    with pytest.raises(api.OptimalLearningException):
        GPP._check_objective(2)
