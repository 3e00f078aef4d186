"""GPU tests (-m gpu) of the leave-one-out objective on the device (csrc/loo.hip behind moe_ll_*) against the host restatement
tests/loo_reference.py (long double; closed form and an independent brute force).

Shapes (loo_reference.CASES): N = n (1 + g) in {1, 2, 63, 64, 65, 129, 257}, (d, g) in {(1,0), (3,0), (5,0), (3,2), (12,3)}, both
kernels where g = 0; (loo_reference.WIDE_CASES): d in {13, 16, 17, 24, 25, 32} -- padded dimensions 16, 24, 32 at both ends of
each -- with N in {20, 30, 36, 70}, (d, g) = (25, 2) among them.  Tolerances: values, predictions and sampler log posteriors 1e-9 max(1, |want|), the project's own for
moe_ll_evaluate (tests/test_gpu_hyper_mcmc.py).  Gradient: see test_gradient_against_closed_form.
"""
import numpy as np
import pytest

import hyper_mcmc_reference as hm
import loo_reference as R
import ms_restatement as ms

pytestmark = pytest.mark.gpu

TOL = 1e-9
LOO, MARGINAL = 1, 0


def _api():
    from cornell_moe_amd import api
    return api


def _handle(case, objective=MARGINAL):
    r = R.reference(case)
    return r, _api().LogLikelihood(r["X"], r["y"], r["derivs"], cov_type=case[0], objective=objective)


def _close(got, want, tol=TOL):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    with np.errstate(invalid="ignore"):   # (infinities match exactly)
        return bool(np.all((got == want) | (np.abs(got - want) <= tol * np.maximum(1, np.abs(want)))))


@pytest.mark.parametrize("case", R.CASES + R.WIDE_CASES + [R.SE_DERIV_CASE], ids=R.case_id)
def test_value_one_set(case):
    r, ll = _handle(case, LOO)
    got = ll.evaluate(r["hyper"][None, :])
    print("value", R.case_id(case), got[0], float(r["value"]), float(abs(got[0] - r["value"]) / max(1, abs(r["value"]))))
    assert _close(got[0], r["value"])


@pytest.mark.parametrize("case", [(R.MATERN, 21, 3, 2), (R.SE, 65, 3, 0)], ids=R.case_id)
def test_value_65_sets_and_a_singular_one(case):
    """65 sets in one call cross the 64-set pass; a set whose noise makes K singular is -inf and leaves its neighbours alone."""
    X, y, derivs, hyper = R.make_problem(case, num_sets=65)
    hyper[37, -1] = -2.0 * hyper[37, 0]
    ll = _api().LogLikelihood(X, y, derivs, cov_type=case[0], objective=LOO)
    got = ll.evaluate(hyper)
    assert got[37] == -np.inf
    for k in (0, 1, 36, 38, 63, 64):
        want = R.closed_form(X, y, derivs, hyper[k], case[0], want_grad=False)[0]
        assert _close(got[k], want), (k, got[k], float(want))
    assert np.all(np.isfinite(np.delete(got, 37)))
    assert ll.evaluate(hyper[64:65])[0] == got[64]   # a set's value does not depend on the sets it shares a call with
    assert ll.evaluate(hyper[37:38])[0] == -np.inf


@pytest.mark.parametrize("case", R.CASES + R.WIDE_CASES + [R.SE_DERIV_CASE], ids=R.case_id)
def test_predictions_against_brute_force(case):
    r, ll = _handle(case)   # the handle's objective stays 0
    before = ll.evaluate(r["hyper"][None, :])[0]
    mean, var = ll.loo_predict(r["hyper"])
    print("predict", R.case_id(case), float(np.max(np.abs(mean - r["bf_mu"]) / np.maximum(1, np.abs(r["bf_mu"])))),
          float(np.max(np.abs(var - r["bf_var"]) / np.maximum(1, np.abs(r["bf_var"])))))
    assert mean.shape == var.shape == r["bf_mu"].shape
    assert _close(mean, r["bf_mu"]) and _close(var, r["bf_var"])
    assert ll.objective == MARGINAL
    after = ll.evaluate(r["hyper"][None, :])[0]
    _, fresh = _handle(case)
    assert before == after == fresh.evaluate(r["hyper"][None, :])[0]


def test_predict_singular():
    api = _api()
    r, ll = _handle((R.MATERN, 21, 3, 2))
    bad = r["hyper"].copy()
    bad[-1] = -2.0 * bad[0]
    with pytest.raises(api.SingularMatrixException):
        ll.loo_predict(bad)
    mean, _ = ll.loo_predict(r["hyper"])   # the handle stays usable
    assert _close(mean, r["bf_mu"])


GRAD_CASES = R.CASES + R.WIDE_CASES   # (the bound below stays that of R.CASES alone)


@pytest.mark.parametrize("case", GRAD_CASES, ids=R.case_id)
def test_gradient_against_closed_form(case):
    """moe_ll_grad under LOO against the restatement's gradient in long double.

    Bound: ten times the gap between the restatement run in float64 and in long double on these inputs (loo_reference.grad_gap(),
    the maximum over loo_reference.CASES of |g64 - gLD| / max(1, |gLD|)), because the device sums in another order.  Measured
    gap: 1.23e-13, so the bound is 1.23e-12 max(1, |want|); the test recomputes it.
    """
    r, ll = _handle(case, LOO)
    bound = 10.0 * R.grad_gap()
    assert 1.0e-13 < bound < 1.0e-11
    got = ll.grad(r["hyper"])
    err = float(np.max(np.abs(got - r["grad"]) / np.maximum(1, np.abs(r["grad"]))))
    print("grad", R.case_id(case), err, bound)
    assert err <= bound, (err, bound, got, r["grad"])


@pytest.mark.parametrize("case", [c for c in R.CASES + R.WIDE_CASES if c[3] == 0], ids=R.case_id)
def test_gradient_against_differences_of_the_device_value(case):
    r, ll = _handle(case, LOO)
    h = r["hyper"]
    got = ll.grad(h)
    sets = []
    for k in range(h.size):
        for sgn in (1.0, -1.0):
            hp = h.copy()
            hp[k] += sgn * 1.0e-5 * h[k]
            sets.append(hp)
    v = ll.evaluate(np.array(sets))
    fd = np.array([(v[2 * k] - v[2 * k + 1]) / (sets[2 * k][k] - sets[2 * k + 1][k]) for k in range(h.size)])
    assert _close(got, fd, 1e-5), (got, fd)


def test_se_with_derivative_observations():
    api = _api()
    r, ll = _handle(R.SE_DERIV_CASE, LOO)
    assert _close(ll.evaluate(r["hyper"][None, :])[0], r["value"])
    mean, var = ll.loo_predict(r["hyper"])
    assert _close(mean, r["bf_mu"]) and _close(var, r["bf_var"])
    with pytest.raises(api.InvalidValueException):
        ll.grad(r["hyper"])


@pytest.mark.parametrize("case", [(R.MATERN, 43, 3, 2), (R.SE, 65, 3, 0)], ids=R.case_id)
def test_objective_switching(case):
    api = _api()
    r, ll = _handle(case)
    _, never = _handle(case)
    h = r["hyper"]
    ll.set_objective(LOO)
    assert ll.objective == LOO
    loo_v, loo_g = ll.evaluate(h[None, :])[0], ll.grad(h)
    ll.set_objective(MARGINAL)
    assert ll.objective == MARGINAL
    v, g = ll.evaluate(h[None, :])[0], ll.grad(h)
    assert v == never.evaluate(h[None, :])[0] and np.array_equal(g, never.grad(h))
    assert loo_v != v and not np.array_equal(loo_g, g)
    with pytest.raises(api.BoundsException):
        ll.set_objective(2)
    assert ll.objective == MARGINAL


def test_optimisers_under_loo():
    """moe_ll_multistart / moe_ll_ascend at n = 24, d = 2, 4 starts, 20 steps: the end is no worse than the best start, its value is
    moe_ll_evaluate at the returned point, and a host ascent over the restatement with the same parameters ends where the device
    does -- to the tolerances test_hyperparameter_optimisers_against_reference gives the marginal likelihood under contractive
    steps (point 1e-6 relative, value 1e-9 max(1, |.|))."""
    api = _api()
    case = (R.MATERN, 24, 2, 0)
    X, y, derivs, _ = R.make_problem(case)
    nh = 4
    gd = (4, 20, 1, 0, 0.7, 1.0e-4, 0.2, 1.0e-12)
    dom = np.array([[-1.0, 1.0], [-1.0, 0.5], [-1.0, 0.5], [-3.0, 0.0]])
    rng = np.random.RandomState(5)
    guesses = 10.0 ** (dom[:, 0] + (dom[:, 1] - dom[:, 0]) * rng.uniform(0.25, 0.75, size=(4, nh)))
    ll = api.LogLikelihood(X, y, derivs, cov_type=case[0], objective=LOO)
    v0 = ll.evaluate(guesses)
    best, val, found = ll.multistart(gd, dom, guesses)
    assert val >= v0.max()
    assert abs(ll.evaluate(best[None, :])[0] - val) <= TOL * max(1.0, abs(val))

    def grad_fn(x):
        return np.array([[np.asarray(R.closed_form(X, y, derivs, p[0], case[0])[1], dtype=np.float64)] for p in x])

    lin = 10.0 ** dom
    ends = ms.gradient_ascent(grad_fn, gd, lin, guesses[:, None, :])[:, 0, :]
    end_vals = np.array([float(R.closed_form(X, y, derivs, p, case[0], want_grad=False)[0]) for p in ends])
    want_best, want_val = guesses[int(np.argmax(v0))], float(v0.max())
    want_found = False
    for s in range(4):
        if end_vals[s] > want_val:
            want_best, want_val, want_found = ends[s], end_vals[s], True
    assert found == want_found
    assert abs(val - want_val) <= 1e-9 * max(abs(want_val), 1.0), (val, want_val)
    assert np.abs(best / want_best - 1.0).max() <= 1e-6, (best, want_best)
    end = ll.ascend(gd, dom, guesses[0])
    assert np.abs(end / ends[0] - 1.0).max() <= 1e-6
    assert ll.evaluate(end[None, :])[0] >= v0[0]


@pytest.mark.parametrize("case", R.MCMC_CASES, ids=lambda c: "g%d" % c[3])
def test_sampler_under_loo(case):
    api = _api()
    pb = R.mcmc_problem(case)
    want = hm.run_chain(pb["p0"], *pb["tables"], pb["table"], pb["lnpost"])
    ll = api.LogLikelihood(pb["X"], pb["y"], pb["derivs"], cov_type=pb["cov_type"], objective=LOO)
    got = ll.mcmc(pb["table"], pb["p0"], *pb["tables"])
    assert _close(got["lnprob0"], want["lnprob0"])
    # the chains agree as long as every decision does: outside the band they must, inside it (at most 2 of 72) the comparison stops
    inside = 0
    for t in range(want["accepted"].shape[0]):
        for w in range(want["accepted"].shape[1]):
            assert _close(got["proposal_lnprob"][t, w], want["proposal_lnprob"][t, w]), (t, w)
            if want["margin"][t, w] <= 1e-8:
                inside += 1
                continue
            assert got["accepted"][t, w] == want["accepted"][t, w], (t, w)
    assert inside <= 2
    assert _close(got["lnprob"], want["lnprob"])


def test_boundary_routes_the_objective():
    """The five boundary functions accept leave_one_out_log_likelihood and return what api.LogLikelihood(objective=1) returns, bit
    for bit; the sampler class trains under it; the log_likelihood classes return the same numbers."""
    import wrappers_mirror as wm
    from cornell_moe_amd import GPP, log_likelihood, log_likelihood_mcmc
    api = _api()
    case = (R.MATERN, 21, 3, 2)
    r = R.reference(case)
    X, y, derivs, h = r["X"], r["y"], r["derivs"], r["hyper"]
    n, d, g = case[1], case[2], case[3]
    T = GPP.LogLikelihoodTypes.leave_one_out_log_likelihood
    ll = api.LogLikelihood(X, y, derivs, objective=LOO)
    ops = (list(X.ravel()), list(y.ravel()), d, n, T, [h[0], list(h[1:1 + d])], derivs, g, list(h[1 + d:]))
    assert GPP.compute_log_likelihood(*ops) == ll.evaluate(h[None, :])[0]
    assert np.array_equal(GPP.compute_hyperparameter_grad_log_likelihood(*ops), ll.grad(h))
    rows = np.array([h, 1.1 * h, 0.9 * h])
    status = {}
    vals = GPP.evaluate_log_likelihood_at_hyperparameter_list(list(rows.ravel()), list(X.ravel()), list(y.ravel()), d, n, T,
                                                              [h[0], list(h[1:1 + d])], list(h[1 + d:]), derivs, g, 3, 4, status)
    assert np.array_equal(vals, ll.evaluate(rows)) and status["evaluate_log_marginal_likelihood_at_hyperparameter_list"]
    # and the marginal likelihood on the same data is still served (the handle cache is keyed on the objective)
    ops0 = ops[:4] + (GPP.LogLikelihoodTypes.log_marginal_likelihood,) + ops[5:]
    assert GPP.compute_log_likelihood(*ops0) == api.LogLikelihood(X, y, derivs).evaluate(h[None, :])[0]

    class Opt(object):
        objective_type = T
        optimizer_type = GPP.OptimizerTypes.gradient_descent
        num_random_samples = 8
        optimizer_parameters = GPP.GradientDescentParameters(4, 10, 1, 0, 0.7, 1.0e-4, 0.2, 1.0e-12)

    nh = 1 + d + 1 + g
    dom = np.array([[-1.0, 1.0]] + [[-1.0, 0.5]] * d + [[-3.0, 0.0]] * (1 + g))
    rnd = GPP.RandomnessSourceContainer(1)
    rnd.SetExplicitUniformGeneratorSeed(7)
    st = {}
    got = GPP.multistart_hyperparameter_optimization(Opt(), list(dom.ravel()), list(X.ravel()), list(y.ravel()), d, n,
                                                     [h[0], list(h[1:1 + d])], list(h[1 + d:]), derivs, g, 4, rnd, st)
    rnd2 = GPP.RandomnessSourceContainer(1)
    rnd2.SetExplicitUniformGeneratorSeed(7)
    guesses = GPP._hyper_guesses(rnd2, dom, 4)
    want, _, found = ll.multistart(GPP._gd_params(Opt()), dom, guesses)
    assert np.array_equal(got, want) and st["log_marginal_likelihood_gradient_descent_found_update"] == found

    class Data(object):
        dim, num_sampled, points_sampled, points_sampled_value = d, n, X, y

        def append_sample_points(self, pts):
            raise NotImplementedError

    class Cov(object):
        hyperparameters = h[:1 + d].copy()
        num_hyperparameters = 1 + d

    mirror = wm.GaussianProcessLogLikelihood(Cov(), Data(), h[1 + d:], derivs, T)
    assert mirror.compute_log_likelihood() == ll.evaluate(h[None, :])[0]
    assert np.array_equal(mirror.compute_grad_log_likelihood(), ll.grad(h))
    ours = log_likelihood.GaussianProcessLeaveOneOutLogLikelihood(Cov(), Data(), h[1 + d:], derivs)
    assert ours.compute_log_likelihood() == ll.evaluate(h[None, :])[0]
    assert np.array_equal(ours.compute_grad_log_likelihood(), ll.grad(h))
    mean, var = ours.leave_one_out_predictions()
    mean1, var1 = ll.loo_predict(h)
    assert np.array_equal(mean, mean1) and np.array_equal(var, var1)
    marg = log_likelihood.GaussianProcessLogMarginalLikelihood(Cov(), Data(), h[1 + d:], derivs)
    ll0 = api.LogLikelihood(X, y, derivs)
    assert marg.compute_log_likelihood() == ll0.evaluate(h[None, :])[0]
    assert np.array_equal(marg.compute_grad_log_likelihood(), ll0.grad(h))
    assert np.array_equal(marg.leave_one_out_predictions()[0], mean1)

    sampler = log_likelihood_mcmc.GaussianProcessLogLikelihoodMCMC(
        Data(), derivs, log_likelihood_mcmc.DefaultPrior(nh, 1 + g, rng=np.random.RandomState(3)), chain_length=3, burnin_steps=2,
        n_hypers=2 * nh, log_likelihood_type=T, rng=np.random.RandomState(4))
    sampler.train()
    assert sampler._handle().objective == LOO
    assert len(sampler.models) > 0
