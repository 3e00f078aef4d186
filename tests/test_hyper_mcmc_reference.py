"""CPU tests (-m "not gpu") of the hyper-parameter sampler's restatement (tests/hyper_mcmc_reference.py) and of the ABI it
restates: the prior formulas against scipy.stats where they are textbook and against hand-evaluated values where they follow
the reference's deviations; stationarity of the restated move on a Gaussian target; the header, the ctypes binding and the
library agree on moe_ll_mcmc and moe_prior_t; none of the GPU suite's committed seeds puts a decision inside the tolerance
band of tests/test_gpu_hyper_mcmc.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.stats as sps

import hyper_mcmc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_textbook_priors_against_scipy():
    for th in (-2.5, -0.3, 0.0, 0.7, 4.0):
        assert abs(R.prior_term(R.NORMAL, 0.25, 2.0, th, False) - sps.norm.logpdf(th, loc=0.25, scale=2.0)) <= 1e-14 * 10
        assert abs(R.prior_term(R.NORMAL, 0.25, 2.0, th, True) - sps.norm.pdf(th, loc=0.25, scale=2.0)) <= 1e-15
        for quirks in (True, False):
            want = sps.lognorm.logpdf(th, 0.8, loc=-1.0)
            got = R.prior_term(R.LOGNORMAL, 0.8, -1.0, th, quirks)
            assert (got == want) if np.isinf(want) else abs(got - want) <= 1e-13 * max(1.0, abs(want))
            assert R.prior_term(R.TOPHAT, -2.0, 3.0, th, quirks) == (0.0 if -2.0 <= th <= 3.0 else -np.inf)
            assert R.prior_term(R.NONE, 0.0, 0.0, th, quirks) == 0.0 and R.prior_term(R.FIXED, 1.0, 0.0, th, quirks) == 0.0
    assert R.prior_term(R.LOGNORMAL, 0.8, -1.0, -1.0, True) == -np.inf  # the edge of the support
    assert R.prior_term(R.TOPHAT, -2.0, 3.0, -2.0, True) == 0.0 and R.prior_term(R.TOPHAT, -2.0, 3.0, 3.0, True) == 0.0


def test_reference_quirk_priors_against_hand_values():
    # NORMAL with quirks: the density (base_prior.py:354); values to 30 digits from the closed forms
    assert abs(R.prior_term(R.NORMAL, 0.0, 1.0, 0.5, True) - 0.352065326764299477774680441597) <= 1e-15
    assert abs(R.prior_term(R.NORMAL, 0.25, 2.0, 1.0, True) - 0.185927546934884455636623267513) <= 1e-15
    # HORSESHOE with quirks: ln ln(1 + 3 (0.1 / theta)^2) of the log-space coordinate, +inf at 0 (base_prior.py:199-201)
    for th, want in ((-3.0, -5.70544683112695001582693724044), (0.5, -2.17746296287808542567162165164),
                     (19.9, -9.48803523741668891149113901379)):
        assert abs(R.prior_term(R.HORSESHOE, 0.1, 0.0, th, True) - want) <= 1e-11 * abs(want)
    assert R.prior_term(R.HORSESHOE, 0.1, 0.0, 0.0, True) == np.inf
    # ... and without: the same formula of exp(theta)
    for th, want in ((-3.0, 0.945006778074140699028023982497), (0.5, -4.51205088032104013898724932141),
                     (18.0, -39.5065578973199846917422129475)):
        assert abs(R.prior_term(R.HORSESHOE, 0.1, 0.0, th, False) - want) <= 1e-13 * abs(want)
    # the sum: -inf wins over +inf, +inf over anything finite (default_priors.py:27-36 adds the terms)
    table = R.default_prior_table(4, 1)
    assert table == [(R.NORMAL, 0.0, 1.0), (R.TOPHAT, -2.0, 3.0), (R.TOPHAT, -2.0, 3.0), (R.HORSESHOE, 0.1, 0.0)]
    assert R.log_prior(table, [0.5, 0.0, 1.0, 0.0], True) == np.inf
    assert R.log_prior(table, [0.5, 3.5, 1.0, 0.0], True) == -np.inf
    want = 0.352065326764299477774680441597 + 0.0 + 0.0 - 5.70544683112695001582693724044
    assert abs(R.log_prior(table, [0.5, 0.0, 1.0, -3.0], True) - want) <= 1e-11
    assert np.array_equal(R.apply_fixed([(R.NONE, 0, 0), (R.FIXED, -18.0, 0)], [1.0, 2.0]), [1.0, -18.0])
    assert R.nh_free([(R.NONE, 0, 0), (R.FIXED, -18.0, 0), (R.TOPHAT, 0, 1)]) == 2


def test_package_priors_agree_with_restatement():
    """cornell_moe_amd.log_likelihood_mcmc lowers its prior classes to the table the restatement evaluates (the package holds
    no formulas of its own: the device evaluates the table)."""
    from cornell_moe_amd import _lib, log_likelihood_mcmc as M
    assert (_lib.PRIOR_NONE, _lib.PRIOR_TOPHAT, _lib.PRIOR_NORMAL, _lib.PRIOR_HORSESHOE, _lib.PRIOR_LOGNORMAL,
            _lib.PRIOR_FIXED) == (R.NONE, R.TOPHAT, R.NORMAL, R.HORSESHOE, R.LOGNORMAL, R.FIXED)
    dp = M.DefaultPrior(6, 2)
    assert dp.table(6) == R.default_prior_table(6, 2)
    assert M.TophatPrior(-1, 2).table(2) == [(R.TOPHAT, -1.0, 2.0)] * 2
    assert M.NormalPrior(sigma=2.0, mean=0.25).row() == (R.NORMAL, 0.25, 2.0)
    assert M.LognormalPrior(0.8, mean=-1.0).row() == (R.LOGNORMAL, 0.8, -1.0)
    assert M.HorseshoePrior(0.3).row() == (R.HORSESHOE, 0.3, 0.0)
    # sample_from_prior: shapes and supports (base_prior.py / default_priors.py)
    s = M.DefaultPrior(6, 2, rng=np.random.RandomState(5)).sample_from_prior(50)
    assert s.shape == (50, 6) and np.all((s[:, 1:4] >= -2) & (s[:, 1:4] <= 3)) and np.all(np.isfinite(s))
    t = M.TophatPrior(-1, 2, rng=np.random.RandomState(5)).sample_from_prior(7)
    assert t.shape == (7, 1) and np.array_equal(t[:, 0], -1 + np.random.RandomState(5).rand(7) * 3)
    with pytest.raises(ValueError):
        M.TophatPrior(1, 1)


def test_stretch_move_leaves_a_gaussian_stationary():
    """The restated move (z from ((a - 1) u + 1)^2 / a, ratio z^(n - 1) p(y) / p(x)) samples a correlated two-coordinate normal:
    the first and second moments of a long chain agree with the target's within 5 standard errors, the standard error being
    the chain's own batch-means estimate (25 batches of 480 steps of the ensemble average, far longer than the
    autocorrelation time), and that standard error is itself small (< 5 % of the scale of the moment)."""
    mu = np.array([1.0, -2.0])
    S = np.array([[1.0, 0.9], [0.9, 2.0]])
    Sinv = np.linalg.inv(S)
    lnpost = lambda th: float(-0.5 * (th - mu) @ Sinv @ (th - mu))  # noqa: E731
    rng = np.random.RandomState(11)
    W, T, burn, batches = 8, 12500, 500, 25
    tables = R.stretch_tables(rng, T, W)
    z = R.stretch_z(2.0, tables[0])
    assert z.min() >= 0.5 and z.max() <= 2.0 and abs(z.mean() - 7.0 / 6.0) < 0.01  # E z = (1 / a) E (u + 1)^2 = 7 / 6
    res = R.run_chain(mu + rng.standard_normal((W, 2)), *tables, table=[(R.NONE, 0.0, 0.0)] * 2, lnpost=lnpost)
    x = res["chain"][burn:] - mu  # [steps][W][2]
    sd = np.sqrt(np.diag(S))
    series = {"mean0": (x[:, :, 0].mean(axis=1), 0.0, sd[0]), "mean1": (x[:, :, 1].mean(axis=1), 0.0, sd[1]),
              "var0": ((x[:, :, 0] ** 2).mean(axis=1), S[0, 0], S[0, 0]), "var1": ((x[:, :, 1] ** 2).mean(axis=1), S[1, 1], S[1, 1]),
              "cov01": ((x[:, :, 0] * x[:, :, 1]).mean(axis=1), S[0, 1], sd[0] * sd[1])}
    for name, (v, want, scale) in series.items():
        bm = v.reshape(batches, -1).mean(axis=1)
        se = bm.std(ddof=1) / np.sqrt(batches)
        assert se < 0.05 * scale, (name, se)
        assert abs(v.mean() - want) <= 5.0 * se, (name, v.mean(), want, se)
    assert 0.3 < res["accepted"].mean() < 0.95
    # bookkeeping of the restated chain itself: a rejected walker keeps its position
    t, w = np.argwhere(res["accepted"][1:] == 0)[0]
    assert np.array_equal(res["chain"][t + 1, w], res["chain"][t, w])


def test_abi_symbol_and_prior_layout():
    """include/moe_hip.h, the ctypes binding and the library agree on moe_ll_mcmc and moe_prior_t."""
    from cornell_moe_amd import _lib, build as moe_build
    text = open(os.path.join(ROOT, "include", "moe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct moe_prior \{\s*int kind;\s*double a, b;\s*\} moe_prior_t;", code)
    assert m, "moe_prior_t is (int kind; double a, b)"
    assert C.sizeof(_lib.Prior) == 24 and (_lib.Prior.kind.offset, _lib.Prior.a.offset, _lib.Prior.b.offset) == (0, 8, 16)
    for name, val in (("NONE", 0), ("TOPHAT", 1), ("NORMAL", 2), ("HORSESHOE", 3), ("LOGNORMAL", 4), ("FIXED", 5)):
        assert re.search(r"#define MOE_PRIOR_%s %d\b" % (name, val), code)
        assert getattr(_lib, "PRIOR_" + name) == val
    decl = re.search(r"int moe_ll_mcmc\((.*?)\);", code, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "ll", "priors", "num_walkers", "num_steps", "stretch_a", "p0", "u_stretch", "partner", "u_accept", "chain", "lnprob",
        "lnprob0", "proposal_lnprob", "accepted", "err"]
    res, args = _lib.SIGNATURES["moe_ll_mcmc"]
    assert res is C.c_int and len(args) == len(params)
    assert args[1] is C.POINTER(_lib.Prior) and args[2] is C.c_int and args[4] is C.c_double and args[7] is _lib.ip
    moe_build.build()
    lib = _lib.load()
    assert hasattr(lib, "moe_ll_mcmc")
    # NULL mandatory arguments are an error code, not a crash (reached without a device)
    err = _lib.MoeError()
    rc = lib.moe_ll_mcmc(None, None, 4, 0, 2.0, None, None, None, None, None, None, None, None, None, C.byref(err))
    assert rc == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_committed_seeds_keep_clear_of_the_decision_band(case):
    """tests/test_gpu_hyper_mcmc.py skips a decision whose |ln u - ln r| is within 1e-8 max(1, |ln r|): for the committed seeds
    the restated chain has none there (nor within 100 times that), and the cases exercise what their names promise."""
    c = R.build_case(case)
    post = R.Posterior(c["cov_type"], c["X"], c["y"], c["derivs"], c["table"], c["quirks"])
    res = R.run_chain(c["p0"], *c["tables"], table=c["table"], lnpost=post)
    assert np.all(np.isfinite(res["lnprob0"]))
    assert res["margin"].min() > 1e-6
    assert 0 < res["accepted"].sum() < res["accepted"].size
    d = c["X"].shape[1]
    if case[5] == "wall":  # proposals beyond the wall, inside the box
        hit = np.isneginf(res["proposal_lnprob"])
        assert hit.sum() >= 3 and np.all((res["chain"][:, :, 1:1 + d] >= -1.3) & (res["chain"][:, :, 1:1 + d] <= -0.1))
    if case[5] == "box":
        assert np.isneginf(res["proposal_lnprob"][:, 0]).sum() >= 1 and np.all(np.abs(res["chain"]) <= 20.0)
    if case[5] == "fixed_noise":
        assert np.all(res["chain"][:, :, 1 + d:] == np.log(1.0e-8))
