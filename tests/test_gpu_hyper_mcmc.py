"""GPU tests (-m gpu) of moe_ll_mcmc, the hyper-parameter ensemble sampler resident on the device, against the numpy restatement
(tests/hyper_mcmc_reference.py; likelihood from the plain-C oracle).  Transitions are checked, not trajectories: for every
half-step the DEVICE's state before it is taken, the proposal, prior and likelihood are recomputed on the host, and
  * proposal coordinates agree within 4 ulp.  The ABI shows a proposal's coordinates only through `chain`, that is where the
    proposal was accepted; the coordinates of a rejected proposal are not observable and are covered through its log posterior;
  * proposal_lnprob agrees within 1e-9 max(1, |want|) -- the tolerance tests/test_gpu_parity.py gives moe_ll_evaluate against
    the same oracle -- and infinities match exactly;
  * the decision is identical wherever |ln u - ln r| > 1e-8 max(1, |ln r|); decisions inside that band are skipped and at most
    1 in 1000 may be (tests/test_hyper_mcmc_reference.py confirms that the restated chains of these seeds have none);
  * chain, lnprob and accepted are consistent with the decisions bit for bit.
Shapes (hyper_mcmc_reference.CASES): (n, d, g) from (12, 2, 0) to (300, 6, 0) and (25, 3, 2) -- padded dimensions 4 and 8 -- and
(d, g) in {(10, 1), (12, 0), (14, 1), (16, 0), (17, 2), (24, 0), (25, 0), (32, 1)} -- padded dimensions 12, 16, 24, 32, each with and
without derivative observations, up to 70 walkers; 132 walkers at d = 2 (66
proposals per half-step: a second workgroup of the propose and accept kernels, passes of 64 + 2 factorisations); n (1 + g) = 300 rows
with g = 2 (a second row block of the covariance kernel with derivative observations).
"""
import os

import numpy as np
import pytest

import hyper_mcmc_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from cornell_moe_amd import _lib, api as _api
    _lib.load()
    _lib.require_gpu()
    return _api


def _run(api, c, quirks=None, **kw):
    LL = api.LogLikelihood(c["X"], c["y"], c["derivs"], cov_type=c["cov_type"])
    api.set_reference_quirks(c["quirks"] if quirks is None else quirks)
    try:
        return api.ll_mcmc(LL, c["table"], c["p0"], *c["tables"], **kw)
    finally:
        api.set_reference_quirks(-1)
        LL.close()


def _close(got, want, rel):
    if np.isinf(want) or np.isinf(got):
        return got == want
    return abs(got - want) <= rel * max(1.0, abs(want))


def check_transitions(c, res):
    """-> (decisions compared, decisions skipped inside the band, worst |proposal_lnprob - want| / max(1, |want|) seen)"""
    post = R.Posterior(c["cov_type"], c["X"], c["y"], c["derivs"], c["table"], c["quirks"])
    us, pt, ua = c["tables"]
    T, W = us.shape[0], c["p0"].shape[0]
    walkers = np.array([R.apply_fixed(c["table"], w) for w in c["p0"]])
    lnp = res["lnprob0"].copy()
    for w in range(W):
        assert _close(lnp[w], post(walkers[w]), 1e-9), ("lnprob0", w, lnp[w], post(walkers[w]))
    compared = skipped = 0
    worst = 0.0
    for t in range(T):
        for h in range(2):
            hs = R.half_step(walkers, lnp, h, us[t, h], pt[t, h], ua[t, h], c["table"], post)
            for i, w in enumerate(hs["index"]):
                want_lp, got_lp = hs["proposal_lnprob"][i], res["proposal_lnprob"][t, w]
                assert _close(got_lp, want_lp, 1e-9), ("proposal_lnprob", t, h, w, got_lp, want_lp)
                if np.isfinite(want_lp):
                    worst = max(worst, abs(got_lp - want_lp) / max(1.0, abs(want_lp)))
                lnr, lnu, acc = hs["lnr"][i], hs["lnu"][i], bool(res["accepted"][t, w])
                assert res["accepted"][t, w] in (0, 1)
                if np.isfinite(lnr) and np.isfinite(lnu) and abs(lnu - lnr) <= 1e-8 * max(1.0, abs(lnr)):
                    skipped += 1
                else:
                    compared += 1
                    assert acc == bool(hs["accept"][i]), ("decision", t, h, w, lnr, lnu)
                if acc:  # the stored position IS the device's proposal
                    assert np.all(np.abs(res["chain"][t, w] - hs["proposal"][i]) <= 4.0 * np.spacing(np.abs(hs["proposal"][i]))), \
                        ("proposal", t, h, w, res["chain"][t, w], hs["proposal"][i])
                    assert res["lnprob"][t, w] == got_lp
                else:
                    assert np.array_equal(res["chain"][t, w], walkers[w]) and res["lnprob"][t, w] == lnp[w]
                walkers[w], lnp[w] = res["chain"][t, w], res["lnprob"][t, w]
        assert np.array_equal(res["chain"][t], walkers) and np.array_equal(res["lnprob"][t], lnp)
    assert skipped * 1000 <= compared + skipped, (skipped, compared)
    return compared, skipped, worst


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_transitions_against_restatement(api, case):
    c = R.build_case(case)
    res = _run(api, c)
    compared, skipped, worst = check_transitions(c, res)
    print("%s: %d decisions compared, %d skipped, acceptance %.2f, worst proposal log posterior error %.3g (bound 1e-9)" % (
        c["name"], compared, skipped, res["accepted"].mean(), worst))
    assert 0 < res["accepted"].sum() < res["accepted"].size
    d = c["X"].shape[1]
    if case[5] == "wall":  # proposals beyond the wall (inside the box) were made and rejected
        assert np.isneginf(res["proposal_lnprob"]).sum() >= 1
        assert np.all((res["chain"][:, :, 1:1 + d] >= -1.3) & (res["chain"][:, :, 1:1 + d] <= -0.1))
    if case[5] == "box":
        assert np.isneginf(res["proposal_lnprob"][:, 0]).sum() >= 1 and np.all(np.abs(res["chain"]) <= 20.0)
    if case[5] == "fixed_noise":
        assert np.all(res["chain"][:, :, 1 + d:] == np.log(1.0e-8))


def test_quirks_switch_changes_the_prior_only(api):
    """the same chain input under both settings of moe_set_reference_quirks: each agrees with its own restatement (above), and the
    two differ"""
    c = R.build_case(R.CASES[0])
    on, off = _run(api, c, quirks=1), _run(api, c, quirks=0)
    assert not np.array_equal(on["lnprob0"], off["lnprob0"])
    c_off = dict(c, quirks=False)
    check_transitions(c_off, off)


def test_horseshoe_pole_is_always_accepted(api):
    """With quirks a proposal whose noise coordinate is exactly 0 has log prior +inf (base_prior.py:199-200) and is accepted whatever
    u is: walker 0 and its partner share coordinates that make c - z (c - s) exact."""
    c = R.build_case(R.CASES[0])
    d = c["X"].shape[1]
    H = c["p0"].shape[0] // 2
    us, pt, ua = [a.copy() for a in c["tables"]]
    us[0, 0, 0], pt[0, 0, 0], ua[0, 0, 0] = 0.0, 0, 1.0 - 2.0 ** -53  # z = 1 / 2: proposal = (c + s) / 2
    p0 = c["p0"].copy()
    p0[0, 1 + d], p0[H, 1 + d] = -0.5, 0.5
    c2 = dict(c, p0=p0, tables=(us, pt, ua))
    res = _run(api, c2)
    assert res["proposal_lnprob"][0, 0] == np.inf and res["accepted"][0, 0] == 1 and res["chain"][0, 0, 1 + d] == 0.0
    check_transitions(c2, res)


def test_two_passes_equal_one_bit_for_bit(api):
    """W / 2 = 12 proposals in one pass and in passes of 5 (MOE_MCMC_PASS_SETS): every output identical."""
    c = R.build_case(("passes", 1, 70, 3, 0, "default", True, 24, 6, 120))
    one = _run(api, c)
    os.environ["MOE_MCMC_PASS_SETS"] = "5"
    try:
        many = _run(api, c)
    finally:
        del os.environ["MOE_MCMC_PASS_SETS"]
    for k in ("chain", "lnprob", "lnprob0", "proposal_lnprob", "accepted"):
        assert np.array_equal(one[k], many[k]), k
    assert 0 < one["accepted"].sum() < one["accepted"].size
    check_transitions(c, many)
    # a pass of ONE matrix at N >= 256 (where a single factorisation would pick other kernels)
    c = R.build_case(("passes1", 1, 260, 2, 0, "default", True, None, 2, 121))
    one = _run(api, c)
    os.environ["MOE_MCMC_PASS_SETS"] = "1"
    try:
        many = _run(api, c)
    finally:
        del os.environ["MOE_MCMC_PASS_SETS"]
    for k in ("chain", "lnprob", "lnprob0", "proposal_lnprob", "accepted"):
        assert np.array_equal(one[k], many[k]), k


def test_error_codes(api):
    c = R.build_case(R.CASES[0])
    nh = c["p0"].shape[1]
    LL = api.LogLikelihood(c["X"], c["y"], c["derivs"], cov_type=c["cov_type"])
    rng = np.random.RandomState(0)

    def call(p0, T=2, table=None, tables=None):
        W = p0.shape[0]
        us, pt, ua = R.stretch_tables(rng, T, W - W % 2)
        if W % 2:  # (shapes a [T][2][W // 2] check accepts; the library must refuse the odd W)
            us, pt, ua = us[:, :, :W // 2], pt[:, :, :W // 2], ua[:, :, :W // 2]
        if tables is not None:
            us, pt, ua = tables
        return api.ll_mcmc(LL, c["table"] if table is None else table, p0, us, pt, ua)

    good = c["p0"]
    with pytest.raises(api.BoundsException) as e:
        call(np.vstack([good, good[:1]]))  # W odd
    assert e.value.value == good.shape[0] + 1 and e.value.min == 2 * nh
    with pytest.raises(api.BoundsException):
        call(good[:2 * nh - 2])  # W < 2 nh
    bad = good.copy()
    bad[3, 1] = 7.0  # outside the tophat: log posterior -inf
    with pytest.raises(api.InvalidValueException) as e:
        call(bad)
    assert e.value.value == 3 and e.value.truth == -np.inf
    bad = good.copy()
    bad[5, 0] = np.nan
    with pytest.raises(api.InvalidValueException) as e:
        call(bad)
    assert e.value.value == 5
    us, pt, ua = R.stretch_tables(rng, 2, good.shape[0])
    pt[1, 0, 2] = good.shape[0] // 2  # a partner index beyond the other half
    with pytest.raises(api.BoundsException):
        call(good, tables=(us, pt, ua))
    with pytest.raises(api.BoundsException):
        call(good, table=c["table"][:-1])
    with pytest.raises(api.BoundsException):
        call(good, table=[(9, 0.0, 0.0)] + c["table"][1:])
    out = call(good, T=0)  # no steps: lnprob0 only, and the handle still works after the errors
    assert out["chain"].shape == (0, good.shape[0], nh) and np.all(np.isfinite(out["lnprob0"]))
    LL.close()


def test_equivalence_with_host_driven_loop(api):
    """What the library could do before: the same tables driven from Python, ONE moe_ll_evaluate call per half-step and the restated
    move on the host.  Log posteriors agree within 1e-9 relative; the accept sequences are identical outside the band for as
    long as the states agree (they do to the end here: the comparison stops at the first skipped decision)."""
    for case in (R.CASES[2], R.CASES[4]):
        c = R.build_case(case)
        res = _run(api, c)
        LL = api.LogLikelihood(c["X"], c["y"], c["derivs"], cov_type=c["cov_type"])
        us, pt, ua = c["tables"]
        W, nh = c["p0"].shape
        H = W // 2
        nf = R.nh_free(c["table"])

        def lnpost(thetas):
            out = np.full(len(thetas), -np.inf)
            pri = np.array([R.log_prior(c["table"], th, c["quirks"]) if np.all(np.abs(th) <= R.BOX) else -np.inf for th in thetas])
            ok = pri > -np.inf
            if ok.any():
                out[ok] = pri[ok] + LL.evaluate(np.exp(thetas[ok]))
            return out

        walkers = np.array([R.apply_fixed(c["table"], w) for w in c["p0"]])
        lnp = lnpost(walkers)
        assert np.all(np.abs(lnp - res["lnprob0"]) <= 1e-9 * np.maximum(1.0, np.abs(lnp)))
        agree = True
        for t in range(us.shape[0]):
            for h in range(2):
                idx, other = np.arange(H) + h * H, (1 - h) * H
                z = R.stretch_z(2.0, us[t, h])
                cc = walkers[other + pt[t, h]]
                prop = np.array([R.apply_fixed(c["table"], p) for p in cc - z[:, None] * (cc - walkers[idx])])
                lp = lnpost(prop)
                with np.errstate(invalid="ignore", divide="ignore"):
                    lnr = (nf - 1) * np.log(z) + lp - lnp[idx]
                    lnu = np.log(ua[t, h])
                for i, w in enumerate(idx):
                    assert _close(res["proposal_lnprob"][t, w], lp[i], 1e-9)
                    in_band = np.isfinite(lnr[i]) and abs(lnu[i] - lnr[i]) <= 1e-8 * max(1.0, abs(lnr[i]))
                    if in_band:
                        agree = False
                    if agree:
                        assert bool(res["accepted"][t, w]) == bool(lp[i] == np.inf or lnr[i] > lnu[i])
                # follow the device's state so that the next proposals are comparable
                walkers[idx], lnp[idx] = res["chain"][t, idx], res["lnprob"][t, idx]
        assert agree
        LL.close()


def _historical(n, d, seed):
    import wrappers_mirror as cw
    X, y, _ = R.make_problem(n, d, 0, seed)
    hd = cw.HistoricalData(dim=d, num_derivatives=0)
    hd.append_sample_points([cw.SamplePoint(X[i], [y[i, 0]], 0.0) for i in range(n)])
    return hd, cw


def test_wrapper_train(api):
    from cornell_moe_amd import log_likelihood_mcmc as M
    hd, cw = _historical(20, 2, 7)

    def make(seed, noisy=True):
        rng = np.random.RandomState(seed)
        return M.GaussianProcessLogLikelihoodMCMC(hd, [], M.DefaultPrior(4, 1, rng=rng), chain_length=30, burnin_steps=40,
                                                  n_hypers=6, noisy=noisy, rng=rng)
    a = make(1)
    assert a.n_chains == 8 and not a.burned
    a.train()
    assert a.burned and a.is_trained and len(a.models) == 6 and a.gaussian_process_mcmc.num_mcmc == 6
    first = a.p0.copy()
    assert first.shape == (8, 4) and np.all(np.abs(first) <= 20.0)
    hyp1 = a.hypers.copy()
    # compute_log_likelihood is the sampler's log posterior
    LL = api.LogLikelihood(hd.points_sampled, hd.points_sampled_value, [])
    out = api.ll_mcmc(LL, a.prior_table(), first, *api.stretch_tables(np.random.RandomState(0), 0, 8))
    for w in range(8):
        assert abs(a.compute_log_likelihood(first[w]) - out["lnprob0"][w]) <= 1e-9 * max(1.0, abs(out["lnprob0"][w]))
    assert a.compute_log_likelihood(np.r_[0.0, 5.0, 0.0, -3.0]) == -np.inf and a.compute_log_likelihood(np.full(4, 21.0)) == -np.inf
    # a second train() starts from the kept positions: no second burn-in, the walkers move on from `first`
    a.train()
    assert a.burned and len(a.models) == 6 and not np.array_equal(a.p0, first)
    b = make(1)
    b.train()
    assert np.array_equal(b.p0, first) and np.array_equal(b.hypers, hyp1)  # reproducible bit for bit from the seed
    b.train()
    assert np.array_equal(b.p0, a.p0) and np.array_equal(b.hypers, a.hypers)
    # the models are usable GPs at the sampled hyper-parameters
    mu = a.models[0].compute_mean_of_points(list(np.asarray(hd.points_sampled)[:3].ravel()), 3)
    assert np.all(np.isfinite(mu))
    # new data: the walkers keep their positions, the next chain runs on the larger data set
    a.add_sampled_points([cw.SamplePoint(np.array([0.3, 0.6]), [0.1], 0.0)])
    kept = a.p0.copy()
    a.train()
    assert a.models[0].num_sampled == 21 and a.p0.shape == kept.shape
    # noisy=False: the noise coordinate is pinned at log 1e-8 throughout
    f = make(2, noisy=False)
    f.train()
    assert np.all(f.p0[:, 3:] == np.log(1.0e-8)) and len(f.models) == 6
