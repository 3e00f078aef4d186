"""Marginal mean / std and batch lower-confidence-bound selection on the device (csrc/lcb.hip: moe_gp_mean_std, moe_gp_lcb_select)
against tests/lcb_reference.py, at the smallest shapes that reach each branch: d in {2, 3, 4} throughout, d = 17 and 32 (padded
dimensions 24 and 32) in test_wide_dimensions.

Continuous outputs are held to the forward bound of the posterior-sampling tests against the extended-precision form:
|mean - want| <= 1e-10 max(1, |want|) and |std^2 - var_want| <= 1e-10 max(1, alpha).  Indices must be equal exactly; every test
first asserts, on the CPU, that every decision margin of its inputs (lcb_reference.Selection.margins) is >= 1e-7 -- three orders
above the forward bound -- and its seed was chosen so that this holds.  The tie cases assert the first-index rule instead.
Every test prints the worst figures it saw (pytest -s)."""
import numpy as np
import pytest

import lcb_reference as lr
import sampling_reference as sr
from cornell_moe_amd import GPP, _lib, api, lower_confidence_bound

pytestmark = pytest.mark.gpu

SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
MARGIN = 1e-7


def _problem(seed, n, d, cov_type, noise=1e-2, length=0.4, alpha=1.3, y_scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, d))
    y = y_scale * rng.normal(size=(n, 1))
    hyper = np.array([alpha] + [length] * d)
    G = api.DeviceGP(hyper, X, y, [noise], cov_type=cov_type)
    return rng, G, sr.Posterior(cov_type, hyper, X, y, [noise]), hyper


def _assert_surface(mean, std, want, alpha, what):
    e_mean = float((np.abs(mean - want.mean) / np.maximum(1.0, np.abs(want.mean))).max())
    e_var = float(np.abs(std * std - want.var).max() / max(1.0, alpha))
    print("%s: mean error %.3g, variance error %.3g (bound 1e-10)" % (what, e_mean, e_var))
    assert e_mean <= 1e-10 and e_var <= 1e-10, (what, e_mean, e_var)
    return e_mean, e_var


def _check(G, want, cand, q, alpha, what):
    """the whole comparison of one selection against a Selection of lcb_reference"""
    print("%s: smallest decision margin %.3g, kept %d of %d" % (what, min(want.margins), want.kept, len(cand)))
    assert min(want.margins) >= MARGIN, (what, want.margins)
    index, points, kept, mean, std = G.lcb_select(cand, q, want_surface=True)
    _assert_surface(mean, std, want, alpha, what)
    assert kept == want.kept, (what, kept, want.kept)
    assert np.array_equal(index, want.index), (what, index, want.index)
    assert np.array_equal(points, cand[want.index])
    m2, s2 = G.mean_std(cand)  # the primitive alone: the same kernels, so the same bits
    assert np.array_equal(m2, mean) and np.array_equal(s2, std)
    i3, p3, k3 = G.lcb_select(cand, q)  # without the surface: the same decisions
    assert np.array_equal(i3, index) and k3 == kept and np.array_equal(p3, points)


# launch_tri_gemm_cols: N < 128 the tiled kernel, N >= 128 the skinny kernels up to 16 columns and split-K beyond; 191 / 192 is the
# row-tile edge of the split-K kernel
@pytest.mark.parametrize("n,C_", [(127, 16), (127, 17), (128, 16), (128, 17), (129, 16), (129, 17), (191, 40), (192, 40)])
def test_kernel_choices_of_the_triangular_product(n, C_):
    rng, G, P, hyper = _problem(100 + n + C_, n, 2, MATERN, y_scale=0.2)
    cand = rng.uniform(0, 1, size=(C_, 2))
    _check(G, lr.extended(P, [1e-2], cand, 3), cand, 3, hyper[0], "N=%d C=%d" % (n, C_))


# lanes (63 / 64 / 65), the lanes' strided share (255 / 256 / 257) and a second workgroup (1025) of the reductions and the compaction
@pytest.mark.parametrize("C_", [63, 64, 65, 255, 256, 257, 1025])
def test_reduction_and_compaction_edges(C_):
    rng, G, P, hyper = _problem(200 + C_, 30, 2, SE, y_scale=0.2)
    cand = rng.uniform(0, 1, size=(C_, 2))
    want = lr.extended(P, [1e-2], cand, 3)
    assert 1 < want.kept < C_  # (the compaction has something to drop and something to keep)
    _check(G, want, cand, 3, hyper[0], "N=30 C=%d" % C_)


@pytest.mark.parametrize("n,C_,d,cov_type,seed", [(600, 384, 4, SE, 1), (300, 200, 3, MATERN, 2)])
def test_split_k_state_and_several_rounds(n, C_, d, cov_type, seed):
    rng, G, P, hyper = _problem(seed, n, d, cov_type, length=0.5, y_scale=0.2)
    cand = rng.uniform(0, 1, size=(C_, d))
    _check(G, lr.extended(P, [1e-2], cand, 4), cand, 4, hyper[0], "N=%d C=%d d=%d" % (n, C_, d))


@pytest.mark.parametrize("n,C_,d,cov_type", [(129, 40, 17, MATERN), (40, 17, 32, SE)])
def test_wide_dimensions(n, C_, d, cov_type):
    """Padded dimensions 24 and 32 of the radial sums (and split-K at N = 129), eight picks.  Lengths 0.1 + 0.25 sqrt(d): the default
    0.4 makes K nearly diagonal at d = 32 and the selection trivial.  The indices are the only output of the rounds, so the seeds are
    the ones of 1 .. 60 whose smallest decision margin is small while still 700 times the rule's 1e-7 (7.6e-5 with 31 of 40 kept,
    7.7e-5 with 16 of 17 kept): an error in a covariance beyond that flips a pick."""
    rng, G, P, hyper = _problem(WIDE_SEEDS[d], n, d, cov_type, length=0.1 + 0.25 * np.sqrt(d))
    cand = rng.uniform(0, 1, size=(C_, d))
    want = lr.extended(P, [1e-2], cand, 8)
    assert 1 < want.kept < C_ and len(set(want.index.tolist())) == 8  # (something to drop, something to keep, eight different picks)
    _check(G, want, cand, 8, hyper[0], "N=%d C=%d d=%d" % (n, C_, d))


def test_kept_set_smaller_than_the_batch():
    """(129, 65, 2) with noise 1e-4: three candidates kept, four asked for -- a point is picked twice, as the reference does.
    (seed chosen for a kept set of exactly three and margins above 1e-7)"""
    rng, G, P, hyper = _problem(KEPT3_SEED, 129, 2, MATERN, noise=1e-4)
    cand = rng.uniform(0, 1, size=(65, 2))
    want = lr.extended(P, [1e-4], cand, 4)
    assert want.kept == 3 and len(set(want.index.tolist())) < 4
    _check(G, want, cand, 4, hyper[0], "kept 3 < q 4")


def test_pass_boundary_and_bits_of_a_candidate_alone():
    """N = 30: passes of moe_lcb_pass_size(30, C) = 16 384 candidates; C = 16 384 + 37 makes two.  A candidate's mean and std carry
    the same bits alone, in a small call and inside the big one, on either side of the boundary."""
    rng, G, P, hyper = _problem(5, 30, 2, SE, y_scale=0.2)
    per_pass = _lib.load().moe_lcb_pass_size(30, 20000)
    assert per_pass == 16384
    C_ = per_pass + 37
    cand = rng.uniform(0, 1, size=(C_, 2))
    want = lr.extended(P, [1e-2], cand, 2)
    _check(G, want, cand, 2, hyper[0], "two passes, C=%d" % C_)
    mean, std = G.mean_std(cand)
    for i in (0, 1023, 1024, per_pass - 1, per_pass, per_pass + 1, C_ - 1):
        m1, s1 = G.mean_std(cand[i:i + 1])
        assert m1[0] == mean[i] and s1[0] == std[i], i
    lo = per_pass - 50
    m100, s100 = G.mean_std(cand[lo:lo + 100])
    assert np.array_equal(m100, mean[lo:lo + 100]) and np.array_equal(s100, std[lo:lo + 100])


def test_derivative_observations_condition_on_whole_blocks():
    """60 points with the derivatives (0, 2) observed: N = 180, and every pick joins the data with its 3 observation rows.  Against
    the literal procedure over the oracle's GP (plain double, itself within 6e-12 / 6e-14 of extended precision without
    derivatives)."""
    rng = np.random.default_rng(11)
    n, d, derivs = 60, 3, (0, 2)
    X, y = rng.uniform(0, 1, size=(n, d)), rng.normal(size=(n, 3))
    hyper, noise = np.array([1.3, 0.5, 0.6, 0.7]), np.array([1e-2, 2e-2, 3e-2])
    cand = rng.uniform(0, 1, size=(100, d))
    for cov_type in (MATERN, SE):
        G = api.DeviceGP(hyper, X, y, noise, derivs, cov_type=cov_type)
        want = lr.literal(lr.OrcLike(cov_type, hyper, X, y, noise, derivs), cand, 3)
        _check(G, want, cand, 3, hyper[0], "derivatives (0, 2), cov %d" % cov_type)
        # the model of the primitive: compute_mean_of_points and entry [0,0] of the single point's factor
        m, s = G.mean_std(cand[:6])
        for i in range(6):
            assert abs(s[i] - G.cholesky_variance(cand[i:i + 1])[0]) <= 1e-10 and abs(m[i] - G.mean(cand[i:i + 1])[0]) <= 1e-10


@pytest.mark.parametrize("where,copies", [("across wavefronts", (70, 200)), ("within a wavefront", (130, 150)),
                                          ("within a lane's strided share", (10, 266, 522))])
def test_exact_ties_take_the_first_index(where, copies):
    """Duplicates of the argmin's candidate and of the first round's argmax sit at `copies` (and the next position each): equal
    bits, so the first index has to win in both reductions.  A flat, uncertain GP keeps every candidate, so positions in the kept
    set are candidate indices."""
    rng, G, P, hyper = _problem(31, 20, 2, MATERN, y_scale=0.01)
    cand = rng.uniform(0, 1, size=(600, 2))
    base = lr.extended(P, [1e-2], cand, 2)
    a0, a1 = int(base.index[0]), int(base.index[1])
    spots0 = list(copies)
    spots1 = [c + 1 for c in copies]
    assert a0 not in spots0 + spots1 and a1 not in spots0 + spots1 and int(np.argmin(base.mean + np.sqrt(base.var))) not in spots0 + spots1
    tied = cand.copy()
    tied[spots0] = cand[a0]
    tied[spots1] = cand[a1]
    want = lr.extended(P, [1e-2], tied, 2)
    assert want.kept == 600
    assert want.index[0] == min(spots0 + [a0]) and want.index[1] == min(spots1 + [a1])  # numpy's first-index rule
    assert want.margins[0] == 0.0 and want.margins[2] == 0.0  # the ties are real
    index, points, kept, mean, std = G.lcb_select(tied, 2, want_surface=True)
    for s in spots0:
        assert mean[s] == mean[a0] and std[s] == std[a0]  # a candidate's bits do not depend on its position
    for s in spots1:
        assert mean[s] == mean[a1] and std[s] == std[a1]
    assert kept == 600 and np.array_equal(index, want.index), (where, index, want.index)


def _isolated_gp():
    """Ten sampled points 100 lengths apart under the square exponential with alpha = 1 and NO noise: every off-diagonal covariance
    underflows to 0, K = I exactly, and the variance at a sampled point is 1 - 1 = 0 in exact floating-point arithmetic."""
    X = np.array([[100.0 * i, 0.0] for i in range(10)])
    y = np.linspace(-1.0, 1.0, 10)[:, None]
    return api.DeviceGP([1.0, 1.0, 1.0], X, y, [0.0], cov_type=SE), X


def test_candidate_on_a_noiseless_sampled_point_is_singular():
    G, X = _isolated_gp()
    cand = X + np.array([0.3, 0.2])
    cand[5] = X[3]
    cand[8] = X[1]
    for call in (lambda: G.mean_std(cand), lambda: G.lcb_select(cand, 2)):
        with pytest.raises(api.SingularMatrixException) as ei:
            call()
        assert ei.value.num_rows == 1 and ei.value.leading_minor_index == 5  # the first failing candidate
    mean, std = G.mean_std(np.delete(cand, [5, 8], axis=0))  # the handle is usable afterwards
    assert np.all(np.isfinite(mean)) and np.all(std > 0.1)
    assert G.n == 10


def test_noiseless_point_picked_twice_fails_the_conditioning_pivot():
    """One candidate, three picks, no noise: round 1 conditions on it (pivot v = 1 - e^2 = 0.1), round 2 picks it again and its Schur
    pivot is v - (v / sqrt v)^2, at most 3 ulp(0.1) = 4e-17 in magnitude: below the pivot rule's 1e-16 whatever its sign -- the
    reference's add_sampled_points raising on a noiseless duplicate."""
    G, X = _isolated_gp()
    cand = X[2:3] + np.array([[np.sqrt(-np.log(0.9)), 0.0]])
    index, points, kept = G.lcb_select(cand, 2)
    assert list(index) == [0, 0] and kept == 1
    before = G.get_factor()
    with pytest.raises(api.SingularMatrixException) as ei:
        G.lcb_select(cand, 3)
    assert ei.value.num_rows == 12 and ei.value.leading_minor_index == 12
    after = G.get_factor()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert list(G.lcb_select(cand, 1)[0]) == [0]


def test_limits():
    rng, G, P, hyper = _problem(Q64_SEED, 30, 2, MATERN, y_scale=0.2)
    cand = rng.uniform(0, 1, size=(80, 2))
    # q = 1: no rounds
    want = lr.extended(P, [1e-2], cand, 1)
    _check(G, want, cand, 1, hyper[0], "q=1")
    # q = 64 at C = 80: the limit (seed chosen for margins above 1e-7 in all 64 decisions)
    _check(G, lr.extended(P, [1e-2], cand, 64), cand, 64, hyper[0], "q=64 C=80")
    for bad_q in (65, 0):
        with pytest.raises(api.BoundsException):
            G.lcb_select(cand, bad_q)
    with pytest.raises(api.BoundsException):
        G.lcb_select(np.zeros((0, 2)), 1)
    with pytest.raises(api.BoundsException):
        G.mean_std(np.zeros((0, 2)))


def _gpp_gp(X, y, hyper, noise):
    n, d = X.shape
    return GPP.GaussianProcess([hyper[0], list(hyper[1:])], list(X.ravel()), list(y.ravel()), list(noise), [], 0, d, n)


@pytest.mark.parametrize("wrapped", [False, True])
def test_quirks_decide_what_is_left_in_the_gp(wrapped):
    import wrappers_mirror as cw
    rng = np.random.default_rng(41)
    n, d, q = 40, 3, 4
    X, y = rng.uniform(0, 1, size=(n, d)), rng.normal(size=(n, 1))
    hyper, noise = np.array([1.3, 0.4, 0.5, 0.6]), [1e-2]
    cand, probe = rng.uniform(0, 1, size=(150, d)), rng.uniform(0, 1, size=(5, d))

    def make():
        if not wrapped:
            gp = _gpp_gp(X, y, hyper, noise)
            return gp, gp
        data = cw.HistoricalData(d, 0)
        data.append_historical_data(X, y, np.full(n, noise[0]))
        gp = cw.GaussianProcess(cw.SquareExponential(hyper), noise, data, [])
        return gp, gp._gaussian_process

    want = lr.extended(sr.Posterior(MATERN, hyper, X, y, noise), noise, cand, q)  # (GPP's kernel is Matern whatever it is called)
    assert min(want.margins) >= MARGIN
    quirks = api.get_reference_quirks()
    try:
        api.set_reference_quirks(1)
        gp, inner = make()
        results, zero = lower_confidence_bound.lower_confidence_bound_optimization(gp, cand, q)
        assert zero == 0.0 and np.array_equal(results, cand[want.index])
        assert gp.num_sampled == n + q - 1
        grown = _gpp_gp(np.vstack([X, results[:-1]]), np.vstack([y, np.zeros((q - 1, 1))]), hyper, noise)
        got, ref = np.array(inner.compute_mean_of_points(list(probe.ravel()), 5)), np.array(grown.compute_mean_of_points(list(probe.ravel()), 5))
        print("quirks on: mean of the grown GP differs by %.3g" % np.abs(got - ref).max())
        assert np.abs(got - ref).max() <= 1e-12
        if wrapped:
            assert gp._historical_data.num_sampled == n + q - 1

        api.set_reference_quirks(0)
        gp, inner = make()
        before = inner._dev.get_factor()
        results, _ = lower_confidence_bound.lower_confidence_bound_optimization(gp, cand, q)
        after = inner._dev.get_factor()
        assert np.array_equal(results, cand[want.index]) and gp.num_sampled == n
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    finally:
        api.set_reference_quirks(1 if quirks else 0)


def test_run_cpp_tests_covers_the_selection():
    from cornell_moe_amd import selftest
    assert selftest.check_lcb() is True
    assert GPP.run_cpp_tests() == 0


# seeds found on the CPU with lcb_reference.extended alone (tests/lcb_reference.py; no device involved)
KEPT3_SEED = 16
Q64_SEED = 0
WIDE_SEEDS = {17: 6, 32: 8}
