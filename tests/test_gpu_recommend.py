"""The ensemble-averaged posterior mean and the recommendation on the device (csrc/recommend.hip: moe_posterior_mean_mcmc_batch,
moe_posterior_mean_mcmc_recommend) against tests/recommend_reference.py, at the smallest shapes that reach each branch.

Values and gradients are held to the forward bound of the sampling and LCB tests against the extended-precision form:
|f - want| <= 1e-10 max(1, |want|), |grad - want| <= 1e-10 max(1, |want|_inf).  Indices and decisions must be equal exactly; every
test first asserts that the decision margins of its inputs are >= 1e-7 (seeds chosen on the CPU so that this holds).  The descent
is checked step by step against the device's own path, |path[i+1] - F_ext(path[i], i)| <= a_i 1e-10 max(1, |grad f|_inf) per
coordinate, so that no trajectory sensitivity enters.  Every test prints the worst figures it saw (pytest -s)."""
import types

import numpy as np
import pytest

import recommend_reference as rr
import sampling_reference as sr
from cornell_moe_amd import GPP, api, posterior_mean_mcmc

pytestmark = pytest.mark.gpu

SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
LD = rr.LD
MARGIN = 1e-7
PASS = 16384  # points per launch (include/moe_hip.h: moe_posterior_mean_mcmc_batch)


def row_stride(E, d):
    """training points a lane strides by in csrc/recommend.hip's ensemble_sums: 64 (W / min(E, W)), W wavefronts from padded d"""
    dp = (d + 3) // 4 * 4 if d <= 16 else (d + 7) // 8 * 8
    W = 16 if dp <= 4 else (8 if dp <= 16 else 4)
    return 64 * (W // min(E, W))


def _build(seed, n, d, E, cov_type, derivs=(), num_fidelity=0):
    members, a = rr.make_ensemble(seed, n, d, E, cov_type, derivs)
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=cov_type) for e in range(E)]
    return gps, rr.Ensemble(members, num_fidelity), a


def _assert_value_grad(value, grad, ens, pts, what):
    want, gwant = ens.f(pts, True)
    want64 = want.astype(np.float64)
    e_val = float(np.max(np.abs(value - want) / np.maximum(1.0, np.abs(want64))))
    scale = np.maximum(1.0, np.max(np.abs(gwant), axis=1).astype(np.float64))
    e_grad = float(np.max(np.abs(grad - gwant) / scale[:, None]))
    print("%s: value error %.3g, gradient error %.3g (bound 1e-10)" % (what, e_val, e_grad))
    assert e_val <= 1e-10 and e_grad <= 1e-10, (what, e_val, e_grad)


# E, d, cov, derivs, num_fidelity, n (None: one below, at, one above the row stride and its next multiple), num_points
BATCH_CASES = [
    (16, 3, MATERN, (), 0, None, 65),
    (3, 8, SE, (), 0, None, 63),
    (1, 8, MATERN, (), 1, (511, 512, 513), 64),
    (2, 9, MATERN, (0, 2), 0, (40,), 1025),
    (3, 32, SE, (), 1, (33,), 65),
    (2, 1, SE, (), 0, (30,), 1),
    (16, 3, SE, (0, 2), 1, (65,), 64),
    (1, 32, MATERN, (1, 31), 0, (20,), 63),
    (17, 3, MATERN, (), 0, (70,), 5),   # more members than wavefronts: two groups
]


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: "E%d-d%d-cov%d-g%d-f%d" % (c[0], c[1], c[2], len(c[3]), c[4]))
def test_averaged_value_and_gradient(case):
    E, d, cov, derivs, nf, ns, P = case
    stride = row_stride(E, d)
    for n in (ns or (stride - 1, stride, stride + 1, 2 * stride)):
        gps, ens, a = _build(10 * E + d + n, n, d, E, cov, derivs, nf)
        rng = np.random.default_rng(n)
        pts = rng.uniform(0, 1, size=(P, d - nf))
        before = [g.mean(a["X"][:3] + 0.01) for g in gps]
        value, grad = api.posterior_mean_mcmc(gps, pts, nf, want_grad=True)
        _assert_value_grad(value, grad, ens, pts, "E=%d d=%d n=%d P=%d" % (E, d, n, P))
        assert np.array_equal(api.posterior_mean_mcmc(gps, pts, nf), value)  # the value-only kernel: the same bits
        # a point evaluated alone gives the bits it has inside the batch
        k = P // 2
        v1, g1 = api.posterior_mean_mcmc(gps, pts[k:k + 1], nf, want_grad=True)
        assert v1[0] == value[k] and np.array_equal(g1[0], grad[k])
        # the handles answer as before
        assert all(np.array_equal(u, g.mean(a["X"][:3] + 0.01)) for u, g in zip(before, gps))


def test_across_a_pass_boundary():
    gps, ens, a = _build(5, 10, 1, 1, MATERN)
    rng = np.random.default_rng(6)
    pts = rng.uniform(0, 1, size=(PASS + 1, 1))
    value, grad = api.posterior_mean_mcmc(gps, pts, 0, want_grad=True)
    _assert_value_grad(value, grad, ens, pts, "P=%d" % (PASS + 1))
    tail, gtail = api.posterior_mean_mcmc(gps, pts[PASS - 1:], 0, want_grad=True)
    assert np.array_equal(tail, value[PASS - 1:]) and np.array_equal(gtail, grad[PASS - 1:])


def test_mismatched_members_and_ranges_are_refused():
    gps, ens, a = _build(1, 12, 3, 2, MATERN)
    other = api.DeviceGP(a["hypers"][0], a["X"][:11], a["y"][:11], a["noises"][0], cov_type=MATERN)
    pts = np.full((2, 3), 0.5)
    with pytest.raises(api.InvalidValueException):
        api.posterior_mean_mcmc([gps[0], other], pts)
    with pytest.raises(api.BoundsException):
        api.posterior_mean_mcmc(gps, pts, num_fidelity=3)
    err = api._lib.MoeError()
    import ctypes as C
    arr = (C.c_void_p * 2)(*[g._h.value for g in gps])
    out = np.zeros(4)
    assert api._lib.load().moe_posterior_mean_mcmc_batch(arr, 2, 3, out.ctypes.data_as(api.dp), 1, out.ctypes.data_as(api.dp), None,
                                                         C.byref(err)) == api._lib.MOE_ERR_BOUNDS


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1025])
def test_screening_index(P):
    gps, ens, a = _build(40 + P, 30, 3, 3, MATERN)
    rng = np.random.default_rng(P)
    cand = rng.uniform(0, 1, size=(P, 3))
    gd = rr.GdParams(1, 0, 0.7, 1e-3, 1.0)
    want = rr.extended(ens, gd, [[0, 1]] * 3, cand, 1)
    print("P=%d: margins %s" % (P, want.margins))
    assert min(want.margins[:-1] or [1.0]) >= MARGIN
    res = api.recommend(gps, cand, rr.gd_tuple(gd), [[0, 1]] * 3, want_values=True)
    assert res["screened_index"] == want.index
    assert np.array_equal(res["candidate_values"], api.posterior_mean_mcmc(gps, cand))


def test_two_identical_candidates_give_the_first_index():
    gps, ens, a = _build(3, 30, 3, 2, SE)
    rng = np.random.default_rng(9)
    cand = rng.uniform(0, 1, size=(300, 3))
    best = int(np.argmax(ens.f(cand)[0]))
    cand = np.vstack([cand, cand[best:best + 1]])  # the maximiser a second time, behind a workgroup's worth of others
    first = best
    res = api.recommend(gps, cand, rr.gd_tuple(rr.GdParams(1, 0, 0.7, 1e-3, 1.0)), [[0, 1]] * 3, want_values=True)
    v = res["candidate_values"]
    assert v[first] == v[-1] == v.max() and res["screened_index"] == first


def _check_descent(gps, ens, gd, bounds, cand, S, what):
    res = api.recommend(gps, cand, rr.gd_tuple(gd), bounds, num_fidelity=ens.num_fidelity, num_starts=S, want_values=True,
                        want_path=True)
    want = rr.extended(ens, gd, bounds, cand, S)
    starts = rr.top_indices(res["candidate_values"], S)
    steps = rr.step_sizes(gd)
    T, k = gd.max_num_steps, rr.averaging_window(gd)
    worst = 0.0
    for s in range(S):
        path = res["path"][s]
        assert np.array_equal(path[0], cand[starts[s]]), what  # the start, exactly
        for i in range(1, T + 1):
            gnorm = float(np.max(np.abs(ens.f(path[i - 1][None, :], True)[1])))
            bound = steps[i - 1] * 1e-10 * max(1.0, gnorm)
            err = float(np.max(np.abs(path[i] - want.F(path[i - 1], i))))
            worst = max(worst, err / bound)
            assert err <= bound, (what, s, i, err, bound)
        mean = np.sum(path[T - k + 1:].astype(LD), axis=0) / LD(k)
        assert np.max(np.abs(res["end_points"][s] - mean)) <= k * 2.0 ** -52 * np.max(np.abs(path)), what
        assert np.all(path >= np.asarray(bounds)[:, 0]) and np.all(path <= np.asarray(bounds)[:, 1])
    print("%s: worst step error / bound %.3g" % (what, worst))
    return res, want


@pytest.mark.parametrize("T,averaged,gamma", [(1, -1, 0.0), (1, 3, 0.7), (6, 0, 0.7), (6, 3, 0.0), (6, 11, 0.7), (40, 3, 0.7),
                                              (40, -1, 0.0), (40, 45, 0.7)])
def test_descent_follows_the_map_step_by_step(T, averaged, gamma):
    gps, ens, a = _build(21, 30, 3, 3, MATERN)
    rng = np.random.default_rng(T + averaged)
    bounds = [[0.0, 1.0]] * 3
    # every candidate is a start: one 1e-3 from a face, one on a face, three in the interior
    cand = rng.uniform(0.2, 0.8, size=(5, 3))
    cand[0, 1] = 1.0 - 1e-3
    cand[1, 2] = 0.0
    res, want = _check_descent(gps, ens, rr.GdParams(T, averaged, gamma, 0.05, 0.02), bounds, cand, 5,
                               "T=%d averaged=%d gamma=%g clamped" % (T, averaged, gamma))
    on_face = int(np.where(rr.top_indices(res["candidate_values"], 5) == 1)[0][0])
    assert np.all(res["path"][on_face][:, 2] == 0.0)  # distance 0: that coordinate's step is exactly 0
    near = int(np.where(rr.top_indices(res["candidate_values"], 5) == 0)[0][0])
    limit = 0.02 * (1.0 - res["path"][near][0, 1])
    assert abs(abs(res["path"][near][1, 1] - res["path"][near][0, 1]) - limit) <= 1e-9 * limit  # the clamp is active
    # small pre_mult in the interior: the clamp is inactive
    _check_descent(gps, ens, rr.GdParams(T, averaged, gamma, 1e-3, 1.0), bounds, cand[2:], 3,
                   "T=%d averaged=%d gamma=%g free" % (T, averaged, gamma))


def test_descent_with_a_fidelity_coordinate_and_with_derivative_observations():
    gps, ens, a = _build(22, 25, 3, 2, MATERN, (), 1)
    rng = np.random.default_rng(4)
    _check_descent(gps, ens, rr.GdParams(6, 3, 0.7, 0.02, 0.5), [[0.0, 1.0]] * 2, rng.uniform(0.1, 0.9, size=(4, 2)), 2, "f=1")
    gps, ens, a = _build(23, 20, 3, 2, SE, (0, 2))
    _check_descent(gps, ens, rr.GdParams(6, 3, 0.7, 0.02, 0.5), [[0.0, 1.0]] * 3, rng.uniform(0.1, 0.9, size=(4, 3)), 2, "g=2")
    gps, ens, a = _build(24, 20, 9, 16, MATERN)
    _check_descent(gps, ens, rr.GdParams(6, 3, 0.7, 0.02, 0.5), [[0.0, 1.0]] * 9, rng.uniform(0.1, 0.9, size=(4, 9)), 1, "d=9 E=16")


def test_a_start_does_not_depend_on_the_other_starts():
    gps, ens, a = _build(2, 25, 2, 2, SE)
    rng = np.random.default_rng(1002)
    cand = np.vstack([rng.uniform(0, 1, size=(5, 2)), a["X"]])
    gd = rr.GdParams(8, -1, 0.0, 0.02, 1.0)
    want = rr.extended(ens, gd, [[0, 1]] * 2, cand, 3)
    print("margins %s" % (want.margins,))
    assert min(want.margins) >= MARGIN
    one = api.recommend(gps, cand, rr.gd_tuple(gd), [[0, 1]] * 2, num_starts=1, want_path=True)
    three = api.recommend(gps, cand, rr.gd_tuple(gd), [[0, 1]] * 2, num_starts=3, want_path=True)
    assert np.array_equal(one["path"][0], three["path"][0]) and np.array_equal(one["end_points"][0], three["end_points"][0])
    assert np.array_equal(three["point"], three["end_points"][want.winner]) and three["refined"] == want.refined


# tests/test_recommend_reference.py's cases: the descent improves on the screened candidate / a large pre_mult makes it end worse
@pytest.mark.parametrize("seed,E,cov,derivs,gd,refined", [(1, 3, MATERN, (), rr.GdParams(12, 4, 0.7, 0.05, 0.5), True),
                                                          (8, 4, SE, (1,), rr.GdParams(4, 0, 0.7, 50.0, 1.0), False)])
def test_keep_or_fall_back(seed, E, cov, derivs, gd, refined):
    n, d = (30, 3) if seed == 1 else (24, 3)
    members, a = rr.make_ensemble(seed, n, d, E, cov, derivs)
    ens = rr.Ensemble(members, 0)
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=cov) for e in range(E)]
    rng = np.random.default_rng(1000 + seed)
    C_ = 40 if seed == 1 else 35
    cand = np.vstack([rng.uniform(0, 1, size=(C_ - n, d)), a["X"]])
    want = rr.extended(ens, gd, [[0, 1]] * d, cand, 1)
    print("margins %s" % (want.margins,))
    assert min(want.margins) >= MARGIN and want.refined == refined
    res = api.recommend(gps, cand, rr.gd_tuple(gd), [[0, 1]] * d, want_values=True)
    assert res["refined"] == refined and res["screened_index"] == want.index
    if refined:
        assert np.array_equal(res["point"], res["end_points"][0])
    else:
        assert np.array_equal(res["point"], cand[want.index]) and res["value"] == res["candidate_values"][want.index]
    assert res["value"] == api.posterior_mean_mcmc(gps, res["point"][None, :])[0]
    assert abs(res["value"] - float(want.value)) <= 1e-8 * max(1.0, abs(float(want.value)))


def test_python_layers_return_what_the_entry_points_return():
    n, d, E, nf = 20, 3, 3, 1
    members, a = rr.make_ensemble(31, n, d, E, MATERN)
    hyp = np.array(a["hypers"])
    noise = np.array(a["noises"])
    mc = GPP.GaussianProcessMCMC(list(hyp.ravel()), list(noise.ravel()), list(a["X"].ravel()), list(a["y"].ravel()), [], E, 0, d, n)
    before = [g.mean(a["X"][:4] + 0.01) for g in mc._dev.gps]
    rng = np.random.default_rng(3)
    cand = rng.uniform(0, 1, size=(50, d - nf))
    bounds = [[0.0, 1.0]] * (d - nf)
    gd = rr.GdParams(6, 3, 0.7, 0.02, 0.5)
    res = api.recommend(mc._dev, cand, rr.gd_tuple(gd), bounds, num_fidelity=nf)
    point = posterior_mean_mcmc.recommend_point(mc, bounds, cand, gd, num_fidelity=nf)
    assert np.array_equal(point, np.concatenate([res["point"], [1.0]]))
    op = types.SimpleNamespace(optimizer_parameters=GPP.GradientDescentParameters(1, 6, 1, 3, 0.7, 0.02, 0.5, 1e-10), domain_type=0)
    flat = GPP.posterior_mean_mcmc_optimization(mc, nf, op, list(np.ravel(bounds)), list(cand.ravel()), 50)
    assert np.array_equal(np.array(flat), res["point"])
    x = cand[5]
    value, grad = api.posterior_mean_mcmc(mc._dev, x[None, :], nf, want_grad=True)
    ps = posterior_mean_mcmc.PosteriorMeanMCMC(mc, nf)
    ps.current_point = x
    assert ps.problem_size == d - nf and ps.compute_objective_function() == value[0]
    assert np.array_equal(ps.compute_grad_objective_function(), grad)
    assert GPP.compute_posterior_mean_mcmc(mc, nf, list(x)) == value[0]
    assert np.array_equal(GPP.compute_grad_posterior_mean_mcmc(mc, nf, list(x)), grad[0])
    assert np.array_equal(GPP.evaluate_posterior_mean_mcmc_at_point_list(mc, nf, list(cand.ravel()), 50),
                          api.posterior_mean_mcmc(mc._dev, cand, nf))
    # against the mean over the members of the single-GP entry point
    ducks = [types.SimpleNamespace(dim=d, _dev=g) for g in mc._dev.gps]
    want = sum(GPP.compute_posterior_mean(g, nf, list(x)) for g in ducks) / E
    assert abs(value[0] - want) <= 1e-10 * max(1.0, abs(want))
    # no handle was modified
    after = [g.mean(a["X"][:4] + 0.01) for g in mc._dev.gps]
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
