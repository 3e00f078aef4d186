"""Joint posterior sampling on the device: moe_gp_sample_points / moe_gp_sample_global_optima and
GPP.GaussianProcess.sample_global_optima (SamplePointsFromGP / SampleGlobalOptimaFromGP, gpp_math.cpp:1800-1870).

The fixture tests/golden/ref_sampling.npz is written by tools/make_golden_sampling.py from the unmodified reference."""
import ctypes as C
import os

import numpy as np
import pytest

from cornell_moe_amd import _lib, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sampling.npz")


def _fixture():
    assert os.path.exists(GOLDEN), "missing fixture %s (tools/make_golden_sampling.py)" % GOLDEN
    return np.load(GOLDEN)


def _case(f, i):
    return {k[len("c%d_" % i):]: f[k] for k in f.files if k.startswith("c%d_" % i)}


def _gp(c):
    return api.DeviceGP(c["hyper"], c["X"], c["y"], c["noise"], [int(v) for v in c["derivs"]], cov_type=int(c["cov_type"]))


def _assert_values(got, want):
    np.testing.assert_array_less(np.abs(got - want), 1e-10 * np.maximum(1.0, np.abs(want)))


def _semidefinite_cholesky(a):
    """ComputeCholeskyFactorL's outer-product algorithm, a failing pivot's column zeroed and the factorisation continued."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    for k in range(n):
        if a[k, k] > 1e-16:
            a[k, k] = np.sqrt(a[k, k])
            a[k + 1:, k] /= a[k, k]
            for j in range(k + 1, n):
                a[j:, j] -= a[j:, k] * a[j, k]
        else:
            a[k:, k] = 0.0
    return np.tril(a)


def test_fixture_is_present_and_small():
    f = _fixture()
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert int(f["num_cases"]) > int(f["num_regular"]) > 0


@pytest.mark.gpu
def test_sample_points_match_reference():
    f = _fixture()
    seen = set()
    exempted = 0
    for i in range(int(f["num_regular"])):
        c = _case(f, i)
        G = _gp(c)
        values, argmin, failed = G.sample_points(c["pts"], c["normals"])
        G.close()
        assert failed == 0
        _assert_values(values, c["values"])
        alpha = float(c["hyper"][0])
        for dd in range(values.shape[0]):
            two = np.sort(c["values"][dd])[:2]
            if len(two) < 2 or two[1] - two[0] > 1e-8 * np.sqrt(alpha):
                assert argmin[dd] == c["argmin"][dd], (i, dd)
            else:
                exempted += 1
        seen.add((len(c["derivs"]), int(c["cov_type"]), c["pts"].shape[0], c["normals"].shape[0]))
    assert exempted == 0  # (the committed fixture has no near-tie: tests/test_sampling_reference.py::test_fixture_has_no_near_ties)
    assert {s[0] for s in seen} == {0, 2} and {s[1] for s in seen} == {0, 1}
    assert {s[2] for s in seen} == {1, 7, 64, 65, 200} and {s[3] for s in seen} == {1, 3, 64}


@pytest.mark.gpu
def test_singular_set_follows_reference_early_stop():
    f = _fixture()
    assert api.get_reference_quirks()
    for i in range(int(f["num_regular"]), int(f["num_cases"])):
        c = _case(f, i)
        G = _gp(c)
        values, argmin, failed = G.sample_points(c["pts"], c["normals"])
        G.close()
        assert failed == int(c["rc"]) and failed > 0
        _assert_values(values, c["values"])


@pytest.mark.gpu
def test_singular_set_semidefinite_continuation_without_quirks():
    f = _fixture()
    api.set_reference_quirks(0)
    try:
        for i in range(int(f["num_regular"]), int(f["num_cases"])):
            c = _case(f, i)
            G = _gp(c)
            mu = G.mean(c["pts"])
            values, argmin, failed = G.sample_points(c["pts"], c["normals"])
            G.close()
            assert failed == int(c["rc"])
            L = _semidefinite_cholesky(c["var"])
            _assert_values(values, np.array([mu + L @ z for z in c["normals"]]))
    finally:
        api.set_reference_quirks(1)


def _far_apart_gp():
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, size=(12, 2))
    G = api.DeviceGP([1.0, 0.05, 0.05], X, rng.normal(size=(12, 1)), [1e-2])
    cand = np.array([[5.0, 5.0], [7.0, 5.0], [5.0, 7.0], [9.0, 9.0]])  # far from the data and from each other
    return G, cand


@pytest.mark.gpu
def test_argmin_minus_one_and_candidate_zero():
    G, cand = _far_apart_gp()
    z = np.zeros((1, 4))
    z[0, 0] = -50.0
    values, argmin, failed = G.sample_points(cand, z)
    assert failed == 0 and argmin[0] == -1 and values[0, 0] < values[0, 1:].min()
    pts, index, failed = G.sample_global_optima(cand[None], np.array([[-50.0, 0.0, 0.0, 0.0]]))
    assert index[0] == -1 and failed[0] == 0
    np.testing.assert_array_equal(pts[0], cand[0])
    pts, index, _ = G.sample_global_optima(cand[None], np.array([[0.0, 0.0, -50.0, 0.0]]))
    assert index[0] == 2
    np.testing.assert_array_equal(pts[0], cand[2])
    G.close()


@pytest.mark.gpu
def test_set_alone_equals_set_in_batch():
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, size=(40, 3))
    G = api.DeviceGP([1.1, 0.3, 0.25, 0.35], X, rng.normal(size=(40, 1)), [1e-3])
    for C_ in (5, 70):
        E = 6
        cand = rng.uniform(0, 1, size=(E, C_, 3))
        z = rng.normal(size=(E, C_))
        pts_b, idx_b, fail_b = G.sample_global_optima(cand, z)
        for e in range(E):
            pts_1, idx_1, fail_1 = G.sample_global_optima(cand[e:e + 1], z[e:e + 1])
            assert idx_1[0] == idx_b[e] and fail_1[0] == fail_b[e] == 0
            assert pts_1[0].tobytes() == pts_b[e].tobytes()
            # the same set through moe_gp_sample_points: the same draw, so the same winner
            v, a, _ = G.sample_points(cand[e], z[e:e + 1])
            assert a[0] == idx_b[e]
    G.close()


@pytest.mark.gpu
def test_sample_covariance_matches_posterior_variance():
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, size=(30, 2))
    G = api.DeviceGP([2.0, 0.4, 0.3], X, rng.normal(size=(30, 1)), [1e-2])
    pts = rng.uniform(0, 1, size=(8, 2))
    n = 20000
    values, _, failed = G.sample_points(pts, rng.normal(size=(n, 8)))
    assert failed == 0
    var = G.variance(pts).reshape(8, 8).T
    mu = G.mean(pts)
    dev = values - mu
    cov = dev.T @ dev / n  # the mean is known: no loss of a degree of freedom
    se = np.sqrt((np.outer(np.diag(var), np.diag(var)) + var ** 2) / n)
    assert np.all(np.abs(cov - var) < 4 * se)
    assert np.all(np.abs(values.mean(axis=0) - mu) < 4 * np.sqrt(np.diag(var) / n))
    G.close()


@pytest.mark.gpu
def test_invalid_sizes_are_bounds_errors():
    G, cand = _far_apart_gp()
    L = _lib.load()
    err = _lib.MoeError()
    vals = np.zeros(16)
    am = np.zeros(4, dtype=np.int32)
    fp = C.c_int(0)
    cp = np.ascontiguousarray(cand)
    z = np.zeros(16)
    dp = _lib.dp
    assert L.moe_gp_sample_points(G._h, cp.ctypes.data_as(dp), 0, z.ctypes.data_as(dp), 1, vals.ctypes.data_as(dp),
                                  am.ctypes.data_as(_lib.ip), C.byref(fp), C.byref(err)) == _lib.MOE_ERR_BOUNDS
    assert L.moe_gp_sample_points(G._h, cp.ctypes.data_as(dp), 4, z.ctypes.data_as(dp), 0, vals.ctypes.data_as(dp),
                                  am.ctypes.data_as(_lib.ip), C.byref(fp), C.byref(err)) == _lib.MOE_ERR_BOUNDS
    pts = np.zeros(8)
    assert L.moe_gp_sample_global_optima(G._h, cp.ctypes.data_as(dp), 4, 0, z.ctypes.data_as(dp), pts.ctypes.data_as(dp),
                                         am.ctypes.data_as(_lib.ip), am.ctypes.data_as(_lib.ip), C.byref(err)) == _lib.MOE_ERR_BOUNDS
    G.close()


@pytest.mark.gpu
def test_gpp_sample_global_optima_in_domain_and_reproducible():
    from cornell_moe_amd import GPP
    rng = np.random.default_rng(8)
    dim, n = 2, 20
    X = rng.uniform(-1, 2, size=(n, dim))
    gp = GPP.GaussianProcess([1.0, [0.5, 0.7]], list(X.ravel()), list(rng.normal(size=n)), [1e-2], [], 0, dim, n)
    bounds = [-1.0, 2.0, 0.5, 1.5]  # cppify([ClosedInterval(-1, 2), ClosedInterval(0.5, 1.5)])
    gp.set_explicit_seed(1234)
    a = gp.sample_global_optima(5, 50, bounds)
    b = gp.sample_global_optima(5, 50, bounds)
    assert len(a) == 5 * dim
    p = np.array(a).reshape(5, dim)
    assert np.all(p[:, 0] >= -1.0) and np.all(p[:, 0] <= 2.0) and np.all(p[:, 1] >= 0.5) and np.all(p[:, 1] <= 1.5)
    assert a != b  # the streams move on
    gp.set_explicit_seed(1234)
    assert gp.sample_global_optima(5, 50, bounds) == a
    assert gp.sample_global_optima(5, 50, bounds) == b
