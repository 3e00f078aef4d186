"""tests/paths_reference.py (the checker of tests/test_gpu_paths.py) held to the properties of pathwise conditioning, its two
arithmetics to each other, and the entry points' refusals and the wrappers' table draws through the library without a device.

E[f_s(x)] = mu(x) exactly for every number of features, and f_s(X_j) = y_j - s z_sj - s^2 v_sj is an algebraic identity: the two make
the checks of the construction sharp.  Every test prints the figures it saw (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import kg1_reference as k1
import paths_reference as pp
import pm_members_reference as pr
import recommend_reference as rr
from cornell_moe_amd import _lib
from cornell_moe_amd import build as moe_build

LD, SE, MATERN = pp.LD, pp.SE, pp.MATERN
MARGIN = 1e-7


def _member(seed, n, d, cov, M, S, T, table_seed=None):
    _, a = rr.make_ensemble(seed, n, d, 1, cov, (), dtype=np.float64)
    tab = pp.draw_tables(cov, d, n, 1, M, S, 100 + seed if table_seed is None else table_seed)
    model = k1.Model(cov, a["hypers"][0], a["X"], a["y"], a["noises"][0], T=T)
    return pp.Paths(model, a["y"], tab["frequencies"], tab["phases"], tab["weights"][0], tab["noise_normals"][0]), model, a


@pytest.mark.parametrize("cov", [SE, MATERN])
@pytest.mark.parametrize("n,d,M", [(20, 3, 64), (300, 3, 257)])
def test_paths_interpolate_the_noised_data(cov, n, d, M):
    """f_s(X_j) = y_j - s z_sj - s^2 v_sj in long double"""
    paths, model, a = _member(3, n, d, cov, M, 3, LD)
    want = paths.y[None, :] - paths.sigma * paths.z - LD(model.noise) * paths.v
    err = float(np.max(np.abs(paths.values(model.X) - want)))
    print("n=%d d=%d M=%d cov=%d: identity error %.3g" % (n, d, M, cov, err))
    assert err <= 1e-14


@pytest.mark.parametrize("cov", [SE, MATERN])
@pytest.mark.parametrize("M", [2048, 256])
@pytest.mark.parametrize("n,d", [(20, 3), (40, 6)])
def test_mean_and_variance_of_many_paths(cov, M, n, d):
    """the mean of 4000 paths lies within 5 standard errors of mu for every M; at M = 2048 their variance within [0.7, 1.4] of the
    exact posterior variance (no factor sqrt 2, alpha or sigma is missing; not a check of accuracy)"""
    S = 4000
    paths, model, a = _member(7, n, d, cov, M, S, np.float64)
    pts = np.random.default_rng(11).uniform(0.05, 0.95, size=(8, d))
    f = paths.values(pts)  # [S][8]
    kx = model.cov(model.X, pts)
    mu = model.mean + kx.T @ model.kinvy
    vx = model.fwd(kx)
    var = model.alpha - np.sum(vx * vx, axis=0)
    z = np.abs(f.mean(axis=0) - mu) / (f.std(axis=0, ddof=1) / np.sqrt(S))
    ratio = f.var(axis=0, ddof=1) / var
    print("cov=%d M=%d n=%d d=%d: |mean - mu| in standard errors max %.2f; variance ratio %.2f .. %.2f" % (
        cov, M, n, d, z.max(), ratio.min(), ratio.max()))
    assert z.max() <= 5.0
    if M == 2048:
        assert 0.7 <= ratio.min() and ratio.max() <= 1.4


@pytest.mark.parametrize("cov", [SE, MATERN])
def test_gradient_against_central_differences(cov):
    paths, model, a = _member(5, 25, 4, cov, 100, 3, LD)
    x = np.random.default_rng(2).uniform(0.2, 0.8, size=(2, 4))
    g = paths.grads(x)
    h, worst = 1e-6, 0.0
    for c in range(2):
        for k in range(4):
            e = np.zeros(4)
            e[k] = h
            num = (paths.values(x[c] + e)[:, 0] - paths.values(x[c] - e)[:, 0]) / LD(2 * h)
            worst = max(worst, float(np.max(np.abs(num - g[:, c, k]))))
    print("cov=%d: gradient against central differences %.3g" % (cov, worst))
    assert worst <= 1e-8  # (the h^2 f''' / 6 of the difference quotient at h = 1e-6, with room for |f'''| up to 1e4)


@pytest.mark.parametrize("case", pp.DESCENT_CASES, ids=lambda c: "seed%d-n%d-d%d-E%d-cov%d-M%d-S%d" % c[:7])
def test_descent_case_margins(case):
    members, a, tab, bounds, cand = pp.case_problem(case, LD)
    worst = np.inf
    for paths in members:
        for s in range(case[6]):
            worst = min(worst, pr.min_margin(pp.run(paths, s, case[8], bounds, cand)))
    print("smallest decision margin %.3g" % worst)
    assert worst >= MARGIN


def test_the_cases_reach_every_padded_dimension_and_the_split_k_side_with_many_columns():
    from test_ei1_reference import padded_dim
    assert {padded_dim(c[2]) for c in pp.EVAL_CASES} == {4, 8, 12, 16, 24, 32}
    assert {padded_dim(c[2]) for c in pp.DESCENT_CASES} == {4, 8, 12, 16, 24, 32}
    assert any(padded_dim(c[2]) in (8, 16) and c[3] == 3 for c in pp.EVAL_CASES)
    assert any(c[1] >= 128 and c[6] > 64 for c in pp.EVAL_CASES)  # (n on the split-K side, more than 64 columns)


def measure_cache_gap():
    """(value, gradient): the float64-against-long-double difference of CACHE_CASE at its points, as paths_reference.gap() measures
    EVAL_CASES -- about a minute for the long-double factor of 3600 rows, so paths_reference.CACHE_GAP records the result and no
    test calls this"""
    m64, _, _, _, pts, _ = pp.cache_problem(np.float64)
    mld = pp.cache_problem(LD)[0]
    want, got = mld[0].values(pts), m64[0].values(pts)
    wg, gg = mld[0].grads(pts), m64[0].grads(pts)
    return (float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want.astype(np.float64))))),
            float(np.max(np.abs(gg - wg)) / max(1.0, float(np.max(np.abs(wg))))))


def test_the_rows_behind_the_cache_carry_every_checked_value():
    """at every (path, point) of CACHE_CASE the rows j >= 3584 add at least 1e-3 to f_s: a device that drops, repeats or mis-indexes
    them misses the value by ten million times tests/test_gpu_paths.py's bound"""
    members, a, tab, bounds, pts, rows = pp.cache_problem(np.float64)
    n, S, C_ = pp.CACHE_CASE[1], pp.CACHE_CASE[6], pp.CACHE_CASE[7]
    assert n > pp.ROW_CACHE and S > 8 and len(members) == 1 and pp.CACHE_CASE[5] == 4096
    assert np.all(rows >= pp.ROW_CACHE) and len(set(rows.tolist())) == C_ and float(np.max(np.abs(pts - a["X"][rows]))) <= 0.02
    tail = np.abs(pp.tail_rows(members[0], pts))
    assert tail.shape == (S, C_)
    print("n = %d: the rows behind %d add between %.3g and %.3g to f_s; recorded float64 - long double %.3g" % (
        n, pp.ROW_CACHE, float(tail.min()), float(tail.max()), pp.CACHE_GAP))
    assert float(tail.min()) >= 1e-3
    # the bound the device is held to stays far below what the rows carry
    assert 0.0 < pp.CACHE_GAP and max(pp.tolerance(), 4.0 * pp.CACHE_GAP) <= 1e-4 * float(tail.min())


def test_the_two_arithmetics_agree():
    g = pp.gap()
    print("gap %.3g, device tolerance %.3g" % (g, pp.tolerance()))
    assert g <= 2.5e-11
    assert pp.tolerance() == 1e-10


# ---- the ABI (fails on a library without the entry points) ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_new_symbols_resolve_and_are_declared(lib):
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moe_hip.h")
    with open(header) as fh:
        text = fh.read()
    for name in ("moe_gp_paths_evaluate", "moe_gp_paths_minimize"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and ("int %s(" % name) in text


def _gd(max_num_steps=5, max_num_restarts=1, domain_type=0):
    g = _lib.GdParams()
    g.num_multistarts, g.max_num_steps, g.max_num_restarts, g.num_steps_averaged = 1, max_num_steps, max_num_restarts, 2
    g.gamma, g.pre_mult, g.max_relative_change, g.tolerance, g.domain_type = 0.0, 1.0, 0.1, 1e-10, domain_type
    return g


def test_bad_arguments_are_refused_without_a_device(lib):
    """the documented codes and payloads in the header's order: everything that needs no handle is checked before one is touched"""
    err = _lib.MoeError()
    p = np.zeros(8).ctypes.data_as(_lib.dp)
    none = (C.c_void_p * 1)(None)  # an ensemble of one NULL handle
    B, R = _lib.MOE_ERR_BOUNDS, _lib.MOE_ERR_RUNTIME

    def ev(gps, E, M, S, C_, tables=p, values=p):
        return lib.moe_gp_paths_evaluate(gps, E, tables, p, M, p, p, S, p, C_, 0, values, None, C.byref(err))

    def mn(gps, E, M, S, C_, gd, tables=p, best=p):
        return lib.moe_gp_paths_minimize(gps, E, tables, p, M, p, p, S, C.byref(gd), p, p, C_, best, None, None, None, None, None,
                                         C.byref(err))

    for call in (lambda *a, **k: ev(*a, **k), lambda gps, E, M, S, C_, **k: mn(gps, E, M, S, C_, _gd(), **k)):
        assert call(None, 1, 8, 1, 4) == R
        assert call(none, 1, 0, 1, 4) == B and tuple(err.payload) == (0.0, 1.0, 4096.0)
        assert call(none, 1, 4097, 1, 4) == B and tuple(err.payload) == (4097.0, 1.0, 4096.0)
        assert call(none, 1, 8, 0, 4) == B and tuple(err.payload) == (0.0, 1.0, 1024.0)
        assert call(none, 1, 8, 1025, 4) == B and tuple(err.payload) == (1025.0, 1.0, 1024.0)
        assert call(none, 0, 8, 1, 4) == B and tuple(err.payload) == (0.0, 1.0, 1024.0)
        assert call(none, 1025, 8, 1, 4) == B and tuple(err.payload) == (1025.0, 1.0, 1024.0)
        assert call(none, 64, 8, 1024, 4) == B and tuple(err.payload) == (65536.0, 1.0, 65535.0)
        assert call(none, 1, 0, 0, 0) == B and b"num_features" in err.message  # the first in the order
        assert call(none, 1, 8, 1, 4, tables=None) == R and b"NULL argument" in err.message
        assert call(none, 1, 8, 1, 0) == B and tuple(err.payload)[:2] == (0.0, 1.0)
        assert call(none, 1, 8, 1, 4) == R and b"NULL GP handle" in err.message
    assert ev(none, 1, 8, 1, 4, values=None) == R and b"NULL argument" in err.message
    assert mn(none, 1, 8, 1, 4, _gd(), best=None) == R and b"NULL argument" in err.message
    assert mn(none, 1, 8, 1, 4, _gd(max_num_steps=0)) == B and b"max_num_steps" in err.message
    assert mn(none, 1, 8, 1, 4, _gd(max_num_restarts=0)) == B and b"max_num_restarts" in err.message
    assert mn(none, 1, 8, 1, 4, _gd(domain_type=1)) == B and b"tensor-product" in err.message
    assert tuple(err.payload) == (1.0, 0.0, 0.0)
    assert lib.moe_gp_paths_evaluate(none, 1, p, p, 0, p, p, 1, p, 4, 0, p, None, None) == B  # (no error record to fill)


def test_table_draws_are_deterministic_and_shaped(lib):
    from cornell_moe_amd import posterior_paths
    for cov in (SE, MATERN):
        a = posterior_paths.draw_path_tables(cov, 3, 11, 2, 16, 5, 42)
        b = posterior_paths.draw_path_tables(cov, 3, 11, 2, 16, 5, 42)
        c = posterior_paths.draw_path_tables(cov, 3, 11, 2, 16, 5, 43)
        assert a["frequencies"].shape == (16, 3) and a["phases"].shape == (16,)
        assert a["weights"].shape == (2, 5, 16) and a["noise_normals"].shape == (2, 5, 11)
        assert all(np.array_equal(a[k], b[k]) for k in a) and not any(np.array_equal(a[k], c[k]) for k in a)
        assert np.all((a["phases"] >= 0.0) & (a["phases"] < 2.0 * np.pi)) and all(np.all(np.isfinite(v)) for v in a.values())
    se = posterior_paths.draw_path_tables(SE, 3, 11, 2, 16, 5, 42)["frequencies"]
    assert not np.array_equal(se, a["frequencies"])  # Matern-5/2 rescales the same normals, feature by feature
    ratio = a["frequencies"] / se
    assert np.allclose(ratio, ratio[:, :1]) and np.all(ratio > 0)
    with pytest.raises(ValueError):
        posterior_paths.draw_path_tables(7, 3, 11, 2, 16, 5, 42)


def test_python_layers_exist():
    from cornell_moe_amd import api, posterior_paths, random_features
    assert callable(api.paths_evaluate) and callable(api.paths_minimize)
    assert callable(posterior_paths.thompson_sampling_batch) and callable(posterior_paths.sample_min_values_from_paths)
    assert callable(posterior_paths.PosteriorPaths) and callable(random_features.sample_from_global_optima)
    assert "pathwise" in random_features.sample_from_global_optima.__doc__
