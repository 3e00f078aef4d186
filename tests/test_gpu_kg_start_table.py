"""GPU tests (-m gpu) of the start table: without derivative observations the LDS-table wave-per-sample kernels (lane-parked and frame
line search) take the FIRST gradient of every sample's line search -- at the sample's discretised point -- from a per-evaluation table
of (1 + m)-term dot products with [1 ; beta] (kg_prep.hip: kg_start_table_kernel; kg_mc.hpp: start_from_table) instead of a pass over the
n + u points.  Checked against the plain-C oracle at test_gpu_parity.py's KG tolerances (helpers.TOL; end points 1e-8 on all but 0.2 %
of the samples; gradient passes counted as the oracle counts them, value passes never more -- test_gpu_sweep.py's relation), and for
the bit-for-bit properties the table must not disturb: lane = frame, alone = in a batch, ensemble-wide = member by member."""
import numpy as np
import pytest

from helpers import TOL

pytestmark = pytest.mark.gpu

GD_DEFAULT = (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)
# one step of one restart: the only gradient of every sample is the table's, the end point is x_c + LimitUpdate(alpha g)
GD_TABLE_ONLY = (1, 1, 1, 3, 0.0, 1.0, 0.1, 1e-10)
# a zero step size: every Armijo trial is rejected and the point restored -- the oracle's end points ARE its start points
GD_STAY = (1, 1, 1, 3, 0.0, 0.0, 0.1, 1e-10)


@pytest.fixture(scope="module")
def api():
    from cornell_moe_amd import _lib, api as moe_api
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"
    return moe_api


def _workload(seed, n, d, q, M, P, f=0, p=0, derivs=()):
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=seed, n=n, d=d, q=q, M=M, P=P, derivs=derivs, p=p)
    w.discrete = w.discrete[:, :d - f]
    w.bounds_inner = w.bounds[:2 * (d - f)]
    return w


_ORACLE = {}


def _oracle(key, w, cov, f, gd):
    """the oracle's evaluation of a case, computed once and shared"""
    if key not in _ORACLE:
        from oracle import orc
        O = orc.OrcGP(cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
        full = np.hstack([w.discrete, np.ones((w.discrete.shape[0], f))])
        best = float(O.additional_mean(full).min())
        ro = O.kg(gd, w.bounds_inner, w.discrete, w.Xq, w.Xp if w.p else None, w.M, best, w.kg_normals, num_fidelity=f)
        _ORACLE[key] = (best, ro)
    return _ORACLE[key]


def _check(rg, ro):
    print("KG rel. error %.2e, grad KG error / scale %.2e, worst end point %.2e, passes (value, gradient) device %d %d oracle %d %d" % (
        abs(rg["kg"] - ro["kg"]) / abs(ro["kg"]),
        np.abs(rg["grad"] - ro["grad"]).max() / max(float(np.abs(ro["grad"]).max()), abs(ro["kg"])),
        np.abs(rg["best_point"] - ro["best_point"]).max(), rg["mean_evals"], rg["grad_evals"], ro["mean_evals"], ro["grad_evals"]))
    assert abs(rg["kg"] - ro["kg"]) <= TOL["kg"] * abs(ro["kg"])
    scale = max(float(np.abs(ro["grad"]).max()), abs(ro["kg"]))
    assert np.abs(rg["grad"] - ro["grad"]).max() <= TOL["grad_kg"] * scale
    mism = np.abs(rg["best_point"] - ro["best_point"]).max(axis=1) > 1e-8
    assert mism.mean() <= 0.002, "fraction of samples whose end point differs by > 1e-8: %g" % mism.mean()
    assert rg["grad_evals"] == ro["grad_evals"] and rg["mean_evals"] <= ro["mean_evals"]


def _device(api, w, cov):
    return api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)


def _kg(G, w, f, gd, best, **kw):
    return G.kg(gd, w.bounds_inner, w.discrete, w.Xq, w.Xp if w.p else None, w.M, best, w.kg_normals, num_fidelity=f,
                want_best_points=True, **kw)


# n + u = 72: two tiles, the second partial; d = 3: four table rows, one of them a pad; A = u + P = 5 table rows
TABLE_ONLY = dict(seed=4101, n=70, d=3, q=2, M=64, P=3)


@pytest.mark.parametrize("cov", [0, 1], ids=["square-exponential", "matern-5/2"])
def test_only_the_table_speaks(api, cov, monkeypatch):
    """One step of one restart: a wrong table entry moves the end points at first order."""
    w = _workload(**TABLE_ONLY)
    best, ro = _oracle(("table-only", cov), w, cov, 0, GD_TABLE_ONLY)
    assert ro["grad_evals"] == w.M   # (one gradient per sample: the table's)
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    G = _device(api, w, cov)
    rg = _kg(G, w, 0, GD_TABLE_ONLY, best)
    info = G.last_kernel_info()
    assert info["variant"] == 0 and info["xlds"] == 1 and info["start_table"] == 1, info
    _check(rg, ro)
    # the end points moved: the step the table's gradient asked for was taken
    _, stay = _oracle(("table-only-stay", cov), w, cov, 0, GD_STAY)
    assert (np.abs(ro["best_point"] - stay["best_point"]).max(axis=1) > 1e-6).mean() > 0.5


@pytest.mark.parametrize("cov", [0, 1], ids=["square-exponential", "matern-5/2"])
def test_lane_and_frame_line_search_agree_bit_for_bit_on_the_table(api, cov, monkeypatch):
    """The table-only case on the lane-parked kernel and on the frame line search (MOE_KG_LANE=0; at this shape the 16-wavefront
    small-shape instantiation, and the 8-wavefront one with the small-shape sample bound lifted): one device function, one operation
    order -- sums, end points and both counters are equal."""
    w = _workload(**TABLE_ONLY)
    best, _ = _oracle(("table-only", cov), w, cov, 0, GD_TABLE_ONLY)
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    G = _device(api, w, cov)
    res = {}
    for lane in ("1", "0"):
        monkeypatch.setenv("MOE_KG_LANE", lane)
        res[lane] = _kg(G, w, 0, GD_TABLE_ONLY, best)
        info = G.last_kernel_info()
        assert info["variant"] == 0 and info["xlds"] == 1 and info["start_table"] == 1, info
        assert info["lane"] == (int(lane) if info["waves"] <= 8 else 0), info
    a, b = res["1"], res["0"]
    assert a["kg_sum"] == b["kg_sum"] and np.array_equal(a["grad_sum"], b["grad_sum"])
    assert np.array_equal(a["best_point"], b["best_point"])
    assert a["grad_evals"] == b["grad_evals"] and a["mean_evals"] == b["mean_evals"]


def test_second_scan_chunk(api, monkeypatch):
    """74 discretised points (4 union points + 70): the scan takes two chunks of 64 and some samples start from a table row beyond the
    first -- seen on the oracle's own start points (its end points under a zero step size)."""
    from oracle import orc
    w = _workload(seed=4102, n=130, d=8, q=4, M=128, P=70)
    # (the discrete points in descending order of their posterior mean: the scan's likely winners sit at the END of the set)
    mu = orc.OrcGP(1, w.alpha, w.lengths, w.X, w.y, w.noise, ()).additional_mean(w.discrete)
    w.discrete = np.ascontiguousarray(w.discrete[np.argsort(-mu, kind="stable")])
    best, ro = _oracle("chunk", w, 1, 0, GD_DEFAULT)
    _, stay = _oracle("chunk-stay", w, 1, 0, GD_STAY)
    disc = np.vstack([w.Xq, w.discrete])   # the discretised set: the union points, then the discrete points
    start = np.array([int(np.flatnonzero((disc == x).all(axis=1))[0]) for x in stay["best_point"]])
    assert (start >= 64).any(), np.bincount(start, minlength=74)
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    G = _device(api, w, 1)
    rg = _kg(G, w, 0, GD_DEFAULT, best)
    info = G.last_kernel_info()
    assert info["variant"] == 0 and info["start_table"] == 1, info
    _check(rg, ro)
    late = start >= 64
    assert np.abs(rg["best_point"][late] - ro["best_point"][late]).max() <= 1e-8


def test_fidelity_rows_gamma_and_a_second_restart(api, monkeypatch):
    """One fidelity dimension (a pinned table row), a point being sampled, gamma != 0, two restarts: the second restart starts from the
    iterate, so its first gradient is a real pass."""
    gd = (1, 4, 2, 3, 0.5, 0.8, 0.3, 1e-8)
    w = _workload(seed=4103, n=130, d=4, q=2, M=64, P=6, f=1, p=1)
    best, ro = _oracle("fidelity", w, 1, 1, gd)
    assert ro["grad_evals"] > 4 * w.M   # (the second restart ran)
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    G = _device(api, w, 1)
    rg = _kg(G, w, 1, gd, best)
    info = G.last_kernel_info()
    assert info["variant"] == 0 and info["start_table"] == 1, info
    _check(rg, ro)


def test_a_restart_alone_and_in_a_batch(api):
    """Three restarts in one call against each alone: the table's sums depend on the evaluation alone."""
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=4104, n=150, d=5, q=3, M=96, P=7, derivs=(), num_restarts=3)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, ())
    best = float(G.additional_mean(w.discrete).min())
    rb = G.kg_batch(GD_DEFAULT, w.bounds, w.discrete, w.Xq_restarts, None, w.M, best, w.kg_normals)
    assert G.last_kernel_info()["start_table"] == 1
    for e in range(3):
        r1 = G.kg(GD_DEFAULT, w.bounds, w.discrete, w.Xq_restarts[e], None, w.M, best, w.kg_normals)
        assert G.last_kernel_info()["start_table"] == 1
        assert r1["kg_sum"] == rb["kg_sum"][e] and np.array_equal(r1["grad_sum"], rb["grad_sum"][e]), e


def test_ensemble_wide_and_member_by_member(api):
    """One small KG-MCMC evaluation batch (n = 30, six members, M = 128: the suggestion's shape, which takes the table) with
    ensemble-wide launches against member-by-member launches: equal."""
    from cornell_moe_amd.workloads import make_workload
    nm, E, d, q = 6, 5, 2, 4
    w = make_workload(seed=4105, n=30, d=d, q=q, M=128, P=10, derivs=())
    rng = np.random.default_rng(4106)
    hypers = np.column_stack([w.alpha * rng.uniform(0.7, 1.4, nm)] + [w.lengths[k] * rng.uniform(0.6, 1.6, nm) for k in range(d)])
    noises = np.tile(np.asarray(w.noise, dtype=np.float64).reshape(1, -1), (nm, 1)) * rng.uniform(0.8, 1.2, (nm, 1))
    Xq_all = rng.uniform(0.05, 0.95, (E, q, d))
    disc = np.tile(w.discrete.reshape(1, -1), (nm, 1)) + 0.01 * rng.standard_normal((nm, w.discrete.size))
    best = rng.uniform(-1.0, 0.0, nm)
    G = api.DeviceGPMCMC(hypers, noises, w.X, w.y, ())
    try:
        api.set_ensemble_launches(0)
        k0, g0 = G.kg_batch(w.inner_gd, w.bounds, disc, Xq_all, None, w.M, best, w.kg_normals)
        api.set_ensemble_launches(1)
        s0 = api.ensemble_launch_stats()
        k1, g1 = G.kg_batch(w.inner_gd, w.bounds, disc, Xq_all, None, w.M, best, w.kg_normals)
        s1 = api.ensemble_launch_stats()
    finally:
        api.set_ensemble_launches(-1)
    assert all(gp.last_kernel_info()["start_table"] == 1 for gp in G.gps)
    assert s1[0] - s0[0] == 1 and s1[1] == s0[1], (s0, s1)   # (the members' chains lined up: one merged evaluation)
    assert np.all(np.isfinite(k0)) and np.abs(g0).max() > 0
    assert np.array_equal(k0, k1) and np.array_equal(g0, g1)


@pytest.mark.parametrize("tag,kw,flag", [
    ("d-KG, one observed derivative", dict(seed=4107, n=80, d=4, q=2, M=48, P=5, derivs=(2,)), None),
    ("d = 17: no coordinate table in LDS", dict(seed=4108, n=60, d=17, q=2, M=24, P=5), "wide_frame"),
], ids=["g1", "wide-frame"])
def test_paths_that_keep_their_first_pass(api, tag, kw, flag):
    """Derivative observations and the wide-frame evaluators do not take the table: they report so, and match the oracle as before."""
    w = _workload(**kw)
    best, ro = _oracle(tag, w, 1, 0, GD_DEFAULT)
    G = _device(api, w, 1)
    rg = _kg(G, w, 0, GD_DEFAULT, best)
    info = G.last_kernel_info()
    assert info["start_table"] == 0, info
    if flag is not None:
        assert info[flag] == 1, info
    _check(rg, ro)
