"""The log expected improvement per unit cost on the device (csrc/logeipc1.hip: moe_log_ei_per_cost_mcmc,
moe_log_ei_per_cost_mcmc_multistart, moe_log_ei_per_cost_mcmc_suggest) against the long-double restatement of
tests/eipc_reference.py on eipc_reference.RUNS, whose inputs tests/test_eipc_reference.py qualifies on the CPU (float64 within
2.5e-11 of long double, the pending points moving a value by at least 1e-5, the two-basin problem's margin).

Tolerances: tests/test_gpu_logcei1.py's, the chains being the same kernels -- |value - want| <= 1e-10 max(1, |want|), |grad -
want|_inf <= 1e-10 max(1, |want|_inf), every log factor like the value.  Everything else is bit for bit: ensemble-wide launches on
against off, value-only against value + gradient, a candidate alone against itself in a batch and across the pass boundary, an
empty pending list against none, exponent 0 against api.log_ei_constrained_ensemble, one member against the left-to-right sum of
its log factors, the ascent against a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch against calls
of the ascent fed their predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.30
records those of the first run."""
import ctypes as C

import numpy as np
import pytest

import cei1_reference as cr
import eipc_reference as pr
import logcei1_reference as lr
from cornell_moe_amd import _lib, api
from test_gpu_logcei1 import _Launches, _ascent_inputs, _host_loop, _same_run

pytestmark = pytest.mark.gpu

LD = pr.LD
dp = _lib.dp
BOUND = 1e-10


class _Device(object):
    """the GPs of an eipc_reference problem on the device: obj [E], cons [K][E], cost [E]"""

    def __init__(self, p):
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, list(g.derivs), cov_type=g.cov_type) for g in row] for row in p.gps]
        K = len(p.gps[0]) - 2
        self.obj = [row[0] for row in self.all]
        self.cons = [[row[1 + k] for row in self.all] for k in range(K)]
        self.cost = [row[-1] for row in self.all]
        self.tau = list(p.thresholds[:K])

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, alpha, pending="problem", **kw):
    pending = p.pending if isinstance(pending, str) else pending
    return api.log_ei_per_cost_ensemble(D.obj, D.cons, p.thresholds, D.cost, alpha, points, p.best, points_being_sampled=pending, **kw)


def _raw(obj, cons, tau, cost, alpha, best, points, pending, want_grad=1):
    """moe_log_ei_per_cost_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array.
    Returns (code, payload, value, grad)."""
    arr, E, d, keep, carr, K, tau, costarr, a, best = api._ei_per_cost_members(obj, cons, tau, cost, alpha, best)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    value, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    rc = _lib.load().moe_log_ei_per_cost_mcmc(arr, E, carr, K, tau.ctypes.data_as(dp) if K else None, costarr, a, best.ctypes.data_as(dp),
                                              pend.ctypes.data_as(dp), pend.shape[0] - 1, pts.ctypes.data_as(dp), len(pts), want_grad,
                                              value.ctypes.data_as(dp), grad.ctypes.data_as(dp), None, C.byref(err))
    return rc, tuple(err.payload), value, grad


def _errors(value, grad, logs, want):
    """the worst relative errors of candidates' values, gradients and log factors against Results"""
    e_v = max(abs(value[i] - float(w.value)) / max(1.0, abs(float(w.value))) for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(w.grad)))) for i, w in enumerate(want))
    e_f = max(abs(logs[e, r, i] - float(f)) / max(1.0, abs(float(f))) for i, w in enumerate(want) for e, row in enumerate(w.log_factors)
              for r, f in enumerate(row))
    return e_v, e_g, e_f


# ---- 1. value, gradient and log factors against long double; 2. the bits of one call ----
@pytest.mark.parametrize("case,shift,alpha", pr.RUNS, ids=pr.RUN_IDS)
def test_against_the_long_double_restatement(case, shift, alpha):
    p, want = pr.expected(case, shift, alpha, LD)
    D = _Device(p)
    C_, d = p.points.shape
    G = 1 + case.K  # (the case's K is K + 1)
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, alpha, want_log_factors=True))
    value, grad, logs = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and logs.shape == (case.E, G, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(logs))
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    low = min(a for w in want for row in w.args for a in row)
    print("%s %s alpha %g: value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds 1e-10); lowest c or z %.1f, "
          "lowest value %.1f, largest |grad| %.3g, cost terms %.3g to %.3g" % (
              case.name, shift, alpha, e_v, e_g, e_f, low, float(value.min()), float(np.max(np.abs(grad))), float(logs[:, -1].min()),
              float(logs[:, -1].max())))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND, (case.name, shift, alpha, e_v, e_g, e_f)
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, alpha, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], alpha, want_log_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], logs[:, :, i]), (case.name, i)
    # no pending point through the symbol's pending arguments against None
    rc, _, raw_v, raw_g = _raw(D.obj, D.cons, p.thresholds, D.cost, alpha, p.best, p.points, p.pending[:0])
    none = _eval(D, p, p.points, alpha, pending=None)
    assert rc == 0 and np.array_equal(raw_v, none[0]) and np.array_equal(raw_g, none[1])
    if case.p:
        assert not np.array_equal(none[0], value)
    D.close()


_N8 = cr.Case("eipc_e1_k1_d2_n8_p2_two_passes", 70, 1, 2, 2, ((8, 8, 8),), 2, (), "median", (0.0, 0.0), None, 4097, None)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    """one candidate more than a pass against the same candidates in two calls"""
    per_pass = _lib.load().moe_ei1_pass_size(8)
    assert per_pass == 4096 and _N8.C == per_pass + 1
    p = pr.make_problem(_N8)
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, 1.0, want_log_factors=True)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    assert np.array_equal(_eval(D, p, p.points, 1.0, want_grad=False), value)
    assert np.array_equal(value, (logs[0, 0] + logs[0, 1]) + logs[0, 2])
    first = _eval(D, p, p.points[:per_pass], 1.0, want_log_factors=True)
    last = _eval(D, p, p.points[per_pass:], 1.0, want_log_factors=True)
    for got, a, b in zip((value, grad, logs), first, last):
        assert np.array_equal(got, np.concatenate([a, b], axis=-1 if got.ndim == 3 else 0))
    checked = [0, per_pass - 1, per_pass]
    members = pr.ensemble(p, 1.0, LD)
    e_v, e_g, e_f = _errors(value[checked], grad[checked], logs[:, :, checked], [pr.evaluate(members, p.points[i]) for i in checked])
    print("%s: value error %.3g, gradient error %.3g, log factor error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g, e_f))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    D.close()


# ---- 3. exponent 0 is the log constrained expected improvement ----
@pytest.mark.parametrize("case", [pr.ENSEMBLE, pr.K0_ENSEMBLE], ids=["e3_k2", "e3_k0"])
def test_exponent_zero_is_the_log_constrained_expected_improvement_bit_for_bit(case):
    p = pr.make_problem(case)
    D = _Device(p)
    K = len(D.cons)
    for pending in (p.pending, None):
        value, grad, logs = _eval(D, p, p.points, 0.0, pending=pending, want_log_factors=True)
        want_v, want_g, want_l = api.log_ei_constrained_ensemble(D.obj, D.cons if K else None, D.tau if K else None, p.points, p.best,
                                                                 points_being_sampled=pending, want_log_factors=True)
        assert np.array_equal(value, want_v) and np.array_equal(grad, want_g)
        assert logs.shape == (case.E, 2 + K, len(p.points)) and np.array_equal(logs[:, :1 + K], want_l)
        assert np.all(logs[:, -1] == 0.0)
        one = _eval(D, p, p.points, 1.0, pending=pending, want_grad=False)
        assert np.min(np.abs(one - value)) > 1e-3  # (the cost is not ignored at another exponent)
    D.close()


# ---- 4. one member ----
@pytest.mark.parametrize("case", [pr.SMALLEST, pr.K0_ENSEMBLE, pr.ENSEMBLE], ids=["k0", "k0_member_1", "k2_member_1"])
def test_one_member_is_the_left_to_right_sum_of_its_log_factors_bit_for_bit(case):
    p0 = pr.make_problem(case)
    e = min(1, case.E - 1)
    p = p0._replace(gps=p0.gps[e:e + 1], best=p0.best[e:e + 1])
    D = _Device(p)
    value, grad, logs = _eval(D, p, p.points, 1.0, want_log_factors=True)
    total = logs[0, 0]
    for r in range(1, logs.shape[1]):
        total = total + logs[0, r]
    assert logs.shape[0] == 1 and logs.shape[1] == len(p.gps[0]) and np.array_equal(value, total)
    D.close()


# ---- 5. the ascent against the host-driven loop; greedy batches ----
def test_the_ascent_is_the_host_driven_loop_bit_for_bit():
    p = pr.make_problem(pr.ENSEMBLE)  # E = 3, K = 2
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], lr.STALL_GD[7])
    assert gd == lr.STALL_GD
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, 1.0, pending=pending, want_grad=g), starts, gd, bounds)
    plain = api.log_ei_per_cost_multistart(D.obj, D.cons, D.tau, D.cost, 1.0, gd, bounds, p.best, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.log_ei_per_cost_multistart(D.obj, D.cons, D.tau, D.cost, 1.0, gd, bounds, p.best, starts, want_path=True,
                                                 points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    without = api.log_ei_constrained_multistart(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, points_being_sampled=pending)
    print("%d kept starts, steps taken %s, value %.12g against the best start's %.12g; without the cost the ascent ends at %s, with it at %s"
          % (len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max(), without["point"],
             want["point"]))
    assert want["found"] and len(want["kept_index"]) == len(starts) and int(want["steps_taken"].max()) > 0
    assert want["value"] >= want["start_values"].max()
    D.close()


def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    p = pr.make_problem(pr.ENSEMBLE)
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], lr.STALL_GD[7])
    pending, q = p.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.log_ei_per_cost_multistart(D.obj, D.cons, D.tau, D.cost, 1.0, gd, bounds, p.best, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ei_per_cost_suggest(D.obj, D.cons, D.tau, D.cost, 1.0, gd, bounds, p.best, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) >= 1e-3
    D.close()


# ---- 6. cost changes the answer ----
def test_the_cost_moves_the_suggestion_to_the_cheap_basin():
    tb = pr.two_basin()
    margin, s, diff = pr.two_basin_margin()
    p = tb.problem
    D = _Device(p)
    got = api.log_ei_per_cost_multistart(D.obj, None, None, D.cost, 1.0, tb.gd, tb.bounds, p.best, tb.starts)
    x = got["point"]
    one, zero = pr.ensemble(p, 1.0, LD), pr.ensemble(p, 0.0, LD)
    gap = float(pr.evaluate(one, x).value - pr.evaluate(one, pr.mirrored(x)).value)
    a, b = pr.evaluate(zero, x).value, pr.evaluate(zero, pr.mirrored(x)).value
    print("two basins: the ascent ends at %s with value %.9g; long double value - mirrored value %.6g at alpha = 1 (margin %.6g), %.3g "
          "at alpha = 0" % (x, got["value"], gap, margin, float(a - b)))
    assert got["found"] and x[0] < 0.5
    assert gap >= margin
    assert abs(float(a - b)) <= 1e-10 * max(1.0, abs(float(a)))
    # the device agrees with itself on the mirror images at alpha = 0 to the bound of the comparison with long double
    v0 = api.log_ei_per_cost_ensemble(D.obj, None, None, D.cost, 0.0, np.vstack([x, pr.mirrored(x)]), p.best, want_grad=False)
    assert abs(v0[0] - v0[1]) <= 2 * BOUND * max(1.0, abs(v0[0]))
    D.close()


# ---- 7. errors that need handles ----
def test_the_cost_gps_are_checked_with_the_flat_indices():
    p = pr.make_problem(pr.ENSEMBLE)  # E = 3, K = 2: flat index e 4 + role, the cost GP role 3
    D = _Device(p)
    V = _lib.MOE_ERR_INVALID_VALUE
    g = p.gps[1][3]
    other_dim = api.DeviceGP(np.append(g.hyper, g.hyper[-1]), np.hstack([g.X, g.X[:, :1]]), g.y, g.noise, cov_type=g.cov_type)
    other_list = api.DeviceGP(g.hyper, g.X, np.hstack([g.y, g.y]), list(g.noise) * 2, [1], cov_type=g.cov_type)

    def call(cost):
        return _raw(D.obj, D.cons, D.tau, cost, 1.0, p.best, p.points, p.pending)[:2]

    rc, payload = call([D.cost[0], other_dim, D.cost[2]])
    assert rc == V and payload == (4.0, 3.0, 7.0)  # (its dim, the first GP's, the flat index)
    rc, payload = call([D.cost[0], other_list, D.cost[2]])
    assert rc == V and payload == (1.0, 0.0, 7.0)  # (its number of derivatives, the first GP's, the flat index)
    rc, payload = call([D.cost[0], D.cost[1], D.obj[1]])
    assert rc == V and payload == (11.0, 4.0, 0.0)  # (the later flat index, the earlier, 0)
    rc, payload = call([D.cost[0], D.cost[0], D.cost[2]])
    assert rc == V and payload == (7.0, 3.0, 0.0)
    assert call(D.cost)[0] == 0
    other_dim.close()
    other_list.close()
    D.close()


def test_a_pending_point_listed_twice_in_a_noise_free_cost_gp_is_singular():
    """tests/test_gpu_cei1.py's construction with the noise-free GP as the cost GP of the second member: flat index 1 (2 + 1) + 2"""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    obj = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [1e-5])]
    con = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [1e-5])]
    cost = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]
    bests = [float(y.min())] * 2
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    for on in (True, False):
        with _Launches(on):
            rc, payload, _, _ = _raw(obj, [con], [0.0], cost, 1.0, bests, starts, pending)
            assert rc == _lib.MOE_ERR_SINGULAR and payload[:2] == (5.0, 3.0)
            with pytest.raises(api.SingularMatrixException) as e:
                api.log_ei_per_cost_multistart(obj, [con], [0.0], cost, 1.0, gd, [[0, 1], [0, 1]], bests, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (5, 3) and "pending point 3" in str(e.value)
    ok = api.log_ei_per_cost_ensemble(obj, [con], [0.0], cost, 1.0, starts, bests, want_grad=False, points_being_sampled=pending[:3])
    assert np.all(np.isfinite(ok))  # (the handles still answer)
    for g in obj + con + cost:
        g.close()


# ---- the wrapper ----
def test_the_wrapper_and_the_optimisation_run_end_to_end():
    import wrappers_mirror as cw
    from cornell_moe_amd import expected_improvement_constrained as eic, expected_improvement_per_cost as epc
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(8, dim))
    ys = np.sin(5.0 * X[:, 0]) + X[:, 1] ** 2
    cs = 4.0 * (np.sum((X - 0.5) ** 2, axis=1) - 0.4 ** 2)
    logcost = 2.0 * X[:, 0] + 0.5 * X[:, 1]
    hypers = np.array([[1.0, 0.3, 0.3], [1.4, 0.25, 0.4], [0.8, 0.45, 0.3]])
    models, cmodels, costmodels = [], [], []
    for vals, out in ((ys, models), (cs, cmodels), (logcost, costmodels)):
        hd = cw.HistoricalData(dim=dim, num_derivatives=0)
        hd.append_sample_points([cw.SamplePoint(X[i], [vals[i]], noise) for i in range(X.shape[0])])
        out.extend(cw.GaussianProcessMCMC(hypers, np.full((num_mcmc, 1), noise), hd, []).member_models())
    members, cmembers, costmembers = (eic._device_members(m) for m in (models, cmodels, costmodels))
    cand = rng.uniform(size=(7, dim))
    bounds, gd = [[0.0, 1.0]] * dim, (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    starts = api.latin_hypercube(31, bounds, 16)
    for cm, cmem, tau in (([cmodels], [cmembers], [0.0]), (None, None, None)):
        obj = epc.LogExpectedImprovementPerCostMCMC(models, costmodels, cost_exponent=0.7, constraint_models=cm, thresholds=tau)
        assert obj.problem_size == dim and obj.num_constraints == (1 if cm else 0) and obj.cost_exponent == 0.7
        want_v, want_g, want_l = api.log_ei_per_cost_ensemble(members, cmem, tau, costmembers, 0.7, cand, obj.best_so_far,
                                                              want_log_factors=True)
        assert np.array_equal(obj.evaluate_at_point_list(cand), want_v)
        obj.set_current_point(cand[3])
        assert obj.compute_objective_function() == want_v[3] and np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
        points, values, found = epc.multistart_log_expected_improvement_per_cost_optimization(
            models, costmodels, bounds, gd, num_multistarts=16, num_to_sample=2, cost_exponent=0.7, constraint_models=cm, thresholds=tau,
            seed=31)
        assert points.shape == (2, dim) and np.all(found) and np.all(np.isfinite(values))
        first = api.log_ei_per_cost_multistart(members, cmem, tau, costmembers, 0.7, gd, bounds, obj.best_so_far, starts)
        assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
        # the cost term is -alpha log E[cost] of predicted_cost's members, to the rounding of the two routes
        mean_cost, member_cost = epc.predicted_cost(costmodels, cand)
        assert member_cost.shape == (num_mcmc, len(cand)) and np.allclose(mean_cost, member_cost.mean(axis=0), rtol=1e-15, atol=0)
        assert np.max(np.abs(want_l[:, -1] + 0.7 * np.log(member_cost))) <= 1e-9
        if cm:
            twin = eic.ConstrainedExpectedImprovementMCMC(models, cm, tau)
            assert np.max(np.abs(obj.probability_of_feasibility(cand) - twin.probability_of_feasibility(cand))) <= 1e-10
        obj.cost_exponent = 0.0
        assert np.array_equal(obj.evaluate_at_point_list(cand), api.log_ei_constrained_ensemble(members, cmem, tau, cand, obj.best_so_far,
                                                                                                  want_grad=False))
