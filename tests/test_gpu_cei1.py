"""The constrained expected improvement on the device (csrc/cei1.hip: moe_ei_constrained_mcmc, moe_ei_constrained_mcmc_multistart,
moe_ei_constrained_mcmc_suggest) against the long-double restatement of tests/cei1_reference.py, on the cases cei1_reference.CASES
and WIDE_CASES (three members of 20, 300 and 600 rows shuffled over the roles at padded dimension 24), whose inputs
tests/test_cei1_reference.py qualifies on the CPU (float64 within 2.5e-11 scale of long double; at the checked
candidates every feasibility factor in [0.02, 0.98], the value above 1e-3 scale, the gradient above 1e-2, and the constraints and
the pending points each moving the value by far more than the bound here: a device that returned zeros, ignored the constraints or
ignored P fails).

Tolerances: tests/test_gpu_ei1.py's, the chains being the same kernels over the same lengths -- |value - want| <= 1e-10 scale,
|grad - want|_inf <= 1e-10 (at most 1e-10 scale and at most 1e-10 max(1, |want|_inf)), the factors like the value.  Everything else
is bit for bit: K = 0 against moe_ei_analytic_mcmc and its ascent, value-only against value + gradient, a candidate alone against
itself in a batch and across the pass boundary, the result against the product rule applied to `factors` on the host, ensemble-wide
launches on against off, the ascent against a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch
against calls of the ascent fed their predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md
section 5.18 records those of the first run."""
import ctypes as C
import math

import numpy as np
import pytest

import cei1_reference as cr
import kg1_reference as kr
import ms_restatement as ms
from cornell_moe_amd import _lib, api, expected_improvement_constrained as eic

pytestmark = pytest.mark.gpu

LD = cr.LD
dp, ip = _lib.dp, _lib.ip


class _Launches(object):
    """ensemble-wide launches switched on or off for a block, the environment's setting restored afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib.load().moe_set_ensemble_launches(1 if self.on else 0)

    def __exit__(self, *exc):
        _lib.load().moe_set_ensemble_launches(-1)
        return False


class _Device(object):
    """the GPs of a problem on the device: obj [E], cons [K][E]"""

    def __init__(self, p, K=None):
        K = len(p.thresholds) if K is None else K
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, list(g.derivs), cov_type=g.cov_type) for g in row[:1 + K]] for row in p.gps]
        self.obj = [row[0] for row in self.all]
        self.cons = [[row[1 + k] for row in self.all] for k in range(K)]
        self.tau = list(p.thresholds[:K])

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", best=None, **kw):
    pending = p.pending if isinstance(pending, str) else pending
    return api.ei_constrained_ensemble(D.obj, D.cons, D.tau, points, p.best if best is None else best, points_being_sampled=pending, **kw)


def _raw_eval(D, p, points, pending):
    """moe_ei_constrained_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array"""
    arr, E, d, keep, carr, K, tau, best = api._ei_constrained_members(D.obj, D.cons, D.tau, p.best)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    value, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(_lib.load().moe_ei_constrained_mcmc(arr, E, carr, K, tau.ctypes.data_as(dp) if K else None, best.ctypes.data_as(dp),
                                                   pend.ctypes.data_as(dp), pend.shape[0] - 1, pts.ctypes.data_as(dp), len(pts), 1,
                                                   value.ctypes.data_as(dp), grad.ctypes.data_as(dp), None, C.byref(err)), err)
    return value, grad


def _errors(value, grad, factors, want):
    e_v = max(abs(value[i] - float(w.value)) / w.scale for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / min(w.scale, max(1.0, float(np.max(np.abs(w.grad)))))
              for i, w in enumerate(want))
    e_f = max(abs(factors[e, r, i] - float(f)) / w.scale for i, w in enumerate(want) for e, row in enumerate(w.factors)
              for r, f in enumerate(row))
    return e_v, e_g, e_f


def _host_product(factors):
    """the documented rule on the host: A_e multiplied left to right, members added in order, divided once"""
    E, G, n = factors.shape
    out = np.zeros(n)
    for i in range(n):
        total = 0.0
        for e in range(E):
            a = float(factors[e, 0, i])
            for r in range(1, G):
                a = a * float(factors[e, r, i])
            total = a if e == 0 else total + a
        out[i] = total / float(E)
    return out


# ---- 1. value, gradient and factors against long double; the bits of one call ----
ALL_CASES = cr.CASES + cr.WIDE_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_against_the_long_double_restatement(case):
    p, want = cr.expected(case, LD)
    D = _Device(p)
    C_, d = p.points.shape
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_factors=True))
    value, grad, factors = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and factors.shape == (case.E, 1 + case.K, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(factors))
    e_v, e_g, e_f = _errors(value, grad, factors, want)
    print("%s: value error %.3g scale, gradient error %.3g, factor error %.3g scale (bounds 1e-10)" % (case.name, e_v, e_g, e_f))
    assert e_v <= 1e-10 and e_g <= 1e-10 and e_f <= 1e-10, (case.name, e_v, e_g, e_f)
    # the call's value is the product rule applied to its own factors on the host, bit for bit
    assert np.array_equal(value, _host_product(factors))
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], factors[:, :, i]), (case.name, i)
    # no pending point through the symbol's pending arguments against NULL
    raw = _raw_eval(D, p, p.points, p.pending[:0])
    none = _eval(D, p, p.points, pending=None)
    assert np.array_equal(raw[0], none[0]) and np.array_equal(raw[1], none[1])
    if case.p:
        assert not np.array_equal(none[0], value)
    D.close()


# ---- 2. K = 0 is the analytic expected improvement, bit for bit ----
MS = dict(starts=12, steps=6, restarts=2, gamma=0.7, pre_mult=1.0, max_rel=0.5)


def _ascent_inputs(d, tolerance):
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], d))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    return starts, gd, np.array([[0.0, 1.0]] * d)


def _same_run(got, want):
    for key in ("start_values", "kept_index", "path", "steps_taken", "end_points", "end_values", "point"):
        assert np.array_equal(got[key], want[key]), key
    assert got["value"] == want["value"] and got["found"] == want["found"]


def test_without_constraints_it_is_the_analytic_expected_improvement_bit_for_bit():
    p = cr.make_problem(cr.case(cr.ENSEMBLE))
    D = _Device(p, K=0)
    for pending in (p.pending, None):
        v, g, f = api.ei_constrained_ensemble(D.obj, None, None, p.points, p.best, points_being_sampled=pending, want_factors=True)
        ev, eg = api.ei_analytic_ensemble(D.obj, p.points, p.best, points_being_sampled=pending)
        assert np.array_equal(v, ev) and np.array_equal(g, eg) and f.shape == (3, 1, len(p.points))
        assert np.array_equal(v, _host_product(f))
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 0.3)
    want = api.ei_analytic_multistart(D.obj, gd, bounds, p.best, starts, want_path=True, points_being_sampled=p.pending[:2])
    got = api.ei_constrained_multistart(D.obj, None, None, gd, bounds, p.best, starts, want_path=True, points_being_sampled=p.pending[:2])
    _same_run(got, want)
    assert int(want["steps_taken"].max()) > 0
    D.close()


# ---- 3. across the pass boundary ----
_N8 = cr.Case("e1_k1_d2_n8_p2_two_passes", 44, 1, 1, 2, ((8, 8),), 2, (), "median", (0.0,), None, 4100, None)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    p = cr.make_problem(_N8)
    checked = (0, per_pass - 1, per_pass, _N8.C - 1)
    members = cr.ensemble(p, LD)
    D = _Device(p)
    for pending in (p.pending, None):
        value, grad, factors = _eval(D, p, p.points, pending=pending, want_factors=True)
        assert np.array_equal(_eval(D, p, p.points, pending=pending, want_grad=False), value)
        assert np.array_equal(value, _host_product(factors))
        for i in checked:
            v1, g1 = _eval(D, p, p.points[i:i + 1], pending=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            want = [cr.evaluate(members, p.points[i]) for i in checked]
            idx = list(checked)
            e_v, e_g, e_f = _errors(value[idx], grad[idx], factors[:, :, idx], want)
            print("%s: value error %.3g scale, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= 1e-10 and e_g <= 1e-10 and e_f <= 1e-10
    D.close()


# ---- 4. the ascent against the host-driven loop ----
def _host_loop(evaluate, starts, gd, bounds):
    """ms_restatement's optimiser, evaluations by `evaluate(points, want_grad)` on the device, updates in numpy; a dict shaped like
    api.ei_constrained_multistart's, path included (a start that is not running repeats its point)"""
    d, T, R = starts.shape[1], gd[1], gd[2]

    def value_fn(x):
        return evaluate(np.asarray(x).reshape(-1, d), False)

    seen, state = {}, {"round": -1, "points": None}

    def grad_fn(x):
        state["points"] = np.array(x, copy=True).reshape(-1, d)
        return evaluate(state["points"], True)[1].reshape(np.shape(x))

    def on_step(i, idx):
        if i == 0:
            state["round"] += 1
        seen[state["round"] * T + i] = (np.array(idx), state["points"])

    vals = np.asarray(value_fn(starts))
    order = ms.top_k_order(vals)
    K = len(order)
    ends = ms.gradient_ascent(grad_fn, gd, bounds, starts[order], on_step=on_step)
    end_vals = np.asarray(value_fn(ends))
    point, value, found = starts[order[0]].copy(), -np.inf, False
    for s in range(K):
        if end_vals[s] > value:
            point, value, found = ends[s].copy(), float(end_vals[s]), True
    path = np.empty((K, R * T + 1, d))
    steps = np.zeros(K, dtype=int)
    for k in range(K):
        took = [(g, seen[g][1][list(seen[g][0]).index(k)]) for g in sorted(seen) if k in seen[g][0]]
        steps[k] = len(took)
        row = 0
        for g, before in took:  # rows up to g hold the point before step g
            path[k, row:g + 1] = before
            row = g + 1
        path[k, row:] = ends[k]
    return {"point": point, "value": value, "found": found, "start_values": vals, "kept_index": order, "end_points": ends,
            "end_values": end_vals, "steps_taken": steps, "path": path}


# (the loose tolerance chosen on the CPU with the float64 restatement: starts stop inside a round after 4 steps, after one round of 6,
#  or run all 12; at tests/test_gpu_ei1.py's 6e-2 every start of this objective runs all 12 and no update is ever masked)
@pytest.mark.parametrize("tolerance", [1e-10, 0.3], ids=["tight", "loose"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(tolerance):
    p = cr.make_problem(cr.case(cr.ENSEMBLE))  # E = 3, K = 2
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], tolerance)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    plain = api.ei_constrained_multistart(D.obj, D.cons, D.tau, gd, bounds, p.best, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    free = api.ei_analytic_multistart(D.obj, gd, bounds, p.best, starts, points_being_sampled=pending)
    assert not np.array_equal(free["start_values"], want["start_values"])  # (nor are the constraints)
    for on in (True, False):
        with _Launches(on):
            got = api.ei_constrained_multistart(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, want_path=True,
                                                points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("tolerance %g: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"]
    if tolerance > 1e-3:
        assert int(want["steps_taken"].min()) < MS["steps"] * MS["restarts"]  # (masked steps occurred)
    else:
        assert want["value"] >= want["start_values"].max()
    none = api.ei_constrained_multistart(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, gradient_ascent=False,
                                         points_being_sampled=pending)
    best = int(np.argmax(want["start_values"]))
    assert np.array_equal(none["point"], starts[best]) and none["value"] == want["start_values"][best] and none["found"]
    D.close()


# ---- 5. greedy batches ----
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    p = cr.make_problem(cr.case(cr.ENSEMBLE))
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.ei_constrained_multistart(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.ei_constrained_suggest(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    # the effect of the believed-feasible incumbent and the conditioned variances: no pick repeats an earlier one
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) >= 1e-3
    D.close()


# ---- 6. behaviour ----
def test_an_unreachable_threshold_gives_zero_and_infinite_incumbents_give_the_probability_of_feasibility():
    p = cr.make_problem(cr.case(cr.ENSEMBLE))
    D = _Device(p)
    low = min(float(np.min(g.y)) for row in p.gps for g in row[1:]) - 100.0  # far below every posterior mean
    v, g = api.ei_constrained_ensemble(D.obj, D.cons, [low, p.thresholds[1]], p.points, p.best, points_being_sampled=p.pending)
    assert np.all(v == 0.0) and np.all(np.isfinite(g))
    inf = [math.inf] * 3
    for pending in (None, p.pending[1:]):
        if pending is not None:  # (no member believes one of these feasible: every incumbent stays +infinity)
            assert not any(m.mask.any() for m in cr.ensemble(p, np.float64, pending=pending))
        v, g, f = api.ei_constrained_ensemble(D.obj, D.cons, D.tau, p.points, inf, points_being_sampled=pending, want_factors=True)
        assert np.all(f[:, 0, :] == 1.0)
        pof = ((f[0, 1] * f[0, 2] + f[1, 1] * f[1, 2]) + f[2, 1] * f[2, 2]) / 3.0
        assert np.array_equal(v, pof) and np.all(np.isfinite(g)) and float(np.max(np.abs(g))) > 1e-3
        members = [cr.Member(row, p.thresholds, math.inf, p.pending[:0] if pending is None else pending, np.float64) for row in p.gps]
        want = [cr.evaluate(members, x) for x in p.points]
        e_v, e_g, e_f = _errors(v, g, f, want)
        print("+infinity incumbents, %d pending: value error %.3g, gradient error %.3g" % (0 if pending is None else len(pending), e_v, e_g))
        assert e_v <= 1e-9 and e_g <= 1e-9  # (against float64: the long-double comparison is test 1's)
    D.close()


# ---- 7. limits ----
def test_nine_constraints_and_sixty_five_rows_are_refused():
    p = cr.make_problem(cr.case("e1_k8_d3_n20_p1"))
    D = _Device(p)
    extra = api.DeviceGP(p.gps[0][1].hyper, p.gps[0][1].X, p.gps[0][1].y, p.gps[0][1].noise)
    with pytest.raises(api.BoundsException) as e:
        api.ei_constrained_ensemble(D.obj, D.cons + [[extra]], D.tau + [0.0], p.points, p.best)
    assert (e.value.value, e.value.min, e.value.max) == (9.0, 0.0, 8.0)
    # a constraint handle equal to an objective handle, or listed twice
    with pytest.raises(api.InvalidValueException) as e:
        api.ei_constrained_ensemble(D.obj, [D.obj], [0.0], p.points, p.best)
    assert "listed twice" in str(e.value)
    with pytest.raises(api.InvalidValueException):
        api.ei_constrained_ensemble(D.obj, [D.cons[0], D.cons[0]], [0.0, 0.0], p.points, p.best)
    gd = (6, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    starts = np.random.default_rng(5).uniform(0.05, 0.95, size=(6, 3))
    bounds = [[0, 1]] * 3
    got = api.ei_constrained_suggest(D.obj, D.cons[:1], D.tau[:1], gd, bounds, p.best, starts, 64, gradient_ascent=False,
                                     points_being_sampled=p.pending[:1])
    assert got["points"].shape == (64, 3) and np.all(got["found"]) and np.all(np.isfinite(got["values"])) and np.all(got["values"] >= 0)
    with pytest.raises(api.BoundsException) as e:
        api.ei_constrained_suggest(D.obj, D.cons[:1], D.tau[:1], gd, bounds, p.best, starts, 65, gradient_ascent=False,
                                   points_being_sampled=p.pending[:1])
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 1.0, 64.0)
    extra.close()
    D.close()


def test_a_pending_point_listed_twice_in_a_noise_free_constraint_gp_is_singular():
    """tests/test_gpu_ei1.py's construction with the noise-free GP as the constraint GP of the second member: flat index 1 (1 + 1) + 1"""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    obj = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [1e-5])]
    con = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]
    bests = [float(y.min())] * 2
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.ei_constrained_ensemble(obj, [con], [0.0], starts, bests, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (3, 3) and "pending point 3" in str(e.value)
            with pytest.raises(api.SingularMatrixException) as e:
                api.ei_constrained_multistart(obj, [con], [0.0], gd, [[0, 1], [0, 1]], bests, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (3, 3)
    ok = api.ei_constrained_ensemble(obj, [con], [0.0], starts, bests, want_grad=False, points_being_sampled=pending[:3])
    assert np.all(np.isfinite(ok))  # (the handles still answer)
    for g in obj + con:
        g.close()


# ---- 8. the wrapper, on Branin with a disc constraint and 8 points ----
def test_the_wrapper_and_the_optimisation_run_end_to_end_on_branin_in_a_disc():
    import wrappers_mirror as cw
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(8, dim))
    a, b = 15.0 * X[:, 0] - 5.0, 15.0 * X[:, 1]
    y = (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0
    ys = (y - y.mean()) / y.std()
    cs = 4.0 * (np.sum((X - 0.5) ** 2, axis=1) - 0.4 ** 2)  # feasible inside the disc of radius 0.4 about the centre
    hypers = np.array([[1.0, 0.3, 0.3], [1.4, 0.25, 0.4], [0.8, 0.45, 0.3]])
    chypers = np.array([[1.0, 0.5, 0.5], [1.3, 0.6, 0.45], [0.8, 0.45, 0.6]])
    models, cmodels = [], []
    for vals, hyp, out in ((ys, hypers, models), (cs, chypers, cmodels)):
        hd = cw.HistoricalData(dim=dim, num_derivatives=0)
        hd.append_sample_points([cw.SamplePoint(X[i], [vals[i]], noise) for i in range(X.shape[0])])
        out.extend(cw.GaussianProcessMCMC(hyp, np.full((num_mcmc, 1), noise), hd, []).member_models())
    thresholds = [0.0]
    incumbent = eic.best_feasible_value(ys, cs, thresholds)
    assert math.isfinite(incumbent) and incumbent > ys.min() - 1e-12
    cei = eic.ConstrainedExpectedImprovementMCMC(models, [cmodels], thresholds)
    assert cei.problem_size == dim and cei.num_constraints == 1 and np.array_equal(cei.best_so_far, np.full(num_mcmc, incumbent))
    members, cmembers = eic._device_members(models), eic._device_members(cmodels)
    cand = rng.uniform(size=(7, dim))
    want_v, want_g = api.ei_constrained_ensemble(members, [cmembers], thresholds, cand, cei.best_so_far)
    assert np.array_equal(cei.evaluate_at_point_list(cand), want_v)
    cei.set_current_point(cand[3])
    assert cei.compute_objective_function() == want_v[3] and np.array_equal(cei.compute_grad_objective_function(), want_g[3:4])
    gd = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    bounds = [[0.0, 1.0]] * dim
    points, values, found = eic.multistart_constrained_expected_improvement_optimization(models, [cmodels], thresholds, bounds, gd,
                                                                                         num_multistarts=16, num_to_sample=3, seed=31)
    assert points.shape == (3, dim) and values.shape == (3,) and np.all(found)
    assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values)) and values[0] > 0.0
    starts = api.latin_hypercube(31, bounds, 16)
    first = api.ei_constrained_multistart(members, [cmembers], thresholds, gd, bounds, cei.best_so_far, starts)
    assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
    # the returned point's ensemble probability of feasibility under the restatement
    # (the wrapper's GPs are Matern-5/2 whatever the Python covariance class is called, as the reference's are)
    gps = [[cr.GP(kr.MATERN, hypers[e], X, ys.reshape(-1, 1), [noise], ()), cr.GP(kr.MATERN, chypers[e], X, cs.reshape(-1, 1), [noise], ())]
           for e in range(num_mcmc)]
    ref = [cr.Member(row, thresholds, incumbent, np.zeros((0, dim)), LD) for row in gps]
    res = cr.evaluate(ref, points[0])
    pof = float(sum(row[1] for row in res.factors) / num_mcmc)
    dev_pof = float(cei.probability_of_feasibility(points[:1])[0])
    print("Branin in a disc, 8 points, 3 members: a batch of 3 at %s, values %s; probability of feasibility of the first %.4f "
          "(device %.4f), its value %.6g against the restatement's %.6g" % (
              np.round(points, 3).tolist(), [float(v) for v in values], pof, dev_pof, values[0], float(res.value)))
    assert pof >= 0.5 and abs(dev_pof - pof) <= 1e-10 and abs(values[0] - float(res.value)) <= 1e-10 * res.scale
