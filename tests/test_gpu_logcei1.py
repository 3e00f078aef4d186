"""The log constrained expected improvement on the device (csrc/logcei1.hip: moe_log_ei_constrained_mcmc,
moe_log_ei_constrained_mcmc_multistart, moe_log_ei_constrained_mcmc_suggest) against the long-double restatement of
tests/logcei1_reference.py, on cei1_reference.CASES at the three shifts of logcei1_reference.SHIFTS and cei1_reference.WIDE_CASES
(unequal members at padded dimension 24) unshifted and at the deepest shift, whose inputs
tests/test_logcei1_reference.py qualifies on the CPU (float64 within 2.5e-11 of long double, the pending points moving a checked
value by at least 1e-5, the stall problems stalling the plain form in float64 and letting the log form climb).

Tolerances: tests/test_gpu_ei1.py's 1e-10, the chains being the same kernels over the same lengths, taken RELATIVE because a log
value is of order c^2 / 2 -- |value - want| <= 1e-10 max(1, |want|), |grad - want|_inf <= 1e-10 max(1, |want|_inf), every log
factor like the value.  Against the plain form the bound is the sum of the two forms' bounds.  Everything else is bit for bit:
value-only against value + gradient, a candidate alone against itself in a batch and across the pass boundary, ensemble-wide
launches on against off, one member without constraints against its own log factor, an empty pending list against none, the ascent
against a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch against calls of the ascent fed their
predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.22 records those of the first
run."""
import ctypes as C
import math

import numpy as np
import pytest

import cei1_reference as cr
import logcei1_reference as lr
import ms_restatement as ms
from cornell_moe_amd import _lib, api

pytestmark = pytest.mark.gpu

LD = lr.LD
dp, ip = _lib.dp, _lib.ip
BOUND = 1e-10

CASE_SHIFTS = [(c, s) for c in lr.CASES for s in lr.SHIFTS] + [(c, s) for c in lr.WIDE_CASES for s in lr.WIDE_SHIFTS]
ALL_CASES = lr.CASES + lr.WIDE_CASES
IDS = ["%s-b%g-t%g" % (c.name, s[0], s[1]) for c, s in CASE_SHIFTS]


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


def _eval(D, p, points, pending="problem", best=None, tau=None, **kw):
    pending = p.pending if isinstance(pending, str) else pending
    return api.log_ei_constrained_ensemble(D.obj, D.cons, p.thresholds[:len(D.cons)] if tau is None else tau, points,
                                           p.best if best is None else best, points_being_sampled=pending, **kw)


def _raw_eval(D, p, points, pending):
    """moe_log_ei_constrained_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array"""
    arr, E, d, keep, carr, K, tau, best = api._ei_constrained_members(D.obj, D.cons, p.thresholds[:len(D.cons)], p.best)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    value, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(_lib.load().moe_log_ei_constrained_mcmc(arr, E, carr, K, tau.ctypes.data_as(dp) if K else None, best.ctypes.data_as(dp),
                                                       pend.ctypes.data_as(dp), pend.shape[0] - 1, pts.ctypes.data_as(dp), len(pts), 1,
                                                       value.ctypes.data_as(dp), grad.ctypes.data_as(dp), None, C.byref(err)), err)
    return value, grad


def _errors(value, grad, logs, want):
    """the worst relative errors of candidates' values, gradients and log factors against Results"""
    e_v = max(abs(value[i] - float(w.value)) / max(1.0, abs(float(w.value))) for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(w.grad)))) for i, w in enumerate(want))
    e_f = max(abs(logs[e, r, i] - float(f)) / max(1.0, abs(float(f))) for i, w in enumerate(want) for e, row in enumerate(w.log_factors)
              for r, f in enumerate(row))
    return e_v, e_g, e_f


# ---- 1. value, gradient and log factors against long double; 4. the bits of one call ----
@pytest.mark.parametrize("case,shift", CASE_SHIFTS, ids=IDS)
def test_against_the_long_double_restatement(case, shift):
    p, want = lr.expected(case, shift, LD)
    D = _Device(p)
    C_, d = p.points.shape
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_log_factors=True))
    value, grad, logs = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and logs.shape == (case.E, 1 + case.K, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(logs))
    e_v, e_g, e_f = _errors(value, grad, logs, want)
    low = min(a for w in want for row in w.args for a in row)
    print("%s %s: value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds 1e-10); lowest c or z %.1f, lowest "
          "value %.1f, largest |grad| %.3g" % (case.name, shift, e_v, e_g, e_f, low, float(value.min()), float(np.max(np.abs(grad)))))
    assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND, (case.name, shift, e_v, e_g, e_f)
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, f1 = _eval(D, p, p.points[i:i + 1], want_log_factors=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(f1[:, :, 0], logs[:, :, i]), (case.name, i)
    # no pending point through the symbol's pending arguments against None
    raw = _raw_eval(D, p, p.points, p.pending[:0])
    none = _eval(D, p, p.points, pending=None)
    assert np.array_equal(raw[0], none[0]) and np.array_equal(raw[1], none[1])
    if case.p:
        assert not np.array_equal(none[0], value)
    D.close()


# ---- 2. against the plain form ----
@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_exp_of_the_value_is_the_constrained_expected_improvement(case):
    p, plain = cr.expected(case, LD)
    D = _Device(p)
    value = _eval(D, p, p.points, want_grad=False)
    A = api.ei_constrained_ensemble(D.obj, D.cons, D.tau, p.points, p.best, points_being_sampled=p.pending, want_grad=False)
    worst = 0.0
    for i in range(len(p.points)):
        bound = BOUND * plain[i].scale + BOUND * A[i] * max(1.0, abs(math.log(A[i])) if A[i] > 0 else 1.0)
        worst = max(worst, abs(math.exp(value[i]) - A[i]) / bound)
    print("%s: |exp(value) - plain value| at most %.3g of its bound" % (case.name, worst))
    assert worst <= 1.0
    D.close()


# ---- 3. the scalar regimes ----
def test_every_regime_of_the_scalars():
    p, limits, want = lr.regime_expected(LD)
    D = _Device(p)
    for i, (w, (best, tau)) in enumerate(zip(want, limits)):
        runs = []
        for on in (True, False):
            with _Launches(on):
                runs.append(_eval(D, p, p.points, pending=None, best=[best], tau=[tau], want_log_factors=True))
        value, grad, logs = runs[0]
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(np.isfinite(logs))
        e_v, e_g, e_f = _errors(value[i:i + 1], grad[i:i + 1], logs[:, :, i:i + 1], [w])
        print("candidate %d: c %.6g z %.6g value %.9g: value error %.3g, gradient error %.3g, log factor error %.3g (relative, bounds "
              "1e-10)" % (i, w.args[0][0], w.args[0][1], value[i], e_v, e_g, e_f))
        assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND, (i, e_v, e_g, e_f)
        assert np.array_equal(_eval(D, p, p.points, pending=None, best=[best], tau=[tau], want_grad=False), value)
    D.close()


# ---- 4. bit for bit: across the pass boundary; one member without constraints ----
_N8 = cr.Case("e1_k1_d2_n8_p2_two_passes", 44, 1, 1, 2, ((8, 8),), 2, (), "median", (0.0,), None, 4100, None)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    p0 = lr.make_problem(_N8)
    shift = lr.SHIFTS[1]
    p = p0._replace(best=[b - shift[0] for b in p0.best])
    checked = (0, per_pass - 1, per_pass, _N8.C - 1)
    members = lr.relimited(lr.ensemble(p0, LD), p.best, p.thresholds)
    D = _Device(p)
    for pending in (p.pending, None):
        value, grad, logs = _eval(D, p, p.points, pending=pending, want_log_factors=True)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
        assert np.array_equal(_eval(D, p, p.points, pending=pending, want_grad=False), value)
        assert np.array_equal(value, logs[0, 0] + logs[0, 1])
        for i in checked:
            v1, g1 = _eval(D, p, p.points[i:i + 1], pending=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            want = [lr.evaluate(members, p.points[i]) for i in checked]
            idx = list(checked)
            e_v, e_g, e_f = _errors(value[idx], grad[idx], logs[:, :, idx], want)
            print("%s: value error %.3g, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
    D.close()


def test_one_member_without_constraints_is_its_own_log_factor_bit_for_bit():
    case = cr.case("e1_k1_d3_n20_p3")
    for shift in lr.SHIFTS:
        p, _ = lr.shifted(case, shift, np.float64, constraints=False)
        D = _Device(p, K=0)
        value, grad, logs = api.log_ei_constrained_ensemble(D.obj, None, None, p.points, p.best, points_being_sampled=p.pending,
                                                            want_log_factors=True)
        assert logs.shape == (1, 1, len(p.points)) and np.array_equal(value, logs[0, 0])
        _, members = lr.shifted(case, shift, LD, constraints=False)
        want = [lr.evaluate(members, x) for x in p.points]
        e_v, e_g, _ = _errors(value, grad, logs, want)
        print("%s without its constraint, %s: value error %.3g, gradient error %.3g" % (case.name, shift, e_v, e_g))
        assert e_v <= BOUND and e_g <= BOUND
        D.close()


# ---- 5. incumbents ----
def test_infinite_and_believed_feasible_incumbents():
    shift = lr.SHIFTS[0]
    seen_inf = seen_join = 0
    for name in (cr.MIXED, cr.INF, cr.INF_FEASIBLE):
        case = cr.case(name)
        p, want = lr.expected(case, shift, LD)
        _, members = lr.shifted(case, shift, LD)
        D = _Device(p)
        value, grad, logs = _eval(D, p, p.points, want_log_factors=True)
        e_v, e_g, e_f = _errors(value, grad, logs, want)
        for e, m in enumerate(members):
            if np.isinf(m.bprime):  # no feasible incumbent, before or after the pending points: log 1, exactly
                assert np.all(logs[e, 0] == 0.0) and not np.any(np.signbit(logs[e, 0]))
                seen_inf += 1
            elif float(m.bprime) != p.best[e]:  # a believed-feasible pending point has joined: b alone would be far off
                alone = lr.relimited([m], [p.best[e]], p.thresholds)[0]
                alone.mask[:] = False
                alone.bprime = LD(p.best[e])
                if np.isfinite(p.best[e]):
                    off = max(abs(float(lr.member_logs(alone, x)[0][0] - w.log_factors[e][0])) for x, w in zip(p.points, want))
                    assert off >= 1e-3
                seen_join += 1
        print("%s: value error %.3g, gradient error %.3g, log factor error %.3g; b' %s against b %s" % (
            name, e_v, e_g, e_f, [float(m.bprime) for m in members], p.best))
        assert e_v <= BOUND and e_g <= BOUND and e_f <= BOUND
        D.close()
    assert seen_inf >= 1 and seen_join >= 2


# ---- 6. the ascent against the host-driven loop ----
MS = dict(starts=12, steps=6, restarts=2, gamma=0.7, pre_mult=1.0, max_rel=0.5)


def _ascent_inputs(d, tolerance):
    starts = lr.stall_starts(d)
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    return starts, gd, np.array([[0.0, 1.0]] * d)


def _same_run(got, want):
    for key in ("start_values", "kept_index", "path", "steps_taken", "end_points", "end_values", "point"):
        assert np.array_equal(got[key], want[key]), key
    assert got["value"] == want["value"] and got["found"] == want["found"]


def _host_loop(evaluate, starts, gd, bounds):
    """ms_restatement's optimiser, evaluations by `evaluate(points, want_grad)` on the device, updates in numpy; a dict shaped like
    api.log_ei_constrained_multistart's, path included (a start that is not running repeats its point)"""
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


# (1e-10 and 6e-2 are tests/test_gpu_ei1.py's; at both every start of this objective runs all 12 steps, so 6e-2 masks no update.
#  0.6 was chosen on the CPU with the float64 restatement: at K = 2 the starts take 8, 3, 6, 12, 9, 3, 6, ... steps and at K = 0
#  12, 6, 6, 6, 5, 6, 3, ...: some stop inside a round, some after one round of 6, so the step kernel's masked update runs under the
#  combined gradient.  At 0.3 two starts stop early at K = 2 and one at K = 0; at 1.0 none reaches the second round.)
@pytest.mark.parametrize("constraints", [True, False], ids=["k2", "k0"])
@pytest.mark.parametrize("tolerance", [1e-10, 6e-2, 0.6], ids=["tight", "loose", "masked"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(tolerance, constraints):
    p = lr.make_problem(cr.case(cr.ENSEMBLE))  # E = 3, K = 2
    D = _Device(p, K=None if constraints else 0)
    cons, tau = (D.cons, D.tau) if constraints else (None, None)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], tolerance)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    plain = api.log_ei_constrained_multistart(D.obj, cons, tau, gd, bounds, p.best, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.log_ei_constrained_multistart(D.obj, cons, tau, gd, bounds, p.best, starts, want_path=True,
                                                    points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("tolerance %g, K = %d: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(D.cons), len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"] and int(want["steps_taken"].max()) > 0
    if tolerance < 1e-3:
        assert want["value"] >= want["start_values"].max()
    if tolerance > 0.1:
        assert int(want["steps_taken"].min()) < MS["steps"] * MS["restarts"]  # (masked steps occurred)
    none = api.log_ei_constrained_multistart(D.obj, cons, tau, gd, bounds, p.best, starts, gradient_ascent=False,
                                             points_being_sampled=pending)
    best = int(np.argmax(want["start_values"]))
    assert np.array_equal(none["point"], starts[best]) and none["value"] == want["start_values"][best] and none["found"]
    D.close()


# ---- 7. greedy batches ----
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    p = lr.make_problem(cr.case(cr.ENSEMBLE))
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.log_ei_constrained_multistart(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.log_ei_constrained_suggest(D.obj, D.cons, D.tau, gd, bounds, p.best, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) >= 1e-3
    D.close()


# ---- 8. the stall ----
@pytest.mark.parametrize("name", lr.STALL_CASES)
def test_the_plain_form_stalls_and_the_log_form_climbs(name):
    p, _ = lr.stall(name, np.float64)
    D = _Device(p)
    d = p.points.shape[1]
    starts, bounds = lr.stall_starts(d), np.array([[0.0, 1.0]] * d)
    plain = api.ei_constrained_multistart(D.obj, D.cons, D.tau, lr.STALL_GD, bounds, p.best, starts, points_being_sampled=p.pending)
    assert np.all(plain["start_values"] == 0.0) and np.array_equal(plain["end_points"], starts[plain["kept_index"]])
    got = api.log_ei_constrained_multistart(D.obj, D.cons, D.tau, lr.STALL_GD, bounds, p.best, starts, points_being_sampled=p.pending)
    print("%s: the plain form's start values are all 0 and no start moves; the log form's best start value %.9g, after the ascent "
          "%.9g (gain %.3g)" % (name, got["start_values"].max(), got["value"], got["value"] - got["start_values"].max()))
    assert np.all(np.isfinite(got["start_values"])) and got["found"]
    assert got["value"] >= got["start_values"].max() + lr.STALL_GAIN
    D.close()


# ---- the wrapper ----
def test_the_wrapper_and_the_optimisation_run_end_to_end():
    import wrappers_mirror as cw
    from cornell_moe_amd import expected_improvement_constrained as eic, log_expected_improvement as lei
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(8, dim))
    ys = np.sin(5.0 * X[:, 0]) + X[:, 1] ** 2
    cs = 4.0 * (np.sum((X - 0.5) ** 2, axis=1) - 0.4 ** 2)
    hypers = np.array([[1.0, 0.3, 0.3], [1.4, 0.25, 0.4], [0.8, 0.45, 0.3]])
    models, cmodels = [], []
    for vals, out in ((ys, models), (cs, cmodels)):
        hd = cw.HistoricalData(dim=dim, num_derivatives=0)
        hd.append_sample_points([cw.SamplePoint(X[i], [vals[i]], noise) for i in range(X.shape[0])])
        out.extend(cw.GaussianProcessMCMC(hypers, np.full((num_mcmc, 1), noise), hd, []).member_models())
    thresholds = [0.0]
    incumbent = eic.best_feasible_value(ys, cs, thresholds)
    members, cmembers = eic._device_members(models), eic._device_members(cmodels)
    cand = rng.uniform(size=(7, dim))
    bounds, gd = [[0.0, 1.0]] * dim, (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    starts = api.latin_hypercube(31, bounds, 16)
    for cm, cmem, tau in (([cmodels], [cmembers], thresholds), (None, None, None)):
        obj = lei.LogExpectedImprovementMCMC(models, constraint_models=cm, thresholds=tau)
        want_best = incumbent if cm else float(ys.min())
        assert obj.problem_size == dim and obj.num_constraints == (1 if cm else 0)
        assert np.array_equal(obj.best_so_far, np.full(num_mcmc, want_best))
        want_v, want_g = api.log_ei_constrained_ensemble(members, cmem, tau, cand, obj.best_so_far)
        assert np.array_equal(obj.evaluate_at_point_list(cand), want_v)
        obj.set_current_point(cand[3])
        assert obj.compute_objective_function() == want_v[3] and np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
        points, values, found = lei.multistart_log_expected_improvement_optimization(
            models, bounds, gd, num_multistarts=16, num_to_sample=2, constraint_models=cm, thresholds=tau, seed=31)
        assert points.shape == (2, dim) and np.all(found) and np.all(np.isfinite(values))
        first = api.log_ei_constrained_multistart(members, cmem, tau, gd, bounds, obj.best_so_far, starts)
        assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
        if cm:
            plain = eic.ConstrainedExpectedImprovementMCMC(models, cm, tau)
            assert np.max(np.abs(obj.probability_of_feasibility(cand) - plain.probability_of_feasibility(cand))) <= 1e-10
