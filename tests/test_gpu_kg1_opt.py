"""The ensemble forms of the discretised one-point knowledge gradient on the device (csrc/kg1_opt.hip: moe_kg_discrete_mcmc,
moe_kg_discrete_mcmc_multistart) on the cases of tests/kg1_opt_cases.py, whose inputs tests/test_kg1_opt_reference.py qualifies on
the CPU.  Shapes: d in {2, 3, 4} with one to four members, and d = 17 with a fidelity coordinate and d = 32 (padded dimensions 24
and 32) with two and three members.

The yardsticks: api.kg_discrete_mcmc (the host loop over the members, one moe_gp_kg_discrete call each) for the evaluator, bit for
bit; tests/ms_restatement.py's optimiser with its evaluations made by api.kg_discrete_mcmc and its updates in numpy for the
optimiser, bit for bit, path row by path row; the long-double restatement of tests/kg1_reference.py for the value at every kept end
point, within 1e-10 of the mean of the members' scales (every member's value is held to 1e-10 of its own scale by
tests/test_gpu_kg1.py, and the ensemble value is their mean).

Figures of the first run on an MI355X are recorded in DESIGN.md section 5.14."""
import ctypes as C

import numpy as np
import pytest

import kg1_opt_cases as kc
import kg1_reference as kr
import ms_restatement as ms
from cornell_moe_amd import _lib, api, knowledge_gradient_discrete

pytestmark = pytest.mark.gpu


def _gps(p):
    c = p.case
    return [api.DeviceGP(p.hyper[e], p.X[e], p.y[e], p.noise[e], cov_type=c.cov[e]) for e in range(len(c.n))]


def _close(gps):
    for g in gps:
        g.close()


def _stats():
    out = (C.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return [int(v) for v in out]


class _Launches(object):
    """ensemble-wide launches switched on or off for a block, the environment's setting restored afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib.load().moe_set_ensemble_launches(1 if self.on else 0)

    def __exit__(self, *exc):
        _lib.load().moe_set_ensemble_launches(-1)
        return False


# ---- 1. the evaluator ----
def _evaluator_inputs(kind):
    """(gps, sets, bests, points, nf, merges)"""
    if kind == "straddle":  # more candidates than one pass takes, as tests/test_gpu_kg1.py builds it: 4095 lines -> passes of 1024
        rng = np.random.default_rng(77)
        n, d, A, C_ = 12, 2, 4095, 1030
        per_pass = _lib.load().moe_kg1_pass_size(n, A)
        assert per_pass == 1024 and per_pass < C_ < 2 * per_pass
        X, y = rng.uniform(0, 1, size=(n, d)), rng.normal(size=(n, 1))
        hyper = np.array([1.3, 0.45, 0.45])
        gps = [api.DeviceGP(hyper * f, X, y, [1e-2 * f]) for f in (1.0, 1.3)]
        sets = [rng.uniform(0, 1, size=(A, d)) for _ in gps]
        return gps, sets, [float(y.min()), float(y.min()) + 0.1], rng.uniform(0, 1, size=(C_, d)), 0, True
    case = kc.CASES[0] if kind == "equal" else kc.CASES[1]
    p = kc.make_problem(case)
    assert (len(set(case.A)) == 1) == (kind == "equal") and len(set(case.n)) == 1
    return _gps(p), p.discrete, p.best, p.starts, case.nf, kind == "equal"


@pytest.mark.parametrize("kind", ["equal", "unequal", "straddle"])
def test_the_one_call_evaluator_is_the_host_loop_bit_for_bit(kind):
    gps, sets, bests, pts, nf, merges = _evaluator_inputs(kind)
    want_kg, want_grad = api.kg_discrete_mcmc(gps, sets, pts, bests, num_fidelity=nf)
    for on in (True, False):
        with _Launches(on):
            before = _stats()
            kg, grad = api.kg_discrete_ensemble(gps, sets, pts, bests, num_fidelity=nf)
            value_only = api.kg_discrete_ensemble(gps, sets, pts, bests, num_fidelity=nf, want_grad=False)
            after = _stats()
        assert kg.shape == want_kg.shape and grad.shape == want_grad.shape and np.all(np.isfinite(kg))
        bad = np.flatnonzero((kg != want_kg) | np.any(grad != want_grad, axis=1))
        assert bad.size == 0, (kind, on, int(bad[0]), kg[bad[0]], want_kg[bad[0]])
        assert np.array_equal(value_only, want_kg)
        grew = [a - b for a, b in zip(after, before)]
        print("%s, ensemble launches %s: merged calls +%d, fallbacks +%d, launches %d instead of %d" % ((kind, on) + tuple(grew)))
        if not on:
            assert grew == [0, 0, 0, 0]
        elif merges:
            assert grew[0] >= 1 and grew[1] == 0 and 0 < grew[2] < grew[3]
    _close(gps)


# ---- 2. the optimiser against the host-driven loop ----
def _host_loop(gps, p):
    """ms_restatement's optimiser, evaluations by api.kg_discrete_mcmc on the device, updates in numpy; returns a dict shaped like
    api.kg_discrete_multistart's, path included (a start that is not running repeats its point)"""
    case = p.case
    nf, d, T, R = case.nf, case.d, case.steps, case.restarts

    def value_fn(x):
        return api.kg_discrete_mcmc(gps, p.discrete, np.asarray(x).reshape(-1, d), p.best, num_fidelity=nf, want_grad=False)

    seen = {}      # global step -> (the starts that took it, their points before it)
    state = {"round": -1, "pending": None}

    def grad_fn(x):
        state["pending"] = np.array(x, copy=True).reshape(-1, d)
        return api.kg_discrete_mcmc(gps, p.discrete, state["pending"], p.best, num_fidelity=nf)[1].reshape(np.shape(x))

    def on_step(i, idx):
        if i == 0:
            state["round"] += 1
        seen[state["round"] * T + i] = (np.array(idx), state["pending"])

    vals = np.asarray(value_fn(p.starts))
    order = ms.top_k_order(vals)
    K = len(order)
    ends = ms.gradient_ascent(grad_fn, p.gd, p.bounds, p.starts[order], on_step=on_step)
    end_vals = np.asarray(value_fn(ends))
    point, value, found = p.starts[order[0]].copy(), -np.inf, False
    for s in range(K):
        if end_vals[s] > value:
            point, value, found = ends[s].copy(), float(end_vals[s]), True
    # the path: between two steps a start takes, and after its last one, its point stays where that step left it
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
        if not took:
            assert np.array_equal(ends[k], p.starts[order[k]])
    return {"point": point, "value": value, "found": found, "start_values": vals, "kept_index": order, "end_points": ends,
            "end_values": end_vals, "steps_taken": steps, "path": path}


_WANT = {}


def _expected(case):
    """the host-driven loop of a case, once per process (its GPs are closed again)"""
    if case.name not in _WANT:
        p = kc.make_problem(case)
        gps = _gps(p)
        _WANT[case.name] = (p, _host_loop(gps, p))
        _close(gps)
    return _WANT[case.name]


def _assert_same_run(case, got, want):
    assert np.array_equal(got["start_values"], want["start_values"])
    assert np.array_equal(got["kept_index"], want["kept_index"])
    diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
    if diff.size:
        k, row = int(diff[np.argmin(diff[:, 1])][0]), int(diff[:, 1].min())
        raise AssertionError("%s: the paths part at start %d (kept index %d), step %d: device %r, host loop %r" % (
            case.name, k, int(want["kept_index"][k]), row - 1, got["path"][k, row], want["path"][k, row]))
    assert np.array_equal(got["steps_taken"], want["steps_taken"])
    assert np.array_equal(got["end_points"], want["end_points"]) and np.array_equal(got["end_points"], got["path"][:, -1])
    assert np.array_equal(got["end_values"], want["end_values"])
    assert np.array_equal(got["point"], want["point"]) and got["value"] == want["value"] and got["found"] == want["found"]


@pytest.mark.parametrize("case", kc.CASES, ids=lambda c: c.name)
def test_the_optimiser_is_the_host_driven_loop_bit_for_bit(case):
    p, want = _expected(case)
    gps = _gps(p)
    for on in (True, False):
        with _Launches(on):
            got = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf, want_path=True)
        _assert_same_run(case, got, want)
    print("%s: %d kept starts, steps taken %s, value %.12g" % (case.name, len(want["kept_index"]), list(want["steps_taken"]),
                                                               want["value"]))
    assert want["found"]
    _close(gps)


# ---- 3. the value at every kept end point against long double ----
@pytest.mark.parametrize("case", kc.CASES, ids=lambda c: c.name)
def test_end_values_against_the_long_double_restatement(case):
    p, want = _expected(case)
    sets = kc.discrete_sets(p, kr.LD)
    worst, margin = 0.0, np.inf
    for k in range(len(want["kept_index"])):  # every kept end point: tests/test_kg1_opt_reference.py holds their margins
        value, res = kc.ensemble_value(sets, p, want["end_points"][k], kr.LD)
        scale = float(np.mean([r.scale for r in res]))
        margin = min(margin, min(min(r.margins) for r in res))
        worst = max(worst, abs(want["end_values"][k] - float(value)) / scale)
    print("%s: ensemble value at the kept end points vs long double %.3g of the members' mean scale (bound 1e-10); smallest margin "
          "%.3g" % (case.name, worst, margin))
    assert worst <= 1e-10


# ---- 4. one member is the single-GP path ----
def test_one_member_is_the_single_gp_path():
    case = [c for c in kc.CASES if len(c.n) == 1][0]
    p = kc.make_problem(case)
    dev = api.DeviceGP(p.hyper[0], p.X[0], p.y[0], p.noise[0], cov_type=case.cov[0])
    kgd = knowledge_gradient_discrete.DiscreteKnowledgeGradient(dev, p.discrete[0], best_so_far=p.best[0])
    vals = kgd.evaluate_at_point_list(p.starts)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: kgd.evaluate_at_point_list(x, want_grad=True)[1].reshape(np.shape(x)), p.gd, p.bounds,
                              p.starts[order])
    end_vals = kgd.evaluate_at_point_list(ends)
    got = api.kg_discrete_multistart(dev, p.gd, p.bounds, p.discrete, p.best, p.starts)  # (one DeviceGP counts as a list of one)
    assert np.array_equal(got["start_values"], vals) and np.array_equal(got["kept_index"], order)
    assert np.array_equal(got["end_points"], ends) and np.array_equal(got["end_values"], end_vals)
    best = int(np.argmax(end_vals))  # (the first of the largest)
    assert np.array_equal(got["point"], ends[best]) and got["value"] == end_vals[best] and got["found"]
    kg1, g1 = api.kg_discrete_ensemble([dev], p.discrete, p.starts, p.best)
    kg0, g0 = dev.kg_discrete(p.discrete[0], p.starts, p.best[0])
    assert np.array_equal(kg1, kg0) and np.array_equal(g1, g0)
    dev.close()


# ---- 5. no ascent ----
def test_without_an_ascent_the_best_start_and_without_a_round_the_kept_starts():
    case = kc.CASES[1]
    p, want = _expected(case)
    gps = _gps(p)
    got = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf, gradient_ascent=False)
    vals = want["start_values"]
    assert np.array_equal(got["start_values"], vals) and got["kept_index"] is None
    first_best = int(np.argmax(vals))
    assert np.array_equal(got["point"], p.starts[first_best]) and got["value"] == vals[first_best] and got["found"]
    tied = np.vstack([p.starts[3:4], p.starts[:6], p.starts[3:4]])  # equal values: the strict compare keeps the first
    got = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, tied, num_fidelity=case.nf, gradient_ascent=False)
    assert got["start_values"][0] == got["start_values"][4] == got["start_values"][7]
    w = int(np.argmax(got["start_values"]))
    assert np.array_equal(got["point"], tied[w]) and got["value"] == got["start_values"][w]
    gd0 = p.gd[:2] + (0,) + p.gd[3:]  # max_num_restarts = 0: nothing moves
    got = api.kg_discrete_multistart(gps, gd0, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf, want_path=True)
    order = want["kept_index"]
    assert np.array_equal(got["kept_index"], order) and np.array_equal(got["end_points"], p.starts[order])
    assert got["path"].shape == (len(order), 1, case.d) and np.array_equal(got["path"][:, 0], p.starts[order])
    assert np.array_equal(got["end_values"], vals[order]) and np.all(got["steps_taken"] == 0)
    w = int(np.argmax(vals[order]))
    assert np.array_equal(got["point"], p.starts[order[w]]) and got["value"] == vals[order[w]] and got["found"]
    _close(gps)


# ---- 6. error returns ----
def test_a_start_on_a_noiseless_sampled_point_is_singular():
    """as tests/test_gpu_kg1.py: alpha = 1 and the FIRST sampled point, in the SECOND member only -- payload (member, index)"""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), rng.normal(size=(6, 1))
    gps = [api.DeviceGP([1.0, 0.5, 0.5], X, y, [1e-2]), api.DeviceGP([1.0, 0.5, 0.5], X, y, [0.0])]
    sets = [rng.uniform(0, 1, size=(10, 2)), rng.uniform(0, 1, size=(7, 2))]
    bests = [float(y.min())] * 2
    starts = np.vstack([rng.uniform(0.1, 0.9, size=(2, 2)), X[:1], rng.uniform(0.1, 0.9, size=(1, 2))])
    gd = (4, 3, 1, 0, kc.GAMMA, kc.PRE_MULT, kc.MAX_REL, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.kg_discrete_multistart(gps, gd, [[0, 1], [0, 1]], sets, bests, starts)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 2)
            with pytest.raises(api.SingularMatrixException) as e:
                api.kg_discrete_ensemble(gps, sets, starts, bests)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 2)
    ok = api.kg_discrete_ensemble(gps, sets, starts[:2], bests, want_grad=False)  # (the handles still answer)
    assert np.all(np.isfinite(ok))
    _close(gps)


def test_mismatched_members_and_the_simplex_are_refused():
    rng = np.random.default_rng(4)
    X2, X3, y = rng.uniform(0, 1, size=(6, 2)), rng.uniform(0, 1, size=(6, 3)), rng.normal(size=(6, 1))
    g2 = api.DeviceGP([1.0, 0.5, 0.5], X2, y, [1e-2])
    g3 = api.DeviceGP([1.0, 0.5, 0.5, 0.5], X3, y, [1e-2])
    gd_obs = api.DeviceGP([1.0, 0.5, 0.5], X2, np.hstack([y, np.zeros((6, 1))]), [1e-2, 1e-2], [0])
    lib, dp, ip = _lib.load(), _lib.dp, _lib.ip
    err = _lib.MoeError()
    buf = np.full(64, 0.5)
    p = buf.ctypes.data_as(dp)
    cnt = np.ascontiguousarray([4, 4], dtype=np.int32)

    def evaluate(a, b):
        arr = (C.c_void_p * 2)(a._h.value, b._h.value)
        return lib.moe_kg_discrete_mcmc(arr, 2, 0, p, cnt.ctypes.data_as(ip), p, p, 2, 1, p, p, C.byref(err))

    assert evaluate(g2, g3) == _lib.MOE_ERR_INVALID_VALUE and tuple(err.payload) == (3.0, 2.0, 1.0) and b"share dim" in err.message
    assert evaluate(g2, gd_obs) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (1.0, 0.0, 0.0)
    assert b"not a minimum of lines" in err.message
    assert evaluate(g2, g2) == _lib.MOE_ERR_INVALID_VALUE and b"listed twice" in err.message
    sets, bests, starts = [buf[:8].reshape(4, 2)] * 2, [0.0, 0.0], rng.uniform(0.1, 0.9, size=(3, 2))
    with pytest.raises(api.BoundsException) as e:
        api.kg_discrete_ensemble([g2, g2], sets, starts, bests, num_fidelity=2)
    assert "num_fidelity" in str(e.value) and (e.value.value, e.value.max) == (2.0, 1.0)
    simplex = (4, 3, 1, 0, kc.GAMMA, kc.PRE_MULT, kc.MAX_REL, 1e-10, 1)
    with pytest.raises(api.InvalidValueException) as e:
        api.kg_discrete_multistart([g2], simplex, [[0, 1], [0, 1]], sets[:1], bests[:1], starts)
    assert "tensor-product" in str(e.value)
    with pytest.raises(api.InvalidValueException):
        api.kg_discrete_multistart([g2, g3], simplex[:8], [[0, 1], [0, 1]], sets, bests, starts)
    with pytest.raises(api.BoundsException):
        api.kg_discrete_multistart([g2, gd_obs], simplex[:8], [[0, 1], [0, 1]], sets, bests, starts)
    kg = api.kg_discrete_ensemble([g2], sets[:1], starts, bests[:1], want_grad=False)  # (the handle still answers)
    assert np.all(np.isfinite(kg))
    for g in (g2, g3, gd_obs):
        g.close()


# ---- 7. the wrapper ----
def test_the_wrapper_runs_the_optimiser_from_latin_hypercube_starts():
    """The suggestion is the best END point, as multistart() returns it: an ascent without a line search may end below the value it
    started from, so "at least every start's value" is a property of the input, not of the optimiser.  On this input the float64
    restatement on the CPU (kg1_opt_cases.float64_run from the same 24 starts) ends 4.1e-4 above the best start; three of the six
    cases would end below theirs by 3.5e-4 to 1.2e-2."""
    case = kc.CASES[1]
    p = kc.make_problem(case)
    gps = _gps(p)
    point, value, found = knowledge_gradient_discrete.multistart_discrete_knowledge_gradient_optimization(
        gps, p.discrete, p.best, p.bounds, p.gd, 24, 31, num_fidelity=case.nf)
    starts = api.latin_hypercube(31, p.bounds, 24)
    res = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, starts, num_fidelity=case.nf)
    assert np.array_equal(point, res["point"]) and value == res["value"] and found and res["found"]
    print("the wrapper's value %.9g, the best start's %.9g" % (value, res["start_values"].max()))
    assert len(res["kept_index"]) == 20 and np.all(value >= res["start_values"])
    assert np.all(point >= 0.0) and np.all(point <= 1.0)
    _close(gps)
