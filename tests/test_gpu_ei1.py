"""The ensemble analytic expected improvement on the device (csrc/ei1.hip: moe_ei_analytic_mcmc, moe_ei_analytic_mcmc_multistart,
moe_ei_analytic_mcmc_suggest) against the long-double restatement of tests/ei1_reference.py, on the cases ei1_reference.PROBLEMS
and WIDE_PROBLEMS (padded dimensions 12 to 24, more than 256 rows, tri_cols' wider K slices), whose inputs tests/test_ei1_reference.py qualifies on the CPU (float64 within 2.5e-11 scale of long double, sigma >= 0.05
sqrt(alpha), P moves a checked candidate's value by >= 1e-5 scale: a device that ignored P fails here).

Tolerances: tests/test_gpu_kg1.py's for the same products and sums -- |EI - want| <= 1e-10 scale, |grad EI - want|_inf <= 1e-10
max(1, |want|_inf).  Everything else is bit for bit: value-only against value + gradient, a candidate alone against itself in a
batch and across the pass boundary, the ensemble against its members added on the host, ensemble-wide launches on against off, the
ascent against a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch against calls of the ascent fed
their predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.16 records those of the
first run."""
import ctypes as C

import numpy as np
import pytest

import ei1_reference as er
import kg1_pending_reference as kp
import kg1_reference as kr
import ms_restatement as ms
from cornell_moe_amd import _lib, api, expected_improvement_analytic as eia

pytestmark = pytest.mark.gpu

LD = kr.LD
dp, ip = _lib.dp, _lib.ip


def _gp(p):
    return api.DeviceGP(p.hyper, p.X, p.y, p.noise, cov_type=p.cov_type)


def _close(gps):
    for g in gps:
        g.close()


class _Launches(object):
    """ensemble-wide launches switched on or off for a block, the environment's setting restored afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib.load().moe_set_ensemble_launches(1 if self.on else 0)

    def __exit__(self, *exc):
        _lib.load().moe_set_ensemble_launches(-1)
        return False


def _raw_eval(gps, points, bests, pending, want_grad=True):
    """moe_ei_analytic_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array"""
    arr, E, d, keep, best = api._ei_analytic_members(gps, bests)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    num = pend.shape[0] - 1
    ei, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(_lib.load().moe_ei_analytic_mcmc(arr, E, best.ctypes.data_as(dp), pend.ctypes.data_as(dp), num, pts.ctypes.data_as(dp),
                                                len(pts), 1 if want_grad else 0, ei.ctypes.data_as(dp),
                                                grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
    return ei, grad


def _errors(ei, grad, want, checked):
    e_v = max(abs(ei[i] - float(want[i].value)) / want[i].scale for i in checked)
    e_g = max(float(np.max(np.abs(grad[i] - want[i].grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(want[i].grad))))
              for i in checked)
    return e_v, e_g


# ---- 1. value and gradient against long double ----
@pytest.mark.parametrize("p", er.PROBLEMS + er.WIDE_PROBLEMS, ids=lambda p: p.name)
def test_against_the_long_double_restatement(p):
    want, without = er.expected(p)
    G = _gp(p)
    C_, d = p.points.shape
    ei, grad = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending)
    assert ei.shape == (C_,) and grad.shape == (C_, d) and np.all(np.isfinite(ei)) and np.all(np.isfinite(grad))
    e_v, e_g = _errors(ei, grad, want, p.checked)
    moved = max(abs(ei[i] - float(without[i])) / want[i].scale for i in p.checked)
    print("%s: value error %.3g scale, gradient error %.3g (bounds 1e-10); P moved EI by up to %.3g scale" % (p.name, e_v, e_g, moved))
    assert e_v <= 1e-10 and e_g <= 1e-10, (p.name, e_v, e_g)
    # the symbol itself (an empty list reaches it as num_being_sampled = 0 beside a non-NULL array): the same bits
    ei2, grad2 = _raw_eval([G], p.points, [p.best], p.pending)
    assert np.array_equal(ei, ei2) and np.array_equal(grad, grad2)
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending, want_grad=False), ei)
    for i in (0, C_ - 1):
        e1, g1 = api.ei_analytic_ensemble(G, p.points[i:i + 1], [p.best], points_being_sampled=p.pending)
        assert e1[0] == ei[i] and np.array_equal(g1[0], grad[i]), (p.name, i)
    G.close()


def test_the_believed_best_binds():
    p = [q for q in er.PROBLEMS if q.name == er.BPRIME][0]
    want, _ = er.expected(p)
    G = _gp(p)
    ei = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending, want_grad=False)
    # with the caller's best value left as it is the expected improvement would be far larger
    base = er.base_model(p, LD)
    cond = kp.PendingModel(base, p.pending)
    wrong = []
    for i in p.checked:
        x = p.points[i].reshape(1, -1)
        k = cond.cov(cond.X, x)[:, 0]
        v = cond.fwd(k)
        mu, var = LD(base.mean) + k @ cond.kinvy, cond.cov(x, x)[0, 0] - v @ v
        t, s = LD(p.best) - mu, np.sqrt(var)
        wrong.append(float(t * er.normal_cdf(t / s, LD) + s * kr.normal_pdf(t / s, LD)))
    gap = min(abs(w - float(want[i].value)) for w, i in zip(wrong, p.checked))
    print("b' = %.4f against best = %.4f: EI with the caller's best differs by >= %.3g" % (want[0].bprime, p.best, gap))
    assert gap > 1e-3 and max(abs(ei[i] - float(want[i].value)) for i in p.checked) <= 1e-10 * want[0].scale
    G.close()


# ---- 2. the reference's recorded values on the committed fixtures, and the host-finished path ----
def test_the_fixtures_of_the_reference_and_the_host_finished_path(golden):
    cases, _ = golden
    seen, worst = 0, [0.0, 0.0, 0.0, 0.0]
    for c in cases:
        i = c.inp
        if len(i["derivs"]) or len(np.ravel(i["noise"])) != 1:
            continue
        seen += 1
        G = api.DeviceGP(np.concatenate([[float(i["alpha"])], i["lengths"]]), i["X"], i["y"], i["noise"], [], cov_type=int(i["cov_type"]))
        best = float(i["ei_best"])
        ei, grad = api.ei_analytic_ensemble(G, i["query"], [best])
        ref_ei, ref_grad = c.out["ei_analytic"], c.out["grad_ei_analytic"]
        old_ei, old_grad = G.ei_analytic_batch(i["query"], best)
        sv, sg = max(np.abs(ref_ei).max(), 1e-6), max(np.abs(ref_grad).max(), 1e-6)
        figs = [np.abs(ei - ref_ei).max() / sv, np.abs(grad - ref_grad).max() / sg, np.abs(ei - old_ei).max() / sv,
                np.abs(grad - old_grad).max() / sg]
        worst = [max(a, float(b)) for a, b in zip(worst, figs)]
        assert figs[0] <= 1e-11 and figs[1] <= 1e-9 and figs[2] <= 1e-11 and figs[3] <= 1e-9, figs
        G.close()
    print("%d fixture cases: against the reference %.3g / %.3g, against ei_analytic_batch %.3g / %.3g (bounds 1e-11 / 1e-9)" % (
        seen, worst[0], worst[1], worst[2], worst[3]))
    assert seen >= 4


# ---- 3. bit for bit ----
_N8 = kp.Case("n8_d2_p2_two_passes", 44, 8, 2, 1, 2, 0, kr.MATERN, 1e-3, 4100)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(_N8.n)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    q = kp.make_problem(_N8)
    p = er.Problem(_N8.name, _N8.cov_type, q.hyper, q.X, q.y, q.noise, q.points, q.pending, q.best, (0, per_pass - 1, per_pass, _N8.C - 1))
    want, _ = er.expected(p)
    G = _gp(p)
    for pending in (p.pending, None):
        ei, grad = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=pending)
        assert np.array_equal(api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=pending, want_grad=False), ei)
        for i in p.checked:
            e1, g1 = api.ei_analytic_ensemble(G, p.points[i:i + 1], [p.best], points_being_sampled=pending)
            assert e1[0] == ei[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            e_v, e_g = _errors(ei, grad, want, p.checked)
            print("%s: value error %.3g scale, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= 1e-10 and e_g <= 1e-10
    G.close()


# more than 4096 rows: the pass is no longer the 4096 cap but follows from N (2^24 doubles of V per pass), and a call of 4036
# candidates is one pass of 4032 and one of 4.  (Seed chosen on the CPU: EI >= 1e-2 scale at all four checked candidates, and b'
# binds; with most seeds mu(P) lies so far below the median that one or two of the four have an EI below 1e-4.)
_N4097 = kp.Case("n4097_d4_p2_short_pass", 48, 4097, 4, 1, 2, 0, kr.MATERN, 1e-2, 4036)


def short_pass_problem():
    per_pass = _lib.load().moe_ei1_pass_size(_N4097.n)
    assert per_pass == 4032 and _N4097.C == per_pass + 4
    q = kp.make_problem(_N4097)
    return er.Problem(_N4097.name, _N4097.cov_type, q.hyper, q.X, q.y, q.noise, q.points, q.pending, float(np.median(q.y)),
                      (0, per_pass - 1, per_pass, _N4097.C - 1))


def test_a_pass_shorter_than_4096_candidates_above_4096_rows():
    """value-only against value + gradient and a candidate alone against itself in the batch, bit for bit, on both sides of the
    boundary at 4032; those four candidates against tests/ei1_reference.py in FLOAT64 (a long-double factorisation of 4099 rows takes
    minutes): 1e-9 scale in value and 1e-9 max(1, |want|) in gradient.  At N = 4097 the float64 restatement lies 6.9e-13 / 4.8e-12
    from long double (one run in d = 2), so the bound is 200 times the reference's own error, and an offset or a width that is off
    by one column moves a value by 1e-3 or more."""
    p = short_pass_problem()
    base = er.base_model(p, np.float64)
    P = np.asarray(p.pending, dtype=np.float64)
    model = kp.PendingModel(base, P)
    y_max = float(np.max(np.abs(p.y)))
    want = {i: er.evaluate_model(model, base, P, p.points[i], p.best, y_max) for i in p.checked}
    big = [i for i in p.checked if float(want[i].value) >= 1e-3 * want[i].scale and float(np.max(np.abs(want[i].grad))) >= 1e-2]
    assert len(big) == 4 and p.best == float(np.median(p.y)) and want[0].bprime < p.best - 1e-2
    G = _gp(p)
    for pending in (p.pending, None):
        ei, grad = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=pending)
        assert np.all(np.isfinite(ei)) and np.all(np.isfinite(grad))
        assert np.array_equal(api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=pending, want_grad=False), ei)
        for i in p.checked:
            e1, g1 = api.ei_analytic_ensemble(G, p.points[i:i + 1], [p.best], points_being_sampled=pending)
            assert e1[0] == ei[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            e_v, e_g = _errors(ei, grad, want, p.checked)
            print("%s: value error %.3g scale, gradient error %.3g against the float64 restatement on both sides of the pass boundary "
                  "(bounds 1e-9); EI / scale of the four %s" % (p.name, e_v, e_g, [float(want[i].value) / want[i].scale for i in p.checked]))
            assert e_v <= 1e-9 and e_g <= 1e-9
    G.close()


def _ensemble_gps(ep):
    return [api.DeviceGP(ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], cov_type=ep.cov[k]) for k in range(len(ep.X))]


def test_the_wide_ensemble_against_long_double_and_its_members_launches_on_and_off():
    """padded dimension 12, members of 20, 300 and 600 rows: tri_cols' K slices 64 and 128 and a member below 128 rows in one call"""
    test_an_ensemble_of_three_against_long_double_and_its_members_launches_on_and_off(er.ENSEMBLE_WIDE)


def test_an_ensemble_of_three_against_long_double_and_its_members_launches_on_and_off(e=er.ENSEMBLE):
    ep = er.make_ensemble(e)
    gps = _ensemble_gps(ep)
    for pending in (ep.pending, ep.pending[:0]):
        want = er.ensemble_expected(ep, pending, LD)
        runs = []
        for on in (True, False):
            with _Launches(on):
                runs.append(api.ei_analytic_ensemble(gps, ep.points, ep.best, points_being_sampled=pending))
        ei, grad = runs[0]
        assert np.array_equal(ei, runs[1][0]) and np.array_equal(grad, runs[1][1])
        e_v = max(abs(ei[i] - float(w[0])) / w[2] for i, w in enumerate(want))
        e_g = max(float(np.max(np.abs(grad[i] - w[1].astype(np.float64)))) / max(1.0, float(np.max(np.abs(w[1])))) for i, w in enumerate(want))
        print("ensemble of 3 (d = %d, n = %s), %d pending: value error %.3g scale, gradient error %.3g (bounds 1e-10)" % (
            e["d"], e["n"], len(pending), e_v, e_g))
        assert e_v <= 1e-10 and e_g <= 1e-10
        # the members' own E = 1 results, added on the host in member order and divided once
        single = [api.ei_analytic_ensemble(g, ep.points, [b], points_being_sampled=pending) for g, b in zip(gps, ep.best)]
        assert np.array_equal(ei, ((single[0][0] + single[1][0]) + single[2][0]) / 3)
        assert np.array_equal(grad, ((single[0][1] + single[1][1]) + single[2][1]) / 3)
        # no pending point through the symbol's pending arguments against NULL
        if len(pending) == 0:
            raw = _raw_eval(gps, ep.points, ep.best, pending)
            none = api.ei_analytic_ensemble(gps, ep.points, ep.best, points_being_sampled=None)
            assert np.array_equal(raw[0], none[0]) and np.array_equal(raw[1], none[1]) and np.array_equal(raw[0], ei)
    _close(gps)


# ---- 4. the floors ----
def test_a_sampled_point_of_a_noise_free_gp_returns_zero_not_an_error():
    rng = np.random.default_rng(17)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.3 * rng.normal(size=(6, 1))
    G = api.DeviceGP([1.3, 0.3, 0.3], X, y, [0.0])
    worst = int(np.argmax(y[:, 0]))  # (a sampled point that is not the best: t < 0 and var = 0 up to rounding)
    pts = np.vstack([X[worst], rng.uniform(0.1, 0.9, size=2)])
    scale = max(1.0, float(np.abs(y).max()), np.sqrt(1.3))
    ei, grad = api.ei_analytic_ensemble(G, pts, [float(y.min())])
    print("on a sampled point of a noise-free GP: EI %.3g, gradient %s; beside it EI %.3g" % (ei[0], grad[0], ei[1]))
    assert np.all(np.isfinite(ei)) and np.all(np.isfinite(grad)) and 0.0 <= ei[0] <= 1e-10 * scale and ei[1] > 1e-6
    G.close()


# ---- 5. the ascent against the host-driven loop ----
MS = dict(starts=12, steps=6, restarts=2, gamma=0.7, pre_mult=1.0, max_rel=0.5)
MS_WIDE = dict(MS, starts=6, steps=4, restarts=1)  # (the host-driven loop over 920 rows in 10 dimensions stays within seconds)


def _ascent_problem(tolerance, e=er.ENSEMBLE, MS=MS):
    ep = er.make_ensemble(e)
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], ep.points.shape[1]))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    bounds = np.array([[0.0, 1.0]] * ep.points.shape[1])
    return ep, starts, gd, bounds


def _host_loop(gps, ep, starts, gd, bounds, pending):
    """ms_restatement's optimiser, evaluations by api.ei_analytic_ensemble on the device, updates in numpy; a dict shaped like
    api.ei_analytic_multistart's, path included (a start that is not running repeats its point)"""
    d, T, R = starts.shape[1], gd[1], gd[2]

    def value_fn(x):
        return api.ei_analytic_ensemble(gps, np.asarray(x).reshape(-1, d), ep.best, points_being_sampled=pending, want_grad=False)

    seen, state = {}, {"round": -1, "points": None}

    def grad_fn(x):
        state["points"] = np.array(x, copy=True).reshape(-1, d)
        return api.ei_analytic_ensemble(gps, state["points"], ep.best, points_being_sampled=pending)[1].reshape(np.shape(x))

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


def _same_run(got, want):
    for key in ("start_values", "kept_index", "path", "steps_taken", "end_points", "end_values", "point"):
        assert np.array_equal(got[key], want[key]), key
    assert got["value"] == want["value"] and got["found"] == want["found"]


@pytest.mark.parametrize("tolerance", [1e-10, 6e-2], ids=["tight", "loose"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(tolerance):
    ep, starts, gd, bounds = _ascent_problem(tolerance)
    gps = _ensemble_gps(ep)
    pending = ep.pending[:2]
    want = _host_loop(gps, ep, starts, gd, bounds, pending)
    plain = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("tolerance %g: %d kept starts (fewer than 20), steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"] and want["value"] >= want["start_values"].max()
    # without the ascent: the best start by a strict compare in list order
    none = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts, gradient_ascent=False, points_being_sampled=pending)
    best = int(np.argmax(want["start_values"]))
    assert np.array_equal(none["point"], starts[best]) and none["value"] == want["start_values"][best] and none["found"]
    assert np.array_equal(none["start_values"], want["start_values"])
    _close(gps)


def test_the_ascent_on_the_wide_ensemble_is_the_host_driven_loop_bit_for_bit():
    """the ascent's own staging and step at padded dimension 12 over members of 20, 300 and 600 rows"""
    ep, starts, gd, bounds = _ascent_problem(1e-10, er.ENSEMBLE_WIDE, MS_WIDE)
    gps = _ensemble_gps(ep)
    pending = ep.pending[:2]
    want = _host_loop(gps, ep, starts, gd, bounds, pending)
    plain = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    moved = float(np.max(np.abs(want["end_points"] - starts[want["kept_index"]])))
    print("wide ensemble: %d kept starts, steps taken %s, value %.12g against the best start's %.12g; the ends lie up to %.3g from "
          "their starts" % (len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max(), moved))
    assert want["found"] and len(want["kept_index"]) == MS_WIDE["starts"] and moved > 1e-3 and int(want["steps_taken"].max()) == 4
    _close(gps)


def test_the_batch_on_the_wide_ensemble_is_the_ascent_fed_its_predecessor_bit_for_bit():
    ep, starts, gd, bounds = _ascent_problem(1e-10, er.ENSEMBLE_WIDE, MS_WIDE)
    gps = _ensemble_gps(ep)
    pending = ep.pending[:1]
    first = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts, points_being_sampled=pending)
    second = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts, points_being_sampled=np.vstack([pending, first["point"][None, :]]))
    assert first["found"] and second["found"]
    for on in (True, False):
        with _Launches(on):
            got = api.ei_analytic_suggest(gps, gd, bounds, ep.best, starts, 2, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array([first["point"], second["point"]])), on
        assert np.array_equal(got["values"], np.array([first["value"], second["value"]])) and np.all(got["found"])
    print("wide ensemble: greedy values %.12g, %.12g; the second pick lies %.3g from the first" % (
        first["value"], second["value"], float(np.max(np.abs(second["point"] - first["point"])))))
    _close(gps)


# ---- 6. greedy batches ----
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    ep, starts, gd, bounds = _ascent_problem(1e-10)
    gps = _ensemble_gps(ep)
    pending, q = ep.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.ei_analytic_suggest(gps, gd, bounds, ep.best, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    # the effect of b': every pick differs from the picks before it by > 1e-3 in some coordinate
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) > 1e-3
    # no pending points: round 0 is the plain ascent
    one = api.ei_analytic_suggest(gps, gd, bounds, ep.best, starts, 2)
    plain = api.ei_analytic_multistart(gps, gd, bounds, ep.best, starts)
    assert np.array_equal(one["points"][0], plain["point"]) and one["values"][0] == plain["value"]
    _close(gps)


def test_sixty_four_rows_are_accepted_at_twenty_sampled_points():
    p = [c for c in er.PROBLEMS if c.name == "n20_d2_A12_p64"][0]
    G = _gp(p)
    gd = (6, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    starts = np.random.default_rng(5).uniform(0.05, 0.95, size=(6, 2))
    got = api.ei_analytic_suggest(G, gd, [[0, 1], [0, 1]], [p.best], starts, 64, gradient_ascent=False, points_being_sampled=p.pending[:1])
    assert got["points"].shape == (64, 2) and np.all(got["found"]) and np.all(np.isfinite(got["values"])) and np.all(got["values"] >= 0)
    with pytest.raises(api.BoundsException) as e:
        api.ei_analytic_suggest(G, gd, [[0, 1], [0, 1]], [p.best], starts, 65, gradient_ascent=False, points_being_sampled=p.pending[:1])
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 1.0, 64.0)
    G.close()


def test_a_pending_point_listed_twice_in_a_noise_free_member_is_singular():
    """tests/test_gpu_kg1_pending.py's construction: alpha = 1e-3 and noise 0 in the second member, a pending point 0.05 from a sampled
    point listed twice; the second copy's Schur pivot is a few ulp of alpha, far under the pivot rule's 1e-16.  An error return with
    payload (member, index of the pending point in the combined list), not a fault; in a batch the index counts the caller's points
    first and then the picks."""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    gps = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]
    bests = [float(y.min())] * 2
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.ei_analytic_ensemble(gps, starts, bests, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 3) and "pending point 3" in str(e.value)
            with pytest.raises(api.SingularMatrixException) as e:
                api.ei_analytic_multistart(gps, gd, [[0, 1], [0, 1]], bests, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 3)
    ok = api.ei_analytic_ensemble(gps, starts, bests, want_grad=False, points_being_sampled=pending[:3])  # (the handles still answer)
    assert np.all(np.isfinite(ok))
    _close(gps)


# ---- 7. the wrapper, on Branin with 8 points ----
def test_the_wrapper_and_the_optimisation_run_end_to_end_on_branin():
    import wrappers_mirror as cw
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(8, dim))
    a, b = 15.0 * X[:, 0] - 5.0, 15.0 * X[:, 1]
    y = (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0
    ys = (y - y.mean()) / y.std()
    hypers = np.array([[1.0, 0.3, 0.3], [1.4, 0.25, 0.4], [0.8, 0.45, 0.3]])
    hd = cw.HistoricalData(dim=dim, num_derivatives=0)
    hd.append_sample_points([cw.SamplePoint(X[i], [ys[i]], noise) for i in range(X.shape[0])])
    gpm = cw.GaussianProcessMCMC(hypers, np.full((num_mcmc, 1), noise), hd, [])
    models = gpm.member_models()
    ei = eia.AnalyticExpectedImprovementMCMC(models)
    assert ei.problem_size == dim and np.array_equal(ei.best_so_far, np.full(num_mcmc, ys.min()))
    members = eia._device_members(models)
    cand = rng.uniform(size=(7, dim))
    want_v, want_g = api.ei_analytic_ensemble(members, cand, ei.best_so_far)
    assert np.array_equal(ei.evaluate_at_point_list(cand), want_v)
    ei.set_current_point(cand[3])
    assert ei.compute_objective_function() == want_v[3] and np.array_equal(ei.compute_grad_objective_function(), want_g[3:4])
    gd = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    bounds = [[0.0, 1.0]] * dim
    points, values, found = eia.multistart_analytic_expected_improvement_optimization(models, bounds, gd, num_multistarts=16, num_to_sample=3,
                                                                                      seed=31)
    assert points.shape == (3, dim) and values.shape == (3,) and np.all(found)
    assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values)) and values[0] > 0.0
    starts = api.latin_hypercube(31, bounds, 16)
    first = api.ei_analytic_multistart(members, gd, bounds, ei.best_so_far, starts)
    assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
    again = eia.multistart_analytic_expected_improvement_optimization(models, bounds, gd, starts=starts, points_being_sampled=points[:1])
    assert np.array_equal(again[0][0], points[1]) and again[1][0] == values[1]
    print("Branin, 8 points, 3 members: a batch of 3 at %s, values %s" % (np.round(points, 3).tolist(), [float(v) for v in values]))
