"""The ensemble min-value entropy acquisition GIBBON on the device (csrc/gibbon1.hip: moe_gibbon_mcmc, moe_gibbon_mcmc_multistart,
moe_gibbon_mcmc_suggest) against the long-double restatement of tests/gibbon_reference.py, on the cases gibbon_reference.PROBLEMS
and WIDE_PROBLEMS, whose inputs tests/test_gibbon_reference.py qualifies on the CPU (float64 within 2.5e-11 scale of long double, gamma in [-6, 40],
sigma0 >= 0.05 sqrt(alpha), P and the min-values each move a checked candidate's value by >= 1e-5 scale: a device that ignored
either fails here).

Tolerances: |value - want| <= 1e-10 scale and |grad - want|_inf <= 1e-10 scale at EVERY candidate of a case.  Everything else is bit
for bit: value-only against value + gradient, a candidate alone against itself in a batch and across the pass boundary, the ensemble
against its members added on the host, ensemble-wide launches on against off, K = 64 against K = 65 with a 65th term that is an exact
zero, the ascent against a host-driven loop over the evaluator (tests/ms_restatement.py), the greedy batch against calls of the
ascent fed their predecessors' points.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.17 records those
of the first run."""
import ctypes as C

import numpy as np
import pytest

import ei1_reference as er
import gibbon_reference as gr
import kg1_pending_reference as kp
import kg1_reference as kr
import ms_restatement as ms
from cornell_moe_amd import _lib, api, min_value_entropy as mve

pytestmark = pytest.mark.gpu

LD = kr.LD
dp, ip = _lib.dp, _lib.ip


def _gp(p):
    return api.DeviceGP(p.hyper, p.X, p.y, p.noise, list(p.derivs), cov_type=p.cov_type)


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


def _raw_eval(gps, points, mins, pending, want_grad=True):
    """moe_gibbon_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array"""
    arr, E, d, keep, m, K = api._gibbon_members(gps, mins)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    num = pend.shape[0] - 1
    value, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(_lib.load().moe_gibbon_mcmc(arr, E, m.ctypes.data_as(dp), K, pend.ctypes.data_as(dp), num, pts.ctypes.data_as(dp),
                                           len(pts), 1 if want_grad else 0, value.ctypes.data_as(dp),
                                           grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
    return value, grad


def _errors(value, grad, want, which):
    e_v = max(abs(value[i] - float(want[i].value)) / want[i].scale for i in which)
    e_g = max(float(np.max(np.abs(grad[i] - want[i].grad.astype(np.float64)))) / want[i].scale for i in which)
    return e_v, e_g


# ---- 1. value and gradient against long double ----
@pytest.mark.parametrize("p", gr.PROBLEMS + gr.WIDE_PROBLEMS, ids=lambda p: p.name)
def test_against_the_long_double_restatement(p):
    want, without, _ = gr.expected(p)
    G = _gp(p)
    C_, d = p.points.shape
    value, grad = api.gibbon_ensemble(G, p.points, p.mins, points_being_sampled=p.pending)
    assert value.shape == (C_,) and grad.shape == (C_, d) and np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    e_v, e_g = _errors(value, grad, want, range(C_))
    moved = max(abs(value[i] - float(without[i])) / want[i].scale for i in p.checked)
    print("%s (K = %d): value error %.3g scale, gradient error %.3g scale (bounds 1e-10); P moved the value by up to %.3g scale" % (
        p.name, len(p.mins), e_v, e_g, moved))
    assert e_v <= 1e-10 and e_g <= 1e-10, (p.name, e_v, e_g)
    # the symbol itself (an empty list reaches it as num_being_sampled = 0 beside a non-NULL array): the same bits
    v2, g2 = _raw_eval([G], p.points, p.mins, p.pending)
    assert np.array_equal(value, v2) and np.array_equal(grad, g2)
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(api.gibbon_ensemble(G, p.points, p.mins, points_being_sampled=p.pending, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1 = api.gibbon_ensemble(G, p.points[i:i + 1], p.mins, points_being_sampled=p.pending)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), (p.name, i)
    G.close()


# ---- 2. bit for bit ----
_N8 = kp.Case("n8_d2_p2_two_passes", 44, 8, 2, 1, 2, 0, kr.MATERN, 1e-3, 4100)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(_N8.n)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    q = kp.make_problem(_N8)
    edge = (0, per_pass - 1, per_pass, _N8.C - 1)
    p = gr.Problem(_N8.name, _N8.cov_type, q.hyper, q.X, q.y, q.noise, (), q.points, q.pending, None, edge)
    p = p._replace(mins=gr.draw_min_values(gr.base_model(p, np.float64), 65, 44))
    base = gr.base_model(p, LD)
    model = gr.conditioned(base, p.pending)
    want = {i: gr.evaluate(base, model, p.points[i], p.mins, float(np.max(np.abs(p.y)))) for i in edge}
    G = _gp(p)
    for pending in (p.pending, None):
        value, grad = api.gibbon_ensemble(G, p.points, p.mins, points_being_sampled=pending)
        assert np.array_equal(api.gibbon_ensemble(G, p.points, p.mins, points_being_sampled=pending, want_grad=False), value)
        for i in edge:
            v1, g1 = api.gibbon_ensemble(G, p.points[i:i + 1], p.mins, points_being_sampled=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            e_v, e_g = _errors(value, grad, want, edge)
            print("%s: value error %.3g scale, gradient error %.3g scale on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= 1e-10 and e_g <= 1e-10
    G.close()


def test_a_pass_shorter_than_4096_candidates_above_4096_rows():
    """tests/test_gpu_ei1.py's 4097-row GP, where a pass holds 4032 candidates, under 64 min-values spread about the median of y
    (gamma on both sides of 0): value-only against value + gradient and a candidate alone against itself in the batch, bit for bit,
    on both sides of the boundary"""
    from test_gpu_ei1 import short_pass_problem
    q = short_pass_problem()
    mins = q.best + np.linspace(-0.3, 0.1, 64)
    G = api.DeviceGP(q.hyper, q.X, q.y, q.noise, cov_type=q.cov_type)
    for pending in (q.pending, None):
        value, grad = api.gibbon_ensemble(G, q.points, mins, points_being_sampled=pending)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
        assert np.array_equal(api.gibbon_ensemble(G, q.points, mins, points_being_sampled=pending, want_grad=False), value)
        for i in q.checked:
            v1, g1 = api.gibbon_ensemble(G, q.points[i:i + 1], mins, points_being_sampled=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        print("%s, %s pending: values of the four %s, their largest |gradient| entries %s" % (
            q.name, "2" if pending is not None else "no", [float(value[i]) for i in q.checked],
            [float(np.max(np.abs(grad[i]))) for i in q.checked]))
        assert all(abs(value[i]) > 1e-6 and np.max(np.abs(grad[i])) > 1e-6 for i in q.checked)  # (no comparison of zeros)
    G.close()


def _ensemble_gps(ep):
    return [api.DeviceGP(ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], cov_type=ep.cov[k]) for k in range(len(ep.X))]


def test_the_wide_ensemble_against_long_double_and_its_members_launches_on_and_off():
    """padded dimension 12, members of 20, 300 and 600 rows: tri_cols' K slices 64 and 128 and a member below 128 rows in one call"""
    test_an_ensemble_of_three_against_long_double_and_its_members_launches_on_and_off(er.ENSEMBLE_WIDE)


def test_an_ensemble_of_three_against_long_double_and_its_members_launches_on_and_off(e=er.ENSEMBLE):
    ep, mins = gr.make_ensemble(e)
    gps = _ensemble_gps(ep)
    for pending in (ep.pending, ep.pending[:0]):
        want = gr.ensemble_expected(ep, mins, pending, LD)
        runs = []
        for on in (True, False):
            with _Launches(on):
                runs.append(api.gibbon_ensemble(gps, ep.points, mins, points_being_sampled=pending))
        value, grad = runs[0]
        assert np.array_equal(value, runs[1][0]) and np.array_equal(grad, runs[1][1])
        e_v = max(abs(value[i] - float(w[0])) / w[2] for i, w in enumerate(want))
        e_g = max(float(np.max(np.abs(grad[i] - w[1].astype(np.float64)))) / w[2] for i, w in enumerate(want))
        print("ensemble of 3 (d = %d, n = %s), %d pending: value error %.3g scale, gradient error %.3g scale (bounds 1e-10)" % (
            e["d"], e["n"], len(pending), e_v, e_g))
        assert e_v <= 1e-10 and e_g <= 1e-10
        # the members' own E = 1 results, added on the host in member order and divided once
        single = [api.gibbon_ensemble(g, ep.points, m, points_being_sampled=pending) for g, m in zip(gps, mins)]
        assert np.array_equal(value, ((single[0][0] + single[1][0]) + single[2][0]) / 3)
        assert np.array_equal(grad, ((single[0][1] + single[1][1]) + single[2][1]) / 3)
        # no pending point through the symbol's pending arguments against NULL
        if len(pending) == 0:
            raw = _raw_eval(gps, ep.points, mins, pending)
            none = api.gibbon_ensemble(gps, ep.points, mins, points_being_sampled=None)
            assert np.array_equal(raw[0], none[0]) and np.array_equal(raw[1], none[1]) and np.array_equal(raw[0], value)
    _close(gps)


def test_a_sixty_fifth_min_value_whose_term_is_an_exact_zero_changes_the_divisor_alone():
    """K = 64 against K = 65 at p = 0, where the value is (sum of the terms) / K and nothing else: the 65th min-value lies 1e6 below
    every mean, gamma > 1e5, erfcx overflows, r = q = 0 and G = -1/2 log1p(-0) = 0 exactly, and it lands on lane 0 behind that lane's
    first term.  64 value_64 is the sum exactly (a power of two), and the device's division is correctly rounded, so value_65 must
    be (64 value_64) / 65 to the last bit.  The gradient's sums gain exact zeros likewise, but pass through products with 1 / K
    before the triangular solve: K grad is compared to rounding, 1e-12 of its largest entry (two solves and a sum over N = 20 rows
    are some 10^3 roundings of 1.1e-16 each, with room for a tenfold cancellation)."""
    p = [q for q in gr.PROBLEMS if q.name == "n20_d6_p0"][0]
    assert len(p.mins) == 64 and len(p.pending) == 0
    G = _gp(p)
    v64, g64 = api.gibbon_ensemble(G, p.points, p.mins)
    v65, g65 = api.gibbon_ensemble(G, p.points, np.concatenate([p.mins, [-1e6]]))
    assert np.all(v64 > 0.0) and np.array_equal(v65, (v64 * 64.0) / 65.0)
    rel = float(np.max(np.abs(g65 * 65.0 - g64 * 64.0)) / np.max(np.abs(g64 * 64.0)))
    print("K = 64 against K = 65: values equal bit for bit after the divisor; gradients times K differ by %.3g relative" % rel)
    assert rel <= 1e-12
    G.close()


# ---- 3. the floors ----
def test_a_sampled_point_of_a_noise_free_gp_has_a_finite_value_and_gradient():
    rng = np.random.default_rng(17)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.3 * rng.normal(size=(6, 1))
    G = api.DeviceGP([1.3, 0.3, 0.3], X, y, [0.0])
    pts = np.vstack([X[int(np.argmax(y[:, 0]))], X[int(np.argmin(y[:, 0]))], rng.uniform(0.1, 0.9, size=2)])
    mins = np.array([float(y.min()) - 0.5, float(y.min()) + 0.1, -2.0])  # (the second lies above the mean at the best sampled point)
    for pending in (None, pts[2:3] + 0.2):
        value, grad = api.gibbon_ensemble(G, pts, mins, points_being_sampled=pending)
        print("on two sampled points of a noise-free GP and beside them: values %s, largest |gradient| entries %s" % (
            value, np.max(np.abs(grad), axis=1)))
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
        if pending is None:
            assert np.all(value >= 0.0) and value[2] > 1e-6
    G.close()


# ---- 4. the ascent against the host-driven loop ----
MS = dict(starts=12, steps=6, restarts=2, gamma=0.7, pre_mult=1.0, max_rel=0.5)
MS_WIDE = dict(MS, starts=6, steps=4, restarts=1)  # (the host-driven loop over 920 rows in 10 dimensions stays within seconds)


def _ascent_problem(tolerance, e=er.ENSEMBLE, MS=MS):
    ep, mins = gr.make_ensemble(e)
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], ep.points.shape[1]))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    bounds = np.array([[0.0, 1.0]] * ep.points.shape[1])
    return ep, mins, starts, gd, bounds


def _host_loop(gps, mins, starts, gd, bounds, pending):
    """ms_restatement's optimiser, evaluations by api.gibbon_ensemble on the device, updates in numpy; a dict shaped like
    api.gibbon_multistart's, path included (a start that is not running repeats its point)"""
    d, T, R = starts.shape[1], gd[1], gd[2]

    def value_fn(x):
        return api.gibbon_ensemble(gps, np.asarray(x).reshape(-1, d), mins, points_being_sampled=pending, want_grad=False)

    seen, state = {}, {"round": -1, "points": None}

    def grad_fn(x):
        state["points"] = np.array(x, copy=True).reshape(-1, d)
        return api.gibbon_ensemble(gps, state["points"], mins, points_being_sampled=pending)[1].reshape(np.shape(x))

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
    ep, mins, starts, gd, bounds = _ascent_problem(tolerance)
    gps = _ensemble_gps(ep)
    pending = ep.pending[:2]
    want = _host_loop(gps, mins, starts, gd, bounds, pending)
    plain = api.gibbon_multistart(gps, gd, bounds, mins, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.gibbon_multistart(gps, gd, bounds, mins, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("tolerance %g: %d kept starts (fewer than 20), steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"] and want["value"] >= want["start_values"].max()
    # without the ascent: the best start by a strict compare in list order
    none = api.gibbon_multistart(gps, gd, bounds, mins, starts, gradient_ascent=False, points_being_sampled=pending)
    best = int(np.argmax(want["start_values"]))
    assert np.array_equal(none["point"], starts[best]) and none["value"] == want["start_values"][best] and none["found"]
    assert np.array_equal(none["start_values"], want["start_values"])
    assert none["kept_index"] is None and none["end_points"] is None
    _close(gps)


def test_the_ascent_on_the_wide_ensemble_is_the_host_driven_loop_bit_for_bit():
    """the ascent's own staging and step at padded dimension 12 over members of 20, 300 and 600 rows"""
    ep, mins, starts, gd, bounds = _ascent_problem(1e-10, er.ENSEMBLE_WIDE, MS_WIDE)
    gps = _ensemble_gps(ep)
    pending = ep.pending[:2]
    want = _host_loop(gps, mins, starts, gd, bounds, pending)
    plain = api.gibbon_multistart(gps, gd, bounds, mins, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.gibbon_multistart(gps, gd, bounds, mins, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    moved = float(np.max(np.abs(want["end_points"] - starts[want["kept_index"]])))
    print("wide ensemble: %d kept starts, steps taken %s, value %.12g against the best start's %.12g; the ends lie up to %.3g from "
          "their starts" % (len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max(), moved))
    assert want["found"] and len(want["kept_index"]) == MS_WIDE["starts"] and moved > 1e-3 and int(want["steps_taken"].max()) == 4
    _close(gps)


def test_the_batch_on_the_wide_ensemble_is_the_ascent_fed_its_predecessor_bit_for_bit():
    ep, mins, starts, gd, bounds = _ascent_problem(1e-10, er.ENSEMBLE_WIDE, MS_WIDE)
    gps = _ensemble_gps(ep)
    pending = ep.pending[:1]
    first = api.gibbon_multistart(gps, gd, bounds, mins, starts, points_being_sampled=pending)
    second = api.gibbon_multistart(gps, gd, bounds, mins, starts, points_being_sampled=np.vstack([pending, first["point"][None, :]]))
    assert first["found"] and second["found"]
    for on in (True, False):
        with _Launches(on):
            got = api.gibbon_suggest(gps, gd, bounds, mins, starts, 2, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array([first["point"], second["point"]])), on
        assert np.array_equal(got["values"], np.array([first["value"], second["value"]])) and np.all(got["found"])
    print("wide ensemble: greedy values %.12g, %.12g; the second pick lies %.3g from the first" % (
        first["value"], second["value"], float(np.max(np.abs(second["point"] - first["point"])))))
    _close(gps)


# ---- 5. greedy batches ----
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    ep, mins, starts, gd, bounds = _ascent_problem(1e-10)
    gps = _ensemble_gps(ep)
    pending, q = ep.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = api.gibbon_multistart(gps, gd, bounds, mins, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.gibbon_suggest(gps, gd, bounds, mins, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    # the effect of the bracket: every pick differs from the picks before it by > 1e-3 in some coordinate
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) > 1e-3
    # no pending points: round 0 is the plain ascent
    one = api.gibbon_suggest(gps, gd, bounds, mins, starts, 2)
    plain = api.gibbon_multistart(gps, gd, bounds, mins, starts)
    assert np.array_equal(one["points"][0], plain["point"]) and one["values"][0] == plain["value"]
    _close(gps)


def test_a_noise_free_batch_does_not_pick_its_first_point_again():
    """the case plain max-value entropy search fails: its value depends on gamma alone and is the same at the pending pick.  The
    second round's starts include the first pick itself, where varc is 0 up to rounding: the bracket is 1/2 log(varc / var0) with
    varc between DBL_MIN and a few ulp of alpha, below -17."""
    p = [q for q in gr.PROBLEMS if q.name == gr.NOISE_FREE][0]
    G = _gp(p)
    bounds = np.array([[0.0, 1.0]] * 2)
    starts = np.random.default_rng(9).uniform(0.05, 0.95, size=(8, 2))
    gd = (9, 6, 2, 0, 0.7, 1.0, 0.5, 1e-10)
    first = api.gibbon_multistart(G, gd, bounds, p.mins, starts)
    again = np.vstack([first["point"], starts])
    second = api.gibbon_multistart(G, gd, bounds, p.mins, again, points_being_sampled=first["point"][None, :])
    gap = float(np.max(np.abs(second["point"] - first["point"])))
    print("noise-free: first pick %s (value %.6g), its value as a start of round two %.6g, second pick %s (value %.6g), gap %.3g" % (
        first["point"], first["value"], second["start_values"][0], second["point"], second["value"], gap))
    assert first["found"] and second["found"] and np.all(np.isfinite(second["start_values"]))
    assert second["start_values"][0] < -10.0 and second["value"] > second["start_values"][0] and gap > 1e-3
    both = api.gibbon_suggest(G, gd, bounds, p.mins, again, 2)
    assert float(np.max(np.abs(both["points"][1] - both["points"][0]))) > 1e-3
    G.close()


# ---- 6. limits ----
def test_the_limits_of_the_extension_and_of_the_min_values():
    p = [c for c in gr.PROBLEMS if c.name == "n20_d2_A12_p64"][0]
    G = _gp(p)
    gd = (6, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    bounds = [[0, 1], [0, 1]]
    starts = np.random.default_rng(5).uniform(0.05, 0.95, size=(6, 2))
    got = api.gibbon_suggest(G, gd, bounds, p.mins, starts, 64, gradient_ascent=False, points_being_sampled=p.pending[:1])
    assert got["points"].shape == (64, 2) and np.all(got["found"]) and np.all(np.isfinite(got["values"]))
    with pytest.raises(api.BoundsException) as e:
        api.gibbon_suggest(G, gd, bounds, p.mins, starts, 65, gradient_ascent=False, points_being_sampled=p.pending[:1])
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 1.0, 64.0)
    assert np.all(np.isfinite(api.gibbon_ensemble(G, starts, p.mins, points_being_sampled=p.pending[:64], want_grad=False)))
    with pytest.raises(api.BoundsException) as e:
        api.gibbon_ensemble(G, starts, p.mins, points_being_sampled=np.vstack([p.pending, p.pending[:1] + 0.01]))
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 0.0, 64.0)
    # K = 1024 accepted, 1025 refused
    many = np.linspace(-3.0, -1.0, 1025)
    assert np.all(np.isfinite(api.gibbon_ensemble(G, starts, many[:1024], want_grad=False)))
    with pytest.raises(api.BoundsException) as e:
        api.gibbon_ensemble(G, starts, many)
    assert (e.value.value, e.value.min, e.value.max) == (1025.0, 1.0, 1024.0)
    G.close()
    # g = 2: 21 pending points are 63 rows, 22 are 66
    q = [c for c in gr.PROBLEMS if c.name == gr.G2][0]
    H = _gp(q)
    pend = np.random.default_rng(6).uniform(0.05, 0.95, size=(22, 2))
    value, grad = api.gibbon_ensemble(H, q.points, q.mins, points_being_sampled=pend[:21])
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad))
    with pytest.raises(api.BoundsException) as e:
        api.gibbon_ensemble(H, q.points, q.mins, points_being_sampled=pend)
    assert (e.value.value, e.value.min, e.value.max) == (22.0, 0.0, 21.0)
    H.close()


def test_a_pending_point_listed_twice_in_a_noise_free_member_is_singular():
    """tests/test_gpu_ei1.py's construction: alpha = 1e-3 and noise 0 in the second member, a pending point 0.05 from a sampled point
    listed twice.  An error return with payload (member, index of the pending point), not a fault; the handles still answer."""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    gps = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]
    mins = np.full((2, 5), float(y.min()) - 0.05)
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.gibbon_ensemble(gps, starts, mins, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 3) and "pending point 3" in str(e.value)
            with pytest.raises(api.SingularMatrixException) as e:
                api.gibbon_multistart(gps, gd, [[0, 1], [0, 1]], mins, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 3)
    ok = api.gibbon_ensemble(gps, starts, mins, want_grad=False, points_being_sampled=pending[:3])  # (the handles still answer)
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
    bounds = [[0.0, 1.0]] * dim
    cand = np.vstack([api.latin_hypercube(5, bounds, 100), X])
    mins = mve.sample_min_values(models, cand, 64, 11)
    assert mins.shape == (num_mcmc, 64) and np.all(np.isfinite(mins)) and np.all(mins <= ys.min() + 0.1)
    assert np.array_equal(mins, mve.sample_min_values(models, cand, 64, 11)) and len(np.unique(mins)) > 100
    obj = mve.MinValueEntropyMCMC(models, mins)
    assert obj.problem_size == dim and np.array_equal(obj.min_values, mins)
    members = mve._device_members(models)
    pts = rng.uniform(size=(7, dim))
    want_v, want_g = api.gibbon_ensemble(members, pts, mins)
    assert np.array_equal(obj.evaluate_at_point_list(pts), want_v) and np.all(want_v >= 0.0)
    obj.set_current_point(pts[3])
    assert obj.compute_objective_function() == want_v[3] and np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
    gd = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    points, values, found = mve.multistart_min_value_entropy_optimization(models, bounds, gd, num_multistarts=16, num_to_sample=3,
                                                                          min_values=mins, seed=31)
    assert points.shape == (3, dim) and values.shape == (3,) and np.all(found)
    assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values)) and values[0] > 0.0
    starts = api.latin_hypercube(31, bounds, 16)
    first = api.gibbon_multistart(members, gd, bounds, mins, starts)
    assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
    again = mve.multistart_min_value_entropy_optimization(models, bounds, gd, starts=starts, points_being_sampled=points[:1], min_values=mins)
    assert np.array_equal(again[0][0], points[1]) and again[1][0] == values[1]
    # the defaults: the optimiser draws its own min-values at Latin-hypercube candidates joined with the observed points
    auto = mve.multistart_min_value_entropy_optimization(models, bounds, gd, num_multistarts=16, seed=31)
    assert auto[0].shape == (1, dim) and bool(auto[2][0]) and np.isfinite(auto[1][0]) and auto[1][0] > 0.0
    assert len(mve._observed_points(models, dim)) == 8
    print("Branin, 8 points, 3 members: a batch of 3 at %s, values %s; min-values from %.3f to %.3f (best observed %.3f)" % (
        np.round(points, 3).tolist(), [float(v) for v in values], mins.min(), mins.max(), ys.min()))
