"""The ensemble analytic expected improvement of GPs with derivative observations on the device (csrc/ei1.hip with
csrc/kg1_pending.hip's rows of 1 + g believed observations per pending point) against the long-double restatement of
tests/ei1_deriv_reference.py, on its PROBLEMS and WIDE_PROBLEMS with and without their pending points.  tests/test_ei1_deriv_reference.py qualifies the
inputs on the CPU: float64 within 2.5e-11 scale of long double, sigma >= 0.05 sqrt(alpha), and P, P's derivative rows and X's
derivative observations each move a checked candidate's value by >= 1e-5 scale, so a device that dropped any of them fails here.

Tolerances are tests/test_gpu_ei1.py's: |EI - want| <= 1e-10 scale, |grad EI - want|_inf <= 1e-10 max(1, |want|_inf).  Everything
else is bit for bit: value-only against value + gradient, a candidate alone against itself in a batch and across the pass boundary,
the ensemble against its members added on the host, ensemble-wide launches on against off, the ascent against a host-driven loop over
the evaluator, the greedy batch against calls of the ascent fed their predecessors' points.  Every test prints the worst figures it
saw (pytest -s); DESIGN.md section 5.16 records those of the first run.  Before derivative observations were accepted every call
here raised BoundsException."""
import numpy as np
import pytest

import ei1_deriv_reference as dr
import ei1_reference as er
import kg1_reference as kr
from cornell_moe_amd import _lib, api, expected_improvement_analytic as eia
from test_gpu_ei1 import _Launches, _close, _errors, _host_loop, _raw_eval, _same_run

pytestmark = pytest.mark.gpu

LD = kr.LD


def _gp(p):
    return api.DeviceGP(p.hyper, p.X, p.y, p.noise, p.derivs, cov_type=p.cov_type)


# ---- 1. value and gradient against long double, with and without P ----
@pytest.mark.parametrize("p", dr.PROBLEMS + dr.PROBLEMS_P0 + dr.WIDE_PROBLEMS + dr.WIDE_PROBLEMS_P0, ids=lambda p: p.name)
def test_against_the_long_double_restatement(p):
    want = dr.expected(p)
    G = _gp(p)
    C_, d = p.points.shape
    ei, grad = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending)
    assert ei.shape == (C_,) and grad.shape == (C_, d) and np.all(np.isfinite(ei)) and np.all(np.isfinite(grad))
    e_v, e_g = _errors(ei, grad, want, p.checked)
    print("%s: value error %.3g scale, gradient error %.3g (bounds 1e-10)" % (p.name, e_v, e_g))
    assert e_v <= 1e-10 and e_g <= 1e-10, (p.name, e_v, e_g)
    # the symbol itself (an empty list reaches it as num_being_sampled = 0 beside a non-NULL array): the same bits
    ei2, grad2 = _raw_eval([G], p.points, [p.best], p.pending)
    assert np.array_equal(ei, ei2) and np.array_equal(grad, grad2)
    if len(p.pending) == 0:
        none = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=None)
        assert np.array_equal(none[0], ei) and np.array_equal(none[1], grad)
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending, want_grad=False), ei)
    for i in (0, C_ - 1):
        e1, g1 = api.ei_analytic_ensemble(G, p.points[i:i + 1], [p.best], points_being_sampled=p.pending)
        assert e1[0] == ei[i] and np.array_equal(g1[0], grad[i]), (p.name, i)
    G.close()


def test_the_believed_best_binds():
    p = [q for q in dr.PROBLEMS if q.name == dr.BPRIME][0]
    want = dr.expected(p)
    G = _gp(p)
    ei = api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending, want_grad=False)
    # with the caller's best value left as it is the expected improvement would be far larger
    base = dr.base_model(p, LD)
    cond = dr.DerivPendingModel(base, p.pending)
    wrong = []
    for i in p.checked:
        x = p.points[i].reshape(1, -1)
        k = np.ascontiguousarray(cond.rows_cov(x, ())[:, 0])
        mu, var = LD(base.mean) + k @ cond.kinvy, dr.conditioned_variance(cond, x)
        t, s = LD(p.best) - mu, np.sqrt(var)
        wrong.append(float(t * er.normal_cdf(t / s, LD) + s * kr.normal_pdf(t / s, LD)))
    gap = min(abs(w - float(want[i].value)) for w, i in zip(wrong, p.checked))
    print("b' = %.4f against best = %.4f: EI with the caller's best differs by >= %.3g" % (want[0].bprime, p.best, gap))
    assert gap > 1e-3 and max(abs(ei[i] - float(want[i].value)) for i in p.checked) <= 1e-10 * want[0].scale
    G.close()


# ---- 2. the reference's recorded values on the six fixtures with derivative observations, and the host-finished path ----
def test_the_fixtures_of_the_reference_and_the_host_finished_path(golden):
    cases, _ = golden
    seen, worst = 0, [0.0, 0.0, 0.0, 0.0]
    for c in cases:
        i = c.inp
        if not len(i["derivs"]):
            continue
        seen += 1
        G = api.DeviceGP(np.concatenate([[float(i["alpha"])], i["lengths"]]), i["X"], i["y"], i["noise"], [int(v) for v in i["derivs"]],
                         cov_type=int(i["cov_type"]))
        best = float(i["ei_best"])
        ei, grad = api.ei_analytic_ensemble(G, i["query"], [best])
        ref_ei, ref_grad = c.out["ei_analytic"], c.out["grad_ei_analytic"]
        old_ei, old_grad = G.ei_analytic_batch(i["query"], best)
        sv, sg = max(np.abs(ref_ei).max(), 1e-6), max(np.abs(ref_grad).max(), 1e-6)
        figs = [np.abs(ei - ref_ei).max() / sv, np.abs(grad - ref_grad).max() / sg, np.abs(ei - old_ei).max() / sv,
                np.abs(grad - old_grad).max() / sg]
        worst = [max(a, float(b)) for a, b in zip(worst, figs)]
        assert figs[0] <= 1e-11 and figs[1] <= 1e-9 and figs[2] <= 1e-11 and figs[3] <= 1e-9, (c.index, figs)
        G.close()
    print("%d fixture cases with derivative observations: against the reference %.3g / %.3g, against ei_analytic_batch %.3g / %.3g "
          "(bounds 1e-11 / 1e-9)" % (seen, worst[0], worst[1], worst[2], worst[3]))
    assert seen == 6


# ---- 3. bit for bit ----
_N8 = dr.Case("n4_d2_D1_p2_two_passes", 44, 4, 2, (1,), 2, kr.MATERN, 1e-3, 4100, False, False)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    q = dr.make_problem(_N8)
    per_pass = _lib.load().moe_ei1_pass_size(q.y.size)
    assert q.y.size == 8 and per_pass == 4096 and _N8.C == per_pass + 4
    p = q._replace(checked=(0, per_pass - 1, per_pass, _N8.C - 1))
    want = dr.expected(p)
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


def _ensemble_gps(ep):
    return [api.DeviceGP(ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], ep.derivs, cov_type=ep.cov[k]) for k in range(len(ep.X))]


def test_an_ensemble_of_three_against_long_double_and_its_members_launches_on_and_off():
    ep = dr.make_ensemble()
    gps = _ensemble_gps(ep)
    for pending in (ep.pending, ep.pending[:0]):
        want = dr.ensemble_expected(ep, pending, LD)
        runs = []
        for on in (True, False):
            with _Launches(on):
                runs.append(api.ei_analytic_ensemble(gps, ep.points, ep.best, points_being_sampled=pending))
        ei, grad = runs[0]
        assert np.array_equal(ei, runs[1][0]) and np.array_equal(grad, runs[1][1])
        e_v = max(abs(ei[i] - float(w[0])) / w[2] for i, w in enumerate(want))
        e_g = max(float(np.max(np.abs(grad[i] - w[1].astype(np.float64)))) / max(1.0, float(np.max(np.abs(w[1])))) for i, w in enumerate(want))
        print("ensemble of 3, %d pending: value error %.3g scale, gradient error %.3g (bounds 1e-10)" % (len(pending), e_v, e_g))
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


# ---- 4. the ascent against the host-driven loop ----
MS = dict(starts=12, steps=6, restarts=2, gamma=0.7, pre_mult=1.0, max_rel=0.5)


def _ascent_problem(tolerance):
    ep = dr.make_ensemble()
    rng = np.random.default_rng(78)
    starts = rng.uniform(0.02, 0.98, size=(MS["starts"], ep.points.shape[1]))
    gd = (MS["starts"], MS["steps"], MS["restarts"], 0, MS["gamma"], MS["pre_mult"], MS["max_rel"], tolerance)
    bounds = np.array([[0.0, 1.0]] * ep.points.shape[1])
    return ep, starts, gd, bounds


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
    print("tolerance %g: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"] and want["value"] >= want["start_values"].max()
    _close(gps)


# ---- 5. greedy batches ----
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
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) >= 1e-3
    _close(gps)


# ---- 6. limits and errors ----
def test_sixty_four_rows_hold_twenty_one_points_of_three_rows():
    p = [c for c in dr.PROBLEMS if c.name == "n12_d2_g2_p21"][0]
    G = _gp(p)
    rng = np.random.default_rng(5)
    more = np.vstack([p.pending, rng.uniform(0.05, 0.95, size=(1, 2))])
    assert len(p.pending) == 21 and np.all(np.isfinite(api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=p.pending)[0]))
    gd = (6, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    starts, box = rng.uniform(0.05, 0.95, size=(6, 2)), [[0, 1], [0, 1]]
    for call in (lambda: api.ei_analytic_ensemble(G, p.points, [p.best], points_being_sampled=more),
                 lambda: api.ei_analytic_multistart(G, gd, box, [p.best], starts, points_being_sampled=more),
                 lambda: api.ei_analytic_suggest(G, gd, box, [p.best], starts, 22, gradient_ascent=False, points_being_sampled=more[:1]),
                 lambda: api.ei_analytic_suggest(G, gd, box, [p.best], starts, 2, gradient_ascent=False, points_being_sampled=more[:21])):
        with pytest.raises(api.BoundsException) as e:
            call()
        assert (e.value.value, e.value.min, e.value.max) == (22.0, 0.0, 21.0)
    # the same count through num_to_sample: 1 + 21 - 1 points are 63 rows
    got = api.ei_analytic_suggest(G, gd, box, [p.best], starts, 21, gradient_ascent=False, points_being_sampled=more[:1])
    assert got["points"].shape == (21, 2) and np.all(got["found"]) and np.all(np.isfinite(got["values"])) and np.all(got["values"] >= 0)
    G.close()


def test_members_with_different_derivative_lists_are_refused():
    p = dr.PROBLEMS[0]
    a = _gp(p)
    b = api.DeviceGP(p.hyper, p.X, p.y[:, :2], p.noise[:2], (0,), cov_type=p.cov_type)
    c = api.DeviceGP(p.hyper, p.X, p.y[:, :2], p.noise[:2], (1,), cov_type=p.cov_type)
    for gps, payload in (([a, b], (1.0, 2.0, 1.0)), ([b, a], (2.0, 1.0, 1.0)), ([b, c], (1.0, 1.0, 1.0))):
        with pytest.raises(api.InvalidValueException) as e:
            api.ei_analytic_ensemble(gps, p.points, [p.best] * 2)
        assert (e.value.value, e.value.truth, e.value.tolerance) == payload and "observed-derivative list" in str(e.value)
    ok = api.ei_analytic_ensemble([b, api.DeviceGP(p.hyper * 1.1, p.X, p.y[:, :2], p.noise[:2], (0,), cov_type=p.cov_type)], p.points,
                                  [p.best] * 2, want_grad=False)
    assert np.all(np.isfinite(ok))
    _close([a, b, c])


def test_a_pending_point_listed_twice_in_a_noise_free_member_is_singular():
    """tests/test_gpu_ei1.py's construction with both partial derivatives observed: alpha = 1e-3 and noise 0 in the second member, a
    pending point 0.05 from a sampled point listed twice; the second copy's first Schur pivot is a few ulp of alpha, far under the
    pivot rule's 1e-16.  An error return with payload (member, index of the pending POINT in the list), not a fault."""
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, size=(6, 2))
    f, grad = dr.smooth(X, 3)
    y = 0.1 * np.column_stack([f, grad])
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    gps = [api.DeviceGP(hyper, X, y, [1e-5, 2e-5, 3e-5], (0, 1)), api.DeviceGP(hyper, X, y, [0.0, 0.0, 0.0], (0, 1))]
    bests = [float(y[:, 0].min())] * 2
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


# ---- 7. the wrapper, on Branin with its gradient observed at 8 points ----
def test_the_wrapper_and_the_optimisation_run_end_to_end_on_branin_with_gradients():
    import wrappers_mirror as cw
    rng = np.random.default_rng(0)
    dim, num_mcmc = 2, 3
    X = rng.uniform(size=(8, dim))
    a, b = 15.0 * X[:, 0] - 5.0, 15.0 * X[:, 1]
    inner = b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0
    y = inner ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0
    dy = np.column_stack([15.0 * (2 * inner * (-2 * 5.1 / (4 * np.pi ** 2) * a + 5.0 / np.pi) - 10.0 * (1 - 1 / (8 * np.pi)) * np.sin(a)),
                          15.0 * 2 * inner])
    vals = np.column_stack([(y - y.mean()) / y.std(), dy / y.std()])
    noise = np.array([1e-4, 2e-4, 3e-4])
    hypers = np.array([[1.0, 0.3, 0.3], [1.4, 0.25, 0.4], [0.8, 0.45, 0.3]])
    hd = cw.HistoricalData(dim=dim, num_derivatives=2)
    hd.append_sample_points([cw.SamplePoint(X[i], vals[i], 1e-4) for i in range(X.shape[0])])
    gpm = cw.GaussianProcessMCMC(hypers, np.tile(noise, (num_mcmc, 1)), hd, [0, 1])
    models = gpm.member_models()
    ei = eia.AnalyticExpectedImprovementMCMC(models)
    assert ei.problem_size == dim and np.array_equal(ei.best_so_far, np.full(num_mcmc, vals[:, 0].min()))
    members = eia._device_members(models)
    cand = rng.uniform(size=(7, dim))
    want_v, want_g = api.ei_analytic_ensemble(members, cand, ei.best_so_far)
    direct = [api.DeviceGP(h, X, vals, noise, (0, 1)) for h in hypers]
    dv, dg = api.ei_analytic_ensemble(direct, cand, ei.best_so_far)
    assert np.array_equal(dv, want_v) and np.array_equal(dg, want_g)
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
    print("Branin with gradients, 8 points, 3 members: a batch of 3 at %s, values %s" % (np.round(points, 3).tolist(), [float(v) for v in values]))
    _close(direct)
