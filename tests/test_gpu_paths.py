"""Posterior function paths and their minimisers on the device (csrc/paths.hip: moe_gp_paths_evaluate, moe_gp_paths_minimize) against
tests/paths_reference.py, at the smallest shapes that reach every dispatch edge: d = 3, 6, 10, 13, 17, 32 (padded to 4, 8, 12, 16,
24, 32), n on both sides of the 256-thread stride, M = 64 .. 4096, S on both sides of the chunk of 8 and of 64 columns on the split-K
side of the set phase, one and three members, both covariances; rows behind the evaluator's row cache (n = 3600) and points behind
its first launch (C = 16384 + 3) in tests of their own.

Values and gradients are held to paths_reference.tolerance() = max(1e-10, 4 gap()) against the extended-precision form, relative to
max(1, |f|) (a gradient: to max(1, its largest component)).  A (path, point) value must carry the same bits whatever C, S, E and
want_grad share the call; the descent must start from the screened bits and follow, bit for bit, the literal host loop driven by
api.paths_evaluate.  Decisions must equal the extended-precision restatement's (tests/test_paths_reference.py asserts their margins
on the CPU); the descent is checked step by step along the device's own trace, |x_next - F_ext(x, i)| <= alpha_i tolerance()
max(1, |grad f|_inf) per coordinate, and end to end within 10 x paths_reference.end_gap() floored at 1e-12, as
tests/test_gpu_pm_members.py derives its own.  Every test prints the worst figures it saw (pytest -s)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import paths_reference as pp
import pm_members_reference as pr
from cornell_moe_amd import api, min_value_entropy, posterior_paths, random_features

pytestmark = pytest.mark.gpu

LD, SE, MATERN = pp.LD, pp.SE, pp.MATERN
MARGIN = 1e-7
_ids = lambda c: "seed%d-n%d-d%d-E%d-cov%d-M%d-S%d-C%d" % c[:8]  # noqa: E731


def _gps(a, cov):
    return [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], cov_type=cov) for e in range(len(a["hypers"]))]


def _tab(t, members=None, paths=None):
    w, z = t["weights"], t["noise_normals"]
    if members is not None:
        w, z = w[members], z[members]
    if paths is not None:
        w, z = w[:, paths], z[:, paths]
    return t["frequencies"], t["phases"], np.ascontiguousarray(w), np.ascontiguousarray(z)


@pytest.fixture(scope="module")
def problems():
    """every case's extended-precision members, built once and left unchanged"""
    return {case: pp.case_problem(case, LD) for case in pp.EVAL_CASES + pp.DESCENT_CASES}


@pytest.mark.parametrize("case", pp.EVAL_CASES, ids=_ids)
def test_values_and_gradients(case, problems):
    members, a, tab, bounds, pts = problems[case]
    E, S, C_ = case[3], case[6], case[7]
    gps = _gps(a, case[4])
    probe = a["X"][:3] + 0.01
    before = [g.mean(probe) for g in gps]
    values, grad = api.paths_evaluate(gps, *_tab(tab), pts, want_grad=True)
    tol, worst_v, worst_g = pp.tolerance(), 0.0, 0.0
    for e in range(E):
        want, wg = members[e].values(pts), members[e].grads(pts)
        worst_v = max(worst_v, float(np.max(np.abs(values[e] - want) / np.maximum(1.0, np.abs(want.astype(np.float64))))))
        worst_g = max(worst_g, float(np.max(np.abs(grad[e] - wg)) / max(1.0, float(np.max(np.abs(wg))))))
    print("value error %.3g, gradient error %.3g (bound %.3g)" % (worst_v, worst_g, tol))
    assert worst_v <= tol and worst_g <= tol
    # the bits of a (path, point) value: without the gradient, alone in its call, and among other points, paths and members
    plain = api.paths_evaluate(gps, *_tab(tab), pts)
    assert np.array_equal(plain, values)
    e, s, c = E // 2, S // 2, C_ // 2
    one = api.paths_evaluate([gps[e]], *_tab(tab, [e], [s]), pts[c:c + 1])
    assert one[0, 0, 0] == values[e, s, c]
    one_v, one_g = api.paths_evaluate([gps[e]], *_tab(tab, [e], [s]), pts[c:c + 1], want_grad=True)
    assert one_v[0, 0, 0] == values[e, s, c] and np.array_equal(one_g[0, 0, 0], grad[e, s, c])
    assert all(np.array_equal(u, g.mean(probe)) for u, g in zip(before, gps))  # the handles answer as before


def test_rows_behind_the_row_cache():
    """paths_reference.CACHE_CASE: n = 3600 rows, M = 4096 features (the largest LDS request), S = 9 paths in two chunks -- the second
    reads the cached rows back and recomputes rows 3584 .. 3599 -- at points beside sampled points behind the cache, where those rows
    add at least 1e-3 to every value (tests/test_paths_reference.py).  Against the float64 form within max(tolerance(), 4 CACHE_GAP);
    the cached kernel, the evaluation kernel that has no cache, a (path, point) alone and the minimiser's screening carry the same
    bits."""
    members, a, tab, bounds, pts, rows = pp.cache_problem(np.float64)
    S, C_ = pp.CACHE_CASE[6], pp.CACHE_CASE[7]
    gps = _gps(a, pp.CACHE_CASE[4])
    values, grad = api.paths_evaluate(gps, *_tab(tab), pts, want_grad=True)
    want, wg = members[0].values(pts), members[0].grads(pts)
    bound = max(pp.tolerance(), 4.0 * pp.CACHE_GAP)
    e_v = float(np.max(np.abs(values[0] - want) / np.maximum(1.0, np.abs(want))))
    e_g = float(np.max(np.abs(grad[0] - wg)) / max(1.0, float(np.max(np.abs(wg)))))
    tail = float(np.min(np.abs(pp.tail_rows(members[0], pts))))
    print("n = %d, M = %d, S = %d: value error %.3g, gradient error %.3g against float64 (bound %.3g); the rows behind the cache add at "
          "least %.3g" % (pp.CACHE_CASE[1], pp.CACHE_CASE[5], S, e_v, e_g, bound, tail))
    assert e_v <= bound and e_g <= bound
    plain = api.paths_evaluate(gps, *_tab(tab), pts)  # (the cached kernel against the evaluation that has no cache)
    assert np.array_equal(plain, values)
    for s, c in ((3, 1), (S - 1, C_ - 1)):  # a path of the first chunk, one of the second
        one = api.paths_evaluate(gps, *_tab(tab, [0], [s]), pts[c:c + 1])
        assert one[0, 0, 0] == values[0, s, c], (s, c)
        one_v, one_g = api.paths_evaluate(gps, *_tab(tab, [0], [s]), pts[c:c + 1], want_grad=True)
        assert one_v[0, 0, 0] == values[0, s, c] and np.array_equal(one_g[0, 0, 0], grad[0, s, c]), (s, c)
    res = api.paths_minimize(gps, *_tab(tab), pp.MAIN_INNER, bounds, pts, want_screened=True)
    assert np.array_equal(res["screened"], values)


def test_points_behind_the_first_launch():
    """paths_reference.PASS_CASE: C = 16384 + 3 points make a second launch of the point kernels, without and with the gradient.  The
    points on both sides of the boundary against long double at tolerance(), and bit for bit against themselves alone in a call."""
    case = pp.PASS_CASE
    members, a, tab, bounds, pts = pp.case_problem(case, LD)
    C_ = case[7]
    assert C_ == pp.PASS + 3 and len(pts) == C_
    checked = [0, pp.PASS - 1, pp.PASS, C_ - 1]
    gps = _gps(a, case[4])
    plain = api.paths_evaluate(gps, *_tab(tab), pts)
    values, grad = api.paths_evaluate(gps, *_tab(tab), pts, want_grad=True)
    assert np.array_equal(plain, values) and np.all(np.isfinite(values)) and np.all(np.isfinite(grad))
    want, wg = members[0].values(pts[checked]), members[0].grads(pts[checked])
    tol = pp.tolerance()
    e_v = float(np.max(np.abs(values[0][:, checked] - want) / np.maximum(1.0, np.abs(want.astype(np.float64)))))
    e_g = float(np.max(np.abs(grad[0][:, checked] - wg)) / max(1.0, float(np.max(np.abs(wg)))))
    print("C = %d: value error %.3g, gradient error %.3g at the points %s (bound %.3g)" % (C_, e_v, e_g, checked, tol))
    assert e_v <= tol and e_g <= tol
    for c in checked:
        one = api.paths_evaluate(gps, *_tab(tab), pts[c:c + 1])
        one_v, one_g = api.paths_evaluate(gps, *_tab(tab), pts[c:c + 1], want_grad=True)
        assert one[0, 0, 0] == values[0, 0, c] and one_v[0, 0, 0] == values[0, 0, c] and np.array_equal(one_g[0, 0, 0], grad[0, 0, c]), c
    # (no point was left at the output's initial zeros, and the points behind the boundary are not copies of those before it)
    assert np.all(values != 0.0) and not np.array_equal(values[0, 0, pp.PASS:], values[0, 0, :3])


_LAUNCH_PROBE = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import paths_reference as pp
from cornell_moe_amd import api
case = pp.PASS_CASE
members, a, tab, bounds, pts = pp.case_problem(case, np.float64)
gps = [api.DeviceGP(a["hypers"][0], a["X"], a["y"], a["noises"][0], cov_type=case[4])]
tables = (tab["frequencies"], tab["phases"], tab["weights"], tab["noise_normals"])
for C_ in (pp.PASS, pp.PASS + 3):
    for grad in (0, 1):
        sys.stderr.write("\nCALL %%d %%d\n" %% (C_, grad))
        sys.stderr.flush()
        api.paths_evaluate(gps, *tables, pts[:C_], want_grad=bool(grad))
"""


def test_the_point_kernels_take_16384_points_per_launch():
    """what test_points_behind_the_first_launch assumes of csrc/paths.hip, by the behaviour: a fresh process under the HIP runtime's
    launch log (AMD_LOG_LEVEL=3: a launch's grid, then the kernel's name) evaluates 16384 and 16384 + 3 points without and with the
    gradient; the point kernel and the gradient kernel go out once over 16384 points, then over 16384 and over 3"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, AMD_LOG_LEVEL="3")
    env.pop("AMD_LOG_MASK", None)
    env.pop("AMD_LOG_LEVEL_FILE", None)
    run = subprocess.run([sys.executable, "-c", _LAUNCH_PROBE % (root, os.path.join(root, "tests"))], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    launches, call, grid = {}, None, None
    for line in run.stderr.splitlines():
        m = re.match(r"CALL (\d+) (\d+)$", line)
        if m:
            call = (int(m.group(1)), int(m.group(2)))
            launches[call] = []
            continue
        m = re.search(r"hipLaunchKernel \( *\S+, *\{(\d+),(\d+),(\d+)\}", line)
        if m:
            grid = tuple(int(v) for v in m.groups())
            continue
        m = re.search(r"ShaderName : .*\b(paths_points_kernel|paths_grad_kernel)<", line)
        if m and call is not None:
            launches[call].append((m.group(1), grid))
    print("launches of the point kernels per call (points, want_grad): %s" % launches)
    assert pp.PASS == 16384
    for grad, name in ((0, "paths_points_kernel"), (1, "paths_grad_kernel")):
        assert launches[(pp.PASS, grad)] == [(name, (pp.PASS, 1, 1))]
        assert launches[(pp.PASS + 3, grad)] == [(name, (pp.PASS, 1, 1)), (name, (3, 1, 1))]


def test_feature_limit():
    """M = 4096 is accepted (EVAL_CASES' last case evaluates there), M = 4097 refused with its payload before anything runs"""
    members, a, tab, bounds, pts = pp.case_problem((6, 20, 3, 1, SE, 8, 1, 1), np.float64)
    gps = _gps(a, SE)
    t = pp.draw_tables(SE, 3, 20, 1, 4097, 1, 1)
    with pytest.raises(api.BoundsException) as ei:
        api.paths_evaluate(gps, *_tab(t), pts)
    print(ei.value)
    assert "num_features" in str(ei.value)


def test_mismatched_members_are_refused():
    _, a, tab, bounds, pts = pp.case_problem((2, 20, 3, 2, MATERN, 8, 1, 2), np.float64)
    g = _gps(a, MATERN)
    other_cov = api.DeviceGP(a["hypers"][1], a["X"], a["y"], a["noises"][1], cov_type=SE)
    other_x = api.DeviceGP(a["hypers"][1], a["X"] + 1e-3, a["y"], a["noises"][1], cov_type=MATERN)
    yd = np.hstack([a["y"], np.zeros((20, 1))])
    with_deriv = [api.DeviceGP(a["hypers"][e], a["X"], yd, np.r_[a["noises"][e], 1e-2], derivatives=[0], cov_type=MATERN)
                  for e in range(2)]
    for bad, word in (([g[0], other_cov], "cov_type"), ([g[0], other_x], "sampled points"), (with_deriv, "derivative")):
        with pytest.raises(api.InvalidValueException) as ei:
            api.paths_evaluate(bad, *_tab(tab), pts)
        assert word in str(ei.value)


def _check_descent(case, problems):
    members, a, tab, bounds, cand = problems[case]
    E, S, gd, d = case[3], case[6], case[8], case[2]
    gps = _gps(a, case[4])
    res = api.paths_minimize(gps, *_tab(tab), gd, bounds, cand, want_screened=True, want_trace=True)
    at = api.paths_evaluate(gps, *_tab(tab), cand)
    assert np.array_equal(res["screened"], at)  # the screening is paths_evaluate at the candidates
    tol, alpha0 = pp.tolerance(), pr.alpha_table(gd)
    bound_end = max(1e-12, 10.0 * pp.end_gap())
    worst_step, worst_end, worst_scr = 0.0, 0.0, 0.0
    for e in range(E):
        for s in range(S):
            obj = pp.PathObjective(members[e], s)
            want = pp.run(members[e], s, gd, bounds, cand)
            assert pr.min_margin(want) >= MARGIN
            worst_scr = max(worst_scr, float(np.max(np.abs(res["screened"][e, s] - want.means) /
                                                    np.maximum(1.0, np.abs(want.means.astype(np.float64))))))
            start = int(res["start_index"][e, s])
            assert start == want.start_index == int(np.argmin(res["screened"][e, s]))
            rows = res["trace"][e, s]
            assert rows[0, 0, d] == -res["screened"][e, s, start]  # the descent's first f0 is the screened value, bit for bit
            got, x = [], cand[start].copy()
            for r in range(rows.shape[0]):
                for i in range(rows.shape[1]):
                    row = rows[r, i]
                    state = int(row[d + 5])
                    if state == 0:
                        break
                    got.append((r, i, int(row[d + 1]), bool(row[d + 2]), bool(row[d + 3]), bool(row[d + 4]), state))
                    step = pr.one_step(obj, gd, bounds, x, i)  # F_ext from the device's own point
                    gscale = max(1.0, step.gnorm)
                    worst_step = max(worst_step, float(np.max(np.abs(row[:d] - step.x.astype(np.float64)))) / (alpha0[i] * gscale))
                    x = row[:d].copy()
            assert got == pr.decisions_of(want.steps), (e, s)
            assert not res["fell_back"][e, s] and not want.fell_back
            end = want.end.astype(np.float64)
            worst_end = max(worst_end, float(np.max(np.abs(res["best_points"][e, s] - end) / np.maximum(1.0, np.abs(end)))))
            assert abs(res["best_values"][e, s] - float(want.best_value)) <= tol * max(1.0, abs(float(want.best_value)))
            assert res["best_values"][e, s] <= res["screened"][e, s].min()
            assert np.all(res["best_points"][e, s] >= 0.0) and np.all(res["best_points"][e, s] <= 1.0)
    print("screened error %.3g (bound %.3g); worst step error / (alpha_i max(1, |g|)) %.3g (bound %.3g); end points %.3g "
          "(bound %.3g)" % (worst_scr, tol, worst_step, tol, worst_end, bound_end))
    assert worst_scr <= tol and worst_step <= tol and worst_end <= bound_end
    return gps, res


@pytest.mark.parametrize("case", pp.DESCENT_CASES, ids=_ids)
def test_minimisers_against_the_restatement(case, problems):
    _check_descent(case, problems)


def test_trace_equals_the_literal_host_loop(problems):
    """the whole trace, bit for bit, from posterior_mean_optimize's loop in plain double with api.paths_evaluate as its evaluator;
    and a path's outputs do not depend on the paths and members that share the call"""
    case = pp.DESCENT_CASES[0]
    members, a, tab, bounds, cand = problems[case]
    gd, d, S = case[8], case[2], case[6]
    gps = _gps(a, case[4])
    res = api.paths_minimize(gps, *_tab(tab), gd, bounds, cand, want_trace=True)
    for s in (0, S - 1):
        t1 = _tab(tab, [0], [s])

        def mean_fn(pt):
            return api.paths_evaluate(gps, *t1, pt[None])[0, 0, 0]

        def grad_fn(pt):
            return api.paths_evaluate(gps, *t1, pt[None], want_grad=True)[1][0, 0, 0]

        x0 = cand[int(res["start_index"][0, s])]
        x, fcur, decisions = pr.literal_float64(mean_fn, grad_fn, d, 0, gd, bounds, x0)
        rows = res["trace"][0, s].reshape(-1, d + api.TRACE_EXTRA)
        rows = rows[rows[:, d + 5] != 0]
        got = [(int(r[d + 1]), bool(r[d + 2]), bool(r[d + 3]), bool(r[d + 4]), int(r[d + 5])) for r in rows]
        assert got == [dec[2:] for dec in decisions]
        assert np.array_equal(x, res["best_points"][0, s]) and np.array_equal(rows[-1, :d], x)
        alone = api.paths_minimize(gps, *t1, gd, bounds, cand, want_trace=True)
        assert np.array_equal(alone["trace"][0, 0], res["trace"][0, s]) and alone["best_values"][0, 0] == res["best_values"][0, s]


def _models(seed=3, n=24, d=2, E=2, cov=MATERN):
    """members over noisy observations of a bowl with its minimum inside the domain and short length scales: the paths' minimisers
    lie in the interior (at a face the limiter's steps depend on the distance to it alone, and two paths can end on the same bits)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, size=(n, d))
    y = (8.0 * np.sum((X - 0.45) ** 2, axis=1) - 1.0 + 0.05 * rng.standard_normal(n))[:, None]
    a = dict(X=X, y=y, hypers=[np.r_[1.0 + 0.2 * e, np.full(d, 0.25 + 0.05 * e)] for e in range(E)], noises=[np.array([1e-2])] * E)
    return _gps(a, cov), a, np.array([[0.0, 1.0]] * d)


def test_thompson_sampling_batch():
    gps, a, bounds = _models()
    for q in (1, 5):
        points, values = posterior_paths.thompson_sampling_batch(gps, bounds, pp.LONG_INNER, q, num_candidates=200, num_features=256,
                                                                  seed=q)
        assert points.shape == (q, 2) and values.shape == (q,)
        assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values))
        assert len({tuple(p) for p in points}) == q
    again = posterior_paths.thompson_sampling_batch(gps, bounds, pp.LONG_INNER, 5, num_candidates=200, num_features=256, seed=5)
    assert np.array_equal(again[0], points) and np.array_equal(again[1], values)


def test_sample_from_global_optima():
    gps, a, bounds = _models(E=1, cov=SE)
    grid = api.latin_hypercube(1, bounds, 100)
    pts = random_features.sample_from_global_optima(gps[0], 128, bounds, grid, 4, seed=2)
    assert pts.shape == (4, 2) and np.all(pts >= 0.0) and np.all(pts <= 1.0)


def test_min_values_from_paths_feed_gibbon_and_lie_below_the_candidate_set():
    """with the same candidates in both, the minima of paths over the domain average below the minima of joint draws over the
    candidates alone: a one-sided sign check"""
    gps, a, bounds = _models()
    K = 64
    cand = api.latin_hypercube(5, bounds, 12)  # (a coarse set: what the descent gains over it is large beside the sampling error)
    mins = posterior_paths.sample_min_values_from_paths(gps, bounds, pp.LONG_INNER, K, num_features=512, seed=1, candidates=cand)
    assert mins.shape == (2, K) and np.all(np.isfinite(mins))
    value = api.gibbon_ensemble(gps, cand[:5], mins, want_grad=False)
    assert value.shape == (5,) and np.all(np.isfinite(value))
    obj = min_value_entropy.MinValueEntropyMCMC(gps, mins)
    assert np.array_equal(obj.evaluate_at_point_list(cand[:5]), value)
    on_set = min_value_entropy.sample_min_values(gps, cand, K, 1)
    print("mean min-value: paths %.4f, candidate set %.4f" % (mins.mean(), on_set.mean()))
    assert mins.mean() < on_set.mean()
