"""Every member's posterior-mean minimiser on the device (csrc/pm_members.hip: moe_posterior_mean_members_minimize) against
tests/pm_members_reference.py, at the smallest shapes that reach each branch.

Screened means are held to the forward bound of the sampling, LCB and recommendation tests against the extended-precision form,
|mu - want| <= 1e-10 max(1, |want|); indices and decisions must be equal exactly wherever the checker's margin of the decision is
>= 1e-7, and every case first asserts on the CPU that the margins of its own trajectory are.  The descent is checked step by step
along the device's own trace, |x_next - F_ext(x, i)| <= alpha_i 1e-10 max(1, |grad mu|_inf) per coordinate (alpha_i the step's
first trial length), so that no trajectory sensitivity enters; end to end the points are held to 10 x pm_members_reference.gap()
(floored at 1e-12) against the extended-precision run and to 1e-8 against DeviceGP.posterior_mean_optimize member by member.
No case falls back: tests/test_pm_members_reference.py::test_the_line_search_cannot_end_worse_than_its_start says why none can.
Every test prints the worst figures it saw (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import pm_members_reference as pr
import recommend_reference as rr
import sampling_reference as sr
from cornell_moe_amd import api, discretisation

pytestmark = pytest.mark.gpu

SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
LD = rr.LD
MARGIN = 1e-7
PASS = 16384   # candidates per launch (include/moe_hip.h: moe_posterior_mean_members_minimize)
STRIDE = 256   # training points a thread strides by in csrc/pm_members.hip's pmm_eval
ONE_STEP = (1, 1, 1, 0, 0.0, 1.0e-3, 1.0, 1.0e-10)


def _build(seed, n, d, E, cov, derivs=()):
    members, a = rr.make_ensemble(seed, n, d, E, cov, derivs)
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=cov) for e in range(E)]
    return gps, members, a


def _unit(size):
    return np.array([[0.0, 1.0]] * size)


# E, d, cov, derivs, num_fidelity, n, C, per-member candidate sets
SCREEN_CASES = [
    (3, 3, MATERN, (), 0, (STRIDE - 1, STRIDE, STRIDE + 1, 2 * STRIDE), 65, False),
    (3, 3, SE, (), 1, (40,), 1025, False),
    (1, 1, SE, (), 0, (30,), 63, False),
    (3, 1, MATERN, (), 0, (30,), 64, True),
    (17, 3, MATERN, (0, 2), 0, (20,), 63, True),
    (3, 3, SE, (0, 2), 1, (20,), 1, False),
    (3, 9, SE, (0, 2), 1, (30,), 64, False),
    (1, 9, MATERN, (0, 2), 0, (30,), 65, True),
    (1, 32, MATERN, (), 0, (33,), 5, False),
    (3, 32, SE, (), 1, (20,), 65, True),
]


@pytest.mark.parametrize("case", SCREEN_CASES, ids=lambda c: "E%d-d%d-cov%d-g%d-f%d-C%d-pm%d" % (c[0], c[1], c[2], len(c[3]), c[4], c[6], c[7]))
def test_screened_means_and_start_index(case):
    _check_screen(case)


def _check_screen(case):
    E, d, cov, derivs, nf, ns, C_, per_member = case
    size = d - nf
    for n in ns:
        gps, members, a = _build(100 * E + d + n, n, d, E, cov, derivs)
        rng = np.random.default_rng(n + C_)
        cand = rng.uniform(0, 1, size=(E, C_, size)) if per_member else rng.uniform(0, 1, size=(C_, size))
        probe = a["X"][:3] + 0.01
        before = [g.mean(probe) for g in gps]
        res = api.minimize_member_means(gps, cand, ONE_STEP, _unit(size), num_fidelity=nf, want_means=True)
        worst, gap = 0.0, np.inf
        for e in range(E):
            ce = cand[e] if per_member else cand
            want = pr.Objective(members[e], nf).mu(ce)
            worst = max(worst, float(np.max(np.abs(res["means"][e] - want) / np.maximum(1.0, np.abs(want.astype(np.float64))))))
            order = np.sort(want)
            if C_ > 1:
                gap = min(gap, float(order[1] - order[0]))
                assert order[1] - order[0] >= MARGIN, "choose another seed: two candidates are closer than the checker's error"
            assert res["start_index"][e] == int(np.argmin(want))
        print("E=%d d=%d n=%d C=%d: mean error %.3g (bound 1e-10), smallest argmin gap %.3g" % (E, d, n, C_, worst, gap))
        assert worst <= 1e-10
        # a (member, candidate) pair alone carries the bits it has in the batch
        e, c = E // 2, C_ // 2
        one = api.minimize_member_means([gps[e]], (cand[e] if per_member else cand)[c:c + 1], ONE_STEP, _unit(size), num_fidelity=nf,
                                        want_means=True)
        assert one["means"][0, 0] == res["means"][e, c]
        # ... and the bits of the GP's own posterior-mean query: mean_kernel makes the same evaluation in the same order
        point = np.concatenate([(cand[e] if per_member else cand)[c], np.ones(nf)])
        assert res["means"][e, c] == gps[e].mean(point[None])[0]
        assert all(np.array_equal(u, g.mean(probe)) for u, g in zip(before, gps))  # the handles answer as before


def test_across_a_pass_boundary():
    gps, members, a = _build(5, 10, 1, 1, MATERN)
    obj = pr.Objective(members[0])
    rng = np.random.default_rng(6)
    draws = rng.uniform(0, 1, size=(3 * (PASS + 1), 1))
    mu = obj.mu(draws)
    best = int(np.argmin(mu))
    others = draws[np.asarray(mu > mu[best] + 1e-3)][:PASS]  # the minimiser stands 1e-3 clear of every other candidate ...
    assert len(others) == PASS
    cand = np.vstack([others, draws[best:best + 1]])         # ... and is the one candidate of the second pass
    res = api.minimize_member_means(gps, cand, ONE_STEP, _unit(1), want_means=True)
    want = obj.mu(cand)
    err = float(np.max(np.abs(res["means"][0] - want) / np.maximum(1.0, np.abs(want.astype(np.float64)))))
    order = np.sort(want)
    print("C=%d: mean error %.3g, argmin gap %.3g" % (PASS + 1, err, float(order[1] - order[0])))
    assert err <= 1e-10 and order[1] - order[0] >= MARGIN
    assert res["start_index"][0] == int(np.argmin(want)) == PASS
    tail = api.minimize_member_means(gps, cand[PASS - 1:], ONE_STEP, _unit(1), want_means=True)
    assert np.array_equal(tail["means"][0], res["means"][0, PASS - 1:]) and tail["start_index"][0] == 1


def test_duplicated_candidates_resolve_to_the_first_index():
    gps, members, a = _build(3, 30, 3, 2, SE)
    rng = np.random.default_rng(9)
    cand = rng.uniform(0, 1, size=(300, 3))
    best = [int(np.argmin(pr.Objective(m).mu(cand))) for m in members]
    cand = np.vstack([cand, cand[best[0]:best[0] + 1], cand[best[1]:best[1] + 1]])  # each minimiser again, a workgroup's worth later
    res = api.minimize_member_means(gps, cand, ONE_STEP, _unit(3), want_means=True)
    for e in range(2):
        v = res["means"][e]
        assert v[best[e]] == v[300 + e] == v.min() and res["start_index"][e] == best[e]


def _check_trace(gps, members, nf, gd, bounds, cand, what, per_member=False):
    """the device's trace, step by step against F_ext from the device's own points; returns (result, decisions per member)"""
    res = api.minimize_member_means(gps, cand, gd, bounds, num_fidelity=nf, want_means=True, want_trace=True)
    size = bounds.shape[0]
    worst, seen, unchecked = 0.0, [], 0
    for e, member in enumerate(members):
        obj = pr.Objective(member, nf)
        ce = cand[e] if per_member else cand
        x = ce[res["start_index"][e]].copy()
        rows = res["trace"][e]  # [R][T][size + 6]
        mine = []
        ended = False
        for r in range(rows.shape[0]):
            x_begin = x.copy()
            for i in range(rows.shape[1]):
                row = rows[r, i]
                state = int(row[size + 5])
                if state == 0:
                    break
                assert not ended, (what, e, r, i, "a step after the optimisation ended")
                want = pr.one_step(obj, gd, bounds, x, i)
                got = (int(row[size + 1]), bool(row[size + 2]), bool(row[size + 3]), bool(row[size + 4]), state)
                if pr.min_margin(want.margins) >= MARGIN:
                    assert got == (want.halvings, want.changed, want.rejected, want.stop_norm, want.state), (what, e, r, i, got, want)
                else:
                    unchecked += 1  # (a decision of the device's own path closer than the checker's error: not compared)
                bound = want.alpha0 * 1e-10 * max(1.0, want.gnorm)  # every recorded step, whatever its margins
                err = float(np.max(np.abs(row[:size] - want.x)))
                worst = max(worst, err / bound)
                assert err <= bound, (what, e, r, i, err, bound)
                assert abs(row[size] - float(want.f0)) <= 1e-10 * max(1.0, abs(float(want.f0)))
                mine.append((r, i) + got)
                x = row[:size].copy()
                if state != 1 or got[3]:
                    break
            moved = float(np.sqrt(np.sum((x_begin - x) ** 2)))
            if not moved > gd[7]:
                ended = True
        assert np.all(x >= bounds[:, 0]) and np.all(x <= bounds[:, 1])
        if not res["fell_back"][e]:
            assert np.array_equal(res["best_points"][e], x), (what, e)  # the last traced point is the end point
        seen.append(mine)
    print("%s: worst step error / bound %.3g; decisions not compared for their margin: %d" % (what, worst, unchecked))
    assert unchecked == 0, "choose another seed: a decision on the device's own path is closer than the checker's error"
    return res, seen


def _margins_ok(members, nf, gd, bounds, cand, per_member=False):
    runs = [pr.run(m, nf, gd, bounds, cand[e] if per_member else cand) for e, m in enumerate(members)]
    low = min(pr.min_margin(r) for r in runs)
    print("smallest margin of the extended-precision trajectories %.3g" % low)
    assert low >= MARGIN, "choose another seed: a decision of this case is closer than the checkers' own error"
    return runs


@pytest.mark.parametrize("case", pr.gpu_cases(), ids=lambda c: "seed%d-d%d-g%d-f%d-T%d-R%d" % (c[0], c[2], len(c[5]), c[6], c[8][1], c[8][2]))
def test_descent_step_by_step_and_end_to_end(case):
    seed, n, d, E, cov, derivs, nf, C_, gd = case
    members, a, bounds, cand = pr.case_problem(case)
    runs = _margins_ok(members, nf, gd, bounds, cand)
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=cov) for e in range(E)]
    res, seen = _check_trace(gps, members, nf, gd, bounds, cand, "seed %d d=%d" % (seed, d))
    tol = max(10.0 * pr.gap(), 1e-12)
    for e, want in enumerate(runs):
        assert res["start_index"][e] == want.start_index and bool(res["fell_back"][e]) == want.fell_back
        assert seen[e] == pr.decisions_of(want.steps)
        x = want.best_point.astype(np.float64)
        err = float(np.max(np.abs(res["best_points"][e] - want.best_point) / np.maximum(1.0, np.abs(x))))
        host, hval = gps[e].posterior_mean_optimize(gd, bounds, cand[want.start_index], num_fidelity=nf)
        herr = float(np.max(np.abs(res["best_points"][e] - host) / np.maximum(1.0, np.abs(host))))
        verr = abs(res["best_values"][e] - float(want.best_value)) / max(1.0, abs(float(want.best_value)))
        print("member %d: end point against extended precision %.3g (bound %.3g), against the host loop %.3g (1e-8), value %.3g "
              "(1e-10)" % (e, err, tol, herr, verr))
        assert err <= tol and herr <= 1e-8 and verr <= 1e-10
        assert res["best_values"][e] <= res["means"][e, want.start_index]


def test_main_inner_parameters_cover_a_clamped_and_a_free_step():
    kinds = set()
    for case in pr.gpu_cases():
        members, a, bounds, cand = pr.case_problem(case)
        for m in members:
            kinds |= {s.changed for _, _, s in pr.run(m, case[6], case[8], bounds, cand).steps}
    assert kinds == {True, False}


def _near_a_face(seed):
    """two coordinates, the candidates 0.002 from a face of the first: with max_relative_change = 1 the limiter halves a step that
    would leave the domain, and the halved step can end below f0"""
    members, a = rr.make_ensemble(seed, 20, 2, 1, MATERN, ())
    rng = np.random.default_rng(900 + seed)
    cand = rng.uniform(0.0, 1.0, size=(6, 2))
    cand[:, 0] = np.where(rng.uniform(size=6) < 0.5, 0.002, 0.998)
    gps = [api.DeviceGP(a["hypers"][0], a["X"], a["y"], a["noises"][0], a["derivs"], cov_type=MATERN)]
    return gps, members, cand


@pytest.mark.parametrize("seed", [98, 123])
def test_a_step_rejected_after_the_limiter(seed):
    gps, members, cand = _near_a_face(seed)
    gd = (1, 4, 1, 3, 0.0, 1.0, 1.0, 1.0e-10)
    runs = _margins_ok(members, 0, gd, _unit(2), cand)
    assert any(s.state == 3 and s.changed for _, _, s in runs[0].steps)
    res, seen = _check_trace(gps, members, 0, gd, _unit(2), cand, "rejected, seed %d" % seed)
    assert seen[0] == pr.decisions_of(runs[0].steps) and seen[0][-1][-1] == 3


def test_stop_by_step_norm_second_restart_and_one_step():
    gps, members, a = _build(41, 30, 3, 2, MATERN)
    rng = np.random.default_rng(41)
    cand = rng.uniform(0.1, 0.9, size=(20, 3))
    # tolerance 1: the first accepted step is shorter than tolerance / max_num_steps, and the restart moved less than tolerance
    gd = (1, 4, 3, 3, 0.0, 1.0, 0.1, 1.0)
    runs = _margins_ok(members, 0, gd, _unit(3), cand)
    res, seen = _check_trace(gps, members, 0, gd, _unit(3), cand, "stop by norm")
    for e in range(2):
        assert seen[e] == pr.decisions_of(runs[e].steps) and len(seen[e]) == 1 and seen[e][0][5] is True
    # two restarts that both move
    gd = (1, 3, 2, 3, 0.0, 1.0, 0.2, 1.0e-9)
    runs = _margins_ok(members, 0, gd, _unit(3), cand)
    res, seen = _check_trace(gps, members, 0, gd, _unit(3), cand, "two restarts")
    for e in range(2):
        assert seen[e] == pr.decisions_of(runs[e].steps) and {r for r, *_ in seen[e]} == {0, 1}
    # max_num_steps = 1
    gd = (1, 1, 1, 3, 0.0, 1.0, 0.1, 1.0e-10)
    runs = _margins_ok(members, 0, gd, _unit(3), cand)
    res, seen = _check_trace(gps, members, 0, gd, _unit(3), cand, "one step")
    for e in range(2):
        assert seen[e] == pr.decisions_of(runs[e].steps) and len(seen[e]) == 1
        assert np.max(np.abs(res["best_points"][e] - runs[e].best_point)) <= 1e-12


def test_a_member_does_not_depend_on_the_others():
    E, k = 17, 11
    gps, members, a = _build(77, 40, 3, E, MATERN, (1,))
    rng = np.random.default_rng(78)
    cand = np.vstack([rng.uniform(0.05, 0.95, size=(30, 3)), a["X"]])
    gd = pr.MAIN_INNER
    probe = a["X"][:3] + 0.01
    before = [g.mean(probe) for g in gps]
    full = api.minimize_member_means(gps, cand, gd, _unit(3), want_means=True, want_trace=True)
    one = api.minimize_member_means([gps[k]], cand, gd, _unit(3), want_means=True, want_trace=True)
    for key in ("best_points", "best_values", "start_index", "fell_back", "means", "trace"):
        assert np.array_equal(one[key][0], full[key][k]), key
    per = api.minimize_member_means(gps, np.repeat(cand[None], E, axis=0), gd, _unit(3), want_means=True, want_trace=True)
    for key in ("best_points", "best_values", "start_index", "fell_back", "means", "trace"):
        assert np.array_equal(per[key], full[key]), key
    assert all(np.array_equal(u, g.mean(probe)) for u, g in zip(before, gps))


def test_mismatched_members_and_a_simplex_domain_are_refused():
    gps, members, a = _build(1, 12, 3, 2, MATERN)
    other = api.DeviceGP(a["hypers"][0], a["X"][:11], a["y"][:11], a["noises"][0], cov_type=MATERN)
    moved = api.DeviceGP(a["hypers"][0], a["X"] + 1e-3, a["y"], a["noises"][0], cov_type=MATERN)
    cand = np.full((2, 3), 0.5)
    for bad in (other, moved):
        with pytest.raises(api.InvalidValueException):
            api.minimize_member_means([gps[0], bad], cand, pr.MAIN_INNER, _unit(3))
    with pytest.raises(api.BoundsException) as info:
        api.minimize_member_means(gps, cand, pr.MAIN_INNER + (1,), _unit(3))
    assert "tensor-product" in str(info.value)
    with pytest.raises(api.BoundsException):
        api.minimize_member_means(gps, cand, pr.MAIN_INNER, _unit(3), num_fidelity=3)
    err = api._lib.MoeError()
    arr = (C.c_void_p * 2)(*[g._h.value for g in gps])
    out = np.zeros(8)
    p = out.ctypes.data_as(api.dp)
    g = api.DeviceGP._gd(pr.MAIN_INNER)
    assert api._lib.load().moe_posterior_mean_members_minimize(arr, 2, 3, C.byref(g), p, p, 1, 0, p, None, None, None, None, None,
                                                               C.byref(err)) == api._lib.MOE_ERR_BOUNDS
    assert tuple(err.payload) == (3.0, 0.0, 2.0)


def test_kg_discrete_points():
    E, nf = 3, 1
    gps, members, a = _build(31, 20, 3, E, MATERN)
    rng = np.random.default_rng(3)
    cand = rng.uniform(0, 1, size=(50, 2))
    shared = rng.uniform(0, 1, size=(7, 2))
    res = api.minimize_member_means(gps, cand, pr.MAIN_INNER, _unit(2), num_fidelity=nf)
    lists = discretisation.kg_discrete_points(gps, shared, cand, _unit(2), pr.MAIN_INNER, num_fidelity=nf)
    assert len(lists) == E
    for e in range(E):
        assert lists[e].shape == (8, 2) and np.array_equal(lists[e][:7], shared) and np.array_equal(lists[e][7], res["best_points"][e])
    same = discretisation.member_posterior_mean_minima(gps, cand, _unit(2), pr.MAIN_INNER, num_fidelity=nf)
    assert np.array_equal(same["best_points"], res["best_points"])
