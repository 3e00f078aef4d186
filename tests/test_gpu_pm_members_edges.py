"""The dispatch branches of csrc/pm_members.hip that tests/test_gpu_pm_members.py does not reach, against tests/pm_members_reference.py
with that file's checks (_check_trace, _margins_ok, _check_screen) and bounds: the descent at padded dimensions 12, 16, 24 and 32 (the
scratch-carrying instantiations among them, one through a second restart), the screening at padded 16 and 24 and at n = 1 and n = 2,
and numpy.argmin's NaN rule for start_index.  The descent's inputs are pm_members_reference.edge_cases();
tests/test_pm_members_reference.py asserts their decision margins (>= 1e-7) on the CPU.  Every test prints the worst figures it saw
(pytest -s)."""
import numpy as np
import pytest

import pm_members_reference as pr
from cornell_moe_amd import api
from test_gpu_pm_members import MATERN, ONE_STEP, SE, _build, _check_screen, _check_trace, _margins_ok, _unit

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", pr.edge_cases(),
                         ids=lambda c: "seed%d-d%d-g%d-f%d-T%d-R%d-pre%g" % (c[0], c[2], len(c[5]), c[6], c[8][1], c[8][2], c[8][5]))
def test_descent_at_every_padded_dimension(case):
    seed, n, d, E, cov, derivs, nf, C_, gd = case
    members, a, bounds, cand = pr.case_problem(case)
    runs = _margins_ok(members, nf, gd, bounds, cand)
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=cov) for e in range(E)]
    res, seen = _check_trace(gps, members, nf, gd, bounds, cand, "seed %d d=%d T=%d R=%d" % (seed, d, gd[1], gd[2]))
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


# test_gpu_pm_members.SCREEN_CASES' layout: E, d, cov, derivs, num_fidelity, n, C, per-member candidate sets.  n = 1 observes
# derivatives: a single function value equals the constant mean, and every candidate would tie.
SCREEN_EDGES = [
    (3, 16, SE, (), 0, (20,), 65, False),
    (3, 24, MATERN, (), 1, (20,), 64, True),
    (2, 3, MATERN, (0, 2), 0, (1,), 9, False),
    (2, 3, SE, (), 0, (2,), 9, True),
    (2, 32, SE, (1, 31), 0, (1,), 9, True),
    (2, 32, MATERN, (), 0, (2,), 9, False),
]


@pytest.mark.parametrize("case", SCREEN_EDGES, ids=lambda c: "E%d-d%d-cov%d-g%d-f%d-n%d-C%d-pm%d" % (c[0], c[1], c[2], len(c[3]), c[4], c[5][0], c[6], c[7]))
def test_screening_at_padded_16_and_24_and_with_one_and_two_training_points(case):
    _check_screen(case)


KEYS = ("best_points", "best_values", "start_index", "fell_back", "means", "trace")


def _nan_inputs():
    gps, members, a = _build(57, 20, 3, 3, MATERN)
    cand = np.random.default_rng(58).uniform(0.05, 0.95, size=(300, 3))
    return gps, cand


def test_a_nan_in_a_shared_candidate_is_every_members_start():
    gps, cand = _nan_inputs()
    clean = api.minimize_member_means(gps, cand, pr.MAIN_INNER, _unit(3), want_means=True, want_trace=True)
    bad = cand.copy()
    bad[270, 1] = np.nan  # the second candidate of thread 14: pmm_argmin_kernel's thread meets a number first
    res = api.minimize_member_means(gps, bad, pr.MAIN_INNER, _unit(3), want_means=True, want_trace=True)
    others = np.arange(300) != 270
    for e in range(3):
        assert res["start_index"][e] == 270 == int(np.argmin(res["means"][e]))  # numpy's rule: a NaN below every number
        assert np.isnan(res["best_values"][e]) and np.isnan(res["best_points"][e, 1])
        assert np.array_equal(res["best_points"][e, [0, 2]], cand[270, [0, 2]])
        assert np.array_equal(res["means"][e, others], clean["means"][e, others]) and np.isnan(res["means"][e, 270])
        assert int(res["trace"][e, 0, 0, 3 + 1]) == 30 and int(res["trace"][e, 0, 0, 3 + 5]) == 2  # 30 halvings, ended without a move
    print("shared NaN candidate: start 270 for every member, 30 halvings, NaN value and coordinate returned")


def test_a_nan_in_one_members_own_set_leaves_the_other_members_bits():
    gps, cand = _nan_inputs()
    sets = np.stack([cand, cand[::-1], cand[:, ::-1]]).copy()
    clean = api.minimize_member_means(gps, sets, pr.MAIN_INNER, _unit(3), want_means=True, want_trace=True)
    bad = sets.copy()
    bad[1, 270, 2] = np.nan
    res = api.minimize_member_means(gps, bad, pr.MAIN_INNER, _unit(3), want_means=True, want_trace=True)
    assert res["start_index"][1] == 270 == int(np.argmin(res["means"][1]))
    assert np.isnan(res["best_values"][1]) and np.isnan(res["best_points"][1, 2]) and not res["fell_back"][1]
    for e in (0, 2):
        for key in KEYS:
            assert np.array_equal(res[key][e], clean[key][e]), (key, e)
        assert np.all(np.isfinite(res["best_points"][e])) and np.isfinite(res["best_values"][e])
    print("NaN in member 1's own set: start 270 there, members 0 and 2 bit-equal to the call without it")
