"""CPU tests (-m "not gpu") of tests/ei1_deriv_reference.py, the checker of tests/test_gpu_ei1_deriv.py: the inputs are qualified (a
case that breaks a condition FAILS: re-seed it), the restatement's gradient is checked against central differences, its p = 0 value
and gradient against the plain-C oracle and the reference's recorded figures on the six committed fixtures with derivative
observations, its conditioned variance against the oracle's GP built on X u P, and with g = 0 it is tests/ei1_reference.py to the
last bit."""
import math

import numpy as np
import pytest

import ei1_deriv_reference as dr
import ei1_reference as er
import kg1_reference as kr
from oracle import orc
from test_ei1_reference import padded_dim, wide_magnitudes

LD = dr.LD


@pytest.mark.parametrize("p", dr.PROBLEMS + dr.PROBLEMS_P0, ids=lambda p: p.name)
def test_the_inputs_are_well_conditioned(p):
    want, w64 = dr.expected(p, LD), dr.expected(p, np.float64)
    e_v = max(abs(float(want[i].value) - float(w64[i].value)) / want[i].scale for i in p.checked)
    e_g = max(float(np.max(np.abs(want[i].grad - w64[i].grad))) / max(1.0, float(np.max(np.abs(want[i].grad)))) for i in p.checked)
    sig = min(want[i].sigma for i in p.checked) / math.sqrt(p.hyper[0])
    no_p, value_only, no_dx = dr.expected_variants(p)
    moved = [max(abs(float(want[i].value - other[i])) / want[i].scale for i in p.checked) for other in (no_p, value_only, no_dx)]
    print("%s: %d + %d rows; float64 against long double %.3g scale in value, %.3g in gradient; min sigma / sqrt(alpha) %.3g; P moves EI "
          "by %.3g scale, P's derivative rows by %.3g, X's derivative observations by %.3g" % (
              p.name, p.y.size, len(p.pending) * p.y.shape[1], e_v, e_g, sig, moved[0], moved[1], moved[2]))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11
    assert sig >= 0.05  # (the gradient divides by sigma)
    assert moved[2] >= 1e-5  # (a device that dropped X's derivative rows fails a 1e-10 test)
    if len(p.pending):
        assert moved[0] >= 1e-5 and moved[1] >= 1e-5  # (... or ignored P, or took P's rows for function values alone)
    else:
        assert moved[0] == 0.0 and moved[1] == 0.0
    if p.name == dr.BPRIME:
        assert want[p.checked[0]].bprime < p.best - 1e-3 and p.best == float(p.y[:, 0].max())


@pytest.mark.parametrize("p", dr.WIDE_PROBLEMS + dr.WIDE_PROBLEMS_P0, ids=lambda p: p.name)
def test_the_wide_inputs_are_well_conditioned(p):
    test_the_inputs_are_well_conditioned(p)
    want = dr.expected(p, LD)
    wide_magnitudes(p.name, [(float(want[i].value) / want[i].scale, want[i].grad) for i in p.checked], p.X.shape[1])
    if len(p.X) >= 256:
        assert p.best == float(np.median(p.y[:, 0]))


def test_the_wide_cases_reach_every_path():
    names = [p.name for p in dr.WIDE_PROBLEMS + dr.WIDE_PROBLEMS_P0]
    assert len(set(names)) == len(names) and not set(names) & {p.name for p in dr.PROBLEMS + dr.PROBLEMS_P0}
    dims = {p.X.shape[1] for p in dr.WIDE_PROBLEMS}
    assert {16, 24} <= {padded_dim(d) for d in dims} and any(d % 4 for d in dims)  # (12 is dr.PROBLEMS' d = 12 case)
    assert {12, 16, 24} <= {padded_dim(p.X.shape[1]) for p in dr.PROBLEMS + dr.WIDE_PROBLEMS}
    big = [p for p in dr.WIDE_PROBLEMS if len(p.X) + len(p.pending) > 256]  # (a second trip of the loop over the points)
    assert big and all(len(p.derivs) >= 1 and 512 < p.y.size <= 1024 for p in big)  # (and tri_cols' K slice 128)
    for p in dr.WIDE_PROBLEMS:
        assert len(p.derivs) >= 1 and len(set(p.noise)) == len(p.noise) == 1 + len(p.derivs)
        assert 0 in p.checked and np.max(np.abs(p.pending[0] - p.points[0])) <= 0.05
    assert any(p.derivs[0] != 0 and p.X.shape[1] > 12 for p in dr.WIDE_PROBLEMS) and any(p.cov_type == dr.SE for p in dr.WIDE_PROBLEMS)
    for p in dr.WIDE_PROBLEMS_P0:
        assert len(p.pending) == 0


def test_the_cases_reach_every_path():
    names = [p.name for p in dr.PROBLEMS]
    assert len(set(names)) == len(names) == 9 and dr.BPRIME in names
    assert {p.X.shape[1] for p in dr.PROBLEMS} >= {2, 3, 4, 6, 12, 32}  # (DP = 4, 8, 12 and 32 gradient kernels)
    rows = [p.y.size for p in dr.PROBLEMS]
    assert min(rows) < 128 <= max(rows)
    assert max(len(p.pending) * p.y.shape[1] for p in dr.PROBLEMS) == 63  # (one row short of the limit: 21 points of 3 rows)
    assert any(p.cov_type == dr.SE for p in dr.PROBLEMS) and any(p.derivs == tuple(range(p.X.shape[1])) for p in dr.PROBLEMS)
    assert any(p.derivs and p.derivs[0] != 0 for p in dr.PROBLEMS)  # (a list that does not start at coordinate 0)
    for p in dr.PROBLEMS:
        assert len(p.derivs) >= 1 and len(set(p.noise)) == len(p.noise) == 1 + len(p.derivs)  # (distinct noise per kind)
        assert 0 in p.checked and np.max(np.abs(p.pending[0] - p.points[0])) <= 0.05
    for p in dr.PROBLEMS_P0:
        assert len(p.pending) == 0
    e = dr.ENSEMBLE
    g1 = 1 + len(e["derivs"])
    assert len(e["n"]) == 3 and min(e["n"]) * g1 < 128 <= max(e["n"]) * g1 and len(set(e["factors"])) == 3


def test_the_ensemble_is_well_conditioned():
    ep = dr.make_ensemble()
    want, w64 = dr.ensemble_expected(ep, ep.pending, LD), dr.ensemble_expected(ep, ep.pending, np.float64)
    without = dr.ensemble_expected(ep, ep.pending[:0], LD)
    e_v = max(abs(float(a[0]) - float(b[0])) / a[2] for a, b in zip(want, w64))
    e_g = max(float(np.max(np.abs(a[1] - b[1]))) / max(1.0, float(np.max(np.abs(a[1])))) for a, b in zip(want, w64))
    moved = max(abs(float(a[0] - b[0])) / a[2] for a, b in zip(want, without))
    print("ensemble of 3: float64 against long double %.3g / %.3g; P moves EI by %.3g scale" % (e_v, e_g, moved))
    assert e_v <= 2.5e-11 and e_g <= 2.5e-11 and moved >= 1e-5


@pytest.mark.parametrize("name", ["n5_d2_g2_p1", "n40_d4_D023_p5_se", "n20_d6_D05_p3", "n9_d12_g12_p2", dr.BPRIME, "n10_d20_D3_19_p2_se"])
def test_the_gradient_is_the_central_difference_of_the_value(name):
    p = [q for q in dr.PROBLEMS + dr.WIDE_PROBLEMS if q.name == name][0]
    base = dr.base_model(p, LD)
    model = dr.DerivPendingModel(base, p.pending)
    h, worst = 1e-6, 0.0
    for i in p.checked[:2]:
        grad = dr.evaluate_model(model, base, p.pending, p.points[i], p.best).grad
        for k in range(p.points.shape[1]):
            xp, xm = p.points[i].copy(), p.points[i].copy()
            xp[k] += h
            xm[k] -= h
            fd = (dr.evaluate_model(model, base, p.pending, xp, p.best).value -
                  dr.evaluate_model(model, base, p.pending, xm, p.best).value) / LD(xp[k] - xm[k])
            worst = max(worst, abs(float(fd - grad[k])) / max(1.0, float(np.max(np.abs(grad)))))
    print("%s: gradient against central differences of the long-double value: %.3g (bound 1e-7)" % (name, worst))
    assert worst <= 1e-7


def _derivative_fixtures(cases):
    return [c for c in cases if len(c.inp["derivs"])]


def test_without_pending_points_the_restatement_is_the_oracle_and_the_reference(golden):
    """the six fixture cases with derivative observations, tests/test_oracle.py's bounds: 1e-12 in value and 1e-10 in gradient,
    against the plain-C oracle point by point and against the reference's recorded figures"""
    cases, _ = golden
    seen = []
    for c in _derivative_fixtures(cases):
        i = c.inp
        derivs = [int(v) for v in i["derivs"]]
        seen.append(c.index)
        gp = orc.OrcGP(int(i["cov_type"]), float(i["alpha"]), i["lengths"], i["X"], i["y"], i["noise"], derivs)
        n = np.shape(i["X"])[0]
        base = dr.DerivModel(int(i["cov_type"]), np.concatenate([[float(i["alpha"])], i["lengths"]]), i["X"],
                             np.reshape(i["y"], (n, 1 + len(derivs))), i["noise"], derivs, LD)
        best = float(i["ei_best"])
        none = np.zeros((0, np.shape(i["X"])[1]))
        ref_ei, ref_grad = np.ravel(c.out["ei_analytic"]), np.reshape(c.out["grad_ei_analytic"], (-1, np.shape(i["X"])[1]))
        for k, pt in enumerate(np.reshape(i["query"], (-1, np.shape(i["X"])[1]))):
            v, g = gp.ei_analytic(pt, best)
            r = dr.evaluate(base, none, pt, best)
            assert abs(float(r.value) - v) <= 1e-12 * max(abs(v), 1e-6)
            assert np.abs(r.grad.astype(np.float64) - g).max() <= 1e-10 * max(np.abs(g).max(), 1e-6)
            assert abs(float(r.value) - ref_ei[k]) <= 1e-12 * max(abs(ref_ei[k]), 1e-6)
            assert np.abs(r.grad.astype(np.float64) - ref_grad[k]).max() <= 1e-10 * max(np.abs(ref_grad[k]).max(), 1e-6)
    print("fixture cases with derivative observations: %s" % seen)
    assert len(seen) == 6


@pytest.mark.parametrize("name", ["n5_d2_g2_p1", "n20_d3_D1_p2", "n40_d4_D023_p5_se", "n20_d6_D05_p3"])
def test_the_conditioned_variance_is_the_oracles_on_the_union(name):
    """the variance does not depend on the observed values (the oracle's prior mean does): the oracle's GP on X u P with values of
    any kind, every row of a pending point carrying the noise of its kind, has the conditioned variance; within 1e-10"""
    p = [q for q in dr.PROBLEMS if q.name == name][0]
    base = dr.base_model(p, LD)
    model = dr.DerivPendingModel(base, p.pending)
    XP = np.vstack([p.X, p.pending])
    any_y = np.random.default_rng(1).normal(size=(len(XP), 1 + len(p.derivs)))
    gp = orc.OrcGP(p.cov_type, float(p.hyper[0]), p.hyper[1:], XP, any_y, p.noise, list(p.derivs))
    g1 = 1 + len(p.derivs)
    worst = 0.0
    for i in p.checked:
        want = float(np.reshape(gp.var(p.points[i]), (g1, g1))[0, 0])
        worst = max(worst, abs(float(dr.conditioned_variance(model, p.points[i])) - want) / p.hyper[0])
    print("%s: conditioned variance against the oracle on X u P: %.3g alpha (bound 1e-10)" % (name, worst))
    assert worst <= 1e-10


@pytest.mark.parametrize("T", [LD, np.float64], ids=["longdouble", "float64"])
def test_without_derivatives_it_is_ei1_reference_to_the_last_bit(T):
    for p in er.PROBLEMS[:3] + [q for q in er.PROBLEMS if q.name in ("n20_d6_p3", er.BPRIME)]:
        plain = er.base_model(p, T)
        mine = dr.DerivModel(p.cov_type, p.hyper, p.X, p.y, p.noise, (), T)
        assert np.array_equal(plain.L, mine.L) and np.array_equal(plain.kinvy, mine.kinvy)
        for i in p.checked[:3]:
            a = er.evaluate(plain, p.pending, p.points[i], p.best)
            b = dr.evaluate(mine, p.pending, p.points[i], p.best)
            assert a.value == b.value and np.array_equal(a.grad, b.grad) and a.sigma == b.sigma and a.bprime == b.bprime, (p.name, i)
