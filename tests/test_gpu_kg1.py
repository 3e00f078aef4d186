"""The exact discretised one-point knowledge gradient on the device (csrc/kg1.hip: moe_gp_kg_discrete) against the long-double
restatement of tests/kg1_reference.py, on the cases kg1_reference.GPU_CASES (tests/test_kg1_reference.py holds the float64
restatement to the same cases on the CPU).  Shapes: d in {2, 3, 4, 6, 8, 12} with n up to 300 and A up to 4095 lines, and
d in {12, 14, 16, 17, 18, 24, 25, 32} at n = 20 / 24, A = 63 / 64 / 65 -- padded dimensions 12, 16, 24, 32, each of them with fidelity
coordinates (one or two) and without: every instantiation of the gradient kernel.

Tolerances: with scale = max(1, max |a|, sqrt(alpha)), |KG - want| <= 1e-10 scale (the bound tests/test_gpu_lcb.py uses for
continuous outputs) and |grad KG - want|_inf <= 1e-10 max(1, |want|_inf).  The number of lines on the envelope must be exact on every
case whose decision margins (kg1_reference.Result.margins) are >= 1e-7, which is asserted on the CPU first; at most 2 cases may fall
below and skip the count.  Every test prints the worst figures it saw (pytest -s).

Figures of the first run on an MI355X are recorded in DESIGN.md section 5.13."""
import numpy as np
import pytest

import kg1_reference as kr
from cornell_moe_amd import GPP, _lib, api, knowledge_gradient_discrete

pytestmark = pytest.mark.gpu

LD = kr.LD
MARGIN = 1e-7


def _gp(p):
    return api.DeviceGP(p.hyper, p.X, p.y, p.noise, cov_type=p.case.cov_type)


def test_at_most_two_cases_skip_the_count():
    below = [c.name for c in kr.GPU_CASES if min(min(w.margins) for w in kr.expected(c)[1].values()) < MARGIN]
    print("cases below the margin of %.0e: %s" % (MARGIN, below))
    assert len(below) <= 2, below


@pytest.mark.parametrize("case", kr.GPU_CASES, ids=lambda c: c.name)
def test_against_the_long_double_restatement(case):
    p, want = kr.expected(case)
    G = _gp(p)
    kg, grad, active = G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, want_active=True)
    assert kg.shape == (case.C,) and grad.shape == (case.C, case.d) and np.all(np.isfinite(kg)) and np.all(np.isfinite(grad))
    margin = min(min(want[i].margins) for i in p.checked)
    e_v = max(abs(kg[i] - float(want[i].value)) / want[i].scale for i in p.checked)
    e_g = max(float(np.max(np.abs(grad[i] - want[i].grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(want[i].grad))))
              for i in p.checked)
    print("%s: value error %.3g scale, gradient error %.3g (bounds 1e-10); lines on the envelope %s; smallest margin %.3g" % (
        case.name, e_v, e_g, sorted(set(int(active[i]) for i in p.checked)), margin))
    assert e_v <= 1e-10 and e_g <= 1e-10, (case.name, e_v, e_g)
    if margin >= MARGIN:
        assert [int(active[i]) for i in p.checked] == [want[i].num_active for i in p.checked]
    # the value alone: the same kernels, so the same bits; and a candidate alone carries the bits it has inside the batch
    assert np.array_equal(G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, want_grad=False), kg)
    for i in (p.checked if case.C > 7 else (0, case.C - 1)):
        k1, g1, a1 = G.kg_discrete(p.discrete, p.points[i:i + 1], p.best, num_fidelity=case.nf, want_active=True)
        assert k1[0] == kg[i] and np.array_equal(g1[0], grad[i]) and a1[0] == active[i], (case.name, i)
    G.close()


def test_the_straddled_pass_is_the_one_the_library_uses():
    case = kr.GPU_CASES[-1]
    per_pass = _lib.load().moe_kg1_pass_size(case.n, case.A)
    assert per_pass == 1024 and per_pass < case.C < 2 * per_pass
    assert set(kr.make_problem(case).checked) >= {per_pass - 1, per_pass}


@pytest.mark.parametrize("name", ["n5_d2_A255", "n20_d3_A63_fid", "n150_d6_A1000", "n24_d24_A65_fid2"])
def test_duplicates_a_permutation_and_the_candidate_itself_change_no_bit(name):
    case = [c for c in kr.GPU_CASES if c.name == name][0]
    p = kr.make_problem(case)
    G = _gp(p)
    pts = p.points[:min(case.C, 7)]
    kg, grad, active = G.kg_discrete(p.discrete, pts, p.best, num_fidelity=case.nf, want_active=True)
    rng = np.random.default_rng(5)
    size = case.d - case.nf
    dup = np.vstack([p.discrete[7:9], p.discrete, p.discrete[:3], p.discrete[-1:]])
    perm = p.discrete[rng.permutation(case.A)]
    for what, disc in (("duplicates", dup), ("permutation", perm)):
        k2, g2, a2 = G.kg_discrete(disc, pts, p.best, num_fidelity=case.nf, want_active=True)
        assert np.array_equal(k2, kg) and np.array_equal(a2, active), what
        assert np.max(np.abs(g2 - grad)) <= 1e-12 * max(1.0, np.max(np.abs(grad))), what
    for i in range(len(pts)):  # x^ of candidate i as a member of the set: its line is x^'s own, bit for bit, and drops out
        own = np.vstack([p.discrete[:5], pts[i:i + 1, :size], p.discrete[5:]])
        k3, g3, a3 = G.kg_discrete(own, pts[i:i + 1], p.best, num_fidelity=case.nf, want_active=True)
        assert k3[0] == kg[i] and a3[0] == active[i], i
        assert np.max(np.abs(g3[0] - grad[i])) <= 1e-12 * max(1.0, np.max(np.abs(grad))), i
    G.close()


def test_one_discrete_point_is_the_two_line_closed_form():
    case = kr.GPU_CASES[0]
    assert case.A == 1
    p, want = kr.expected(case)
    G = _gp(p)
    kg = G.kg_discrete(p.discrete, p.points, p.best, want_grad=False)
    worst = 0.0
    for i in p.checked:
        w = want[i]
        closed = min(LD(p.best), w.a[0]) - kr.two_line_emin(w.a[0], w.b[0], w.a[1], w.b[1])
        worst = max(worst, abs(kg[i] - float(closed)) / w.scale)
    print("two lines: device vs closed form %.3g scale" % worst)
    assert worst <= 1e-10
    G.close()


@pytest.mark.parametrize("name", ["n20_d3_A63_fid", "n70_d4_A64_se", "n24_d24_A65_fid2", "n20_d32_A63_fid"])
def test_best_so_far_on_either_side_of_the_mean(name):
    """KG + E[min] = min(best, mu_n(x^)): moving best across mu_n(x^) moves KG by exactly what the minimum moves, and the gradient
    gains or loses grad mu_n(x^) (zero on the fidelity coordinates)."""
    case = [c for c in kr.GPU_CASES if c.name == name][0]
    p = kr.make_problem(case)
    dset = kr.DiscreteSet(kr.Model(case.cov_type, p.hyper, p.X, p.y, p.noise, LD), p.discrete, case.nf)
    G = _gp(p)
    worst = 0.0
    for i in range(3):
        x = p.points[i:i + 1]
        lo, hi = kr.evaluate(dset, x[0], -50.0), kr.evaluate(dset, x[0], 50.0)
        mu, scale = float(lo.a[0]), lo.scale
        k_lo, g_lo = G.kg_discrete(p.discrete, x, mu - 0.25, num_fidelity=case.nf)
        k_hi, g_hi = G.kg_discrete(p.discrete, x, mu + 0.25, num_fidelity=case.nf)
        emin = float(lo.emin)
        assert abs(k_lo[0] + emin - (mu - 0.25)) <= 1e-10 * scale and abs(k_hi[0] + emin - mu) <= 1e-10 * scale
        grad_mu = (hi.grad - lo.grad).astype(np.float64)
        assert np.all(grad_mu[case.d - case.nf:] == 0.0)
        worst = max(worst, float(np.max(np.abs((g_hi[0] - g_lo[0]) - grad_mu))) / max(1.0, float(np.max(np.abs(grad_mu)))))
    print("%s: gradient gained across the mean vs grad mu_n %.3g" % (name, worst))
    assert worst <= 1e-10
    G.close()


def test_errors():
    case = kr.GPU_CASES[0]
    p = kr.make_problem(case)
    G = _gp(p)
    with pytest.raises(api.BoundsException) as e:
        G.kg_discrete(np.zeros((4096, 2)), p.points, p.best)
    assert (e.value.value, e.value.min, e.value.max) == (4096.0, 1.0, 4095.0)
    with pytest.raises(api.BoundsException) as e:
        G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.d)
    assert "num_fidelity" in str(e.value) and (e.value.value, e.value.max) == (float(case.d), float(case.d - 1))
    kg = G.kg_discrete(p.discrete, p.points, p.best, want_grad=False)  # (the handle still answers)
    assert np.all(np.isfinite(kg))
    G.close()
    Gd = api.DeviceGP(p.hyper, p.X, np.hstack([p.y, np.zeros((case.n, 1))]), [1e-2, 1e-2], [0], cov_type=case.cov_type)
    with pytest.raises(api.BoundsException) as e:
        Gd.kg_discrete(p.discrete, p.points, p.best)
    assert "not a minimum of lines" in str(e.value) and (e.value.value, e.value.min, e.value.max) == (1.0, 0.0, 0.0)
    Gd.close()


def test_a_noiseless_sampled_point_is_singular():
    """alpha = 1 and the FIRST sampled point: its column of the factor is (1, 0, ..., 0), so Sigma_n(x, x) is zero to a few 1e-17
    and s^2 fails the pivot rule s^2 > 1e-16 -- an argument check, reported with the candidate's index"""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), rng.normal(size=(6, 1))
    G = api.DeviceGP([1.0, 0.5, 0.5], X, y, [0.0])
    pts = np.vstack([rng.uniform(0, 1, size=(2, 2)), X[:1], rng.uniform(0, 1, size=(1, 2))])
    with pytest.raises(api.SingularMatrixException) as e:
        G.kg_discrete(rng.uniform(0, 1, size=(10, 2)), pts, float(y.min()))
    assert (e.value.num_rows, e.value.leading_minor_index) == (1, 2)
    G.close()


def test_the_ensemble_average_is_the_mean_of_the_members():
    case = kr.GPU_CASES[1]
    p = kr.make_problem(case)
    rng = np.random.default_rng(9)
    gps = [api.DeviceGP(p.hyper * f, p.X, p.y, [case.noise * f], cov_type=case.cov_type) for f in (1.0, 1.3, 0.8)]
    sets = [rng.uniform(0, 1, size=(A, case.d - case.nf)) for A in (63, 40, 100)]
    bests = [p.best, p.best + 0.2, p.best - 0.1]
    kg, grad = api.kg_discrete_mcmc(gps, sets, p.points, bests, num_fidelity=case.nf)
    single = [g.kg_discrete(s, p.points, b, num_fidelity=case.nf) for g, s, b in zip(gps, sets, bests)]
    assert np.array_equal(kg, ((single[0][0] + single[1][0]) + single[2][0]) / 3)
    assert np.array_equal(grad, ((single[0][1] + single[1][1]) + single[2][1]) / 3)
    assert np.array_equal(api.kg_discrete_mcmc(gps, sets, p.points, bests, num_fidelity=case.nf, want_grad=False), kg)
    for g in gps:
        g.close()


def test_the_wrapper_and_ten_steps_of_gradient_ascent():
    case = kr.GPU_CASES[5]
    p = kr.make_problem(case)
    hyper = [p.hyper[0], list(p.hyper[1:])]
    gp = GPP.GaussianProcess(hyper, p.X.ravel(), p.y.ravel(), p.noise, [], 0, case.d, case.n)
    kgd = knowledge_gradient_discrete.DiscreteKnowledgeGradient(gp, p.discrete)
    assert kgd.best_so_far == float(p.y.min()) and kgd.problem_size == case.d
    G = _gp(p)
    kg, grad = G.kg_discrete(p.discrete, p.points, p.best)
    assert np.array_equal(kgd.evaluate_at_point_list(p.points), kg)
    x = p.points[0].copy()
    kgd.set_current_point(x)
    assert kgd.compute_knowledge_gradient() == kg[0] and kgd.compute_objective_function() == kg[0]
    assert np.array_equal(kgd.compute_grad_knowledge_gradient(), grad[:1]) and np.array_equal(kgd.compute_grad_objective_function(), grad[:1])
    values = [kg[0]]
    for _ in range(10):
        g = kgd.compute_grad_objective_function()[0]
        x = np.clip(x + 0.02 * g / max(1e-12, float(np.max(np.abs(g)))), 0.0, 1.0)
        kgd.set_current_point(x)
        values.append(kgd.compute_objective_function())
        assert np.all(x >= 0.0) and np.all(x <= 1.0) and np.isfinite(values[-1])
    print("ten ascent steps: KG %.6g -> %.6g" % (values[0], values[-1]))
    assert max(values[1:]) > values[0]  # (a step of 0.02 along the gradient's sign pattern finds something better on the way)
    G.close()
