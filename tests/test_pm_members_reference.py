"""CPU tests of the checker of the members' posterior-mean minimisation (tests/pm_members_reference.py) and of the new ABI.

The extended-precision restatement is held (1) to the unmodified reference: RefGP.kg with a zero normal table runs the reference's
own ComputeOptimalPosteriorMean on a fantasy GP whose mean is the GP's mean up to rounding, over the discretised set
[Xq ; discrete] -- its end point must be the restatement's (before the fall-back) to 1e-8 max(1, |x|), the project's end-point
tolerance (skipped where oracle/_ref is not built); (2) to a line-for-line float64 copy of the library's host loop
(posterior_mean_optimize) over the plain-C oracle's additional_mean / grad_additional_mean: equal decisions, points within 1e-10.
Every case first asserts that all its decision margins are >= 1e-7 (seeds chosen so).  The library exports the new symbol, the
header declares it, bad arguments are refused without a device, and the Python layers exist."""
import ctypes as C
import os

import numpy as np
import pytest

import pm_members_reference as pr
import recommend_reference as rr
import sampling_reference as sr
from cornell_moe_amd import _lib, build as moe_build
from oracle import orc, ref

SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
MARGIN = 1e-7
FREE = (1, 6, 1, 3, 0.0, 1.0, 1.0, 1.0e-10)   # max_relative_change 1: steps the limiter leaves alone, then one it halves at a face
# LONG_INNER converges within its 2 x 40 steps, and a converged search compares quantities that differ by less than 1e-7: at d = 2
# none of the seeds 0 .. 199 keeps every margin, so that shape runs 2 x 20 steps (the margin stays); at d = 8 seed 80 does.
LONG_20 = pr.LONG_INNER[:1] + (20,) + pr.LONG_INNER[2:]

# seed, n, d, derivs, num_fidelity, gd, points in `discrete`, q
REF_CASES = [
    (0, 20, 2, (), 0, pr.MAIN_INNER, 12, 2),
    (0, 20, 2, (), 0, LONG_20, 12, 2),
    (0, 16, 3, (0, 2), 0, pr.MAIN_INNER, 10, 1),
    (0, 16, 3, (0, 2), 1, pr.MAIN_INNER, 10, 2),
    (0, 30, 8, (), 0, pr.MAIN_INNER, 15, 2),
    (80, 30, 8, (), 1, pr.LONG_INNER, 15, 1),
    (6, 20, 2, (), 0, FREE, 12, 2),
]


def _problem(case, dtype):
    seed, n, d, derivs, nf, gd, P, q = case
    members, a = rr.make_ensemble(seed, n, d, 1, MATERN, derivs, dtype=dtype)
    rng = np.random.default_rng(500 + seed)
    size = d - nf
    discrete = rng.uniform(0.05, 0.95, size=(P, size))
    Xq = rng.uniform(0.1, 0.9, size=(q, d))
    if nf:
        Xq[:, size:] = 1.0
    cand = np.vstack([Xq[:, :size], discrete])
    return members[0], a, np.array([[0.0, 1.0]] * size), discrete, Xq, cand


def _descent(member, nf, gd, bounds, cand):
    res = pr.run(member, nf, gd, bounds, cand)
    worst = sorted(res.margins, key=lambda m: m[1])[:2]
    print("start %d, %d steps, smallest margins %s" % (res.start_index, len(res.steps), worst))
    assert pr.min_margin(res) >= MARGIN, "choose another seed: a decision of this case is closer than the checkers' own error"
    return res


_ids = lambda c: "seed%d-d%d-g%d-f%d-T%d-mrc%g" % (c[0], c[2], len(c[3]), c[4], c[5][1], c[5][6])  # noqa: E731


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built (the reference tree is absent)")
@pytest.mark.parametrize("case", REF_CASES, ids=_ids)
def test_reference_optimal_posterior_mean_is_the_restatement(case):
    seed, n, d, derivs, nf, gd, P, q = case
    member, a, bounds, discrete, Xq, cand = _problem(case, rr.LD)
    res = _descent(member, nf, gd, bounds, cand)
    G = ref.RefGP(MATERN, a["hypers"][0][0], a["hypers"][0][1:], a["X"], a["y"], a["noises"][0], derivs)
    m = q * (1 + len(derivs))
    best_so_far = float(np.min(res.means))
    out = G.kg(list(gd), bounds, discrete, Xq, None, 2, best_so_far, np.zeros(m), want_grad=False, num_fidelity=nf)
    got = out["best_point"][0][:d - nf]
    want = res.end.astype(np.float64)
    err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print("reference end point against the restatement: %.3g (bound 1e-8)" % err)
    assert err <= 1e-8


def test_the_reference_cases_cover_both_limiter_branches_and_a_restart():
    changed, restarts = set(), set()
    for case in REF_CASES:
        member, a, bounds, discrete, Xq, cand = _problem(case, rr.LD)
        res = pr.run(member, case[4], case[5], bounds, cand)
        changed |= {s.changed for _, _, s in res.steps}
        restarts |= {r for r, _, _ in res.steps}
    assert changed == {True, False} and 1 in restarts


@pytest.mark.parametrize("case", REF_CASES, ids=_ids)
def test_literal_float64_host_loop_takes_the_same_decisions(case):
    seed, n, d, derivs, nf, gd, P, q = case
    member, a, bounds, discrete, Xq, cand = _problem(case, rr.LD)
    res = _descent(member, nf, gd, bounds, cand)
    O = orc.OrcGP(MATERN, a["hypers"][0][0], a["hypers"][0][1:], a["X"], a["y"], a["noises"][0], derivs)
    x, fcur, decisions = pr.literal_float64(lambda pt: O.additional_mean(pt[None, :])[0],
                                            lambda pt: O.grad_additional_mean(pt[None, :]), d, nf, gd, bounds, cand[res.start_index])
    assert decisions == pr.decisions_of(res.steps)
    err = float(np.max(np.abs(x - res.end)))
    print("literal float64 end point against extended precision: %.3g (bound 1e-10)" % err)
    assert err <= 1e-10
    assert abs(-fcur - float(res.mu_end)) <= 1e-10 * max(1.0, abs(float(res.mu_end)))
    # the float64 twin of the checker's own algebra
    twin = pr.run(_problem(case, np.float64)[0], nf, gd, bounds, cand)
    assert twin.start_index == res.start_index and pr.decisions_of(twin.steps) == pr.decisions_of(res.steps)
    assert twin.fell_back == res.fell_back and float(np.max(np.abs(twin.end - res.end))) <= 1e-10


def test_gap_between_the_arithmetics_over_the_gpu_cases():
    """what plain double loses end to end on the GPU tests' cases: the device is held to 10 x this, floored at 1e-12"""
    for case in pr.gpu_cases():
        members, a, bounds, cand = pr.case_problem(case)
        for member in members:
            assert pr.min_margin(pr.run(member, case[6], case[8], bounds, cand)) >= MARGIN
    g = pr.gap()
    print("gap %.3g" % g)
    assert 0.0 < g <= 1e-11


@pytest.mark.parametrize("pre_mult", [1.0, 50.0, 1.0e4])
def test_the_line_search_cannot_end_worse_than_its_start(pre_mult):
    """Why no case here falls back: a step is taken only after f_trial - f0 > alpha |g|^2 / 2 >= 0 and, where the limiter changed
    it, after f(x + step) > f0, so f = -mu rises with every accepted step whatever pre_mult -- a large pre_mult buys halvings, not an
    overshoot.  mu(end) > mu(start) needs a rounding error as large as the whole improvement; main.py's fall-back is dead code over
    this optimiser, kept by the library because the reference keeps it."""
    case = (3, 24, 3, (), 0, (1, 6, 2, 3, 0.0, pre_mult, 1.0, 1.0e-10), 20, 2)
    member, a, bounds, discrete, Xq, cand = _problem(case, rr.LD)
    res = pr.run(member, 0, case[5], bounds, cand)
    f = [-float(res.mu_start)] + [s.f0 for _, _, s in res.steps[1:]] + [-float(res.mu_end)]
    accepted = [s.state == 1 for _, _, s in res.steps]
    print("pre_mult %g: halvings %s, f along the path %s" % (pre_mult, [s.halvings for _, _, s in res.steps], f))
    assert any(accepted) and not res.fell_back
    assert all(float(f[k + 1]) > float(f[k]) for k in range(len(res.steps)) if accepted[k])


# ---- the ABI (fails on a library without the entry point) ----
@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_new_symbol_resolves_and_is_declared(lib):
    name = "moe_posterior_mean_members_minimize"
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moe_hip.h")
    with open(header) as fh:
        assert ("int %s(" % name) in fh.read()


def _gd(max_num_steps=5, max_num_restarts=1, domain_type=0):
    g = _lib.GdParams()
    g.num_multistarts, g.max_num_steps, g.max_num_restarts, g.num_steps_averaged = 1, max_num_steps, max_num_restarts, 2
    g.gamma, g.pre_mult, g.max_relative_change, g.tolerance, g.domain_type = 0.0, 1.0, 0.1, 1e-10, domain_type
    return g


def test_bad_arguments_are_refused_without_a_device(lib):
    """the documented codes, in the documented order: everything that needs no handle is checked before a handle is touched"""
    dp = _lib.dp
    err = _lib.MoeError()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(dp)
    none = (C.c_void_p * 1)(None)  # an ensemble of one NULL handle

    def call(gps, E, nf, gd, C_, per_member=0):
        return lib.moe_posterior_mean_members_minimize(gps, E, nf, C.byref(gd), p, p, C_, per_member, p, None, None, None, None, None,
                                                       C.byref(err))

    assert call(None, 1, 0, _gd(), 4) == _lib.MOE_ERR_RUNTIME
    assert call(none, 0, 0, _gd(), 4) == _lib.MOE_ERR_BOUNDS and tuple(err.payload)[:2] == (0.0, 1.0)
    assert call(none, 1, 0, _gd(), 0) == _lib.MOE_ERR_BOUNDS and tuple(err.payload)[:2] == (0.0, 1.0)
    assert call(none, 1, -1, _gd(), 4) == _lib.MOE_ERR_BOUNDS and tuple(err.payload)[:2] == (-1.0, 0.0)
    assert call(none, 1, 0, _gd(max_num_steps=0), 4) == _lib.MOE_ERR_BOUNDS and b"max_num_steps" in err.message
    assert call(none, 1, 0, _gd(max_num_restarts=0), 4) == _lib.MOE_ERR_BOUNDS and b"max_num_restarts" in err.message
    assert call(none, 1, 0, _gd(domain_type=1), 4) == _lib.MOE_ERR_BOUNDS and b"tensor-product" in err.message
    assert tuple(err.payload) == (1.0, 0.0, 0.0)
    assert call(none, 1, 0, _gd(), 4) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert call(none, 1, 0, _gd(), 4, 1) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert lib.moe_posterior_mean_members_minimize(none, 1, 0, None, p, p, 4, 0, p, None, None, None, None, None,
                                                   None) == _lib.MOE_ERR_RUNTIME
    assert lib.moe_posterior_mean_members_minimize(none, 1, 0, C.byref(_gd()), p, p, 4, 0, None, None, None, None, None, None,
                                                   C.byref(err)) == _lib.MOE_ERR_RUNTIME


def test_python_layers_exist():
    from cornell_moe_amd import api, discretisation
    assert callable(api.minimize_member_means) and callable(discretisation.kg_discrete_points)
    assert callable(discretisation.member_posterior_mean_minima)


# ---- the inputs of tests/test_gpu_pm_members_edges.py: every decision margin on the CPU ----
_edge_ids = lambda c: "seed%d-d%d-g%d-f%d-T%d-R%d-pre%g" % (c[0], c[2], len(c[5]), c[6], c[8][1], c[8][2], c[8][5])  # noqa: E731


@pytest.mark.parametrize("case", pr.edge_cases(), ids=_edge_ids)
def test_edge_case_margins(case):
    members, a, bounds, cand = pr.case_problem(case)
    for member in members:
        res = pr.run(member, case[6], case[8], bounds, cand)
        print("start %d, %d steps, smallest margins %s" % (res.start_index, len(res.steps), sorted(res.margins, key=lambda m: m[1])[:2]))
        assert pr.min_margin(res) >= MARGIN, "choose another seed: a decision of this case is closer than the checkers' own error"
        assert not res.fell_back


def test_edge_descents_cover_clamped_free_halved_steps_and_a_second_restart_that_moves():
    changed, halvings, restarts, padded = set(), 0, set(), set()
    for case in pr.edge_cases():
        members, a, bounds, cand = pr.case_problem(case)
        d = case[2]
        padded.add((d + 3) // 4 * 4 if d <= 16 else (d + 7) // 8 * 8)
        for member in members:
            for r, i, s in pr.run(member, case[6], case[8], bounds, cand).steps:
                changed.add(s.changed)
                halvings = max(halvings, s.halvings)
                if s.state == 1 and s.moved:
                    restarts.add(r)
    assert changed == {True, False} and halvings > 0 and 1 in restarts and padded == {12, 16, 24, 32}
    assert any(len(c[5]) == 2 and c[6] == 1 and c[2] > 16 for c in pr.edge_cases())
    assert any(c[2] == 32 and c[8][1:3] == (12, 2) for c in pr.edge_cases())
