"""CPU tests of the checkers of the device recommendation (tests/recommend_reference.py) and of the new ABI: the literal
restatement of the reference's procedure and the extended-precision form agree; the reference's own, unmodified PosteriorMeanMCMC,
GradientDescentOptimizer, TensorProductDomain, RepeatedDomain and multistart_optimize, run over duck-typed GPs that answer from the
checker, return the literal restatement's path and end point (skipped where the reference tree or a package it imports is absent);
the library exports the new symbols and refuses bad arguments without a device."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

import recommend_reference as rr
import sampling_reference as sr
from cornell_moe_amd import _lib, build as moe_build

REF = "/root/reference"
SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5

# seed, n, d, E, cov_type, derivs, num_fidelity, candidates, num_starts, gd (T, averaged, gamma, pre_mult, max_relative_change)
CASES = [
    (1, 30, 3, 3, MATERN, (), 0, 40, 1, rr.GdParams(12, 4, 0.7, 0.05, 0.5)),
    (2, 25, 2, 2, SE, (), 0, 30, 3, rr.GdParams(8, -1, 0.0, 0.02, 1.0)),
    (3, 20, 3, 2, MATERN, (0, 2), 1, 25, 2, rr.GdParams(6, 0, 0.7, 0.05, 0.02)),
    (8, 24, 3, 4, SE, (1,), 0, 35, 1, rr.GdParams(4, 0, 0.7, 50.0, 1.0)),  # a large pre_mult: the descent ends worse, the screened candidate is kept
]


def _case(case, dtype):
    seed, n, d, E, cov_type, derivs, nf, C_, S, gd = case
    members, arrays = rr.make_ensemble(seed, n, d, E, cov_type, derivs, dtype=dtype)
    rng = np.random.default_rng(1000 + seed)
    size = d - nf
    bounds = np.array([[0.0, 1.0]] * size)
    cand = np.vstack([rng.uniform(0, 1, size=(C_ - n, size)), arrays["X"][:, :size]])
    return members, nf, gd, bounds, cand, S


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d" % c[0])
def test_literal_and_extended_agree(case):
    members, nf, gd, bounds, cand, S = _case(case, rr.LD)
    b = rr.extended(rr.Ensemble(members, nf), gd, bounds, cand, S)
    members64 = _case(case, np.float64)[0]
    a = rr.literal(members64, nf, gd, bounds, cand, S)
    print("margins %s refined %s" % (np.array(b.margins), b.refined))
    assert min(b.margins) >= 1e-7, "choose another seed: a decision of this case is closer than the checkers' own error"
    assert a.index == b.index and np.array_equal(a.starts, b.starts) and a.winner == b.winner and a.refined == b.refined
    want = b.values.astype(np.float64)
    assert np.all(np.abs(a.values - want) <= 1e-10 * np.maximum(1.0, np.abs(want)))
    # the gradient at every candidate, plain double against extended precision: the forward bound the device is held to
    g64 = rr.Ensemble(members64, nf).f(cand, True)[1]
    gld = rr.Ensemble(members, nf).f(cand, True)[1]
    scale = np.maximum(1.0, np.max(np.abs(gld), axis=1).astype(np.float64))
    assert np.all(np.abs(g64 - gld.astype(np.float64)) <= 1e-10 * scale[:, None])
    assert abs(a.value - float(b.value)) <= 1e-10 * max(1.0, abs(float(b.value)))


def test_both_branches_of_the_last_comparison_are_covered():
    got = set()
    for case in CASES:
        members, nf, gd, bounds, cand, S = _case(case, rr.LD)
        got.add(rr.extended(rr.Ensemble(members, nf), gd, bounds, cand, S).refined)
    assert got == {True, False}


def _import_reference():
    here = os.path.dirname(os.path.abspath(__file__))
    added = [p for p in (os.path.join(here, "shims"), REF) if p not in sys.path]
    sys.path[:0] = added
    return added


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "moe", "optimal_learning", "python", "cpp_wrappers")),
                    reason="the reference tree is not present")
def test_reference_classes_return_the_literal_path():
    """cpp_wrappers/knowledge_gradient_mcmc.py: PosteriorMeanMCMC and python_version's optimiser and domains, imported unchanged,
    with moe.build.GPP aliased to cornell_moe_amd.GPP and GPs whose device object answers from the checker."""
    pytest.importorskip("scipy.optimize")
    before = set(sys.modules)
    saved = {k: sys.modules.get(k) for k in ("moe", "moe.build", "moe.build.GPP")}
    added = _import_reference()
    try:
        import cornell_moe_amd.GPP as GPP
        import moe
        build = types.ModuleType("moe.build")
        build.GPP = GPP
        sys.modules["moe.build"] = build
        sys.modules["moe.build.GPP"] = GPP
        moe.build = build
        from moe.optimal_learning.python.cpp_wrappers.knowledge_gradient_mcmc import PosteriorMeanMCMC
        from moe.optimal_learning.python.geometry_utils import ClosedInterval
        from moe.optimal_learning.python.python_version.domain import TensorProductDomain
        from moe.optimal_learning.python.python_version.optimization import (GradientDescentOptimizer,
                                                                              GradientDescentParameters, multistart_optimize)
        from moe.optimal_learning.python.repeated_domain import RepeatedDomain

        class Dev(object):
            """what GPP.compute_posterior_mean / compute_grad_posterior_mean touch of api.DeviceGP"""

            def __init__(self, member):
                self.member = member

            def posterior_mean(self, point, num_fidelity=0, want_grad=True):
                d = self.member.X.shape[1]
                full = np.concatenate([np.asarray(point)[:d - num_fidelity], np.ones(num_fidelity)])[None, :]
                mu, g = self.member.mu_grad(full, want_grad)
                return -float(mu[0]), (-g[0, :d - num_fidelity] if want_grad else None)

        class Duck(object):
            def __init__(self, member):
                self.dim = member.X.shape[1]
                self._gaussian_process = types.SimpleNamespace(dim=self.dim, _dev=Dev(member))

        for case in CASES[:3]:
            members, nf, gd, bounds, cand, S = _case(case, np.float64)
            want = rr.literal(members, nf, gd, bounds, cand, 1)
            ps = PosteriorMeanMCMC([Duck(m) for m in members], nf)
            domain = RepeatedDomain(num_repeats=1, domain=TensorProductDomain([ClosedInterval(lo, hi) for lo, hi in bounds]))
            params = GradientDescentParameters(max_num_steps=gd.max_num_steps, max_num_restarts=1,
                                               num_steps_averaged=gd.num_steps_averaged, gamma=gd.gamma, pre_mult=gd.pre_mult,
                                               max_relative_change=gd.max_relative_change, tolerance=1.0e-10)
            opt = GradientDescentOptimizer(domain, ps, params)
            start = cand[want.index].reshape(1, -1)
            # the path: the optimiser's own loop, observed through the points it sets
            seen = []
            setter = PosteriorMeanMCMC.set_current_point

            def spy(self, pts, _seen=seen, _setter=setter):
                _seen.append(np.array(pts, dtype=np.float64).ravel())
                _setter(self, pts)

            PosteriorMeanMCMC.current_point = property(PosteriorMeanMCMC.get_current_point, spy)
            try:
                end = multistart_optimize(opt, start, num_multistarts=1)[0]
            finally:
                PosteriorMeanMCMC.current_point = property(PosteriorMeanMCMC.get_current_point, setter)
            # seen: the start (MultistartOptimizer), x_0 .. x_{T-1} (the steps), the end point
            path = np.array(seen[1:1 + gd.max_num_steps])
            assert np.max(np.abs(path - want.paths[0][:gd.max_num_steps])) <= 1e-12
            assert np.max(np.abs(np.ravel(end) - want.end_points[0])) <= 1e-12
            assert abs(ps.compute_objective_function() - want.end_values[0]) <= 1e-12
    finally:
        for p in added:
            sys.path.remove(p)
        for k in set(sys.modules) - before:
            if k == "moe" or k.startswith("moe.") or k in ("future", "future.utils", "past", "past.utils", "builtins_shim"):
                sys.modules.pop(k, None)
        for k, v in saved.items():
            if v is not None:
                sys.modules[k] = v


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_new_symbols_resolve(lib):
    for name in ("moe_posterior_mean_mcmc_batch", "moe_posterior_mean_mcmc_recommend"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def _gd(max_num_steps=5, domain_type=0):
    g = _lib.GdParams()
    g.num_multistarts, g.max_num_steps, g.max_num_restarts, g.num_steps_averaged = 1, max_num_steps, 1, 2
    g.gamma, g.pre_mult, g.max_relative_change, g.tolerance, g.domain_type = 0.7, 1.0, 0.5, 1e-10, domain_type
    return g


def test_bad_arguments_are_refused_without_a_device(lib):
    """the documented codes, in the documented order: everything that needs no handle is checked before a handle is touched"""
    dp = _lib.dp
    err = _lib.MoeError()
    buf = np.zeros(8)
    p = buf.ctypes.data_as(dp)
    none = (C.c_void_p * 1)(None)  # an ensemble of one NULL handle

    def batch(gps, E, nf, P):
        return lib.moe_posterior_mean_mcmc_batch(gps, E, nf, p, P, p, None, C.byref(err))

    def rec(gps, E, nf, gd, C_, S):
        return lib.moe_posterior_mean_mcmc_recommend(gps, E, nf, C.byref(gd), p, p, C_, S, p, None, None, None, None, None, None,
                                                     C.byref(err))

    assert batch(None, 1, 0, 1) == _lib.MOE_ERR_RUNTIME
    assert batch(none, 0, 0, 1) == _lib.MOE_ERR_BOUNDS
    assert batch(none, 1, 0, 0) == _lib.MOE_ERR_BOUNDS
    assert batch(none, 1, -1, 1) == _lib.MOE_ERR_BOUNDS
    assert batch(none, 1, 0, 1) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert rec(None, 1, 0, _gd(), 4, 1) == _lib.MOE_ERR_RUNTIME
    assert rec(none, 0, 0, _gd(), 4, 1) == _lib.MOE_ERR_BOUNDS
    assert rec(none, 1, 0, _gd(), 0, 1) == _lib.MOE_ERR_BOUNDS
    assert rec(none, 1, 0, _gd(), 4, 0) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 4.0)
    assert rec(none, 1, 0, _gd(), 4, 5) == _lib.MOE_ERR_BOUNDS
    assert rec(none, 1, 0, _gd(max_num_steps=0), 4, 1) == _lib.MOE_ERR_BOUNDS
    assert rec(none, 1, 0, _gd(domain_type=1), 4, 1) == _lib.MOE_ERR_BOUNDS and b"tensor-product" in err.message
    assert rec(none, 1, -1, _gd(), 4, 1) == _lib.MOE_ERR_BOUNDS
    assert rec(none, 1, 0, _gd(), 4, 1) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert lib.moe_posterior_mean_mcmc_recommend(none, 1, 0, None, p, p, 4, 1, p, None, None, None, None, None, None,
                                                 None) == _lib.MOE_ERR_RUNTIME


# ---- the inputs of tests/test_gpu_recommend_edges.py: every decision margin on the CPU ----
@pytest.mark.parametrize("case", rr.edge_cases(), ids=rr.edge_id)
def test_edge_case_margins(case):
    if case.kind == "ties":
        margins = rr.ties_problem(case)[5]
    elif case.kind == "nan":
        margins = rr.nan_problem(case, 0)[5] + rr.nan_problem(case, case.C - 1)[5]
    else:
        members, a, bounds, cand = rr.edge_problem(case)
        ens = rr.Ensemble(members, case.num_fidelity)
        want = rr.extended(ens, case.gd, bounds, cand, case.S)
        margins = list(want.margins)
        if case.kind == "descent":
            margins.append(rr.clamp_kinds(ens, case.gd, bounds, want.paths)[1])
    print("margins %s" % np.array(margins))
    assert min(margins) >= 1e-7, "choose another seed: a decision of this case is closer than the checkers' own error"


def test_edge_descents_cover_a_clamped_and_a_free_step_and_every_padded_dimension():
    kinds, padded, shapes = set(), set(), set()
    for case in rr.edge_cases():
        if case.kind != "descent":
            continue
        members, a, bounds, cand = rr.edge_problem(case)
        ens = rr.Ensemble(members, case.num_fidelity)
        kinds |= rr.clamp_kinds(ens, case.gd, bounds, rr.extended(ens, case.gd, bounds, cand, case.S).paths)[0]
        padded.add((case.d + 3) // 4 * 4 if case.d <= 16 else (case.d + 7) // 8 * 8)
        shapes.add((case.cov, len(case.derivs), case.num_fidelity))
        assert case.n == 20 and case.E in (3, 5) and case.S == 2 and case.gd[:2] == (6, 3)
    assert kinds == {True, False} and padded == {8, 16, 24, 32}
    assert {s[0] for s in shapes} == {SE, MATERN} and (MATERN, 2, 1) in shapes
