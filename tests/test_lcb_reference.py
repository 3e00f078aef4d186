"""CPU tests of the checkers of batch LCB selection (tests/lcb_reference.py) and of the new ABI: the literal restatement of the
reference's procedure and the extended-precision form agree; the reference's own, unmodified lower_confidence_bound_optimization
run over a duck-typed GP returns the same points (skipped where the reference tree is absent); the library exports the new symbols
and refuses bad arguments without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import lcb_reference as lr
import sampling_reference as sr
from cornell_moe_amd import _lib, build as moe_build

REF = "/root/reference"
SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5


def _problem(seed, n, d, cov_type, noise, C_, length=0.4, alpha=1.3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, d))
    y = rng.normal(size=(n, 1))
    hyper = np.array([alpha] + [length] * d)
    return hyper, X, y, np.array([noise]), rng.uniform(0, 1, size=(C_, d))


@pytest.mark.parametrize("seed,n,d,cov_type,noise,C_,q", [(1, 40, 3, MATERN, 1e-2, 60, 4), (2, 50, 2, SE, 1e-3, 45, 5),
                                                         (3, 33, 2, MATERN, 1e-4, 30, 6)])
def test_literal_and_extended_agree(seed, n, d, cov_type, noise, C_, q):
    hyper, X, y, nz, cand = _problem(seed, n, d, cov_type, noise, C_)
    a = lr.literal(lr.OrcLike(cov_type, hyper, X, y, nz), cand, q)
    b = lr.extended(sr.Posterior(cov_type, hyper, X, y, nz), nz, cand, q)
    print("margins literal %s extended %s kept %d" % (np.array(a.margins), np.array(b.margins), b.kept))
    assert min(b.margins) >= 1e-7, "choose another seed: a decision of this case is closer than the checkers' own error"
    assert np.array_equal(a.index, b.index) and a.kept == b.kept
    # the plain-double restatement against extended precision: the forward bound the device is held to
    assert np.all(np.abs(a.mean - b.mean) <= 1e-10 * np.maximum(1.0, np.abs(b.mean)))
    assert np.all(np.abs(a.var - b.var) <= 1e-10 * max(1.0, hyper[0]))
    assert np.allclose(a.margins, b.margins, rtol=0, atol=1e-8)


def test_small_kept_set_picks_a_point_twice():
    """the reference's own behaviour when fewer candidates are kept than asked for: argmax runs over the kept set again"""
    hyper, X, y, nz, cand = _problem(7, 25, 2, MATERN, 1e-4, 20, length=0.15)
    b = lr.extended(sr.Posterior(MATERN, hyper, X, y, nz), nz, cand, 5)
    a = lr.literal(lr.OrcLike(MATERN, hyper, X, y, nz), cand, 5)
    assert np.array_equal(a.index, b.index)
    if b.kept < 5:
        assert len(set(b.index.tolist())) <= b.kept


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "moe", "optimal_learning", "python", "cpp_wrappers")),
                    reason="the reference tree is not present")
def test_reference_function_returns_the_same_points():
    """moe/optimal_learning/python/cpp_wrappers/lower_confidence_bound.py, imported unchanged, over a GP that answers from OrcGP."""
    here = os.path.dirname(os.path.abspath(__file__))
    added = [p for p in (os.path.join(here, "shims"), REF) if p not in sys.path]
    before = set(sys.modules)
    sys.path[:0] = added
    try:
        from moe.optimal_learning.python.cpp_wrappers import lower_confidence_bound as ref_lcb

        class Duck(object):
            """what the function touches of the wrapper-class GP"""

            def __init__(self, like, g):
                self.like, self.num_derivatives, self.added = like, g, []
                self.dim = like.args[2].shape[1]

            def compute_mean_of_points(self, pts):
                return np.array(self.like.mean(pts))

            def compute_cholesky_variance_of_points(self, pts):
                m = pts.shape[0] * (1 + self.num_derivatives)
                return np.reshape(self.like.chol_var(pts), (m, m)).T

            def add_sampled_points(self, sampled_points):
                for sp in sampled_points:
                    assert np.all(np.asarray(sp.value) == 0.0) and sp.noise_variance == 0.25
                    self.added.append(np.array(sp.point))
                    self.like = self.like.with_point(sp.point)

        for seed, cov_type, derivs, q in ((1, MATERN, (), 4), (4, SE, (0, 2), 3)):
            rng = np.random.default_rng(seed)
            n, d, g = 30, 3, len(derivs)
            X, y = rng.uniform(0, 1, size=(n, d)), rng.normal(size=(n, 1 + g))
            hyper, nz = np.array([1.3, 0.4, 0.5, 0.6]), np.full(1 + g, 1e-2)
            cand = rng.uniform(0, 1, size=(40, d))
            duck = Duck(lr.OrcLike(cov_type, hyper, X, y, nz, derivs), g)
            results, zero = ref_lcb.lower_confidence_bound_optimization(duck, cand, q)
            want = lr.literal(lr.OrcLike(cov_type, hyper, X, y, nz, derivs), cand, q)
            assert zero == 0.0 and np.array_equal(results, cand[want.index])
            # what the reference leaves behind: its first q - 1 picks, appended to the GP it was given
            assert np.array_equal(np.array(duck.added), cand[want.index[:-1]])
    finally:
        for p in added:
            sys.path.remove(p)
        for k in set(sys.modules) - before:
            if k == "moe" or k.startswith("moe.") or k in ("future", "future.utils", "past", "past.utils", "builtins_shim"):
                sys.modules.pop(k, None)


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_new_symbols_resolve_and_refuse_without_a_handle(lib):
    for name in ("moe_gp_mean_std", "moe_gp_lcb_select", "moe_lcb_pass_size"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    err = _lib.MoeError()
    out = np.zeros(4)
    idx = np.zeros(4, dtype=np.int32)
    dp, ip = _lib.dp, _lib.ip
    assert lib.moe_gp_mean_std(None, out.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), out.ctypes.data_as(dp),
                               C.byref(err)) == _lib.MOE_ERR_RUNTIME
    assert b"NULL GP handle" in err.message
    assert lib.moe_gp_lcb_select(None, out.ctypes.data_as(dp), 1, 1, idx.ctypes.data_as(ip), None, None, None, None,
                                 C.byref(err)) == _lib.MOE_ERR_RUNTIME
    assert lib.moe_gp_lcb_select(None, None, 0, 0, None, None, None, None, None, None) == _lib.MOE_ERR_RUNTIME


def test_pass_size_is_a_function_of_the_row_count(lib):
    """candidates per pass: 2^26 doubles of K* at most, a multiple of 1024 between 1024 and 16 384, whatever the candidate count"""
    for N, want in ((30, 16384), (127, 16384), (4096, 16384), (8000, 8192), (26000, 2048), (100000, 1024)):
        for C_ in (1, 17, 100000):
            assert lib.moe_lcb_pass_size(N, C_) == want, (N, C_)
