"""CPU tests of the ensemble forms of the discretised one-point knowledge gradient (csrc/kg1_opt.hip: moe_kg_discrete_mcmc,
moe_kg_discrete_mcmc_multistart): the symbols, the refusals that need no device in their documented order, and the qualification
of the inputs of tests/test_gpu_kg1_opt.py -- the float64 restatement of the optimiser (tests/ms_restatement.py over
tests/kg1_reference.py, tests/kg1_opt_cases.py) must take every branch on them that the device code has."""
import ctypes as C
import os

import numpy as np
import pytest

import kg1_opt_cases as kc
import kg1_reference as kr
from cornell_moe_amd import _lib, build as moe_build

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moe_hip.h")


@pytest.fixture(scope="module")
def lib():
    moe_build.build()
    return _lib.load()


def test_the_header_declares_both_symbols_and_the_library_has_them(lib):
    with open(HEADER) as f:
        text = f.read()
    for name in ("moe_kg_discrete_mcmc", "moe_kg_discrete_mcmc_multistart"):
        assert ("int %s(" % name) in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "It has NO counterpart in the reference" in text


def _gd(steps=4, restarts=1, domain_type=0):
    g = _lib.GdParams()
    g.num_multistarts, g.max_num_steps, g.max_num_restarts, g.num_steps_averaged = 4, steps, restarts, 0
    g.gamma, g.pre_mult, g.max_relative_change, g.tolerance, g.domain_type = 0.7, 1.0, 0.5, 1e-10, domain_type
    return g


def test_the_evaluator_refuses_bad_arguments_without_a_device(lib):
    """in the order include/moe_hip.h documents; no handle exists without a device, so the handles are NULL and are looked at last"""
    dp, ip = _lib.dp, _lib.ip
    err = _lib.MoeError()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(dp)
    gps = (C.c_void_p * 3)(None, None, None)

    def call(E=3, nf=0, counts=(4, 4, 4), C_=2, arr=gps, disc=p, grad=p, want_grad=1):
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        return lib.moe_kg_discrete_mcmc(arr, E, nf, disc, cnt.ctypes.data_as(ip), p, p, C_, want_grad, p, grad, C.byref(err))

    assert call(E=0) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 1024.0) and b"num_mcmc" in err.message
    assert call(arr=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(disc=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(grad=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(grad=None, want_grad=0) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message  # (no gradient asked for)
    assert call(counts=(4, 0, 4096)) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 4095.0)
    assert call(counts=(4, 4, 4096), C_=0) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (4096.0, 1.0, 4095.0)
    assert b"4096 lines" in err.message
    assert call(C_=0, nf=-1) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 1e9) and b"candidates" in err.message
    assert call(nf=-1) == _lib.MOE_ERR_BOUNDS and b"num_fidelity" in err.message
    assert call(counts=(1, 4095, 12)) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    cnt = np.ascontiguousarray([4], dtype=np.int32)
    assert lib.moe_kg_discrete_mcmc(gps, 1, 0, p, cnt.ctypes.data_as(ip), p, p, 2, 1, p, p, None) == _lib.MOE_ERR_RUNTIME


def test_the_optimiser_refuses_bad_arguments_without_a_device(lib):
    dp, ip = _lib.dp, _lib.ip
    err = _lib.MoeError()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(dp)
    gps = (C.c_void_p * 2)(None, None)
    value, found = C.c_double(0.0), C.c_int(0)

    def call(E=2, nf=0, counts=(4, 4), S=3, gd=_gd(), ascent=1, arr=gps, bounds=p, point=p):
        cnt = np.ascontiguousarray(counts, dtype=np.int32)
        return lib.moe_kg_discrete_mcmc_multistart(arr, E, nf, C.byref(gd) if gd is not None else None, bounds, p,
                                                   cnt.ctypes.data_as(ip), p, p, S, ascent, point, C.byref(value), C.byref(found),
                                                   None, None, None, None, None, None, C.byref(err))

    assert call(E=0) == _lib.MOE_ERR_BOUNDS and b"num_mcmc" in err.message
    assert call(gd=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(bounds=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(point=None) == _lib.MOE_ERR_RUNTIME and b"NULL argument" in err.message
    assert call(counts=(4096, 4), S=0) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (4096.0, 1.0, 4095.0)
    assert call(S=0, nf=-1) == _lib.MOE_ERR_BOUNDS and tuple(err.payload) == (0.0, 1.0, 1e9)
    assert call(nf=-1, gd=_gd(steps=0)) == _lib.MOE_ERR_BOUNDS and b"num_fidelity" in err.message
    assert call(gd=_gd(steps=0, domain_type=1)) == _lib.MOE_ERR_BOUNDS and b"max_num_steps" in err.message
    assert tuple(err.payload) == (0.0, 1.0, 1e9)
    assert call(gd=_gd(steps=0, domain_type=1), ascent=0) == _lib.MOE_ERR_INVALID_VALUE  # (no ascent: the steps are not looked at)
    assert call(gd=_gd(domain_type=1)) == _lib.MOE_ERR_INVALID_VALUE and b"tensor-product" in err.message
    assert tuple(err.payload) == (1.0, 0.0, 0.0)
    assert call() == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message
    assert call(gd=_gd(restarts=0)) == _lib.MOE_ERR_RUNTIME and b"NULL GP handle" in err.message  # (no restart round is no error)


# ---- the inputs of the GPU tests ----
def _stops(case, r):
    """(starts stopped by their step norm, starts a restart round ended by its delta, starts that took every step of every round)"""
    by_norm, by_delta = set(), set()
    for rd in r.rounds:
        for i in range(len(rd) - 1):
            by_norm |= set(rd[i]) - set(rd[i + 1])
    for a, b in zip(r.rounds[:-1], r.rounds[1:]):
        by_delta |= set(a[0]) - set(b[0])
    full = set(k for k in range(len(r.kept))
               if len(r.rounds) == case.restarts and all(len(rd) == case.steps and all(k in st for st in rd) for rd in r.rounds))
    return by_norm, by_delta, full


def test_every_outcome_of_the_limiter_occurs():
    total = np.zeros(3, dtype=int)
    for case in kc.CASES:
        limiter = kc.float64_run(case)[1].limiter
        print("%s: clipped %d, halved at a bound %d, half-way to the bound %d" % ((case.name,) + tuple(limiter)))
        if case.max_rel <= 1.0:  # (a clipped step of at most the distance to the bound never leaves the domain)
            assert limiter[1] == 0 and limiter[2] == 0
        total += np.array(limiter)
    assert np.all(total >= 1), total
    main = [kc.float64_run(c)[1].limiter[0] for c in kc.CASES if c.max_rel == kc.MAX_REL]
    assert all(n >= 1 for n in main), main  # (every case at the outer parameters of examples/main.py clips some step)


@pytest.mark.parametrize("name", kc.LOOSE)
def test_the_loose_cases_stop_starts_in_every_way(name):
    case = [c for c in kc.CASES if c.name == name][0]
    r = kc.float64_run(case)[1]
    by_norm, by_delta, full = _stops(case, r)
    print("%s: stopped by the step norm %s, ended by the delta %s, took every step %s" % (name, sorted(by_norm), sorted(by_delta),
                                                                                       sorted(full)))
    assert len(by_norm) >= 1 and len(by_delta) >= 1 and len(full) >= 1


def test_a_round_is_left_early_where_every_start_has_stopped():
    case = [c for c in kc.CASES if c.name == "e4_n40_d3_all_stop_early"][0]
    r = kc.float64_run(case)[1]
    assert any(len(rd) < case.steps for rd in r.rounds), [len(rd) for rd in r.rounds]


def test_more_than_twenty_starts_drop_some():
    for case in kc.CASES:
        r = kc.float64_run(case)[1]
        assert len(r.kept) == min(20, case.starts)
        if case.starts > 20:
            assert len(set(range(case.starts)) - set(int(k) for k in r.kept)) == case.starts - 20
    assert any(c.starts > 20 for c in kc.CASES)


@pytest.mark.parametrize("case", kc.CASES, ids=lambda c: c.name)
def test_every_kept_end_point_has_its_margins(case):
    """kg1_reference's decision margins in long double, at every kept end point and in every member: >= 1e-6, so that the value
    check of tests/test_gpu_kg1_opt.py leaves no end point out"""
    p, r = kc.float64_run(case)
    sets = kc.discrete_sets(p, kr.LD)
    worst = min(min(min(res.margins) for res in kc.ensemble_value(sets, p, x, kr.LD)[1]) for x in r.ends)
    print("%s: smallest decision margin at the %d kept end points %.3g" % (case.name, len(r.ends), worst))
    assert worst >= 1e-6
    assert r.found and np.all(np.isfinite(r.end_values)) and np.all(r.ends >= 0.0) and np.all(r.ends <= 1.0)
