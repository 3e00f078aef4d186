"""q,p-EI on the device (csrc/ei.hip) where the parity and sweep tests do not reach: every union-size class of the state and Monte-Carlo
kernels with and without the gradient (value-only calls above u = 16 among them), every layout of the final sum (129 components and
more, a second and a third round of them, the union-point staging exactly full), sample counts around a wavefront and a workgroup and
beyond 256 workgroups, GP sizes on either side of the fused / K-sliced switch of the state kernels and beyond the 1024 rows the fused
kernel stages from registers, batches (wide unions and the K-sliced side among them), saturated decisions, and an ensemble of GPs above
u = 16.  tests/ei_cases.py holds the shapes and says which path each takes.

The checker is tests/ei_reference.py (np.longdouble), not the double-precision oracle: tests/test_ei_reference.py holds it to the
reference's recorded results, and shows for every shape used here that no sample's decision is rounding-sized and that plain double
arithmetic stays within a tenth of the tolerance.  Every device result is held to it at the suite's own TOL["ei"] / TOL["grad_ei"]
(1e-10 / 1e-9 relative, floor 1e-3).  GPs with derivative observations keep the oracle as their checker.

Every test prints what it observed: `ei-edge <group> <id> <value distance> <gradient distance>`."""
import numpy as np
import pytest

import ei_cases
from ei_cases import ei_distance, grad_distance
import ei_reference as er
from cornell_moe_amd import api
from helpers import TOL

pytestmark = pytest.mark.gpu


def _gp(P, hyper=None, noise=None):
    w = P.w
    return api.DeviceGP(w.hyperparameters if hyper is None else hyper, w.X, w.y, w.noise if noise is None else noise, w.derivs, cov_type=P.cov)


def _reference(P, hyper=None, noise=None):
    w = P.w
    return er.EiReference(P.cov, w.hyperparameters if hyper is None else hyper, w.X, w.y, w.noise if noise is None else noise)


def _hold(case, what, ei, grad, want_ei, want_grad):
    """the device's (ei, grad or None) against the checker's, at TOL; returns the two distances"""
    de = ei_distance(ei, want_ei)
    dg = grad_distance(grad, want_grad) if grad is not None else 0.0
    assert np.isfinite(ei) and de <= TOL["ei"], (case["id"], what, float(ei), float(want_ei), de)
    assert dg <= TOL["grad_ei"], (case["id"], what, dg)
    return de, dg


def _report(case, de, dg):
    print("ei-edge %s %s %.2e %.2e" % (case["group"], case["id"], de, dg))


_SINGLE = [c for c in ei_cases.CASES if c["E"] == 1 and not c["nm"]]


@pytest.mark.parametrize("case", _SINGLE, ids=[c["id"] for c in _SINGLE])
def test_single_evaluation_against_extended_reference(case):
    """groups a - d and f of tests/ei_cases.py"""
    P = ei_cases.problem(case)
    w = P.w
    G, R = _gp(P), _reference(P)
    r = R.ei(w.Xq, P.Xp, P.best, P.normals, True in case["grad"])
    worst = [0.0, 0.0]
    for want_grad in case["grad"]:
        ei, grad = G.ei(w.Xq, P.Xp, w.M, P.best, P.normals, want_grad=want_grad)
        assert (grad is not None) == want_grad
        de, dg = _hold(case, want_grad, ei, grad, r.ei, r.grad if want_grad else None)
        worst = [max(worst[0], de), max(worst[1], dg)]
        if case["best"] == "below":                       # no sample improves: nothing is added up
            assert ei == 0.0 and (grad is None or not grad.any()), (case["id"], ei)
        else:
            assert ei > 0.0 and (grad is None or np.abs(grad).max() > 0.0), case["id"]
        again = G.ei(w.Xq, P.Xp, w.M, P.best, P.normals, want_grad=want_grad)   # (tickets and workspaces left as they were found)
        assert again[0] == ei and (grad is None or np.array_equal(again[1], grad)), case["id"]
    G.close()
    _report(case, *worst)


_BATCH = [c for c in ei_cases.CASES if c["E"] > 1 and not c["nm"]]


@pytest.mark.parametrize("case", _BATCH, ids=[c["id"] for c in _BATCH])
def test_batch_entries_against_reference_and_single_evaluations(case):
    """group e: every entry of moe_ei_batch against the checker, and equal to its single evaluation BIT FOR BIT"""
    P = ei_cases.problem(case)
    w, E = P.w, case["E"]
    G, R = _gp(P), _reference(P)
    refs = [R.ei(P.Xq_all[e], P.Xp, P.best, P.normals, True in case["grad"]) for e in range(E)]
    worst = [0.0, 0.0]
    for want_grad in case["grad"]:
        ei, grad = G.ei_batch(P.Xq_all, P.Xp, w.M, P.best, P.normals, want_grad=want_grad)
        assert ei.shape == (E,) and (grad is not None) == want_grad
        for e in range(E):
            de, dg = _hold(case, (want_grad, e), ei[e], grad[e] if want_grad else None, refs[e].ei, refs[e].grad if want_grad else None)
            worst = [max(worst[0], de), max(worst[1], dg)]
            e1, g1 = G.ei(P.Xq_all[e], P.Xp, w.M, P.best, P.normals, want_grad=want_grad)
            assert e1 == ei[e] and (not want_grad or np.array_equal(g1, grad[e])), (case["id"], want_grad, e)
        assert len(set(ei.tolist())) == E                 # (the entries did get answers of their own)
    G.close()
    _report(case, *worst)


_ENSEMBLE = [c for c in ei_cases.CASES if c["nm"]]


@pytest.mark.parametrize("case", _ENSEMBLE, ids=[c["id"] for c in _ENSEMBLE])
def test_ensemble_above_sixteen_points(case):
    """group g: DeviceGPMCMC.ei_batch at u = 20 -- the host-algebra branch of ei_launch, which waits on the stream mid-way and so stays
    out of what the ensemble path records: the same bits with ensemble-wide launches on and off, and the mean of the members' values"""
    P = ei_cases.problem(case)
    w, E, nm = P.w, case["E"], case["nm"]
    hypers, noises = ei_cases.ensemble_members(P)
    G = api.DeviceGPMCMC(hypers, noises, w.X, w.y, ())
    best = np.full(nm, P.best)
    out = {}
    try:
        for on in (0, 1):
            api.set_ensemble_launches(on)
            out[on] = [G.ei_batch(P.Xq_all, P.Xp, w.M, best, P.normals), G.ei_batch(P.Xq_all, P.Xp, w.M, best, P.normals, want_grad=False),
                       G.ei_batch(P.Xq_all, P.Xp, w.M, best, P.normals)]
    finally:
        api.set_ensemble_launches(-1)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a[0], b[0])
        assert (a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])
    ei, grad = out[1][0]
    assert np.all(np.isfinite(ei)) and np.all(np.isfinite(grad)) and np.abs(grad).max() > 0
    assert np.array_equal(out[1][2][0], ei) and np.array_equal(out[1][2][1], grad)
    members = [_reference(P, h, nz) for h, nz in zip(hypers, noises)]
    worst = [0.0, 0.0]
    for e in range(E):
        refs = [R.ei(P.Xq_all[e], P.Xp, P.best, P.normals) for R in members]
        want_ei = sum(r.ei for r in refs) / er.LD(nm)
        want_grad = sum(r.grad for r in refs) / er.LD(nm)
        de, dg = _hold(case, e, ei[e], grad[e], want_ei, want_grad)
        dv, _ = _hold(case, (e, "value only"), out[1][1][0][e], None, want_ei, None)
        worst = [max(worst[0], de, dv), max(worst[1], dg)]
    _report(case, *worst)


@pytest.mark.parametrize("case", ei_cases.DERIV_CASES, ids=[c["id"] for c in ei_cases.DERIV_CASES])
def test_gps_with_observed_derivatives_against_oracle(case):
    """group a, the GPs with derivative observations (u = 9: the 16-wide state kernel; u = 20: the host algebra): EI points carry no
    derivative rows, so what differs from the cases above is the state set-up; the double-precision oracle is the checker"""
    from oracle import orc
    P = ei_cases.problem(case)
    w = P.w
    G = _gp(P)
    O = orc.OrcGP(P.cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
    eo, go = O.ei(w.Xq, P.Xp, w.M, P.best, P.normals)
    worst = [0.0, 0.0]
    for want_grad in case["grad"]:
        ei, grad = G.ei(w.Xq, P.Xp, w.M, P.best, P.normals, want_grad=want_grad)
        de, dg = _hold(case, want_grad, ei, grad, eo, go if want_grad else None)
        worst = [max(worst[0], de), max(worst[1], dg)]
        assert ei > 0.0 and (grad is None or np.abs(grad).max() > 0.0)
    G.close()
    _report(case, *worst)
