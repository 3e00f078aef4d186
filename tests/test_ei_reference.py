"""tests/ei_reference.py (the extended-precision checker of the device's q,p-EI) against what the unmodified reference recorded in
tests/golden/ (the EI outputs of the golden cases, the C2 entry of ref_shapes.npz) and against the double-precision oracle, and the
qualification of every shape of tests/ei_cases.py.  No GPU: this is what makes tests/test_gpu_ei_edges.py trustworthy.

Qualification, per shape:
 (1) no sample has a decision margin (|best - y_winner|, or the lead of the winner over the runner-up) inside a band of
     1e-9 max(1, |best|, max |y|): four orders of magnitude above the error of y in double arithmetic, so a correct double-precision
     evaluation takes every decision as the extended one does, and a distance from the reference is rounding, never a flipped sample;
 (2) the oracle (the same algorithm in plain double arithmetic) lies within a TENTH of TOL["ei"] / TOL["grad_ei"] of the extended
     reference, in the relative form with the 1e-3 floor of the EI tests: the tolerance the device is held to has headroom there.
A shape that fails either is replaced in the table, never exempted."""
import numpy as np
import pytest

import ei_cases
from ei_cases import ei_distance, grad_distance
import ei_reference as er
from helpers import TOL, load_golden, load_golden_shapes, shape_checksum
from oracle import orc

BAND = 1e-9


def test_reference_module_reproduces_the_golden_ei():
    """every golden case without derivative observations: both covariance types, p = 0 and p > 0"""
    cases, _ = load_golden()
    seen, worst = set(), [0.0, 0.0]
    for c in cases:
        i = c.inp
        if len(i["derivs"]):
            continue
        R = er.EiReference(int(i["cov_type"]), np.r_[float(i["alpha"]), i["lengths"]], i["X"], i["y"], i["noise"])
        Xp = i["Xp"] if int(i["p"]) > 0 else None
        u = np.asarray(i["Xq"]).reshape(-1, R.X.shape[1]).shape[0] + int(i["p"])
        r = R.ei(i["Xq"], Xp, float(i["ei_best"]), np.ravel(i["ei_normals"])[:int(i["M"]) * u])
        assert r.near_ties(BAND) == 0
        de, dg = ei_distance(r.ei, c.out["ei"]), grad_distance(r.grad, np.asarray(c.out["grad_ei"]).reshape(r.grad.shape))
        worst = [max(worst[0], de), max(worst[1], dg)]
        assert de <= TOL["ei"] and dg <= TOL["grad_ei"], (c.index, de, dg)
        seen.add((int(i["cov_type"]), int(i["p"]) > 0))
    print("extended reference vs golden EI: worst %.2e (value), %.2e (gradient)" % tuple(worst))
    assert {s[0] for s in seen} == {0, 1} and {s[1] for s in seen} == {False, True}, seen


def test_reference_module_reproduces_c2():
    """BASELINE C2 (n = 500, d = 4, q = 2, M = 1000) as the reference evaluated it, at both recorded incumbents; n = 500 takes the
    refinement path of k_inverse_times, which is held to the direct solve here as well"""
    from cornell_moe_amd.workloads import make_workload
    z = load_golden_shapes()
    w = make_workload("C2")
    assert np.array_equal(shape_checksum(w), z["c2_check"])
    R = er.EiReference(1, w.hyperparameters, w.X, w.y, w.noise)
    D = er.EiReference(1, w.hyperparameters, w.X, w.y, w.noise, refine=False)
    assert R.refine and not D.refine
    assert float(np.abs(R.a - D.a).max() / np.abs(D.a).max()) <= 1e-14
    for tag in ("", "_median"):
        best = float(z["c2_best" + tag])
        r = R.ei(w.Xq, None, best, w.ei_normals)
        assert ei_distance(r.ei, z["c2_ei" + tag]) <= TOL["ei"]
        assert grad_distance(r.grad, z["c2_grad_ei" + tag].reshape(r.grad.shape)) <= TOL["grad_ei"]
        r2 = D.ei(w.Xq, None, best, w.ei_normals)
        assert ei_distance(r.ei, r2.ei) <= 1e-14 and grad_distance(r.grad, r2.grad) <= 1e-13


def test_smith_recursion_is_the_derivative_of_the_factor():
    """against the closed form dL = L Phi(L^-1 dV L^-T) (Phi: the lower triangle with half the diagonal) and a central difference"""
    rng = np.random.default_rng(3)
    u = 7
    a = rng.normal(size=(u, u))
    V = (a @ a.T + u * np.eye(u)).astype(er.LD)
    s = rng.normal(size=(2, u, u))
    dV = (s + s.transpose(0, 2, 1)).astype(er.LD)
    L = er.sr.cholesky_spd(V)
    dL = er.smith_factor_derivative(L, dV)
    for b in range(2):
        inner = er.sr.forward_solve(L, er.sr.forward_solve(L, dV[b]).T).T     # L^-1 dV L^-T
        phi = np.tril(inner)
        phi[np.arange(u), np.arange(u)] /= 2
        assert float(np.abs(dL[b] - L @ phi).max()) <= 1e-17
        h = er.LD(2) ** -20
        fd = (er.sr.cholesky_spd(V + h * dV[b]) - er.sr.cholesky_spd(V - h * dV[b])) / (2 * h)
        assert float(np.abs(dL[b] - fd).max()) <= 1e-10
        assert not np.triu(dL[b], 1).any()


def test_margins_and_first_index_rule():
    """u = 1: no runner-up; a sample at the incumbent counts for nothing; equal values go to the first index (np.argmax)"""
    rng = np.random.default_rng(5)
    X = rng.uniform(size=(12, 2))
    y = rng.normal(size=(12, 1))
    R = er.EiReference(1, [1.0, 0.5, 0.5], X, y, [0.01])
    one = R.ei(X[:1] + 0.1, None, 0.0, rng.normal(size=(9, 1)))
    assert np.isinf(one.winner_margin).all() and one.near_ties(BAND) == 0
    mu, L, _, _ = R.state(X[:1] + 0.1, None, want_grad=False)
    tie = R.ei(X[:1] + 0.1, None, float(mu[0]), np.zeros((1, 1)))
    assert abs(float(tie.ei)) <= 1e-15 and tie.near_ties(BAND) == 1                  # (y = mu in extended precision, best = mu rounded)
    two = R.ei(X[:2] + 0.1, None, 50.0, np.zeros((4, 2)))                      # t_s the same four times: margins repeat
    assert two.improving == 4 and len(set(two.winner_margin.tolist())) == 1


def _members(P):
    """(extended reference, oracle) per GP of a case: one, or the members of its ensemble"""
    w = P.w
    if not P.case["nm"]:
        return [(er.EiReference(P.cov, w.hyperparameters, w.X, w.y, w.noise), orc.OrcGP(P.cov, w.alpha, w.lengths, w.X, w.y, w.noise, ()))]
    hypers, noises = ei_cases.ensemble_members(P)
    return [(er.EiReference(P.cov, h, w.X, w.y, nz), orc.OrcGP(P.cov, float(h[0]), h[1:], w.X, w.y, nz, ())) for h, nz in zip(hypers, noises)]


@pytest.mark.parametrize("case", ei_cases.CASES, ids=[c["id"] for c in ei_cases.CASES])
def test_case_is_qualified(case):
    P = ei_cases.problem(case)
    w = P.w
    want_grad = True in case["grad"]
    worst, improving = [0.0, 0.0], []
    sets = range(case["E"]) if case["E"] <= 8 else (0, 1, case["E"] // 2, case["E"] - 1)   # (the oracle's share of a big batch)
    for R, O in _members(P):
        for e in range(case["E"]):
            r = R.ei(P.Xq_all[e], P.Xp, P.best, P.normals, want_grad)
            assert r.near_ties(BAND) == 0, (case["id"], e, float(r.zero_margin.min()), float(r.winner_margin.min()), float(r.scale))
            improving.append(r.improving)
            if case["best"] == "below":
                assert r.improving == 0
            elif case["best"] == "above":
                assert r.improving == w.M
            else:
                assert r.improving > 0                   # (a case whose samples all miss would check nothing)
            if e not in sets:
                continue
            eo, go = O.ei(P.Xq_all[e], P.Xp, w.M, P.best, P.normals, want_grad=want_grad)
            worst[0] = max(worst[0], ei_distance(eo, r.ei))
            if want_grad:
                worst[1] = max(worst[1], grad_distance(go, r.grad))
    print("%s: oracle vs extended reference %.2e (value; a tenth of TOL: %.0e), %.2e (gradient; %.0e); %d .. %d of %d samples improve"
          % (case["id"], worst[0], TOL["ei"] / 10, worst[1], TOL["grad_ei"] / 10, min(improving), max(improving), w.M))
    assert worst[0] <= TOL["ei"] / 10 and worst[1] <= TOL["grad_ei"] / 10, (case["id"], worst)
