"""The dispatch branches of csrc/recommend.hip that tests/test_gpu_recommend.py does not reach, against tests/recommend_reference.py
with that file's checks (_check_descent, _assert_value_grad) and bounds: the descent at every padded dimension (8, 16, 24, 32 -- the
4-wavefront instantiations among them) with idle wavefronts and a second member group; the batch at padded 16 and 24 around the row
stride; n = 1 and n = 2; the MOE_RECOMMEND_XLDS=1 variant at, below and above its two limits, bit for bit against the default, which
is itself held to the extended-precision map; pm_select_kernel with more candidates than threads, with equal values in rounds t > 0
and with a NaN candidate.  The inputs are recommend_reference.edge_cases(); tests/test_recommend_reference.py asserts their decision
margins (>= 1e-7) on the CPU.  Every test prints the worst figures it saw (pytest -s)."""
import numpy as np
import pytest

import recommend_reference as rr
from cornell_moe_amd import api
from test_gpu_recommend import MARGIN, MATERN, SE, _assert_value_grad, _build, _check_descent, row_stride

pytestmark = pytest.mark.gpu


def _cases(kind):
    return [c for c in rr.edge_cases() if c.kind == kind]


def _device(case):
    members, a, bounds, cand = rr.edge_problem(case)
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=case.cov) for e in range(case.E)]
    return gps, rr.Ensemble(members, case.num_fidelity), bounds, cand


@pytest.mark.parametrize("case", _cases("descent"), ids=rr.edge_id)
def test_descent_at_every_padded_dimension(case):
    gps, ens, bounds, cand = _device(case)
    res, want = _check_descent(gps, ens, case.gd, bounds, cand, case.S, rr.edge_id(case))
    assert min(want.margins) >= MARGIN
    assert np.array_equal(rr.top_indices(res["candidate_values"], case.S), want.starts)
    assert res["screened_index"] == want.index and res["refined"] == want.refined
    assert np.array_equal(res["point"], res["end_points"][want.winner] if want.refined else cand[want.index])


# E, d, cov, derivs, num_fidelity: padded 16 (d = 16, 13), 8 with a second member group, 32 with a second group, 24 with an idle wavefront
BATCH_CASES = [(3, 16, SE, (), 0), (5, 13, MATERN, (0, 12), 1), (9, 8, MATERN, (), 0), (5, 32, SE, (), 0), (3, 24, MATERN, (), 1)]


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: "E%d-d%d-cov%d-g%d-f%d" % (c[0], c[1], c[2], len(c[3]), c[4]))
def test_batch_around_the_row_stride(case):
    E, d, cov, derivs, nf = case
    stride = row_stride(E, d)
    P = 7
    for n in (stride - 1, stride, stride + 1):
        gps, ens, a = _build(10 * E + d + n, n, d, E, cov, derivs, nf)
        pts = np.random.default_rng(n).uniform(0, 1, size=(P, d - nf))
        value, grad = api.posterior_mean_mcmc(gps, pts, nf, want_grad=True)
        _assert_value_grad(value, grad, ens, pts, "E=%d d=%d n=%d (stride %d) P=%d" % (E, d, n, stride, P))
        assert np.array_equal(api.posterior_mean_mcmc(gps, pts, nf), value)  # the value-only kernel: the same bits
        k = P // 2
        v1, g1 = api.posterior_mean_mcmc(gps, pts[k:k + 1], nf, want_grad=True)
        assert v1[0] == value[k] and np.array_equal(g1[0], grad[k])  # a point alone: the bits it has inside the batch


@pytest.mark.parametrize("case", _cases("small"), ids=rr.edge_id)
def test_one_and_two_training_points(case):
    gps, ens, bounds, cand = _device(case)
    pts = np.random.default_rng(case.n + case.d).uniform(0, 1, size=(5, case.d))
    value, grad = api.posterior_mean_mcmc(gps, pts, 0, want_grad=True)
    _assert_value_grad(value, grad, ens, pts, rr.edge_id(case))
    assert np.array_equal(api.posterior_mean_mcmc(gps, pts, 0), value)
    assert float(np.max(np.abs(grad))) > 0.0  # (a single function value would equal the constant mean: these members observe more)
    res, want = _check_descent(gps, ens, case.gd, bounds, cand, 1, rr.edge_id(case) + " descent")
    assert min(want.margins) >= MARGIN and res["screened_index"] == want.index and res["refined"] == want.refined


@pytest.mark.parametrize("case", _cases("lds"), ids=rr.edge_id)
def test_training_points_staged_in_lds_give_the_same_bits(case, monkeypatch):
    """8 n DP bytes of dynamic LDS: d = 32 at n = 192 is exactly 48 KiB (no attribute call), 193 needs the attribute, 384 is exactly
    96 KiB (the last that is staged), 385 goes back to global memory.  The switch is read per call."""
    gps, ens, bounds, cand = _device(case)
    monkeypatch.delenv("MOE_RECOMMEND_XLDS", raising=False)
    off, want = _check_descent(gps, ens, case.gd, bounds, cand, 1, rr.edge_id(case) + " (switch off)")  # the pair cannot agree on a wrong answer
    assert min(want.margins) >= MARGIN and off["screened_index"] == want.index
    monkeypatch.setenv("MOE_RECOMMEND_XLDS", "1")
    on = api.recommend(gps, cand, rr.gd_tuple(case.gd), bounds, want_values=True, want_path=True)
    for key in ("path", "end_points", "point", "candidate_values"):
        assert np.array_equal(on[key], off[key]), key
    assert on["value"] == off["value"] and on["screened_index"] == off["screened_index"] and on["refined"] == off["refined"]
    print("%s: %d bytes of training points, staged and default agree bit for bit" % (rr.edge_id(case), 8 * case.n * (4 if case.d <= 4 else 32)))


@pytest.mark.parametrize("case", _cases("select"), ids=rr.edge_id)
def test_selection_with_more_candidates_than_threads(case):
    gps, ens, bounds, cand = _device(case)
    want = rr.extended(ens, case.gd, bounds, cand, case.S)
    print("%s: margins at rank 1 and at the cut %s" % (rr.edge_id(case), want.margins[:2]))
    assert min(want.margins[:2]) >= MARGIN
    res = api.recommend(gps, cand, rr.gd_tuple(case.gd), bounds, num_starts=case.S, want_values=True, want_path=True)
    starts = rr.top_indices(res["candidate_values"], case.S)
    assert np.array_equal(res["path"][:, 0], cand[starts])  # exactly, in this order
    assert set(starts) == set(want.starts) and res["screened_index"] == want.index == starts[0]


def test_equal_values_in_later_rounds_go_by_index():
    case = _cases("ties")[0]
    members, a, bounds, cand, picks, margins = rr.ties_problem(case)
    print("ties: margins between ranks 1 .. 5 %s, picks %s" % (margins, picks))
    assert min(margins) >= MARGIN
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=case.cov) for e in range(case.E)]
    res = api.recommend(gps, cand, rr.gd_tuple(case.gd), bounds, num_starts=4, want_values=True, want_path=True)
    v = res["candidate_values"]
    assert v[picks[1]] == v[picks[2]] and picks[2] >= 256  # a point's value does not depend on its index
    assert np.array_equal(cand[picks[1]], cand[picks[2]]) and (picks[1] % 256) // 64 != (picks[2] % 256) // 64
    assert list(rr.top_indices(v, 4)) == picks
    assert np.array_equal(res["path"][:, 0], cand[picks]) and res["screened_index"] == picks[0]
    # the second-best and its copy start the same descent
    assert np.array_equal(res["path"][1], res["path"][2]) and np.array_equal(res["end_points"][1], res["end_points"][2])


@pytest.mark.parametrize("where", [0, 299])
def test_a_nan_candidate_is_never_picked(where):
    case = _cases("nan")[0]
    members, a, bounds, cand, starts, margins = rr.nan_problem(case, where)
    print("NaN at %d: margins at rank 1 and at the cut among the others %s" % (where, margins))
    assert min(margins) >= MARGIN and where not in starts
    gps = [api.DeviceGP(a["hypers"][e], a["X"], a["y"], a["noises"][e], a["derivs"], cov_type=case.cov) for e in range(case.E)]
    res = api.recommend(gps, cand, rr.gd_tuple(case.gd), bounds, num_starts=case.S, want_values=True, want_path=True)
    v = res["candidate_values"]
    assert np.isnan(v[where]) and int(np.sum(np.isnan(v))) == 1
    assert res["screened_index"] == starts[0]
    got = [int(np.where(np.all(cand == res["path"][s, 0], axis=1))[0][0]) for s in range(case.S)]  # (a NaN row equals nothing)
    assert set(got) == set(int(i) for i in starts) and got[0] == starts[0]
    assert got == [int(i) for i in np.array(sorted((i for i in range(case.C) if i != where), key=lambda i: (-v[i], i))[:case.S])]
    assert np.all(np.isfinite(res["path"])) and np.all(np.isfinite(res["end_points"])) and np.isfinite(res["value"])
