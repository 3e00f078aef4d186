"""GPU tests (-m gpu) of the lookup-first tile loops of the LDS-table wave-per-sample q-KG kernels (kg_mc.hpp: eval_loop,
eval_multi_loop_s, eval_multi_exact; kg_mc_lane.hpp: grad_pass_parked).  The loops issue their exp-table reads ahead of the
next tile's reads and finish the exponentials afterwards: a reordering of independent LDS loads that adds, removes, reassociates and
contracts no floating-point operation.  So every case is held BIT FOR BIT (np.array_equal) to what the library of the commit before
the reordering returned on the same seeded inputs -- tests/golden/kg_lookup_order/*.npy, recorded by tools/record_kg_lookup_order.py
through this file's own CASES / run_case / pack: kg_sum, grad_sum, every sample's end point, both pass counters.  Each case also asserts
through moe_last_kernel_info that the intended kernel ran (and the same one as when the fixture was recorded), so that a change of the
dispatch cannot hide a path that is no longer exercised.  The lane-parked kernel takes the new order at padded dimension <= 8 with at
most one derivative slot (cases a, b, c, e_n200: kg_mc_lane.hpp kLaneLookupFirst); the other cases -- padded dimension 12 / 16, the
exact small-shape sweep, the frame kernel -- keep one lookup at a time and are held to the same fixtures.  moe_last_kernel_info does
not report which sweep (exact / line-decomposed / single-trial) a small shape took: run_case clears the switches that choose it, so the
default dispatch is what runs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (workload arguments, covariance (0 squared exponential, 1 Matern-5/2), MOE_KG_LANE, what moe_last_kernel_info must report)
# `expect`: variant 0 = wave-per-sample kernel, xlds 1 = coordinate table in LDS, lane 1 = lane-parked line search (0: frame line search)
_LANE = dict(variant=0, xlds=1, lane=1)
_FRAME = dict(variant=0, xlds=1, lane=0)
CASES = {
    # three tiles: the sweep's two-tile and the gradient pass's four-tile unroll both run their remainder iterations
    "a_n150_d6": (dict(seed=7101, n=150, d=6, q=2, M=64, P=10), 1, "1", _LANE),
    # the headline's own 16-tile trip count
    "b_n1000_d8": (dict(seed=7102, n=1000, d=8, q=4, M=64, P=10), 1, "1", _LANE),
    # the squared-exponential path
    "c_n150_d6_se": (dict(seed=7101, n=150, d=6, q=2, M=64, P=10), 0, "1", _LANE),
    # padded dimensions 12 and 16
    "d_n200_d10": (dict(seed=7104, n=200, d=10, q=2, M=64, P=10), 1, "1", _LANE),
    "d_n200_d14": (dict(seed=7105, n=200, d=14, q=2, M=64, P=10), 1, "1", _LANE),
    # one observed derivative: the derivative slot (two tiles: the small shapes' exact multi-trial sweep; four tiles: the line sweep)
    "e_n120_d3_g1": (dict(seed=7106, n=120, d=3, q=2, M=64, P=10, derivs=(0,)), 1, "1", _LANE),
    "e_n200_d3_g1": (dict(seed=7107, n=200, d=3, q=2, M=64, P=10, derivs=(0,)), 1, "1", _LANE),
    # the small shapes' exact multi-trial sweep, one tile
    "f_n60_d3": (dict(seed=7108, n=60, d=3, q=2, M=128, P=10), 1, "1", _LANE),
    # (a) and (b) on the frame kernel
    "g_n150_d6_frame": (dict(seed=7101, n=150, d=6, q=2, M=64, P=10), 1, "0", _FRAME),
    "g_n1000_d8_frame": (dict(seed=7102, n=1000, d=8, q=4, M=64, P=10), 1, "0", _FRAME),
}
_DISPATCH_ENV = ("MOE_KG_LANE", "MOE_KG_VARIANT", "MOE_KG_SMALL_MULTI", "MOE_KG_SMALL_LANE_MAX_SAMPLES", "MOE_KG_DOT_MAX_RADIUS2")
INFO_KEYS = ("variant", "xlds", "lane", "waves", "start_table")


def run_case(api, name):
    """One q-KG evaluation of case `name` under its MOE_KG_LANE; returns (result dict with best_point, last_kernel_info)."""
    from cornell_moe_amd.workloads import make_workload
    args, cov, lane, _ = CASES[name]
    w = make_workload(**args)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
    best = float(G.additional_mean(w.discrete).min())
    # the dispatch switches at their defaults: which kernel and which sweep run is part of what a case pins
    saved = {k: os.environ.pop(k, None) for k in _DISPATCH_ENV}
    os.environ["MOE_KG_LANE"] = lane
    try:
        res = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, None, w.M, best, w.kg_normals, want_best_points=True)
        info = G.last_kernel_info()
    finally:
        os.environ.pop("MOE_KG_LANE", None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return res, info


def pack(res, info):
    """[kg_sum | passes: value, gradient | the INFO_KEYS of moe_last_kernel_info | grad_sum (q d) | best_point (M d)] as float64"""
    head = [res["kg_sum"], float(res["mean_evals"]), float(res["grad_evals"])] + [float(info[k]) for k in INFO_KEYS]
    return np.concatenate([np.array(head), res["grad_sum"].ravel(), res["best_point"].ravel()])


@pytest.fixture(scope="module")
def api():
    from cornell_moe_amd import _lib, api as moe_api
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"
    return moe_api


@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_parent_commit(api, name):
    args, _, _, expect = CASES[name]
    want = np.load(os.path.join(_ROOT, "tests", "golden", "kg_lookup_order", name + ".npy"))
    res, info = run_case(api, name)
    for key, val in expect.items():
        assert info[key] == val, (key, info)
    if name.startswith("f_") or name == "e_n120_d3_g1":
        assert info["waves"] <= 8  # one or two tiles on the lane-parked kernel (kg.hip: small_lane; by default its exact multi-trial sweep)
    got = pack(res, info)
    nh = 3 + len(INFO_KEYS)
    q, d, M = args["q"], args["d"], args["M"]
    assert want.shape == got.shape == (nh + q * d + M * d,)
    assert np.array_equal(got[3:nh], want[3:nh]), "another kernel than the recorded one: %s" % (info,)
    assert got[0] == want[0], "kg_sum %.17g, recorded %.17g" % (got[0], want[0])
    assert np.array_equal(got[nh:nh + q * d], want[nh:nh + q * d]), "grad_sum"
    assert np.array_equal(got[nh + q * d:], want[nh + q * d:]), "best_point"
    assert np.array_equal(got[1:3], want[1:3]), "pass counters"
