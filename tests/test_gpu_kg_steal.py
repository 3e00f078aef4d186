"""GPU tests (-m gpu) of the hand-over between evaluations in the q-KG / d-KG Monte-Carlo kernels (kg_mc.hpp: next_evaluation; DESIGN
5.3 item 3).  A workgroup whose evaluation has no sample tickets left moves to the evaluation with the most tickets left instead of
exiting.  Which wavefront computes which sample never enters the arithmetic: every per-sample output has its own slot and the pass
counters are integer atomics.  So there is no tolerance here: every case runs three times -- MOE_KG_STEAL=0 (the static assignment),
MOE_KG_STEAL=1, and MOE_KG_STEAL=1 with MOE_KG_STEAL_SKEW=1 (every workgroup starts on evaluation 0, so every other evaluation is
reached by moving only) -- and kg_sum, grad_sum, every sample's end point and both pass counters must be np.array_equal across the
three.  Each case asserts through moe_last_kernel_info that the kernel family it is meant for ran, and through moe_last_kg_moves that
the static run moved nothing and the skewed run (more than one evaluation) moved at least once."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_LANE = dict(variant=0, xlds=1, lane=1)
_FRAME = dict(variant=0, xlds=1, lane=0)
_A = dict(seed=7301, n=150, d=6, q=2, M=256, P=10)
_G1 = dict(seed=7305, n=120, d=3, q=2, M=64, P=10, derivs=(0,))
# name: (workload arguments, evaluations per call, switches of the case, what moe_last_kernel_info must report, call arguments)
CASES = {
    # the lane-parked kernel at padded dimension 8, three tiles
    "lane_dp8": (_A, 5, {}, _LANE, {}),
    # the headline's own 16-tile trip count
    "headline_tiles": (dict(seed=7302, n=1000, d=8, q=4, M=64, P=10), 3, {}, _LANE, {}),
    # the small shapes' exact multi-trial sweep, one tile
    "small_exact": (dict(seed=7303, n=60, d=3, q=2, M=128, P=10), 3, {}, _LANE, {}),
    # the frame line search
    "frame": (_A, 5, {"MOE_KG_LANE": "0"}, _FRAME, {}),
    # streamed weights, and the workgroup-per-sample kernel (one ticket per workgroup and sample)
    "stream": (_G1, 3, {"MOE_KG_VARIANT": "2"}, dict(variant=2), {}),
    "block": (_G1, 3, {"MOE_KG_VARIANT": "1"}, dict(variant=1), {}),
    # one evaluation: nowhere to move to
    "one_eval": (_A, 1, {}, _LANE, {}),
    # fewer samples than wavefronts: the first draw of every wavefront empties the counters
    "few_samples": (dict(seed=7307, n=150, d=6, q=2, M=4, P=10), 4, {}, _LANE, {}),
    # more evaluations than workgroups: the walk over the static share, then the hand-over
    "grid_stride": (dict(seed=7308, n=60, d=3, q=2, M=16, P=10), 260, {}, _LANE, {}),
    # an MC shard: first_sample > 0 and an odd number of samples
    "mc_shard": (dict(seed=7309, n=150, d=6, q=2, M=64, P=10), 3, {}, _LANE, dict(first_sample=2, num_local=61)),
    # the threshold of the hand-over at four tickets per wavefront instead of one
    "min_per_wave_4": (_A, 5, {"MOE_KG_STEAL_MIN_PER_WAVE": "4"}, _LANE, {}),
}
_DISPATCH_ENV = ("MOE_KG_LANE", "MOE_KG_VARIANT", "MOE_KG_SMALL_MULTI", "MOE_KG_SMALL_LANE_MAX_SAMPLES", "MOE_KG_DOT_MAX_RADIUS2",
                 "MOE_KG_STEAL", "MOE_KG_STEAL_SKEW", "MOE_KG_STEAL_MIN_PER_WAVE", "MOE_KG_PREP", "MOE_KG_TR")
MODES = (("static", {"MOE_KG_STEAL": "0"}), ("steal", {"MOE_KG_STEAL": "1"}),
         ("skew", {"MOE_KG_STEAL": "1", "MOE_KG_STEAL_SKEW": "1"}))


@pytest.fixture(scope="module")
def api():
    from cornell_moe_amd import _lib, api as moe_api
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"
    return moe_api


def _set_env(monkeypatch, *switch_sets):
    for k in _DISPATCH_ENV:
        monkeypatch.delenv(k, raising=False)
    for switches in switch_sets:
        for k, v in switches.items():
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_wherever_the_workgroups_go(api, monkeypatch, name):
    from cornell_moe_amd.workloads import make_workload
    args, E, switches, expect, call = CASES[name]
    w = make_workload(num_restarts=E, **args)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs)
    best = float(G.additional_mean(w.discrete).min())
    runs = {}
    for mode, mode_env in MODES:
        _set_env(monkeypatch, switches, mode_env)
        r = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, None, w.M, best, w.kg_normals, **call)
        info = G.last_kernel_info()
        for key, val in expect.items():
            assert info[key] == val, (mode, key, info)
        pts = G.last_kg_best_points()
        assert pts.shape == (E, call.get("num_local", w.M), w.d)
        runs[mode] = (r, pts, G.last_kg_moves(), info)
    r0, p0, moves0, info0 = runs["static"]
    assert moves0 == 0
    assert np.all(np.isfinite(r0["kg_sum"])) and np.abs(r0["grad_sum"]).max() > 0 and r0["mean_evals"] > 0 and r0["grad_evals"] > 0
    if name == "grid_stride":
        assert info0["blocks"] < E, info0
    if name == "small_exact":
        assert info0["waves"] <= 8
    for mode in ("steal", "skew"):
        r, p, moves, info = runs[mode]
        print("%s %s: %d moves, %d workgroups x %d waves" % (name, mode, moves, info["blocks"], info["waves"]))
        assert info == info0
        assert np.array_equal(r["kg_sum"], r0["kg_sum"]), (mode, "kg_sum")
        assert np.array_equal(r["grad_sum"], r0["grad_sum"]), (mode, "grad_sum")
        assert np.array_equal(p, p0), (mode, "best_point")
        assert (r["mean_evals"], r["grad_evals"]) == (r0["mean_evals"], r0["grad_evals"]), (mode, "pass counters")
    if E == 1:
        assert runs["steal"][2] == 0 and runs["skew"][2] == 0
    else:
        assert runs["skew"][2] >= 1


def test_one_merged_ensemble_launch(api, monkeypatch):
    """Two members of a GP ensemble in ONE launch of the MC kernel's ensemble twin (launch.hpp), skewed against the static assignment:
    the twin runs the same body, so its workgroups move within their own member's evaluations."""
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=7311, n=150, d=6, q=2, M=128, P=10, num_restarts=4)
    hypers = np.stack([np.concatenate([[w.alpha], w.lengths]), np.concatenate([[1.1 * w.alpha], 0.9 * w.lengths])])
    noises = np.tile(np.asarray(w.noise, dtype=np.float64).reshape(1, -1), (2, 1))
    disc = np.tile(w.discrete.reshape(1, -1), (2, 1))
    Gm = api.DeviceGPMCMC(hypers, noises, w.X, w.y, ())
    bests = np.array([float(gp.additional_mean(w.discrete).min()) for gp in Gm.gps])
    out = {}
    try:
        api.set_ensemble_launches(1)
        for mode, mode_env in (MODES[0], MODES[2]):
            _set_env(monkeypatch, mode_env)
            s0 = api.ensemble_launch_stats()
            kg, grad = Gm.kg_batch(w.inner_gd, w.bounds, disc, w.Xq_restarts, None, w.M, bests, w.kg_normals)
            s1 = api.ensemble_launch_stats()
            assert s1[0] > s0[0] and s1[1] == s0[1], (mode, s0, s1)  # merged, no fall-back to per-member launches
            for gp in Gm.gps:
                info = gp.last_kernel_info()
                assert (info["variant"], info["lane"]) == (0, 1), info
            out[mode] = (kg, grad, [gp.last_kg_best_points() for gp in Gm.gps], [gp.last_kg_moves() for gp in Gm.gps])
    finally:
        api.set_ensemble_launches(-1)
    k0, g0, p0, m0 = out["static"]
    k1, g1, p1, m1 = out["skew"]
    assert m0 == [0, 0] and min(m1) >= 1, (m0, m1)
    assert np.all(np.isfinite(k0)) and np.abs(g0).max() > 0
    assert np.array_equal(k0, k1) and np.array_equal(g0, g1)
    for a, b in zip(p0, p1):
        assert a.shape == (4, w.M, w.d) and np.array_equal(a, b)
