"""GPU tests (-m gpu) of the S_W-free form of the T-free q-KG gradient tail (kg_tail.hip: kg_fused_point_kernel's union rows and
kg_zc_direct_kernel; MOE_KG_FUSED_ONE_PASS=1, the default).  The form replaces the per-sample S_W,i = W^T T_i and
c_i = L^-1 alpha (k(Xu, x*_i) - S_W,i) by ZC = L^T (KB - TB^T W) L^-T, with the sum over the samples taken first.  It is held
  * to the two-kernel form (MOE_KG_FUSED_ONE_PASS=0: kg_fused_sample_kernel + kg_fused_c_kernel + kg_fused_point_kernel + kg_zc_part)
    at test_one_pass_tail_matches_two_kernel_tail's bound -- kg_sum bit for bit, grad_sum within 1e-12 max(|grad_sum|, |kg_sum|) -- on
    either side of a 256-point block and a 128-sample chunk, for m in {1, 2, 4, 5, 8}, padded dimensions 4, 8, 12, both kernels;
  * to its own bits alone, in a batch and at another position of the batch;
  * to the unsharded call when the samples are dealt to two MC shards (1e-12: the project's bound for MC shards);
  * to the CPU oracle where the subtraction after the sum is at its worst: a point being sampled 1e-3 length scales from a training
    point under a noise of 1e-6 alpha, so that the posterior covariance is orders below the prior one;
  * to its own bits with ensemble-wide launches on and off."""
import numpy as np
import pytest

from helpers import TOL, reference_checker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from cornell_moe_amd import _lib, api as moe_api
    _lib.load()
    assert _lib.device_count() > 0, "no GPU visible"
    return moe_api


def _both_forms(monkeypatch, call):
    """call() under the two-kernel form, then under the S_W-free form"""
    monkeypatch.setenv("MOE_KG_FUSED_ONE_PASS", "0")
    a = call()
    monkeypatch.setenv("MOE_KG_FUSED_ONE_PASS", "1")
    b = call()
    return a, b


# every n, M, m = q + p, d and kernel of the issue's list at least once; n M m small enough for a fraction of a second each
CASES = [
    (5001, 255, 2, 1, 0, 127, 0),
    (5002, 257, 8, 2, 0, 129, 1),
    (5003, 513, 12, 4, 0, 300, 0),
    (5004, 255, 8, 3, 2, 129, 1),
    (5005, 257, 12, 4, 4, 127, 0),
    (5006, 513, 2, 5, 3, 300, 1),
    (5007, 257, 2, 2, 2, 300, 1),
    (5008, 513, 8, 1, 1, 127, 0),
    (5009, 255, 12, 1, 0, 300, 1),
]


@pytest.mark.parametrize("seed,n,d,q,p,M,cov", CASES, ids=["n%d-d%d-m%d-M%d-cov%d" % (c[1], c[2], c[3] + c[4], c[5], c[6]) for c in CASES])
def test_against_the_two_kernel_form(api, monkeypatch, seed, n, d, q, p, M, cov):
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=seed, n=n, d=d, q=q, M=M, P=6, derivs=(), p=p)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, (), cov_type=cov)
    best = float(G.additional_mean(w.discrete).min())
    Xp = w.Xp if p else None
    a, b = _both_forms(monkeypatch, lambda: G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals))
    assert G.last_kernel_info()["fused_tail"] == 1
    scale = max(float(np.abs(a["grad_sum"]).max()), abs(a["kg_sum"]))
    err = float(np.abs(a["grad_sum"] - b["grad_sum"]).max())
    print("grad_sum difference / scale %.2e" % (err / scale))
    assert a["kg_sum"] == b["kg_sum"]
    assert np.abs(a["grad_sum"]).max() > 0 and err <= 1e-12 * scale, err / scale


def test_alone_in_a_batch_and_at_another_position(api):
    """n = 300: two point blocks, the second holding the union rows; M = 200: two chunks; m = 5: the eight-wide instantiation."""
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=5020, n=300, d=5, q=3, M=200, P=7, derivs=(), p=2, num_restarts=3)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, ())
    best = float(G.additional_mean(w.discrete).min())
    args = (w.Xp, w.M, best, w.kg_normals)
    batch = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, *args)
    assert G.last_kernel_info()["fused_tail"] == 1
    order = [2, 0, 1]
    moved = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts[order], *args)
    assert np.abs(batch["grad_sum"]).max() > 0
    for e in range(3):
        one = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts[e], *args)
        assert one["kg_sum"] == batch["kg_sum"][e] and np.array_equal(one["grad_sum"], batch["grad_sum"][e]), e
        at = order.index(e)
        assert moved["kg_sum"][at] == batch["kg_sum"][e] and np.array_equal(moved["grad_sum"][at], batch["grad_sum"][e]), e


def test_two_mc_shards_add_up(api):
    """The samples dealt to two shards as dist.shard_samples deals them (even-aligned): ZC is formed per shard and the sums add up."""
    from cornell_moe_amd import dist as mdist
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=5030, n=257, d=8, q=4, M=300, P=6, derivs=(), p=1)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, ())
    best = float(G.additional_mean(w.discrete).min())
    args = (w.inner_gd, w.bounds, w.discrete, w.Xq, w.Xp, w.M, best, w.kg_normals)
    whole = G.kg(*args)
    assert G.last_kernel_info()["fused_tail"] == 1
    ks, gs = 0.0, np.zeros_like(whole["grad_sum"])
    for r in range(2):
        first, count = mdist.shard_samples(w.M, r, 2)
        assert first % 2 == 0 and count > 0
        part = G.kg(*args, first_sample=first, num_local=count)
        ks += part["kg_sum"]
        gs += part["grad_sum"]
    gscale = max(float(np.abs(whole["grad_sum"]).max()), abs(whole["kg_sum"]))
    err = float(np.abs(gs - whole["grad_sum"]).max())
    print("kg_sum rel. %.2e, grad_sum / scale %.2e" % (abs(ks - whole["kg_sum"]) / abs(whole["kg_sum"]), err / gscale))
    assert abs(ks - whole["kg_sum"]) <= 1e-12 * abs(whole["kg_sum"])
    assert np.abs(whole["grad_sum"]).max() > 0 and err <= 1e-12 * gscale


def _hard_input():
    """n = 200, d = 2, noise 1e-6 alpha; the point being sampled sits 0.9e-3 length scales from training point 17."""
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=5040, n=200, d=2, q=2, M=256, P=6, derivs=(), p=1)
    w.lengths = np.full(2, 0.1)   # (about the spacing of 200 points in the unit square: at the workload's 0.7 the posterior is pinned
    w.hyperparameters = np.concatenate([[w.alpha], w.lengths])   # everywhere and the gradient vanishes against KG itself)
    w.noise = np.full(1, 1.0e-6 * w.alpha)
    w.Xp = (w.X[17] + 0.9e-3 * w.lengths * np.array([0.6, 0.8])).reshape(1, 2)
    return w


def test_hard_conditioning_against_the_oracle(api, monkeypatch):
    """The posterior covariance between the union points and x* is far below the prior one (noise 1e-6 alpha, a point being sampled
    within 1e-3 length scales of a training point): the S_W-free form subtracts after the sum over the samples.  Both forms against
    the CPU oracle at the q-KG gradient's parity tolerance (helpers.TOL["grad_kg"], as test_gpu_parity.py applies it), and the
    S_W-free form's deviation no more than ten times the two-kernel form's (one reordered sum of M terms).  The input is first
    checked to be well inside the tolerance on the CPU: the posterior really is orders below the prior there, and where the
    unmodified reference is built it agrees with the oracle to a tenth of the tolerance."""
    from oracle import orc
    w = _hard_input()
    cov = 1
    O = orc.OrcGP(cov, w.alpha, w.lengths, w.X, w.y, w.noise, ())
    best = float(O.additional_mean(w.discrete).min())
    var_p = float(np.asarray(O.var(w.Xp)).reshape(-1)[0])
    assert 0.0 < var_p <= 1.0e-4 * w.alpha, var_p   # posterior variance at the point being sampled against the prior's alpha
    ro = O.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, w.Xp, w.M, best, w.kg_normals)
    scale = max(float(np.abs(ro["grad"]).max()), abs(ro["kg"]))
    assert np.all(np.isfinite(ro["grad"])) and np.abs(ro["grad"]).max() > 0
    R = reference_checker(cov, w.alpha, w.lengths, w.X, w.y, w.noise, ())
    if R is not None:
        rr = R.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, w.Xp, w.M, best, w.kg_normals)
        own = float(np.abs(rr["grad"] - ro["grad"]).max()) / scale
        print("oracle against the reference / scale %.2e" % own)
        assert own <= 0.1 * TOL["grad_kg"], own
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, (), cov_type=cov)
    a, b = _both_forms(monkeypatch, lambda: G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, w.Xp, w.M, best, w.kg_normals))
    assert G.last_kernel_info()["fused_tail"] == 1
    dev_two = float(np.abs(a["grad"] - ro["grad"]).max()) / scale
    dev_new = float(np.abs(b["grad"] - ro["grad"]).max()) / scale
    msg = "deviation from the oracle / scale: two-kernel form %.3e, S_W-free form %.3e" % (dev_two, dev_new)
    print(msg)
    assert a["kg_sum"] == b["kg_sum"], msg
    assert abs(b["kg"] - ro["kg"]) <= TOL["kg"] * abs(ro["kg"]), msg
    assert dev_two <= TOL["grad_kg"] and dev_new <= TOL["grad_kg"], msg
    assert dev_new <= 10.0 * dev_two, msg


def test_ensemble_wide_and_member_by_member(api):
    """One small KG-MCMC evaluation of three members with ensemble-wide launches against member-by-member launches: equal bits (the
    point kernel with its union rows and kg_zc_direct_kernel run as ensemble twins)."""
    from cornell_moe_amd.workloads import make_workload
    nm, E, d, q = 3, 2, 3, 3
    w = make_workload(seed=5050, n=70, d=d, q=q, M=160, P=8, derivs=(), p=2)
    rng = np.random.default_rng(5051)
    hypers = np.column_stack([w.alpha * rng.uniform(0.7, 1.4, nm)] + [w.lengths[k] * rng.uniform(0.6, 1.6, nm) for k in range(d)])
    noises = np.tile(np.asarray(w.noise, dtype=np.float64).reshape(1, -1), (nm, 1)) * rng.uniform(0.8, 1.2, (nm, 1))
    Xq_all = rng.uniform(0.05, 0.95, (E, q, d))
    disc = np.tile(w.discrete.reshape(1, -1), (nm, 1)) + 0.01 * rng.standard_normal((nm, w.discrete.size))
    best = rng.uniform(-1.0, 0.0, nm)
    G = api.DeviceGPMCMC(hypers, noises, w.X, w.y, ())
    try:
        api.set_ensemble_launches(0)
        k0, g0 = G.kg_batch(w.inner_gd, w.bounds, disc, Xq_all, w.Xp, w.M, best, w.kg_normals)
        api.set_ensemble_launches(1)
        s0 = api.ensemble_launch_stats()
        k1, g1 = G.kg_batch(w.inner_gd, w.bounds, disc, Xq_all, w.Xp, w.M, best, w.kg_normals)
        s1 = api.ensemble_launch_stats()
    finally:
        api.set_ensemble_launches(-1)
    assert all(gp.last_kernel_info()["fused_tail"] == 1 for gp in G.gps)
    assert s1[0] - s0[0] == 1 and s1[1] == s0[1], (s0, s1)   # (the members' chains lined up: one merged evaluation)
    assert np.all(np.isfinite(k0)) and np.abs(g0).max() > 0
    assert np.array_equal(k0, k1) and np.array_equal(g0, g1)
