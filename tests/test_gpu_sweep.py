"""GPU parity sweep: seeded random configurations at the edges of the kernels' parameter space, each checked against the
plain-C oracle on the same normal table -- fidelity dimensions, points being sampled, tile-boundary point counts, odd MC
counts, both kernels, derivative observations on arbitrary dimensions, both MC kernel variants, many evaluations per
batch, gamma != 0, several restarts of the inner optimiser, MC shards."""
import os

import numpy as np
import pytest

from helpers import TOL, reference_checker

pytestmark = pytest.mark.gpu

CASES = [
    # seed, n, d, q, p, P, M, derivs, cov, num_fidelity, inner_gd
    (101, 60, 2, 1, 0, 3, 51, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),      # one tile, odd M
    (102, 64, 3, 2, 0, 4, 40, (), 0, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),      # n + u = 66: spills into a 2nd tile
    (103, 62, 3, 2, 0, 4, 40, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),      # n + u = 64 exactly
    (104, 130, 4, 2, 1, 6, 64, (), 1, 1, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),     # one fidelity dimension, p = 1
    (105, 90, 5, 3, 2, 5, 32, (), 0, 2, (1, 4, 2, 3, 0.5, 0.8, 0.3, 1e-8)),       # two fidelity dims, gamma != 0, 2 restarts
    (106, 80, 4, 2, 0, 5, 48, (2,), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),    # d-KG, one derivative on dim 2
    (107, 70, 4, 2, 1, 5, 36, (3, 0), 0, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # d-KG, derivatives listed out of order
    (108, 50, 5, 1, 1, 4, 24, (0, 1, 2, 4), 1, 0, (1, 5, 1, 3, 0.0, 1.0, 0.2, 1e-9)),  # four derivatives (all slots used)
    (109, 200, 8, 4, 0, 10, 100, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),   # headline shape, small
    (110, 40, 12, 2, 0, 6, 30, (0, 5, 11), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # d = 12 (C5's dimension), g = 3
    (111, 33, 16, 1, 0, 3, 20, (), 0, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),     # largest supported dimension
    # extremes of the parameter space
    (112, 1, 1, 1, 0, 1, 1, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),        # one training point, d = 1, ONE MC sample, P = 1
    (113, 3, 2, 1, 0, 1, 2, (), 0, 0, (1, 1, 1, 3, 0.0, 1.0, 0.1, 1e-10)),        # one antithetic pair, a single GD step
    (114, 45, 3, 16, 0, 4, 12, (0, 1, 2), 1, 0, (1, 3, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # m = (q+p)(1+g) = 64: the kernels' limit
    (115, 40, 3, 13, 3, 4, 12, (1, 2, 0), 0, 0, (1, 3, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # m = 64 with points being sampled
    (116, 30, 4, 2, 0, 5, 24, (), 1, 3, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),      # three of four dimensions are fidelities
    (117, 70, 3, 2, 0, 5, 30, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1.0)),        # loose tolerance: the inner GD stops at once
    (118, 70, 3, 2, 0, 5, 30, (), 0, 0, (1, 6, 3, 3, 1.0, 2.5, 1.0, 1e-12)),      # big steps against the walls, 3 restarts
    # more than four observed derivatives (r2: up to 12, the 8- and 12-slot instantiations of the workgroup-per-sample kernel)
    (119, 40, 8, 2, 0, 5, 24, (0, 1, 2, 4, 5, 7), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),          # g = 6 -> 8 slots
    (120, 30, 12, 4, 0, 6, 20, tuple(range(12)), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),           # g = 12: all of C5's dims
    (121, 36, 10, 2, 1, 4, 16, (9, 0, 3, 8, 1, 6, 2, 7, 5), 0, 0, (1, 5, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # g = 9, out of order, SE
    # more components than lanes, m = (q + p)(1 + g) in (64, 128]: thread-per-sample pre-pass + workgroup-per-sample kernel
    (122, 50, 12, 8, 0, 5, 16, tuple(range(12)), 1, 0, (1, 4, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # m = 104: q = 8, every C5 derivative
    (123, 40, 3, 30, 2, 4, 12, (0, 1, 2), 0, 0, (1, 3, 1, 3, 0.0, 1.0, 0.1, 1e-10)),         # m = 128: the limit, with p = 2
    (124, 70, 5, 10, 3, 6, 14, (4, 1, 0, 2), 1, 1, (1, 3, 1, 3, 0.0, 1.0, 0.1, 1e-10)),      # m = 65, one fidelity, 4 slots
    # d = 17 .. 32 (r2): the padded-dimension 24 and 32 instantiations, derivative slots {0, 4, 8, 12}
    (125, 60, 17, 2, 0, 5, 24, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),                  # d = 17 -> 24 rows, 7 padded
    (126, 50, 24, 2, 1, 4, 20, (3, 20), 0, 0, (1, 5, 1, 3, 0.0, 1.0, 0.1, 1e-10)),             # d = 24, g = 2 in 4 slots, SE
    (127, 70, 32, 3, 0, 5, 20, (), 1, 1, (1, 5, 1, 3, 0.0, 1.0, 0.1, 1e-10)),                  # d = 32: the limit, one fidelity
    (128, 40, 29, 2, 0, 4, 16, (0, 7, 15, 22, 28, 11), 1, 0, (1, 4, 1, 3, 0.0, 1.0, 0.1, 1e-10)),  # d = 29, g = 6 in 8 slots
    (129, 30, 20, 1, 0, 3, 12, tuple(range(12)), 0, 0, (1, 4, 1, 3, 0.0, 1.0, 0.1, 1e-10)),    # d = 20, g = 12
    (130, 200, 18, 2, 0, 6, 16, (5,), 1, 0, (1, 4, 1, 3, 0.0, 1.0, 0.1, 1e-10)),               # d = 18, 4 tiles, g = 1
    # beyond the LDS coordinate table (r2): the wave-per-sample kernel streams coordinates from L2, multi-trial passes in
    # direct-difference form; variant 1 = the workgroup-per-sample kernel on the same shape
    (131, 1700, 8, 2, 0, 5, 16, (), 1, 0, (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)),
]


def _mk(case):
    from cornell_moe_amd.workloads import make_workload
    seed, n, d, q, p, P, M, derivs, cov, f, gd = case
    w = make_workload(seed=seed, n=n, d=d, q=q, M=M, P=P, derivs=derivs, p=p)
    w.discrete = w.discrete[:, :d - f]
    w.bounds_inner = w.bounds[:2 * (d - f)]
    return w, cov, f, gd


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_kg_against_oracle(case, monkeypatch):
    from cornell_moe_amd import api
    from oracle import orc
    w, cov, f, gd = _mk(case)
    O = orc.OrcGP(cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
    full = np.hstack([w.discrete, np.ones((w.discrete.shape[0], f))])
    best = float(O.additional_mean(full).min())
    Xp = w.Xp if w.p else None
    ro = O.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f)
    # r4: the checker of KG, grad KG and the end points is the REFERENCE itself where oracle/_ref is built (it travels to the GPU box);
    # the restatement stays for the pass counts, which the reference does not expose
    R = reference_checker(cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
    rc = R.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f) if R is not None else ro
    scale = max(float(np.abs(rc["grad"]).max()), abs(rc["kg"]))
    ptol = 1e-8 if gd[1] * gd[2] <= 8 else 1e-6
    # both MC kernels, and the wave-per-sample kernel with the sample pre-pass off (beta / discretised-set scan in the kernel)
    # (r3: and the streamed-weights wave-per-sample kernel, variant 2, wherever it is built for the shape)
    for variant, prep in (("0", "1"), ("1", "1"), ("0", "0"), ("2", "1")):
        if (len(w.derivs) > 4 or (w.q + w.p) * (1 + len(w.derivs)) > 64) and variant == "0":
            continue  # more than four derivative slots / more than 64 components: not the LDS-slab wave-per-sample kernel
                      # (r4: the streamed-weights kernel takes 8 / 12 observed derivatives and m > 64 where every slot is observed)
        if w.d > 16 and prep == "0":
            continue  # (one wave-per-sample configuration is enough for the reduced instantiation set of d > 16)
        monkeypatch.setenv("MOE_KG_VARIANT", variant)
        monkeypatch.setenv("MOE_KG_PREP", prep)
        try:
            rg = G.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, want_best_points=True)
        except api.OptimalLearningException as e:
            if variant == "2" and "streamed-weights" in str(e):
                continue  # (d > 16 with 1 .. 3 observed derivatives: they occupy four slots, the table rows are not the weights)
            raise
        assert G.last_kernel_info()["variant"] == int(variant)
        assert abs(rg["kg"] - rc["kg"]) <= TOL["kg"] * max(abs(rc["kg"]), 1e-6), (variant, rg["kg"], rc["kg"])
        assert np.abs(rg["grad"] - rc["grad"]).max() <= TOL["grad_kg"] * max(scale, 1e-6), variant
        mism = np.abs(rg["best_point"] - rc["best_point"]).max(axis=1) > ptol
        assert mism.mean() <= 0.002, (variant, mism.mean())  # <= 0.2 % of the samples
        assert rg["grad_evals"] == ro["grad_evals"] and rg["mean_evals"] <= ro["mean_evals"]
        rv = G.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, want_grad=False)
        # (the same MC kernel on the same operands; the state set-up of the value-only call has fewer columns, and where that
        #  moves its L^-1 products from the MFMA GEMM to the tile GEMM the operands differ in the last bits)
        assert abs(rv["kg_sum"] - rg["kg_sum"]) <= 1e-13 * abs(rg["kg_sum"])
        # two even-aligned MC shards add up to the whole
        h = 2 * ((w.M // 2 + 1) // 2)
        if 0 < h < w.M:
            a = G.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, first_sample=0, num_local=h)
            b = G.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, first_sample=h,
                     num_local=w.M - h)
            assert abs(a["kg_sum"] + b["kg_sum"] - rg["kg_sum"]) <= 1e-11 * abs(rg["kg_sum"])
            gscale = max(np.abs(rg["grad_sum"]).max(), abs(rg["kg_sum"]))
            assert np.abs(a["grad_sum"] + b["grad_sum"] - rg["grad_sum"]).max() <= 1e-10 * gscale


def test_many_evaluations_per_batch(monkeypatch):
    """More evaluations than workgroups-per-evaluation slots: 300 point sets in one batch == 300 single calls (first few
    checked bitwise), for both MC kernel variants."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=120, n=50, d=2, q=2, M=16, P=4, derivs=(), num_restarts=300)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, ())
    best = float(G.additional_mean(w.discrete).min())
    for variant in ("0", "1"):
        monkeypatch.setenv("MOE_KG_VARIANT", variant)
        b = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, None, w.M, best, w.kg_normals)
        assert np.all(np.isfinite(b["kg_sum"])) and np.all(np.isfinite(b["grad_sum"]))
        for e in (0, 1, 255, 256, 299):
            one = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts[e], None, w.M, best, w.kg_normals)
            assert one["kg_sum"] == b["kg_sum"][e] and np.array_equal(one["grad_sum"], b["grad_sum"][e])
    # a batch beyond the device-workspace budget goes down in pieces (kg_evaluate_batch): same results, same counters
    monkeypatch.setenv("MOE_KG_BATCH_GB", "0")  # budget 0 -> one evaluation per piece
    w2 = make_workload(seed=121, n=40, d=3, q=2, M=12, P=4, derivs=(1,), num_restarts=7)
    G2 = api.DeviceGP(w2.hyperparameters, w2.X, w2.y, w2.noise, w2.derivs)
    best2 = float(G2.additional_mean(w2.discrete).min())
    pieces = G2.kg_batch(w2.inner_gd, w2.bounds, w2.discrete, w2.Xq_restarts, None, w2.M, best2, w2.kg_normals)
    monkeypatch.delenv("MOE_KG_BATCH_GB")
    whole = G2.kg_batch(w2.inner_gd, w2.bounds, w2.discrete, w2.Xq_restarts, None, w2.M, best2, w2.kg_normals)
    assert np.array_equal(pieces["kg_sum"], whole["kg_sum"]) and np.array_equal(pieces["grad_sum"], whole["grad_sum"])
    assert pieces["mean_evals"] == whole["mean_evals"] and pieces["grad_evals"] == whole["grad_evals"]


def test_batches_beyond_64_components_and_16_dimensions():
    """Batches through the paths that only exist beyond the old limits: m = (q + p)(1 + g) = 78 > 64 (thread-per-sample pre-pass,
    two-slot tail solve, chunked TB, the strided z c^T kernel) and d = 20 (padded dimension 24): every entry of a batch of three
    is the single evaluation to round-off, value-only calls agree, and two MC shards add up."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    for kwargs in (dict(seed=301, n=60, d=12, q=5, p=1, M=24, P=4, derivs=tuple(range(12))),   # m = 6 * 13 = 78
                   dict(seed=302, n=90, d=20, q=2, p=0, M=32, P=5, derivs=(3, 17))):            # d = 20, g = 2 in 4 slots
        w = make_workload(num_restarts=3, **kwargs)
        G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs)
        best = float(G.additional_mean(w.discrete).min())
        Xp = w.Xp if w.p else None
        b = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, Xp, w.M, best, w.kg_normals)
        assert np.all(np.isfinite(b["kg_sum"])) and np.all(np.isfinite(b["grad_sum"]))
        for e in range(3):
            one = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts[e], Xp, w.M, best, w.kg_normals)
            # (to round-off, not bit for bit: at these widths the state set-up of one evaluation and of three may cut their
            #  Gram sums into different numbers of K slices and take different GEMM kernels)
            assert abs(one["kg_sum"] - b["kg_sum"][e]) <= 1e-13 * abs(b["kg_sum"][e])
            assert np.abs(one["grad_sum"] - b["grad_sum"][e]).max() <= 1e-12 * max(np.abs(b["grad_sum"][e]).max(), abs(b["kg_sum"][e]))
        v = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, Xp, w.M, best, w.kg_normals, want_grad=False)
        assert np.abs(v["kg_sum"] - b["kg_sum"]).max() <= 1e-13 * np.abs(b["kg_sum"]).max()
        h = w.M // 2
        a1 = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts[1], Xp, w.M, best, w.kg_normals, first_sample=0, num_local=h)
        a2 = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts[1], Xp, w.M, best, w.kg_normals, first_sample=h, num_local=w.M - h)
        assert abs(a1["kg_sum"] + a2["kg_sum"] - b["kg_sum"][1]) <= 1e-11 * abs(b["kg_sum"][1])
        gs = max(np.abs(b["grad_sum"][1]).max(), abs(b["kg_sum"][1]))
        assert np.abs(a1["grad_sum"] + a2["grad_sum"] - b["grad_sum"][1]).max() <= 1e-10 * gs


def test_limit_update_decides_in_original_units(monkeypatch):
    """max_relative_change = 1 lets a step go to the wall itself: x + (upper - x) is exactly `upper` in the reference's units but can
    round one ulp past the wall's image in a centred, scaled frame -- and LimitUpdate then halves the step
    (gpp_domain.cpp:80-101).  The wave-per-sample kernel's line search evaluates in its frame but takes these decisions on an
    original-unit copy of the point; this is the case of tools/fuzz_parity.py (seed 101, case 93: domain offset by up to 1000,
    rescaled per dimension, 7 steps x 2 restarts) in which one of 59 samples went to another optimum before that."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    from oracle import orc
    rng = np.random.default_rng(101)
    for case in range(94):  # (replays the fuzzer's generator up to the case)
        d = int(rng.integers(1, 17))
        g = int(rng.integers(0, min(4, d) + 1)) if rng.uniform() < 0.5 else 0
        derivs = tuple(int(v) for v in rng.permutation(d)[:g])
        umax = 64 // (1 + g)
        q = int(rng.integers(1, min(4, umax) + 1))
        p = int(rng.integers(0, min(3, umax - q) + 1))
        n, P, M, cov = int(rng.integers(1, 300)), int(rng.integers(1, 13)), int(rng.integers(1, 65)), int(rng.integers(0, 2))
        f = int(rng.integers(0, d)) if rng.uniform() < 0.3 else 0
        gd = (1, int(rng.integers(1, 8)), int(rng.integers(1, 3)), 3, float(rng.choice([0.0, 0.5, 1.0])),
              float(rng.choice([1.0, 0.3, 2.0])), float(rng.choice([0.1, 0.5, 1.0])), float(rng.choice([1e-10, 1e-6])))
        affine = rng.uniform() < 0.4
        if affine:
            shift = rng.choice([-50.0, 10.0, 100.0, 1000.0], size=d) * (rng.uniform(size=d) < 0.7)
            scale = rng.choice([0.1, 1.0, 10.0], size=d)
    assert (n, d, q, p, derivs, M, gd[6], affine) == (211, 10, 3, 3, (7, 5), 59, 1.0, True)
    w = make_workload(seed=10_000 + 93, n=n, d=d, q=q, M=M, P=P, derivs=derivs, p=p)
    for name in ("X", "Xq", "Xp", "discrete"):
        setattr(w, name, shift + scale * getattr(w, name))
    lengths = w.lengths * scale
    bounds = np.column_stack([shift, shift + scale]).reshape(-1)
    O = orc.OrcGP(cov, w.alpha, lengths, w.X, w.y, w.noise, derivs)
    G = api.DeviceGP(np.r_[w.alpha, lengths], w.X, w.y, w.noise, derivs, cov_type=cov)
    best = float(O.additional_mean(w.discrete).min())
    ro = O.kg(gd, bounds, w.discrete, w.Xq, w.Xp, M, best, w.kg_normals)
    for variant in ("0", "1"):
        monkeypatch.setenv("MOE_KG_VARIANT", variant)
        rg = G.kg(gd, bounds, w.discrete, w.Xq, w.Xp, M, best, w.kg_normals, want_best_points=True)
        assert abs(rg["kg"] - ro["kg"]) <= TOL["kg"] * abs(ro["kg"]), (variant, rg["kg"], ro["kg"])
        assert np.abs(rg["best_point"] - ro["best_point"]).max() <= 1e-6


def test_wide_dimensions_gp_posterior_and_likelihood():
    """d = 17 .. 32 outside the KG kernels: posterior mean / variance and their gradients, q,p-EI, the log likelihood and its
    hyper-parameter gradient, against the oracle."""
    from cornell_moe_amd import api
    from oracle import orc
    rng = np.random.default_rng(77)
    for d, derivs, cov in ((17, (), 1), (24, (2, 19), 0), (32, (31,), 1), (27, (), 0)):
        n, g = 45, len(derivs)
        X = rng.uniform(size=(n, d))
        y = rng.normal(size=(n, 1 + g))
        lengths = rng.uniform(1.0, 2.5, size=d)
        noise = np.full(1 + g, 0.03)
        O = orc.OrcGP(cov, 1.3, lengths, X, y, noise, derivs)
        G = api.DeviceGP(np.r_[1.3, lengths], X, y, noise, derivs, cov_type=cov)
        pts = rng.uniform(size=(4, d))
        assert np.abs(G.mean(pts) - O.mean(pts)).max() <= 1e-10
        assert np.abs(G.grad_mean(pts) - O.grad_mean(pts)).max() <= 1e-9
        assert np.abs(G.variance(pts) - O.var(pts)).max() <= 1e-10
        assert np.abs(G.grad_cholesky_variance(pts, 2) - O.grad_chol_var(pts, 2)).max() <= 1e-8
        Mei = 40
        zn = rng.normal(size=(Mei, 4))
        eo, go = O.ei(pts[:3], pts[3:], Mei, float(np.median(y[:, 0])), zn)
        eg, gg = G.ei(pts[:3], pts[3:], Mei, float(np.median(y[:, 0])), zn)
        assert abs(eo - eg) <= TOL["ei"] * max(abs(eo), 1e-3)
        assert np.abs(gg - go).max() <= TOL["grad_ei"] * max(np.abs(go).max(), 1e-3)
        th = np.r_[1.3, lengths, noise]
        LL = api.LogLikelihood(X, y, derivs, cov_type=cov)
        vo = orc.log_likelihood(cov, th[0], lengths, X, y, noise, derivs)
        assert abs(LL.evaluate(th[None, :])[0] - vo) <= 1e-10 * max(1.0, abs(vo))
        if cov == 1 or g == 0:  # (the oracle restates the squared-exponential hyper-parameter gradient for g = 0 only)
            go = orc.log_likelihood_grad(cov, th[0], lengths, X, y, noise, derivs)
            assert np.abs(LL.grad(th) - go).max() <= 1e-8 * max(1.0, np.abs(go).max())
    with pytest.raises(api.BoundsException):  # d = 33
        api.DeviceGP(np.r_[1.0, np.ones(33)], rng.uniform(size=(5, 33)), rng.normal(size=(5, 1)), [0.1])


def test_ei_against_oracle_sweep():
    from cornell_moe_amd import api
    from oracle import orc
    for case in CASES[:6]:
        w, cov, f, gd = _mk(case)
        O = orc.OrcGP(cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
        G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
        Xp = w.Xp if w.p else None
        eb = float(np.median(w.y[:, 0]))
        R = reference_checker(cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
        eo, go = (R.ei(w.Xq, Xp, w.M, eb, w.ei_normals)[:2] if R is not None else O.ei(w.Xq, Xp, w.M, eb, w.ei_normals))
        eg, gg = G.ei(w.Xq, Xp, w.M, eb, w.ei_normals)
        assert abs(eo - eg) <= TOL["ei"] * max(abs(eo), 1e-3)
        assert np.abs(gg - go).max() <= TOL["grad_ei"] * max(np.abs(go).max(), 1e-3)


def test_ei_batch_matches_single_evaluations_and_oracle():
    """moe_ei_batch (EvaluateEIAtPointList, gpp_math.hpp:1900-1950): each entry is the single-evaluation result bit for bit
    (same kernels, same table), and agrees with the oracle."""
    from cornell_moe_amd import api
    from oracle import orc
    w, cov, f, gd = _mk(CASES[3])
    rng = np.random.default_rng(5)
    E = 9
    Xq_all = rng.uniform(0.05, 0.95, size=(E, w.q, w.d))
    O = orc.OrcGP(cov, w.alpha, w.lengths, w.X, w.y, w.noise, w.derivs)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
    eb = float(np.median(w.y[:, 0]))
    ei, grad = G.ei_batch(Xq_all, w.Xp, w.M, eb, w.ei_normals)
    ei_only, none = G.ei_batch(Xq_all, w.Xp, w.M, eb, w.ei_normals, want_grad=False)
    assert none is None and np.array_equal(ei_only, ei)
    for e in range(E):
        e1, g1 = G.ei(Xq_all[e], w.Xp, w.M, eb, w.ei_normals)
        assert e1 == ei[e] and np.array_equal(g1, grad[e])
        eo, go = O.ei(Xq_all[e], w.Xp, w.M, eb, w.ei_normals)
        assert abs(eo - ei[e]) <= TOL["ei"] * max(abs(eo), 1e-3)
        assert np.abs(grad[e] - go).max() <= TOL["grad_ei"] * max(np.abs(go).max(), 1e-3)


def test_limits_fail_loudly_and_ei_extremes():
    """Beyond the kernels' limits the C ABI reports BoundsException (never a silent fallback); at the limits q,p-EI still
    matches the oracle (u = q + p = 16, one MC sample; r6: u up to 64)."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    from oracle import orc
    w = make_workload(seed=130, n=40, d=3, q=33, M=8, P=3, derivs=(0, 1, 2))
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs)
    with pytest.raises(api.BoundsException):   # m = 33 * 4 = 132 > 128
        G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, None, w.M, 0.0, w.kg_normals)
    w65 = make_workload(seed=132, n=40, d=3, q=65, M=8, P=3, derivs=())
    with pytest.raises(api.BoundsException):   # u = 65 > 64
        G.ei(w65.Xq, None, w65.M, 0.0, w65.ei_normals)
    with pytest.raises(api.BoundsException):   # num_mc must be positive
        G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq[:2], None, 0, 0.0, w.kg_normals)
    with pytest.raises(api.BoundsException):   # num_fidelity must leave at least one free dimension
        G.kg(w.inner_gd, w.bounds[:0], w.discrete[:, :0], w.Xq[:2], None, w.M, 0.0, w.kg_normals, num_fidelity=3)
    with pytest.raises(api.BoundsException):   # thirteen observed derivatives: more slots than the MC kernels carry (12)
        w5 = make_workload(seed=131, n=20, d=13, q=1, M=8, P=3, derivs=tuple(range(13)))
        G5 = api.DeviceGP(w5.hyperparameters, w5.X, w5.y, w5.noise, w5.derivs)
        G5.kg(w5.inner_gd, w5.bounds, w5.discrete, w5.Xq, None, w5.M, 0.0, w5.kg_normals)
    # (r6: unions of 17 .. 64 points -- the MC kernel's 32- and 64-wide classes, the u x u algebra on the host)
    for q, p, M in ((16, 0, 1), (9, 7, 3), (1, 15, 64), (4, 16, 200), (17, 0, 50), (8, 24, 300), (33, 0, 64), (5, 59, 128)):
        w = make_workload(seed=140 + q, n=50 + 3 * p, d=3, q=q, M=M, P=3, derivs=(), p=p)
        O = orc.OrcGP(1, w.alpha, w.lengths, w.X, w.y, w.noise, ())
        G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, ())
        Xp = w.Xp if p else None
        eb = float(np.median(w.y[:, 0]))
        eo, go = O.ei(w.Xq, Xp, M, eb, w.ei_normals)
        eg, gg = G.ei(w.Xq, Xp, M, eb, w.ei_normals)
        assert abs(eo - eg) <= TOL["ei"] * max(abs(eo), 1e-3)
        assert np.abs(gg - go).max() <= TOL["grad_ei"] * max(np.abs(go).max(), 1e-3)


def test_fused_tail_matches_materialised_tail(monkeypatch):
    """The T-free gradient tail (q-KG: g = 0, m <= 8) against the path that materialises T = K(X, x*) in HBM: same gradient to
    rounding (the two differ only in summation order and in where 1/length is applied), for both kernels and m in {1..8}."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    for seed, n, d, q, p, cov in ((150, 333, 8, 4, 0, 1), (151, 130, 3, 1, 0, 0), (152, 257, 5, 5, 3, 1), (153, 64, 12, 2, 1, 0)):
        w = make_workload(seed=seed, n=n, d=d, q=q, M=300, P=6, derivs=(), p=p)
        G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, (), cov_type=cov)
        best = float(G.additional_mean(w.discrete).min())
        Xp = w.Xp if p else None
        monkeypatch.setenv("MOE_KG_FUSED_TAIL", "0")
        a = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals)
        monkeypatch.setenv("MOE_KG_FUSED_TAIL", "1")
        b = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals)
        assert a["kg_sum"] == b["kg_sum"]
        scale = max(np.abs(a["grad_sum"]).max(), abs(a["kg_sum"]))
        assert np.abs(a["grad_sum"] - b["grad_sum"]).max() <= 1e-11 * scale


def test_materialised_tail_beyond_48_kb_of_lds(monkeypatch):
    """The materialised tail with W^T T formed in kg_sw_kernel from W staged in LDS, N m 8 = 800 x 8 x 8 = 51 200 bytes: more than the
    48 KB a kernel may take without opting in, less than the 96 KB from which the driver forms W^T T by GEMM.  A single evaluation
    against the batch, ensemble-wide against member-by-member launches (the twin's opt-in against the per-member kernel's), and
    the T-free tail as the comparator at the neighbouring test's bound."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(n=800, d=2, q=8, p=0, M=64, P=6, derivs=(), num_restarts=3)
    assert w.X.shape[0] * w.q * 8 > 48 * 1024
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, ())
    best = float(G.additional_mean(w.discrete).min())
    monkeypatch.setenv("MOE_KG_FUSED_TAIL", "0")
    a = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, None, w.M, best, w.kg_normals)
    assert G.last_kernel_info()["fused_tail"] == 0
    batch = G.kg_batch(w.inner_gd, w.bounds, w.discrete, w.Xq_restarts, None, w.M, best, w.kg_normals)
    assert a["kg_sum"] == batch["kg_sum"][0] and np.array_equal(a["grad_sum"], batch["grad_sum"][0])
    # two members with the same hyper-parameters: their chains line up, every kernel of the tail runs as an ensemble twin
    hypers = np.tile(np.concatenate([[w.alpha], w.lengths]), (2, 1))
    noises = np.tile(np.asarray(w.noise, dtype=np.float64).reshape(1, -1), (2, 1))
    disc = np.tile(w.discrete.reshape(1, -1), (2, 1))
    Gm = api.DeviceGPMCMC(hypers, noises, w.X, w.y, ())
    bests = np.array([best, best])
    try:
        api.set_ensemble_launches(1)
        s0 = api.ensemble_launch_stats()
        k1, g1 = Gm.kg_batch(w.inner_gd, w.bounds, disc, w.Xq_restarts, None, w.M, bests, w.kg_normals)
        s1 = api.ensemble_launch_stats()
        api.set_ensemble_launches(0)
        k0, g0 = Gm.kg_batch(w.inner_gd, w.bounds, disc, w.Xq_restarts, None, w.M, bests, w.kg_normals)
    finally:
        api.set_ensemble_launches(-1)
    assert all(gp.last_kernel_info()["fused_tail"] == 0 for gp in Gm.gps)
    assert s1[0] > s0[0] and s1[1] == s0[1] and s1[2] > s0[2], (s0, s1)  # merged evaluations, no fall-back, launches they issued
    assert np.all(np.isfinite(k1)) and np.abs(g1).max() > 0
    assert np.array_equal(k0, k1) and np.array_equal(g0, g1)
    monkeypatch.setenv("MOE_KG_FUSED_TAIL", "1")
    b = G.kg(w.inner_gd, w.bounds, w.discrete, w.Xq, None, w.M, best, w.kg_normals)
    assert G.last_kernel_info()["fused_tail"] == 1
    assert a["kg_sum"] == b["kg_sum"]
    scale = max(np.abs(a["grad_sum"]).max(), abs(a["kg_sum"]))
    dev = np.abs(a["grad_sum"] - b["grad_sum"]).max()
    print("materialised against T-free tail at n = 800: max |d grad_sum| = %.3e, bound %.3e" % (dev, 1e-11 * scale))
    assert dev <= 1e-11 * scale


def test_one_pass_tail_matches_two_kernel_tail(monkeypatch):
    """r6: for m <= 4 and d <= 8 the T-free tail computes every entry of T once, for both of its contractions, in one kernel
    (kg_fused_pair_kernel) instead of once in each of two: same gradient to rounding (the partial sums of S_W and TB are taken in
    another order), for point counts on either side of a 256-point block, sample counts on either side of a 128-sample chunk,
    m in {1..4}, both kernels; and an evaluation's bits do not depend on the batch it is made in."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    for seed, n, d, q, p, M, cov in ((160, 1000, 8, 4, 0, 700, 1), (161, 257, 2, 2, 2, 129, 0), (162, 30, 2, 4, 0, 128, 1),
                                    (163, 600, 7, 3, 0, 500, 0), (164, 256, 4, 1, 0, 127, 1), (165, 513, 6, 1, 2, 384, 1)):
        w = make_workload(seed=seed, n=n, d=d, q=q, M=M, P=7, derivs=(), p=p)
        G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, (), cov_type=cov)
        best = float(G.additional_mean(w.discrete).min())
        Xp = w.Xp if p else None
        rng = np.random.default_rng(seed)
        Xq_all = np.concatenate([w.Xq[None], rng.uniform(0.05, 0.95, (2, q, d))])
        monkeypatch.setenv("MOE_KG_FUSED_ONE_PASS", "0")
        a = G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xq_all, Xp, w.M, best, w.kg_normals)
        monkeypatch.setenv("MOE_KG_FUSED_ONE_PASS", "1")
        b = G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xq_all, Xp, w.M, best, w.kg_normals)
        assert np.array_equal(a["kg_sum"], b["kg_sum"])
        scale = max(np.abs(a["grad_sum"]).max(), np.abs(a["kg_sum"]).max())
        assert np.abs(a["grad_sum"]).max() > 0 and np.abs(a["grad_sum"] - b["grad_sum"]).max() <= 1e-12 * scale, (n, d, q, p, M)
        one = G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xq_all[1:2], Xp, w.M, best, w.kg_normals)
        assert one["kg_sum"][0] == b["kg_sum"][1] and np.array_equal(one["grad_sum"][0], b["grad_sum"][1])


def test_offset_and_rescaled_domain():
    """The MC kernel takes squared distances as |x|^2 + |q|^2 - 2 x.q in a frame centred on the training-set mean: a domain far
    from the origin (x in [1000, 1001] and [-50, -40]) and anisotropic scales must not cost accuracy against the oracle,
    which works on the coordinates as given."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    from oracle import orc
    gd = (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)
    for n, d, q, M, derivs in ((600, 8, 4, 60, ()), (150, 6, 2, 40, (1, 4))):
        w = make_workload(seed=321 + n, n=n, d=d, q=q, M=M, P=8, derivs=derivs)
        shift = np.array([1000.0, -50.0, 0.0, 3.0e4, 10.0, -1.0, 100.0, 7.0])[:d]
        scale = np.array([1.0, 10.0, 0.1, 1.0, 100.0, 1.0, 0.01, 1.0])[:d]
        X, Xq, disc = (shift + scale * a for a in (w.X, w.Xq, w.discrete))
        lengths = w.lengths * scale
        bounds = np.column_stack([shift, shift + scale]).reshape(-1)
        O = orc.OrcGP(1, w.alpha, lengths, X, w.y, w.noise, derivs)
        G = api.DeviceGP(np.r_[w.alpha, lengths], X, w.y, w.noise, derivs)
        best = float(O.additional_mean(disc).min())
        ro = O.kg(gd, bounds, disc, Xq, None, M, best, w.kg_normals)
        gscale = np.abs(ro["grad"] * scale).max()  # gradients carry 1 / scale per dimension
        rg = G.kg(gd, bounds, disc, Xq, None, M, best, w.kg_normals, want_best_points=True)
        assert abs(rg["kg"] - ro["kg"]) <= TOL["kg"] * max(abs(ro["kg"]), 1e-6)
        assert np.abs((rg["grad"] - ro["grad"]) * scale).max() <= TOL["grad_kg"] * max(gscale, abs(ro["kg"]), 1e-6)
        assert rg["grad_evals"] == ro["grad_evals"]
        mism = np.abs((rg["best_point"] - ro["best_point"]) / scale).max(axis=1) > 1e-8
        assert mism.mean() <= 0.002


@pytest.mark.parametrize("cov", [0, 1])
def test_tiny_length_scales(cov):
    """Length scales of 1/500 of the domain: squared distances reach 1e6 length scales^2 and Armijo trial points (unclamped,
    step ~ gradient ~ 1 / length) land thousands of length scales outside the domain -- the table exp's 32-bit exponent
    arithmetic must not wrap (it did for the squared exponential: 0 weight x inf = NaN).  Beyond 1e5 length scales of
    extent the call is refused."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    from oracle import orc
    gd = (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)
    w = make_workload(seed=909 + cov, n=120, d=3, q=2, M=40, P=6)
    lengths = np.array([2e-3, 0.7, 5e-3])
    O = orc.OrcGP(cov, w.alpha, lengths, w.X, w.y, w.noise, ())
    G = api.DeviceGP(np.r_[w.alpha, lengths], w.X, w.y, w.noise, (), cov_type=cov)
    best = float(O.additional_mean(w.discrete).min())
    ro = O.kg(gd, w.bounds, w.discrete, w.Xq, None, w.M, best, w.kg_normals)
    for variant in ("0", "1"):
        os.environ["MOE_KG_VARIANT"] = variant
        try:
            rg = G.kg(gd, w.bounds, w.discrete, w.Xq, None, w.M, best, w.kg_normals)
        finally:
            os.environ.pop("MOE_KG_VARIANT", None)
        assert np.isfinite(rg["kg"]) and np.all(np.isfinite(rg["grad"]))
        assert abs(rg["kg"] - ro["kg"]) <= TOL["kg"] * max(abs(ro["kg"]), 1e-6)
        # gradients carry 1 / length, and at these scales an x* moved by 1e-10 moves them by 10 %: the reference and its
        # restatement differ by 4e-7 / 1.6e-7 (relative to KG) on this very case, so the bound here is 1e-6
        gscale = max(np.abs(ro["grad"] * lengths).max(), abs(ro["kg"]), 1e-6)
        assert np.abs((rg["grad"] - ro["grad"]) * lengths).max() <= 1e-6 * gscale
    bad = api.DeviceGP(np.r_[w.alpha, [1e-7, 0.7, 0.7]], w.X, w.y, w.noise, (), cov_type=cov)
    with pytest.raises(api.BoundsException):
        bad.kg(gd, w.bounds, w.discrete, w.Xq, None, w.M, 0.0, w.kg_normals)


def test_wide_frame_takes_direct_differences(monkeypatch):
    """a correlated point set spanning ~700 length scales (n = 500 on [0, 2000], length 3: neighbours
    1.3 length scales apart).  The |x|^2 + |q|^2 - 2 x.q distances of the LDS-table kernel carry eps (|x|^2 + |q|^2) ~ 5e-11 of
    absolute error in r^2 there; beyond a frame radius of 100 length scales the host selects the direct-difference kernels
    (kg.hip: wide_frame), which hold the 1e-8 parity; the error of the forced DOT path is printed next to it."""
    from cornell_moe_amd import api
    from oracle import orc
    rng = np.random.default_rng(77)
    n, q, M, P = 500, 2, 60, 6
    X = np.sort(rng.uniform(0.0, 2000.0, size=n))[:, None]
    y = (np.sin(X[:, 0] / 9.0) + 0.05 * rng.uniform(size=n))[:, None]
    lengths, noise = np.array([3.0]), np.array([0.01])
    bounds = np.array([0.0, 2000.0])
    Xq, disc = rng.uniform(0, 2000, size=(q, 1)), rng.uniform(0, 2000, size=(P, 1))
    Z = rng.standard_normal(((M + 1) // 2, q))
    gd = (1, 6, 1, 3, 0.0, 1.0, 0.1, 1e-10)
    O = orc.OrcGP(1, 1.0, lengths, X, y, noise, ())
    G = api.DeviceGP(np.r_[1.0, lengths], X, y, noise, ())
    best = float(O.additional_mean(disc).min())
    ro = O.kg(gd, bounds, disc, Xq, None, M, best, Z)
    scale = max(np.abs(ro["grad"] * lengths).max(), abs(ro["kg"]))
    errs = {}
    for label, radius2 in (("direct differences (default)", None), ("dot-product distances (forced)", "2000000000")):
        if radius2 is None:
            monkeypatch.delenv("MOE_KG_DOT_MAX_RADIUS2", raising=False)
        else:
            monkeypatch.setenv("MOE_KG_DOT_MAX_RADIUS2", radius2)
        rg = G.kg(gd, bounds, disc, Xq, None, M, best, Z)
        # (r4: the decision is visible to the caller -- moe_last_kernel_info, bit 1 of the second word)
        assert G.last_kernel_info()["far_frame"] == (1 if radius2 is None else 0)
        errs[label] = (abs(rg["kg"] - ro["kg"]) / abs(ro["kg"]), np.abs((rg["grad"] - ro["grad"]) * lengths).max() / scale)
        print("wide frame, %s: KG rel. error %.2e, grad KG rel. error %.2e" % ((label,) + errs[label]))
    e = errs["direct differences (default)"]
    assert e[0] <= TOL["kg"] and e[1] <= TOL["grad_kg"]


def test_randomised_parity_fuzz():
    """tools/fuzz_parity.py: 60 random shapes / kernels / derivative sets / fidelity dimensions / optimiser settings, q-KG (both
    MC kernels) and q-EI against the oracle -- no violation of the stated tolerances."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py")
    spec = importlib.util.spec_from_file_location("fuzz_parity", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run(60, 11) == 0


@pytest.mark.parametrize("case", [CASES[i] for i in (0, 3, 4, 5, 7, 8, 9, 10, 17)], ids=lambda c: str(c[0]))
def test_lane_kernel_bit_identical_to_frame_kernel(case, monkeypatch):
    """r5: the lane-parked wave-per-sample kernel (kg_mc_lane.hpp) against the frame line search it replaces (MOE_KG_LANE=0): every
    sum, every sample's end point and value, and both pass counters agree BIT FOR BIT -- the two take the row-order sums (|grad|^2,
    |step|^2, the trial line's three sums) in the same order over the same values; q-KG and d-KG, both covariances, fidelity
    dimensions, gamma != 0, several restarts, d = 12 / 16."""
    from cornell_moe_amd import api
    w, cov, f, gd = _mk(case)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
    full = np.hstack([w.discrete, np.ones((w.discrete.shape[0], f))])
    best = float(G.additional_mean(full).min())
    Xp = w.Xp if w.p else None
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    res = {}
    for lane in ("1", "0"):
        monkeypatch.setenv("MOE_KG_LANE", lane)
        res[lane] = G.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, want_best_points=True)
        info = G.last_kernel_info()
        # (one or two tiles at d <= 4: the lane-parked kernel for a call this small, else the 16-wavefront instantiation of the frame
        #  kernel -- case 101, test_small_shape_kernels_agree)
        assert info["variant"] == 0 and info["xlds"] == 1 and info["lane"] == (int(lane) if info["waves"] <= 8 else 0), info
    a, b = res["1"], res["0"]
    assert a["kg_sum"] == b["kg_sum"] and np.array_equal(a["grad_sum"], b["grad_sum"])
    assert np.array_equal(a["best_point"], b["best_point"])
    assert a["grad_evals"] == b["grad_evals"] and a["mean_evals"] == b["mean_evals"]


@pytest.mark.parametrize("case", [CASES[i] for i in (0, 1, 2, 11, 12, 15, 16, 17)], ids=lambda c: str(c[0]))
def test_small_shape_kernels_agree(case, monkeypatch):
    """r5: one or two tiles at d <= 4.  A call with few samples takes the lane-parked kernel (eight wavefronts, single-trial passes), a
    big one the 16-wavefront small-shape instantiation of the frame kernel (kg.hip: small_lane): which of the two runs depends on the
    SIZE of the call, so they must agree bit for bit -- sums, end points, pass counters."""
    from cornell_moe_amd import api
    w, cov, f, gd = _mk(case)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
    full = np.hstack([w.discrete, np.ones((w.discrete.shape[0], f))])
    best = float(G.additional_mean(full).min())
    Xp = w.Xp if w.p else None
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    res = {}
    for cap in ("8192", "0"):
        monkeypatch.setenv("MOE_KG_SMALL_LANE_MAX_SAMPLES", cap)
        res[cap] = G.kg(gd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, want_best_points=True)
        info = G.last_kernel_info()
        assert info["variant"] == 0 and info["xlds"] == 1, info
        assert (info["lane"], info["waves"]) == ((1, 8) if cap == "8192" else (0, 16)), info
    a, b = res["8192"], res["0"]
    assert a["kg_sum"] == b["kg_sum"] and np.array_equal(a["grad_sum"], b["grad_sum"])
    assert np.array_equal(a["best_point"], b["best_point"])
    assert a["grad_evals"] == b["grad_evals"] and a["mean_evals"] == b["mean_evals"]


@pytest.mark.parametrize("case", [CASES[i] for i in (0, 1, 2, 11, 12, 15, 16, 17)], ids=lambda c: str(c[0]))
def test_small_shape_exact_multi_trial_passes_agree(case, monkeypatch):
    """r6: the small shapes on the lane-parked kernel take several Armijo trials per sweep, each computed exactly as a single-trial pass
    computes it (kg_mc.hpp eval_multi_exact) -- against one trial per pass (MOE_KG_SMALL_MULTI=0, the r5 form): sums, end points and
    pass counters bit for bit, with the tensor-product and the simplex inner domain."""
    from cornell_moe_amd import api
    w, cov, f, gd = _mk(case)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, cov_type=cov)
    full = np.hstack([w.discrete, np.ones((w.discrete.shape[0], f))])
    best = float(G.additional_mean(full).min())
    Xp = w.Xp if w.p else None
    monkeypatch.setenv("MOE_KG_VARIANT", "0")
    monkeypatch.setenv("MOE_KG_SMALL_LANE_MAX_SAMPLES", "8192")
    for domain in (0, 1):
        if domain == 1 and w.d - f < 2:
            continue
        gdd = tuple(gd[:8]) + (domain,)
        res = {}
        for multi in ("1", "0"):
            monkeypatch.setenv("MOE_KG_SMALL_MULTI", multi)
            try:
                res[multi] = G.kg(gdd, w.bounds_inner, w.discrete, w.Xq, Xp, w.M, best, w.kg_normals, num_fidelity=f, want_best_points=True)
            except api.OptimalLearningException as e:
                assert domain == 1 and "EMPTY" in str(e)   # (a box outside the simplex: the reference's exception, either way)
                res = None
                break
            info = G.last_kernel_info()
            assert info["variant"] == 0 and info["lane"] == 1, info
        if res is None:
            continue
        a, b = res["1"], res["0"]
        assert a["kg_sum"] == b["kg_sum"] and np.array_equal(a["grad_sum"], b["grad_sum"]), domain
        assert np.array_equal(a["best_point"], b["best_point"]), domain
        assert a["grad_evals"] == b["grad_evals"] and a["mean_evals"] == b["mean_evals"], domain


def test_skinny_triangular_products_do_not_depend_on_the_column_grouping(monkeypatch):
    """r6: the skinny triangular products (L^-1 / L^-T on the few columns of K* per evaluation) take their columns 4, 8 or 16 per
    workgroup by the size of the CALL; a column's arithmetic must not depend on it -- a batch of KG evaluations on a GP of several
    hundred points, bit for bit under the three groupings, and equal to the evaluations made one at a time."""
    from cornell_moe_amd import api
    from cornell_moe_amd.workloads import make_workload
    w = make_workload(seed=91, n=700, d=6, q=3, M=64, P=8, p=1)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs)
    rng = np.random.default_rng(5)
    Xq_all = rng.uniform(0.05, 0.95, (7, w.q, w.d))
    best = float(G.additional_mean(w.discrete).min())
    res = {}
    for cb in ("4", "8", "16", "", "one column of the factor per wavefront"):
        monkeypatch.setenv("MOE_TRI_SKINNY_CB", cb if len(cb) <= 2 else "")
        monkeypatch.setenv("MOE_TRI_SKINNY_TJ", "1" if len(cb) > 2 else "")
        res[cb] = G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xq_all, w.Xp, w.M, best, w.kg_normals)
    monkeypatch.setenv("MOE_TRI_SKINNY_TJ", "")
    for cb in ("8", "16", "", "one column of the factor per wavefront"):
        assert np.array_equal(res["4"]["kg_sum"], res[cb]["kg_sum"]) and np.array_equal(res["4"]["grad_sum"], res[cb]["grad_sum"]), cb
    assert np.all(np.isfinite(res[""]["kg_sum"])) and np.abs(res[""]["grad_sum"]).max() > 0
    monkeypatch.setenv("MOE_TRI_SKINNY_CB", "")
    for e in range(3):
        one = G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xq_all[e:e + 1], w.Xp, w.M, best, w.kg_normals)
        assert one["kg_sum"][0] == res[""]["kg_sum"][e] and np.array_equal(one["grad_sum"][0], res[""]["grad_sum"][e])
