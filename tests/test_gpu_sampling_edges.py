"""Joint posterior sampling on the device (csrc/sample.hip) where tests/test_gpu_sampling.py does not reach: GPs of hundreds to
1500 observations (the split-K triangular products and the K-sliced Gram kernel with hundreds of columns per problem), candidate
sets of more than 256 points (several row blocks of the TRMV kernel, the strided loop of the finishing kernel), the draw counts on
either side of the TRMV / TRMM switch, more sets than one pass takes, singular sets inside a batch, exact ties, and a batch whose
set count times set size exceeds 65 535.

Two kinds of assertion:
 (a) forward: the device's values against tests/sampling_reference.py (np.longdouble; held to the reference's recorded results by
     tests/test_sampling_reference.py), |got - want| <= 1e-10 max(1, |want|) as tests/test_gpu_sampling.py::_assert_values, and the
     argmin wherever the two smallest reference values are more than 1e-8 sqrt(alpha) apart;
 (b) factor read-out: with unit vectors as normals a draw is mu + L[:, d] and its products are exact, so the device's own factor is
     read through the public entry point -- through the TRMM path (>= 8 unit vectors per call) and the TRMV path (<= 7) -- and random
     draws are then held to mu_dev + L_dev Z evaluated in extended precision within 64 C 2^-53 (|L_dev| |Z|) entry by entry: C fused
     multiply-adds per entry in any order, the factor 64 for the accumulation order on the matrix pipe and the final addition of
     mu.  That bound does not depend on the conditioning of the GP; a wrong row, a dropped k range or a missed last block breaks it by
     many orders of magnitude.

Every test prints what it observed (forward error, share of the read-out bound, seconds)."""
import time

import numpy as np
import pytest

import sampling_reference as sr
from cornell_moe_amd import api

pytestmark = pytest.mark.gpu

SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
U53 = 2.0 ** -53


def _took(t0, what):
    print("%s: %.2f s" % (what, time.perf_counter() - t0))


def _forward_error(got, want):
    """max of |got - want| / max(1, |want|): assertion (a) holds it to 1e-10."""
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _assert_argmin(argmin, want_values, alpha, what):
    """The reference's index wherever its two smallest values are further apart than 1e-8 sqrt(alpha); returns the exempted share."""
    exempt = 0
    for dd, v in enumerate(want_values):
        two = np.sort(v)[:2]
        if len(two) < 2 or two[1] - two[0] > 1e-8 * np.sqrt(alpha):
            assert argmin[dd] == sr.reference_argmin(v), (what, dd)
        else:
            exempt += 1
    return exempt / float(len(want_values))


def _problem(seed, n, d, length, cov_type, alpha=1.3, noise=1e-2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, size=(n, d))
    y = rng.normal(size=(n, 1))
    hyper = np.array([alpha] + [length] * d)
    G = api.DeviceGP(hyper, X, y, [noise], cov_type=cov_type)
    return rng, G, sr.Posterior(cov_type, hyper, X, y, [noise])


def _check_forward(G, P, pts, rng, draws, alpha, what):
    """assertion (a) for every draw count in `draws`"""
    C_ = pts.shape[0]
    mu, var = P.mu_var(pts)
    worst = 0.0
    for D in draws:
        z = rng.normal(size=(D, C_))
        want, _, rc, _ = sr.draws_from(mu, var, z)
        assert rc == 0, (what, rc)
        values, argmin, failed = G.sample_points(pts, z)
        assert failed == 0, (what, D, failed)
        err = _forward_error(values, want)
        worst = max(worst, err)
        assert err <= 1e-10, (what, D, err)
        _assert_argmin(argmin, want, alpha, what)
    return worst, mu, var


def _read_factor(G, pts, per_call):
    """The device's factor through unit normals, `per_call` of them per call: (mu_dev [C], raw [C][C] with raw[d, i] = mu_i + L[i, d])."""
    C_ = pts.shape[0]
    eye = np.eye(C_)
    raw = np.zeros((C_, C_))
    for d0 in range(0, C_, per_call):
        v, _, failed = G.sample_points(pts, eye[d0:d0 + per_call])
        assert failed == 0
        raw[d0:d0 + per_call] = v
    mu_dev, _, _ = G.sample_points(pts, np.zeros((1, C_)))
    return mu_dev[0], raw


def _assert_draws_follow_factor(G, pts, mu_dev, L_dev, z, what):
    """the random-Z half of (b): L_dev [row][col] in extended precision"""
    C_ = pts.shape[0]
    values, _, failed = G.sample_points(pts, z)
    assert failed == 0
    zl = z.astype(sr.LD)
    want = mu_dev.astype(sr.LD)[None, :] + zl @ L_dev.T
    bound = 64.0 * C_ * U53 * (np.abs(zl) @ np.abs(L_dev).T)
    ratio = float((np.abs(values.astype(sr.LD) - want) / bound).max())
    assert ratio <= 1.0, (what, z.shape[0], ratio)
    return ratio


# ---- 1. real GP sizes -------------------------------------------------------------------------------------------------------------
# launch_tri_gemm_cols: N < 128 the plain tiled kernel; N >= 128 with C <= 16 the skinny kernels, with C > 16 split-K on the matrix
# pipe.  gram_batch_slices = min(ceil(1024 / tiles), max(1, N / 64), 16) with tiles = t (t + 1) / 2, t = ceil(C / 32):
#   (600, 384): t = 12, tiles = 78, min(14, 9, 16) = 9      (1500, 300): t = 10, tiles = 55, min(19, 23, 16) = 16
#   (200, 513): t = 17, tiles = 153, min(7, 3, 16) = 3      C = 16 / 17: tiles = 1, N / 64 = 1 at N = 127 and 2 at N = 128, 129
#   C = 40: t = 2, tiles = 3, min(342, N / 64, 16) = 2 at N = 191 and 3 at N = 192 -- the pair below
_SIZES = [(600, 384, 4, 0.25), (1500, 300, 6, 0.3), (200, 513, 3, 0.15)]
_THRESHOLDS = [(n, c, 3, 0.2) for n in (127, 128, 129) for c in (16, 17)] + [(191, 40, 3, 0.2), (192, 40, 3, 0.2)]


@pytest.mark.parametrize("cov_type", [SE, MATERN])
@pytest.mark.parametrize("n,c,d,length", _SIZES + _THRESHOLDS)
def test_large_gp_draws_against_extended_reference(n, c, d, length, cov_type):
    t0 = time.perf_counter()
    rng, G, P = _problem(1000 * n + c, n, d, length, cov_type)
    pts = rng.uniform(0, 1, size=(c, d))
    what = "N = %d, C = %d, d = %d, cov %d" % (n, c, d, cov_type)
    worst, _, _ = _check_forward(G, P, pts, rng, (3, 9), 1.3, what)
    G.close()
    print("%s: forward error %.2e (bound 1e-10)" % (what, worst))
    _took(t0, what)


@pytest.mark.parametrize("cov_type", [SE, MATERN])
def test_factor_read_out_at_600_observations(cov_type):
    t0 = time.perf_counter()
    n, c, d, length = _SIZES[0]
    rng, G, P = _problem(1000 * n + c, n, d, length, cov_type)
    pts = rng.uniform(0, 1, size=(c, d))
    _, var = P.mu_var(pts)
    mu_mm, raw_mm = _read_factor(G, pts, c)     # every unit vector in one call: TRMM
    mu_mv, raw_mv = _read_factor(G, pts, 7)     # seven per call: TRMV, all its accumulators but one live
    assert mu_mm.tobytes() == mu_mv.tobytes()
    assert raw_mm.tobytes() == raw_mv.tobytes()
    above = np.tril_indices(c, -1)              # raw[d, i] with i < d is L[i, d], above the diagonal of L: the draw is mu itself
    assert np.array_equal(raw_mm[above], np.broadcast_to(mu_mm, (c, c))[above])
    L_dev = np.tril((raw_mm.astype(sr.LD) - mu_mm.astype(sr.LD)[None, :]).T)
    scale = float(np.abs(var).max())
    llt = float(np.abs(L_dev @ L_dev.T - var).max()) / scale
    print("N = %d, C = %d, cov %d: max |L L^T - Var_ref| / max |Var_ref| = %.2e (bound 1e-9)" % (n, c, cov_type, llt))
    assert llt <= 1e-9
    for D in (3, 9):
        ratio = _assert_draws_follow_factor(G, pts, mu_mm, L_dev, rng.normal(size=(D, c)), "read-out N = %d" % n)
        print("  D = %d: draws vs mu_dev + L_dev Z at %.3f of the 64 C 2^-53 |L||Z| bound" % (D, ratio))
    G.close()
    _took(t0, "factor read-out, cov %d" % cov_type)


# ---- 2. row blocks of the TRMV kernel, draw counts around the TRMV / TRMM switch ---------------------------------------------------
@pytest.mark.parametrize("c", [255, 256, 257, 512, 513])
def test_row_block_and_draw_count_edges(c):
    t0 = time.perf_counter()
    rng, G, P = _problem(77 + c, 30, 3, 0.2, MATERN)
    pts = rng.uniform(0, 1, size=(c, 3))
    mu_dev, raw = _read_factor(G, pts, c)
    L_dev = np.tril((raw.astype(sr.LD) - mu_dev.astype(sr.LD)[None, :]).T)
    mu, var = P.mu_var(pts)
    worst_f = worst_r = 0.0
    for D in (1, 7, 8, 9, 63, 65):
        z = rng.normal(size=(D, c))
        want, _, rc, _ = sr.draws_from(mu, var, z)
        assert rc == 0
        values, argmin, failed = G.sample_points(pts, z)
        assert failed == 0
        err = _forward_error(values, want)
        assert err <= 1e-10, (c, D, err)
        _assert_argmin(argmin, want, 1.3, (c, D))
        worst_f = max(worst_f, err)
        worst_r = max(worst_r, _assert_draws_follow_factor(G, pts, mu_dev, L_dev, z, "C = %d" % c))
    G.close()
    print("C = %d, N = 30: forward error %.2e (bound 1e-10), draws at %.3f of the read-out bound" % (c, worst_f, worst_r))
    _took(t0, "C = %d" % c)


# ---- 3. derivative observations at size -------------------------------------------------------------------------------------------
def test_draws_with_derivative_observations_at_900_rows():
    """N = 300 points with the derivatives (0, 2) observed (900 rows), C = 150: mu and Var of the function values from the unmodified
    reference when it is built, else from its C restatement; their factor and the draws in extended precision.  d = 4: the smallest
    pivot of Var is 2.4e-4 there (3e-6 at d = 3, where the reference and its restatement -- two double-precision evaluations of the
    same Var -- already give draws 2e-12 apart; 3e-13 here), so the 1e-10 bound measures the kernels, not the conditioning."""
    from cornell_moe_amd.workloads import make_workload
    from helpers import reference_checker
    from oracle import orc
    t0 = time.perf_counter()
    derivs, c = (0, 2), 150
    w = make_workload(seed=650, n=300, d=4, q=2, M=8, P=4, derivs=derivs)
    noise = np.maximum(w.noise, 1e-2)
    G = api.DeviceGP(w.hyperparameters, w.X, w.y, noise, derivs)
    R = reference_checker(1, w.alpha, w.lengths, w.X, w.y, noise, derivs) or orc.OrcGP(1, w.alpha, w.lengths, w.X, w.y, noise, derivs)
    rng = np.random.default_rng(651)
    pts = rng.uniform(0.02, 0.98, size=(c, 4))
    m = c * 3
    rows = np.arange(c) * 3                      # the function-value rows of the reference's [point][1 + g] layout
    var = np.asarray(R.var(pts)).reshape(m, m).T[np.ix_(rows, rows)]
    mu = np.asarray(R.mean(pts)).reshape(-1)
    mu = mu if mu.size == c else mu[rows]
    worst = 0.0
    for D in (3, 9):
        z = rng.normal(size=(D, c))
        want, _, rc, _ = sr.draws_from(mu, var, z)
        assert rc == 0
        values, argmin, failed = G.sample_points(pts, z)
        assert failed == 0
        err = _forward_error(values, want)
        worst = max(worst, err)
        assert err <= 1e-10, (D, err)
        _assert_argmin(argmin, want, float(w.alpha), D)
    G.close()
    print("N = 900 (300 points, 2 derivatives), C = 150: forward error %.2e (bound 1e-10)" % worst)
    _took(t0, "derivative observations")


# ---- 4. more sets than one pass takes ---------------------------------------------------------------------------------------------
def _tiny_alpha_gp(rng, n, d=3):
    """The singular construction of tools/make_golden_sampling.py: alpha = 1e-6, so that the pivot of an exactly repeated candidate
    (residue ~1e-22) fails the 1e-16 rule while the genuine pivots (1e-8 and up) pass."""
    X = rng.uniform(0, 1, size=(n, d))
    y = rng.normal(size=(n, 1)) * 1e-3
    hyper = np.array([1e-6, 0.15, 0.2, 0.12])
    return api.DeviceGP(hyper, X, y, [1e-8]), sr.Posterior(MATERN, hyper, X, y, [1e-8]), hyper


def _assert_sets_alone(G, cand, z, batch, which):
    pts_b, idx_b, fail_b = batch
    for e in which:
        pts_1, idx_1, fail_1 = G.sample_global_optima(cand[e:e + 1], z[e:e + 1])
        assert pts_1[0].tobytes() == pts_b[e].tobytes(), e
        assert idx_1[0] == idx_b[e] and fail_1[0] == fail_b[e], e


def _assert_optima(P, cand, z, batch, alpha, stop_at_failure=True):
    """index (and through it the point) of every set against the extended reference; returns the exempted share"""
    pts_b, idx_b, fail_b = batch
    exempt = 0
    for e in range(cand.shape[0]):
        want, _, rc, _ = P.draws(cand[e], z[e:e + 1], stop_at_failure)[:4]
        assert fail_b[e] == rc, (e, fail_b[e], rc)
        exempt += int(_assert_argmin(idx_b[e:e + 1], want, alpha, e) > 0)
        np.testing.assert_array_equal(pts_b[e], cand[e, max(int(idx_b[e]), 0)])
    return exempt / float(cand.shape[0])


def test_more_sets_than_one_pass():
    t0 = time.perf_counter()
    E, c = 2048 + 37, 5
    watch = (0, 1, 2047, 2048, 2049, E - 1)
    rng = np.random.default_rng(41)
    X = rng.uniform(0, 1, size=(40, 3))
    y = rng.normal(size=(40, 1))
    hyper = np.array([1.1, 0.3, 0.25, 0.35])
    G = api.DeviceGP(hyper, X, y, [1e-3])
    P = sr.Posterior(MATERN, hyper, X, y, [1e-3])
    cand = rng.uniform(0, 1, size=(E, c, 3))
    z = rng.normal(size=(E, c))
    t1 = time.perf_counter()
    batch = G.sample_global_optima(cand, z)
    t_batch = time.perf_counter() - t1
    assert not batch[2].any()
    _assert_sets_alone(G, cand, z, batch, watch)
    share = _assert_optima(P, cand, z, batch, 1.1)
    assert share <= 0.02
    G.close()
    print("E = %d sets of %d in two passes: %.3f s on the device (one covariance launch per set), near-ties exempted %.4f"
          % (E, c, t_batch, share))

    # the same with one singular set in the second pass
    G, P, hyper = _tiny_alpha_gp(rng, 40)
    bad = 2050
    cand_s = cand.copy()
    cand_s[bad, 3] = cand_s[bad, 1]
    healthy = G.sample_global_optima(cand, z)
    assert not healthy[2].any()
    batch = G.sample_global_optima(cand_s, z)
    want_failed = np.zeros(E, dtype=np.int32)
    want_failed[bad] = 4
    np.testing.assert_array_equal(batch[2], want_failed)
    others = np.arange(E) != bad
    assert batch[0][others].tobytes() == healthy[0][others].tobytes()
    assert np.array_equal(batch[1][others], healthy[1][others])
    _assert_sets_alone(G, cand_s, z, batch, watch + (bad,))
    share = _assert_optima(P, cand_s, z, batch, float(hyper[0]))
    assert share <= 0.02
    G.close()
    _took(t0, "more sets than one pass")


# ---- 5. failed sets inside a batch ------------------------------------------------------------------------------------------------
def test_failed_sets_inside_a_batch():
    t0 = time.perf_counter()
    E, c = 6, 100
    rng = np.random.default_rng(51)
    G, P, hyper = _tiny_alpha_gp(rng, 25)
    alpha = float(hyper[0])
    cand = rng.uniform(0, 1, size=(E, c, 3))
    cand[1, 80] = cand[1, 10]                   # fails at pivot 80: the second 64-block of the factorisation
    cand[4, 5] = cand[4, 2]                     # fails at pivot 5: the first block
    z = rng.normal(size=(E, c))
    want_failed = np.array([0, 81, 0, 0, 6, 0], dtype=np.int32)
    good = [0, 2, 3, 5]
    assert api.get_reference_quirks()
    try:
        for quirks in (1, 0):
            api.set_reference_quirks(quirks)
            stop = bool(quirks)
            batch = G.sample_global_optima(cand, z)
            np.testing.assert_array_equal(batch[2], want_failed)
            alone = G.sample_global_optima(cand[good], z[good])
            assert not alone[2].any()
            assert batch[0][good].tobytes() == alone[0].tobytes() and np.array_equal(batch[1][good], alone[1])
            _assert_optima(P, cand, z, batch, alpha, stop)
            worst = 0.0
            for e in range(E):
                # the batch's own draw through moe_gp_sample_points: the same kernels, so the same winner
                v1, a1, f1 = G.sample_points(cand[e], z[e:e + 1])
                assert f1 == want_failed[e] and a1[0] == batch[1][e], e
                mu, var = P.mu_var(cand[e])
                for D in (3, 9):                 # (9: the draws made again after the resumed factorisation take the TRMM path)
                    zz = rng.normal(size=(D, c))
                    want, _, rc, _ = sr.draws_from(mu, var, zz, stop)
                    values, argmin, failed = G.sample_points(cand[e], zz)
                    assert failed == rc == want_failed[e], (quirks, e, D, failed, rc)
                    err = _forward_error(values, want)
                    worst = max(worst, err)
                    assert err <= 1e-10, (quirks, e, D, err)
                    _assert_argmin(argmin, want, alpha, (quirks, e, D))
                    print("  quirks %d set %d D %d: |got - want| max %.2e (values ~%.1e)"
                          % (quirks, e, D, float(np.abs(values - want).max()), float(np.abs(want).max())))
            print("quirks = %d: forward error %.2e (bound 1e-10)" % (quirks, worst))
    finally:
        api.set_reference_quirks(1)
    G.close()
    _took(t0, "failed sets inside a batch")


# ---- 6. ties ----------------------------------------------------------------------------------------------------------------------
def test_ties_take_the_first_index():
    """320 candidates on a grid 40 length scales apart and as far from the data (square exponential): every cross covariance
    underflows, so Var = alpha I and mu = mean to the last bit and equal normals give equal values.  draw_finish_kernel handles
    candidate i in thread i mod 256: wavefront (i mod 256) / 64."""
    c = 320
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, size=(12, 2))
    G = api.DeviceGP([1.0, 0.05, 0.05], X, rng.normal(size=(12, 1)), [1e-2], cov_type=SE)
    grid = 5.0 + 2.0 * np.arange(18)            # 2.0 = 40 length scales; 18 x 18 >= 320
    cand = np.array([[a, b] for a in grid for b in grid])[:c]
    cases = [((3, 100), 3),                     # wavefronts 0 and 1
             ((3, 40), 3),                      # one wavefront
             ((3, 259), 3),                     # one lane, two trips of its loop
             ((70, 65, 300), 65),               # 300 sits in wavefront 0, the winner in wavefront 1
             ((0, 300), -1),
             (tuple(range(c)), -1)]
    z = np.zeros((len(cases), c))
    for k, (tied, _) in enumerate(cases):
        z[k, list(tied)] = -3.0
    values, argmin, failed = G.sample_points(cand, z)
    assert failed == 0
    for k, (tied, want) in enumerate(cases):
        # the precondition: the tied candidates share the minimum to the last bit
        assert all(values[k, i] == values[k, tied[0]] for i in tied), (k, values[k, list(tied)])
        assert values[k].min() == values[k, tied[0]]
        assert (values[k] == values[k].min()).sum() == len(tied)
        assert argmin[k] == want, (tied, argmin[k], want)
    # one draw per set through sample_global_optima (the TRMV path; six draws above took it too) and nine copies (TRMM)
    for k, (tied, want) in enumerate(cases):
        pts, index, _ = G.sample_global_optima(cand[None], z[k:k + 1])
        assert index[0] == want
        np.testing.assert_array_equal(pts[0], cand[max(want, 0)])
    v9, a9, _ = G.sample_points(cand, np.vstack([z, z[:3]]))
    assert np.array_equal(v9[:len(cases)], values)
    assert list(a9) == [w for _, w in cases] + [w for _, w in cases[:3]]
    G.close()


# ---- 7. a grid dimension that grows with the batch --------------------------------------------------------------------------------
def test_batch_with_more_than_65535_candidates():
    """N = 150, C = 40: the split-K triangular product adds its slices up with one grid row per candidate of a pass.  E = 1600
    (64 000 rows) is one pass; E = 1700 would be 68 000 rows, more than the 65 536 the device advertises for grid.y, so
    sample.hip's sets_per_pass(N, C) cuts it into passes of 65 535 / 40 = 1638 sets: set 1699 is then set 61 of the second pass."""
    rng = np.random.default_rng(71)
    n, c = 150, 40
    X = rng.uniform(0, 1, size=(n, 3))
    G = api.DeviceGP([1.3, 0.2, 0.2, 0.2], X, rng.normal(size=(n, 1)), [1e-2])
    for E in (1600, 1700):
        t0 = time.perf_counter()
        cand = rng.uniform(0, 1, size=(E, c, 3))
        z = rng.normal(size=(E, c))
        batch = G.sample_global_optima(cand, z)
        assert not batch[2].any()
        _assert_sets_alone(G, cand, z, batch, sorted({0, E // 2, min(1637, E - 1), min(1638, E - 1), E - 1}))
        assert len({tuple(p) for p in batch[0]}) > E // 2     # (the sets did get answers of their own)
        _took(t0, "E = %d sets of %d (E C = %d)" % (E, c, E * c))
    G.close()
