"""The discretised one-point knowledge gradient with pending points on the device (csrc/kg1_pending.hip:
moe_kg_discrete_mcmc_pending, moe_kg_discrete_mcmc_multistart_pending, moe_kg_discrete_mcmc_suggest) against the long-double
restatement of tests/kg1_pending_reference.py, on the cases kg1_pending_reference.GPU_CASES, whose inputs
tests/test_kg1_pending_reference.py qualifies on the CPU (float64 within 2.5e-11 scale of long double, every decision margin
>= 1e-7, P moves a checked candidate's value by >= 1e-4 scale: a device that ignored P fails here).  Shapes: d in {2, 3, 4} with n up
to 130, A up to 4095 and up to 64 pending points; d in {16, 24, 32} at n = 20 (padded dimensions 16, 24, 32); n = 520 and 1030 (the
128- and 192-wide K slices of the split-K triangular products); ensembles, the ascent and the greedy batch also at d = 17 with a
fidelity coordinate and members of different N.

Tolerances: tests/test_gpu_kg1.py's -- |KG - want| <= 1e-10 scale, |grad KG - want|_inf <= 1e-10 max(1, |want|_inf), the number of
lines on the envelope exact.  Everything else is bit for bit: the new symbols with no pending point against their twins, a candidate
alone against itself inside a batch, duplicates in the set, the ascent against a host-driven loop over the evaluator
(tests/ms_restatement.py), the greedy batch against calls of the ascent fed their predecessors' points, ensemble-wide launches on
against off.  Every test prints the worst figures it saw (pytest -s); DESIGN.md section 5.15 records those of the first run."""
import ctypes as C

import numpy as np
import pytest

import kg1_opt_cases as kc
import kg1_pending_reference as kp
import kg1_reference as kr
import ms_restatement as ms
from cornell_moe_amd import _lib, api, knowledge_gradient_discrete

pytestmark = pytest.mark.gpu

LD = kr.LD
dp, ip = _lib.dp, _lib.ip


def _gp(p):
    return api.DeviceGP(p.hyper, p.X, p.y, p.noise, cov_type=p.case.cov_type)


def _close(gps):
    for g in gps:
        g.close()


class _Launches(object):
    """ensemble-wide launches switched on or off for a block, the environment's setting restored afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib.load().moe_set_ensemble_launches(1 if self.on else 0)

    def __exit__(self, *exc):
        _lib.load().moe_set_ensemble_launches(-1)
        return False


# ---- the new symbols called directly, so that num_being_sampled = 0 reaches them ----
def _raw_eval(gps, sets, points, bests, nf, pending):
    arr, E, d, keep, disc, counts, best = api._kg_discrete_members(gps, sets, bests, nf)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(pending, dtype=np.float64).reshape(-1, d)
    kg, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(_lib.load().moe_kg_discrete_mcmc_pending(
        arr, E, nf, disc.ctypes.data_as(dp), counts.ctypes.data_as(ip), best.ctypes.data_as(dp),
        pend.ctypes.data_as(dp) if len(pend) else None, len(pend), pts.ctypes.data_as(dp), len(pts), 1, kg.ctypes.data_as(dp),
        grad.ctypes.data_as(dp), C.byref(err)), err)
    return kg, grad


def _raw_ascent(gps, gd, bounds, sets, bests, starts, nf, pending, q=None):
    """moe_kg_discrete_mcmc_multistart_pending (q None: a dict shaped like api.kg_discrete_multistart's, path included) or
    moe_kg_discrete_mcmc_suggest (points [q][d], values [q], found [q])"""
    arr, E, d, keep, disc, counts, best = api._kg_discrete_members(gps, sets, bests, nf)
    g = api.DeviceGP._gd(gd)
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(pending, dtype=np.float64).reshape(-1, d)
    head = (arr, E, nf, C.byref(g), b.ctypes.data_as(dp), disc.ctypes.data_as(dp), counts.ctypes.data_as(ip), best.ctypes.data_as(dp),
            pend.ctypes.data_as(dp) if len(pend) else None, len(pend), st.ctypes.data_as(dp), len(st), 1)
    err = _lib.MoeError()
    if q is not None:
        points, values, found = np.zeros((q, d)), np.zeros(q), np.zeros(q, dtype=np.int32)
        api._check(_lib.load().moe_kg_discrete_mcmc_suggest(*(head + (q, points.ctypes.data_as(dp), values.ctypes.data_as(dp),
                                                                      found.ctypes.data_as(ip), C.byref(err)))), err)
        return points, values, found
    K, rows = min(len(st), 20), g.max_num_restarts * g.max_num_steps + 1
    point, vals, kept, ends = np.zeros(d), np.zeros(len(st)), np.zeros(K, dtype=np.int32), np.zeros((K, d))
    end_vals, steps, path = np.zeros(K), np.zeros(K, dtype=np.int32), np.zeros((K, rows, d))
    value, found = C.c_double(0.0), C.c_int(0)
    api._check(_lib.load().moe_kg_discrete_mcmc_multistart_pending(*(head + (
        point.ctypes.data_as(dp), C.byref(value), C.byref(found), vals.ctypes.data_as(dp), kept.ctypes.data_as(ip),
        ends.ctypes.data_as(dp), end_vals.ctypes.data_as(dp), path.ctypes.data_as(dp), steps.ctypes.data_as(ip), C.byref(err)))), err)
    return {"point": point, "value": value.value, "found": bool(found.value), "start_values": vals, "kept_index": kept,
            "end_points": ends, "end_values": end_vals, "steps_taken": steps, "path": path}


def _same_run(got, want):
    for key in ("start_values", "kept_index", "path", "steps_taken", "end_points", "end_values", "point"):
        assert np.array_equal(got[key], want[key]), key
    assert got["value"] == want["value"] and got["found"] == want["found"]


# ---- 1. value, gradient and the number of lines against long double ----
@pytest.mark.parametrize("case", kp.GPU_CASES, ids=lambda c: c.name)
def test_against_the_long_double_restatement(case):
    p, want, without = kp.expected(case)
    G = _gp(p)
    kg, grad, active = G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, want_active=True,
                                     points_being_sampled=p.pending)
    assert kg.shape == (case.C,) and grad.shape == (case.C, case.d) and np.all(np.isfinite(kg)) and np.all(np.isfinite(grad))
    e_v = max(abs(kg[i] - float(want[i].value)) / want[i].scale for i in p.checked)
    e_g = max(float(np.max(np.abs(grad[i] - want[i].grad.astype(np.float64)))) / max(1.0, float(np.max(np.abs(want[i].grad))))
              for i in p.checked)
    moved = max(abs(kg[i] - float(without[i])) / want[i].scale for i in p.checked)
    print("%s: value error %.3g scale, gradient error %.3g (bounds 1e-10); lines on the envelope %s; P moved KG by up to %.3g scale" % (
        case.name, e_v, e_g, sorted(set(int(active[i]) for i in p.checked)), moved))
    assert e_v <= 1e-10 and e_g <= 1e-10, (case.name, e_v, e_g)
    assert [int(active[i]) for i in p.checked] == [want[i].num_active for i in p.checked]
    # the value alone: the same kernels, the same bits; a candidate alone carries the bits it has inside the batch (two passes in the
    # last case, whose checked candidates lie on both sides of the pass boundary)
    assert np.array_equal(G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, want_grad=False,
                                        points_being_sampled=p.pending), kg)
    for i in (p.checked if case.C > 7 else (0, case.C - 1)):
        k1, g1, a1 = G.kg_discrete(p.discrete, p.points[i:i + 1], p.best, num_fidelity=case.nf, want_active=True,
                                   points_being_sampled=p.pending)
        assert k1[0] == kg[i] and np.array_equal(g1[0], grad[i]) and a1[0] == active[i], (case.name, i)
    G.close()


def test_the_straddled_pass_is_the_one_the_library_uses():
    case = kp.GPU_CASES[-1]
    per_pass = _lib.load().moe_kg1_pass_size(case.n, case.A)
    assert per_pass == 1024 and per_pass < case.C < 2 * per_pass
    assert set(kp.make_problem(case).checked) >= {per_pass - 1, per_pass}
    assert max(c.p for c in kp.GPU_CASES) == 64 and any(c.n >= 128 for c in kp.GPU_CASES)


def test_an_ensemble_of_three_against_long_double_launches_on_and_off():
    _ensemble_against_long_double(kp.ENSEMBLE)


def test_a_wide_ensemble_of_two_against_long_double_launches_on_and_off():
    """d = 17 with a fidelity coordinate (padded dimension 24), members of 12 and 20 sampled points"""
    _ensemble_against_long_double(kp.ENSEMBLE_WIDE)


def _ensemble_against_long_double(spec):
    ep = kp.make_ensemble(spec)
    want = kp.ensemble_expected(ep, ep.pending, LD)
    gps = [api.DeviceGP(ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], cov_type=ep.cov[k]) for k in range(len(ep.X))]
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(api.kg_discrete_ensemble(gps, ep.discrete, ep.points, ep.best, num_fidelity=ep.nf,
                                                 points_being_sampled=ep.pending))
    kg, grad = runs[0]
    assert np.array_equal(kg, runs[1][0]) and np.array_equal(grad, runs[1][1])
    e_v = max(abs(kg[i] - float(w[0])) / w[2] for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w[1].astype(np.float64)))) / max(1.0, float(np.max(np.abs(w[1])))) for i, w in enumerate(want))
    print("ensemble of %d, d = %d: value error %.3g of the members' mean scale, gradient error %.3g (bounds 1e-10)" % (
        len(gps), ep.points.shape[1], e_v, e_g))
    assert e_v <= 1e-10 and e_g <= 1e-10
    # the mean of the members' own calls, added in member order and divided once
    single = [g.kg_discrete(s, ep.points, b, num_fidelity=ep.nf, points_being_sampled=ep.pending)
              for g, s, b in zip(gps, ep.discrete, ep.best)]
    sum_kg, sum_grad = single[0][0], single[0][1]
    for one in single[1:]:
        sum_kg, sum_grad = sum_kg + one[0], sum_grad + one[1]
    assert np.array_equal(kg, sum_kg / len(gps))
    assert np.array_equal(grad, sum_grad / len(gps))
    _close(gps)


# ---- 2. no pending point: the twins, array for array ----
def test_without_pending_points_every_new_symbol_is_its_twin():
    case = kc.CASES[3]  # a fidelity coordinate, members of different N
    p = kc.make_problem(case)
    gps = [api.DeviceGP(p.hyper[e], p.X[e], p.y[e], p.noise[e], cov_type=case.cov[e]) for e in range(len(case.n))]
    none = np.zeros((0, case.d))
    kg, grad = api.kg_discrete_ensemble(gps, p.discrete, p.starts, p.best, num_fidelity=case.nf)
    kg2, grad2 = _raw_eval(gps, p.discrete, p.starts, p.best, case.nf, none)
    assert np.array_equal(kg, kg2) and np.array_equal(grad, grad2)
    want = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf, want_path=True)
    _same_run(_raw_ascent(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, case.nf, none), want)
    for q in (1, 3):  # (q = 3: room for two more rows under every column, none of them in use in round 0)
        points, values, found = _raw_ascent(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, case.nf, none, q=q)
        assert np.array_equal(points[0], want["point"]) and values[0] == want["value"] and bool(found[0]) == want["found"]
    # the Python layer takes the old symbols for None and for an empty array
    assert np.array_equal(api.kg_discrete_ensemble(gps, p.discrete, p.starts, p.best, num_fidelity=case.nf, points_being_sampled=none)[0], kg)
    assert np.array_equal(gps[0].kg_discrete(p.discrete[0], p.starts, p.best[0], num_fidelity=case.nf, points_being_sampled=None)[0],
                          gps[0].kg_discrete(p.discrete[0], p.starts, p.best[0], num_fidelity=case.nf)[0])
    _close(gps)


# ---- 3. duplicates in the set and the candidate itself, with pending points ----
@pytest.mark.parametrize("name", ["n20_d3_A12_p2_fid", "n12_d2_A129_p8", "n130_d3_A65_p3", "n20_d32_A12_p2_fid"])
def test_duplicates_and_the_candidate_itself_change_no_bit(name):
    case = [c for c in kp.GPU_CASES if c.name == name][0]
    p = kp.make_problem(case)
    G = _gp(p)
    kw = dict(num_fidelity=case.nf, want_active=True, points_being_sampled=p.pending)
    kg, grad, active = G.kg_discrete(p.discrete, p.points, p.best, **kw)
    size = case.d - case.nf
    dup = np.vstack([p.discrete[7:9], p.discrete, p.discrete[:3], p.discrete[-1:]])
    k2, g2, a2 = G.kg_discrete(dup, p.points, p.best, **kw)
    assert np.array_equal(k2, kg) and np.array_equal(a2, active)
    assert np.max(np.abs(g2 - grad)) <= 1e-12 * max(1.0, np.max(np.abs(grad)))
    for i in range(case.C):  # x^ of candidate i as a member of the set: its line is x^'s own, bit for bit, and drops out
        own = np.vstack([p.discrete[:5], p.points[i:i + 1, :size], p.discrete[5:]])
        k3, g3, a3 = G.kg_discrete(own, p.points[i:i + 1], p.best, **kw)
        assert k3[0] == kg[i] and a3[0] == active[i], i
        assert np.max(np.abs(g3[0] - grad[i])) <= 1e-12 * max(1.0, np.max(np.abs(grad))), i
    G.close()


# ---- 4. the ascent against the host-driven loop, the batch against calls of the ascent ----
def _host_loop(gps, p, pending):
    """ms_restatement's optimiser, evaluations by api.kg_discrete_ensemble with the pending points on the device, updates in numpy;
    a dict shaped like api.kg_discrete_multistart's, path included (a start that is not running repeats its point)"""
    case = p.case
    nf, d, T, R = case.nf, case.d, case.steps, case.restarts

    def value_fn(x):
        return api.kg_discrete_ensemble(gps, p.discrete, np.asarray(x).reshape(-1, d), p.best, num_fidelity=nf, want_grad=False,
                                        points_being_sampled=pending)

    seen, state = {}, {"round": -1, "points": None}

    def grad_fn(x):
        state["points"] = np.array(x, copy=True).reshape(-1, d)
        return api.kg_discrete_ensemble(gps, p.discrete, state["points"], p.best, num_fidelity=nf,
                                        points_being_sampled=pending)[1].reshape(np.shape(x))

    def on_step(i, idx):
        if i == 0:
            state["round"] += 1
        seen[state["round"] * T + i] = (np.array(idx), state["points"])

    vals = np.asarray(value_fn(p.starts))
    order = ms.top_k_order(vals)
    K = len(order)
    ends = ms.gradient_ascent(grad_fn, p.gd, p.bounds, p.starts[order], on_step=on_step)
    end_vals = np.asarray(value_fn(ends))
    point, value, found = p.starts[order[0]].copy(), -np.inf, False
    for s in range(K):
        if end_vals[s] > value:
            point, value, found = ends[s].copy(), float(end_vals[s]), True
    path = np.empty((K, R * T + 1, d))
    steps = np.zeros(K, dtype=int)
    for k in range(K):
        took = [(g, seen[g][1][list(seen[g][0]).index(k)]) for g in sorted(seen) if k in seen[g][0]]
        steps[k] = len(took)
        row = 0
        for g, before in took:  # rows up to g hold the point before step g
            path[k, row:g + 1] = before
            row = g + 1
        path[k, row:] = ends[k]
    return {"point": point, "value": value, "found": found, "start_values": vals, "kept_index": order, "end_points": ends,
            "end_values": end_vals, "steps_taken": steps, "path": path}


# d = 17 with a fidelity coordinate (padded dimension 24) and members of different N: the batch appends each pick to the pending list
# on the device as a padded row of dp coordinates
WIDE_BATCH = kc.Case("e2_n12_20_d17_fid_s8", 53, 17, 1, (12, 20), (12, 12), (kc.MATERN, kc.SE), 8, 6, 2, 1e-10, kc.MAX_REL)


def _opt_problem(name, num_pending):
    case = [c for c in kc.CASES + [WIDE_BATCH] if c.name == name][0]
    p = kc.make_problem(case)
    rng = np.random.default_rng(400 + num_pending)
    pending = rng.uniform(0.05, 0.95, size=(num_pending, case.d))
    pending[0] = p.starts[0] + rng.uniform(-0.05, 0.05, size=case.d)
    gps = [api.DeviceGP(p.hyper[e], p.X[e], p.y[e], p.noise[e], cov_type=case.cov[e]) for e in range(len(case.n))]
    return case, p, pending, gps


@pytest.mark.parametrize("name", ["e3_n12_d2_A12_s8_tight", "e3_n12_40_d3_fid_s48_loose", "e2_n20_d17_fid_s8"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(name):
    case, p, pending, gps = _opt_problem(name, 3)
    want = _host_loop(gps, p, pending)
    plain = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    for on in (True, False):
        with _Launches(on):
            got = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf, want_path=True,
                                             points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (name, on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("%s with 3 pending points: %d kept starts, steps taken %s, value %.12g" % (name, len(want["kept_index"]),
                                                                                   list(want["steps_taken"]), want["value"]))
    assert want["found"]
    _close(gps)


@pytest.mark.parametrize("name,num_pending", [("e3_n12_d2_A12_s8_tight", 0), ("e3_n12_40_d3_fid_s48_loose", 2),
                                              ("e2_n12_20_d17_fid_s8", 2)])
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit(name, num_pending):
    case, p, pending, gps = _opt_problem(name, max(num_pending, 1))
    pending = pending[:num_pending]
    q = 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points]) if (num_pending or t) else None
        res = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, num_fidelity=case.nf,
                                         points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = api.kg_discrete_suggest(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, q, num_fidelity=case.nf,
                                          points_being_sampled=pending if num_pending else None)
        assert np.array_equal(got["points"], np.array(want_points)), (name, on)
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    gaps = [float(np.min(np.linalg.norm(np.array(want_points)[:t] - want_points[t], axis=1))) for t in range(1, q)]
    print("%s, %d pending: greedy values %s, distance of each pick to the picks before it %s" % (name, num_pending, want_values, gaps))
    _close(gps)


# ---- 5. error returns ----
def test_a_pending_point_listed_twice_in_a_noise_free_member_is_singular():
    """alpha = 1e-3 and noise 0 in the second member; a pending point 0.05 from a sampled point, listed twice.  The second copy's Schur
    pivot is alpha - |v'|^2 = 0 in exact arithmetic and a few ulp of alpha (1e-19) in any floating-point order of the sums: the
    float64 restatement below gives |pivot| <= 1e-17, far under the pivot rule's 1e-16, while the first copy's is ~ 1e-5.  An
    error return with payload (member, index of the pending point in the combined list) -- not a fault."""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    # the extension restated in float64: v = L^-1 k(X, P), Schur complement of k(P, P) (noise 0), its Cholesky pivots
    m = kr.Model(kr.MATERN, hyper, X, y, [0.0], np.float64)
    V = np.linalg.solve(m.L, m.cov(X, pending))
    S = m.cov(pending, pending) - V.T @ V
    pivots = []
    Lp = np.zeros((4, 4))
    for j in range(4):
        for i in range(j):
            Lp[j, i] = (S[j, i] - Lp[j, :i] @ Lp[i, :i]) / Lp[i, i]
        pivots.append(S[j, j] - Lp[j, :j] @ Lp[j, :j])
        Lp[j, j] = np.sqrt(max(pivots[-1], 1e-300))
    print("Schur pivots of the four pending points in float64: %s" % pivots)
    assert min(pivots[:3]) > 1e-7 and abs(pivots[3]) <= 1e-17
    gps = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]
    sets = [rng.uniform(0, 1, size=(10, 2)), rng.uniform(0, 1, size=(7, 2))]
    bests = [float(y.min())] * 2
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, kc.GAMMA, kc.PRE_MULT, kc.MAX_REL, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.kg_discrete_ensemble(gps, sets, starts, bests, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 3) and "pending point 3" in str(e.value)
            with pytest.raises(api.SingularMatrixException) as e:
                api.kg_discrete_multistart(gps, gd, [[0, 1], [0, 1]], sets, bests, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (1, 3)
    ok = api.kg_discrete_ensemble(gps, sets, starts, bests, want_grad=False, points_being_sampled=pending[:3])  # (the handles still answer)
    assert np.all(np.isfinite(ok))
    _close(gps)


def test_the_limits_are_refused_and_the_handles_are_not_modified():
    case = kp.GPU_CASES[1]
    p = kp.make_problem(case)
    G = _gp(p)
    before = G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, want_active=True)
    rng = np.random.default_rng(8)
    with pytest.raises(api.BoundsException) as e:
        G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, points_being_sampled=rng.uniform(0, 1, size=(65, case.d)))
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 0.0, 64.0)
    gd = (4, 3, 1, 0, kc.GAMMA, kc.PRE_MULT, kc.MAX_REL, 1e-10)
    bounds = [[0.0, 1.0]] * case.d
    with pytest.raises(api.BoundsException) as e:
        api.kg_discrete_suggest(G, gd, bounds, [p.discrete], [p.best], p.points, 64, num_fidelity=case.nf, points_being_sampled=p.pending)
    assert (e.value.value, e.value.min, e.value.max) == (64.0, 1.0, 63.0)
    with pytest.raises(api.BoundsException) as e:
        api.kg_discrete_suggest(G, gd, bounds, [p.discrete], [p.best], p.points, 0, num_fidelity=case.nf)
    assert (e.value.value, e.value.min, e.value.max) == (0.0, 1.0, 65.0)
    with pytest.raises(api.BoundsException) as e:
        api.kg_discrete_multistart(G, gd, bounds, [p.discrete], [p.best], p.points, num_fidelity=case.d, points_being_sampled=p.pending)
    assert "num_fidelity" in str(e.value) and (e.value.value, e.value.max) == (float(case.d), float(case.d - 1))
    # calls that condition on pending points leave the GP as it was: the same arrays before and after
    G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, points_being_sampled=p.pending)
    api.kg_discrete_suggest(G, gd, bounds, [p.discrete], [p.best], p.points, 3, num_fidelity=case.nf, points_being_sampled=p.pending)
    after = G.kg_discrete(p.discrete, p.points, p.best, num_fidelity=case.nf, want_active=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    G.close()


# ---- 6. the wrapper ----
def test_the_wrapper_returns_a_batch_inside_the_bounds():
    case = kc.CASES[1]
    p = kc.make_problem(case)
    gps = [api.DeviceGP(p.hyper[e], p.X[e], p.y[e], p.noise[e], cov_type=case.cov[e]) for e in range(len(case.n))]
    pending = np.random.default_rng(12).uniform(0.1, 0.9, size=(2, case.d))
    points, values, found = knowledge_gradient_discrete.multistart_discrete_knowledge_gradient_optimization(
        gps, p.discrete, p.best, p.bounds, p.gd, 24, 31, num_fidelity=case.nf, num_to_sample=4, points_being_sampled=pending)
    assert points.shape == (4, case.d) and values.shape == (4,) and np.all(found)
    assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values))
    starts = api.latin_hypercube(31, p.bounds, 24)
    first = api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, starts, num_fidelity=case.nf, points_being_sampled=pending)
    assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
    one = knowledge_gradient_discrete.multistart_discrete_knowledge_gradient_optimization(
        gps, p.discrete, p.best, p.bounds, p.gd, 24, 31, num_fidelity=case.nf, points_being_sampled=pending)
    assert one[0].shape == (1, case.d) and np.array_equal(one[0][0], points[0])
    kgd = knowledge_gradient_discrete.DiscreteKnowledgeGradient(gps[0], p.discrete[0], num_fidelity=case.nf, best_so_far=p.best[0],
                                                                points_being_sampled=pending)
    assert np.array_equal(kgd.evaluate_at_point_list(starts),
                          gps[0].kg_discrete(p.discrete[0], starts, p.best[0], num_fidelity=case.nf, want_grad=False,
                                             points_being_sampled=pending))
    print("a batch of 4 with 2 pending points: values %s" % list(values))
    _close(gps)
