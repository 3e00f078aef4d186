"""The three-objective expected hypervolume improvement on the device (csrc/ehvi3.hip: moe_ehvi3_mcmc, moe_ehvi3_mcmc_multistart,
moe_ehvi3_mcmc_suggest) against the long-double restatement of tests/ehvi3_reference.py, on the cases ehvi3_reference.CASES,
BELIEVED, BELIEVED_WIDE, FULL and MANY, which tests/test_ehvi3_reference.py checks on the CPU (box counts, the branches of the
believed-front rule, values and gradients far above the bound here, the front and the pending points each moving the value, each
limit case reaching the branch it is there for).

Tolerances: |value - want| and |A_e - want| <= max(1e-10, 4 ld_diff) scale, the gradient likewise as tests/test_gpu_ehvi.py applies
it.  Everything else is bit for bit: value-only against value + gradient, a candidate alone against itself in a batch and across
the pass boundary, the value against the mean of the members' values formed on the host, an empty pending array against NULL,
ensemble-wide launches on against off, the empty front against the product of three analytic expected improvements, the ascent
against a host-driven loop over the evaluator (at d = 3 and at the padded dimension 24), the greedy batch against calls of the ascent
fed their predecessors' points.  The limits run: a member of 256 points and 33 153 boxes, reached through the pending points and
through a greedy pick; 341 members; sampled points of noise-free GPs, where the variance floors decide.  Every
test prints the worst figures it saw (pytest -s); DESIGN.md section 5.23 records those of the first run."""
import ctypes as C
import time

import numpy as np
import pytest

import ehvi3_reference as h3
import kg1_reference as kr
import test_ehvi3_reference as t3
import test_gpu_cei1 as tc
from cornell_moe_amd import _lib, api, expected_hypervolume_improvement as ehvi

pytestmark = pytest.mark.gpu

LD = h3.LD
dp, ip = _lib.dp, _lib.ip
_Launches, _host_loop, _same_run = tc._Launches, tc._host_loop, tc._same_run

# (BELIEVED_WIDE: the front kernel past lane stride 0; FULL: a member of 256 points and 33 153 boxes with member 1's table behind it)
CASES = h3.CASES + [h3.BELIEVED, h3.BELIEVED_WIDE, h3.FULL]


class _Device(object):
    """the GPs of a problem on the device: objs[k] [E], objective k + 1"""

    def __init__(self, p):
        self.all = [[api.DeviceGP(g.hyper, g.X, g.y, g.noise, [], cov_type=g.cov_type) for g in row] for row in p.gps]
        self.objs = [[row[k] for row in self.all] for k in range(3)]

    def close(self):
        for row in self.all:
            for g in row:
                g.close()


def _eval(D, p, points, pending="problem", front="problem", **kw):
    pending = p.pending if isinstance(pending, str) else pending
    front = p.front if isinstance(front, str) else front
    return api.ehvi3_ensemble(D.objs[0], D.objs[1], D.objs[2], p.ref, front, points, points_being_sampled=pending, **kw)


def _multistart(D, p, front, gd, bounds, starts, **kw):
    return api.ehvi3_multistart(D.objs[0], D.objs[1], D.objs[2], p.ref, front, gd, bounds, starts, **kw)


def _suggest(D, p, front, gd, bounds, starts, q, **kw):
    return api.ehvi3_suggest(D.objs[0], D.objs[1], D.objs[2], p.ref, front, gd, bounds, starts, q, **kw)


def _raw_eval(D, p, points, pending):
    """moe_ehvi3_mcmc called directly: an empty `pending` reaches it with num_being_sampled = 0 and a non-NULL array"""
    arrs, E, d, keep, ref, fr, F = api._ehvi3_members(D.objs[0], D.objs[1], D.objs[2], p.ref, p.front)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    pend = np.ascontiguousarray(np.vstack([np.reshape(pending, (-1, d)), np.zeros((1, d))]))  # (never NULL)
    value, grad = np.zeros(len(pts)), np.zeros((len(pts), d))
    err = _lib.MoeError()
    api._check(_lib.load().moe_ehvi3_mcmc(arrs[0], arrs[1], arrs[2], E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F,
                                          pend.ctypes.data_as(dp), pend.shape[0] - 1, pts.ctypes.data_as(dp), len(pts), 1,
                                          value.ctypes.data_as(dp), grad.ctypes.data_as(dp), None, C.byref(err)), err)
    return value, grad


def _errors(value, grad, members, want):
    e_v = max(abs(value[i] - float(w.value)) / w.scale for i, w in enumerate(want))
    e_g = max(float(np.max(np.abs(grad[i] - w.grad.astype(np.float64)))) / min(w.scale, max(1.0, float(np.max(np.abs(w.grad)))))
              for i, w in enumerate(want))
    e_m = max(abs(members[e, i] - float(a)) / w.scale for i, w in enumerate(want) for e, a in enumerate(w.members))
    return e_v, e_g, e_m


def _host_mean(members):
    """the documented rule on the host: the members added in member order, divided once"""
    E, n = members.shape
    out = np.zeros(n)
    for i in range(n):
        total = float(members[0, i])
        for e in range(1, E):
            total = total + float(members[e, i])
        out[i] = total / float(E)
    return out


# ---- 1. value, gradient and the members' values against long double; the bits of one call ----
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_against_the_long_double_restatement(case):
    p, want = h3.expected(case, LD)
    D = _Device(p)
    C_, d = p.points.shape
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_member_values=True))
    value, grad, members = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert value.shape == (C_,) and grad.shape == (C_, d) and members.shape == (case.E, C_)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(grad)) and np.all(members >= 0.0) and np.all(value >= 0.0)
    bound = max(1e-10, 4.0 * case.ld_diff)
    e_v, e_g, e_m = _errors(value, grad, members, want)
    print("%s: value error %.3g scale, gradient error %.3g, members' error %.3g scale (bound %.3g)" % (case.name, e_v, e_g, e_m, bound))
    assert e_v <= bound and e_g <= bound and e_m <= bound, (case.name, e_v, e_g, e_m)
    # the call's value is the mean of its own members' values formed on the host, bit for bit
    assert np.array_equal(value, _host_mean(members))
    # the value alone: the same bits; a candidate alone carries the bits it has inside the batch
    assert np.array_equal(_eval(D, p, p.points, want_grad=False), value)
    for i in (0, C_ - 1):
        v1, g1, m1 = _eval(D, p, p.points[i:i + 1], want_member_values=True)
        assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]) and np.array_equal(m1[:, 0], members[:, i]), (case.name, i)
    # no pending point through the symbol's pending arguments against NULL
    raw = _raw_eval(D, p, p.points, p.pending[:0])
    none = _eval(D, p, p.points, pending=None)
    assert np.array_equal(raw[0], none[0]) and np.array_equal(raw[1], none[1])
    if len(p.pending):
        assert not np.array_equal(none[0], value)
    if len(p.front):
        assert not np.array_equal(_eval(D, p, p.points, front=None, want_grad=False), value)
    D.close()


# ---- 2. an empty front and one member: the product of three analytic expected improvements, exactly ----
def test_with_an_empty_front_it_is_the_product_of_three_expected_improvements_exactly():
    p = h3.make_problem(h3.case("e1_d3_n20_p3_f1"))
    D = _Device(p)
    v, g, m = _eval(D, p, p.points, pending=None, front=None, want_member_values=True)
    ei = [api.ei_analytic_ensemble(D.objs[k], p.points, [p.ref[k]], want_grad=False) for k in range(3)]
    want = (ei[0] * ei[1]) * ei[2]
    print("F = 0, E = 1: value - (EI_1 EI_2) EI_3 at most %.3g; the smallest value %.3g" % (float(np.max(np.abs(v - want))), float(np.min(v))))
    assert np.array_equal(v, want) and np.array_equal(m[0], want) and float(np.min(v)) > 1e-3
    # (the believed outcomes are a front of their own)
    assert not np.array_equal(_eval(D, p, p.points, front=None, want_grad=False), v)
    D.close()


# ---- 3. a front flat in the third objective, through the two-objective device path ----
def test_a_front_flat_in_the_third_objective_agrees_with_the_two_objective_path():
    p = h3.make_problem(h3.case(h3.FLAT))
    assert len(p.pending) == 0 and len(p.front) == 12
    D = _Device(p)
    w_star = float(p.front[0, 2])
    v = _eval(D, p, p.points, want_grad=False)
    ei1 = api.ei_analytic_ensemble(D.objs[0], p.points, [p.ref[0]], want_grad=False)
    ei2 = api.ei_analytic_ensemble(D.objs[1], p.points, [p.ref[1]], want_grad=False)
    psi3_star = api.ei_analytic_ensemble(D.objs[2], p.points, [w_star], want_grad=False)
    psi3_r = api.ei_analytic_ensemble(D.objs[2], p.points, [p.ref[2]], want_grad=False)
    two = api.ehvi_ensemble(D.objs[0], D.objs[1], p.ref[:2], p.front[:, :2], p.points, want_grad=False)
    want = psi3_star * ei1 * ei2 + (psi3_r - psi3_star) * two
    scale = h3.member_scale(p.gps[0], p.ref)
    worst = float(np.max(np.abs(v - want))) / scale
    print("flat front, F = 12: value - identity through moe_ehvi_mcmc and moe_ei_analytic_mcmc %.3g scale (bound 1e-10)" % worst)
    assert worst <= 1e-10 and float(np.min(v)) > 1e-3
    D.close()


# ---- 4. across the pass boundary ----
_N8 = h3.Case("e1_d2_n8_p2_f5_two_passes", 44, 1, 2, ((8, 8, 8),), 2, 5, "random", None, 4100, 0.0)


def test_a_candidate_carries_its_bits_across_the_pass_boundary():
    per_pass = _lib.load().moe_ei1_pass_size(8)
    assert per_pass == 4096 and _N8.C == per_pass + 4
    p = h3.make_problem(_N8)
    checked = (0, per_pass - 1, per_pass, _N8.C - 1)
    ref_members = h3.ensemble(p, LD)
    D = _Device(p)
    for pending in (p.pending, None):
        value, grad, members = _eval(D, p, p.points, pending=pending, want_member_values=True)
        assert np.array_equal(_eval(D, p, p.points, pending=pending, want_grad=False), value)
        assert np.array_equal(value, _host_mean(members)) and np.all(value >= 0.0)
        for i in checked:
            v1, g1 = _eval(D, p, p.points[i:i + 1], pending=pending)
            assert v1[0] == value[i] and np.array_equal(g1[0], grad[i]), i
        if pending is not None:
            want = [h3.evaluate(ref_members, p.points[i]) for i in checked]
            idx = list(checked)
            e_v, e_g, e_m = _errors(value[idx], grad[idx], members[:, idx], want)
            print("%s: value error %.3g scale, gradient error %.3g on both sides of the pass boundary" % (p.name, e_v, e_g))
            assert e_v <= 1e-10 and e_g <= 1e-10 and e_m <= 1e-10
    D.close()


# ---- 5. the ascent against the host-driven loop ----
MS = tc.MS
_ascent_inputs = tc._ascent_inputs


@pytest.mark.parametrize("tolerance", [1e-10, 0.3], ids=["tight", "loose"])
def test_the_ascent_is_the_host_driven_loop_bit_for_bit(tolerance):
    p = h3.make_problem(h3.case(h3.ENSEMBLE))  # E = 3, F = 60
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], tolerance)
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    plain = _multistart(D, p, p.front, gd, bounds, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    bare = _multistart(D, p, None, gd, bounds, starts, points_being_sampled=pending)
    assert not np.array_equal(bare["start_values"], want["start_values"])  # (nor is the front)
    for on in (True, False):
        with _Launches(on):
            got = _multistart(D, p, p.front, gd, bounds, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    print("tolerance %g: %d kept starts, steps taken %s, value %.12g against the best start's %.12g" % (
        tolerance, len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max()))
    assert want["found"] and len(want["kept_index"]) == MS["starts"]
    if tolerance > 1e-3:
        assert int(want["steps_taken"].min()) < MS["steps"] * MS["restarts"]  # (masked steps occurred)
    else:
        assert want["value"] >= want["start_values"].max()
    none = _multistart(D, p, p.front, gd, bounds, starts, gradient_ascent=False, points_being_sampled=pending)
    best = int(np.argmax(want["start_values"]))
    assert np.array_equal(none["point"], starts[best]) and none["value"] == want["start_values"][best] and none["found"]
    D.close()


# ---- 6. greedy batches ----
def test_the_batch_is_the_ascent_fed_its_predecessors_bit_for_bit():
    p = h3.make_problem(h3.case(h3.ENSEMBLE))
    D = _Device(p)
    starts, gd, bounds = _ascent_inputs(p.points.shape[1], 1e-10)
    pending, q = p.pending[:1], 3
    want_points, want_values = [], []
    for t in range(q):
        fed = np.vstack([pending] + [x[None, :] for x in want_points])
        res = _multistart(D, p, p.front, gd, bounds, starts, points_being_sampled=fed)
        assert res["found"]
        want_points.append(res["point"])
        want_values.append(res["value"])
    for on in (True, False):
        with _Launches(on):
            got = _suggest(D, p, p.front, gd, bounds, starts, q, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array(want_points)), on
        assert np.array_equal(got["values"], np.array(want_values)) and np.all(got["found"])
    # the effect of the believed outcomes and the conditioned variances: no pick repeats an earlier one
    gaps = [float(np.min(np.max(np.abs(np.array(want_points)[:t] - want_points[t]), axis=1))) for t in range(1, q)]
    print("greedy values %s, largest coordinate gap of each pick to the nearest pick before it %s" % (want_values, gaps))
    assert min(gaps) >= 1e-3
    D.close()


# ---- 6b. the ascent and the batch at padded dimension 24 ----
# (tests/test_gpu_ehvi.py's settings: the host-driven loop over six GPs of up to 522 rows in 20 dimensions stays within seconds)
MS_WIDE = dict(MS, starts=6, steps=4, restarts=1)


def _wide_ascent_inputs(d):
    rng = np.random.default_rng(77)
    starts = rng.uniform(0.02, 0.98, size=(MS_WIDE["starts"], d))
    gd = (MS_WIDE["starts"], MS_WIDE["steps"], MS_WIDE["restarts"], 0, MS_WIDE["gamma"], MS_WIDE["pre_mult"], MS_WIDE["max_rel"], 1e-10)
    return starts, gd, np.array([[0.0, 1.0]] * d)


def test_the_ascent_on_the_wide_ensemble_is_the_host_driven_loop_bit_for_bit():
    """the ascent's own staging and step at padded dimension 24 over members of 20, 300 and 520 rows, groups of three"""
    p = h3.make_problem(h3.case(h3.WIDE))
    D = _Device(p)
    starts, gd, bounds = _wide_ascent_inputs(p.points.shape[1])
    pending = p.pending[:2]
    want = _host_loop(lambda x, g: _eval(D, p, x, pending=pending, want_grad=g), starts, gd, bounds)
    plain = _multistart(D, p, p.front, gd, bounds, starts)
    assert not np.array_equal(plain["start_values"], want["start_values"])  # (the pending points are not ignored)
    bare = _multistart(D, p, None, gd, bounds, starts, points_being_sampled=pending)
    assert not np.array_equal(bare["start_values"], want["start_values"])  # (nor is the front)
    for on in (True, False):
        with _Launches(on):
            got = _multistart(D, p, p.front, gd, bounds, starts, want_path=True, points_being_sampled=pending)
        diff = np.argwhere(np.any(got["path"] != want["path"], axis=2))
        assert diff.size == 0, (on, "the paths part at (start, row)", diff[np.argmin(diff[:, 1])])
        _same_run(got, want)
    moved = float(np.max(np.abs(want["end_points"] - starts[want["kept_index"]])))
    print("wide ensemble: %d kept starts, steps taken %s, value %.12g against the best start's %.12g; the ends lie up to %.3g from "
          "their starts" % (len(want["kept_index"]), [int(k) for k in want["steps_taken"]], want["value"], want["start_values"].max(), moved))
    assert want["found"] and len(want["kept_index"]) == MS_WIDE["starts"] and moved > 1e-3 and int(want["steps_taken"].max()) == 4
    D.close()


def test_the_batch_on_the_wide_ensemble_is_the_ascent_fed_its_predecessor_bit_for_bit():
    p = h3.make_problem(h3.case(h3.WIDE))
    D = _Device(p)
    starts, gd, bounds = _wide_ascent_inputs(p.points.shape[1])
    pending = p.pending[:1]
    first = _multistart(D, p, p.front, gd, bounds, starts, points_being_sampled=pending)
    second = _multistart(D, p, p.front, gd, bounds, starts, points_being_sampled=np.vstack([pending, first["point"][None, :]]))
    assert first["found"] and second["found"]
    for on in (True, False):
        with _Launches(on):
            got = _suggest(D, p, p.front, gd, bounds, starts, 2, points_being_sampled=pending)
        assert np.array_equal(got["points"], np.array([first["point"], second["point"]])), on
        assert np.array_equal(got["values"], np.array([first["value"], second["value"]])) and np.all(got["found"])
    print("wide ensemble: greedy values %.12g, %.12g; the second pick lies %.3g from the first" % (
        first["value"], second["value"], float(np.max(np.abs(second["point"] - first["point"])))))
    D.close()


# ---- 7. behaviour ----
def test_means_far_beyond_the_reference_point_give_exactly_zero():
    p = h3.make_problem(h3.case(h3.ENSEMBLE))
    D = _Device(p)
    low = min(float(np.min(g.y)) for row in p.gps for g in row) - 100.0  # far below every posterior mean
    for k in range(3):
        ref = list(p.ref)
        ref[k] = low
        v, g = api.ehvi3_ensemble(D.objs[0], D.objs[1], D.objs[2], ref, None, p.points, points_being_sampled=p.pending)
        assert np.all(v == 0.0) and np.all(np.isfinite(g))
    v, g = api.ehvi3_ensemble(D.objs[0], D.objs[1], D.objs[2], (low, low, low), None, p.points, points_being_sampled=p.pending)
    assert np.all(v == 0.0) and np.all(np.isfinite(g))
    D.close()


# ---- 8. limits ----
def test_a_front_of_192_with_64_pending_points_and_the_refusals():
    rng = np.random.default_rng(12)
    d, n = 2, 8
    X = rng.uniform(0, 1, size=(n, d))
    gps = [h3.GP(kr.MATERN, [1.3, 0.4, 0.4], X, 0.3 * rng.normal(size=(n, 1)), [1e-2], ()),
           h3.GP(kr.SE, [1.1, 0.5, 0.5], X, 0.3 * rng.normal(size=(n, 1)), [1e-2], ()),
           h3.GP(kr.MATERN, [1.2, 0.45, 0.5], X, 0.3 * rng.normal(size=(n, 1)), [1e-2], ())]
    front = h3.staircase_front(192)
    p = h3.Problem("f192", [gps], h3.REF, front, rng.uniform(0.1, 0.9, size=(4, d)), np.zeros((0, d)), (0, 1, 2, 3))
    D = _Device(p)
    starts = rng.uniform(0.05, 0.95, size=(6, d))
    gd = (6, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    bounds = [[0, 1]] * d
    # 65 picks without the ascent: the last round holds 64 pending points beside the 192 front points
    got = _suggest(D, p, p.front, gd, bounds, starts, 65, gradient_ascent=False)
    assert got["points"].shape == (65, d) and np.all(got["found"]) and np.all(np.isfinite(got["values"])) and np.all(got["values"] >= 0)
    fed = got["points"][:64]
    v, g, m = _eval(D, p, starts, pending=fed, want_member_values=True)
    assert float(np.max(v)) == got["values"][64] and np.array_equal(starts[int(np.argmax(v))], got["points"][64])
    members = [h3.Member(gps, p.ref, p.front, fed, LD)]
    want = [h3.evaluate(members, x) for x in starts]
    e_v, e_g, e_m = _errors(v, g, m, want)
    print("F = 192, p = 64 (the member's front holds %d points, its table %d boxes): value error %.3g scale, gradient error %.3g "
          "(bound 1e-10)" % (len(members[0].front), len(members[0].table), e_v, e_g))
    assert e_v <= 1e-10 and e_g <= 1e-10 and e_m <= 1e-10
    with pytest.raises(api.BoundsException) as e:
        _eval(D, p, p.points, front=h3.staircase_front(193))
    assert (e.value.value, e.value.min, e.value.max) == (193.0, 0.0, 192.0)
    with pytest.raises(api.BoundsException) as e:
        _suggest(D, p, p.front, gd, bounds, starts, 66, gradient_ascent=False)
    assert (e.value.value, e.value.min, e.value.max) == (66.0, 1.0, 65.0)
    with pytest.raises(api.BoundsException) as e:  # q = 65 beside one pending point: a 65th pending point
        _suggest(D, p, p.front, gd, bounds, starts, 65, gradient_ascent=False, points_being_sampled=starts[:1])
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 1.0, 64.0)
    with pytest.raises(api.BoundsException) as e:
        _eval(D, p, p.points, pending=rng.uniform(size=(65, d)))
    assert (e.value.value, e.value.min, e.value.max) == (65.0, 0.0, 64.0)
    # a handle listed twice, within an objective or across them
    with pytest.raises(api.InvalidValueException) as e:
        api.ehvi3_ensemble(D.objs[0], D.objs[1], D.objs[0], p.ref, p.front, p.points)
    assert "listed twice" in str(e.value)
    # a GP with a derivative observation
    deriv = api.DeviceGP([1.3, 0.4, 0.4], X, 0.3 * rng.normal(size=(n, 2)), [1e-2, 1e-2], [0])
    with pytest.raises(api.InvalidValueException) as e:
        api.ehvi3_ensemble(D.objs[0], D.objs[1], [deriv], p.ref, p.front, p.points)
    assert "derivative" in str(e.value)
    deriv.close()
    D.close()


def test_the_full_front_is_reached_through_a_greedy_pick():
    """63 of the full case's pending points fed, a value-only batch of 2 from starts on the pending line: the first pick's outcome
    joins as member 0's 256th point inside device memory (tests/test_ehvi3_reference.py asserts it for whichever start is picked),
    and the second round runs on 33 153 boxes"""
    c = h3.FULL
    p = h3.make_problem(c)
    D = _Device(p)
    starts, fed = h3.full_starts(p.pending), p.pending[:63]
    gd = (len(starts), 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    got = _suggest(D, p, p.front, gd, [[0, 1]] * 2, starts, 2, gradient_ascent=False, points_being_sampled=fed)
    assert got["points"].shape == (2, 2) and np.all(got["found"])
    picks = [int(np.flatnonzero(np.all(starts == x, axis=1))[0]) for x in got["points"]]  # (a noisy GP may pick a start twice)
    bound = max(1e-10, 4.0 * c.ld_diff)
    worst, sizes = [], []
    for t in range(2):
        members = h3.ensemble(p, LD, pending=np.vstack([fed, got["points"][:t]]))
        want = h3.evaluate(members, got["points"][t])
        worst.append(abs(got["values"][t] - float(want.value)) / want.scale)
        sizes.append((len(members[0].front), len(members[0].table)))
    assert sizes == [(255, 32896), (256, 33153)]
    # (the second round's value would miss the bound by far without the table's last box, strip 256 of slab 256)
    share = float(h3.last_box_share(members[0], got["points"][1])) / len(members) / (bound * want.scale)
    assert share >= 100.0
    # the second round is the evaluator's with all 64 fed, bit for bit, and that within the bound at every start
    all64 = np.vstack([fed, got["points"][:1]])
    v, g, m = _eval(D, p, starts, pending=all64, want_member_values=True)
    assert float(np.max(v)) == got["values"][1] and int(np.argmax(v)) == picks[1]
    e_v, e_g, e_m = _errors(v, g, m, [h3.evaluate(members, x) for x in starts])
    print("the full front through a pick (starts %s picked): the rounds' value errors %.3g and %.3g scale on %s (points, boxes), the last "
          "box %.3g times the bound; all 64 fed: value error %.3g scale, gradient error %.3g, members' error %.3g scale (bound %.3g)" % (
              picks, worst[0], worst[1], sizes, share, e_v, e_g, e_m, bound))
    assert max(worst) <= bound and e_v <= bound and e_g <= bound and e_m <= bound
    D.close()


def test_341_members():
    """E at its limit: 1023 handles, pointer tables of 1023 entries, a box-kernel grid of (C, 341)"""
    t0 = time.perf_counter()
    c = h3.MANY
    p, want = h3.expected(c, LD)
    t1 = time.perf_counter()
    D = _Device(p)
    t2 = time.perf_counter()
    assert len(D.objs[0]) == 341 and sum(len(row) for row in D.all) == 1023
    runs = []
    for on in (True, False):
        with _Launches(on):
            runs.append(_eval(D, p, p.points, want_member_values=True))
    value, grad, members = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)  # ensemble-wide launches on against off
    assert members.shape == (341, c.C) and np.all(np.isfinite(grad))
    bound = max(1e-10, 4.0 * c.ld_diff)
    e_v, e_g, e_m = _errors(value, grad, members, want)
    assert e_v <= bound and e_g <= bound and e_m <= bound, (e_v, e_g, e_m)
    assert np.array_equal(value, _host_mean(members))
    assert all(len(set(members[:, i])) == 341 for i in range(c.C))  # (no two members' values agree)
    starts = np.random.default_rng(341).uniform(0.1, 0.9, size=(3, c.d))
    res = _multistart(D, p, p.front, (3, 2, 1, 0, 0.7, 1.0, 0.5, 1e-10), [[0, 1]] * c.d, starts, points_being_sampled=p.pending)
    assert res["found"] and np.isfinite(res["value"]) and res["value"] > 0.0 and np.all(np.isfinite(res["point"]))
    t3 = time.perf_counter()
    D.close()
    t4 = time.perf_counter()
    print("E = 341: value error %.3g scale, gradient error %.3g, members' error %.3g scale (bound %.3g); an ascent of 3 starts and 2 steps "
          "ends at %.6g; wall time %.2f s: the long-double restatement %.2f (0 when another test built it), 1023 handles built in %.2f, "
          "the device calls %.2f, the handles closed in %.2f" % (e_v, e_g, e_m, bound, res["value"], t4 - t0, t1 - t0, t2 - t1, t3 - t2,
                                                                 t4 - t3))


def test_sampled_points_of_noise_free_gps_meet_the_variance_floors():
    """tests/test_gpu_ei1.py's construction for the box kernel's floors: three noise-free GPs on shared rows; candidate 0 on an
    observation a front point dominates by 0.15 in every objective, candidate 1 on one no front point dominates, candidate 2
    anywhere.  At candidate 1 the limit as the variances go to 0 is the deterministic gain of hypervolume_3; a device variance there
    is rounding noise, so the bound is formed from the float64 restatement's variances at that point: |psi - max(t - mu, 0)| <=
    0.4 sigma, carried through the box sum by h3.floor_bound with ten times the largest such sigma."""
    rng = np.random.default_rng(17)
    d, n = 2, 6
    X, Y = rng.uniform(0, 1, size=(n, d)), 0.3 * rng.normal(size=(n, 3))
    i0, i1 = int(np.argmax(Y[:, 0])), int(np.argmin(Y[:, 0]))
    front = ehvi.pareto_front_3(np.array([Y[i0] - 0.15, Y[i1] + (0.1, -0.2, 0.1)]), h3.REF)
    assert len(front) == 2 and Y[i0, 0] - Y[i1, 0] >= 0.3 and not any(np.all(q <= Y[i1]) for q in front)
    kinds = (kr.MATERN, kr.SE, kr.MATERN)
    gps = [h3.GP(kinds[k], np.array([1.3, 0.3, 0.3]), X, Y[:, k:k + 1].copy(), [0.0], ()) for k in range(3)]
    pts = np.vstack([X[i0], X[i1], rng.uniform(0.1, 0.9, size=d)])
    p = h3.Problem("floors", [gps], h3.REF, front, pts, np.zeros((0, d)), (0, 1, 2))
    scale = h3.member_scale(gps, h3.REF)
    m = h3.Member(gps, p.ref, front, p.pending, np.float64)
    sigma = max(np.sqrt(abs(float(h3.cr.moments(mm, b, X[i1])[1]))) for mm, b in zip(m.models, m.bases))
    gain = ehvi.hypervolume_3(np.vstack([front, Y[i1:i1 + 1]]), p.ref) - ehvi.hypervolume_3(front, p.ref)
    bound = h3.floor_bound(front, p.ref, Y[i1], 10.0 * sigma)
    D = _Device(p)
    v, g = _eval(D, p, pts)
    print("on sampled points of noise-free GPs: dominated %.3g, gradient %s; undominated %.12g against the deterministic gain %.12g "
          "(difference %.3g, bound %.3g from the restatement's sigma %.3g; 1e-6 scale is %.3g); beside them %.3g" % (
              v[0], g[0], v[1], gain, abs(v[1] - gain), bound, sigma, 1e-6 * scale, v[2]))
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(g)) and np.all(v >= 0.0)
    assert 0.0 <= v[0] <= 1e-10 * scale and v[2] > 1e-6
    assert gain > 1e-3 and bound <= 1e-6 * scale  # (the bound binds: the assertion on candidate 1 is kept)
    assert abs(v[1] - gain) <= bound
    D.close()


def test_bad_arguments_are_refused_in_the_headers_order():
    t3.refusals_in_order(_lib.load())


def test_a_pending_point_listed_twice_in_a_noise_free_gp_is_singular():
    """tests/test_gpu_ei1.py's construction with the noise-free GP as objective 3 of the second member: flat index 3 * 1 + 2"""
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    objs = [[api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [1e-5])] for _ in range(2)]
    objs.append([api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])])
    ref, front = (1.0, 1.0, 1.0), [(-0.5, 0.5, 0.0), (0.5, -0.5, 0.5)]
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, 0.7, 1.0, 0.5, 1e-10)
    for on in (True, False):
        with _Launches(on):
            with pytest.raises(api.SingularMatrixException) as e:
                api.ehvi3_ensemble(objs[0], objs[1], objs[2], ref, front, starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (5, 3) and "pending point 3" in str(e.value)
            with pytest.raises(api.SingularMatrixException) as e:
                api.ehvi3_multistart(objs[0], objs[1], objs[2], ref, front, gd, [[0, 1], [0, 1]], starts, points_being_sampled=pending)
            assert (e.value.num_rows, e.value.leading_minor_index) == (5, 3)
    ok = api.ehvi3_ensemble(objs[0], objs[1], objs[2], ref, front, starts, want_grad=False, points_being_sampled=pending[:3])
    assert np.all(np.isfinite(ok))  # (the handles still answer)
    for row in objs:
        for g in row:
            g.close()


# ---- 9. the wrapper, on three competing objectives and 8 points ----
def test_the_wrapper_and_the_optimisation_run_end_to_end_on_three_objectives():
    import wrappers_mirror as cw
    rng = np.random.default_rng(0)
    dim, noise, num_mcmc = 2, 1e-4, 3
    X = rng.uniform(size=(8, dim))
    centres = ((0.25, 0.25), (0.75, 0.75), (0.25, 0.75))
    ys = [np.sum((X - np.array(c)) ** 2, axis=1) * 4.0 - 1.0 for c in centres]
    hypers = np.array([[1.0, 0.5, 0.5], [1.4, 0.45, 0.6], [0.8, 0.6, 0.5]])
    models = []
    for vals in ys:
        hd = cw.HistoricalData(dim=dim, num_derivatives=0)
        hd.append_sample_points([cw.SamplePoint(X[i], [vals[i]], noise) for i in range(X.shape[0])])
        models.append(cw.GaussianProcessMCMC(hypers, np.full((num_mcmc, 1), noise), hd, []).member_models())
    ref = (2.0, 2.0, 2.0)
    front = ehvi.pareto_front_3(np.stack(ys, axis=1), ref)
    obj = ehvi.ExpectedHypervolumeImprovement3MCMC(models[0], models[1], models[2], ref)
    assert obj.problem_size == dim and np.array_equal(obj.front, front) and len(front) >= 2
    dev = [ehvi._device_members(m) for m in models]
    cand = rng.uniform(size=(7, dim))
    want_v, want_g = api.ehvi3_ensemble(dev[0], dev[1], dev[2], ref, front, cand)
    assert np.array_equal(obj.evaluate_at_point_list(cand), want_v)
    obj.set_current_point(cand[3])
    assert obj.compute_objective_function() == want_v[3] and np.array_equal(obj.compute_grad_objective_function(), want_g[3:4])
    gd = (16, 10, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    bounds = [[0.0, 1.0]] * dim
    points, values, found = ehvi.multistart_expected_hypervolume_improvement_3_optimization(
        models[0], models[1], models[2], ref, bounds, gd, num_multistarts=16, num_to_sample=3, seed=31)
    assert points.shape == (3, dim) and values.shape == (3,) and np.all(found)
    assert np.all(points >= 0.0) and np.all(points <= 1.0) and np.all(np.isfinite(values)) and values[0] > 0.0
    starts = api.latin_hypercube(31, bounds, 16)
    first = api.ehvi3_multistart(dev[0], dev[1], dev[2], ref, front, gd, bounds, starts)
    assert np.array_equal(points[0], first["point"]) and values[0] == first["value"]
    # the first member's believed outcome of the first pick extends the front: the hypervolume grows
    gps = [h3.GP(kr.MATERN, hypers[0], X, y.reshape(-1, 1), [noise], ()) for y in ys]
    member = h3.Member(gps, ref, front, points[:1], LD)
    believed = np.array([[float(x) for x in member.outcomes[0]]])
    before, after = ehvi.hypervolume_3(front, ref), ehvi.hypervolume_3(np.vstack([front, believed]), ref)
    res = h3.evaluate([h3.Member([h3.GP(kr.MATERN, hypers[e], X, y.reshape(-1, 1), [noise], ()) for y in ys], ref, front,
                                 np.zeros((0, dim)), LD) for e in range(num_mcmc)], points[0])
    print("three quadratic bowls, 8 points, 3 members: a batch of 3 at %s, values %s; hypervolume %.4f -> %.4f with the first pick's "
          "believed outcome; its value %.6g against the restatement's %.6g" % (
              np.round(points, 3).tolist(), [float(v) for v in values], before, after, values[0], float(res.value)))
    assert after > before and abs(values[0] - float(res.value)) <= 1e-10 * res.scale
