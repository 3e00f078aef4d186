"""Every ensemble member's own posterior-mean minimiser (moe_posterior_mean_members_minimize; the reference's examples/main.py:175-193
over ComputeOptimalPosteriorMean from one start) restated on the host: the checker of tests/test_gpu_pm_members.py, itself held to
the unmodified reference and to a literal copy of the library's host loop by tests/test_pm_members_reference.py.  NumPy only.

For one member (recommend_reference.Member: sampling_reference's posterior, derivative observations included), mu = its posterior
mean with the num_fidelity trailing coordinates pinned to 1, f = -mu:
    screen    mu at every candidate; start = numpy.argmin
    descend   posterior_mean_optimize (csrc/multistart.hip) decision for decision: restarts x steps; alpha_0 = pre_mult (i + 1)^-gamma
              (numpy.power's double, as the library takes it from the host's pow); up to 30 halvings under
              f_trial - f0 > alpha |g|^2 / 2; TensorProductDomain::LimitUpdate per coordinate; the re-evaluation when the limiter
              changed the step; the three stopping rules; the restart rule
    keep      the start if mu(end) > mu(start), the end otherwise

run(member, ...) works in the member's arithmetic: np.longdouble members give the checker, np.float64 members its twin of the same
algebra.  Both return every output AND the margin of every decision: (name, |left - right|) of each comparison taken.  one_step(x, i)
is the map of step i (0-based) from a given point with its decisions and margins, F_ext of the GPU tests.
"""
import collections

import numpy as np

import recommend_reference as rr
from sampling_reference import LD

# moe_gd_params_t's order: num_multistarts, max_num_steps, max_num_restarts, num_steps_averaged, gamma, pre_mult,
# max_relative_change, tolerance
MAIN_INNER = (1, 6, 1, 3, 0.0, 1.0, 0.1, 1.0e-10)   # examples/main.py's inner parameters
LONG_INNER = (1, 40, 2, 3, 0.0, 1.0, 0.2, 1.0e-9)

Step = collections.namedtuple("Step", "x f0 gnorm alpha0 halvings changed rejected moved stop_norm state margins")
Result = collections.namedtuple("Result", "means start_index gap path steps end mu_end mu_start fell_back best_point best_value "
                                          "margins")


def alpha_table(gd):
    return np.array([gd[5] * np.power(float(i + 1), -gd[4]) for i in range(gd[1])], dtype=np.float64)


class Objective(object):
    """f = -mu and its gradient over the free coordinates, in the member's arithmetic."""

    def __init__(self, member, num_fidelity=0):
        self.m, self.nf = member, int(num_fidelity)
        self.t = member.dtype
        self.size = member.X.shape[1] - self.nf

    def full(self, pts):
        pts = np.asarray(pts).astype(self.t).reshape(-1, self.size)
        return np.concatenate([pts, np.ones((pts.shape[0], self.nf), dtype=self.t)], axis=1)

    def mu(self, pts):
        return self.m.mu_grad(self.full(pts), False)[0]

    def f(self, x):
        return -self.m.mu_grad(self.full(x), False)[0][0]

    def f_grad(self, x):
        mu, g = self.m.mu_grad(self.full(x), True)
        return -mu[0], -g[0, :self.size]


def limit_1d(t, lo, hi, mrc, x, desired, margins, k):
    """limit_update_1d (csrc/multistart.hip; gpp_domain.cpp:64-105) with the margin of every branch taken"""
    lo, hi, mrc, half = t(lo), t(hi), t(mrc), t(0.5)
    dist = np.fmin(x - lo, hi - x)
    margins.append(("limit%d" % k, abs(float(np.fabs(desired) - mrc * dist))))
    if np.fabs(desired) > mrc * dist:
        desired = np.copysign(mrc * dist, desired)
    nxt = x + desired
    margins.append(("inside%d" % k, float(min(abs(nxt - lo), abs(hi - nxt)))))
    if nxt < lo:
        margins.append(("halflo%d" % k, abs(float(x + desired * half - lo))))
        desired = (lo - x) * half if x + desired * half < lo else desired * half
    elif nxt > hi:
        margins.append(("halfhi%d" % k, abs(float(x + desired * half - hi))))
        desired = (hi - x) * half if x + desired * half > hi else desired * half
    return desired


def one_step(obj, gd, bounds, x, i):
    """Step i (0-based within its restart) of the line search from x, in obj's arithmetic.  state: 1 accepted, 2 ended without a
    move (30 failed trials or a zero step), 3 rejected by f(x + step) <= f0."""
    t = obj.t
    T, mrc, tol = int(gd[1]), gd[6], gd[7]
    x = np.asarray(x).astype(t).reshape(obj.size)
    bounds = np.asarray(bounds, dtype=np.float64).reshape(obj.size, 2)
    margins = []
    f0, g = obj.f_grad(x)
    alpha0 = alpha_table(gd)[i]
    alpha = t(alpha0)
    n2 = t(0)
    for k in range(obj.size):
        n2 = n2 + g[k] * g[k]
    search, ftrial = 0, f0
    while search < 30:
        ftrial = obj.f(x + alpha * g)
        margins.append(("armijo%d" % search, abs(float((ftrial - f0) - t(0.5) * alpha * n2))))
        if ftrial - f0 > t(0.5) * alpha * n2:
            break
        alpha = alpha * t(0.5)
        search += 1
    step = np.zeros(obj.size, dtype=t)
    changed = nonzero = False
    for k in range(obj.size):
        raw = alpha * g[k]
        step[k] = limit_1d(t, bounds[k, 0], bounds[k, 1], mrc, x[k], raw, margins, k)
        changed = changed or bool(step[k] != raw)
        nonzero = nonzero or bool(step[k] != 0)
    gnorm = float(np.max(np.abs(g))) if obj.size else 0.0
    if search == 30 or not nonzero:
        return Step(x, f0, gnorm, alpha0, search, changed, False, False, False, 2, margins)
    obj2 = obj.f(x + step) if changed else ftrial
    margins.append(("obj2", abs(float(obj2 - f0))))
    if obj2 <= f0:
        return Step(x, f0, gnorm, alpha0, search, changed, True, False, False, 3, margins)
    norm = np.sqrt(np.sum(step * step))
    step_tol = t(tol) / t(max(T, 1))
    margins.append(("stepnorm", abs(float(norm - step_tol))))
    return Step(x + step, f0, gnorm, alpha0, search, changed, False, True, bool(norm < step_tol), 1, margins)


def descend(obj, gd, bounds, x0):
    """(end point, steps [(restart, step index, Step)], margins) of the whole optimisation from x0"""
    T, R, tol = int(gd[1]), int(gd[2]), gd[7]
    x = np.asarray(x0).astype(obj.t).reshape(obj.size)
    steps, margins = [], []
    for r in range(R):
        x_begin = x.copy()
        for i in range(T):
            s = one_step(obj, gd, bounds, x, i)
            steps.append((r, i, s))
            margins += [("r%d.i%d.%s" % (r, i, n), v) for n, v in s.margins]
            x = s.x
            if s.state != 1 or s.stop_norm:
                break
        moved = np.sqrt(np.sum((x_begin - x) * (x_begin - x)))
        margins.append(("r%d.restart" % r, abs(float(moved - obj.t(tol)))))
        if not moved > obj.t(tol):
            break
    return x, steps, margins


def run(member, num_fidelity, gd, bounds, candidates):
    """The whole procedure for one member over its candidates [C][size]."""
    obj = Objective(member, num_fidelity)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, obj.size)
    means = obj.mu(cand)
    start = int(np.argmin(means))
    order = np.sort(means)
    gap = float(order[1] - order[0]) if len(order) > 1 else np.inf
    margins = [("argmin", gap)] if len(order) > 1 else []
    end, steps, m2 = descend(obj, gd, bounds, cand[start])
    margins += m2
    mu_end, mu_start = -obj.f(end), means[start]
    margins.append(("keep", abs(float(mu_end - mu_start))))
    fell_back = bool(mu_end > mu_start)
    best = cand[start].astype(obj.t) if fell_back else end
    path = [cand[start].astype(obj.t)] + [s.x for _, _, s in steps]
    return Result(means, start, gap, path, steps, end, mu_end, mu_start, fell_back, best, mu_start if fell_back else mu_end, margins)


def min_margin(result_or_margins):
    margins = getattr(result_or_margins, "margins", result_or_margins)
    return min([v for _, v in margins] or [np.inf])


def literal_float64(mean_fn, grad_fn, d, num_fidelity, gd, bounds, x0):
    """posterior_mean_optimize (csrc/multistart.hip:459-516) line for line in plain double over two callables of full-dimensional
    points: mean_fn(pt [d]) -> mu, grad_fn(pt [d]) -> d mu / d x [d].  Returns (best_point, f at it, decisions per step)."""
    size = d - num_fidelity
    T, R, gamma, pre_mult, mrc, tol = int(gd[1]), int(gd[2]), gd[4], gd[5], gd[6], gd[7]
    bounds = np.asarray(bounds, dtype=np.float64).reshape(size, 2)
    x = np.array(x0, dtype=np.float64).reshape(size)

    def f(p, want_grad=False):
        pt = np.concatenate([p, np.ones(num_fidelity)])
        mu = float(mean_fn(pt))
        if want_grad:
            return -mu, -np.asarray(grad_fn(pt), dtype=np.float64).ravel()[:size]
        return -mu

    def limit_update_1d(lo, hi, max_relative_change, xk, desired):
        dist = np.fmin(xk - lo, hi - xk)
        if np.fabs(desired) > max_relative_change * dist:
            desired = np.copysign(max_relative_change * dist, desired)
        nxt = xk + desired
        if nxt < lo:
            desired = (lo - xk) * 0.5 if xk + desired * 0.5 < lo else desired * 0.5
        elif nxt > hi:
            desired = (hi - xk) * 0.5 if xk + desired * 0.5 > hi else desired * 0.5
        return desired

    fcur = f(x)
    step_tol = tol / float(max(T, 1))
    decisions = []
    for r in range(R):
        x_begin = x.copy()
        for i in range(T):
            f0, g = f(x, True)
            fcur = f0
            alpha = pre_mult * np.power(float(i + 1), -gamma)
            n2 = 0.0
            for k in range(size):
                n2 += g[k] * g[k]
            search, ftrial = 0, f0
            while search < 30:
                trial = x + alpha * g
                ftrial = f(trial)
                if ftrial - f0 > 0.5 * alpha * n2:
                    break
                alpha *= 0.5
                search += 1
            step = np.array([limit_update_1d(bounds[k, 0], bounds[k, 1], mrc, x[k], alpha * g[k]) for k in range(size)])
            changed = bool(np.any(step != alpha * g))
            nonzero = bool(np.any(step != 0.0))
            if search == 30 or not nonzero:
                decisions.append((r, i, search, changed, False, False, 2))
                break
            obj2 = ftrial
            if changed:
                obj2 = f(x + step)
            if obj2 <= f0:
                decisions.append((r, i, search, changed, True, False, 3))
                break
            x = x + step
            fcur = obj2
            stop = bool(np.sqrt(np.sum(step * step)) < step_tol)
            decisions.append((r, i, search, changed, False, stop, 1))
            if stop:
                break
        if not np.sqrt(np.sum((x_begin - x) ** 2)) > tol:
            break
    return x, fcur, decisions


def decisions_of(steps):
    return [(r, i, s.halvings, s.changed, s.rejected, s.stop_norm, s.state) for r, i, s in steps]


# ---- the cases of the GPU tests, and the gap between the two arithmetics over them ----
# seed, n, d, E, cov_type, derivs, num_fidelity, C, gd, candidate range
def gpu_cases():
    import sampling_reference as sr
    SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
    return [
        (2, 30, 2, 3, MATERN, (), 0, 40, MAIN_INNER),
        (0, 25, 3, 2, SE, (0, 2), 1, 30, MAIN_INNER),
        (0, 40, 8, 2, MATERN, (), 0, 50, MAIN_INNER),
        (5, 30, 3, 2, MATERN, (), 0, 40, (1, 12, 2, 3, 0.0, 1.0, 0.2, 1.0e-9)),
    ]


def edge_cases():
    """the cases of tests/test_gpu_pm_members_edges.py, gpu_cases()'s layout: every padded dimension above 8 (d = 9 .. 32 pad to 12, 16,
    24, 24, 32, 32), one with two observed derivatives and a fidelity coordinate, LONG_INNER cut to 12 steps at d = 32 (its second
    restart moves), and main.py's parameters with a pre_mult small enough for steps that the limiter leaves alone"""
    import sampling_reference as sr
    SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
    return [
        (1, 20, 9, 2, MATERN, (), 0, 30, MAIN_INNER),
        (0, 20, 16, 2, SE, (), 0, 30, MAIN_INNER),
        (1, 20, 17, 2, MATERN, (), 0, 30, MAIN_INNER),
        (1, 20, 24, 2, SE, (), 0, 30, MAIN_INNER),
        (1, 20, 25, 2, MATERN, (0, 2), 1, 30, MAIN_INNER),
        (1, 20, 32, 2, SE, (), 0, 30, MAIN_INNER),
        (2, 20, 32, 2, MATERN, (), 0, 30, LONG_INNER[:1] + (12,) + LONG_INNER[2:]),
        (0, 20, 24, 2, MATERN, (), 0, 30, MAIN_INNER[:5] + (1.0e-3,) + MAIN_INNER[6:]),
    ]


def case_problem(case, dtype=LD):
    """(members, arrays, bounds, candidates) of a case: the candidates are uniform draws followed by the sampled points, as main.py
    screens them"""
    seed, n, d, E, cov, derivs, nf, C_, gd = case
    members, a = rr.make_ensemble(seed, n, d, E, cov, derivs, dtype=dtype)
    size = d - nf
    rng = np.random.default_rng(7000 + seed)
    cand = np.vstack([rng.uniform(0.05, 0.95, size=(C_ - n, size)), a["X"][:, :size]]) if C_ > n else rng.uniform(0.05, 0.95, size=(C_, size))
    return members, a, np.array([[0.0, 1.0]] * size), cand


_GAP = {}


def gap():
    """max over the GPU cases and their members of |float64 twin - long double| of the end point, relative to max(1, |x|): what
    plain double arithmetic with this algebra loses end to end; the device's end-to-end bound is derived from it."""
    if "v" not in _GAP:
        worst = 0.0
        for case in gpu_cases():
            mld, a, bounds, cand = case_problem(case, LD)
            m64 = case_problem(case, np.float64)[0]
            for e in range(len(mld)):
                want = run(mld[e], case[6], case[8], bounds, cand)
                got = run(m64[e], case[6], case[8], bounds, cand)
                if want.start_index != got.start_index or decisions_of(want.steps) != decisions_of(got.steps):
                    continue  # (a decision closer than the arithmetic: the GPU tests refuse such a case by its margins)
                x = want.end.astype(np.float64)
                worst = max(worst, float(np.max(np.abs(got.end - want.end) / np.maximum(1.0, np.abs(x)))))
        _GAP["v"] = worst
    return _GAP["v"]
