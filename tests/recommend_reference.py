"""The recommendation step of a Bayesian-optimisation iteration (examples/main.py:243-260 of the reference) restated on the host:
the checker of tests/test_gpu_recommend.py, itself held to the reference's own classes by tests/test_recommend_reference.py.

    f(x)      = -(1/E) sum_e mu_e(x, fidelity coordinates = 1), members summed in ascending order, then divided by E
    screen    i0 = the first index of the largest f over the candidates
    starts    the num_starts candidates with the largest f, equal values by index
    descent   x_i = x_{i-1} + clamp(a_i grad f(x_{i-1})), a_i = pre_mult i^-gamma, i = 1 .. T; per coordinate
              dist = fmin(x - lo, hi - x), |step| > max_relative_change dist -> copysign(max_relative_change dist, step)
              end point = the mean of the last k steps (k = T for num_steps_averaged < 0 or > T, 1 for 0)
    pick      the first of the largest f over the end points
    keep      the screened candidate if -f(winner) > -f(candidate i0), the winner otherwise

extended(): every quantity in np.longdouble (sampling_reference's arithmetic; the GP may observe derivatives), with the margin of
every decision.  literal(): the same in plain double, call for call as the reference writes it (PosteriorMeanMCMC,
GradientDescentOptimizer.optimize, TensorProductDomain.compute_update_restricted_to_domain, MultistartOptimizer.optimize).
a_i is numpy.power's double in both, as the library takes it from the host's pow.
"""
import collections

import numpy as np

import loo_reference as lo
import sampling_reference as sr
from ei_reference import backward_solve
from sampling_reference import LD

GdParams = collections.namedtuple("GdParams", "max_num_steps num_steps_averaged gamma pre_mult max_relative_change")


def gd_tuple(gd, num_multistarts=1, max_num_restarts=1, tolerance=1.0e-10):
    """the 8-tuple api.DeviceGP._gd takes"""
    return (num_multistarts, gd.max_num_steps, max_num_restarts, gd.num_steps_averaged, gd.gamma, gd.pre_mult,
            gd.max_relative_change, tolerance)


def averaging_window(gd):
    T, k = gd.max_num_steps, gd.num_steps_averaged
    if k < 0 or k > T:
        return T
    return 1 if k == 0 else k


def step_sizes(gd):
    return np.array([gd.pre_mult * np.power(float(i), -gd.gamma) for i in range(1, gd.max_num_steps + 1)], dtype=np.float64)


class Member(object):
    """One GP of the ensemble in the arithmetic `dtype` (np.longdouble: the checker; np.float64: the literal restatement).
    hyper = [alpha, lengths (d)], noise [1 + g], y [n][1 + g], derivs: the observed partial derivatives."""

    def __init__(self, cov_type, hyper, X, y, noise, derivs=(), dtype=LD):
        self.dtype, self.cov_type, self.derivs = dtype, int(cov_type), [int(v) for v in derivs]
        self.X = np.asarray(X, dtype=np.float64)
        n, d = self.X.shape
        g1 = 1 + len(self.derivs)
        hyper = np.asarray(hyper, dtype=np.float64).ravel()
        self.alpha, self.lengths = dtype(hyper[0]), hyper[1:1 + d].astype(dtype)
        K = lo.covariance(self.cov_type, self.X, self.derivs, self.alpha, self.lengths, dtype)
        K[np.diag_indices(n * g1)] += np.tile(np.asarray(noise, dtype=np.float64).ravel()[:g1].astype(dtype), n)
        Y = np.asarray(y, dtype=np.float64).reshape(n, g1)
        self.mean = sr.constant_mean(Y[:, 0])  # (accumulated in double in observation order, as the library forms it)
        yc = Y.astype(dtype)
        yc[:, 0] -= dtype(self.mean)
        if dtype is LD:
            L = sr.cholesky_spd(K)
            self.w = backward_solve(L, sr.forward_solve(L, yc.ravel())).reshape(n, g1)
        else:
            self.w = np.linalg.solve(K, yc.ravel()).reshape(n, g1)

    def mu_grad(self, pts, want_grad=True):
        """(mu [P], d mu / d x [P][d] or None) of the function value at pts [P][d]."""
        t = self.dtype
        pts = np.asarray(pts).astype(t).reshape(-1, self.X.shape[1])
        il2 = t(1) / (self.lengths * self.lengths)
        diff = pts[:, None, :] - self.X.astype(t)[None, :, :]  # [P][n][d]: x - X_j
        r2 = np.sum(diff * diff * il2, axis=2)
        if self.cov_type == sr.COV_SQUARE_EXPONENTIAL:
            base = self.alpha * np.exp(-r2 / t(2))
            first = second = base
        else:
            a = np.sqrt(t(5) * r2)
            e = np.exp(-a)
            base = self.alpha * e * (t(1) + a + t(5) / t(3) * r2)
            first = t(5) / t(3) * self.alpha * e * (a + t(1))
            second = t(25) / t(3) * self.alpha * e
        mu = t(self.mean) + np.sum(base * self.w[None, :, 0], axis=1)
        for b, i2 in enumerate(self.derivs):
            mu = mu + np.sum(first * diff[:, :, i2] * il2[i2] * self.w[None, :, 1 + b], axis=1)
        if not want_grad:
            return mu, None
        di = -diff * il2  # [P][n][d]
        grad = np.sum(di * (first * self.w[None, :, 0])[:, :, None], axis=1)
        for b, i2 in enumerate(self.derivs):
            wb = self.w[None, :, 1 + b]
            grad = grad + np.sum(di * (second * diff[:, :, i2] * il2[i2] * wb)[:, :, None], axis=1)
            grad[:, i2] = grad[:, i2] + np.sum(first * il2[i2] * wb, axis=1)
        return mu, grad


class Ensemble(object):
    """f and its gradient over the free coordinates, in the members' arithmetic."""

    def __init__(self, members, num_fidelity=0):
        self.members, self.num_fidelity = list(members), int(num_fidelity)
        self.dim = self.members[0].X.shape[1]
        self.size = self.dim - self.num_fidelity
        self.dtype = self.members[0].dtype

    def full(self, pts):
        pts = np.asarray(pts).astype(self.dtype).reshape(-1, self.size)
        return np.concatenate([pts, np.ones((pts.shape[0], self.num_fidelity), dtype=self.dtype)], axis=1)

    def f(self, pts, want_grad=False):
        """(f [P], grad f [P][size] or None): members ascending, then the division."""
        x = self.full(pts)
        total, gtotal = 0, 0
        for m in self.members:
            mu, g = m.mu_grad(x, want_grad)
            total = total + (-mu)
            if want_grad:
                gtotal = gtotal + (-g[:, :self.size])
        E = self.dtype(len(self.members))
        return total / E, (gtotal / E if want_grad else None)


def clamp_step(x, step, bounds, max_relative_change):
    """python_version/domain.py:187-200, per coordinate, in the arithmetic of x"""
    t = x.dtype.type
    dist = np.fmin(x - bounds[:, 0].astype(x.dtype), bounds[:, 1].astype(x.dtype) - x)
    limit = t(max_relative_change) * dist
    return np.where(np.fabs(step) > limit, np.copysign(limit, step), step)


def top_indices(f, count):
    """the `count` largest, equal values by index"""
    f = np.asarray(f)
    return np.array(sorted(range(len(f)), key=lambda i: (-f[i], i))[:count], dtype=np.int64)


Result = collections.namedtuple("Result", "index starts values F paths end_points end_values winner refined point value margins")


def extended(ens, gd, bounds, candidates, num_starts=1):
    """The procedure in extended precision.  F(x, i) is the map of step i (1-based) from the point x; margins: best against
    second-best candidate, the num_starts cut, best against second-best end point, the keep-or-fall-back comparison."""
    assert ens.dtype is LD
    bounds = np.asarray(bounds, dtype=np.float64).reshape(ens.size, 2)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, ens.size)
    steps = step_sizes(gd)
    fc = ens.f(cand)[0]
    order = top_indices(fc, len(fc))
    starts = order[:num_starts]
    margins = []
    if len(fc) > 1:
        margins.append(float(fc[order[0]] - fc[order[1]]))
    if num_starts > 1 and len(fc) > num_starts:
        margins.append(float(fc[order[num_starts - 1]] - fc[order[num_starts]]))

    def F(x, i):
        x = np.asarray(x).astype(LD).reshape(ens.size)
        g = ens.f(x[None, :], True)[1][0]
        return x + clamp_step(x, LD(steps[i - 1]) * g, bounds, gd.max_relative_change)

    T, k = gd.max_num_steps, averaging_window(gd)
    paths = np.zeros((num_starts, T + 1, ens.size), dtype=LD)
    for s, c in enumerate(starts):
        paths[s, 0] = cand[c].astype(LD)
        for i in range(1, T + 1):
            paths[s, i] = F(paths[s, i - 1], i)
    ends = np.sum(paths[:, T - k + 1:], axis=1) / LD(k)
    fe = ens.f(ends)[0]
    eorder = top_indices(fe, len(fe))
    winner = int(eorder[0])
    if num_starts > 1:
        margins.append(float(fe[eorder[0]] - fe[eorder[1]]))
    i0 = int(order[0])
    margins.append(float(abs(fe[winner] - fc[i0])))
    fall_back = -fe[winner] > -fc[i0]
    point = cand[i0].astype(LD) if fall_back else ends[winner]
    value = fc[i0] if fall_back else fe[winner]
    return Result(i0, starts, fc, F, paths, ends, fe, winner, not fall_back, point, value, margins)


class LiteralPosteriorMeanMCMC(object):
    """cpp_wrappers/knowledge_gradient_mcmc.py:25-157 over double-precision members (Member(..., dtype=np.float64))."""

    def __init__(self, gaussian_process_list, num_fidelity):
        self._gaussian_process_list = gaussian_process_list
        self._num_fidelity = num_fidelity
        self._points_to_sample = np.zeros((1, gaussian_process_list[0].X.shape[1]))

    dim = property(lambda self: self._gaussian_process_list[0].X.shape[1])
    problem_size = property(lambda self: self.dim - self._num_fidelity)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def _full(self):
        return np.concatenate([self._points_to_sample.ravel()[:self.problem_size], np.ones(self._num_fidelity)])[None, :]

    def compute_posterior_mean_mcmc(self):
        total = 0
        for gp in self._gaussian_process_list:
            total += -float(gp.mu_grad(self._full(), False)[0][0])  # C_GP.compute_posterior_mean
        return total / len(self._gaussian_process_list)

    compute_objective_function = compute_posterior_mean_mcmc

    def compute_grad_posterior_mean_mcmc(self):
        total = np.zeros((1, self.problem_size))
        for gp in self._gaussian_process_list:
            total += -gp.mu_grad(self._full(), True)[1][:, :self.problem_size]  # C_GP.compute_grad_posterior_mean
        return total / len(self._gaussian_process_list)

    compute_grad_objective_function = compute_grad_posterior_mean_mcmc


def _literal_descent(ps, gd, bounds):
    """GradientDescentOptimizer.optimize (:498-527) with RepeatedDomain(1, TensorProductDomain)"""
    initial_guess = ps.current_point
    x_path = np.empty((gd.max_num_steps + 1, ) + initial_guess.shape)
    x_path[0, ...] = initial_guess
    step_counter = 1
    while step_counter <= gd.max_num_steps:
        alpha_n = gd.pre_mult * np.power(float(step_counter), -gd.gamma)
        ps.current_point = x_path[step_counter - 1, ...]
        orig_step = ps.compute_grad_objective_function()
        orig_step *= alpha_n
        current = x_path[step_counter - 1, ...]
        fixed_step = np.empty_like(orig_step)
        for j, step in enumerate(orig_step[0]):
            distance_to_boundary = np.fmin(current[0, j] - bounds[j, 0], bounds[j, 1] - current[0, j])
            desired_step = step
            if np.fabs(step) > gd.max_relative_change * distance_to_boundary:
                desired_step = np.copysign(gd.max_relative_change * distance_to_boundary, step)
            fixed_step[0, j] = desired_step
        x_path[step_counter, ...] = fixed_step + x_path[step_counter - 1, ...]
        step_counter += 1
    k = averaging_window(gd)
    start, end = (step_counter - 1) - k + 1, (step_counter - 1) + 1
    ps.current_point = np.mean(x_path[start:end, ...], axis=0)
    return x_path


def literal(members, num_fidelity, gd, bounds, candidates, num_starts=1):
    """The procedure in plain double, the reference's calls in the reference's order; the Result's F is None."""
    ps = LiteralPosteriorMeanMCMC(members, num_fidelity)
    size = ps.problem_size
    bounds = np.asarray(bounds, dtype=np.float64).reshape(size, 2)
    eval_pts = np.asarray(candidates, dtype=np.float64).reshape(-1, size)
    test = np.zeros(eval_pts.shape[0])
    for i, pt in enumerate(eval_pts):
        ps.set_current_point(pt.reshape((1, size)))
        test[i] = -ps.compute_objective_function()
    i0 = int(np.argmin(test))
    starts = top_indices(-test, num_starts)
    best_function_value, best_point, winner = -np.inf, eval_pts[starts[0]].reshape(1, size), 0
    paths, ends, end_values = [], [], []
    for s, c in enumerate(starts):  # MultistartOptimizer.optimize (:595-603)
        ps.current_point = eval_pts[c].reshape((1, size))
        paths.append(_literal_descent(ps, gd, bounds)[:, 0, :])
        function_value = ps.compute_objective_function()
        ends.append(ps.current_point.ravel())
        end_values.append(function_value)
        if function_value > best_function_value:
            best_function_value, best_point, winner = function_value, ps.current_point, s
    report_point = best_point
    ps.set_current_point(report_point.reshape((1, size)))
    refined = True
    if -ps.compute_objective_function() > np.min(test):
        report_point, refined = eval_pts[i0].reshape((1, size)), False
    ps.set_current_point(report_point)
    return Result(i0, starts, -test, None, np.array(paths), np.array(ends), np.array(end_values), winner, refined,
                  report_point.ravel(), ps.compute_objective_function(), None)


def make_ensemble(seed, n, d, E, cov_type, derivs=(), noise=1e-2, dtype=LD):
    """A seeded problem: (members in `dtype`, the arrays api.DeviceGP takes per member)."""
    rng = np.random.default_rng(seed)
    g1 = 1 + len(derivs)
    X = rng.uniform(0.0, 1.0, size=(n, d))
    y = rng.normal(size=(n, g1))
    hypers = [np.concatenate([[rng.uniform(0.8, 1.6)], rng.uniform(0.3, 0.9, size=d) * np.sqrt(d)]) for _ in range(E)]
    noises = [np.full(g1, noise * rng.uniform(0.5, 2.0)) for _ in range(E)]
    members = [Member(cov_type, hypers[e], X, y, noises[e], derivs, dtype) for e in range(E)]
    return members, dict(X=X, y=y, hypers=hypers, noises=noises, derivs=list(derivs), cov_type=cov_type)


# ---- the cases of tests/test_gpu_recommend_edges.py; tests/test_recommend_reference.py asserts their margins on the CPU ----
EDGE_GD = GdParams(6, 3, 0.7, 1.0, 0.02)       # clamped: a_i |grad f| exceeds 0.02 of the distance to the nearer face at every step
EDGE_GD_FREE = GdParams(6, 3, 0.7, 0.02, 0.5)  # a small pre_mult in the interior: the clamp is inactive at every step
EDGE_GD_3 = GdParams(3, 3, 0.7, 0.02, 0.5)
EDGE_GD_1 = GdParams(1, 0, 0.7, 0.02, 0.5)

EdgeCase = collections.namedtuple("EdgeCase", "kind seed n d E cov derivs num_fidelity C S gd")


def edge_cases():
    """kind: 'descent' (every padded dimension; E = 3 leaves wavefronts idle at W = 8 and W = 4, E = 5 makes a second member group
    at W = 4), 'small' (n = 1, 2: n = 1 observes derivatives, for a single function value equals the constant mean and f is flat),
    'lds' (the training points at, below and above the LDS-staging limits), 'select' (more candidates than threads), 'ties' and 'nan'
    (the selection's base sets)."""
    SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
    cases = [
        EdgeCase("descent", 0, 20, 8, 3, MATERN, (), 0, 6, 2, EDGE_GD),
        EdgeCase("descent", 0, 20, 16, 5, SE, (), 0, 6, 2, EDGE_GD_FREE),
        EdgeCase("descent", 0, 20, 17, 3, MATERN, (), 0, 6, 2, EDGE_GD),
        EdgeCase("descent", 0, 20, 24, 5, SE, (), 0, 6, 2, EDGE_GD_FREE),
        EdgeCase("descent", 0, 20, 25, 5, MATERN, (0, 2), 1, 6, 2, EDGE_GD),
        EdgeCase("descent", 0, 20, 32, 3, SE, (), 0, 6, 2, EDGE_GD),
    ]
    for d, derivs in ((3, (0, 2)), (32, (1, 31))):
        for n in (1, 2):
            for E in (1, 17):
                cases.append(EdgeCase("small", 0, n, d, E, MATERN, derivs if n == 1 else (), 0, 3, 1, EDGE_GD_3))
    for d, n in ((3, 30), (32, 192), (32, 193), (32, 384), (32, 385)):
        cases.append(EdgeCase("lds", 0, n, d, 2, MATERN if n % 2 else SE, (), 0, 4, 1, EDGE_GD_3))
    for C in (257, 600):
        for S in (2, 7):
            cases.append(EdgeCase("select", 0, 12, 2, 2, MATERN, (), 0, C, S, EDGE_GD_1))
    cases.append(EdgeCase("ties", 0, 12, 2, 2, SE, (), 0, 256, 4, EDGE_GD_1))
    cases.append(EdgeCase("nan", 0, 12, 2, 2, MATERN, (), 0, 300, 3, EDGE_GD_1))
    return cases


def edge_id(c):
    return "%s-seed%d-n%d-d%d-E%d-C%d-S%d" % (c.kind, c.seed, c.n, c.d, c.E, c.C, c.S)


def edge_problem(case, dtype=LD):
    """(members, arrays, bounds, candidates) of an edge case: candidates uniform in [0.1, 0.9]^size"""
    members, a = make_ensemble(case.seed, case.n, case.d, case.E, case.cov, case.derivs, dtype=dtype)
    size = case.d - case.num_fidelity
    rng = np.random.default_rng(2000 + case.seed)
    cand = rng.uniform(0.1, 0.9, size=(case.C, size))
    return members, a, np.array([[0.0, 1.0]] * size), cand


def clamp_kinds(ens, gd, bounds, paths):
    """{True, False} over the steps of extended()'s paths: whether the clamp changed any coordinate of the step, with the smallest
    |a_i |grad f| - limit| met (the margin of that decision)"""
    bounds = np.asarray(bounds, dtype=np.float64).reshape(ens.size, 2)
    steps = step_sizes(gd)
    kinds, low = set(), np.inf
    for path in paths:
        for i in range(1, gd.max_num_steps + 1):
            x = path[i - 1]
            step = LD(steps[i - 1]) * ens.f(x[None, :], True)[1][0]
            limit = LD(gd.max_relative_change) * np.fmin(x - bounds[:, 0].astype(LD), bounds[:, 1].astype(LD) - x)
            kinds.add(bool(np.any(np.fabs(step) > limit)))
            low = min(low, float(np.min(np.abs(np.fabs(step) - limit))))
    return kinds, low


def ties_problem(case):
    """(members, arrays, bounds, candidates [256 + 128], the picks num_starts = 4 must give, their margins): behind the case's 256
    candidates 128 copies of the worst of them (never picked), among which one copy each of the second-best and of the third-best, in
    a slot that pm_select_kernel gives to a thread of another wavefront than the original's (index i belongs to thread i % 256)."""
    members, a, bounds, cand = edge_problem(case)
    fc = Ensemble(members, case.num_fidelity).f(cand)[0]
    order = top_indices(fc, len(fc))
    best, second, third = int(order[0]), int(order[1]), int(order[2])
    extra = np.repeat(cand[order[-1]:order[-1] + 1], 128, axis=0)

    def slot(i, k):
        return (64 if (i % 256) // 64 == 0 else 0) + k

    extra[slot(second, 1)] = cand[second]
    extra[slot(third, 2)] = cand[third]
    picks = [best, second, 256 + slot(second, 1), third]
    margins = [float(fc[order[k]] - fc[order[k + 1]]) for k in range(4)]
    return members, a, bounds, np.vstack([cand, extra]), picks, margins


def nan_problem(case, where):
    """(members, arrays, bounds, candidates with a NaN coordinate in candidate `where`, the starts among the others, margins at rank
    1 and at the cut among the others)"""
    members, a, bounds, cand = edge_problem(case)
    cand[where, -1] = np.nan
    keep = np.array([i for i in range(case.C) if i != where])
    fc = Ensemble(members, case.num_fidelity).f(cand[keep])[0]
    order = top_indices(fc, len(fc))
    margins = [float(fc[order[0]] - fc[order[1]]), float(fc[order[case.S - 1]] - fc[order[case.S]])]
    return members, a, bounds, cand, keep[order[:case.S]], margins
