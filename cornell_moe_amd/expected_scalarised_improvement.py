"""The Chebyshev-scalarised expected improvement for two to eight objectives, averaged over a hyper-parameter ensemble, as an
optimiser's objective and as a whole suggestion.

An experiment that returns M values to minimise is modelled by M GPs per hyper-sample.  The exact expected hypervolume improvement
stops at three objectives (expected_hypervolume_improvement.py): its box count grows like F^(M/2).  The classic answer for many
objectives is ParEGO (Knowles 2006), in its modern form qParEGO (Daulton, Balandat & Bakshy 2020): pick weights w on the simplex,
fold the objectives into the weighted Chebyshev scalarisation

    g(y) = max_j w_j (y_j - ideal_j) / (nadir_j - ideal_j) = max_j (a_j y_j + b_j)

and maximise the expected improvement of g over the smallest g observed so far; fresh weights for every point of a batch spread
the batch over the front.  Here the scalarisation is applied to the MODEL OUTPUTS, and at one point, with an independent GP per
objective, the expected improvement is a one-dimensional integral of a product of normal CDFs that a fixed quadrature evaluates
to rounding (csrc/chebei1.hip): no Monte Carlo.  Its value, its gradient, the multistart ascent and greedy batches are one library
call each; the cost is linear in M.  ``points_being_sampled`` names experiments that are running: all M GPs' posterior covariances
are conditioned on them, the means are left alone, and every member's incumbent takes the scalarised outcome it believes.

``ChebyshevExpectedImprovementMCMC`` carries the method names ``ExpectedHypervolumeImprovement3MCMC`` carries.
``multistart_chebyshev_expected_improvement_optimization`` is the whole suggestion.
"""
import numpy as np

from .expected_improvement_analytic import _member_list
from .knowledge_gradient_discrete import _observed_values
from .posterior_mean_mcmc import _device_members


def chebyshev_scalarisation(weights, ideal_point, nadir_point):
    """(a [M], b [M]) of the weighted Chebyshev scalarisation max_j (a_j y_j + b_j): a_j = w_j / (nadir_j - ideal_j), b_j = -a_j
    ideal_j.  The weights must be positive and the nadir point strictly above the ideal point."""
    w = np.asarray(weights, dtype=np.float64).ravel()
    lo = np.asarray(ideal_point, dtype=np.float64).ravel()
    hi = np.asarray(nadir_point, dtype=np.float64).ravel()
    if not (w.size == lo.size == hi.size):
        raise ValueError("weights, ideal_point and nadir_point must have one entry per objective: %d, %d, %d" % (w.size, lo.size, hi.size))
    if not (np.all(np.isfinite(w)) and np.all(w > 0.0)):
        raise ValueError("the weights must be positive and finite")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError("the nadir point must lie strictly above the ideal point, both finite")
    a = w / (hi - lo)
    return a, -a * lo


def chebyshev_best_so_far(objective_values, a, b):
    """The incumbent: the smallest max_j (a_j y_j + b_j) over the observed outcomes objective_values [n][M] (rows with a value
    that is not finite are left out; +inf is never returned: without a finite row a ValueError is raised)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    y = np.asarray(objective_values, dtype=np.float64).reshape(-1, a.size)
    g = np.max(a[None, :] * y + b[None, :], axis=1)
    g = g[np.isfinite(g)]
    if g.size == 0:
        raise ValueError("no observed outcome is finite: there is no incumbent")
    return float(np.min(g))


def sample_simplex_weights(num, num_objectives, seed):
    """num weight vectors [num][num_objectives], uniform on the simplex (normalised exponentials), reproducible from the seed; every
    weight is at least 1e-3 before normalising, so that no objective is switched off."""
    rng = np.random.RandomState(int(seed))
    w = np.maximum(rng.exponential(size=(int(num), int(num_objectives))), 1e-3)
    return w / np.sum(w, axis=1, keepdims=True)


def _objective_members(objective_models):
    return [_device_members(m) for m in objective_models]


def _observed_outcomes(objective_models):
    """per member the observed outcomes [n][M] of its M models (observed at the same points, in the same order)"""
    per_objective = []
    for models in objective_models:
        try:
            ys = [_observed_values(m) for m in models]
        except TypeError:  # (an ensemble object: every member saw the same values)
            ys = [_observed_values(models)] * len(_member_list(_device_members(models)))
        per_objective.append(ys)
    E = len(per_objective[0])
    out = []
    for e in range(E):
        ys = [np.asarray(per_objective[j][e], dtype=np.float64).ravel() for j in range(len(per_objective))]
        if len(set(y.size for y in ys)) != 1:
            raise ValueError("the default incumbent needs every objective observed at the same points: %s values" % [y.size for y in ys])
        out.append(np.stack(ys, axis=1))
    return out


class ChebyshevExpectedImprovementMCMC(object):
    """objective_models: the M objectives' ensembles (each whatever posterior_mean_mcmc._device_members accepts), as many members
    each; weights, ideal_point, nadir_point [M] (chebyshev_scalarisation); best_so_far [E] or one number: the members' incumbents,
    by default every member's smallest scalarised observation.  The method names of ExpectedHypervolumeImprovement3MCMC."""

    def __init__(self, objective_models, weights, ideal_point, nadir_point, best_so_far=None, points_being_sampled=None,
                 points_to_sample=None):
        self._members = _objective_members(objective_models)
        self._a, self._b = chebyshev_scalarisation(weights, ideal_point, nadir_point)
        self._dim = int(_member_list(self._members[0])[0].d)
        num = len(_member_list(self._members[0]))
        if best_so_far is None:
            best_so_far = [chebyshev_best_so_far(y, self._a, self._b) for y in _observed_outcomes(objective_models)]
        self._best_so_far = np.ascontiguousarray(np.broadcast_to(np.asarray(best_so_far, dtype=np.float64).ravel(), (num,)))
        self._points_to_sample = np.zeros((1, self._dim)) if points_to_sample is None else np.copy(np.atleast_2d(points_to_sample))
        self._points_being_sampled = (np.zeros((0, self._dim)) if points_being_sampled is None else
                                      np.ascontiguousarray(points_being_sampled, dtype=np.float64).reshape(-1, self._dim))
        self.objective_type = None

    @property
    def dim(self):
        return self._dim

    @property
    def problem_size(self):
        return self._dim

    @property
    def scalarisation(self):
        return np.copy(self._a), np.copy(self._b)

    @property
    def best_so_far(self):
        return np.copy(self._best_so_far)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def evaluate_at_point_list(self, points, want_grad=False, want_member_values=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_member_values the
        members' own values [E][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.ei_chebyshev_ensemble(self._members, np.concatenate([self._a, self._b]), self._best_so_far, points,
                                         points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                         want_member_values=want_member_values)

    def compute_expected_improvement(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_improvement

    def compute_grad_expected_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the scalarised expected improvement.')


def multistart_chebyshev_expected_improvement_optimization(objective_models, ideal_point, nadir_point, bounds, gd_params,
                                                           num_multistarts, num_to_sample=1, points_being_sampled=None, weights=None,
                                                           seed=0):
    """``num_to_sample`` points under the M objectives' ensembles: the multistart gradient ascent of the ensemble-averaged
    Chebyshev-scalarised expected improvement from ``num_multistarts`` Latin-hypercube starts in ``bounds`` [dim][2]
    (moe_latin_hypercube with ``seed``).  Point t has its own weight vector ``weights[t]`` [M] -- with ``weights=None`` one vector
    per point is drawn by sample_simplex_weights from ``seed`` -- and its own incumbents, every member's smallest scalarised
    observation under those weights; q > 1 points are picked greedily, each round conditioned on ``points_being_sampled`` and on
    the points picked before, whose believed outcomes lower the members' incumbents, in one device call.  Returns (points
    [q][dim], values [q], found [q])."""
    from . import api
    q = int(num_to_sample)
    M = len(list(objective_models))
    w = sample_simplex_weights(q, M, seed) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1, M)
    if w.shape[0] != q:
        raise ValueError("one weight vector per point: %d for %d points" % (w.shape[0], q))
    outcomes = _observed_outcomes(objective_models)
    scal, best = [], []
    for t in range(q):
        a, b = chebyshev_scalarisation(w[t], ideal_point, nadir_point)
        scal.append(np.concatenate([a, b]))
        best.append([chebyshev_best_so_far(y, a, b) for y in outcomes])
    starts = api.latin_hypercube(seed, bounds, num_multistarts)
    res = api.ei_chebyshev_suggest(_objective_members(objective_models), np.array(scal), np.array(best), gd_params, bounds, starts, q,
                                   points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]


# ---- the log form, constrained too (csrc/logchebei1.hip) ----
def feasible_chebyshev_best_so_far(objective_values, constraint_values, thresholds, a, b):
    """The incumbent of the FEASIBLE observations: chebyshev_best_so_far over the rows of objective_values [n][M] whose
    constraint_values [n][K] satisfy constraint_values[i][k] <= thresholds[k] for every k.  The log form integrates up to its
    incumbent, so the incumbent must be finite: where no observation is feasible the cap is the LARGEST finite scalarised
    observation -- every outcome better than the worst seen then counts as an improvement, and the probabilities of feasibility
    steer the search towards the feasible region."""
    a = np.asarray(a, dtype=np.float64).ravel()
    tau = np.asarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    y = np.asarray(objective_values, dtype=np.float64).reshape(-1, a.size)
    if tau.size == 0:
        return chebyshev_best_so_far(y, a, b)
    con = np.asarray(constraint_values, dtype=np.float64).reshape(-1, tau.size)
    if con.shape[0] != y.shape[0]:
        raise ValueError("the feasible incumbent needs objectives and constraints observed at the same points: %d and %d rows" % (
            y.shape[0], con.shape[0]))
    feasible = np.all(con <= tau[None, :], axis=1)
    g = np.max(a[None, :] * y + np.asarray(b, dtype=np.float64).ravel()[None, :], axis=1)
    if np.any(feasible & np.isfinite(g)):
        return float(np.min(g[feasible & np.isfinite(g)]))
    g = g[np.isfinite(g)]
    if g.size == 0:
        raise ValueError("no observed outcome is finite: there is no incumbent")
    return float(np.max(g))


def _feasible_incumbents(objective_models, constraint_models, thresholds, a, b):
    """per member the incumbent of its feasible observations (the constraints observed where the objectives are)"""
    outcomes = _observed_outcomes(objective_models)
    if not constraint_models:
        return [chebyshev_best_so_far(y, a, b) for y in outcomes]
    constraints = _observed_outcomes(constraint_models)
    return [feasible_chebyshev_best_so_far(y, c, thresholds, a, b) for y, c in zip(outcomes, constraints)]


class LogChebyshevExpectedImprovementMCMC(ChebyshevExpectedImprovementMCMC):
    """The LOG of ChebyshevExpectedImprovementMCMC's quantity times the probabilities of feasibility of K <= 8 constraints
    (constraint_models: K ensembles shaped like the objectives', constraint k satisfied where c_k(x) <= thresholds[k]; None: none),
    under the ensemble's log-sum-exp: finite with a useful gradient where the plain form is exactly 0.  best_so_far defaults to
    every member's smallest scalarised FEASIBLE observation (feasible_chebyshev_best_so_far)."""

    def __init__(self, objective_models, weights, ideal_point, nadir_point, best_so_far=None, points_being_sampled=None,
                 constraint_models=None, thresholds=None, points_to_sample=None):
        self._constraints = [] if constraint_models is None else _objective_members(constraint_models)
        self._thresholds = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
        if self._thresholds.size != len(self._constraints):
            raise ValueError("one threshold per constraint: %d for %d" % (self._thresholds.size, len(self._constraints)))
        if best_so_far is None:
            a, b = chebyshev_scalarisation(weights, ideal_point, nadir_point)
            best_so_far = _feasible_incumbents(objective_models, constraint_models, self._thresholds, a, b)
        super(LogChebyshevExpectedImprovementMCMC, self).__init__(objective_models, weights, ideal_point, nadir_point,
                                                                  best_so_far=best_so_far, points_being_sampled=points_being_sampled,
                                                                  points_to_sample=points_to_sample)

    @property
    def num_constraints(self):
        return len(self._constraints)

    def evaluate_at_point_list(self, points, want_grad=False, want_factors=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_factors the groups'
        own logs [E][1 + K][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.log_ei_chebyshev_constrained_ensemble(self._members, self._constraints, self._thresholds,
                                                         np.concatenate([self._a, self._b]), self._best_so_far, points,
                                                         points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                                         want_factors=want_factors)


def multistart_log_chebyshev_expected_improvement_optimization(objective_models, ideal_point, nadir_point, bounds, gd_params,
                                                               num_multistarts, num_to_sample=1, points_being_sampled=None,
                                                               weights=None, seed=0, constraint_models=None, thresholds=None):
    """multistart_chebyshev_expected_improvement_optimization by the log form, with constraints: the same starts, weights and greedy
    rounds; every round's incumbents come from the FEASIBLE observations only, and a pick lowers a member's incumbent only where
    that member believes it feasible.  Returns (points [q][dim], values [q], found [q]); the values are logs."""
    from . import api
    q = int(num_to_sample)
    M = len(list(objective_models))
    w = sample_simplex_weights(q, M, seed) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1, M)
    if w.shape[0] != q:
        raise ValueError("one weight vector per point: %d for %d points" % (w.shape[0], q))
    scal, best = [], []
    for t in range(q):
        a, b = chebyshev_scalarisation(w[t], ideal_point, nadir_point)
        scal.append(np.concatenate([a, b]))
        best.append(_feasible_incumbents(objective_models, constraint_models, thresholds, a, b))
    starts = api.latin_hypercube(seed, bounds, num_multistarts)
    cons = None if not constraint_models else _objective_members(constraint_models)
    res = api.log_ei_chebyshev_constrained_suggest(_objective_members(objective_models), cons, thresholds, np.array(scal),
                                                   np.array(best), gd_params, bounds, starts, q,
                                                   points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
