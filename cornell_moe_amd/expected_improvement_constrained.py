"""Expected improvement under unknown constraints, averaged over a hyper-parameter ensemble, as an optimiser's objective and as a
whole suggestion.

An experiment that returns, beside the value to minimise, K constraint values c_1 .. c_K (a budget, a temperature limit, a "did not
diverge" score) is modelled by 1 + K GPs per hyper-sample: the objective's and one per constraint, constraint k being satisfied
where c_k(x) <= thresholds[k].  The acquisition is the expected improvement over the best FEASIBLE value times the probability of
feasibility (Schonlau, Welch & Jones 1998; Gardner et al. 2014; Gelbart, Snoek & Adams 2014),
    A_e(x) = EI_e(x) prod_k Phi((thresholds[k] - mu_{e,k}(x)) / sigma_{e,k}(x)),
averaged over the members; its value, its gradient, the multistart ascent and greedy batches of q > 1 points are one library call
each (csrc/cei1.hip).  Before any observation is feasible the best value is +inf and a member's acquisition is its probability of
feasibility alone: the search looks for the feasible region first.  ``points_being_sampled`` names experiments that are running:
every GP's posterior covariance is conditioned on them, the means are left alone, and a pending point's believed objective value
joins a member's best value only where that member believes the point feasible.

``ConstrainedExpectedImprovementMCMC`` carries the method names ``AnalyticExpectedImprovementMCMC`` carries.
``multistart_constrained_expected_improvement_optimization`` is the whole suggestion; ``best_feasible_value`` is the incumbent.
"""
import numpy as np

from .expected_improvement_analytic import _member_list
from .knowledge_gradient_discrete import _observed_values
from .posterior_mean_mcmc import _device_members


def best_feasible_value(objective_values, constraint_values, thresholds):
    """The smallest of objective_values [n] among the observations whose constraint_values [n][K] (or [n] with one constraint)
    satisfy constraint_values[i][k] <= thresholds[k] for every k; +inf if none does."""
    y = np.asarray(objective_values, dtype=np.float64)
    y = y.reshape(y.shape[0], -1)[:, 0] if y.ndim > 1 else y.ravel()
    tau = np.asarray(thresholds, dtype=np.float64).ravel()
    c = np.asarray(constraint_values, dtype=np.float64).reshape(y.shape[0], -1) if tau.size else np.zeros((y.shape[0], 0))
    if c.shape[1] != tau.size:
        raise ValueError("one threshold per constraint column: %d columns, %d thresholds" % (c.shape[1], tau.size))
    feasible = np.all(c <= tau[None, :], axis=1)
    return float(np.min(y[feasible])) if feasible.any() else float("inf")


def _constraint_members(constraint_models):
    return [] if constraint_models is None else [_device_members(c) for c in constraint_models]


def _default_best(models, constraint_models, thresholds, num):
    """per member the best feasible observed value, from GP objects that keep their observations (objective and constraints observed
    at the same points, in the same order)"""
    def values(ensemble):
        try:
            return [_observed_values(m) for m in ensemble]
        except TypeError:  # (an ensemble object: every member saw the same values)
            return [_observed_values(ensemble)] * num
    ys = values(models)
    cs = [values(c) for c in ([] if constraint_models is None else constraint_models)]
    return [best_feasible_value(ys[e], np.stack([c[e] for c in cs], axis=1) if cs else np.zeros((len(ys[e]), 0)), thresholds)
            for e in range(num)]


class ConstrainedExpectedImprovementMCMC(object):
    """models: the objective's ensemble (whatever posterior_mean_mcmc._device_members accepts); constraint_models: K such ensembles
    of as many members; thresholds [K]; best_so_far [E] (or one number): the best feasible value per member, +inf for none; it
    defaults to best_feasible_value of the members' own observations."""

    def __init__(self, models, constraint_models, thresholds, best_so_far=None, points_being_sampled=None, points_to_sample=None):
        self._models, self._constraint_models = models, constraint_models
        self._members = _device_members(models)
        self._constraint_members = _constraint_members(constraint_models)
        self._thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).ravel()
        num = len(_member_list(self._members))
        self._dim = int(_member_list(self._members)[0].d)
        best = _default_best(models, constraint_models, self._thresholds, num) if best_so_far is None else best_so_far
        self._best_so_far = np.ascontiguousarray(np.broadcast_to(np.asarray(best, dtype=np.float64).ravel(), (num,)))
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
    def num_constraints(self):
        return len(self._constraint_members)

    @property
    def best_so_far(self):
        return np.copy(self._best_so_far)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def evaluate_at_point_list(self, points, want_grad=False, want_factors=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_factors the factors
        [E][1 + K][C] (the improvement factor, then the probabilities of feasibility) as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.ei_constrained_ensemble(self._members, self._constraint_members, self._thresholds, points, self._best_so_far,
                                           points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                           want_factors=want_factors)

    def probability_of_feasibility(self, points):
        """the ensemble mean of prod_k F_{e,k} at points [C][dim]"""
        factors = self.evaluate_at_point_list(points, want_factors=True)[1]
        return np.mean(np.prod(factors[:, 1:, :], axis=1), axis=0)

    def compute_expected_improvement(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_improvement

    def compute_grad_expected_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the constrained expected improvement.')


def multistart_constrained_expected_improvement_optimization(models, constraint_models, thresholds, bounds, gd_params,
                                                             num_multistarts=None, starts=None, num_to_sample=1,
                                                             points_being_sampled=None, best_so_far=None, seed=0):
    """``num_to_sample`` points under the objective's ensemble ``models`` and the K constraint ensembles ``constraint_models``: the
    multistart gradient ascent of the ensemble-averaged constrained expected improvement from ``starts`` [S][dim], or from
    ``num_multistarts`` Latin-hypercube starts in ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``); q > 1 points are picked
    greedily, each round conditioned on ``points_being_sampled`` and on the points picked before, in one device call.
    ``best_so_far`` [E] defaults per member to the best feasible observed value (+inf if none is feasible).  Returns (points
    [q][dim], values [q], found [q])."""
    from . import api
    members = _device_members(models)
    num = len(_member_list(members))
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    best = _default_best(models, constraint_models, thresholds, num) if best_so_far is None else best_so_far
    best = np.broadcast_to(np.asarray(best, dtype=np.float64).ravel(), (num,))
    res = api.ei_constrained_suggest(members, _constraint_members(constraint_models), thresholds, gd_params, bounds, best, starts,
                                     num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
