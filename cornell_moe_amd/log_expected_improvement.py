"""The log of the expected improvement, with or without unknown constraints, averaged over a hyper-parameter ensemble, as an
optimiser's objective and as a whole suggestion.

After a few dozen observations most of the box has a small posterior variance and a mean well above the incumbent.  There
c = (best - mu) / sigma lies below -38, Phi(c) and phi(c) are exactly 0 in float64, and the expected improvement and its gradient
are exactly 0: every start of an ascent ties, none moves, and the "suggestion" is one of the starts.  With constraints one region
that looks infeasible zeroes the whole product.  The log of the same quantity (Ament et al., NeurIPS 2023, "Unexpected
improvements to expected improvement"),
    L_e(x) = log EI_e(x) + sum_k log Phi((thresholds[k] - mu_{e,k}(x)) / sigma_{e,k}(x)),   value = log mean_e exp L_e,
is computed without forming the quantities that underflow (csrc/logcei1.hip) and is finite with a useful gradient everywhere.
With one member and no constraint it has the maximiser of the expected improvement; under an ensemble or with constraints it is
the log of the very quantity ``expected_improvement_analytic`` / ``expected_improvement_constrained`` maximise.  Pending points,
greedy batches, derivative observations and the believed-feasible incumbent are those modules', unchanged.

``LogExpectedImprovementMCMC`` carries the method names ``ConstrainedExpectedImprovementMCMC`` carries.
``multistart_log_expected_improvement_optimization`` is the whole suggestion.
"""
import numpy as np

from .expected_improvement_analytic import _member_list
from .expected_improvement_constrained import _constraint_members, _default_best, best_feasible_value  # noqa: F401
from .posterior_mean_mcmc import _device_members


def _thresholds(thresholds):
    return np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()


class LogExpectedImprovementMCMC(object):
    """models: the objective's ensemble (whatever posterior_mean_mcmc._device_members accepts); best_so_far [E] (or one number):
    the best feasible value per member, +inf for none; it defaults to best_feasible_value of the members' own observations.
    constraint_models: K ensembles of as many members with thresholds [K]; None: no constraints, the log of the analytic expected
    improvement."""

    def __init__(self, models, best_so_far=None, points_being_sampled=None, constraint_models=None, thresholds=None,
                 points_to_sample=None):
        self._models, self._constraint_models = models, constraint_models
        self._members = _device_members(models)
        self._constraint_members = _constraint_members(constraint_models)
        self._thresholds = _thresholds(thresholds)
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

    def evaluate_at_point_list(self, points, want_grad=False, want_log_factors=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_log_factors the
        log factors [E][1 + K][C] (the log improvement factor, then the log probabilities of feasibility) as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.log_ei_constrained_ensemble(self._members, self._constraint_members, self._thresholds, points, self._best_so_far,
                                               points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                               want_log_factors=want_log_factors)

    def log_probability_of_feasibility(self, points):
        """the log of the ensemble mean of prod_k F_{e,k} at points [C][dim]"""
        logs = np.sum(self.evaluate_at_point_list(points, want_log_factors=True)[1][:, 1:, :], axis=1)
        top = np.max(logs, axis=0)
        return top + np.log(np.mean(np.exp(logs - top[None, :]), axis=0))

    def probability_of_feasibility(self, points):
        """the ensemble mean of prod_k F_{e,k} at points [C][dim]"""
        return np.exp(self.log_probability_of_feasibility(points))

    def compute_expected_improvement(self, force_monte_carlo=False):
        """the LOG of the ensemble-averaged (constrained) expected improvement at the current point"""
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_improvement

    def compute_grad_expected_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the log expected improvement.')


def multistart_log_expected_improvement_optimization(models, bounds, gd_params, num_multistarts=None, starts=None, num_to_sample=1,
                                                     points_being_sampled=None, constraint_models=None, thresholds=None,
                                                     best_so_far=None, seed=0):
    """``num_to_sample`` points under the objective's ensemble ``models`` (and the K constraint ensembles ``constraint_models`` with
    ``thresholds`` [K], if any): the multistart gradient ascent of the log of the ensemble-averaged (constrained) expected
    improvement from ``starts`` [S][dim], or from ``num_multistarts`` Latin-hypercube starts in ``bounds`` [dim][2]
    (moe_latin_hypercube with ``seed``); q > 1 points are picked greedily, each round conditioned on ``points_being_sampled`` and on
    the points picked before, in one device call.  ``best_so_far`` [E] defaults per member to the best feasible observed value
    (+inf if none is feasible).  Returns (points [q][dim], values [q], found [q])."""
    from . import api
    members = _device_members(models)
    num = len(_member_list(members))
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    tau = _thresholds(thresholds)
    best = _default_best(models, constraint_models, tau, num) if best_so_far is None else best_so_far
    best = np.broadcast_to(np.asarray(best, dtype=np.float64).ravel(), (num,))
    res = api.log_ei_constrained_suggest(members, _constraint_members(constraint_models), tau, gd_params, bounds, best, starts,
                                         num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
