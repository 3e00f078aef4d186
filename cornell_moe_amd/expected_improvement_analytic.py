"""The analytic one-point expected improvement averaged over a hyper-parameter ensemble, as an optimiser's objective and as a whole
suggestion.

At q = 1 the expected improvement of a GP has a closed form (the reference's OnePotentialSampleExpectedImprovementEvaluator); the
reference averages it member after member on the host.  Here the ensemble mean, its gradient, the multistart ascent and greedy
batches of q > 1 points are one library call each (csrc/ei1.hip).  ``points_being_sampled`` names experiments that are running: each
member's posterior covariance is conditioned on them, its posterior mean is left alone, and the believed values min_j mu_e(P_j)
join the member's best value (the Kriging-believer fantasy of csrc/kg1_pending.hip), so a greedy batch does not re-pick its own
points.  The GPs may carry derivative observations (the same list in every member): a pending point is then believed to return its
value and those derivatives, 1 + num_derivatives rows of at most 64, and the best value defaults to the minimum of the observed
FUNCTION values.

``AnalyticExpectedImprovementMCMC`` carries the method names python_version/optimization.py's GradientDescentOptimizer calls
(``problem_size``, ``current_point``, ``compute_objective_function``, ``compute_grad_objective_function``), the way
``DiscreteKnowledgeGradient`` does.  ``multistart_analytic_expected_improvement_optimization`` is the whole suggestion; its points
are also a deterministic source of ``shared_points`` for ``discretisation.kg_discrete_points``.
"""
import numpy as np

from .knowledge_gradient_discrete import _observed_values
from .posterior_mean_mcmc import _device_members


def _member_list(members):
    return list(members.gps) if hasattr(members, "gps") else list(members)


def _default_best(models):
    """per member the minimum of the member's observed values"""
    try:
        return [float(np.min(_observed_values(m))) for m in models]
    except TypeError:  # (an ensemble object: every member saw the same values)
        return [float(np.min(_observed_values(models)))] * len(_member_list(_device_members(models)))


class AnalyticExpectedImprovementMCMC(object):
    def __init__(self, models, best_so_far=None, points_being_sampled=None, points_to_sample=None):
        self._models = models
        self._members = _device_members(models)
        num = len(_member_list(self._members))
        self._dim = int(_member_list(self._members)[0].d)
        best = _default_best(models) if best_so_far is None else best_so_far
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
    def best_so_far(self):
        return np.copy(self._best_so_far)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def evaluate_at_point_list(self, points, want_grad=False):
        """ei [C] of points [C][dim] in one device call; with want_grad (ei, grad [C][dim])"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.ei_analytic_ensemble(self._members, points, self._best_so_far, points_being_sampled=self._points_being_sampled,
                                        want_grad=want_grad)

    def compute_expected_improvement(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_improvement

    def compute_grad_expected_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the expected improvement.')


def multistart_analytic_expected_improvement_optimization(models, bounds, gd_params, num_multistarts=None, starts=None, num_to_sample=1,
                                                          points_being_sampled=None, best_so_far=None, seed=0):
    """``num_to_sample`` points under the ensemble ``models`` (whatever posterior_mean_mcmc._device_members accepts): the multistart
    gradient ascent of the ensemble-averaged analytic expected improvement from ``starts`` [S][dim], or from ``num_multistarts``
    Latin-hypercube starts in ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``); q > 1 points are picked greedily, each round
    conditioned on ``points_being_sampled`` and on the points picked before, in one device call.  ``best_so_far`` [E] defaults per
    member to the minimum of the member's observed values.  Returns (points [q][dim], values [q], found [q])."""
    from . import api
    members = _device_members(models)
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    best = _default_best(models) if best_so_far is None else best_so_far
    best = np.broadcast_to(np.asarray(best, dtype=np.float64).ravel(), (len(_member_list(members)),))
    res = api.ei_analytic_suggest(members, gd_params, bounds, best, starts, num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
