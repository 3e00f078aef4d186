"""The constrained expected hypervolume improvement for two or three objectives, averaged over a hyper-parameter ensemble, as an
optimiser's objective and as a whole suggestion.

An experiment that returns two or three values to minimise AND values that must stay under limits (error against cost under a
memory limit, say) is modelled by M objective GPs and K constraint GPs per hyper-sample.  What is known so far is the Pareto front
of the FEASIBLE observed outcomes; the acquisition is the expected growth of its hypervolume when x is evaluated, times the
probability that x is feasible: EHVI(x) Pr[c_1(x) <= tau_1] ... Pr[c_K(x) <= tau_K] with independent constraint GPs (the
expected hypervolume improvement of expected_hypervolume_improvement.py under the constraint handling of
expected_improvement_constrained.py).  Its value, its gradient, the multistart ascent and greedy batches of q > 1 points are one
library call each (csrc/cehvi1.hip).  ``points_being_sampled`` names experiments that are running: every GP's posterior covariance
is conditioned on them, the means are left alone, and a member's own front takes the outcome it believes a point will return only
where it also believes that point feasible -- a pick the member believes infeasible does not shrink the region it still hopes to
gain.

``ConstrainedExpectedHypervolumeImprovementMCMC`` carries the method names ``ExpectedHypervolumeImprovementMCMC`` carries.
``multistart_constrained_expected_hypervolume_improvement_optimization`` is the whole suggestion; ``feasible_pareto_front`` is the
bookkeeping around it.  The log forms for two and for three objectives are log_expected_hypervolume_improvement.py;
derivative observations and four or more objectives are out of scope.
"""
import numpy as np

from .expected_hypervolume_improvement import pareto_front, pareto_front_3
from .expected_improvement_analytic import _member_list
from .knowledge_gradient_discrete import _observed_values
from .posterior_mean_mcmc import _device_members


def _front_of(values, reference_point):
    ref = np.asarray(reference_point, dtype=np.float64).ravel()
    if ref.size not in (2, 3):
        raise ValueError("two or three objectives: the reference point has %d coordinates" % ref.size)
    return (pareto_front if ref.size == 2 else pareto_front_3)(np.asarray(values, dtype=np.float64).reshape(-1, ref.size), ref)


def feasible_pareto_front(objective_values, constraint_values, thresholds, reference_point):
    """The Pareto front (minimisation) of the observations that satisfy every constraint: objective_values [n][M], M = 2 or 3 as
    reference_point has coordinates; constraint_values [n][K]; observation i is feasible where constraint_values[i][k] <=
    thresholds[k] for every k.  The result has pareto_front's form (M = 2) or pareto_front_3's (M = 3), strictly inside the
    reference point.  ValueError where the row counts or the number of thresholds do not fit."""
    ref = np.asarray(reference_point, dtype=np.float64).ravel()
    tau = np.asarray(thresholds, dtype=np.float64).ravel()
    obj = np.asarray(objective_values, dtype=np.float64).reshape(-1, max(ref.size, 1))
    con = np.asarray(constraint_values, dtype=np.float64).reshape(obj.shape[0] if tau.size == 0 else -1, tau.size)
    if con.shape[0] != obj.shape[0]:
        raise ValueError("the feasible front needs objectives and constraints observed at the same points: %d and %d rows" % (
            obj.shape[0], con.shape[0]))
    feasible = np.all(con <= tau[None, :], axis=1) if tau.size else np.ones(obj.shape[0], dtype=bool)
    return _front_of(obj[feasible], ref)


def _default_front(objective_models, constraint_models, thresholds, reference_point):
    """the feasible front of the outcomes the first member's M + K models have observed (at the same points, in the same order)"""
    def first(ensemble):
        try:
            return _observed_values(ensemble[0])
        except TypeError:  # (an ensemble object)
            return _observed_values(ensemble)
    ys = []
    for m in list(objective_models) + list(constraint_models):
        y = np.asarray(first(m), dtype=np.float64)
        ys.append(y.reshape(y.shape[0], -1)[:, 0])
    if len(set(y.size for y in ys)) != 1:
        raise ValueError("the default front needs the objectives and the constraints observed at the same points: %s values" % [
            y.size for y in ys])
    M = len(objective_models)
    n = ys[0].size
    con = np.stack(ys[M:], axis=1) if len(ys) > M else np.zeros((n, 0))
    return feasible_pareto_front(np.stack(ys[:M], axis=1), con, thresholds, reference_point)


class ConstrainedExpectedHypervolumeImprovementMCMC(object):
    """objective_models: a list of 2 or 3 ensembles (whatever posterior_mean_mcmc._device_members accepts), as many members each;
    constraint_models: a list of K <= 8 such ensembles (None or empty: none), constraint k satisfied where c_k(x) <=
    thresholds[k]; reference_point [M]; front [F][M] (any set of FEASIBLE outcomes: its Pareto front inside the reference point is
    taken); it defaults to the feasible front of the first member's own observations.  The method names of
    ExpectedHypervolumeImprovementMCMC."""

    def __init__(self, objective_models, constraint_models, thresholds, reference_point, front=None, points_being_sampled=None,
                 points_to_sample=None):
        objective_models = list(objective_models)
        constraint_models = [] if constraint_models is None else list(constraint_models)
        if len(objective_models) not in (2, 3):
            raise ValueError("two or three objectives: %d ensembles given" % len(objective_models))
        self._objectives = [_device_members(m) for m in objective_models]
        self._constraints = [_device_members(m) for m in constraint_models]
        self._thresholds = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
        self._reference_point = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
        if self._reference_point.size != len(objective_models):
            raise ValueError("one reference coordinate per objective: %d and %d" % (self._reference_point.size, len(objective_models)))
        self._dim = int(_member_list(self._objectives[0])[0].d)
        self._front = (_default_front(objective_models, constraint_models, self._thresholds, self._reference_point) if front is None
                       else _front_of(front, self._reference_point))
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
    def num_objectives(self):
        return len(self._objectives)

    @property
    def num_constraints(self):
        return len(self._constraints)

    @property
    def thresholds(self):
        return np.copy(self._thresholds)

    @property
    def reference_point(self):
        return np.copy(self._reference_point)

    @property
    def front(self):
        return np.copy(self._front)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def evaluate_at_point_list(self, points, want_grad=False, want_factors=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_factors the members'
        hypervolume terms and feasibility factors [E][1 + K][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.ehvi_constrained_ensemble(self._objectives, self._constraints, self._thresholds, self._reference_point, self._front,
                                             points, points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                             want_factors=want_factors)

    def compute_expected_hypervolume_improvement(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_hypervolume_improvement

    def compute_grad_expected_hypervolume_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_hypervolume_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the constrained expected hypervolume improvement.')


def multistart_constrained_expected_hypervolume_improvement_optimization(objective_models, constraint_models, thresholds,
                                                                         reference_point, bounds, gd_params, num_multistarts=None,
                                                                         starts=None, num_to_sample=1, points_being_sampled=None,
                                                                         front=None, seed=0):
    """``num_to_sample`` points under the objectives' and the constraints' ensembles: the multistart gradient ascent of the
    ensemble-averaged constrained expected hypervolume improvement from ``starts`` [S][dim], or from ``num_multistarts``
    Latin-hypercube starts in ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``); q > 1 points are picked greedily, each round
    conditioned on ``points_being_sampled`` and on the points picked before, whose believed outcomes join the fronts of the members
    that believe them feasible, in one device call.  ``front`` [F][M] defaults to the feasible front of the first member's own
    observations.  Returns (points [q][dim], values [q], found [q])."""
    from . import api
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    objective_models = list(objective_models)
    constraint_models = [] if constraint_models is None else list(constraint_models)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    tau = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    fr = _default_front(objective_models, constraint_models, tau, ref) if front is None else _front_of(front, ref)
    res = api.ehvi_constrained_suggest([_device_members(m) for m in objective_models], [_device_members(m) for m in constraint_models],
                                       tau, ref, fr, gd_params, bounds, starts, num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
