"""The LOG of the two- and of the three-objective expected hypervolume improvement, with or without constraints, averaged over a
hyper-parameter ensemble, as an optimiser's objective and as a whole suggestion.

The plain forms (expected_hypervolume_improvement.py, expected_hypervolume_improvement_constrained.py) multiply two or three psi
factors and K probabilities of feasibility in float64.  Wherever a candidate's posterior mean lies a few dozen posterior standard
deviations above the reference point in any one objective -- a tight reference point, a small-noise GP near its own observations --
or one constraint is far from feasible, the product and its gradient are exactly 0: every start of the ascent ties at 0 and none
moves, and the suggestion is whichever start the tie rule prefers.  The log of the same quantity is finite with a useful gradient
for every finite input (csrc/logehvi1.hip: a log-sum-exp over the strips of the front and over the members; csrc/logehvi3.hip: over
the boxes of the member's table); where the plain form does not underflow, exp of the value is the plain value.  Fronts, pending points and the believed-feasibility rule are the plain
constrained form's.

``LogExpectedHypervolumeImprovementMCMC`` carries the method names the two plain classes carry
(``compute_expected_hypervolume_improvement`` returns the log);
``multistart_log_expected_hypervolume_improvement_optimization`` is the whole suggestion.  ``LogExpectedHypervolumeImprovement3MCMC``
and ``multistart_log_expected_hypervolume_improvement_3_optimization`` are the same for three objectives.  Derivative observations
and simplex domains are not built.
"""
import numpy as np

from .expected_hypervolume_improvement_constrained import (ConstrainedExpectedHypervolumeImprovementMCMC, _default_front, _front_of)
from .posterior_mean_mcmc import _device_members

LIMIT = "the log expected hypervolume improvement is built for two objectives: %d ensembles given"
LIMIT3 = "the three-objective log expected hypervolume improvement takes three objectives: %d ensembles given"


class LogExpectedHypervolumeImprovementMCMC(ConstrainedExpectedHypervolumeImprovementMCMC):
    """objective_models: a list of 2 ensembles (whatever posterior_mean_mcmc._device_members accepts), as many members each;
    reference_point [2]; front [F][2] (any set of FEASIBLE outcomes: its Pareto front inside the reference point is taken; default:
    the feasible front of the first member's own observations); constraint_models: a list of K <= 8 such ensembles (None or empty:
    none), constraint k satisfied where c_k(x) <= thresholds[k].  The method names of ExpectedHypervolumeImprovementMCMC; every
    value is the LOG of the plain form's."""

    def __init__(self, objective_models, reference_point, front=None, points_being_sampled=None, constraint_models=None,
                 thresholds=None):
        objective_models = list(objective_models)
        if len(objective_models) != 2:
            raise ValueError(LIMIT % len(objective_models))
        super(LogExpectedHypervolumeImprovementMCMC, self).__init__(objective_models, constraint_models, thresholds, reference_point,
                                                                    front=front, points_being_sampled=points_being_sampled)

    def evaluate_at_point_list(self, points, want_grad=False, want_log_factors=False):
        """log value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_log_factors the
        members' log hypervolume terms and log feasibility factors [E][1 + K][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.log_ehvi_constrained_ensemble(self._objectives, self._constraints, self._thresholds, self._reference_point,
                                                 self._front, points, points_being_sampled=self._points_being_sampled,
                                                 want_grad=want_grad, want_log_factors=want_log_factors)

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the log expected hypervolume improvement.')


def multistart_log_expected_hypervolume_improvement_optimization(objective_models, reference_point, bounds, gd_params,
                                                                 num_multistarts, num_to_sample=1, points_being_sampled=None,
                                                                 front=None, constraint_models=None, thresholds=None, starts=None,
                                                                 seed=0):
    """``num_to_sample`` points under the two objectives' (and the constraints') ensembles: the multistart gradient ascent of the
    log of the ensemble-averaged (constrained) expected hypervolume improvement from ``num_multistarts`` Latin-hypercube starts in
    ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``), or from ``starts`` [S][dim]; q > 1 points are picked greedily, each
    round conditioned on ``points_being_sampled`` and on the points picked before, in one device call.  ``front`` [F][2] defaults to
    the feasible front of the first member's own observations.  Returns (points [q][dim], values [q], found [q]); the values are
    logs."""
    from . import api
    objective_models = list(objective_models)
    if len(objective_models) != 2:
        raise ValueError(LIMIT % len(objective_models))
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    constraint_models = [] if constraint_models is None else list(constraint_models)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    tau = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    fr = _default_front(objective_models, constraint_models, tau, ref) if front is None else _front_of(front, ref)
    res = api.log_ehvi_constrained_suggest([_device_members(m) for m in objective_models],
                                           [_device_members(m) for m in constraint_models], tau, ref, fr, gd_params, bounds, starts,
                                           num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]


class LogExpectedHypervolumeImprovement3MCMC(ConstrainedExpectedHypervolumeImprovementMCMC):
    """LogExpectedHypervolumeImprovementMCMC for three objectives: objective_models a list of 3 ensembles, reference_point [3], front
    [F][3] (default: the feasible three-objective front of the first member's own observations).  Every value is the LOG of the
    plain form's."""

    def __init__(self, objective_models, reference_point, front=None, points_being_sampled=None, constraint_models=None,
                 thresholds=None):
        objective_models = list(objective_models)
        if len(objective_models) != 3:
            raise ValueError(LIMIT3 % len(objective_models))
        super(LogExpectedHypervolumeImprovement3MCMC, self).__init__(objective_models, constraint_models, thresholds, reference_point,
                                                                     front=front, points_being_sampled=points_being_sampled)

    def evaluate_at_point_list(self, points, want_grad=False, want_log_factors=False):
        """log value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_log_factors the
        members' log hypervolume terms and log feasibility factors [E][1 + K][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.log_ehvi3_constrained_ensemble(self._objectives, self._constraints, self._thresholds, self._reference_point,
                                                  self._front, points, points_being_sampled=self._points_being_sampled,
                                                  want_grad=want_grad, want_log_factors=want_log_factors)

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the log expected hypervolume improvement.')


def multistart_log_expected_hypervolume_improvement_3_optimization(objective_models, reference_point, bounds, gd_params,
                                                                   num_multistarts, num_to_sample=1, points_being_sampled=None,
                                                                   front=None, constraint_models=None, thresholds=None, starts=None,
                                                                   seed=0):
    """multistart_log_expected_hypervolume_improvement_optimization for three objectives: ``front`` [F][3] defaults to the feasible
    three-objective front of the first member's own observations.  Returns (points [q][dim], values [q], found [q]); the values
    are logs."""
    from . import api
    objective_models = list(objective_models)
    if len(objective_models) != 3:
        raise ValueError(LIMIT3 % len(objective_models))
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    constraint_models = [] if constraint_models is None else list(constraint_models)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    tau = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    fr = _default_front(objective_models, constraint_models, tau, ref) if front is None else _front_of(front, ref)
    res = api.log_ehvi3_constrained_suggest([_device_members(m) for m in objective_models],
                                            [_device_members(m) for m in constraint_models], tau, ref, fr, gd_params, bounds, starts,
                                            num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
