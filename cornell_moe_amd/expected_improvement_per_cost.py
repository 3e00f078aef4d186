"""The log of the (constrained) expected improvement per unit cost, averaged over a hyper-parameter ensemble, as an optimiser's
objective and as a whole suggestion.

Every other acquisition here assumes that an evaluation costs the same wherever it is made.  Where the cost depends strongly on the
point (depth, batch size, step count of a model being tuned) and is itself unknown and noisy, the standard answer is the expected
improvement per unit cost (Snoek, Larochelle & Adams, NeurIPS 2012, "EI per second") with the LOG of the cost modelled by a GP of
its own, and cost-cooling (Lee et al. 2020), which raises the expected cost to an exponent alpha that is lowered towards 0 as the
budget runs out.  Under a log-normal cost E[cost] = exp(mu_c + var_c / 2), so per member
    L_e(x) = log EI_e(x) + sum_k log Phi((thresholds[k] - mu_{e,k}(x)) / sigma_{e,k}(x)) - alpha (mu_{e,c}(x) + var_{e,c}(x) / 2),
    value = log mean_e exp L_e
(csrc/logeipc1.hip): ``log_expected_improvement``'s quantity with one more additive role.  It has the maximiser of the plain
ensemble mean of EI_e F_e / E[cost_e]^alpha and does not underflow.  Pending points condition every GP's covariance, the cost GP's
too; greedy batches, derivative observations and the believed-feasible incumbent are ``log_expected_improvement``'s, unchanged,
and the cost GP takes no part in the incumbent.

``LogExpectedImprovementPerCostMCMC`` carries the method names ``LogExpectedImprovementMCMC`` carries, plus ``cost_exponent``.
``multistart_log_expected_improvement_per_cost_optimization`` is the whole suggestion; ``predicted_cost`` the expected cost at
points; ``cost_cooling_exponent`` the exponent's schedule.
"""
import numpy as np

from .expected_improvement_analytic import _member_list
from .expected_improvement_constrained import _constraint_members, _default_best
from .log_expected_improvement import LogExpectedImprovementMCMC, _thresholds
from .posterior_mean_mcmc import _device_members


class LogExpectedImprovementPerCostMCMC(LogExpectedImprovementMCMC):
    """models, best_so_far, points_being_sampled, constraint_models, thresholds: LogExpectedImprovementMCMC's.  cost_models: an
    ensemble of as many members, GPs of the LOG of the evaluation cost; cost_exponent: alpha >= 0 (1: per unit cost, 0: the cost
    plays no part)."""

    def __init__(self, models, cost_models, cost_exponent=1.0, best_so_far=None, points_being_sampled=None, constraint_models=None,
                 thresholds=None, points_to_sample=None):
        super(LogExpectedImprovementPerCostMCMC, self).__init__(models, best_so_far=best_so_far,
                                                                points_being_sampled=points_being_sampled,
                                                                constraint_models=constraint_models, thresholds=thresholds,
                                                                points_to_sample=points_to_sample)
        self._cost_models = cost_models
        self._cost_members = _device_members(cost_models)
        self._cost_exponent = float(cost_exponent)

    @property
    def cost_exponent(self):
        return self._cost_exponent

    @cost_exponent.setter
    def cost_exponent(self, value):
        self._cost_exponent = float(value)

    def evaluate_at_point_list(self, points, want_grad=False, want_log_factors=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_log_factors the
        log factors [E][2 + K][C] (the log improvement factor, the log probabilities of feasibility, then the cost's term) as the
        last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.log_ei_per_cost_ensemble(self._members, self._constraint_members, self._thresholds, self._cost_members,
                                            self._cost_exponent, points, self._best_so_far,
                                            points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                            want_log_factors=want_log_factors)

    def log_probability_of_feasibility(self, points):
        """the log of the ensemble mean of prod_k F_{e,k} at points [C][dim]"""
        K = self.num_constraints
        logs = np.sum(self.evaluate_at_point_list(points, want_log_factors=True)[1][:, 1:1 + K, :], axis=1)
        top = np.max(logs, axis=0)
        return top + np.log(np.mean(np.exp(logs - top[None, :]), axis=0))

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the log expected improvement per unit cost.')


def multistart_log_expected_improvement_per_cost_optimization(models, cost_models, bounds, gd_params, num_multistarts=None,
                                                              starts=None, num_to_sample=1, points_being_sampled=None,
                                                              cost_exponent=1.0, constraint_models=None, thresholds=None,
                                                              best_so_far=None, seed=0):
    """``num_to_sample`` points under the objective's ensemble ``models``, the cost's ensemble ``cost_models`` (GPs of the LOG of the
    evaluation cost) and the K constraint ensembles, if any: multistart_log_expected_improvement_optimization with the log expected
    improvement per unit cost at ``cost_exponent`` as the objective.  Returns (points [q][dim], values [q], found [q])."""
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
    res = api.log_ei_per_cost_suggest(members, _constraint_members(constraint_models), tau, _device_members(cost_models), cost_exponent,
                                      gd_params, bounds, best, starts, num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]


def predicted_cost(cost_models, points):
    """The expected evaluation cost at points [C][dim] under GPs of the LOG cost: (the ensemble mean [C], the members' [E][C]) of
    exp(mu + std^2 / 2), from DeviceGP.mean_std.  No pending points."""
    members = _member_list(_device_members(cost_models))
    d = int(members[0].d)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, d)
    per_member = np.empty((len(members), points.shape[0]))
    for e, gp in enumerate(members):
        mean, std = gp.mean_std(points)
        per_member[e] = np.exp(mean + 0.5 * std * std)
    return np.mean(per_member, axis=0), per_member


def cost_cooling_exponent(spent, budget, spent_at_start=0.0):
    """Lee et al.'s schedule: clip((budget - spent) / (budget - spent_at_start), 0, 1) -- 1 when the optimisation starts, 0 once the
    budget is spent."""
    total = float(budget) - float(spent_at_start)
    if not total > 0.0:
        raise ValueError("the budget must exceed what was spent at the start")
    return float(np.clip((float(budget) - float(spent)) / total, 0.0, 1.0))
