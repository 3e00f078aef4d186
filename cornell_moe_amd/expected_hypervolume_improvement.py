"""The two-objective expected hypervolume improvement, averaged over a hyper-parameter ensemble, as an optimiser's objective and as a
whole suggestion.

An experiment that returns two values to minimise (error against cost, impurity against loss of yield) is modelled by two GPs per
hyper-sample.  What is known so far is the Pareto front of the observed outcomes, and its quality the hypervolume it dominates
inside a reference point r.  The acquisition is the expected growth of that hypervolume when x is evaluated (EHVI; Emmerich,
Giannakoglou & Naujoks 2006; Emmerich, Deutz & Klinkenberg 2011; Yang et al. 2019), which in two dimensions is an exact sum over
the front's F + 1 strips; its value, its gradient, the multistart ascent and greedy batches of q > 1 points are one library call
each (csrc/ehvi1.hip).  ``points_being_sampled`` names experiments that are running: both GPs' posterior covariances are
conditioned on them, the means are left alone, and every member's own front takes the outcome it believes the point will return.

``ExpectedHypervolumeImprovementMCMC`` carries the method names ``ConstrainedExpectedImprovementMCMC`` carries.
``multistart_expected_hypervolume_improvement_optimization`` is the whole suggestion; ``pareto_front`` and ``hypervolume`` are the
bookkeeping around it.

Three objectives (error, cost and latency, say) have the same four under the names ``pareto_front_3``, ``hypervolume_3``,
``ExpectedHypervolumeImprovement3MCMC`` and ``multistart_expected_hypervolume_improvement_3_optimization``: three GPs per
hyper-sample, and the quantity an exact sum over the boxes of the non-dominated region, cut into slabs by the third objective
(csrc/ehvi3.hip).  Four or more objectives: expected_scalarised_improvement.py.
"""
import numpy as np

from .expected_improvement_analytic import _member_list
from .knowledge_gradient_discrete import _observed_values
from .posterior_mean_mcmc import _device_members


def pareto_front(values, reference_point=None):
    """The non-dominated subset of values [n][2] (minimisation), sorted by the first objective ascending -- the second then descends
    strictly -- and, with reference_point [2], only the points strictly inside it.  Of equal points one is kept; of two points that
    tie in one objective the one better in the other."""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 2)
    if reference_point is not None:
        r = np.asarray(reference_point, dtype=np.float64).ravel()
        v = v[(v[:, 0] < r[0]) & (v[:, 1] < r[1])]
    v = v[np.all(np.isfinite(v), axis=1)]
    order = np.lexsort((v[:, 1], v[:, 0]))  # by the first objective, ties by the second
    out, best = [], np.inf
    for i in order:
        if v[i, 1] < best:  # (a point that ties the first objective of its predecessor has a larger or equal second: dropped)
            out.append(v[i])
            best = v[i, 1]
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def hypervolume(front, reference_point):
    """The area dominated by the points front [F][2] inside reference_point [2] (minimisation): points outside the reference point
    or dominated by others add nothing."""
    r = np.asarray(reference_point, dtype=np.float64).ravel()
    f = pareto_front(front, r)
    total, height = 0.0, r[1]
    for u, v in f:
        total += (r[0] - u) * (height - v)
        height = v
    return float(total)


def _default_front(models_1, models_2, reference_point):
    """the front of the outcomes the first member's two models have observed (observed at the same points, in the same order)"""
    def first(ensemble):
        try:
            return _observed_values(ensemble[0])
        except TypeError:  # (an ensemble object)
            return _observed_values(ensemble)
    y1, y2 = np.asarray(first(models_1), dtype=np.float64), np.asarray(first(models_2), dtype=np.float64)
    y1 = y1.reshape(y1.shape[0], -1)[:, 0]
    y2 = y2.reshape(y2.shape[0], -1)[:, 0]
    if y1.size != y2.size:
        raise ValueError("the default front needs both objectives observed at the same points: %d and %d values" % (y1.size, y2.size))
    return pareto_front(np.stack([y1, y2], axis=1), reference_point)


class ExpectedHypervolumeImprovementMCMC(object):
    """models_1, models_2: the two objectives' ensembles (whatever posterior_mean_mcmc._device_members accepts), as many members
    each; reference_point [2]; front [F][2] (any point set: its pareto_front inside the reference point is taken); it defaults to
    the front of the first member's own observations."""

    def __init__(self, models_1, models_2, reference_point, front=None, points_being_sampled=None, points_to_sample=None):
        self._members_1, self._members_2 = _device_members(models_1), _device_members(models_2)
        self._reference_point = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
        self._dim = int(_member_list(self._members_1)[0].d)
        self._front = (_default_front(models_1, models_2, self._reference_point) if front is None else
                       pareto_front(front, self._reference_point))
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

    def evaluate_at_point_list(self, points, want_grad=False, want_member_values=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_member_values the
        members' own values [E][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.ehvi_ensemble(self._members_1, self._members_2, self._reference_point, self._front, points,
                                 points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                 want_member_values=want_member_values)

    def compute_expected_hypervolume_improvement(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_hypervolume_improvement

    def compute_grad_expected_hypervolume_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_hypervolume_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the expected hypervolume improvement.')


def multistart_expected_hypervolume_improvement_optimization(models_1, models_2, reference_point, bounds, gd_params,
                                                             num_multistarts=None, starts=None, num_to_sample=1,
                                                             points_being_sampled=None, front=None, seed=0):
    """``num_to_sample`` points under the two objectives' ensembles ``models_1`` and ``models_2``: the multistart gradient ascent of
    the ensemble-averaged expected hypervolume improvement from ``starts`` [S][dim], or from ``num_multistarts`` Latin-hypercube
    starts in ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``); q > 1 points are picked greedily, each round conditioned on
    ``points_being_sampled`` and on the points picked before, whose believed outcomes join the members' fronts, in one device call.
    ``front`` [F][2] defaults to the front of the first member's own observations.  Returns (points [q][dim], values [q], found
    [q])."""
    from . import api
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    fr = _default_front(models_1, models_2, ref) if front is None else pareto_front(front, ref)
    res = api.ehvi_suggest(_device_members(models_1), _device_members(models_2), ref, fr, gd_params, bounds, starts, num_to_sample,
                           points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]


# ---- three objectives ----
def pareto_front_3(values, reference_point=None):
    """The non-dominated subset of values [n][3] (minimisation) in the canonical order of csrc/ehvi3.hip -- the third objective
    ascending, ties by the first, then by the second -- and, with reference_point [3], only the points strictly inside it.  Of
    equal points one is kept."""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 3)
    v = v[np.all(np.isfinite(v), axis=1)]
    if reference_point is not None:
        r = np.asarray(reference_point, dtype=np.float64).ravel()
        v = v[np.all(v < r[None, :], axis=1)]
    v = v[np.lexsort((v[:, 1], v[:, 0], v[:, 2]))]  # by the third objective, ties by the first, then by the second
    out = []
    for i in range(v.shape[0]):
        # a point <= v[i] in all three sorts before it or equals it; those kept so far cover those they dominate
        if not any(np.all(o <= v[i]) for o in out):
            out.append(v[i])
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def hypervolume_3(front, reference_point):
    """The volume dominated by the points front [F][3] inside reference_point [3] (minimisation): points outside the reference
    point or dominated by others add nothing.  Slab by slab in the third objective, each slab the area its points' projections
    dominate."""
    r = np.asarray(reference_point, dtype=np.float64).ravel()
    f = pareto_front_3(front, r)
    total = 0.0
    for k in range(f.shape[0]):
        upper = f[k + 1, 2] if k + 1 < f.shape[0] else r[2]
        if upper > f[k, 2]:
            total += hypervolume(f[:k + 1, :2], r[:2]) * (upper - f[k, 2])
    return float(total)


def _default_front_3(models, reference_point):
    """the front of the outcomes the first member's three models have observed (at the same points, in the same order)"""
    def first(ensemble):
        try:
            return _observed_values(ensemble[0])
        except TypeError:  # (an ensemble object)
            return _observed_values(ensemble)
    ys = []
    for m in models:
        y = np.asarray(first(m), dtype=np.float64)
        ys.append(y.reshape(y.shape[0], -1)[:, 0])
    if len(set(y.size for y in ys)) != 1:
        raise ValueError("the default front needs the three objectives observed at the same points: %s values" % [y.size for y in ys])
    return pareto_front_3(np.stack(ys, axis=1), reference_point)


class ExpectedHypervolumeImprovement3MCMC(object):
    """models_1, models_2, models_3: the three objectives' ensembles (whatever posterior_mean_mcmc._device_members accepts), as
    many members each; reference_point [3]; front [F][3] (any point set: its pareto_front_3 inside the reference point is taken);
    it defaults to the front of the first member's own observations.  The method names of ExpectedHypervolumeImprovementMCMC."""

    def __init__(self, models_1, models_2, models_3, reference_point, front=None, points_being_sampled=None, points_to_sample=None):
        self._members = [_device_members(m) for m in (models_1, models_2, models_3)]
        self._reference_point = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
        self._dim = int(_member_list(self._members[0])[0].d)
        self._front = (_default_front_3((models_1, models_2, models_3), self._reference_point) if front is None else
                       pareto_front_3(front, self._reference_point))
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

    def evaluate_at_point_list(self, points, want_grad=False, want_member_values=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim]); with want_member_values the
        members' own values [E][C] as the last item"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.ehvi3_ensemble(self._members[0], self._members[1], self._members[2], self._reference_point, self._front, points,
                                  points_being_sampled=self._points_being_sampled, want_grad=want_grad,
                                  want_member_values=want_member_values)

    def compute_expected_hypervolume_improvement(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_expected_hypervolume_improvement

    def compute_grad_expected_hypervolume_improvement(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_expected_hypervolume_improvement

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the expected hypervolume improvement.')


def multistart_expected_hypervolume_improvement_3_optimization(models_1, models_2, models_3, reference_point, bounds, gd_params,
                                                               num_multistarts=None, starts=None, num_to_sample=1,
                                                               points_being_sampled=None, front=None, seed=0):
    """``num_to_sample`` points under the three objectives' ensembles: multistart_expected_hypervolume_improvement_optimization
    with a third objective.  ``front`` [F][3] defaults to the front of the first member's own observations.  Returns (points
    [q][dim], values [q], found [q])."""
    from . import api
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    fr = _default_front_3((models_1, models_2, models_3), ref) if front is None else pareto_front_3(front, ref)
    res = api.ehvi3_suggest(_device_members(models_1), _device_members(models_2), _device_members(models_3), ref, fr, gd_params,
                            bounds, starts, num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
