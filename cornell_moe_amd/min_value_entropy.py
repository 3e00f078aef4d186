"""The min-value entropy acquisition GIBBON averaged over a hyper-parameter ensemble, as an optimiser's objective and as a whole
suggestion.

GIBBON (Moss, Leslie, Gonzalez & Rayson, JMLR 2021) is the max-value entropy search of Wang & Jegelka (2017) in the form that stays
right under observation noise and for batches; here for minimisation.  Its input besides the GPs is a set of samples of the global
minimum VALUE per ensemble member, ``min_values`` [E][K]: ``sample_min_values`` draws them as the minima of joint posterior draws at
a candidate set.  The value, its gradient, the multistart ascent and greedy batches of q > 1 points are one library call each
(csrc/gibbon1.hip).  ``points_being_sampled`` names experiments that are running: each member's covariance is conditioned on them and
the value gains 1/2 log of the conditioned over the unconditioned predictive variance -- the exact greedy increment of GIBBON's batch
term, which tends to minus infinity at a noise-free pending point, so a greedy batch does not re-pick its own points (plain max-value
entropy search, whose value depends on (mu - m) / sigma alone, would).

``MinValueEntropyMCMC`` carries the method names ``AnalyticExpectedImprovementMCMC`` carries.
``multistart_min_value_entropy_optimization`` is the whole suggestion.
"""
import numpy as np

from .expected_improvement_analytic import _member_list
from .posterior_mean_mcmc import _device_members


def sample_min_values(models, candidates, num_samples, seed):
    """[E][num_samples] samples of the minimum value per member of ``models``: per member ONE ``sample_points`` call, num_samples joint
    posterior draws of the function values at ``candidates`` [C][dim] from ``api.normal_draws(seed + member, num_samples * C)``
    normals, and the minimum of every draw's row.  This is the minimum over the CANDIDATE SET: an upper bound of the minimum over the
    domain that tightens as the set grows (a denser set or one that holds the posterior mean's minimisers gives sharper values)."""
    from . import api
    members = _member_list(_device_members(models))
    cand = np.ascontiguousarray(candidates, dtype=np.float64).reshape(-1, int(members[0].d))
    D, C_ = int(num_samples), cand.shape[0]
    out = np.empty((len(members), D))
    for e, gp in enumerate(members):
        normals = api.normal_draws(int(seed) + e, D * C_).reshape(D, C_)
        out[e] = gp.sample_points(cand, normals)[0].min(axis=1)
    return out


def _observed_points(models, dim):
    """the sampled points of the GPs behind ``models`` from whichever layer keeps them ([0][dim] where none does)"""
    first = models
    try:
        first = list(models)[0]
    except TypeError:
        pass
    for obj in (first, getattr(first, "_gaussian_process", None), models):
        for name in ("_points_sampled", "_X"):
            X = getattr(obj, name, None)
            if X is not None:
                return np.asarray(X, dtype=np.float64).reshape(-1, dim)
    return np.zeros((0, dim))


class MinValueEntropyMCMC(object):
    def __init__(self, models, min_values, points_being_sampled=None, points_to_sample=None):
        self._models = models
        self._members = _device_members(models)
        num = len(_member_list(self._members))
        self._dim = int(_member_list(self._members)[0].d)
        self._min_values = np.ascontiguousarray(np.asarray(min_values, dtype=np.float64).reshape(num, -1))
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
    def min_values(self):
        return np.copy(self._min_values)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def evaluate_at_point_list(self, points, want_grad=False):
        """value [C] of points [C][dim] in one device call; with want_grad (value, grad [C][dim])"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.gibbon_ensemble(self._members, points, self._min_values, points_being_sampled=self._points_being_sampled,
                                   want_grad=want_grad)

    def compute_min_value_entropy(self):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_min_value_entropy

    def compute_grad_min_value_entropy(self):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_min_value_entropy

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the min-value entropy acquisition.')


def multistart_min_value_entropy_optimization(models, bounds, gd_params, num_multistarts=None, starts=None, num_to_sample=1,
                                              points_being_sampled=None, min_values=None, num_min_values=64, candidates=None, seed=0):
    """``num_to_sample`` points under the ensemble ``models`` (whatever posterior_mean_mcmc._device_members accepts): the multistart
    gradient ascent of the ensemble-averaged min-value entropy acquisition from ``starts`` [S][dim], or from ``num_multistarts``
    Latin-hypercube starts in ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``); q > 1 points are picked greedily, each round
    conditioned on ``points_being_sampled`` and on the points picked before, in one device call.  ``min_values`` [E][K] defaults to
    ``sample_min_values(models, candidates, num_min_values, seed)``; ``candidates`` [C][dim] defaults to 100 dim Latin-hypercube points
    (at most 2000, seed + 1) joined with the observed points where the GP objects keep them.  Returns (points [q][dim], values [q],
    found [q])."""
    from . import api
    members = _device_members(models)
    dim = int(_member_list(members)[0].d)
    if starts is None:
        if num_multistarts is None:
            raise ValueError("give num_multistarts or starts")
        starts = api.latin_hypercube(seed, bounds, num_multistarts)
    if min_values is None:
        if candidates is None:
            candidates = np.vstack([api.latin_hypercube(int(seed) + 1, bounds, min(100 * dim, 2000)), _observed_points(models, dim)])
        min_values = sample_min_values(models, candidates, num_min_values, seed)
    res = api.gibbon_suggest(members, gd_params, bounds, min_values, starts, num_to_sample, points_being_sampled=points_being_sampled)
    return res["points"], res["values"], res["found"]
