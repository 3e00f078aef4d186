"""The exact discretised one-point knowledge gradient as an optimiser's objective.

At q = 1 over a finite set A the knowledge gradient is the expectation of the minimum of |A| + 1 lines in one standard normal
(Frazier, Powell & Dayanik 2009), so it has a closed form where the reference only has Monte Carlo
(cpp_wrappers/knowledge_gradient.py: KnowledgeGradient with an inner line search per sample).  The value is deterministic and is
a lower bound of the continuous knowledge gradient the Monte-Carlo evaluators estimate: their inner minimum runs over the whole
domain, this one over {the candidate with its fidelity coordinates at 1} and A.

``DiscreteKnowledgeGradient`` carries the method names python_version/optimization.py's GradientDescentOptimizer calls
(``problem_size``, ``current_point``, ``compute_objective_function``, ``compute_grad_objective_function``), the way
``PosteriorMeanMCMC`` of this package does.  Every evaluation is one ``moe_gp_kg_discrete`` call (csrc/kg1.hip).

``multistart_discrete_knowledge_gradient_optimization`` is the whole suggestion under a hyper-parameter ensemble in one library
call (csrc/kg1_opt.hip): what the reference's examples/main.py asks ``gen_sample_from_qkg_mcmc`` for, deterministic; with
``num_to_sample`` = q > 1 the q points are picked greedily, and ``points_being_sampled`` names experiments that are running: the
posterior covariance is conditioned on the pending points, the posterior mean is not (csrc/kg1_pending.hip).
"""
import numpy as np


def _device_gp(gaussian_process):
    """the api.DeviceGP behind an api.DeviceGP, a GPP.GaussianProcess or a wrapper-class GP (its C-level object in
    ``._gaussian_process``)"""
    inner = getattr(gaussian_process, "_gaussian_process", gaussian_process)
    return getattr(inner, "_dev", inner)


def _observed_values(gaussian_process):
    """the observed function values of the GP, from whichever layer keeps them"""
    for obj in (gaussian_process, getattr(gaussian_process, "_gaussian_process", None)):
        for name in ("_points_sampled_value", "_y"):
            y = getattr(obj, name, None)
            if y is not None:
                y = np.asarray(y, dtype=np.float64)
                return y.reshape(y.shape[0], -1)[:, 0]
    raise ValueError("best_so_far=None needs a GP object that keeps its observed values; pass best_so_far")


class DiscreteKnowledgeGradient(object):
    def __init__(self, gaussian_process, discrete_pts, num_fidelity=0, best_so_far=None, points_to_sample=None,
                 points_being_sampled=None):
        self._gaussian_process = gaussian_process
        self._dev = _device_gp(gaussian_process)
        self._num_fidelity = int(num_fidelity)
        self._dim = int(self._dev.d)
        self._discrete_pts = np.ascontiguousarray(discrete_pts, dtype=np.float64).reshape(-1, self._dim - self._num_fidelity)
        self._best_so_far = float(np.min(_observed_values(gaussian_process))) if best_so_far is None else float(best_so_far)
        self._points_to_sample = np.zeros((1, self._dim)) if points_to_sample is None else np.copy(np.atleast_2d(points_to_sample))
        self._points_being_sampled = (np.zeros((0, self._dim)) if points_being_sampled is None else
                                      np.ascontiguousarray(points_being_sampled, dtype=np.float64).reshape(-1, self._dim))
        self.objective_type = None

    @property
    def dim(self):
        return self._dim

    @property
    def problem_size(self):
        return self._dim  # (the candidate moves in all its coordinates, the fidelity ones included, as the reference's q-KG point does)

    @property
    def best_so_far(self):
        return self._best_so_far

    @property
    def discrete_pts(self):
        return np.copy(self._discrete_pts)

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def evaluate_at_point_list(self, points, want_grad=False):
        """kg [C] of points [C][dim] in one device call; with want_grad (kg, grad [C][dim])"""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return self._dev.kg_discrete(self._discrete_pts, points, self._best_so_far, num_fidelity=self._num_fidelity,
                                     want_grad=want_grad, points_being_sampled=self._points_being_sampled)

    def compute_knowledge_gradient(self, force_monte_carlo=False):
        return float(self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim])[0])

    compute_objective_function = compute_knowledge_gradient

    def compute_grad_knowledge_gradient(self, force_monte_carlo=False):
        return self.evaluate_at_point_list(self._points_to_sample.ravel()[:self._dim], want_grad=True)[1].reshape(1, self._dim)

    compute_grad_objective_function = compute_grad_knowledge_gradient

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the knowledge gradient.')


def multistart_discrete_knowledge_gradient_optimization(gps, discrete_all, best_so_far_all, bounds, gd_params, num_multistarts, seed,
                                                        num_fidelity=0, num_to_sample=None, points_being_sampled=None):
    """The next point to sample under the ensemble ``gps`` (an api.DeviceGPMCMC, a list of api.DeviceGP or one api.DeviceGP): the
    multistart gradient ascent of the ensemble-averaged discretised knowledge gradient from ``num_multistarts`` Latin-hypercube
    starts in ``bounds`` [dim][2] (moe_latin_hypercube with ``seed``), member e over its own set discrete_all[e] and best value
    best_so_far_all[e].  Returns (point [dim], value, found).
    With ``num_to_sample`` = q or ``points_being_sampled`` [p][dim] given: q points greedily (api.kg_discrete_suggest), each round
    conditioned on the pending points and on the points picked before; returns (points [q][dim], values [q], found [q])."""
    from . import api
    starts = api.latin_hypercube(seed, bounds, num_multistarts)
    if num_to_sample is not None or points_being_sampled is not None:
        res = api.kg_discrete_suggest(gps, gd_params, bounds, discrete_all, best_so_far_all, starts,
                                      1 if num_to_sample is None else num_to_sample, num_fidelity=num_fidelity,
                                      points_being_sampled=points_being_sampled)
        return res["points"], res["values"], res["found"]
    res = api.kg_discrete_multistart(gps, gd_params, bounds, discrete_all, best_so_far_all, starts, num_fidelity=num_fidelity)
    return res["point"], res["value"], res["found"]
