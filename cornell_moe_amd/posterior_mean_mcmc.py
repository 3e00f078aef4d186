"""The posterior mean averaged over a hyper-parameter ensemble, and the recommendation step built on it, each as ONE device call.

``PosteriorMeanMCMC`` carries the interface of the reference's class of the same name
(python/cpp_wrappers/knowledge_gradient_mcmc.py:25-157): the objective is -(mean over the ensemble of the posterior mean) with the
fidelity coordinates pinned to 1.  The reference answers with one ``C_GP.compute_posterior_mean`` call per member; here
``compute_posterior_mean_mcmc`` and ``compute_grad_posterior_mean_mcmc`` are one ``moe_posterior_mean_mcmc_batch`` call each,
whatever the ensemble size.

``recommend_point`` is examples/main.py:142-157 / :243-260: evaluate the objective at the candidates, take the best, run the Python
gradient descent of python_version/optimization.py from it, keep the candidate unless the descent did at least as well -- on the
device, in one call (``moe_posterior_mean_mcmc_recommend``).
"""
import numpy as np

from . import api


def _device_members(models):
    """The device GPs behind `models`: an api.DeviceGPMCMC, a GPP.GaussianProcessMCMC, or a sequence of api.DeviceGP,
    GPP.GaussianProcess or wrapper-class GPs (their C-level object in ``._gaussian_process``)."""
    inner = getattr(models, "_dev", models)
    if isinstance(inner, api.DeviceGPMCMC):
        return inner
    out = []
    for m in models:
        m = getattr(m, "_gaussian_process", m)
        out.append(getattr(m, "_dev", m))
    return out


class PosteriorMeanMCMC(object):
    def __init__(self, gaussian_process_list, num_fidelity, points_to_sample=None, randomness=None):
        self._gaussian_process_list = gaussian_process_list
        self._members = _device_members(gaussian_process_list)
        self._num_fidelity = int(num_fidelity)
        first = self._members.gps[0] if isinstance(self._members, api.DeviceGPMCMC) else self._members[0]
        self._dim = first.d
        self._points_to_sample = np.zeros((1, self._dim)) if points_to_sample is None else np.copy(np.atleast_2d(points_to_sample))
        self._randomness = randomness  # (the reference builds a RandomnessSourceContainer it never draws from)
        self.objective_type = None

    @property
    def dim(self):
        return self._dim

    @property
    def problem_size(self):
        return self.dim - self._num_fidelity

    def get_current_point(self):
        return np.copy(self._points_to_sample)

    def set_current_point(self, points_to_sample):
        self._points_to_sample = np.copy(np.atleast_2d(points_to_sample))

    current_point = property(get_current_point, set_current_point)

    def _point(self):
        return self._points_to_sample.ravel()[:self.problem_size].reshape(1, self.problem_size)

    def compute_posterior_mean_mcmc(self, force_monte_carlo=False):
        return float(api.posterior_mean_mcmc(self._members, self._point(), self._num_fidelity)[0])

    compute_objective_function = compute_posterior_mean_mcmc

    def compute_grad_posterior_mean_mcmc(self, force_monte_carlo=False):
        return api.posterior_mean_mcmc(self._members, self._point(), self._num_fidelity, want_grad=True)[1].reshape(1, self.problem_size)

    compute_grad_objective_function = compute_grad_posterior_mean_mcmc

    def compute_hessian_objective_function(self, **kwargs):
        raise NotImplementedError('Currently we cannot compute the hessian of the posterior mean.')


def recommend_point(models, search_domain_bounds, candidates, gd_parameters, num_fidelity=0, num_starts=1):
    """The recommended point [dim]: the free coordinates from the device recommendation, the fidelity coordinates appended as ones
    (main.py:265-266).  search_domain_bounds [dim - num_fidelity][2]; candidates [C][dim - num_fidelity]; gd_parameters: an object
    with the GradientDescentParameters fields (max_num_steps, num_steps_averaged, gamma, pre_mult, max_relative_change) or the
    8-tuple api.DeviceGP._gd takes."""
    if hasattr(gd_parameters, "max_num_steps"):
        g = gd_parameters
        gd_parameters = (getattr(g, "num_multistarts", 1), g.max_num_steps, getattr(g, "max_num_restarts", 1), g.num_steps_averaged,
                         g.gamma, g.pre_mult, g.max_relative_change, getattr(g, "tolerance", 0.0))
    res = api.recommend(_device_members(models), candidates, gd_parameters, search_domain_bounds, num_fidelity=num_fidelity,
                        num_starts=num_starts)
    return np.concatenate((res["point"], np.ones(int(num_fidelity))))
