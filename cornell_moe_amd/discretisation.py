"""The per-member discretisation of a KG-MCMC iteration as ONE device call.

The reference's examples/main.py:172-197 builds, for every member of the hyper-parameter ensemble, the discrete set the knowledge
gradient is taken over: it evaluates the member's posterior mean at some thousand candidate points (one ``compute_posterior_mean``
call each), starts the C++ line-search optimiser (``posterior_mean_optimization``) from the best of them, keeps the start if the
optimiser ended worse, and appends the result to the points all members share.  ``member_posterior_mean_minima`` is that procedure
for all members at once (``moe_posterior_mean_members_minimize``); ``kg_discrete_points`` returns main.py's ``discrete_pts_list``.
"""
import numpy as np

from . import api
from .posterior_mean_mcmc import _device_members


def _gd_tuple(gd_params):
    if hasattr(gd_params, "max_num_steps"):
        g = gd_params
        return (getattr(g, "num_multistarts", 1), g.max_num_steps, getattr(g, "max_num_restarts", 1),
                getattr(g, "num_steps_averaged", 0), g.gamma, g.pre_mult, g.max_relative_change, getattr(g, "tolerance", 0.0))
    return gd_params


def member_posterior_mean_minima(models, candidates, bounds, gd_params, num_fidelity=0, want_means=False, want_trace=False):
    """api.minimize_member_means for `models`: an api.DeviceGPMCMC, a GPP.GaussianProcessMCMC, or a sequence of device or wrapper
    GPs over the same data.  candidates [C][dim - num_fidelity] (shared) or [E][C][dim - num_fidelity] (per member); bounds
    [dim - num_fidelity][2]; gd_params: an object with the GradientDescentParameters fields or the 8-tuple api.DeviceGP._gd takes."""
    return api.minimize_member_means(_device_members(models), candidates, _gd_tuple(gd_params), bounds, num_fidelity=num_fidelity,
                                     want_means=want_means, want_trace=want_trace)


def kg_discrete_points(models, shared_points, candidates, bounds, gd_params, num_fidelity=0):
    """main.py's ``discrete_pts_list``: per member the array [shared_points ; that member's posterior-mean minimiser], shape
    (len(shared_points) + 1, dim - num_fidelity).  A deterministic source of ``shared_points``:
    expected_improvement_analytic.multistart_analytic_expected_improvement_optimization(models, ..., num_to_sample=10)."""
    res = member_posterior_mean_minima(models, candidates, bounds, gd_params, num_fidelity=num_fidelity)
    best = res["best_points"]
    shared = np.asarray(shared_points, dtype=np.float64).reshape(-1, best.shape[1])
    return [np.concatenate((shared, best[e:e + 1]), axis=0) for e in range(best.shape[0])]
