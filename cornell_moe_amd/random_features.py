"""The reference's moe/optimal_learning/python/random_features.py in this repository's terms: samples of the GP's global minimiser
from posterior function paths.

The construction differs from the reference's.  The reference draws the weights of a random-feature model from their weight-space
posterior (its own M x M or n x n system).  Here a path is a random-feature draw of the PRIOR corrected by pathwise conditioning on
the factor the device GP holds (cornell_moe_amd/posterior_paths.py, include/moe_hip.h: moe_gp_paths_minimize), which is exact in the
mean for any number of features.  Both are draws of an approximate posterior function followed by its minimisation from the best
point of a grid; draw-for-draw agreement with the reference is not claimed, and the reference's other two functions
(sample_gp_with_random_features, global_optimization_of_GP_approximation) are the two halves of the one device call here.
"""
import numpy as np

from .posterior_paths import PosteriorPaths

# moe_gd_params_t's order: num_multistarts, max_num_steps, max_num_restarts, num_steps_averaged, gamma, pre_mult, max_relative_change,
# tolerance
DEFAULT_GD = (1, 40, 2, 3, 0.0, 1.0, 0.2, 1.0e-9)


def sample_from_global_optima(gp, nFeatures, domain_bounds, grid, nPoints, seed=0, gd_params=DEFAULT_GD):
    """nPoints samples [nPoints][dim] of the global minimiser of ``gp`` (an api.DeviceGP or a GP object that carries one) over
    domain_bounds [dim][2]: nPoints posterior paths of nFeatures random features, each screened at ``grid`` [G][dim] and minimised
    from its best grid point on the device.  The paths are built by pathwise conditioning, not by the reference's weight-space draw;
    see the module's docstring."""
    paths = PosteriorPaths([gp], int(nFeatures), int(nPoints), seed)
    res = paths.minimize(np.asarray(domain_bounds, dtype=np.float64), gd_params, grid)
    return np.ascontiguousarray(res["best_points"][0])
