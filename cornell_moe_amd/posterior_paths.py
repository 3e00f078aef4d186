"""Posterior function paths of a GP ensemble and what their minimisers give: Thompson-sampling batches and samples of the global
minimum value for GIBBON.

A path is one posterior draw AS A FUNCTION of x, by pathwise conditioning (Wilson et al. 2020) on the factor each member already
holds (include/moe_hip.h: moe_gp_paths_evaluate): a random-feature draw of the prior plus the kernel-weighted correction that makes
it agree with the data.  It costs O(M + n) per evaluation and has a gradient, so its minimiser over the domain is found by the line
search that ``api.minimize_member_means`` runs on the posterior mean (csrc/paths.hip), where ``sample_points`` and
``sample_global_optima`` are tied to a candidate set of a few thousand points.

Everything random enters through tables (``draw_path_tables``): the same seed gives the same paths.
"""
import numpy as np

from . import _lib
from .expected_improvement_analytic import _member_list
from .posterior_mean_mcmc import _device_members


def draw_path_tables(cov_type, dim, n, num_members, num_features, num_paths, seed):
    """The tables of moe_gp_paths_evaluate / moe_gp_paths_minimize: a dict of frequencies [M][dim] (unit scale: standard normals for
    the squared exponential, standard normals divided by sqrt(u / 5), u ~ chi^2_5 as the sum of five squared normals, for Matern-5/2:
    the spectral density is a multivariate t with 5 degrees of freedom), phases [M] uniform on [0, 2 pi), weights [E][S][M] and
    noise_normals [E][S][n].  Normals are api.normal_draws(seed + k, .), k = 0 frequencies, 1 the chi^2 draws, 2 weights, 3 noise
    normals; phases come from numpy.random.default_rng(seed)."""
    from . import api
    M, S, E, dim, n, seed = int(num_features), int(num_paths), int(num_members), int(dim), int(n), int(seed)
    freq = api.normal_draws(seed, M * dim).reshape(M, dim)
    if int(cov_type) == _lib.COV_MATERN_NU_2P5:
        u = np.sum(api.normal_draws(seed + 1, 5 * M).reshape(M, 5) ** 2, axis=1)
        freq = freq / np.sqrt(u / 5.0)[:, None]
    elif int(cov_type) != _lib.COV_SQUARE_EXPONENTIAL:
        raise ValueError("no spectral density for cov_type %r" % (cov_type,))
    phases = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, size=M)
    weights = api.normal_draws(seed + 2, E * S * M).reshape(E, S, M)
    noise_normals = api.normal_draws(seed + 3, E * S * n).reshape(E, S, n)
    return dict(frequencies=np.ascontiguousarray(freq), phases=phases, weights=weights, noise_normals=noise_normals)


class PosteriorPaths(object):
    """``num_paths`` posterior function paths of every member of ``models`` (whatever posterior_mean_mcmc._device_members accepts; the
    members share the sampled points and the covariance type and have no derivative observations), from ``num_features`` random
    features."""

    def __init__(self, models, num_features, num_paths, seed=0):
        self._members = _device_members(models)
        gps = _member_list(self._members)
        self._dim, self._n = int(gps[0].d), int(gps[0].n)
        self.cov_type = int(getattr(gps[0], "cov_type", _lib.COV_MATERN_NU_2P5))
        self.tables = draw_path_tables(self.cov_type, self._dim, self._n, len(gps), num_features, num_paths, seed)

    @property
    def dim(self):
        return self._dim

    def _args(self):
        t = self.tables
        return t["frequencies"], t["phases"], t["weights"], t["noise_normals"]

    def evaluate(self, points, want_grad=False):
        """values [E][S][C] of points [C][dim]; with want_grad (values, grad [E][S][C][dim])"""
        from . import api
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self._dim)
        return api.paths_evaluate(self._members, *self._args(), points, want_grad=want_grad)

    def minimize(self, bounds, gd_params, candidates, **kwargs):
        """api.paths_minimize's dict: every path screened at candidates [C][dim] and minimised from its best one"""
        from . import api
        candidates = np.ascontiguousarray(candidates, dtype=np.float64).reshape(-1, self._dim)
        return api.paths_minimize(self._members, *self._args(), gd_params, bounds, candidates, **kwargs)


def _candidates(models, bounds, dim, num_candidates, seed):
    """Latin-hypercube points followed by the sampled points where the GP objects keep them"""
    from . import api
    from .min_value_entropy import _observed_points
    return np.vstack([api.latin_hypercube(int(seed) + 4, bounds, int(num_candidates)), _observed_points(models, dim)])


def thompson_sampling_batch(models, bounds, gd_params, num_to_sample, num_candidates=2000, num_features=1024, seed=0):
    """``num_to_sample`` points, each the minimiser over ``bounds`` [dim][2] of its own posterior path: ceil(q / E) paths per member
    of ``models`` are drawn and minimised in one device call, and the first q minimisers taken in (path, member) order.  Returns
    (points [q][dim], values [q]: each path's value at its minimiser)."""
    gps = _member_list(_device_members(models))
    q, E = int(num_to_sample), len(gps)
    paths = PosteriorPaths(models, num_features, -(-q // E), seed)
    res = paths.minimize(bounds, gd_params, _candidates(models, bounds, paths.dim, num_candidates, seed))
    points = np.swapaxes(res["best_points"], 0, 1).reshape(-1, paths.dim)[:q]
    values = np.swapaxes(res["best_values"], 0, 1).ravel()[:q]
    return np.ascontiguousarray(points), np.ascontiguousarray(values)


def sample_min_values_from_paths(models, bounds, gd_params, num_samples, num_candidates=2000, num_features=1024, seed=0,
                                 candidates=None):
    """[E][num_samples] samples of the global minimum VALUE per member: the minima over the domain of num_samples posterior paths per
    member, each found by the line search from the best of ``candidates`` (default: num_candidates Latin-hypercube points followed by
    the sampled points).  What min_value_entropy.sample_min_values bounds from above on its candidate set; accepted as ``min_values=``
    by MinValueEntropyMCMC and multistart_min_value_entropy_optimization."""
    paths = PosteriorPaths(models, num_features, num_samples, seed)
    if candidates is None:
        candidates = _candidates(models, bounds, paths.dim, num_candidates, seed)
    return np.ascontiguousarray(paths.minimize(bounds, gd_params, candidates)["best_values"])
