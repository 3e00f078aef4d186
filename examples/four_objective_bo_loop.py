"""A four-objective Bayesian-optimisation loop on the device path: minimise the four squared distances f_k(x) = |x - c_k|^2 to the
corners of a square in [0, 1]^2, whose Pareto set is the square itself.  Four objectives are beyond the exact expected hypervolume
improvement (examples/three_objective_bo_loop.py stops at three); each iteration fits one GP ensemble per objective (a small fixed
spread of hyper-parameters stands for the chain that examples/bo_loop.py samples) and picks the next q points by the
ensemble-averaged Chebyshev-scalarised expected improvement, every point under a weight vector of its own, greedily, in one device
call (cornell_moe_amd/expected_scalarised_improvement.py -> moe_ei_chebyshev_mcmc_suggest, csrc/chebei1.hip).  Per iteration it
prints the number of non-dominated observations and a scalarised regret: over eight fixed weight vectors, the mean of the smallest
observed Chebyshev scalarisation minus its minimum over a 101 x 101 grid.

    python examples/four_objective_bo_loop.py [iterations] [q] [num_mcmc]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "tests"))  # the wrapper mirror is test infrastructure (tests/wrappers_mirror.py)
from cornell_moe_amd import expected_scalarised_improvement as esi  # noqa: E402
import wrappers_mirror as cw  # noqa: E402

CORNERS = np.array([(0.2, 0.2), (0.8, 0.2), (0.8, 0.8), (0.2, 0.8)])
IDEAL, NADIR = np.zeros(4), np.full(4, 0.72)  # a corner's own distance, and the distance between opposite corners


def objectives(x):
    return np.stack([np.sum((x - c) ** 2, axis=-1) for c in CORNERS], axis=-1)


def ensemble(X, values, hypers, noise):
    hd = cw.HistoricalData(dim=X.shape[1], num_derivatives=0)
    hd.append_sample_points([cw.SamplePoint(X[i], [values[i]], noise) for i in range(X.shape[0])])
    return cw.GaussianProcessMCMC(hypers, np.full((hypers.shape[0], 1), noise), hd, []).member_models()


def num_non_dominated(Y):
    return sum(1 for i in range(len(Y)) if not any(np.all(Y[j] <= Y[i]) and np.any(Y[j] < Y[i]) for j in range(len(Y))))


def scalarised_regret(Y, weights, grid_values):
    total = 0.0
    for w in weights:
        a, b = esi.chebyshev_scalarisation(w, IDEAL, NADIR)
        total += esi.chebyshev_best_so_far(Y, a, b) - esi.chebyshev_best_so_far(grid_values, a, b)
    return total / len(weights)


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    q = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    num_mcmc = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    rng = np.random.default_rng(0)
    dim, noise = 2, 1e-4
    X = rng.uniform(size=(8, dim))
    Y = objectives(X)
    bounds = [[0.0, 1.0]] * dim
    gd = (40, 20, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    spread = np.exp(0.2 * rng.standard_normal((num_mcmc, 1 + dim)))
    axis = np.linspace(0.0, 1.0, 101)
    grid_values = objectives(np.stack(np.meshgrid(axis, axis), axis=-1).reshape(-1, 2))
    test_weights = esi.sample_simplex_weights(8, 4, 1234)
    print("initially %d observations, %d non-dominated, scalarised regret %.4f" % (
        len(Y), num_non_dominated(Y), scalarised_regret(Y, test_weights, grid_values)))
    for it in range(iterations):
        t0 = time.perf_counter()
        models = [ensemble(X, Y[:, k], np.array([1.0, 0.5, 0.5]) * spread, noise) for k in range(4)]
        nxt, values, found = esi.multistart_chebyshev_expected_improvement_optimization(
            models, IDEAL, NADIR, bounds, gd, 40, num_to_sample=q, seed=it)
        t1 = time.perf_counter()
        got = objectives(nxt)
        X, Y = np.vstack([X, nxt]), np.vstack([Y, got])
        print("iteration %d: %.2f s; suggested %s (acquisition %s, found=%s); %d of %d observations non-dominated; scalarised regret %.4f" % (
            it, t1 - t0, np.round(nxt, 3).tolist(), np.round(values, 5).tolist(), found.tolist(), num_non_dominated(Y), len(Y),
            scalarised_regret(Y, test_weights, grid_values)), flush=True)
    return Y


if __name__ == "__main__":
    main()
