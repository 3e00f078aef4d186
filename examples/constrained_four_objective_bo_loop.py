"""examples/four_objective_bo_loop.py inside a disc: minimise the four squared distances f_k(x) = |x - c_k|^2 to the corners of a
square in [0, 1]^2 subject to the unknown constraint c(x) = |x - (0.5, 0.5)|^2 - 0.09 <= 0, which cuts the corners off the Pareto
set.  Each iteration fits one GP ensemble per objective and one for the constraint and picks the next q points by the LOG
Chebyshev-scalarised expected improvement times the probability of feasibility, every point under a weight vector of its own,
greedily, in one device call (cornell_moe_amd/expected_scalarised_improvement.py -> moe_log_ei_chebyshev_constrained_mcmc_suggest,
csrc/logchebei1.hip); every round's incumbents come from the feasible observations only.  The log form keeps a gradient late in
the run, where the incumbents are good and the plain form is exactly 0 over most of the domain.  Per iteration it prints the
number of feasible observations and a scalarised regret over the feasible ones: over eight fixed weight vectors, the mean of the
smallest feasible observed Chebyshev scalarisation minus its minimum over the feasible part of a 101 x 101 grid.

    python examples/constrained_four_objective_bo_loop.py [iterations] [q] [num_mcmc]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "examples"))
from cornell_moe_amd import expected_scalarised_improvement as esi  # noqa: E402
import four_objective_bo_loop as plain  # noqa: E402

IDEAL, NADIR = plain.IDEAL, plain.NADIR
CENTRE, RADIUS2 = np.array([0.5, 0.5]), 0.09


def constraint(x):
    return np.sum((x - CENTRE) ** 2, axis=-1) - RADIUS2


def feasible_regret(Y, c, weights, grid_values):
    total = 0.0
    for w in weights:
        a, b = esi.chebyshev_scalarisation(w, IDEAL, NADIR)
        total += esi.feasible_chebyshev_best_so_far(Y, c[:, None], [0.0], a, b) - esi.chebyshev_best_so_far(grid_values, a, b)
    return total / len(weights)


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    q = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    num_mcmc = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    rng = np.random.default_rng(0)
    dim, noise = 2, 1e-4
    X = rng.uniform(size=(8, dim))
    X[0] = CENTRE + 0.1  # (one feasible observation to start from)
    Y, c = plain.objectives(X), constraint(X)
    bounds = [[0.0, 1.0]] * dim
    gd = (40, 20, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    spread = np.exp(0.2 * rng.standard_normal((num_mcmc, 1 + dim)))
    axis = np.linspace(0.0, 1.0, 101)
    grid = np.stack(np.meshgrid(axis, axis), axis=-1).reshape(-1, 2)
    grid_values = plain.objectives(grid[constraint(grid) <= 0.0])
    test_weights = esi.sample_simplex_weights(8, 4, 1234)
    print("initially %d observations, %d feasible, feasible scalarised regret %.4f" % (
        len(Y), int(np.sum(c <= 0.0)), feasible_regret(Y, c, test_weights, grid_values)))
    for it in range(iterations):
        t0 = time.perf_counter()
        hypers = np.array([1.0, 0.5, 0.5]) * spread
        models = [plain.ensemble(X, Y[:, k], hypers, noise) for k in range(4)]
        constraint_models = [plain.ensemble(X, c, hypers, noise)]
        nxt, values, found = esi.multistart_log_chebyshev_expected_improvement_optimization(
            models, IDEAL, NADIR, bounds, gd, 40, num_to_sample=q, seed=it, constraint_models=constraint_models, thresholds=[0.0])
        t1 = time.perf_counter()
        X, Y, c = np.vstack([X, nxt]), np.vstack([Y, plain.objectives(nxt)]), np.concatenate([c, constraint(nxt)])
        print("iteration %d: %.2f s; suggested %s (log acquisition %s, found=%s, feasible=%s); %d of %d observations feasible; "
              "feasible scalarised regret %.4f" % (it, t1 - t0, np.round(nxt, 3).tolist(), np.round(values, 3).tolist(), found.tolist(),
                                                   (constraint(nxt) <= 0.0).tolist(), int(np.sum(c <= 0.0)), len(c),
                                                   feasible_regret(Y, c, test_weights, grid_values)), flush=True)
    return Y, c


if __name__ == "__main__":
    main()
