"""A three-objective Bayesian-optimisation loop on the device path: minimise the three squared distances
f_k(x) = |x - c_k|^2 to the corners c_1 = (0.2, 0.2), c_2 = (0.8, 0.2), c_3 = (0.5, 0.8) of a triangle in [0, 1]^2, whose Pareto
set is the triangle itself.  Each iteration fits one GP ensemble per objective (a small fixed spread of hyper-parameters stands for
the chain that examples/bo_loop.py samples), takes the Pareto front of the observed outcomes inside the reference point, and picks
the next q points by the ensemble-averaged three-objective expected hypervolume improvement, greedily, in one device call
(cornell_moe_amd/expected_hypervolume_improvement.py -> moe_ehvi3_mcmc_suggest, csrc/ehvi3.hip).  The hypervolume of the observed
front is printed per iteration.

    python examples/three_objective_bo_loop.py [iterations] [q] [num_mcmc]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "tests"))  # the wrapper mirror is test infrastructure (tests/wrappers_mirror.py)
from cornell_moe_amd import expected_hypervolume_improvement as ehvi  # noqa: E402
import wrappers_mirror as cw  # noqa: E402

REFERENCE = (1.0, 1.0, 1.0)
CORNERS = np.array([(0.2, 0.2), (0.8, 0.2), (0.5, 0.8)])


def objectives(x):
    return np.stack([np.sum((x - c) ** 2, axis=-1) for c in CORNERS], axis=-1)


def ensemble(X, values, hypers, noise):
    hd = cw.HistoricalData(dim=X.shape[1], num_derivatives=0)
    hd.append_sample_points([cw.SamplePoint(X[i], [values[i]], noise) for i in range(X.shape[0])])
    return cw.GaussianProcessMCMC(hypers, np.full((hypers.shape[0], 1), noise), hd, []).member_models()


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
    print("initial hypervolume %.4f of %d observations (%d on the front)" % (
        ehvi.hypervolume_3(Y, REFERENCE), len(Y), len(ehvi.pareto_front_3(Y, REFERENCE))))
    for it in range(iterations):
        t0 = time.perf_counter()
        models = [ensemble(X, Y[:, k], np.array([1.0, 0.5, 0.5]) * spread, noise) for k in range(3)]
        front = ehvi.pareto_front_3(Y, REFERENCE)[:192]
        nxt, values, found = ehvi.multistart_expected_hypervolume_improvement_3_optimization(
            models[0], models[1], models[2], REFERENCE, bounds, gd, num_multistarts=40, num_to_sample=q, front=front, seed=it)
        t1 = time.perf_counter()
        got = objectives(nxt)
        X, Y = np.vstack([X, nxt]), np.vstack([Y, got])
        print("iteration %d: %.2f s; front of %d points; suggested %s (acquisition %s, found=%s); they returned %s; hypervolume %.4f" % (
            it, t1 - t0, len(front), np.round(nxt, 3).tolist(), np.round(values, 4).tolist(), found.tolist(),
            np.round(got, 3).tolist(), ehvi.hypervolume_3(Y, REFERENCE)), flush=True)
    return Y


if __name__ == "__main__":
    main()
