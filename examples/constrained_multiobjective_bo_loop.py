"""A two-objective Bayesian-optimisation loop under one black-box constraint on the device path: minimise both objectives of the
ZDT1-like pair f1(x) = x_0, f2(x) = g(x) (1 - sqrt(x_0 / g(x))) with g(x) = 1 + 3 x_1 on [0, 1]^2, inside the disc
c(x) = (x_0 - 0.5)^2 + (x_1 - 0.4)^2 <= 0.16, which cuts both ends off the unconstrained Pareto front (x_1 = 0).  Each iteration
fits one GP ensemble per objective and one for the constraint (a small fixed spread of hyper-parameters stands for the chain that
examples/bo_loop.py samples), takes the Pareto front of the FEASIBLE observed outcomes inside the reference point, and picks the
next q points by the ensemble-averaged constrained expected hypervolume improvement, greedily, in one device call
(cornell_moe_amd/expected_hypervolume_improvement_constrained.py -> moe_ehvi_constrained_mcmc_suggest, csrc/cehvi1.hip).  The
hypervolume of the feasible observed front is printed per iteration.

    python examples/constrained_multiobjective_bo_loop.py [iterations] [q] [num_mcmc]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "tests"))  # the wrapper mirror is test infrastructure (tests/wrappers_mirror.py)
from cornell_moe_amd import expected_hypervolume_improvement as ehvi  # noqa: E402
from cornell_moe_amd import expected_hypervolume_improvement_constrained as cehvi  # noqa: E402
import wrappers_mirror as cw  # noqa: E402

REFERENCE = (1.1, 4.1)
THRESHOLDS = (0.16,)


def objectives(x):
    f1 = x[..., 0]
    g = 1.0 + 3.0 * x[..., 1]
    return np.stack([f1, g * (1.0 - np.sqrt(f1 / g))], axis=-1)


def constraint(x):
    return ((x[..., 0] - 0.5) ** 2 + (x[..., 1] - 0.4) ** 2)[..., None]


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
    X = rng.uniform(size=(10, dim))
    Y, Cv = objectives(X), constraint(X)
    bounds = [[0.0, 1.0]] * dim
    gd = (40, 20, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    spread = np.exp(0.2 * rng.standard_normal((num_mcmc, 1 + dim)))
    front = cehvi.feasible_pareto_front(Y, Cv, THRESHOLDS, REFERENCE)
    print("initial feasible hypervolume %.4f: %d observations, %d feasible, %d on the feasible front" % (
        ehvi.hypervolume(front, REFERENCE), len(Y), int(np.sum(Cv[:, 0] <= THRESHOLDS[0])), len(front)))
    for it in range(iterations):
        t0 = time.perf_counter()
        models = [ensemble(X, Y[:, 0], np.array([1.0, 0.5, 0.5]) * spread, noise),
                  ensemble(X, Y[:, 1], np.array([2.0, 0.5, 0.5]) * spread, noise)]
        constraints = [ensemble(X, Cv[:, 0], np.array([0.5, 0.6, 0.6]) * spread, noise)]
        front = cehvi.feasible_pareto_front(Y, Cv, THRESHOLDS, REFERENCE)
        nxt, values, found = cehvi.multistart_constrained_expected_hypervolume_improvement_optimization(
            models, constraints, THRESHOLDS, REFERENCE, bounds, gd, num_multistarts=40, num_to_sample=q, front=front, seed=it)
        t1 = time.perf_counter()
        got, cgot = objectives(nxt), constraint(nxt)
        X, Y, Cv = np.vstack([X, nxt]), np.vstack([Y, got]), np.vstack([Cv, cgot])
        after = cehvi.feasible_pareto_front(Y, Cv, THRESHOLDS, REFERENCE)
        print("iteration %d: %.2f s; feasible front of %d points; suggested %s (acquisition %s, found=%s); they returned %s, constraint "
              "%s (feasible: %s); feasible hypervolume %.4f" % (
                  it, t1 - t0, len(front), np.round(nxt, 3).tolist(), np.round(values, 4).tolist(), found.tolist(),
                  np.round(got, 3).tolist(), np.round(cgot[:, 0], 3).tolist(), (cgot[:, 0] <= THRESHOLDS[0]).tolist(),
                  ehvi.hypervolume(after, REFERENCE)), flush=True)
    return Y, Cv


if __name__ == "__main__":
    main()
