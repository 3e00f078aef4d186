"""A Bayesian-optimisation loop under an unknown constraint on the device path: minimise Branin on [0, 1]^2 inside a disc that the
optimiser only learns about through the constraint values its experiments return.  Each iteration fits one GP ensemble to the
objective values and one to the constraint values (here a small fixed spread of hyper-parameters stands for the chain that
examples/bo_loop.py samples), takes the best FEASIBLE observation as the incumbent (+inf while there is none: the acquisition is
then the probability of feasibility and the search looks for the feasible region first), and picks the next q points by the
ensemble-averaged expected improvement times the probability of feasibility, greedily, in one device call
(cornell_moe_amd/expected_improvement_constrained.py -> moe_ei_constrained_mcmc_suggest, csrc/cei1.hip).

    python examples/constrained_bo_loop.py [iterations] [q] [num_mcmc]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "tests"))  # the wrapper mirror is test infrastructure (tests/wrappers_mirror.py)
from cornell_moe_amd import expected_improvement_constrained as eic  # noqa: E402
import wrappers_mirror as cw  # noqa: E402

CENTRE, RADIUS = np.array([0.35, 0.65]), 0.3


def branin(x):
    """Branin on [0, 1]^2 (rescaled from [-5, 10] x [0, 15]); minimum 0.397887."""
    a = 15.0 * x[..., 0] - 5.0
    b = 15.0 * x[..., 1]
    return (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0


def disc(x):
    """the constraint value: <= 0 inside the disc of radius 0.3 about (0.35, 0.65), which holds none of Branin's three minima"""
    return (np.sum((x - CENTRE) ** 2, axis=-1) - RADIUS ** 2) / RADIUS ** 2


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
    y, c = branin(X), disc(X)
    bounds = [[0.0, 1.0]] * dim
    gd = (40, 20, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    spread = np.exp(0.2 * rng.standard_normal((num_mcmc, 1 + dim)))
    print("initial best feasible value %s of %d observations (%d feasible)" % (
        eic.best_feasible_value(y, c, [0.0]), len(y), int(np.sum(c <= 0.0))))
    for it in range(iterations):
        t0 = time.perf_counter()
        ys = (y - y.mean()) / y.std()  # the GPs see standardised values; the constraint keeps its own zero
        models = ensemble(X, ys, np.array([1.0, 0.3, 0.3]) * spread, noise)
        cmodels = ensemble(X, c, np.array([1.0, 0.5, 0.5]) * spread, noise)
        best = eic.best_feasible_value(ys, c, [0.0])
        nxt, values, found = eic.multistart_constrained_expected_improvement_optimization(
            models, [cmodels], [0.0], bounds, gd, num_multistarts=40, num_to_sample=q, best_so_far=best, seed=it)
        cei = eic.ConstrainedExpectedImprovementMCMC(models, [cmodels], [0.0], best_so_far=best)
        pof = cei.probability_of_feasibility(nxt)
        t1 = time.perf_counter()
        X = np.vstack([X, nxt])
        y, c = np.r_[y, branin(nxt)], np.r_[c, disc(nxt)]
        print("iteration %d: %.2f s; incumbent %s; suggested %s (acquisition %s, probability of feasibility %s, found=%s); they "
              "returned f = %s, c = %s; best feasible value %s" % (
                  it, t1 - t0, "none" if np.isinf(best) else "%.4f (standardised)" % best, np.round(nxt, 3).tolist(),
                  np.round(values, 4).tolist(), np.round(pof, 3).tolist(), found.tolist(), np.round(branin(nxt), 3).tolist(),
                  np.round(disc(nxt), 3).tolist(), eic.best_feasible_value(y, c, [0.0])), flush=True)
    return y, c


if __name__ == "__main__":
    main()
