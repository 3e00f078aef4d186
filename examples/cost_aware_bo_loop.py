"""A cost-aware Bayesian-optimisation loop on the device path: minimise a Branin-like function on [0, 1]^dim whose evaluation COST
grows along the first coordinate (as a model's training time grows with its depth), under a budget on the total cost.  Each
iteration fits one GP ensemble to the objective values and one to the LOG of the observed costs (a small fixed spread of
hyper-parameters stands for the chain that examples/bo_loop.py samples), sets the cost's exponent by cost-cooling -- 1 at the
start, lowered towards 0 as the budget runs out (Lee et al. 2020) -- and picks the next point by the log of the ensemble-averaged
expected improvement per unit cost in one device call (cornell_moe_amd/expected_improvement_per_cost.py ->
moe_log_ei_per_cost_mcmc_suggest, csrc/logeipc1.hip).  The loop stops after `iterations` or when the budget is spent.

    python examples/cost_aware_bo_loop.py [iterations] [dim] [members]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "tests"))  # the wrapper mirror is test infrastructure (tests/wrappers_mirror.py)
from cornell_moe_amd import expected_improvement_per_cost as epc  # noqa: E402
import wrappers_mirror as cw  # noqa: E402


def objective(x):
    """Branin on the first two coordinates of [0, 1]^dim (rescaled from [-5, 10] x [0, 15]; minimum 0.397887 at three points, one
    of them at a small first coordinate) plus a bowl in the others"""
    a = 15.0 * x[..., 0] - 5.0
    b = 15.0 * x[..., 1]
    f = (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0
    return f + 10.0 * np.sum((x[..., 2:] - 0.5) ** 2, axis=-1)


def cost(x, rng):
    """what an evaluation at x costs: e^3 = 20 times as much at x0 = 1 as at x0 = 0, with 5 per cent noise"""
    return np.exp(3.0 * x[..., 0] + 0.05 * rng.standard_normal(np.shape(x)[:-1]))


def ensemble(X, values, hypers, noise):
    hd = cw.HistoricalData(dim=X.shape[1], num_derivatives=0)
    hd.append_sample_points([cw.SamplePoint(X[i], [values[i]], noise) for i in range(X.shape[0])])
    return cw.GaussianProcessMCMC(hypers, np.full((hypers.shape[0], 1), noise), hd, []).member_models()


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    num_mcmc = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    if dim < 2:
        raise SystemExit("dim must be at least 2")
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(4 * dim, dim))
    y, paid = objective(X), cost(X, rng)
    spent_at_start = float(paid.sum())
    budget = spent_at_start + 8.0 * iterations  # (a cheap evaluation costs about 1, a dear one about 20)
    bounds = [[0.0, 1.0]] * dim
    gd = (40, 20, 2, 0, 0.7, 1.0, 0.5, 1e-8)
    spread = np.exp(0.2 * rng.standard_normal((num_mcmc, 1 + dim)))
    print("budget %.1f, of which the %d initial observations cost %.1f; best value %.4f" % (budget, len(y), spent_at_start, y.min()))
    for it in range(iterations):
        spent = float(paid.sum())
        if spent >= budget:
            print("the budget is spent after %d iterations" % it)
            break
        t0 = time.perf_counter()
        alpha = epc.cost_cooling_exponent(spent, budget, spent_at_start)
        ys = (y - y.mean()) / y.std()  # the GPs see standardised values; the log cost keeps its own scale
        models = ensemble(X, ys, np.array([1.0] + [0.3] * dim) * spread, 1e-4)
        cost_models = ensemble(X, np.log(paid), np.array([1.0] + [0.6] * dim) * spread, 1e-2)
        nxt, values, found = epc.multistart_log_expected_improvement_per_cost_optimization(
            models, cost_models, bounds, gd, num_multistarts=40, cost_exponent=alpha, best_so_far=float(ys.min()), seed=it)
        expected_cost = epc.predicted_cost(cost_models, nxt)[0]
        t1 = time.perf_counter()
        f, c = objective(nxt), cost(nxt, rng)
        X, y, paid = np.vstack([X, nxt]), np.r_[y, f], np.r_[paid, c]
        print("iteration %d: %.2f s; cost spent %.1f of %.1f, exponent %.3f; suggested %s (acquisition %.4f, found=%s, predicted cost "
              "%.2f); it returned f = %.4f at cost %.2f; best value %.4f" % (
                  it, t1 - t0, spent, budget, alpha, np.round(nxt[0], 3).tolist(), values[0], bool(found[0]), expected_cost[0], f[0], c[0],
                  y.min()), flush=True)
    return y, paid


if __name__ == "__main__":
    main()
