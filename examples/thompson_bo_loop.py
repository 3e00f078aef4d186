"""A Bayesian-optimisation loop by Thompson sampling on the device path: minimise Branin on [0, 1]^2, q points per iteration, each
the minimiser over the domain of its own posterior function path.  Each iteration fits a GP ensemble to the values seen so far (here
a small fixed spread of hyper-parameters stands for the chain that examples/bo_loop.py samples), draws ceil(q / E) paths per member
by pathwise conditioning, screens them at Latin-hypercube candidates joined with the observed points and minimises every path from
its best candidate, all in one device call (cornell_moe_amd/posterior_paths.py -> moe_gp_paths_minimize, csrc/paths.hip).

    python examples/thompson_bo_loop.py [iterations] [q] [num_mcmc]
"""
import sys
import time

import numpy as np

_ROOT = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
sys.path.insert(0, _ROOT)
sys.path.insert(0, __import__("os").path.join(_ROOT, "tests"))  # the wrapper mirror is test infrastructure (tests/wrappers_mirror.py)
from cornell_moe_amd import posterior_paths  # noqa: E402
import wrappers_mirror as cw  # noqa: E402


def branin(x):
    """Branin on [0, 1]^2 (rescaled from [-5, 10] x [0, 15]); minimum 0.397887."""
    a = 15.0 * x[..., 0] - 5.0
    b = 15.0 * x[..., 1]
    return (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0


def ensemble(X, values, hypers, noise):
    hd = cw.HistoricalData(dim=X.shape[1], num_derivatives=0)
    hd.append_sample_points([cw.SamplePoint(X[i], [values[i]], noise) for i in range(X.shape[0])])
    return cw.GaussianProcessMCMC(hypers, np.full((hypers.shape[0], 1), noise), hd, []).member_models()


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    q = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    num_mcmc = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    rng = np.random.default_rng(0)
    dim, noise = 2, 1e-4
    X = rng.uniform(size=(8, dim))
    y = branin(X)
    bounds = [[0.0, 1.0]] * dim
    gd = (1, 40, 2, 3, 0.0, 1.0, 0.2, 1e-9)
    spread = np.exp(0.2 * rng.standard_normal((num_mcmc, 1 + dim)))
    print("initial best value %.4f of %d observations" % (y.min(), len(y)))
    for it in range(iterations):
        t0 = time.perf_counter()
        ys = (y - y.mean()) / y.std()  # the GPs see standardised values
        models = ensemble(X, ys, np.array([1.0, 0.3, 0.3]) * spread, noise)
        nxt, values = posterior_paths.thompson_sampling_batch(models, bounds, gd, q, num_candidates=500, num_features=1024, seed=it)
        t1 = time.perf_counter()
        X = np.vstack([X, nxt])
        y = np.r_[y, branin(nxt)]
        print("iteration %d: %.2f s; suggested %s (the paths' minima %s, standardised); they returned %s; best value %.4f" % (
            it, t1 - t0, np.round(nxt, 3).tolist(), np.round(values, 3).tolist(), np.round(branin(nxt), 3).tolist(), y.min()),
            flush=True)
    return y


if __name__ == "__main__":
    main()
