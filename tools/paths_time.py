"""Time the posterior function paths: one device call against the routes it replaces.

    python tools/paths_time.py [--members 16] [--paths 64] [--n 500] [--dim 6] [--features 1024] [--candidates 2000]
                               [--repeat 9] [--out profiles/paths_time.txt]

  minimise   api.paths_minimize (moe_gp_paths_minimize): members x paths paths screened at the candidates and minimised with
             (1, 40, 2, 3, 0, 1, 0.2, 1e-9), one call; against the host-driven line search over api.paths_evaluate (one call per
             evaluation, tests/pm_members_reference.literal_float64) on as many of those paths as finish in a few seconds (the count
             is printed, the time scaled to all paths); and beside it min_value_entropy.sample_min_values at the same candidates and
             K = paths draws per member, today's route to GIBBON's input
  evaluate   api.paths_evaluate at the candidates for all paths of a member in one call against one call per path: what sharing a
             point's cosines and covariance entries among the paths returns
One build, the calls alternated in one process, medians of --repeat whole calls after a warm-up.  No GPU, no numbers.
"""
import argparse
import os
import sys
import time

import numpy as np

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, _ROOT)
sys.path.insert(0, os.path.join(_ROOT, "tests"))  # the literal host loop is test infrastructure (tests/pm_members_reference.py)

from cornell_moe_amd import _lib, api, min_value_entropy, posterior_paths  # noqa: E402
import pm_members_reference as pr  # noqa: E402

GD = (1, 40, 2, 3, 0.0, 1.0, 0.2, 1.0e-9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--dim", type=int, default=6)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--host-seconds", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join("profiles", "paths_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    E, S, n, d, M, C_ = args.members, args.paths, args.n, args.dim, args.features, args.candidates
    rng = np.random.default_rng(1)
    X = rng.uniform(0, 1, size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1, keepdims=True)) + 0.1 * rng.normal(size=(n, 1))
    gps = [api.DeviceGP(np.concatenate([[rng.uniform(0.8, 1.5)], rng.uniform(0.5, 1.5, size=d)]), X, y, [rng.uniform(0.01, 0.05)])
           for _ in range(E)]
    bounds = np.array([[0.0, 1.0]] * d)
    cand = api.latin_hypercube(3, bounds, C_)
    t = posterior_paths.draw_path_tables(_lib.COV_MATERN_NU_2P5, d, n, E, M, S, 0)
    tabs = (t["frequencies"], t["phases"], t["weights"], t["noise_normals"])

    def one_path(e, s):
        return (t["frequencies"], t["phases"], np.ascontiguousarray(t["weights"][e:e + 1, s:s + 1]),
                np.ascontiguousarray(t["noise_normals"][e:e + 1, s:s + 1]))

    def minimise():
        return api.paths_minimize(gps, *tabs, GD, bounds, cand)

    def min_values_today():
        return min_value_entropy.sample_min_values(gps, cand, S, 0)

    def evaluate_all():
        return api.paths_evaluate(gps[:1], t["frequencies"], t["phases"], t["weights"][:1], t["noise_normals"][:1], cand)

    def evaluate_one_by_one():
        return [api.paths_evaluate(gps[:1], *one_path(0, s), cand) for s in range(S)]

    calls = [minimise, min_values_today, evaluate_all, evaluate_one_by_one]
    for fn in calls:
        fn()  # warm-up: code objects, buffers
    times = {fn.__name__: [] for fn in calls}
    for _ in range(args.repeat):
        for fn in calls:  # alternated
            t0 = time.perf_counter()
            fn()
            times[fn.__name__].append(time.perf_counter() - t0)
    med = {k: 1e3 * float(np.median(v)) for k, v in times.items()}

    # the host-driven line search on as many paths as finish in --host-seconds
    res = minimise()
    done, worst, t_host = 0, 0.0, 0.0
    for e in range(E):
        for s in range(S):
            if t_host > args.host_seconds:
                break
            tab1 = one_path(e, s)
            t0 = time.perf_counter()
            screened = api.paths_evaluate(gps[e:e + 1], *tab1, cand)[0, 0]
            x0 = cand[int(np.argmin(screened))]
            x, _, _ = pr.literal_float64(lambda p: api.paths_evaluate(gps[e:e + 1], *tab1, p[None])[0, 0, 0],
                                         lambda p: api.paths_evaluate(gps[e:e + 1], *tab1, p[None], want_grad=True)[1][0, 0, 0],
                                         d, 0, GD, bounds, x0)
            t_host += time.perf_counter() - t0
            done += 1
            worst = max(worst, float(np.max(np.abs(x - res["best_points"][e, s]))))
    per_path = 1e3 * t_host / max(done, 1)
    lines = [
        "posterior function paths: %d members x %d paths, n = %d, d = %d, M = %d features, %d candidates, gd = %s; medians of %d "
        "whole calls, alternated in one process after a warm-up" % (E, S, n, d, M, C_, GD, args.repeat),
        "minimise   one paths_minimize call, all %d paths                      %10.2f ms" % (E * S, med["minimise"]),
        "           host-driven line search over paths_evaluate, %3d paths run  %10.2f ms per path = %.0f ms for all (ratio %.0f); "
        "max |dx| against the call %.2e" % (done, per_path, per_path * E * S, per_path * E * S / med["minimise"], worst),
        "           sample_min_values, the same candidates, K = %d per member   %10.2f ms" % (S, med["min_values_today"]),
        "evaluate   one paths_evaluate call, %d paths of one member             %10.2f ms" % (S, med["evaluate_all"]),
        "           one call per path (S = 1, %d calls)                         %10.2f ms (ratio %.1f)" % (
            S, med["evaluate_one_by_one"], med["evaluate_one_by_one"] / med["evaluate_all"]),
    ]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
