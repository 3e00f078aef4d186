"""Time the per-member discretisation of a KG-MCMC iteration: one device call against the host-driven loop it replaces.

    python tools/discretise_time.py [--ensemble 16] [--random 1000] [--repeat 5] [--out profiles/discretise_time.txt]

The shape is the reference's examples/main.py:172-197: for each of E = 16 ensemble members, screen 1000 random points plus the n
sampled points on the member's posterior mean, start the line-search optimiser from the best, keep or fall back.
  device     cornell_moe_amd.api.minimize_member_means (moe_posterior_mean_members_minimize), one call; and the same call with
             max_num_steps = max_num_restarts = 1, whose difference to the full call is the descent kernel's share
  host       the loop over the existing entry points: one moe_gp_additional_mean (all candidates of a member in one call) and one
             moe_posterior_mean_optimize per member
at d = 2 and 8, n = 50 and 1000, with main.py's inner parameters (1, 6, 1, 3, 0, 1, 0.1, 1e-10) and with 100 steps x 10 restarts.
Both run in this process after a warm-up; the figures are medians of --repeat runs.  No GPU, no numbers: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from cornell_moe_amd import _lib, api  # noqa: E402


def host_driven(gps, cand, gd, bounds):
    d = gps[0].d
    best = np.zeros((len(gps), d))
    for e, gp in enumerate(gps):
        mu = gp.additional_mean(cand)
        i0 = int(np.argmin(mu))
        x, fval = gp.posterior_mean_optimize(gd, bounds, cand[i0])
        best[e] = cand[i0] if -fval > mu[i0] else x
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", type=int, default=16)
    ap.add_argument("--random", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "discretise_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    E = args.ensemble
    lines = ["per-member discretisation: ensemble = %d, candidates = %d + n; medians of %d runs after a warm-up" % (E, args.random, args.repeat),
             "%3s %5s %-22s %12s %12s %12s %8s %10s" % ("d", "n", "steps x restarts", "device ms", "screen ms", "host ms", "ratio",
                                                       "max |dx|")]

    def timed(fn):
        fn()  # warm-up: code objects, buffers
        t = []
        for _ in range(max(args.repeat, 5)):
            t0 = time.perf_counter()
            out = fn()
            t.append(time.perf_counter() - t0)
        return out, float(np.median(t))

    slower = []
    for d in (2, 8):
        for n in (50, 1000):
            rng = np.random.default_rng(1000 * d + n)
            X = rng.uniform(0, 1, size=(n, d))
            y = np.sin(3.0 * X.sum(axis=1, keepdims=True)) + 0.1 * rng.normal(size=(n, 1))
            gps = [api.DeviceGP(np.concatenate([[rng.uniform(0.8, 1.5)], rng.uniform(0.5, 1.5, size=d)]), X, y, [rng.uniform(0.01, 0.05)])
                   for _ in range(E)]
            cand = np.vstack([rng.uniform(0, 1, size=(args.random, d)), X])
            bounds = np.array([[0.0, 1.0]] * d)
            for gd in ((1, 6, 1, 3, 0.0, 1.0, 0.1, 1.0e-10), (1, 100, 10, 3, 0.0, 1.0, 0.1, 1.0e-10)):
                res, t_dev = timed(lambda: api.minimize_member_means(gps, cand, gd, bounds))
                _, t_scr = timed(lambda: api.minimize_member_means(gps, cand, (1, 1, 1) + gd[3:], bounds))
                host, t_host = timed(lambda: host_driven(gps, cand, gd, bounds))
                lines.append("%3d %5d %-22s %12.3f %12.3f %12.3f %8.1f %10.2e"
                             % (d, n, "%d x %d" % (gd[1], gd[2]), 1e3 * t_dev, 1e3 * t_scr, 1e3 * t_host, t_host / t_dev,
                                float(np.max(np.abs(host - res["best_points"])))))
                if not t_host / t_dev > 1.0:
                    slower.append("d = %d, n = %d, %d x %d" % (d, n, gd[1], gd[2]))
            del gps
    lines.append("screen ms: the same call with one step and one restart (screening, selection, one step); device ms - screen ms is "
                 "the rest of the descent kernel.  Trials are evaluated one per pass over the training rows; batching several per "
                 "pass was not tried.")
    lines.append("rows at which the single call is NOT faster than the host-driven loop: %s" % ("; ".join(slower) if slower else "none"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
