"""Time one recommendation on the device against the same procedure driven from the host, point by point.

    python tools/recommend_time.py [--n 1000] [--dim 8] [--ensemble 16] [--random 10000] [--steps 1000] [--host-steps 20]
                                   [--host-candidates 500] [--out profiles/recommend_time.txt]

The shape is the reference's recommend step (examples/main.py:243-260): 10 000 random candidates plus the n sampled points, then
T = 1000 steps of the Python gradient descent from the best of them, at E = 16 ensemble members.
  device     cornell_moe_amd.api.recommend (moe_posterior_mean_mcmc_recommend), one call; and the screening alone
             (moe_posterior_mean_mcmc_batch)
  host       the reference's loop over moe_posterior_mean: one call per candidate and member for the screening, one call per step
             and member for the descent, with --host-candidates candidates and --host-steps steps, scaled to the full counts
The host-driven figure is a scaled measurement, marked as such.  No GPU, no numbers: there is no fallback.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from cornell_moe_amd import _lib, api  # noqa: E402


def host_driven(gps, candidates, steps, gd, bounds):
    """(seconds of the screening, seconds of the descent, end point) for the given candidates and step count"""
    E = len(gps)
    t0 = time.perf_counter()
    test = np.zeros(len(candidates))
    for i, pt in enumerate(candidates):
        total = 0.0
        for gp in gps:
            total += gp.posterior_mean(pt, 0, want_grad=False)[0]
        test[i] = -(total / E)
    t1 = time.perf_counter()
    x = candidates[int(np.argmin(test))].copy()
    for i in range(1, steps + 1):
        a_i = gd[5] * np.power(float(i), -gd[4])
        g = np.zeros_like(x)
        for gp in gps:
            g += gp.posterior_mean(x, 0, want_grad=True)[1]
        step = a_i * (g / E)
        dist = np.fmin(x - bounds[:, 0], bounds[:, 1] - x)
        lim = gd[6] * dist
        x = x + np.where(np.fabs(step) > lim, np.copysign(lim, step), step)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--ensemble", type=int, default=16)
    ap.add_argument("--random", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("--host-candidates", type=int, default=500)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "recommend_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    n, d, E = args.n, args.dim, args.ensemble
    X = rng.uniform(0, 1, size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1, keepdims=True)) + 0.1 * rng.normal(size=(n, 1))
    gps = [api.DeviceGP(np.concatenate([[rng.uniform(0.8, 1.5)], rng.uniform(0.5, 1.5, size=d)]), X, y, [rng.uniform(0.01, 0.05)])
           for _ in range(E)]
    cand = np.vstack([rng.uniform(0, 1, size=(args.random, d)), X])
    bounds = np.array([[0.0, 1.0]] * d)
    gd = (1, args.steps, 1, 4, 0.7, 1.0, 0.5, 1.0e-10)  # py_sgd_params_ps of examples/main.py, T = --steps
    lines = ["recommendation: n = %d, dim = %d, ensemble = %d, candidates = %d, steps = %d" % (n, d, E, len(cand), args.steps)]

    def timed(fn):
        fn()  # warm-up: code objects, buffers
        best = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            out = fn()
            best.append(time.perf_counter() - t0)
        return out, float(np.median(best)), float(np.min(best)), float(np.max(best))

    res, med, lo, hi = timed(lambda: api.recommend(gps, cand, gd, bounds))
    lines.append("device, whole recommendation        : median %9.3f ms (min %.3f, max %.3f, %d runs); refined = %s"
                 % (1e3 * med, 1e3 * lo, 1e3 * hi, args.repeat, res["refined"]))
    _, med_s, lo_s, hi_s = timed(lambda: api.posterior_mean_mcmc(gps, cand))
    lines.append("device, screening alone             : median %9.3f ms (min %.3f, max %.3f)" % (1e3 * med_s, 1e3 * lo_s, 1e3 * hi_s))
    lines.append("device, descent and the rest        : %9.3f ms (difference of the medians), %.2f us per step"
                 % (1e3 * (med - med_s), 1e6 * (med - med_s) / args.steps))
    os.environ["MOE_RECOMMEND_XLDS"] = "1"
    res_l, med_l, lo_l, hi_l = timed(lambda: api.recommend(gps, cand, gd, bounds))
    os.environ.pop("MOE_RECOMMEND_XLDS")
    lines.append("device, training points staged in LDS: median %9.3f ms (min %.3f, max %.3f); same bits: %s"
                 % (1e3 * med_l, 1e3 * lo_l, 1e3 * hi_l, bool(np.array_equal(res_l["point"], res["point"]))))
    hc, hs = min(args.host_candidates, len(cand)), min(args.host_steps, args.steps)
    host_driven(gps, cand[:8], 2, gd, bounds)
    t_screen, t_descent, _ = host_driven(gps, cand[:hc], hs, gd, bounds)
    per_q, per_g = t_screen / (hc * E), t_descent / (hs * E)
    scaled = per_q * len(cand) * E + per_g * args.steps * E
    lines.append("host-driven over moe_posterior_mean : %.2f us per value query (%d candidates), %.2f us per gradient query (%d steps)"
                 % (1e6 * per_q, hc, 1e6 * per_g, hs))
    lines.append("host-driven, SCALED to %d candidates and %d steps: %.3f s  (%.0f x the device call)"
                 % (len(cand), args.steps, scaled, scaled / med))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
