"""Time of a hyper-parameter chain: moe_ll_mcmc (the whole chain resident on the device) against the host-driven loop the library
offered before it -- the same stretch move and the same random tables driven from numpy, ONE moe_ll_evaluate call per half-step
(all W/2 proposals factorised together), prior and accept on the host.  Both do the same number of factorisations.

    python tools/hyper_mcmc_time.py [--steps 200] [--repeats 5] [--out profiles/hyper_mcmc_time.txt | -] [--only N,D,W]

DefaultPrior with the reference's quirks, Matern-5/2, noisy.  Per size: median, min and max of `repeats` whole chains after one
warm-up chain, wall clock around the call (the call ends with its own device wait).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cornell_moe_amd import _lib, api  # noqa: E402
from cornell_moe_amd.log_likelihood_mcmc import DefaultPrior  # noqa: E402

SIZES = [(20, 2), (200, 6), (1000, 8)]


def default_log_prior(theta, d):
    """DefaultPrior with quirks for rows of theta [m][nh] (one noise): vectorised, what a careful host loop would do"""
    with np.errstate(divide="ignore"):
        lp = np.exp(-0.5 * theta[:, 0] ** 2) / np.sqrt(2.0 * np.pi)
        lp = lp + np.where(np.any((theta[:, 1:1 + d] < -2.0) | (theta[:, 1:1 + d] > 3.0), axis=1), -np.inf, 0.0)
        lp = lp + np.log(np.log1p(3.0 * (0.1 / theta[:, 1 + d]) ** 2))
    lp[np.any(np.abs(theta) > 20.0, axis=1)] = -np.inf
    return lp


def host_chain(LL, p0, us, pt, ua, d, a=2.0):
    W, nh = p0.shape
    H = W // 2

    def lnpost(th):
        out = default_log_prior(th, d)
        ok = out > -np.inf
        if ok.any():
            out[ok] += LL.evaluate(np.exp(th[ok]))
        return out
    walkers = p0.copy()
    lnp = np.r_[lnpost(walkers[:H]), lnpost(walkers[H:])]
    for t in range(us.shape[0]):
        for h in range(2):
            idx, other = slice(h * H, (h + 1) * H), (1 - h) * H
            z = ((a - 1.0) * us[t, h] + 1.0) ** 2 / a
            c = walkers[other + pt[t, h]]
            prop = c - z[:, None] * (c - walkers[idx])
            lp = lnpost(prop)
            with np.errstate(invalid="ignore", divide="ignore"):
                acc = (nh - 1) * np.log(z) + lp - lnp[idx] > np.log(ua[t, h])
            sel = np.arange(h * H, (h + 1) * H)[acc]
            walkers[sel], lnp[sel] = prop[acc], lp[acc]
    return walkers, lnp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "hyper_mcmc_time.txt"), help="the table goes here too ('-': stdout only)")
    ap.add_argument("--only", default=None, help="n,d,W: one size (profiling runs)")
    ap.add_argument("--resident-only", action="store_true")
    args = ap.parse_args()
    _lib.load()
    _lib.require_gpu()
    lines = ["# hyper-parameter chain, T = %d steps, median [min, max] of %d chains after one warm-up, seconds" % (args.steps, args.repeats),
             "# %5s %3s %4s %5s | %-28s | %-28s | %s" % ("n", "d", "W", "fact.", "resident (moe_ll_mcmc)", "host loop (moe_ll_evaluate)", "host / resident")]
    sizes = [(n, d, W) for n, d in SIZES for W in (2 * (1 + d + 1), 64)]
    if args.only:
        sizes = [tuple(int(v) for v in args.only.split(","))]
    for n, d, W in sizes:
        nh = 1 + d + 1
        rng = np.random.RandomState(1000 * n + W)
        X = rng.uniform(size=(n, d))
        y = (np.sin(3.0 * X[:, 0]) + 0.5 * np.cos(2.0 * X.sum(axis=1)) + 0.05 * rng.standard_normal(n))[:, None]
        LL = api.LogLikelihood(X, y)
        table = DefaultPrior(nh, 1).table(nh)
        p0 = np.r_[0.0, np.full(d, np.log(0.5)), -3.0] + 0.3 * rng.standard_normal((W, nh))
        us, pt, ua = api.stretch_tables(rng, args.steps, W)
        times = {"resident": [], "host": []}
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            res = api.ll_mcmc(LL, table, p0, us, pt, ua, diagnostics=False)
            t1 = time.perf_counter()
            if not args.resident_only:
                host_chain(LL, p0, us, pt, ua, d)
            t2 = time.perf_counter()
            if rep > 0:
                times["resident"].append(t1 - t0)
                times["host"].append(t2 - t1)
        acc = np.mean(np.any(res["chain"][1:] != res["chain"][:-1], axis=2)) if args.steps > 1 else 0.0
        fmt = lambda v: "%.4f [%.4f, %.4f]" % (np.median(v), min(v), max(v))  # noqa: E731
        ratio = "-" if args.resident_only else "%.2f" % (np.median(times["host"]) / np.median(times["resident"]))
        lines.append("  %5d %3d %4d %5d | %-28s | %-28s | %s   (acceptance %.2f)" % (
            n, d, W, W * (args.steps + 1), fmt(times["resident"]), "-" if args.resident_only else fmt(times["host"]), ratio, acc))
        print(lines[-1], flush=True)
        LL.close()
    text = "\n".join(lines) + "\n"
    if args.out and args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
