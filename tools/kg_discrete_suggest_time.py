"""Time one suggestion by the ensemble-averaged discretised knowledge gradient: api.kg_discrete_multistart
(moe_kg_discrete_mcmc_multistart: the whole multistart ascent in one library call, csrc/kg1_opt.hip) against the host-driven loop --
tests/ms_restatement.py's optimiser with every evaluation one api.kg_discrete_mcmc call (one device call per member) and the
updates in numpy.  16 members, 200 Latin-hypercube starts of which 20 are kept, 2 rounds of 50 steps, discrete sets of A = 11 and
A = 1010 points, on two GPs: a Branin GP of the size of the reference's examples/main.py (n = 8 + 12, d = 2) and the n = 500,
d = 6 GP of tools/kg_discrete_time.py.
   python tools/kg_discrete_suggest_time.py [--out profiles/kg_discrete_suggest_time.txt] [--no-mc] [--repeat 9]

Both run on the same build, alternated, median of --repeat whole suggestions (host clock around calls that end in a device
synchronise); the two walk the same path bit for bit, which is asserted.  Launches per optimiser step come from
moe_ensemble_launch_stats around one suggestion.  As a side note, DeviceGPMCMC.kg_multistart (moe_kg_mcmc_multistart: the
Monte-Carlo knowledge gradient) at q = 1 with 2^7 samples from the same starts: it estimates another quantity (the exact value is a
lower bound of it) and its inner line searches make each of its evaluations far dearer, so that figure is a cost, not a race."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the host-driven loop is the tests' restatement of the optimiser
from cornell_moe_amd import _lib, api  # noqa: E402
import ms_restatement as ms  # noqa: E402

lines = []


def say(text):
    print(text)
    sys.stdout.flush()
    lines.append(text)


def clocks(tag):
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True, timeout=60).stdout
        got = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln or "fclk" in ln]
        say("clocks %s: %s" % (tag, "; ".join(got) if got else "rocm-smi printed none"))
    except Exception as e:  # noqa: BLE001
        say("clocks %s: rocm-smi not available (%s)" % (tag, type(e).__name__))
    say("sustained FP64 FMA rate %s: %.1f TFLOP/s" % (tag, api.fp64_rate()))


def branin(x):
    a, b = 15.0 * x[..., 0] - 5.0, 15.0 * x[..., 1]
    return (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0


def stats():
    out = (C.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return np.array([int(v) for v in out])


E, STARTS, STEPS, ROUNDS, M = 16, 200, 50, 2, 128
repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 9
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py
inner = (1, 20, 1, 4, 0.7, 1.0, 0.1, 1e-9)


def problem(name, rng):
    if name == "branin":
        n, d = 20, 2
        X = rng.uniform(size=(n, d))
        y = branin(X)[:, None]
        y = (y - y.mean()) / y.std()
        base, noise = np.array([1.0, 0.3, 0.3]), 1e-4
    else:
        n, d = 500, 6
        X = rng.uniform(size=(n, d))
        y = np.sin(3 * X).sum(1, keepdims=True)
        base, noise = np.array([1.0] + [0.4] * d), 1e-2
    hypers = base[None, :] * np.exp(0.15 * rng.standard_normal((E, d + 1)))  # the spread of a hyper-parameter chain
    return n, d, X, y, hypers, np.full((E, 1), noise)


def host_loop(ens, sets, bests, bounds, starts):
    d = starts.shape[1]
    vals = api.kg_discrete_mcmc(ens, sets, starts, bests, want_grad=False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: api.kg_discrete_mcmc(ens, sets, np.asarray(x).reshape(-1, d), bests)[1].reshape(np.shape(x)),
                              gd, bounds, starts[order])
    end_vals = api.kg_discrete_mcmc(ens, sets, ends, bests, want_grad=False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w]), ends


clocks("before")
say("%d members, %d starts -> 20 kept, %d x %d steps; whole suggestions, median / min of %d, alternated" % (E, STARTS, ROUNDS, STEPS,
                                                                                                          repeat))
say("%-7s %5s | %22s | %22s | %7s | %28s | %s" % ("GP", "A", "one call ms (med/min)", "host loop ms (med/min)", "ratio",
                                                  "launches / step (of unmerged)", "moe_kg_mcmc_multistart q=1 M=128 ms"))
for name in ("branin", "n500_d6"):
    rng = np.random.default_rng(0)
    n, d, X, y, hypers, noises = problem(name, rng)
    ens = api.DeviceGPMCMC(hypers, noises, X, y)
    bounds = np.array([[0.0, 1.0]] * d)
    starts = api.latin_hypercube(5, bounds, STARTS)
    bests = [float(y.min())] * E
    for A in (11, 1010):
        sets = [rng.uniform(size=(A, d)) for _ in range(E)]
        one = lambda: api.kg_discrete_multistart(ens, gd, bounds, sets, bests, starts)  # noqa: E731
        res = one()  # workspaces
        point, value, ends = host_loop(ens, sets, bests, bounds, starts)
        assert np.array_equal(res["end_points"], ends) and np.array_equal(res["point"], point) and res["value"] == value
        t_one, t_host = [], []
        for _ in range(repeat):
            t0 = time.perf_counter()
            one()
            t1 = time.perf_counter()
            host_loop(ens, sets, bests, bounds, starts)
            t2 = time.perf_counter()
            t_one.append(1e3 * (t1 - t0))
            t_host.append(1e3 * (t2 - t1))
        before = stats()
        res = one()
        grew = stats() - before
        evals = max(int(grew[0] + grew[1]), 1)  # evaluations of the ensemble in the suggestion (screening and end values included)
        per_step = "%.1f (of %.1f)" % (grew[2] / evals + 1, grew[3] / evals + 1) if grew[0] > 0 else "not merged"  # (+ 1: the step kernel)
        mc = "not run"
        if "--no-mc" not in sys.argv:
            normals = np.random.default_rng(1).standard_normal((M // 2, 1))
            try:
                t0 = time.perf_counter()
                ens.kg_multistart(gd, inner, bounds, np.array(sets), starts.reshape(STARTS, 1, d), None, M, bests, normals)
                mc = "%.0f" % (1e3 * (time.perf_counter() - t0))
            except api.OptimalLearningException as e:
                mc = "refused: %s" % e
        say("%-7s %5d | %10.1f / %9.1f | %10.1f / %9.1f | %6.2fx | %28s | %s" % (
            name, A, np.median(t_one), min(t_one), np.median(t_host), min(t_host), np.median(t_host) / np.median(t_one), per_step, mc))
        say("        steps taken by the kept starts: %d .. %d of %d; KG of the suggestion %.6g" % (
            res["steps_taken"].min(), res["steps_taken"].max(), ROUNDS * STEPS, res["value"]))
    for g in ens.gps:
        g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
