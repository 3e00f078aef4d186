"""Time one suggestion by the log expected improvement per unit cost (api.log_ei_per_cost_suggest: moe_log_ei_per_cost_mcmc_suggest,
csrc/logeipc1.hip) at the shapes of tools/log_ei_time.py -- 16 members, K = 2 constraints, n = 500, d = 6, 200 Latin-hypercube
starts of which 20 are kept, 2 rounds of 50 steps -- against api.log_ei_constrained_suggest on the same objective GPs with K + 1 = 3
constraints, the cost GPs standing in as the third: the existing path over the same number of chains, and the baseline.  Then the
host-driven loop (tests/ms_restatement.py's optimiser with every evaluation one api.log_ei_per_cost_ensemble call), a greedy batch
of q = 4, K = 0, and the evaluate call at 512 candidates.
   python tools/log_ei_per_cost_time.py [--out profiles/log_ei_per_cost_time.txt] [--windows 5]

All on one build in one process: a warm-up call of every shape, then --windows windows of more than a second per call, the calls of
a comparison alternated window by window; a window's figure is its wall time over its calls (host clock around calls that end in a
device synchronise).  The cost role does less arithmetic per candidate than a feasibility role (no erfcx) over identical chains, and
its sub-member takes no part in the believed-feasible incumbent: the one-call suggestion must not exceed the baseline's time by
more than the baseline's own min-to-max spread over the windows of the same run, and the tool says whether it does and exits 1 if so."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the host-driven loop is the tests' restatement of the optimiser
from cornell_moe_amd import _lib, api, expected_improvement_constrained as eic  # noqa: E402
import ms_restatement as ms  # noqa: E402

lines = []


def say(text):
    print(text)
    sys.stdout.flush()
    lines.append(text)


E, N, D, STARTS, STEPS, ROUNDS, Q, K, CANDIDATES, ALPHA = 16, 500, 6, 200, 50, 2, 4, 2, 512, 1.0
windows = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 5
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


def stats():
    out = (C.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return np.array(list(out), dtype=np.int64)


def launch_stats(name, call):
    s0 = stats()
    call()
    ds = stats() - s0
    say("moe_ensemble_launch_stats for one call of %s: %d evaluations issued zipped, %d member by member; %d launches issued for %d "
        "recorded" % (name, ds[0], ds[1], ds[2], ds[3]))


def window(call):
    """ms per call over a window of more than a second"""
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        t = time.perf_counter() - t0
        if t > 1.0:
            return 1e3 * t / n


def compare(title, calls):
    """calls: [(name, callable)], the first one the baseline; warmed up, then alternated window by window.  Returns the windows."""
    for _, call in calls:
        call()
    t = {name: [] for name, _ in calls}
    for _ in range(windows):
        for name, call in calls:
            t[name].append(window(call))
    say(title)
    for name, _ in calls:
        say("  %-52s ms per call, %d windows: %s | median %.2f, spread %.2f to %.2f" % (
            name, windows, " ".join("%.2f" % v for v in t[name]), np.median(t[name]), min(t[name]), max(t[name])))
    base = t[calls[0][0]]
    for name, _ in calls[1:]:
        m = float(np.median(t[name]))
        say("  %s / %s by medians: %.3f; excess over the baseline's median %.2f ms against the baseline's own spread of %.2f ms" % (
            name, calls[0][0], m / np.median(base), m - float(np.median(base)), max(base) - min(base)))
    return t


say("sustained FP64 FMA rate before: %.1f TFLOP/s" % api.fp64_rate())
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y = np.sin(3 * X).sum(1, keepdims=True)
cvals = [np.cos(2.5 * X + 0.7 * k).sum(1, keepdims=True) - np.median(np.cos(2.5 * X + 0.7 * k).sum(1)) for k in range(K)]
logcost = (2.0 * X[:, :1] + 0.5 * X[:, 1:2]) + 0.05 * rng.standard_normal((N, 1))  # the cost grows e^2-fold along coordinate 0
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
ens = api.DeviceGPMCMC(np.array([1.0] + [0.4] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)
cons = [api.DeviceGPMCMC(np.array([1.0] + [0.5] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, c) for c in cvals]
cost = api.DeviceGPMCMC(np.array([1.0] + [0.8] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, logcost)
tau = [0.0] * K
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
bests = [eic.best_feasible_value(y, np.hstack(cvals), tau)] * E
say("%d members, K = %d constraints and a cost GP (%d GPs), n = %d, d = %d, %d starts -> 20 kept, %d x %d steps, cost_exponent %g" % (
    E, K, E * (2 + K), N, D, STARTS, ROUNDS, STEPS, ALPHA))


def host_loop():
    ev = lambda x, g: api.log_ei_per_cost_ensemble(ens, cons, tau, cost, ALPHA, np.asarray(x).reshape(-1, D), bests, want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


# the baseline: the same 4 chains per member through the existing client, the cost GPs as a third constraint that is as good as always
# satisfied (threshold far above the log costs) -- its chains, kernels and launches are a feasibility role's
base1 = lambda: api.log_ei_constrained_suggest(ens, cons + [cost], tau + [50.0], gd, bounds, bests, starts, 1)  # noqa: E731
cost1 = lambda: api.log_ei_per_cost_suggest(ens, cons, tau, cost, ALPHA, gd, bounds, bests, starts, 1)  # noqa: E731
got, looped, free = cost1(), host_loop(), api.log_ei_per_cost_suggest(ens, cons, tau, cost, 0.0, gd, bounds, bests, starts, 1)
say("  per unit cost %.12g at %s; host loop %.12g, the same point: %s" % (
    got["values"][0], np.round(got["points"][0], 6).tolist(), looped[1], bool(np.array_equal(looped[0], got["points"][0]))))
say("  cost_exponent 0: %.12g at %s" % (free["values"][0], np.round(free["points"][0], 6).tolist()))
launch_stats("log_ei_constrained_suggest, K + 1 = %d, q = 1" % (K + 1), base1)
launch_stats("log_ei_per_cost_suggest, K = %d, q = 1" % K, cost1)
t = compare("one suggestion, K = %d and the cost:" % K, [("log_ei_constrained_suggest, K + 1 = %d" % (K + 1), base1),
                                                        ("log_ei_per_cost_suggest", cost1),
                                                        ("host loop over log_ei_per_cost_ensemble", host_loop)])
base, mine = t["log_ei_constrained_suggest, K + 1 = %d" % (K + 1)], t["log_ei_per_cost_suggest"]
excess, room = float(np.median(mine) - np.median(base)), max(base) - min(base)
within = excess <= room
say("  the requirement: median %.2f ms against the baseline's %.2f ms, excess %.2f ms, the baseline's own spread %.2f ms: %s" % (
    np.median(mine), np.median(base), excess, room, "MET" if within else "NOT MET"))

baseq = lambda: api.log_ei_constrained_suggest(ens, cons + [cost], tau + [50.0], gd, bounds, bests, starts, Q)  # noqa: E731
costq = lambda: api.log_ei_per_cost_suggest(ens, cons, tau, cost, ALPHA, gd, bounds, bests, starts, Q)  # noqa: E731
compare("a greedy batch of q = %d:" % Q, [("log_ei_constrained_suggest, K + 1 = %d" % (K + 1), baseq), ("log_ei_per_cost_suggest", costq)])
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in costq()["values"])))

best0 = [float(y.min())] * E
base0 = lambda: api.log_ei_constrained_suggest(ens, [cost], [50.0], gd, bounds, best0, starts, 1)  # noqa: E731
cost0 = lambda: api.log_ei_per_cost_suggest(ens, None, None, cost, ALPHA, gd, bounds, best0, starts, 1)  # noqa: E731
compare("one suggestion, K = 0 and the cost:", [("log_ei_constrained_suggest, K + 1 = 1", base0), ("log_ei_per_cost_suggest, K = 0", cost0)])

cand = rng.uniform(size=(CANDIDATES, D))
basee = lambda: api.log_ei_constrained_ensemble(ens, cons + [cost], tau + [50.0], cand, bests)  # noqa: E731
coste = lambda: api.log_ei_per_cost_ensemble(ens, cons, tau, cost, ALPHA, cand, bests)  # noqa: E731
compare("value and gradient at %d candidates:" % CANDIDATES, [("log_ei_constrained_ensemble, K + 1 = %d" % (K + 1), basee),
                                                             ("log_ei_per_cost_ensemble", coste)])
for m in [ens, cost] + cons:
    for g in m.gps:
        g.close()
say("sustained FP64 FMA rate after: %.1f TFLOP/s" % api.fp64_rate())
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if within else 1)
