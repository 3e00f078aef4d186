"""Time one suggestion by the LOG of the ensemble-averaged constrained expected improvement (api.log_ei_constrained_suggest:
moe_log_ei_constrained_mcmc_suggest, csrc/logcei1.hip) against the same suggestion by the plain form (api.ei_constrained_suggest:
the existing call and the baseline) and against the host-driven loop -- tests/ms_restatement.py's optimiser with every evaluation
one api.log_ei_constrained_ensemble call -- at the shapes of tools/ei_constrained_time.py: 16 members, K = 2 constraints, n = 500,
d = 6, 200 Latin-hypercube starts of which 20 are kept, 2 rounds of 50 steps.  Then a greedy batch of q = 4 by both forms, and
K = 0 beside api.ei_analytic_suggest.
   python tools/log_ei_time.py [--out profiles/log_ei_time.txt] [--windows 5]

All on one build in one process: a warm-up call of every shape, then --windows windows of more than a second per call, the calls of
a comparison alternated window by window; a window's figure is its wall time over its calls (host clock around calls that end in a
device synchronise).  The launch chain of the log form is the plain form's kernel for kernel (its candidate and combine kernels in
the places of cei1.hip's) -- moe_ensemble_launch_stats for one suggestion by each form is printed -- except at K = 0, where the
plain form takes the mean of the members and the log form its combine kernel.  No ratio is set in advance; the windows and
medians are a finding."""
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


E, N, D, STARTS, STEPS, ROUNDS, Q, K = 16, 500, 6, 200, 50, 2, 4, 2
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
    """calls: [(name, callable)], the first one the baseline; warmed up, then alternated window by window"""
    for _, call in calls:
        call()
    t = {name: [] for name, _ in calls}
    for _ in range(windows):
        for name, call in calls:
            t[name].append(window(call))
    say(title)
    for name, _ in calls:
        say("  %-44s ms per call, %d windows: %s | median %.2f, spread %.2f to %.2f" % (
            name, windows, " ".join("%.2f" % v for v in t[name]), np.median(t[name]), min(t[name]), max(t[name])))
    base = t[calls[0][0]]
    for name, _ in calls[1:]:
        m = float(np.median(t[name]))
        say("  %s / %s by medians: %.3f; its median lies %s the baseline's own spread" % (
            name, calls[0][0], m / np.median(base), "inside" if min(base) <= m <= max(base) else "OUTSIDE"))
    return t


def host_loop(ens, cons, tau, bests, bounds, starts):
    ev = lambda x, g: api.log_ei_constrained_ensemble(ens, cons, tau, np.asarray(x).reshape(-1, D), bests, want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


say("sustained FP64 FMA rate before: %.1f TFLOP/s" % api.fp64_rate())
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y = np.sin(3 * X).sum(1, keepdims=True)
# constraint k: a smooth function of its own, about half of the box feasible under the threshold 0
cvals = [np.cos(2.5 * X + 0.7 * k).sum(1, keepdims=True) - np.median(np.cos(2.5 * X + 0.7 * k).sum(1)) for k in range(K)]
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
ens = api.DeviceGPMCMC(np.array([1.0] + [0.4] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)
cons = [api.DeviceGPMCMC(np.array([1.0] + [0.5] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, c) for c in cvals]
tau = [0.0] * K
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
bests = [eic.best_feasible_value(y, np.hstack(cvals), tau)] * E
say("%d members, K = %d constraints (%d GPs), n = %d, d = %d, %d starts -> 20 kept, %d x %d steps" % (
    E, K, E * (1 + K), N, D, STARTS, ROUNDS, STEPS))

log1 = lambda: api.log_ei_constrained_suggest(ens, cons, tau, gd, bounds, bests, starts, 1)  # noqa: E731
plain1 = lambda: api.ei_constrained_suggest(ens, cons, tau, gd, bounds, bests, starts, 1)  # noqa: E731
loop1 = lambda: host_loop(ens, cons, tau, bests, bounds, starts)  # noqa: E731
got, want, looped = log1(), plain1(), loop1()
say("  log form %.12g at %s; host loop %.12g, the same point: %s" % (
    got["values"][0], np.round(got["points"][0], 6).tolist(), looped[1], bool(np.array_equal(looped[0], got["points"][0]))))
say("  plain form %.12g (its log %.12g) at %s" % (want["values"][0], np.log(want["values"][0]), np.round(want["points"][0], 6).tolist()))
launch_stats("ei_constrained_suggest, q = 1", plain1)
launch_stats("log_ei_constrained_suggest, q = 1", log1)
compare("one suggestion, K = %d:" % K, [("ei_constrained_suggest", plain1), ("log_ei_constrained_suggest", log1),
                                        ("host loop over log_ei_constrained_ensemble", loop1)])

logq = lambda: api.log_ei_constrained_suggest(ens, cons, tau, gd, bounds, bests, starts, Q)  # noqa: E731
plainq = lambda: api.ei_constrained_suggest(ens, cons, tau, gd, bounds, bests, starts, Q)  # noqa: E731
compare("a greedy batch of q = %d, K = %d:" % (Q, K), [("ei_constrained_suggest", plainq), ("log_ei_constrained_suggest", logq)])
say("  values of the %d picks, log form: %s" % (Q, " ".join("%.6g" % v for v in logq()["values"])))

best0 = [float(y.min())] * E
log0 = lambda: api.log_ei_constrained_suggest(ens, None, None, gd, bounds, best0, starts, 1)  # noqa: E731
ei0 = lambda: api.ei_analytic_suggest(ens, gd, bounds, best0, starts, 1)  # noqa: E731
launch_stats("ei_analytic_suggest, q = 1", ei0)
launch_stats("log_ei_constrained_suggest, K = 0, q = 1", log0)
compare("one suggestion, K = 0:", [("ei_analytic_suggest", ei0), ("log_ei_constrained_suggest, K = 0", log0)])
for m in [ens] + cons:
    for g in m.gps:
        g.close()
say("sustained FP64 FMA rate after: %.1f TFLOP/s" % api.fp64_rate())
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
