"""Time one suggestion by the LOG of the ensemble-averaged three-objective constrained expected hypervolume improvement
(api.log_ehvi3_constrained_suggest: moe_log_ehvi3_constrained_mcmc_suggest, csrc/logehvi3.hip) against the same suggestion by the
plain form (api.ehvi_constrained_suggest with three objectives: the existing call and the yardstick) and against the host-driven
loop -- tests/ms_restatement.py's optimiser with every evaluation one api.log_ehvi3_constrained_ensemble call -- at the shapes of
tools/log_ehvi_time.py: 16 members, K = 2 constraints, n = 500, d = 6, 200 Latin-hypercube starts of which 20 are kept, 2 rounds of
50 steps, a front of 32 points.  Then a staircase of 192 points (18 721 boxes), a greedy batch of q = 4 by both forms, K = 0 beside
api.ehvi3_suggest, and the evaluate calls of both forms at 512 candidates against the staircase, whose difference over the 512 x 16
(candidate, member) pairs is what a log box evaluation costs beyond a plain one.
   python tools/log_ehvi3_time.py [--out profiles/log_ehvi3_time.txt] [--windows 5]
   python tools/log_ehvi3_time.py --suggestions 5 [--staircase]     (nothing timed: suggestions by each form, for a kernel trace)

All on one build in one process: a warm-up call of every shape, then --windows windows of more than a second per call, the calls of
a comparison alternated window by window; a window's figure is its wall time over its calls (host clock around calls that end in a
device synchronise).  The launch chain of the log form is the plain form's kernel for kernel (its box, feasibility and combine
kernels in the places of ehvi3.hip's and cehvi1.hip's) except at K = 0, where the plain form is ehvi3.hip's own client and the log
form keeps cehvi1.hip's staging.  No ratio is set in advance and no time is asserted; the windows and medians are a finding.  The
box kernels' own times come from a kernel trace of the --suggestions run (DESIGN.md section 5.26 says how it was taken)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the host-driven loop is the tests' restatement of the optimiser
from cornell_moe_amd import api  # noqa: E402
import ms_restatement as ms  # noqa: E402

lines = []


def say(text):
    print(text)
    sys.stdout.flush()
    lines.append(text)


E, N, D, STARTS, STEPS, ROUNDS, Q, F, FULL, K, CANDIDATES = 16, 500, 6, 200, 50, 2, 4, 32, 192, 2, 512
windows = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 5
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


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
        say("  %-48s ms per call, %d windows: %s | median %.2f, spread %.2f to %.2f" % (
            name, windows, " ".join("%.2f" % v for v in t[name]), np.median(t[name]), min(t[name]), max(t[name])))
    base = t[calls[0][0]]
    for name, _ in calls[1:]:
        m = float(np.median(t[name]))
        say("  %s / %s by medians: %.3f; its median lies %s the baseline's own spread" % (
            name, calls[0][0], m / np.median(base), "inside" if min(base) <= m <= max(base) else "OUTSIDE"))
    return {name: float(np.median(v)) for name, v in t.items()}


def staircase(count, ref):
    """count mutually non-dominated points strictly inside ref, u ascending, v descending, w ascending: every slab keeps all its
    points, (count + 1)(count + 2) / 2 boxes, in the canonical order"""
    t = (np.arange(count) + 0.5) / count
    return np.ascontiguousarray(np.stack([ref[0] - 4.0 * (1.0 - t) ** 2 - 0.5, ref[1] - 4.0 * t ** 2 - 0.5, ref[2] - 4.5 + 4.0 * t], axis=1))


def host_loop(objs, cons, tau, ref, front, bounds, starts):
    ev = lambda x, g: api.log_ehvi3_constrained_ensemble(objs, cons, tau, ref, front, np.asarray(x).reshape(-1, D), want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y1 = np.sin(3 * X).sum(1, keepdims=True)
y2 = np.cos(2.5 * X + 0.7).sum(1, keepdims=True)
y3 = np.sin(2 * X + 1.3).sum(1, keepdims=True)
c1 = ((X - 0.5) ** 2).sum(1, keepdims=True)        # inside a ball about the centre ...
c2 = np.sin(4 * X[:, :2]).sum(1, keepdims=True)    # ... and on one side of a wave
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
gp = lambda length, y: api.DeviceGPMCMC(np.array([1.0] + [length] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)  # noqa: E731
objs = [gp(0.4, y1), gp(0.5, y2), gp(0.45, y3)]
cons = [gp(0.5, c1), gp(0.4, c2)]
tau = [float(np.median(c1)), float(np.median(c2))]
ref = (float(y1.max()) + 0.5, float(y2.max()) + 0.5, float(y3.max()) + 0.5)
front, full = staircase(F, ref), staircase(FULL, ref)
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)

log1 = lambda: api.log_ehvi3_constrained_suggest(objs, cons, tau, ref, front, gd, bounds, starts, 1)  # noqa: E731
plain1 = lambda: api.ehvi_constrained_suggest(objs, cons, tau, ref, front, gd, bounds, starts, 1)  # noqa: E731
loop1 = lambda: host_loop(objs, cons, tau, ref, front, bounds, starts)  # noqa: E731
logf = lambda: api.log_ehvi3_constrained_suggest(objs, cons, tau, ref, full, gd, bounds, starts, 1)  # noqa: E731
plainf = lambda: api.ehvi_constrained_suggest(objs, cons, tau, ref, full, gd, bounds, starts, 1)  # noqa: E731

if "--suggestions" in sys.argv:
    a, b = (plainf, logf) if "--staircase" in sys.argv else (plain1, log1)
    for _ in range(int(sys.argv[sys.argv.index("--suggestions") + 1])):
        a()
        b()
    sys.exit(0)

say("sustained FP64 FMA rate before: %.1f TFLOP/s" % api.fp64_rate())
say("%d members, three objectives, K = %d constraints (%d GPs), n = %d, d = %d, %d starts -> 20 kept, %d x %d steps, a front of %d "
    "points (%d boxes)" % (E, K, E * (3 + K), N, D, STARTS, ROUNDS, STEPS, F, (F + 1) * (F + 2) // 2))
got, want, looped = log1(), plain1(), loop1()
say("  log form %.12g at %s; host loop %.12g, the same point: %s" % (
    got["values"][0], np.round(got["points"][0], 6).tolist(), looped[1], bool(np.array_equal(looped[0], got["points"][0]))))
say("  plain form %.12g (its log %.12g) at %s" % (want["values"][0], np.log(want["values"][0]), np.round(want["points"][0], 6).tolist()))
compare("one suggestion, K = %d, a front of %d:" % (K, F), [("ehvi_constrained_suggest (M = 3)", plain1), ("log_ehvi3_constrained_suggest", log1),
                                                             ("host loop over log_ehvi3_constrained_ensemble", loop1)])

compare("one suggestion, K = %d, a staircase of %d (%d boxes):" % (K, FULL, (FULL + 1) * (FULL + 2) // 2),
        [("ehvi_constrained_suggest (M = 3)", plainf), ("log_ehvi3_constrained_suggest", logf)])

logq = lambda: api.log_ehvi3_constrained_suggest(objs, cons, tau, ref, front, gd, bounds, starts, Q)  # noqa: E731
plainq = lambda: api.ehvi_constrained_suggest(objs, cons, tau, ref, front, gd, bounds, starts, Q)  # noqa: E731
compare("a greedy batch of q = %d, K = %d, a front of %d:" % (Q, K, F), [("ehvi_constrained_suggest (M = 3)", plainq),
                                                                          ("log_ehvi3_constrained_suggest", logq)])
say("  values of the %d picks, log form: %s" % (Q, " ".join("%.6g" % v for v in logq()["values"])))

log0 = lambda: api.log_ehvi3_constrained_suggest(objs, None, None, ref, front, gd, bounds, starts, 1)  # noqa: E731
free0 = lambda: api.ehvi3_suggest(objs[0], objs[1], objs[2], ref, front, gd, bounds, starts, 1)  # noqa: E731
compare("one suggestion, K = 0, a front of %d:" % F, [("ehvi3_suggest", free0), ("log_ehvi3_constrained_suggest, K = 0", log0)])

cand = rng.uniform(size=(CANDIDATES, D))
for name, fr in (("a front of %d" % F, front), ("the staircase of %d" % FULL, full)):
    for g in (False, True):
        pe = lambda: api.ehvi_constrained_ensemble(objs, cons, tau, ref, fr, cand, want_grad=g)  # noqa: E731
        le = lambda: api.log_ehvi3_constrained_ensemble(objs, cons, tau, ref, fr, cand, want_grad=g)  # noqa: E731
        t = compare("evaluate %d candidates, %s, want_grad = %d:" % (CANDIDATES, name, g), [("ehvi_constrained_ensemble (M = 3)", pe),
                                                                                          ("log_ehvi3_constrained_ensemble", le)])
        extra = 1e3 * (t["log_ehvi3_constrained_ensemble"] - t["ehvi_constrained_ensemble (M = 3)"]) / (CANDIDATES * E)
        say("  the log call's extra time over the %d x %d (candidate, member) pairs: %.3f us per pair" % (CANDIDATES, E, extra))
for m in objs + cons:
    for g in m.gps:
        g.close()
say("sustained FP64 FMA rate after: %.1f TFLOP/s" % api.fp64_rate())
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
