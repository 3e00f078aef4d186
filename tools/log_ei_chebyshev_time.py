"""Time one suggestion by the log Chebyshev-scalarised expected improvement (api.log_ei_chebyshev_constrained_suggest:
moe_log_ei_chebyshev_constrained_mcmc_suggest, csrc/logchebei1.hip) at M = 4, K = 0 beside the same suggestion by the plain form
(api.ei_chebyshev_suggest: the existing call and the yardstick) in the same run, at M = 4, K = 2 against the host-driven loop --
tests/ms_restatement.py's optimiser with every evaluation one api.log_ei_chebyshev_constrained_ensemble call -- and at M = 8, K = 0,
at the shapes of tools/ei_chebyshev_time.py: 16 members, n = 500, d = 6, 200 Latin-hypercube starts of which 20 are kept, 2 rounds
of 50 steps.  Then a greedy batch of q = 4 with four weight vectors at M = 4, K = 2, and the evaluate calls of both forms at 512
candidates, value only and with the gradient: the chain of the 4 x 16 GPs is the same in both, so the difference over the 512 x 16
(candidate, member) pairs is the log-node kernel's time per evaluation beside the node kernel's.
   python tools/log_ei_chebyshev_time.py [--out profiles/log_ei_chebyshev_time.txt] [--windows 5]
   python tools/log_ei_chebyshev_time.py --suggestions 3     (nothing timed: M = 4 suggestions by both forms, for a kernel trace)

All on one build in one process: a warm-up call of every shape, then --windows windows of more than a second per call, the calls of
a comparison alternated window by window; a window's figure is its wall time over its calls (host clock around calls that end in a
device synchronise).  No ratio is set in advance and no time is asserted; the windows and medians are a finding.  The kernels' own
times come from a kernel trace of the --suggestions run (tools/ktrace_cmd.sh)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the host-driven loop is the tests' restatement of the optimiser
from cornell_moe_amd import api, expected_scalarised_improvement as esi  # noqa: E402
import ms_restatement as ms  # noqa: E402

lines = []


def say(text):
    print(text)
    sys.stdout.flush()
    lines.append(text)


E, N, D, STARTS, STEPS, ROUNDS, Q, CANDIDATES, MMAX, KMAX = 16, 500, 6, 200, 50, 2, 4, 512, 8, 2
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
        say("  %-52s ms per call, %d windows: %s | median %.2f, spread %.2f to %.2f" % (
            name, windows, " ".join("%.2f" % v for v in t[name]), np.median(t[name]), min(t[name]), max(t[name])))
    base = t[calls[0][0]]
    for name, _ in calls[1:]:
        m = float(np.median(t[name]))
        say("  %s / %s by medians: %.3f; its median lies %s the baseline's own spread" % (
            name, calls[0][0], m / np.median(base), "inside" if min(base) <= m <= max(base) else "OUTSIDE"))
    return {name: float(np.median(v)) for name, v in t.items()}


rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
ys = [np.sin((3.0 - 0.25 * j) * X + 0.7 * j).sum(1, keepdims=True) for j in range(MMAX)]
cs = [np.cos((2.0 + 0.5 * k) * X + 0.3 * k).sum(1, keepdims=True) for k in range(KMAX)]
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
gp = lambda length, y: api.DeviceGPMCMC(np.array([1.0] + [length] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)  # noqa: E731
objs = [gp(0.4 + 0.02 * j, ys[j]) for j in range(MMAX)]
cons = [gp(0.45 + 0.02 * k, cs[k]) for k in range(KMAX)]
Y, CY = np.hstack(ys), np.hstack(cs)
taus = [float(np.median(CY[:, k])) for k in range(KMAX)]  # (half the observations satisfy each constraint)
ideal, nadir = Y.min(axis=0), Y.max(axis=0)
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)


def rounds(M, K, q, seed=3):
    """q scalarisations [q][2 M] over the first M objectives and every member's incumbents of the feasible observations [q][E]"""
    w = esi.sample_simplex_weights(q, M, seed)
    scal, best = [], []
    for t in range(q):
        a, b = esi.chebyshev_scalarisation(w[t], ideal[:M], nadir[:M])
        scal.append(np.concatenate([a, b]))
        best.append([esi.feasible_chebyshev_best_so_far(Y[:, :M], CY[:, :K], taus[:K], a, b)] * E)
    return np.array(scal), np.array(best)


def plain(M, q=1):
    scal, best = rounds(M, 0, q)
    return lambda: api.ei_chebyshev_suggest(objs[:M], scal, best, gd, bounds, starts, q)


def log_form(M, K, q=1):
    scal, best = rounds(M, K, q)
    return lambda: api.log_ei_chebyshev_constrained_suggest(objs[:M], cons[:K] or None, taus[:K] or None, scal, best, gd, bounds,
                                                            starts, q)


def host_loop(M, K):
    scal, best = rounds(M, K, 1)
    ev = lambda x, g: api.log_ei_chebyshev_constrained_ensemble(  # noqa: E731
        objs[:M], cons[:K] or None, taus[:K] or None, scal[0], best[0], np.asarray(x).reshape(-1, D), want_grad=g)
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


plain4, log4, log42 = plain(4), log_form(4, 0), log_form(4, 2)

if "--suggestions" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--suggestions") + 1])):
        plain4()
        log4()
    sys.exit(0)

say("sustained FP64 FMA rate before: %.1f TFLOP/s" % api.fp64_rate())
say("%d members, n = %d, d = %d, %d starts -> 20 kept, %d x %d steps" % (E, N, D, STARTS, ROUNDS, STEPS))
a, b = plain4(), log4()
say("  M = 4, K = 0: the plain form %.12g at %s; the log form %.12g (exp: %.6g) at %s" % (
    a["values"][0], np.round(a["points"][0], 6).tolist(), b["values"][0], np.exp(b["values"][0]), np.round(b["points"][0], 6).tolist()))
got, looped = log42(), host_loop(4, 2)
say("  M = 4, K = 2: one call %.12g at %s; host loop %.12g, the same point: %s" % (
    got["values"][0], np.round(got["points"][0], 6).tolist(), looped[1], bool(np.array_equal(looped[0], got["points"][0]))))
compare("one suggestion, M = 4, K = 0, the plain form above the log form:", [
    ("ei_chebyshev_suggest, M = 4", plain4), ("log_ei_chebyshev_constrained_suggest, M = 4, K = 0", log4)])
compare("one suggestion, M = 4, K = 2, beside the host-driven loop:", [
    ("log_ei_chebyshev_constrained_suggest, M = 4, K = 2", log42), ("host loop over the evaluator, M = 4, K = 2", lambda: host_loop(4, 2))])
compare("one suggestion, M = 8, K = 0:", [("ei_chebyshev_suggest, M = 8", plain(8)),
                                          ("log_ei_chebyshev_constrained_suggest, M = 8, K = 0", log_form(8, 0))])
batch = log_form(4, 2, Q)
compare("a greedy batch of q = %d with %d weight vectors, M = 4, K = 2:" % (Q, Q), [
    ("log_ei_chebyshev_constrained_suggest, q = 1", log42), ("log_ei_chebyshev_constrained_suggest, q = %d" % Q, batch)])
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in batch()["values"])))

cand = rng.uniform(size=(CANDIDATES, D))
scal4, best4 = rounds(4, 0, 1)
for g in (False, True):
    pe = lambda: api.ei_chebyshev_ensemble(objs[:4], scal4[0], best4[0], cand, want_grad=g)  # noqa: E731
    le = lambda: api.log_ei_chebyshev_constrained_ensemble(objs[:4], None, None, scal4[0], best4[0], cand, want_grad=g)  # noqa: E731
    t = compare("evaluate %d candidates, M = 4, K = 0, want_grad = %d:" % (CANDIDATES, g), [
        ("ei_chebyshev_ensemble", pe), ("log_ei_chebyshev_constrained_ensemble", le)])
    say("  over the %d x %d (candidate, member) pairs: the log call costs %.3f us per pair more than the plain one" % (
        CANDIDATES, E, 1e3 * (t["log_ei_chebyshev_constrained_ensemble"] - t["ei_chebyshev_ensemble"]) / (CANDIDATES * E)))
for m in objs + cons:
    for g in m.gps:
        g.close()
say("sustained FP64 FMA rate after: %.1f TFLOP/s" % api.fp64_rate())
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
