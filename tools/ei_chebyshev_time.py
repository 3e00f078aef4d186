"""Time one suggestion by the ensemble-averaged Chebyshev-scalarised expected improvement (api.ei_chebyshev_suggest:
moe_ei_chebyshev_mcmc_suggest, csrc/chebei1.hip) at M = 3 beside the same suggestion by the three-objective expected hypervolume
improvement (api.ehvi3_suggest: the existing call and the yardstick) at a front of 32 points and at a staircase of 192 (18 721
boxes), against the host-driven loop -- tests/ms_restatement.py's optimiser with every evaluation one api.ei_chebyshev_ensemble call
-- and at M = 4 and M = 8, at the shapes of tools/log_ehvi3_time.py: 16 members, n = 500, d = 6, 200 Latin-hypercube starts of
which 20 are kept, 2 rounds of 50 steps.  Then a greedy batch of q = 4 with four weight vectors, and the evaluate calls of both
acquisitions at 512 candidates, value only and with the gradient: the chain of the 3 x 16 GPs is the same in both, so the
difference over the 512 x 16 (candidate, member) pairs is the node kernel's time per evaluation beside the box kernel's.
   python tools/ei_chebyshev_time.py [--out profiles/ei_chebyshev_time.txt] [--windows 5]
   python tools/ei_chebyshev_time.py --suggestions 3     (nothing timed: staircase suggestions by both, for a kernel trace)

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


E, N, D, STARTS, STEPS, ROUNDS, Q, F, FULL, CANDIDATES, MMAX = 16, 500, 6, 200, 50, 2, 4, 32, 192, 512, 8
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
        say("  %-44s ms per call, %d windows: %s | median %.2f, spread %.2f to %.2f" % (
            name, windows, " ".join("%.2f" % v for v in t[name]), np.median(t[name]), min(t[name]), max(t[name])))
    base = t[calls[0][0]]
    for name, _ in calls[1:]:
        m = float(np.median(t[name]))
        say("  %s / %s by medians: %.3f; its median lies %s the baseline's own spread" % (
            name, calls[0][0], m / np.median(base), "inside" if min(base) <= m <= max(base) else "OUTSIDE"))
    return {name: float(np.median(v)) for name, v in t.items()}


def staircase(count, ref):
    """count mutually non-dominated points strictly inside ref, u ascending, v descending, w ascending: every slab keeps all its
    points, (count + 1)(count + 2) / 2 boxes, in the canonical order (tools/log_ehvi3_time.py's)"""
    t = (np.arange(count) + 0.5) / count
    return np.ascontiguousarray(np.stack([ref[0] - 4.0 * (1.0 - t) ** 2 - 0.5, ref[1] - 4.0 * t ** 2 - 0.5, ref[2] - 4.5 + 4.0 * t], axis=1))


rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
ys = [np.sin((3.0 - 0.25 * j) * X + 0.7 * j).sum(1, keepdims=True) for j in range(MMAX)]
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
gp = lambda length, y: api.DeviceGPMCMC(np.array([1.0] + [length] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)  # noqa: E731
objs = [gp(0.4 + 0.02 * j, ys[j]) for j in range(MMAX)]
Y = np.hstack(ys)
ideal, nadir = Y.min(axis=0), Y.max(axis=0)
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)


def rounds(M, q, seed=3):
    """q scalarisations [q][2 M] over the first M objectives and every member's observed incumbents under each [q][E]"""
    w = esi.sample_simplex_weights(q, M, seed)
    scal, best = [], []
    for t in range(q):
        a, b = esi.chebyshev_scalarisation(w[t], ideal[:M], nadir[:M])
        scal.append(np.concatenate([a, b]))
        best.append([esi.chebyshev_best_so_far(Y[:, :M], a, b)] * E)
    return np.array(scal), np.array(best)


def cheb(M, q=1):
    scal, best = rounds(M, q)
    return lambda: api.ei_chebyshev_suggest(objs[:M], scal, best, gd, bounds, starts, q)


def host_loop(M):
    scal, best = rounds(M, 1)
    ev = lambda x, g: api.ei_chebyshev_ensemble(objs[:M], scal[0], best[0], np.asarray(x).reshape(-1, D), want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


ref = tuple(float(v) + 0.5 for v in nadir[:3])
front, full = staircase(F, ref), staircase(FULL, ref)
box32 = lambda: api.ehvi3_suggest(objs[0], objs[1], objs[2], ref, front, gd, bounds, starts, 1)  # noqa: E731
box192 = lambda: api.ehvi3_suggest(objs[0], objs[1], objs[2], ref, full, gd, bounds, starts, 1)  # noqa: E731
cheb3 = cheb(3)

if "--suggestions" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--suggestions") + 1])):
        box192()
        cheb3()
    sys.exit(0)

say("sustained FP64 FMA rate before: %.1f TFLOP/s" % api.fp64_rate())
say("%d members, n = %d, d = %d, %d starts -> 20 kept, %d x %d steps" % (E, N, D, STARTS, ROUNDS, STEPS))
got, looped = cheb3(), host_loop(3)
say("  M = 3: one call %.12g at %s; host loop %.12g, the same point: %s" % (
    got["values"][0], np.round(got["points"][0], 6).tolist(), looped[1], bool(np.array_equal(looped[0], got["points"][0]))))
compare("one suggestion, M = 3, beside the box sum:", [("ehvi3_suggest, a front of %d" % F, box32), ("ehvi3_suggest, a staircase of %d" % FULL, box192),
                                                        ("ei_chebyshev_suggest, M = 3", cheb3),
                                                        ("host loop over ei_chebyshev_ensemble, M = 3", lambda: host_loop(3))])
compare("one suggestion by the number of objectives:", [("ei_chebyshev_suggest, M = 3", cheb3), ("ei_chebyshev_suggest, M = 4", cheb(4)),
                                                         ("ei_chebyshev_suggest, M = 8", cheb(8))])
batch = cheb(4, Q)
compare("a greedy batch of q = %d with %d weight vectors, M = 4:" % (Q, Q), [("ei_chebyshev_suggest, M = 4, q = 1", cheb(4)),
                                                                            ("ei_chebyshev_suggest, M = 4, q = %d" % Q, batch)])
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in batch()["values"])))

cand = rng.uniform(size=(CANDIDATES, D))
scal3, best3 = rounds(3, 1)
for g in (False, True):
    b32 = lambda: api.ehvi3_ensemble(objs[0], objs[1], objs[2], ref, front, cand, want_grad=g)  # noqa: E731
    b192 = lambda: api.ehvi3_ensemble(objs[0], objs[1], objs[2], ref, full, cand, want_grad=g)  # noqa: E731
    ce = lambda: api.ei_chebyshev_ensemble(objs[:3], scal3[0], best3[0], cand, want_grad=g)  # noqa: E731
    t = compare("evaluate %d candidates, M = 3, want_grad = %d:" % (CANDIDATES, g), [
        ("ehvi3_ensemble, a front of %d" % F, b32), ("ehvi3_ensemble, a staircase of %d" % FULL, b192), ("ei_chebyshev_ensemble", ce)])
    pairs = CANDIDATES * E
    say("  over the %d x %d (candidate, member) pairs: the staircase call costs %.3f us per pair more than the front of %d, the "
        "Chebyshev call %.3f us per pair more than the front of %d" % (
            CANDIDATES, E, 1e3 * (t["ehvi3_ensemble, a staircase of %d" % FULL] - t["ehvi3_ensemble, a front of %d" % F]) / pairs, F,
            1e3 * (t["ei_chebyshev_ensemble"] - t["ehvi3_ensemble, a front of %d" % F]) / pairs, F))
for m in objs:
    for g in m.gps:
        g.close()
say("sustained FP64 FMA rate after: %.1f TFLOP/s" % api.fp64_rate())
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
