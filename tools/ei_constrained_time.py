"""Time one suggestion by the ensemble-averaged constrained expected improvement: api.ei_constrained_multistart
(moe_ei_constrained_mcmc_multistart: the evaluation, the product rule, the step and the rounds on the device, ensemble-wide launches;
csrc/cei1.hip) against the host-driven loop -- tests/ms_restatement.py's optimiser with every evaluation one
api.ei_constrained_ensemble call -- on the same starts; no other path to this objective exists.  The suggestion by the analytic
expected improvement on the objective GPs alone (api.ei_analytic_multistart) with the same settings stands beside it: each of the
1 + K GPs of a member runs EI's chain, so the expectation is about (1 + K) times its GPU time.  16 members, K = 2 constraints,
n = 500, d = 6, 200 Latin-hypercube starts of which 20 are kept, 2 rounds of 50 steps.
   python tools/ei_constrained_time.py [--out profiles/ei_constrained_time.txt] [--repeat 9]

All on one build, alternated in one process, median of --repeat whole calls (host clock around calls that end in a device
synchronise).  Then a greedy batch of q = 4 in one call (api.ei_constrained_suggest) against four calls of the ascent each fed its
predecessors (the same bits, asserted), one suggestion at K = 0 against K = 4, and what moe_ensemble_launch_stats counts for one
suggestion.  No threshold is set; a ratio near or under 1 is a finding, not a failure."""
import ctypes as C
import os
import subprocess
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


def clocks(tag):
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             universal_newlines=True, timeout=60).stdout
        got = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln or "fclk" in ln]
        say("clocks %s: %s" % (tag, "; ".join(got) if got else "rocm-smi printed none"))
    except Exception as e:  # noqa: BLE001
        say("clocks %s: rocm-smi not available (%s)" % (tag, type(e).__name__))
    say("sustained FP64 FMA rate %s: %.1f TFLOP/s" % (tag, api.fp64_rate()))


E, N, D, STARTS, STEPS, ROUNDS, Q, K, KMAX = 16, 500, 6, 200, 50, 2, 4, 2, 4
repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 9
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


def med_min(t):
    return "%9.1f / %8.1f" % (np.median(t), min(t))


def stats():
    out = (C.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return np.array(list(out), dtype=np.int64)


def host_loop(ens, cons, tau, bests, bounds, starts):
    ev = lambda x, g: api.ei_constrained_ensemble(ens, cons, tau, np.asarray(x).reshape(-1, D), bests, want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


def host_calls(ens, cons, tau, bests, bounds, starts):
    points, values = [], []
    for _ in range(Q):
        res = api.ei_constrained_multistart(ens, cons, tau, gd, bounds, bests, starts,
                                            points_being_sampled=np.array(points) if points else None)
        points.append(res["point"])
        values.append(res["value"])
    return np.array(points), np.array(values)


clocks("before")
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y = np.sin(3 * X).sum(1, keepdims=True)
# constraint k: a smooth function of its own, about half of the box feasible under the threshold 0
cvals = [np.cos(2.5 * X + 0.7 * k).sum(1, keepdims=True) - np.median(np.cos(2.5 * X + 0.7 * k).sum(1)) for k in range(KMAX)]
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
ens = api.DeviceGPMCMC(np.array([1.0] + [0.4] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)
cons_all = [api.DeviceGPMCMC(np.array([1.0] + [0.5] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, c) for c in cvals]
tau_all = [0.0] * KMAX
cons, tau = cons_all[:K], tau_all[:K]
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
best = eic.best_feasible_value(y, np.hstack(cvals[:K]), tau)
bests = [best] * E
say("%d members, K = %d constraints (%d GPs), n = %d, d = %d, %d starts -> 20 kept, %d x %d steps; whole calls, median / min of %d, "
    "alternated" % (E, K, E * (1 + K), N, D, STARTS, ROUNDS, STEPS, repeat))
say("best feasible observed value %.3f (the best observed value is %.3f; %d of %d observations are feasible)" % (
    best, float(y.min()), int(np.sum(np.all(np.hstack(cvals[:K]) <= 0.0, axis=1))), N))
one = lambda: api.ei_constrained_multistart(ens, cons, tau, gd, bounds, bests, starts)  # noqa: E731
loop = lambda: host_loop(ens, cons, tau, bests, bounds, starts)  # noqa: E731
ei = lambda: api.ei_analytic_multistart(ens, gd, bounds, bests, starts)  # noqa: E731
new_res, loop_res, ei_res = one(), loop(), ei()  # workspaces
s0 = stats()
one()
ds = stats() - s0
say("moe_ensemble_launch_stats for one suggestion: %d evaluations issued zipped, %d member by member; %d launches issued for %d "
    "recorded (x%.1f fewer)" % (ds[0], ds[1], ds[2], ds[3], ds[3] / max(ds[2], 1)))
t_one, t_loop, t_ei = [], [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    one()
    t1 = time.perf_counter()
    loop()
    t2 = time.perf_counter()
    ei()
    t3 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_loop.append(1e3 * (t2 - t1))
    t_ei.append(1e3 * (t3 - t2))
say("moe_ei_constrained_mcmc_multistart %s ms | host loop over moe_ei_constrained_mcmc %s ms (med/min) | ratio %.2fx" % (
    med_min(t_one), med_min(t_loop), np.median(t_loop) / np.median(t_one)))
say("moe_ei_analytic_mcmc_multistart on the objective GPs alone, the same settings %s ms (med/min) | constrained / EI %.2fx "
    "(expected about 1 + K = %d)" % (med_min(t_ei), np.median(t_one) / np.median(t_ei), 1 + K))
say("  constrained EI %.12g at %s (one call)" % (new_res["value"], np.round(new_res["point"], 6).tolist()))
say("  constrained EI %.12g at %s (host loop); the same point: %s" % (loop_res[1], np.round(loop_res[0], 6).tolist(),
                                                                      bool(np.array_equal(loop_res[0], new_res["point"]))))
say("  EI %.12g at %s" % (ei_res["value"], np.round(ei_res["point"], 6).tolist()))

batch = lambda: api.ei_constrained_suggest(ens, cons, tau, gd, bounds, bests, starts, Q)  # noqa: E731
res = batch()
points, values = host_calls(ens, cons, tau, bests, bounds, starts)
assert np.array_equal(res["points"], points) and np.array_equal(res["values"], values)
t_one, t_host = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    batch()
    t1 = time.perf_counter()
    host_calls(ens, cons, tau, bests, bounds, starts)
    t2 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_host.append(1e3 * (t2 - t1))
say("greedy q = %d: one call %s ms | %d calls %s ms (med/min) | ratio %.2fx" % (Q, med_min(t_one), Q, med_min(t_host),
                                                                               np.median(t_host) / np.median(t_one)))
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in values)))

best4 = [eic.best_feasible_value(y, np.hstack(cvals), tau_all)] * E
runs = {0: lambda: api.ei_constrained_multistart(ens, None, None, gd, bounds, bests, starts),  # noqa: E731
        KMAX: lambda: api.ei_constrained_multistart(ens, cons_all, tau_all, gd, bounds, best4, starts)}  # noqa: E731
t = {0: [], KMAX: []}
for k in runs:
    runs[k]()  # workspaces
for _ in range(repeat):
    for k in runs:
        t0 = time.perf_counter()
        runs[k]()
        t[k].append(1e3 * (time.perf_counter() - t0))
say("one suggestion, %d members: K = 0 %s ms, K = %d %s ms (med/min), ratio %.2fx (expected about %d)" % (
    E, med_min(t[0]), KMAX, med_min(t[KMAX]), np.median(t[KMAX]) / np.median(t[0]), 1 + KMAX))
for m in [ens] + cons_all:
    for g in m.gps:
        g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
