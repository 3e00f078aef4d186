"""Time one suggestion by the ensemble-averaged min-value entropy acquisition GIBBON: api.gibbon_multistart
(moe_gibbon_mcmc_multistart: the evaluation, the step and the rounds on the device, ensemble-wide launches; csrc/gibbon1.hip) against
the host-driven loop -- tests/ms_restatement.py's optimiser with every evaluation one api.gibbon_ensemble call -- on the same starts;
no other path to this objective exists.  The suggestion by the analytic expected improvement (api.ei_analytic_multistart) with the
same settings stands beside it.  16 members, n = 500, d = 6, 200 Latin-hypercube starts of which 20 are kept, 2 rounds of 50 steps,
K = 64 min-values per member drawn by min_value_entropy.sample_min_values at 600 Latin-hypercube candidates.
   python tools/gibbon_time.py [--out profiles/gibbon_time.txt] [--repeat 9]

All on one build, alternated in one process, median of --repeat whole suggestions (host clock around calls that end in a device
synchronise).  Then a greedy batch of q = 4 in one call (api.gibbon_suggest) against four calls of the ascent each fed its
predecessors (the same bits, asserted), and one evaluation of 1024 candidates with gradient at K = 64 against K = 1024.  No threshold
is set; a ratio near or under 1 is a finding, not a failure."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the host-driven loop is the tests' restatement of the optimiser
from cornell_moe_amd import api, min_value_entropy as mve  # noqa: E402
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


E, N, D, STARTS, STEPS, ROUNDS, Q, K = 16, 500, 6, 200, 50, 2, 4, 64
repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 9
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


def med_min(t):
    return "%9.1f / %8.1f" % (np.median(t), min(t))


def host_loop(ens, mins, bounds, starts):
    vals = api.gibbon_ensemble(ens, starts, mins, want_grad=False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: api.gibbon_ensemble(ens, np.asarray(x).reshape(-1, D), mins)[1].reshape(np.shape(x)), gd, bounds,
                              starts[order])
    end_vals = api.gibbon_ensemble(ens, ends, mins, want_grad=False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


def host_calls(ens, mins, bounds, starts):
    points, values = [], []
    for _ in range(Q):
        res = api.gibbon_multistart(ens, gd, bounds, mins, starts, points_being_sampled=np.array(points) if points else None)
        points.append(res["point"])
        values.append(res["value"])
    return np.array(points), np.array(values)


clocks("before")
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y = np.sin(3 * X).sum(1, keepdims=True)
hypers = np.array([1.0] + [0.4] * D)[None, :] * np.exp(0.15 * rng.standard_normal((E, D + 1)))  # the spread of a hyper-parameter chain
ens = api.DeviceGPMCMC(hypers, np.full((E, 1), 1e-2), X, y)
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
bests = [float(y[:, 0].min())] * E
t0 = time.perf_counter()
mins = mve.sample_min_values(ens, api.latin_hypercube(6, bounds, 600), K, 7)
say("%d members, n = %d, d = %d, %d starts -> 20 kept, %d x %d steps, K = %d; whole suggestions, median / min of %d, alternated" % (
    E, N, D, STARTS, ROUNDS, STEPS, K, repeat))
say("min-values: %d x %d draws at 600 candidates in %.1f ms (first call), from %.3f to %.3f; the best observed value is %.3f" % (
    E, K, 1e3 * (time.perf_counter() - t0), mins.min(), mins.max(), bests[0]))
one = lambda: api.gibbon_multistart(ens, gd, bounds, mins, starts)  # noqa: E731
loop = lambda: host_loop(ens, mins, bounds, starts)  # noqa: E731
ei = lambda: api.ei_analytic_multistart(ens, gd, bounds, bests, starts)  # noqa: E731
new_res, loop_res, ei_res = one(), loop(), ei()  # workspaces
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
say("moe_gibbon_mcmc_multistart %s ms | host loop over moe_gibbon_mcmc %s ms (med/min) | ratio %.2fx" % (
    med_min(t_one), med_min(t_loop), np.median(t_loop) / np.median(t_one)))
say("moe_ei_analytic_mcmc_multistart, the same settings %s ms (med/min) | GIBBON / EI %.2fx" % (
    med_min(t_ei), np.median(t_one) / np.median(t_ei)))
say("  GIBBON %.12g at %s (one call)" % (new_res["value"], np.round(new_res["point"], 6).tolist()))
say("  GIBBON %.12g at %s (host loop); the same point: %s" % (loop_res[1], np.round(loop_res[0], 6).tolist(),
                                                              bool(np.array_equal(loop_res[0], new_res["point"]))))
say("  EI %.12g at %s" % (ei_res["value"], np.round(ei_res["point"], 6).tolist()))

batch = lambda: api.gibbon_suggest(ens, gd, bounds, mins, starts, Q)  # noqa: E731
res = batch()
points, values = host_calls(ens, mins, bounds, starts)
assert np.array_equal(res["points"], points) and np.array_equal(res["values"], values)
t_one, t_host = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    batch()
    t1 = time.perf_counter()
    host_calls(ens, mins, bounds, starts)
    t2 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_host.append(1e3 * (t2 - t1))
say("greedy q = %d: one call %s ms | %d calls %s ms (med/min) | ratio %.2fx" % (Q, med_min(t_one), Q, med_min(t_host),
                                                                               np.median(t_host) / np.median(t_one)))
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in values)))

cand = np.random.default_rng(2).uniform(size=(1024, D))
many = mve.sample_min_values(ens, api.latin_hypercube(6, bounds, 600), 1024, 7)
t = {64: [], 1024: []}
for k, m in ((64, mins), (1024, many)):
    api.gibbon_ensemble(ens, cand, m)  # workspaces
for _ in range(repeat):
    for k, m in ((64, mins), (1024, many)):
        t0 = time.perf_counter()
        api.gibbon_ensemble(ens, cand, m)
        t[k].append(1e3 * (time.perf_counter() - t0))
say("1024 candidates with gradient, %d members: K = 64 %s ms, K = 1024 %s ms (med/min), ratio %.2fx" % (
    E, med_min(t[64]), med_min(t[1024]), np.median(t[1024]) / np.median(t[64])))
for g in ens.gps:
    g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
