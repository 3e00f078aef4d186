"""Time one suggestion by the ensemble-averaged analytic expected improvement: api.ei_analytic_multistart
(moe_ei_analytic_mcmc_multistart: the evaluation, the step and the rounds on the device, ensemble-wide launches; csrc/ei1.hip)
against DeviceGPMCMC.ei_multistart at q = 1 (moe_ei_mcmc_multistart: one batched state pass per member and step, every point's state
copied back, mu, sigma^2, EI and grad EI finished per point in host code), on the same starts.  16 members, n = 500, d = 6, 200
Latin-hypercube starts of which 20 are kept, 2 rounds of 50 steps.
   python tools/ei_analytic_time.py [--out profiles/ei_analytic_time.txt] [--repeat 9] [--derivatives G]

--derivatives G: every member also observes the first G partial derivatives at every point (N = n (1 + G) rows; G = 3 is the
shape of BASELINE.json's d-KG configuration scaled to n = 500), the pending evaluation runs with p = 4 (16 extension rows at G = 3),
and the lines are APPENDED to --out.  moe_ei_mcmc_multistart is the only other path such GPs have.

Both run on the same build, alternated in one process, median of --repeat whole suggestions (host clock around calls that end in a
device synchronise).  The two paths need not return the same point to the last bit (their arithmetic order differs): the distance
between their end points is reported beside the times.  Then a greedy batch of q = 4 in one call (api.ei_analytic_suggest) against
four calls of the ascent each fed its predecessors (the same bits, asserted), and one evaluation of 1024 candidates with p = 8
pending points against p = 0 (p = 4 with --derivatives).  No threshold is set; a ratio near or under 1 is a finding, not a failure."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from cornell_moe_amd import api  # noqa: E402

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


E, N, D, STARTS, STEPS, ROUNDS, Q = 16, 500, 6, 200, 50, 2, 4
repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 9
G = int(sys.argv[sys.argv.index("--derivatives") + 1]) if "--derivatives" in sys.argv else 0
DERIVS = tuple(range(G))
PEND = 4 if G else 8
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


def med_min(t):
    return "%9.1f / %8.1f" % (np.median(t), min(t))


def host_calls(ens, bests, bounds, starts):
    points, values = [], []
    for _ in range(Q):
        res = api.ei_analytic_multistart(ens, gd, bounds, bests, starts, points_being_sampled=np.array(points) if points else None)
        points.append(res["point"])
        values.append(res["value"])
    return np.array(points), np.array(values)


clocks("before")
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y = np.hstack([np.sin(3 * X).sum(1, keepdims=True)] + [3 * np.cos(3 * X[:, i:i + 1]) for i in DERIVS])
hypers = np.array([1.0] + [0.4] * D)[None, :] * np.exp(0.15 * rng.standard_normal((E, D + 1)))  # the spread of a hyper-parameter chain
ens = api.DeviceGPMCMC(hypers, np.full((E, 1 + G), 1e-2), X, y, DERIVS)
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
bests = [float(y[:, 0].min())] * E

if G:
    say("derivatives %s observed: N = %d rows per member" % (list(DERIVS), N * (1 + G)))
say("%d members, n = %d, d = %d, %d starts -> 20 kept, %d x %d steps; whole suggestions, median / min of %d, alternated" % (
    E, N, D, STARTS, ROUNDS, STEPS, repeat))
one = lambda: api.ei_analytic_multistart(ens, gd, bounds, bests, starts)  # noqa: E731
old = lambda: ens.ei_multistart(gd, bounds, starts.reshape(STARTS, 1, D), None, 1, bests, None)  # noqa: E731
new_res, old_res = one(), old()  # workspaces
t_one, t_old = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    one()
    t1 = time.perf_counter()
    old()
    t2 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_old.append(1e3 * (t2 - t1))
say("moe_ei_analytic_mcmc_multistart %s ms | moe_ei_mcmc_multistart q = 1 %s ms (med/min) | ratio %.2fx" % (
    med_min(t_one), med_min(t_old), np.median(t_old) / np.median(t_one)))
say("  EI %.12g at %s (one call)" % (new_res["value"], np.round(new_res["point"], 6).tolist()))
say("  EI %.12g at %s (host-finished); distance between the end points %.3g" % (
    old_res[1], np.round(old_res[0].ravel(), 6).tolist(), float(np.linalg.norm(new_res["point"] - old_res[0].ravel()))))

batch = lambda: api.ei_analytic_suggest(ens, gd, bounds, bests, starts, Q)  # noqa: E731
res = batch()
points, values = host_calls(ens, bests, bounds, starts)
assert np.array_equal(res["points"], points) and np.array_equal(res["values"], values)
t_one, t_host = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    batch()
    t1 = time.perf_counter()
    host_calls(ens, bests, bounds, starts)
    t2 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_host.append(1e3 * (t2 - t1))
say("greedy q = %d: one call %s ms | %d calls %s ms (med/min) | ratio %.2fx" % (Q, med_min(t_one), Q, med_min(t_host),
                                                                               np.median(t_host) / np.median(t_one)))
say("  EI of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in values)))

cand = np.random.default_rng(2).uniform(size=(1024, D))
pend = np.random.default_rng(3).uniform(size=(PEND, D))
t = {0: [], PEND: []}
for p in (0, PEND):
    api.ei_analytic_ensemble(ens, cand, bests, points_being_sampled=pend[:p])  # workspaces
for _ in range(repeat):
    for p in (0, PEND):
        t0 = time.perf_counter()
        api.ei_analytic_ensemble(ens, cand, bests, points_being_sampled=pend[:p])
        t[p].append(1e3 * (time.perf_counter() - t0))
say("1024 candidates with gradient, %d members: p = 0 %s ms, p = %d %s ms (med/min), ratio %.2fx" % (
    E, med_min(t[0]), PEND, med_min(t[PEND]), np.median(t[PEND]) / np.median(t[0])))
for g in ens.gps:
    g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a" if G else "w") as f:
        f.write("\n".join(lines) + "\n")
