"""Time a greedy batch of q = 4 points by the ensemble-averaged discretised knowledge gradient with pending points:
api.kg_discrete_suggest (moe_kg_discrete_mcmc_suggest: one upload, the set phase once, one appended row per round;
csrc/kg1_pending.hip) against q host calls of api.kg_discrete_multistart (moe_kg_discrete_mcmc_multistart_pending), each fed the
points of the calls before it.  16 members, 200 Latin-hypercube starts of which 20 are kept, 2 rounds of 50 steps, discrete sets of
A = 11 and A = 1010 points, on the two GPs of tools/kg_discrete_suggest_time.py (Branin n = 20, d = 2; n = 500, d = 6).
   python tools/kg_discrete_batch_time.py [--out profiles/kg_discrete_batch_time.txt] [--no-mc] [--repeat 9]

Both run on the same build, alternated, median of --repeat whole batches (host clock around calls that end in a device
synchronise); they return the same bits, which is asserted.  What the one call saves is structural: the set phase paid once
instead of q times and q - 1 uploads; a ratio near 1 is a finding, not a failure.  As a cost column, not a race:
DeviceGPMCMC.kg_multistart (moe_kg_mcmc_multistart, the Monte-Carlo knowledge gradient) at q = 4 with 2^7 samples from the same
starts.  Last, one evaluation of 1024 candidates with p = 8 pending points against p = 0 (what the extension's rows cost)."""
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


def branin(x):
    a, b = 15.0 * x[..., 0] - 5.0, 15.0 * x[..., 1]
    return (b - 5.1 / (4 * np.pi ** 2) * a ** 2 + 5.0 / np.pi * a - 6.0) ** 2 + 10.0 * (1 - 1 / (8 * np.pi)) * np.cos(a) + 10.0


E, STARTS, STEPS, ROUNDS, M, Q = 16, 200, 50, 2, 128, 4
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


def host_calls(ens, sets, bests, bounds, starts):
    points, values = [], []
    for _ in range(Q):
        res = api.kg_discrete_multistart(ens, gd, bounds, sets, bests, starts, points_being_sampled=np.array(points) if points else None)
        points.append(res["point"])
        values.append(res["value"])
    return np.array(points), np.array(values)


def med_min(t):
    return "%9.1f / %8.1f" % (np.median(t), min(t))


clocks("before")
say("%d members, %d starts -> 20 kept, %d x %d steps, q = %d; whole batches, median / min of %d, alternated" % (E, STARTS, ROUNDS, STEPS,
                                                                                                               Q, repeat))
say("%-7s %5s | %21s | %21s | %7s | %s" % ("GP", "A", "one call ms (med/min)", "q calls ms (med/min)", "ratio",
                                           "moe_kg_mcmc_multistart q=4 M=128 ms"))
for name in ("branin", "n500_d6"):
    rng = np.random.default_rng(0)
    n, d, X, y, hypers, noises = problem(name, rng)
    ens = api.DeviceGPMCMC(hypers, noises, X, y)
    bounds = np.array([[0.0, 1.0]] * d)
    starts = api.latin_hypercube(5, bounds, STARTS)
    bests = [float(y.min())] * E
    for A in (11, 1010):
        sets = [rng.uniform(size=(A, d)) for _ in range(E)]
        one = lambda: api.kg_discrete_suggest(ens, gd, bounds, sets, bests, starts, Q)  # noqa: E731
        res = one()  # workspaces
        points, values = host_calls(ens, sets, bests, bounds, starts)
        assert np.array_equal(res["points"], points) and np.array_equal(res["values"], values)
        t_one, t_host = [], []
        for _ in range(repeat):
            t0 = time.perf_counter()
            one()
            t1 = time.perf_counter()
            host_calls(ens, sets, bests, bounds, starts)
            t2 = time.perf_counter()
            t_one.append(1e3 * (t1 - t0))
            t_host.append(1e3 * (t2 - t1))
        mc = "not run"
        if "--no-mc" not in sys.argv:
            normals = np.random.default_rng(1).standard_normal((M // 2, Q))
            mc_starts = np.stack([np.roll(starts, -k, axis=0) for k in range(Q)], axis=1)  # [STARTS][Q][d]
            try:
                t0 = time.perf_counter()
                ens.kg_multistart(gd, inner, bounds, np.array(sets), mc_starts, None, M, bests, normals)
                mc = "%.0f" % (1e3 * (time.perf_counter() - t0))
            except api.OptimalLearningException as e:
                mc = "refused: %s" % e
        say("%-7s %5d | %s | %s | %6.2fx | %s" % (name, A, med_min(t_one), med_min(t_host), np.median(t_host) / np.median(t_one), mc))
        say("        KG of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in values)))
    if name == "n500_d6":  # one evaluation of 1024 candidates, p = 8 against p = 0
        cand = np.random.default_rng(2).uniform(size=(1024, d))
        pend = np.random.default_rng(3).uniform(size=(8, d))
        for A in (11, 1010):
            sets = [rng.uniform(size=(A, d)) for _ in range(E)]
            t = {0: [], 8: []}
            for p in (0, 8):
                api.kg_discrete_ensemble(ens, sets, cand, bests, points_being_sampled=pend[:p])  # workspaces
            for _ in range(repeat):
                for p in (0, 8):
                    t0 = time.perf_counter()
                    api.kg_discrete_ensemble(ens, sets, cand, bests, points_being_sampled=pend[:p])
                    t[p].append(1e3 * (time.perf_counter() - t0))
            say("n500_d6 %5d | 1024 candidates with gradient, %d members: p = 0 %s ms, p = 8 %s ms (med/min), ratio %.2fx" % (
                A, E, med_min(t[0]), med_min(t[8]), np.median(t[8]) / np.median(t[0])))
    for g in ens.gps:
        g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
