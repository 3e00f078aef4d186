"""Time one suggestion by the ensemble-averaged constrained expected hypervolume improvement: api.ehvi_constrained_multistart
(moe_ehvi_constrained_mcmc_multistart: the evaluation, the strip sums, the feasibility factors, the product rule, the step and the
rounds on the device, ensemble-wide launches; csrc/cehvi1.hip) against the host-driven loop -- tests/ms_restatement.py's optimiser
with every evaluation one api.ehvi_constrained_ensemble call -- on the same starts, and beside it the unconstrained suggestion on the
objective GPs alone (api.ehvi_multistart) with the same settings: every sub-member runs the same chain, so the expectation is the
ratio of the sub-member counts, (M + K) / M.  16 members, M = 2, K = 2, n = 500, d = 6, 200 Latin-hypercube starts of which 20 are
kept, 2 rounds of 50 steps, a front of 32 points.
   python tools/ehvi_constrained_time.py [--out profiles/ehvi_constrained_time.txt] [--repeat 9]

All on one build, alternated in one process, median of --repeat whole calls (host clock around calls that end in a device
synchronise).  Then the same suggestion with three objectives (M = 3, K = 2), a greedy batch of q = 4 in one call
(api.ehvi_constrained_suggest) against four calls of the ascent each fed its predecessors (the same bits, asserted), and what
moe_ensemble_launch_stats counts for one suggestion.  The one-call form must be faster than the host-driven loop of the same run
(asserted); the ratio to the unconstrained suggestion is reported, not bounded."""
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
from cornell_moe_amd import expected_hypervolume_improvement as ehvi  # noqa: E402
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


E, N, D, STARTS, STEPS, ROUNDS, Q, F, K = 16, 500, 6, 200, 50, 2, 4, 32, 2
repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 9
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


def med_min(t):
    return "%9.1f / %8.1f" % (np.median(t), min(t))


def stats():
    out = (C.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return np.array(list(out), dtype=np.int64)


def staircase(count, ref):
    """count mutually non-dominated points on a convex curve through the observed outcomes' range, strictly inside ref"""
    t = (np.arange(count) + 0.5) / count
    return np.ascontiguousarray(np.stack([ref[0] - 4.0 * (1.0 - t) ** 2 - 0.5, ref[1] - 4.0 * t ** 2 - 0.5], axis=1))


def host_loop(objs, cons, tau, ref, front, bounds, starts):
    ev = lambda x, g: api.ehvi_constrained_ensemble(objs, cons, tau, ref, front, np.asarray(x).reshape(-1, D), want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


def host_calls(objs, cons, tau, ref, front, bounds, starts):
    points, values = [], []
    for _ in range(Q):
        res = api.ehvi_constrained_multistart(objs, cons, tau, ref, front, gd, bounds, starts,
                                              points_being_sampled=np.array(points) if points else None)
        points.append(res["point"])
        values.append(res["value"])
    return np.array(points), np.array(values)


clocks("before")
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
y1 = np.sin(3 * X).sum(1, keepdims=True)
y2 = np.cos(2.5 * X + 0.7).sum(1, keepdims=True)
y3 = np.sin(2 * X + 1.3).sum(1, keepdims=True)
c1 = ((X - 0.5) ** 2).sum(1, keepdims=True)        # inside a ball about the centre ...
c2 = np.sin(4 * X[:, :2]).sum(1, keepdims=True)    # ... and on one side of a wave
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
gp = lambda length, y: api.DeviceGPMCMC(np.array([1.0] + [length] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)  # noqa: E731
one, two, three = gp(0.4, y1), gp(0.5, y2), gp(0.45, y3)
cons = [gp(0.5, c1), gp(0.4, c2)]
tau = [float(np.median(c1)), float(np.median(c2))]
ref = (float(y1.max()) + 0.5, float(y2.max()) + 0.5)
ref3 = ref + (float(y3.max()) + 0.5,)
front = staircase(F, ref)
feasible = (c1[:, 0] <= tau[0]) & (c2[:, 0] <= tau[1])
front3 = ehvi.pareto_front_3(np.hstack([y1, y2, y3])[feasible], ref3)[:F]
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
say("%d members (%d GPs: M = 2, K = %d), n = %d, d = %d, %d starts -> 20 kept, %d x %d steps, a front of %d points; whole calls, "
    "median / min of %d, alternated" % (E, (2 + K) * E, K, N, D, STARTS, ROUNDS, STEPS, F, repeat))
call = lambda: api.ehvi_constrained_multistart([one, two], cons, tau, ref, front, gd, bounds, starts)  # noqa: E731
loop = lambda: host_loop([one, two], cons, tau, ref, front, bounds, starts)  # noqa: E731
free = lambda: api.ehvi_multistart(one, two, ref, front, gd, bounds, starts)  # noqa: E731
new_res, loop_res, free_res = call(), loop(), free()  # workspaces
s0 = stats()
call()
ds = stats() - s0
say("moe_ensemble_launch_stats for one suggestion: %d evaluations issued zipped, %d member by member; %d launches issued for %d "
    "recorded (x%.1f fewer)" % (ds[0], ds[1], ds[2], ds[3], ds[3] / max(ds[2], 1)))
t_one, t_loop, t_free = [], [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    loop()
    t2 = time.perf_counter()
    free()
    t3 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_loop.append(1e3 * (t2 - t1))
    t_free.append(1e3 * (t3 - t2))
say("moe_ehvi_constrained_mcmc_multistart %s ms | host loop over moe_ehvi_constrained_mcmc %s ms (med/min) | ratio %.2fx" % (
    med_min(t_one), med_min(t_loop), np.median(t_loop) / np.median(t_one)))
say("moe_ehvi_mcmc_multistart on the objective GPs alone, the same settings %s ms (med/min) | constrained / unconstrained %.2fx "
    "(sub-member count: %.2fx)" % (med_min(t_free), np.median(t_one) / np.median(t_free), (2 + K) / 2.0))
say("  constrained EHVI %.12g at %s (one call)" % (new_res["value"], np.round(new_res["point"], 6).tolist()))
say("  constrained EHVI %.12g at %s (host loop); the same point: %s" % (loop_res[1], np.round(loop_res[0], 6).tolist(),
                                                                        bool(np.array_equal(loop_res[0], new_res["point"]))))
say("  EHVI %.12g at %s" % (free_res["value"], np.round(free_res["point"], 6).tolist()))
faster = np.median(t_one) < np.median(t_loop)

call3 = lambda: api.ehvi_constrained_multistart([one, two, three], cons, tau, ref3, front3, gd, bounds, starts)  # noqa: E731
res3 = call3()  # workspaces
t2o, t3o = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    call3()
    t2 = time.perf_counter()
    t2o.append(1e3 * (t1 - t0))
    t3o.append(1e3 * (t2 - t1))
say("one suggestion, %d members, K = %d: M = 2 %s ms, M = 3 (a front of %d points) %s ms (med/min), ratio %.2fx (sub-member count: "
    "%.2fx)" % (E, K, med_min(t2o), len(front3), med_min(t3o), np.median(t3o) / np.median(t2o), (3 + K) / (2.0 + K)))
say("  M = 3: constrained EHVI %.12g at %s" % (res3["value"], np.round(res3["point"], 6).tolist()))

batch = lambda: api.ehvi_constrained_suggest([one, two], cons, tau, ref, front, gd, bounds, starts, Q)  # noqa: E731
res = batch()
points, values = host_calls([one, two], cons, tau, ref, front, bounds, starts)
assert np.array_equal(res["points"], points) and np.array_equal(res["values"], values)
t_one, t_host = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    batch()
    t1 = time.perf_counter()
    host_calls([one, two], cons, tau, ref, front, bounds, starts)
    t2 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_host.append(1e3 * (t2 - t1))
say("greedy q = %d: one call %s ms | %d calls %s ms (med/min) | ratio %.2fx" % (Q, med_min(t_one), Q, med_min(t_host),
                                                                               np.median(t_host) / np.median(t_one)))
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in values)))
for m in [one, two, three] + cons:
    for g in m.gps:
        g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
assert faster, "the one-call suggestion is not faster than the host-driven loop of the same run"
