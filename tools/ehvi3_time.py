"""Time one suggestion by the ensemble-averaged three-objective expected hypervolume improvement: api.ehvi3_multistart
(moe_ehvi3_mcmc_multistart: the evaluation, the box sums, the step and the rounds on the device, ensemble-wide launches;
csrc/ehvi3.hip) against the host-driven loop -- tests/ms_restatement.py's optimiser with every evaluation one api.ehvi3_ensemble
call -- on the same starts; no other path to this objective exists.  The two-objective suggestion on objectives 1 and 2
(api.ehvi_multistart) with the same settings stands beside it: a member runs three chains in the place of two, and the box kernel
in the place of the strip kernel.  16 members (48 GPs), n = 500, d = 6, 200 Latin-hypercube starts of which 20 are kept, 2 rounds
of 50 steps, a front of 32 points.
   python tools/ehvi3_time.py [--out profiles/ehvi3_time.txt] [--repeat 9]

All on one build, alternated in one process, median of --repeat whole calls (host clock around calls that end in a device
synchronise).  Then the same suggestion with a staircase front of 192 points (18 721 boxes per member), a greedy batch of q = 4 in
one call (api.ehvi3_suggest) against four calls of the ascent each fed its predecessors (the same bits, asserted), the table
kernel's share of a greedy round -- the value at ONE point with the staircase of 192 against the same call with an empty front,
which differ by the front kernel, the table kernel and one candidate's box sums per member -- and what moe_ensemble_launch_stats
counts for one suggestion.  No threshold is set; a ratio near or under 1 is a finding, not a failure."""
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


E, N, D, STARTS, STEPS, ROUNDS, Q, F, FMAX = 16, 500, 6, 200, 50, 2, 4, 32, 192
repeat = int(sys.argv[sys.argv.index("--repeat") + 1]) if "--repeat" in sys.argv else 9
gd = (STARTS, STEPS, ROUNDS, 0, 0.7, 1.0, 0.5, 1e-10)  # the outer parameters of examples/main.py


def med_min(t):
    return "%9.1f / %8.1f" % (np.median(t), min(t))


def stats():
    out = (C.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return np.array(list(out), dtype=np.int64)


def staircase(count, ref):
    """count mutually non-dominated points, u ascending, v descending, w ascending (every slab keeps all its points: (count + 1)
    (count + 2) / 2 boxes), through the observed outcomes' range, strictly inside ref"""
    t = (np.arange(count) + 0.5) / count
    return np.ascontiguousarray(np.stack([ref[0] - 4.0 * (1.0 - t) ** 2 - 0.5, ref[1] - 4.0 * t ** 2 - 0.5, ref[2] - 4.5 + 4.0 * t],
                                         axis=1))


def host_loop(gps, ref, front, bounds, starts):
    ev = lambda x, g: api.ehvi3_ensemble(gps[0], gps[1], gps[2], ref, front, np.asarray(x).reshape(-1, D), want_grad=g)  # noqa: E731
    vals = ev(starts, False)
    order = ms.top_k_order(vals)
    ends = ms.gradient_ascent(lambda x: ev(x, True)[1].reshape(np.shape(x)), gd, bounds, starts[order])
    end_vals = ev(ends, False)
    w = int(np.argmax(end_vals))
    return ends[w], float(end_vals[w])


def host_calls(gps, ref, front, bounds, starts):
    points, values = [], []
    for _ in range(Q):
        res = api.ehvi3_multistart(gps[0], gps[1], gps[2], ref, front, gd, bounds, starts,
                                   points_being_sampled=np.array(points) if points else None)
        points.append(res["point"])
        values.append(res["value"])
    return np.array(points), np.array(values)


clocks("before")
rng = np.random.default_rng(0)
X = rng.uniform(size=(N, D))
ys = [np.sin(3 * X).sum(1, keepdims=True), np.cos(2.5 * X + 0.7).sum(1, keepdims=True), np.sin(2 * X + 1.9).sum(1, keepdims=True)]
spread = lambda: np.exp(0.15 * rng.standard_normal((E, D + 1)))  # noqa: E731  (the spread of a hyper-parameter chain)
gps = [api.DeviceGPMCMC(np.array([1.0] + [length] * D)[None, :] * spread(), np.full((E, 1), 1e-2), X, y)
       for length, y in zip((0.4, 0.5, 0.45), ys)]
ref = tuple(float(y.max()) + 0.5 for y in ys)
front, front_max = staircase(F, ref), staircase(FMAX, ref)
bounds = np.array([[0.0, 1.0]] * D)
starts = api.latin_hypercube(5, bounds, STARTS)
say("%d members (%d GPs), n = %d, d = %d, %d starts -> 20 kept, %d x %d steps, a front of %d points (%d boxes); whole calls, median / "
    "min of %d, alternated" % (E, 3 * E, N, D, STARTS, ROUNDS, STEPS, F, (F + 1) * (F + 2) // 2, repeat))
call = lambda: api.ehvi3_multistart(gps[0], gps[1], gps[2], ref, front, gd, bounds, starts)  # noqa: E731
loop = lambda: host_loop(gps, ref, front, bounds, starts)  # noqa: E731
two = lambda: api.ehvi_multistart(gps[0], gps[1], ref[:2], front[:, :2], gd, bounds, starts)  # noqa: E731
new_res, loop_res, two_res = call(), loop(), two()  # workspaces
s0 = stats()
call()
ds = stats() - s0
say("moe_ensemble_launch_stats for one suggestion: %d evaluations issued zipped, %d member by member; %d launches issued for %d "
    "recorded (x%.1f fewer)" % (ds[0], ds[1], ds[2], ds[3], ds[3] / max(ds[2], 1)))
t_one, t_loop, t_two = [], [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    loop()
    t2 = time.perf_counter()
    two()
    t3 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_loop.append(1e3 * (t2 - t1))
    t_two.append(1e3 * (t3 - t2))
say("moe_ehvi3_mcmc_multistart %s ms | host loop over moe_ehvi3_mcmc %s ms (med/min) | ratio %.2fx" % (
    med_min(t_one), med_min(t_loop), np.median(t_loop) / np.median(t_one)))
say("moe_ehvi_mcmc_multistart on objectives 1 and 2, the same settings %s ms (med/min) | three objectives / two %.2fx (three chains "
    "and the box kernel against two and the strip kernel)" % (med_min(t_two), np.median(t_one) / np.median(t_two)))
say("  EHVI3 %.12g at %s (one call)" % (new_res["value"], np.round(new_res["point"], 6).tolist()))
say("  EHVI3 %.12g at %s (host loop); the same point: %s" % (loop_res[1], np.round(loop_res[0], 6).tolist(),
                                                             bool(np.array_equal(loop_res[0], new_res["point"]))))
say("  EHVI2 %.12g at %s" % (two_res["value"], np.round(two_res["point"], 6).tolist()))

runs = {F: call, FMAX: lambda: api.ehvi3_multistart(gps[0], gps[1], gps[2], ref, front_max, gd, bounds, starts)}  # noqa: E731
t = {F: [], FMAX: []}
runs[FMAX]()  # workspaces
for _ in range(repeat):
    for k in runs:
        t0 = time.perf_counter()
        runs[k]()
        t[k].append(1e3 * (time.perf_counter() - t0))
say("one suggestion, %d members: F = %d %s ms, staircase F = %d (%d boxes) %s ms (med/min), ratio %.2fx" % (
    E, F, med_min(t[F]), FMAX, (FMAX + 1) * (FMAX + 2) // 2, med_min(t[FMAX]), np.median(t[FMAX]) / np.median(t[F])))

batch = lambda: api.ehvi3_suggest(gps[0], gps[1], gps[2], ref, front, gd, bounds, starts, Q)  # noqa: E731
res = batch()
points, values = host_calls(gps, ref, front, bounds, starts)
assert np.array_equal(res["points"], points) and np.array_equal(res["values"], values)
t_one, t_host = [], []
for _ in range(repeat):
    t0 = time.perf_counter()
    batch()
    t1 = time.perf_counter()
    host_calls(gps, ref, front, bounds, starts)
    t2 = time.perf_counter()
    t_one.append(1e3 * (t1 - t0))
    t_host.append(1e3 * (t2 - t1))
say("greedy q = %d: one call %s ms | %d calls %s ms (med/min) | ratio %.2fx" % (Q, med_min(t_one), Q, med_min(t_host),
                                                                               np.median(t_host) / np.median(t_one)))
say("  values of the %d picks: %s" % (Q, " ".join("%.6g" % v for v in values)))
round_ms = float(np.median(t_one)) / Q

one_point = starts[:1]
probe = {n: (lambda f: (lambda: api.ehvi3_ensemble(gps[0], gps[1], gps[2], ref, f, one_point, want_grad=False)))(f)  # noqa: E731
         for n, f in ((0, None), (F, front), (FMAX, front_max))}
tp = {n: [] for n in probe}
for n in probe:
    probe[n]()
for _ in range(4 * repeat):
    for n in probe:
        t0 = time.perf_counter()
        probe[n]()
        tp[n].append(1e3 * (time.perf_counter() - t0))
say("the value at one point, %d members: empty front %s ms, F = %d %s ms, staircase F = %d %s ms (med/min)" % (
    E, med_min(tp[0]), F, med_min(tp[F]), FMAX, med_min(tp[FMAX])))
for n in (F, FMAX):
    extra = float(np.median(tp[n]) - np.median(tp[0]))
    say("  front, table and one candidate's boxes at F = %d: %.3f ms over the empty front's call, %.2f %% of a greedy round of %.1f ms "
        "(the table is built once per round)" % (n, extra, 100.0 * extra / round_ms, round_ms))
for m in gps:
    for g in m.gps:
        g.close()
clocks("after")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
