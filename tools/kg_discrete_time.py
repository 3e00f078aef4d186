"""Time the exact discretised one-point knowledge gradient: ms per whole call of DeviceGP.kg_discrete at n = 500, d = 6 for
C = 1024 candidates and a discrete set of A in {128, 1010, 4095} points, with and without the gradient, beside the Monte-Carlo
evaluator (DeviceGP.kg_batch, q = 1, 2^7 samples, the inner line search of a suggestion) on the same candidates and the same set.
   python tools/kg_discrete_time.py [--out profiles/kg_discrete_time.txt] [--no-mc]

The two compute different quantities -- the exact value is a lower bound of what the Monte-Carlo evaluator estimates -- so the
figures are costs per candidate, not a race.  The Monte-Carlo evaluator takes the candidates in calls of 128 evaluations; a refusal
(its own size limits) is printed instead of a time.  The device's clocks (rocm-smi, read only) and its sustained FP64 rate are
recorded before and after."""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
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


rng = np.random.default_rng(0)
n, d, noise, C, M = 500, 6, 1e-2, 1024, 128
hyper = [1.0] + [0.4] * d
X = rng.uniform(size=(n, d))
y = np.sin(3 * X).sum(1, keepdims=True)
gp = api.DeviceGP(hyper, X, y, [noise])
cand = rng.uniform(size=(C, d))
best = float(y.min())
bounds = np.array([[0.0, 1.0]] * d)
inner = (1, 20, 1, 4, 0.7, 1.0, 0.1, 1e-9)  # the inner line search of a suggestion
normals = rng.standard_normal((M // 2, 1))


def timed(fn, repeat):
    fn()  # workspaces
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * min(ts)


def monte_carlo(disc):
    for lo in range(0, C, 128):
        gp.kg_batch(inner, bounds, disc, cand[lo:lo + 128].reshape(-1, 1, d), None, M, best, normals, want_grad=True)


say("GP: n = %d, d = %d, noise %g; C = %d candidates; whole-call times, host clock around calls that end in a device synchronise" % (
    n, d, noise, C))
clocks("before")
say("%5s | %13s | %24s | %24s | %s" % ("A", "lines on env.", "value ms (med/min)", "value + gradient ms", "kg_batch q=1 M=128, value + gradient ms"))
for A in (128, 1010, 4095):
    disc = rng.uniform(size=(A, d))
    active = gp.kg_discrete(disc, cand, best, want_grad=False, want_active=True)[1]
    v = timed(lambda: gp.kg_discrete(disc, cand, best, want_grad=False), 9)
    g = timed(lambda: gp.kg_discrete(disc, cand, best, want_grad=True), 9)
    if "--no-mc" in sys.argv:
        mc = "not run"
    else:
        try:
            mc = "%.1f / %.1f" % timed(lambda: monte_carlo(disc), 2)
        except api.OptimalLearningException as e:
            mc = "refused: %s" % e
    say("%5d | %4d .. %-5d | %13.3f / %8.3f | %13.3f / %8.3f | %s" % (A, active.min(), active.max(), v[0], v[1], g[0], g[1], mc))
clocks("after")
gp.close()
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
