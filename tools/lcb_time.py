"""Time batch lower-confidence-bound selection: ms per whole call of DeviceGP.lcb_select at n = 500, d = 6 for C candidates and a
batch of q, beside the same selection driven through the older entry points the way the reference's Python drives it (one
cholesky_variance call per candidate and round, add_points of a zero-valued observation on a scratch copy of the GP per round).
   python tools/lcb_time.py [--out profiles/lcb_time.txt] [--no-baseline]

The baseline loop uses nothing this selection added, so it runs unchanged on older builds.  The device's clocks (rocm-smi, read
only) and its sustained FP64 rate are recorded before and after."""
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
n, d, noise = 500, 6, 1e-2
hyper = [1.0] + [0.15] * d
X = rng.uniform(size=(n, d))
y = np.sin(3 * X).sum(1, keepdims=True)
gp = api.DeviceGP(hyper, X, y, [noise])


def reference_style(cand, q):
    """lower_confidence_bound.py's loop over the older entry points, on a scratch GP"""
    scratch = api.DeviceGP(hyper, X, y, [noise])
    mean = scratch.mean(cand)
    std = np.array([scratch.cholesky_variance(cand[i:i + 1])[0] for i in range(len(cand))])
    target, ucb = mean - std, mean + std
    index = [int(np.argmin(target))]
    kept = np.flatnonzero(target <= ucb.min())
    for _ in range(1, q):
        scratch.add_points(cand[index[-1]:index[-1] + 1], np.zeros((1, 1)))
        cstd = np.array([scratch.cholesky_variance(cand[i:i + 1])[0] for i in kept])
        index.append(int(kept[int(np.argmax(cstd))]))
    scratch.close()
    return np.array(index), len(kept)


baseline = "--no-baseline" not in sys.argv
say("GP: n = %d, d = %d, noise %g; whole-call times, host clock around calls that end in a device synchronise" % (n, d, noise))
clocks("before")
say("%7s %3s %6s | %22s | %18s | %s" % ("C", "q", "kept", "lcb_select ms (med/min)", "reference-style ms", "same picks"))
for C in (1024, 16384):
    cand = rng.uniform(size=(C, d))
    for q in (1, 4, 16):
        index, _, kept = gp.lcb_select(cand, q)  # workspaces
        ts = []
        for _ in range(9):
            t0 = time.perf_counter()
            gp.lcb_select(cand, q)
            ts.append(time.perf_counter() - t0)
        if baseline:
            t0 = time.perf_counter()
            ref_index, ref_kept = reference_style(cand, q)
            base = "%18.1f" % (1e3 * (time.perf_counter() - t0))
            same = "yes" if np.array_equal(ref_index, index) and ref_kept == kept else "NO %s / %s" % (ref_index, index)
        else:
            base, same = "%18s" % "not run", "-"
        say("%7d %3d %6d | %12.3f / %7.3f | %s | %s" % (C, q, kept, 1e3 * np.median(ts), 1e3 * min(ts), base, same))
clocks("after")
gp.close()
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
