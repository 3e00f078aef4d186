"""What the static workgroup-to-evaluation assignment of the q-KG MC kernel costs at the headline batch (C3: 64 restarts per call).

    python tools/mc_balance.py [restarts = 64] [repeats = 10] [warm-ups = 3]

A workgroup serves one evaluation for its lifetime, so the MC kernel ends with its COSTLIEST evaluation and the workgroups of the
cheaper ones idle until then.  This tool measures how much that is: every restart's cost from a call of its own (its pass
counters, weighted as bench.py's pass_flops weights them), then the MC kernel's device time (last_kernel_ms()["mc"]: HIP events
on the library's stream) of (a) the mixed batch that bench.py runs, (b) the cheapest restart R times, (c) the costliest R times.
(b) and (c) are balanced batches: every evaluation of the call costs the same, so they give time as a function of cost without
any between-evaluation spread.  The line through them, read at the batch's MEAN cost, is what (a) would take with perfect
balance; (a) minus that is the loss that moving idle workgroups to running evaluations can recover at most.
MOE_KG_STEAL and the other switches are read by the library per call: set them in the environment to measure a variant."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from cornell_moe_amd.api import DeviceGP  # noqa: E402
from cornell_moe_amd.workloads import make_workload  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 64
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARMUPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3

w = make_workload("C3", num_restarts=R)
G = DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs)
best = float(G.additional_mean(w.discrete).min())
_, f_val, f_grad = bench.pass_flops(w)


def call(Xq):
    return G.kg_batch(w.inner_gd, w.bounds, w.discrete, Xq, None, w.M, best, w.kg_normals)


# ---- every restart alone: its passes per sample and its weighted cost ----
val = np.zeros(R)
grad = np.zeros(R)
for i in range(R):
    r = call(w.Xq_restarts[i:i + 1])
    val[i], grad[i] = r["mean_evals"] / w.M, r["grad_evals"] / w.M
cost = f_val * val + f_grad * grad
order = np.argsort(cost)
lo, hi = int(order[0]), int(order[-1])
print("library: %s" % os.environ.get("MOE_LIB_PATH", "in tree"))
print("switches: %s" % {k: v for k, v in sorted(os.environ.items()) if k.startswith("MOE_KG_")})
print("%d restarts, M = %d; passes per sample: value %.3f .. %.3f (mean %.3f), gradient %.3f .. %.3f (mean %.3f)"
      % (R, w.M, val.min(), val.max(), val.mean(), grad.min(), grad.max(), grad.mean()))
print("weighted cost (value pass %d, gradient pass %d flops per point) relative to the mean: cheapest %.4f (restart %d), "
      "costliest %.4f (restart %d), standard deviation %.4f" % (f_val, f_grad, cost[lo] / cost.mean(), lo, cost[hi] / cost.mean(), hi,
                                                                 cost.std() / cost.mean()))
print("ranking, cheapest first: %s" % " ".join("%d:%.4f" % (i, cost[i] / cost.mean()) for i in order))


def timed(name, Xq):
    for _ in range(WARMUPS):
        call(Xq)
    ms = np.zeros(REPEATS)
    for k in range(REPEATS):
        call(Xq)
        ms[k] = G.last_kernel_ms()["mc"]
    info = G.last_kernel_info()
    print("%-28s mc ms per evaluation: mean %.4f  min %.4f  max %.4f  range %.4f   [%s]  (variant %d, lane %d, %d workgroups x %d waves)"
          % (name, ms.mean(), ms.min(), ms.max(), ms.max() - ms.min(), " ".join("%.3f" % v for v in ms), info["variant"], info["lane"],
             info["blocks"], info["waves"]), flush=True)
    return ms


# (a) twice, around the balanced batches: a drift of the clock over the session shows as a difference between the two
a1 = timed("(a) mixed batch", w.Xq_restarts)
b = timed("(b) cheapest x %d" % R, np.repeat(w.Xq_restarts[lo:lo + 1], R, axis=0))
c = timed("(c) costliest x %d" % R, np.repeat(w.Xq_restarts[hi:hi + 1], R, axis=0))
a2 = timed("(a) mixed batch, again", w.Xq_restarts)
a = np.concatenate([a1, a2])
slope = (c.mean() - b.mean()) / (cost[hi] - cost[lo])
balanced = b.mean() + slope * (cost.mean() - cost[lo])
worst = b.mean() + slope * (cost[hi] - cost[lo])
loss = a.mean() - balanced
rng = max(v.max() - v.min() for v in (a1, a2, b, c))
print("time at the mean cost, on the line through (b) and (c): %.4f ms; at the costliest restart's: %.4f ms" % (balanced, worst))
print("(a) %.4f ms (first block %.4f, second %.4f) -> loss to recover: %.4f ms = %.2f %% of (a); largest range of the repeats %.4f ms; "
      "loss / range = %.2f (%s three times the range)" % (a.mean(), a1.mean(), a2.mean(), loss, 100.0 * loss / a.mean(), rng,
                                                         loss / rng if rng > 0 else float("inf"),
                                                         "at least" if loss >= 3.0 * rng else "BELOW"))
