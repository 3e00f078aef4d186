"""Time moe_gp_add_points: the rank-k block-row append vs a GP built from scratch on the same points, at a few sizes.
   python tools/add_points_time.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cornell_moe_amd import api  # noqa: E402

rng = np.random.default_rng(0)
for n, d, k, derivs in ((1000, 8, 4, ()), (4000, 8, 4, ()), (8000, 8, 4, ()), (2000, 12, 4, (0, 1, 2))):
    X = rng.uniform(size=(n + 10 * k, d))
    y = np.sin(3 * X).sum(1, keepdims=True)
    if derivs:
        y = np.hstack([y] + [3 * np.cos(3 * X[:, [j]]) for j in derivs])
    gp = api.DeviceGP([1.0] + [0.7] * d, X[:n], y[:n], [0.01] * (1 + len(derivs)), derivatives=derivs)
    at = n
    ts, tb = [], []
    for r in range(10):
        t0 = time.perf_counter()
        gp.add_points(X[at:at + k], y[at:at + k])
        ts.append(time.perf_counter() - t0)
        at += k
        t0 = time.perf_counter()
        api.DeviceGP([1.0] + [0.7] * d, X[:at], y[:at], [0.01] * (1 + len(derivs)), derivatives=derivs)
        tb.append(time.perf_counter() - t0)
    print("n=%5d g=%d N=%6d  add %d points: median %.3f ms (first %.3f); built from scratch: median %.3f ms" % (
        n, len(derivs), n * (1 + len(derivs)), k, 1e3 * np.median(ts[1:]), 1e3 * ts[0], 1e3 * np.median(tb[1:])))
