"""Time joint posterior sampling: ms per call for C candidates, E candidate sets and D draws per set.
   python tools/sample_time.py

E = 1 goes through moe_gp_sample_points (D draws of one set), E = 16 through moe_gp_sample_global_optima (one draw per set, so
D = 1 only: no entry point draws several times from each of several sets)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cornell_moe_amd import api  # noqa: E402

rng = np.random.default_rng(0)
n, d = 500, 6
X = rng.uniform(size=(n, d))
gp = api.DeviceGP([1.0] + [0.15] * d, X, np.sin(3 * X).sum(1, keepdims=True), [1e-2])
print("GP: n = %d, d = %d" % (n, d))
for C in (256, 1024, 4096):
    for E in (1, 16):
        for D in (1, 64):
            if E > 1 and D > 1:
                print("C=%5d E=%2d D=%2d: no entry point" % (C, E, D))
                continue
            cand = rng.uniform(size=(E, C, d))
            z = rng.normal(size=(E, D, C))
            if E == 1:
                call = lambda: gp.sample_points(cand[0], z[0])  # noqa: E731
            else:
                call = lambda: gp.sample_global_optima(cand, z[:, 0])  # noqa: E731
            call()  # workspaces
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            print("C=%5d E=%2d D=%2d: median %.3f ms  (min %.3f)" % (C, E, D, 1e3 * np.median(ts), 1e3 * min(ts)))
            sys.stdout.flush()
gp.close()
