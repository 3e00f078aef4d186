"""Leave-one-out objective against the log marginal likelihood on the same handle: the value for 64 hyper-parameter sets in one
call and the gradient at one set, N = 1000 and N = 8000, d = 8 -- and the share of the LOO gradient's time that the M = B^T B
product (2 N^3 flop) would take at the FP64 matrix peak.   python tools/loo_time.py [peak TFLOP/s, default 78.6]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cornell_moe_amd import _lib, api  # noqa: E402

peak = float(sys.argv[1]) if len(sys.argv) > 1 else 78.6
for n, d, reps in ((1000, 8, 3), (8000, 8, 1)):
    rng = np.random.default_rng(3)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.normal(size=n)
    LL = api.LogLikelihood(X, y)
    th = np.r_[1.0, np.full(d, 0.7), 0.05]
    sets = np.array([th * (1.0 + 0.002 * i) for i in range(64)])
    row = {}
    for name, objective in (("marginal", _lib.LL_LOG_MARGINAL), ("loo", _lib.LL_LEAVE_ONE_OUT)):
        LL.set_objective(objective)
        for label, fn in (("value x64", lambda: LL.evaluate(sets)), ("grad", lambda: LL.grad(th))):
            v0 = fn()   # (buffers, first launches)
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            row[name, label] = (time.perf_counter() - t0) / reps
            print("N=%d d=%d  %-8s %-9s %9.2f ms per call   first: %s" % (n, d, name, label, 1e3 * row[name, label],
                                                                         np.array2string(np.ravel(v0)[:2], precision=10)), flush=True)
    m_ms = 2.0 * n ** 3 / (peak * 1e12) * 1e3
    print("N=%d  LOO / marginal: value x64 %.2fx, grad %.2fx;  M = B^T B at %.1f TFLOP/s: %.3f ms = %.1f %% of the LOO gradient"
          % (n, row["loo", "value x64"] / row["marginal", "value x64"], row["loo", "grad"] / row["marginal", "grad"], peak, m_ms,
             100.0 * m_ms / (1e3 * row["loo", "grad"])), flush=True)
