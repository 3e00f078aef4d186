#!/usr/bin/env python3
"""Fixtures of tests/test_gpu_kg_lookup_order.py: what the LDS-table wave-per-sample q-KG kernels returned BEFORE their tile loops were
reordered (exp-table lookups first).  The reordering changes no floating-point operation, so the test holds every later
build to these numbers bit for bit.

    MOE_LIB_PATH=<libmoe_hip.so of the commit before the reordering> python tools/record_kg_lookup_order.py [out_dir]

writes one float64 vector per case to tests/golden/kg_lookup_order/<case>.npy (layout: the test's `pack`).  Run on the GPU; inputs are
seeded (cornell_moe_amd.workloads.make_workload).  The cases, the call and the layout are the TEST's (CASES / run_case / pack, loaded
from its file), so that the recorder cannot drift from what the test runs."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kg_lookup_order")


def _test_module():
    spec = importlib.util.spec_from_file_location("test_gpu_kg_lookup_order", os.path.join(ROOT, "tests", "test_gpu_kg_lookup_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path.insert(0, ROOT)
    from cornell_moe_amd import _lib, api
    T = _test_module()
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    os.makedirs(out, exist_ok=True)
    print("library:", _lib.LIB_PATH)
    for name in T.CASES:
        res, info = T.run_case(api, name)
        v = T.pack(res, info)
        assert np.all(np.isfinite(v)) and np.abs(res["grad_sum"]).max() > 0
        np.save(os.path.join(out, name + ".npy"), v)
        print("%-18s kg_sum %.17g  passes %d / %d  %s  (%d doubles)" % (name, res["kg_sum"], res["mean_evals"], res["grad_evals"],
                                                                       {k: info[k] for k in T.INFO_KEYS + ("blocks",)}, v.size), flush=True)


if __name__ == "__main__":
    main()
