"""The shapes of tests/test_gpu_ei_edges.py, one table for the device tests and for the CPU test that qualifies them
(tests/test_ei_reference.py: no rounding-sized decision margin, the double-precision oracle within a tenth of TOL of the extended
reference).  Every entry carries the keyword dict `kw` of cornell_moe_amd.workloads.make_workload; beside it
    cov   0 = square exponential, 1 = Matern-5/2
    grad  the want_grad settings the device test runs
    E     evaluations per call (1: moe_ei; more: moe_ei_batch over the E point sets `problem` draws)
    best  "near": the value observed at the training point nearest to the last point of the union, so that best - mu there is of the size
          of the posterior deviation and the samples split into improving and not; "below" / "above": that -/+ 100 (no / every sample improves)
    nm    members of a GP ensemble (`ensemble_members`), 0 for a single GP

What selects a path (csrc/ei.hip, gp.hpp):
    u = q + p        ei_state_kernel<., 4 / 8 / 16>, the host algebra above 16; ei_mc_kernel<16 / 32 / 64>
    c = u + nd d     nd = q with the gradient, 0 without.  state_fits_lds(N, c): c <= 48 and 8 (c^2 + c + N + 2 c N) <= 144 KiB, i.e.
                     c^2 + c + (2 c + 1) N <= 18432 -- then the fused state kernel, otherwise the K-sliced Gram kernels.
                     c = 10: N <= 872;  c = 3: N <= 2631;  c = 2: N <= 3685;  c = 48: N <= 165;  c = 49: never
    N > 1024         inside the fused kernel: the tail loop that stages K^-1 y beyond its four registers per lane
    u dp <= 512      the fused kernel's two registers per lane for the union points (dp: d padded to 4, 8, 12, 16, 24 or 32)
    ncomp = 1 + q d  sum_partials_body: 256 / ncomp' lanes per component, a second round of components above 256
    M                ceil(M / 256) workgroups; sum_partials_body walks them with a stride of at most 256
"""
import numpy as np

SE, MATERN = 0, 1
GROUPS = ("union", "final-sum", "samples", "threshold", "batch", "saturated", "ensemble")


def _case(group, name, cov=MATERN, grad=(True, False), E=1, best="near", nm=0, **kw):
    kw.setdefault("P", 1)
    kw.setdefault("p", 0)
    kw.setdefault("derivs", ())
    return dict(id="%s-%s" % (group, name), group=group, cov=cov, grad=tuple(grad), E=E, best=best, nm=nm, kw=kw)


CASES = []

# ---- a. union classes: u in {1, 4, 5, 8, 9, 16, 17, 32, 33, 64} with mixed splits (p = 0 and q = 1 among them), d in {1, 3}, both
# covariances, with and without the gradient; M = 300: two workgroups, the second with 44 live lanes
_SPLITS = {1: ((1, 0), (1, 0)), 4: ((2, 2), (4, 0)), 5: ((1, 4), (3, 2)), 8: ((8, 0), (5, 3)), 9: ((4, 5), (1, 8)),
           16: ((16, 0), (1, 15)), 17: ((1, 16), (17, 0)), 32: ((20, 12), (32, 0)), 33: ((33, 0), (6, 27)), 64: ((40, 24), (1, 63))}
for _u, _splits in sorted(_SPLITS.items()):
    for _d, (_q, _p) in zip((1, 3), _splits):
        for _cov in (SE, MATERN):
            CASES.append(_case("union", "u%d-q%dp%d-d%d-cov%d" % (_u, _q, _p, _d, _cov), cov=_cov,
                               seed=5000 + 10 * _u + 2 * _d + _cov, n=40 + _u // 4, d=_d, q=_q, p=_p, M=300))

# ---- b. the layout of the final sum, ncomp = 1 + q d.  q d = 127 is prime and neither (1, 127) nor (127, 1) is a legal shape, so 128
# itself cannot be reached: 127 (two lanes per component) and 129 (one) are its neighbours; 64 fills the 256 lanes exactly with four
# lanes per component; 256 / 257: one round / two rounds; 513: three rounds, with p = 0 and u dp = 16 x 32 = 512 the union-point staging
# exactly full -- in the VALUE-ONLY call, whose c = 16 is fused (with the gradient c = 528 takes the K-sliced kernels, which load the union
# points in a loop); 261: two rounds behind the host algebra (u = 20)
for _q, _d, _p in ((7, 9, 1), (7, 18, 0), (8, 16, 0), (15, 17, 1), (16, 16, 0), (16, 32, 0), (20, 13, 0)):
    CASES.append(_case("final-sum", "ncomp%d-q%dd%dp%d" % (1 + _q * _d, _q, _d, _p),
                       seed=5200 + _q * _d, n=48, d=_d, q=_q, p=_p, M=300))

# ---- c. sample counts: one lane; a wavefront short of one lane / full; a workgroup short of one lane / full / one lane into the second;
# one lane into the third.  70 000 samples are 274 workgroups: more than the 256 partial sums one pass of sum_partials_body takes
for _M in (1, 63, 64, 255, 256, 257, 513):
    CASES.append(_case("samples", "M%d-u3" % _M, seed=5300 + _M, n=44, d=2, q=2, p=1, M=_M))
CASES.append(_case("samples", "M70000-u1", seed=5391, n=44, d=2, q=1, p=0, M=70000))
CASES.append(_case("samples", "M70000-u2", grad=(True,), seed=5392, n=44, d=2, q=2, p=0, M=70000))

# ---- d. fused / K-sliced threshold (state_fits_lds above) and the fused kernel beyond 1024 rows
for _n in (872, 873):                                              # c = 2 + 2 x 4 = 10: the last fused size, the first K-sliced one
    CASES.append(_case("threshold", "c10-N%d" % _n, grad=(True,), seed=5400 + _n, n=_n, d=4, q=2, p=0, M=300))
for _p in (0, 1):                                                  # c = 8 + p + 8 x 5 = 48 (fused) / 49 (never fused)
    CASES.append(_case("threshold", "c%d-N150" % (48 + _p), grad=(True,), seed=5410 + _p, n=150, d=5, q=8, p=_p, M=300))
for _n in (1024, 1025, 1281):                                      # c = 2, value only: no tail; one row in the tail; a second trip of the tail
    CASES.append(_case("threshold", "c2-N%d" % _n, grad=(False,), seed=5420 + _n, n=_n, d=2, q=1, p=1, M=300))
CASES.append(_case("threshold", "c3-N1030", grad=(True,), seed=5431, n=1030, d=2, q=1, p=0, M=300))
for _n in (2631, 2632):                                            # c = 1 + 1 x 2 = 3: the last fused size, the first K-sliced one
    CASES.append(_case("threshold", "c3-N%d" % _n, grad=(True,), seed=5440 + _n, n=_n, d=2, q=1, p=0, M=300))

# ---- e. batches: grid.y, blob_stride, one ticket per evaluation
for _E in (2, 65, 300):
    CASES.append(_case("batch", "E%d-u2" % _E, E=_E, seed=5500 + _E, n=40, d=2, q=1, p=1, M=300))
CASES.append(_case("batch", "E5-u20", E=5, seed=5505, n=50, d=3, q=16, p=4, M=300))                 # host algebra
CASES.append(_case("batch", "E7-c10-N873", E=7, grad=(True,), seed=5507, n=873, d=4, q=2, p=0, M=300))  # K-sliced state kernels

# ---- f. saturated decisions
for _q, _p in ((2, 1), (14, 6)):
    for _best in ("below", "above"):
        CASES.append(_case("saturated", "%s-u%d" % (_best, _q + _p), best=_best, seed=5600 + _q, n=45, d=3, q=_q, p=_p, M=300))

# ---- g. an ensemble of GPs above u = 16
CASES.append(_case("ensemble", "nm4-u20-E3", E=3, nm=4, seed=5700, n=45, d=3, q=14, p=6, M=300))

# GPs with observed derivatives (the state kernels' derivative rows; EI points carry none): checked against oracle/orc.py
DERIV_CASES = [
    _case("derivs", "u9", seed=5801, n=40, d=3, q=4, p=5, M=300, derivs=(0, 2)),
    _case("derivs", "u20", seed=5802, n=40, d=3, q=12, p=8, M=300, derivs=(1,)),
]

# Seeds replaced because the first choice failed the qualification of tests/test_ei_reference.py: no sample improved (u1, M63; one entry of
# E7), or the double-precision oracle was further than a tenth of TOL from the extended reference (u17 in one dimension: gradient
# 1.0e-10 of 1e-10; N2631: value 1.1e-11 of 1e-11)
for _id, _seed in (("union-u1-q1p0-d3-cov0", 5018), ("union-u17-q1p16-d1-cov0", 5176), ("samples-M63-u3", 5364), ("threshold-c3-N2631", 8073),
                   ("batch-E7-c10-N873", 5509)):
    [c for c in CASES if c["id"] == _id][0]["kw"]["seed"] = _seed

assert len({c["id"] for c in CASES + DERIV_CASES}) == len(CASES) + len(DERIV_CASES)


def ei_distance(got, want):
    """|got - want| / max(|want|, 1e-3): held to TOL["ei"] by every EI test of the suite"""
    return abs(float(got) - float(want)) / max(abs(float(want)), 1e-3)


def grad_distance(got, want):
    """max |got - want| / max(max |want|, 1e-3): held to TOL["grad_ei"]"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / max(float(np.abs(want).max()), 1e-3)


class Problem(object):
    pass


def problem(case):
    """The workload of a case, the incumbent and the E point sets (the first is the workload's own)."""
    from cornell_moe_amd.workloads import make_workload
    P = Problem()
    P.case, P.cov = case, case["cov"]
    P.w = w = make_workload(**case["kw"])
    P.Xp = w.Xp if w.p else None
    P.normals = w.ei_normals
    last = P.Xp[-1] if w.p else w.Xq[-1]
    near = float(w.y[np.argmin(((w.X - last[None, :]) ** 2).sum(axis=1)), 0])
    P.best = near + {"near": 0.0, "below": -100.0, "above": 100.0}[case["best"]]
    rng = np.random.default_rng(case["kw"]["seed"] + 7)
    P.Xq_all = np.concatenate([w.Xq[None], rng.uniform(0.05, 0.95, size=(case["E"] - 1, w.q, w.d))])
    return P


def ensemble_members(P):
    """(hypers [nm][1 + d], noises [nm][1]) of a case's ensemble: the workload's hyper-parameters scaled member by member."""
    w, nm = P.w, P.case["nm"]
    rng = np.random.default_rng(P.case["kw"]["seed"] + 1)
    hypers = np.column_stack([w.alpha * rng.uniform(0.7, 1.4, nm)] + [w.lengths[k] * rng.uniform(0.6, 1.6, nm) for k in range(w.d)])
    noises = np.asarray(w.noise, dtype=np.float64).reshape(1, -1) * rng.uniform(0.8, 1.2, (nm, 1))
    return hypers, noises
