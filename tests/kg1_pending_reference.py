"""The discretised one-point knowledge gradient with pending points restated on the CPU (the checker of
tests/test_gpu_kg1_pending.py), on top of tests/kg1_reference.py, which is imported unchanged.

The posterior covariance is conditioned on the pending points P (with the GP's noise), the posterior mean is left alone: the
Kriging-believer fantasy, whose believed values are mu_n(P).  PendingModel is the conditioned GP written out in full: rows X u P,
L' = chol(K') of the whole (N + p) x (N + p) matrix in the arithmetic T, the base model's mean, and K'^-1 (y' - mean) = [alpha ; 0].
kg1_reference's DiscreteSet, lines and evaluate then apply as they are -- nothing of the device's extension (V_P, L_P, r) appears.
"""
import collections
import math

import numpy as np

import kg1_reference as kr
import sampling_reference as sr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN


class PendingModel(kr.Model):
    def __init__(self, base, pending):
        T = base.T
        self.T, self.cov_type, self.alpha, self.lengths = T, base.cov_type, base.alpha, base.lengths
        self.noise, self.mean, self.base = base.noise, base.mean, base
        P = np.asarray(pending, dtype=np.float64).reshape(-1, base.X.shape[1])
        self.X = np.vstack([base.X, P])
        rows = self.X.shape[0]
        K = self.cov(self.X, self.X)
        K[np.arange(rows), np.arange(rows)] += T(self.noise)
        self.L = sr.cholesky_spd(K) if T is LD else np.linalg.cholesky(K)
        self.kinvy = np.concatenate([base.kinvy, np.zeros(P.shape[0], dtype=T)])


# ---- the cases of tests/test_gpu_kg1_pending.py (tests/test_kg1_pending_reference.py qualifies them on the CPU) ----
Case = collections.namedtuple("Case", "name seed n d A p nf cov_type noise C")
GPU_CASES = [
    Case("n5_d2_A1_p1", 1, 5, 2, 1, 1, 0, MATERN, 1e-2, 5),
    Case("n20_d3_A12_p2_fid", 2, 20, 3, 12, 2, 1, MATERN, 1e-2, 5),
    Case("n40_d4_A64_p5_se", 3, 40, 4, 64, 5, 0, SE, 1e-2, 5),
    Case("n130_d3_A65_p3", 4, 130, 3, 65, 3, 0, MATERN, 1e-3, 5),  # 130 rows: the split-K side of tri_cols
    Case("n12_d2_A129_p8", 5, 12, 2, 129, 8, 0, MATERN, 1e-2, 5),
    Case("n130_d4_A12_p63_fid", 6, 130, 4, 12, 63, 1, MATERN, 1e-2, 5),
    Case("n20_d2_A12_p64", 7, 20, 2, 12, 64, 0, MATERN, 1e-2, 5),
    # padded dimensions 16, 24 and 32: the pending rows and the gradient's back product over run-time dp
    Case("n20_d16_A12_p3", 51, 20, 16, 12, 3, 0, MATERN, 1e-2, 5),
    Case("n20_d24_A12_p3_se", 55, 20, 24, 12, 3, 0, SE, 1e-2, 5),  # (seed chosen on the CPU: smallest margin 1.6e-4)
    Case("n20_d32_A12_p2_fid", 52, 20, 32, 12, 2, 1, MATERN, 1e-2, 5),
    # tri_cols' K slice: 128 for 512 < N <= 1024, 192 beyond (six slices at 1032 rows); the 'T' product over ld = N + pcap
    Case("n520_d3_A20_p2", 61, 520, 3, 20, 2, 0, MATERN, 1e-2, 5),
    Case("n1030_d4_A20_p2", 62, 1030, 4, 20, 2, 0, MATERN, 1e-2, 3),
    # (the last case stays last: tests/test_gpu_kg1_pending.py takes it by position)
    Case("n8_d2_A4095_p2", 28, 8, 2, 4095, 2, 0, MATERN, 1e-3, 1030),  # passes of 1024 candidates: C straddles one
]

# Length scales 0.05 + 0.1 sqrt(dim) and observations of spread 0.3 under alpha = 1.3: the posterior variance away from the data is of
# the order of alpha, so the slopes are of the order of the intercepts' spread, several lines share the envelope and conditioning on
# P moves the value (with tests/kg1_reference.py's inputs one line carries nearly all of the minimum and P moves the 6th digit).
LENGTH_0, LENGTH_D = 0.05, 0.1

Problem = collections.namedtuple("Problem", "case hyper X y noise discrete points pending best checked")


def make_problem(case):
    """the inputs of a case.  The first pending point lies within 0.05 of candidate 0 in every coordinate, so that conditioning on P
    moves that candidate's knowledge gradient by far more than the tolerance: a device that ignored P would fail."""
    rng = np.random.default_rng(8200 + case.seed)
    X = rng.uniform(0, 1, size=(case.n, case.d))
    y = 0.3 * rng.normal(size=(case.n, 1))
    hyper = np.array([1.3] + [LENGTH_0 + LENGTH_D * math.sqrt(case.d)] * case.d)
    discrete = rng.uniform(0, 1, size=(case.A, case.d - case.nf))
    points = rng.uniform(0.1, 0.9, size=(case.C, case.d))
    points[:, case.d - case.nf:] = rng.uniform(0.8, 0.95, size=(case.C, case.nf))  # (near the fidelity the set lives at)
    pending = rng.uniform(0, 1, size=(case.p, case.d))
    pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=case.d)
    checked = tuple(range(case.C)) if case.C <= 7 else (0, 1023, 1024, case.C - 1)
    return Problem(case, hyper, X, y, [case.noise], discrete, points, pending, float(y.min()), checked)


_WANT = {}


def models(p, T=LD):
    """(the base model, the model conditioned on the pending points) of a problem in the arithmetic of T"""
    base = kr.Model(p.case.cov_type, p.hyper, p.X, p.y, p.noise, T)
    return base, PendingModel(base, p.pending)


def expected(case, T=LD):
    """(problem, {candidate index: Result with P}, {candidate index: value without P}) in the arithmetic of T, once per process"""
    key = (case.name, T)
    if key not in _WANT:
        p = make_problem(case)
        base, cond = models(p, T)
        dset, dset0 = kr.DiscreteSet(cond, p.discrete, case.nf), kr.DiscreteSet(base, p.discrete, case.nf)
        with_p = {i: kr.evaluate(dset, p.points[i], p.best) for i in p.checked}
        without = {i: kr.evaluate(dset0, p.points[i], p.best, want_grad=False).value for i in p.checked}
        _WANT[key] = (p, with_p, without)
    return _WANT[key]


# ---- an ensemble: members of different N and different A_e, one list of pending points ----
ENSEMBLE = dict(seed=21, d=3, nf=1, n=(12, 40, 20), A=(12, 64, 5), cov=(MATERN, SE, MATERN), factors=(1.0, 1.3, 0.8), p=3, C=6)
# padded dimension 24 with a fidelity coordinate, two members of different N
ENSEMBLE_WIDE = dict(seed=71, d=17, nf=1, n=(12, 20), A=(12, 12), cov=(MATERN, SE), factors=(1.0, 1.3), p=3, C=6)

EnsembleProblem = collections.namedtuple("EnsembleProblem", "hyper X y noise cov discrete best points pending nf")


def make_ensemble(e=ENSEMBLE):
    rng = np.random.default_rng(8200 + e["seed"])
    X = rng.uniform(0, 1, size=(max(e["n"]), e["d"]))
    y = 0.3 * rng.normal(size=(max(e["n"]), 1))
    base = np.array([1.3] + [LENGTH_0 + LENGTH_D * math.sqrt(e["d"])] * e["d"])
    hyper = [base * f for f in e["factors"]]
    noise = [[1e-2 * f] for f in e["factors"]]
    discrete = [rng.uniform(0, 1, size=(A, e["d"] - e["nf"])) for A in e["A"]]
    best = [float(y[:n].min()) + 0.1 * k for k, n in enumerate(e["n"])]
    points = rng.uniform(0.1, 0.9, size=(e["C"], e["d"]))
    points[:, e["d"] - e["nf"]:] = rng.uniform(0.8, 0.95, size=(e["C"], e["nf"]))
    pending = rng.uniform(0, 1, size=(e["p"], e["d"]))
    pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=e["d"])
    return EnsembleProblem(hyper, [X[:n] for n in e["n"]], [y[:n] for n in e["n"]], noise, e["cov"], discrete, best, points, pending,
                           e["nf"])


def ensemble_expected(ep, pending, T=LD):
    """per candidate (mean of the members' values, mean of their gradients, mean scale, smallest margin) in the arithmetic of T"""
    sets = []
    for k in range(len(ep.X)):
        base = kr.Model(ep.cov[k], ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], T)
        model = PendingModel(base, pending) if len(pending) else base
        sets.append(kr.DiscreteSet(model, ep.discrete[k], ep.nf))
    out = []
    for x in ep.points:
        res = [kr.evaluate(s, x, b) for s, b in zip(sets, ep.best)]
        value, grad = T(0), np.zeros(len(x), dtype=T)
        for r in res:
            value, grad = value + r.value, grad + r.grad
        out.append((value / T(len(res)), grad / T(len(res)), float(np.mean([r.scale for r in res])),
                    min(min(r.margins) for r in res)))
    return out
