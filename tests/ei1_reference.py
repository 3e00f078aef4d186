"""The analytic one-point expected improvement with pending points, averaged over an ensemble, restated on the CPU (the checker of
tests/test_gpu_ei1.py) in np.longdouble or float64, on top of tests/kg1_reference.py (Model) and tests/kg1_pending_reference.py
(PendingModel), both imported unchanged.

PendingModel is the GP conditioned on the pending points P written out in full: rows X u P, the whole (N + p) x (N + p) matrix
factored in the arithmetic T, the base model's mean, and K'^-1 (y' - mean) = [K^-1 (y - mean) ; 0] -- nothing of the device's
extension appears.  With it, for a candidate x and a best value b:
    mu = mean + k(X', x) . kinvy',   var = k(x, x) - |L'^-1 k(X', x)|^2   (the latent function: no noise added)
    b' = min(b, min_j mu(P_j)),   t = b' - mu
    sigma = sqrt(max(DBL_MIN, var)),  c = t / sigma,   EI = max(0, t Phi(c) + sigma phi(c))
    sigma_g = sqrt(max(150 eps^2, var)),  c_g = t / sigma_g,   grad EI = -Phi(c_g) grad mu + phi(c_g) grad var / (2 sigma_g)
    grad mu = sum_r kinvy'_r grad_x k(X'_r, x),   grad var = -2 sum_r (L'^-T L'^-1 k(X', x))_r grad_x k(X'_r, x)
(OnePotentialSampleExpectedImprovementEvaluator, gpp_math.cpp:2195-2259: its two variance floors, its gradient d_a + d_b with the
d_c terms cancelled).  scale = max(1, |b|, max |y|, sqrt(alpha)).
"""
import collections
import math

import numpy as np

import kg1_pending_reference as kp
import kg1_reference as kr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN

MIN_VAR_EI = float(np.finfo(np.float64).tiny)                 # gpp_math.hpp:1316
MIN_VAR_GRAD_EI = 150.0 * float(np.finfo(np.float64).eps) ** 2  # gpp_math.hpp:1323

Result = collections.namedtuple("Result", "value grad sigma c bprime scale")


def normal_cdf(x, T):
    return kr.normal_cdf_diff(T(-np.inf), T(x), T)


def believed_best(base, pending, best):
    """b' = min(best, min_j mu(P_j)) in the arithmetic of the model"""
    T = base.T
    b = T(best)
    P = np.asarray(pending, dtype=np.float64).reshape(-1, base.X.shape[1])
    if len(P):
        mu = T(base.mean) + base.cov(base.X, P).T @ base.kinvy
        b = min(b, min(mu))
    return b


def evaluate(base, pending, x, best, y_max=0.0):
    """EI and its gradient at x for the model `base` conditioned on `pending` [p][dim] (may be empty)"""
    P = np.asarray(pending, dtype=np.float64).reshape(-1, base.X.shape[1])
    return evaluate_model(kp.PendingModel(base, P) if len(P) else base, base, P, x, best, y_max)


def evaluate_model(model, base, P, x, best, y_max=0.0):
    """the same with the conditioned model at hand (model = PendingModel(base, P), or base itself for an empty P): one factorisation
    serves every candidate"""
    T = base.T
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    k = model.cov(model.X, x)[:, 0]
    v = model.fwd(k)
    mu = T(base.mean) + k @ model.kinvy
    var = model.cov(x, x)[0, 0] - v @ v
    bp = believed_best(base, P, best)
    t = bp - mu
    sigma = np.sqrt(max(T(MIN_VAR_EI), var))
    c = t / sigma
    value = max(T(0), t * normal_cdf(c, T) + sigma * kr.normal_pdf(c, T))
    sg = np.sqrt(max(T(MIN_VAR_GRAD_EI), var))
    cg = t / sg
    gk = model.grad_cov(model.X, x)  # [N + p][dim]
    grad_mu = gk.T @ model.kinvy
    grad_var = T(-2) * (gk.T @ model.back(v))
    grad = -normal_cdf(cg, T) * grad_mu + kr.normal_pdf(cg, T) * grad_var / (T(2) * sg)
    scale = max(1.0, abs(float(best)), float(y_max), math.sqrt(float(base.alpha)))
    return Result(value, grad, float(sigma), float(c), float(bp), scale)


# ---- the cases of tests/test_gpu_ei1.py (tests/test_ei1_reference.py qualifies them on the CPU) ----
Problem = collections.namedtuple("Problem", "name cov_type hyper X y noise points pending best checked")


def _from_kp(case, name=None, p=None, best=None):
    q = kp.make_problem(case)
    pending = q.pending if p is None else q.pending[:p]
    return Problem(name or case.name, case.cov_type, q.hyper, q.X, q.y, q.noise, q.points, pending,
                   q.best if best is None else best(q), q.checked)


_D6 = kp.Case("n20_d6_p3", 41, 20, 6, 1, 3, 0, MATERN, 1e-2, 5)    # the DP = 8 gradient kernel
_D32 = kp.Case("n20_d32_p2", 42, 20, 32, 1, 2, 0, MATERN, 1e-2, 5)  # the DP = 32 gradient kernel
_BP = kp.Case("n40_d3_p4_bprime", 43, 40, 3, 1, 4, 0, MATERN, 1e-2, 5)


def problems():
    """kg1_pending_reference.GPU_CASES' first seven inputs (candidate 0 within 0.05 of pending point 0), d = 6 and d = 32 with and
    without pending points, and one case whose best value is max(y), so that b' binds"""
    out = [_from_kp(c) for c in kp.GPU_CASES[:7]]
    out += [_from_kp(_D6), _from_kp(_D32), _from_kp(_D6, "n20_d6_p0", 0), _from_kp(_D32, "n20_d32_p0", 0),
            _from_kp(_BP, best=lambda q: float(q.y.max()))]
    return out


PROBLEMS = problems()
BPRIME = "n40_d3_p4_bprime"

# ---- padded dimensions 12, 16 and 24, a second 256-row trip of the gradient kernel, tri_cols' K slices under ld = N + pcap ----
# From 256 rows on the best value is median(y): with min(y) and uniform candidates a GP on hundreds of points in 3 or 4 dimensions
# has c below -5 everywhere, EI below 1e-8 and a gradient below 1e-6, and an absolute bound of 1e-10 scale would pass a device that
# returned zeros.  With the median EI is 1e-2 .. 0.5 scale and the gradient of order 1 (tests/test_ei1_reference.py asserts both).
_W10 = kp.Case("n20_d10_p3", 81, 20, 10, 1, 3, 0, MATERN, 1e-2, 5)        # DP = 12, two padded coordinates
_W13 = kp.Case("n20_d13_p3_se", 82, 20, 13, 1, 3, 0, SE, 1e-2, 5)         # DP = 16, three padded coordinates
_W20 = kp.Case("n20_d20_p3", 83, 20, 20, 1, 3, 0, MATERN, 1e-2, 5)        # DP = 24, four padded coordinates
# (seed chosen on the CPU: b' = min(median, mu(P)) leaves every candidate an EI above 1e-2 scale; with most seeds two or three vanish)
_W300 = kp.Case("n300_d3_p3", 92, 300, 3, 1, 3, 0, MATERN, 1e-2, 5)       # 303 rows: a second trip; K slice 64, five slices
_W520 = kp.Case("n520_d3_p2", 85, 520, 3, 1, 2, 0, MATERN, 1e-2, 5)       # K slice 128
_W1030 = kp.Case("n1030_d4_p2", 86, 1030, 4, 1, 2, 0, MATERN, 1e-2, 3)    # K slice 192


def median_best(q):
    return float(np.median(q.y))


def wide_problems():
    return [_from_kp(_W10), _from_kp(_W13), _from_kp(_W20), _from_kp(_W300, best=median_best), _from_kp(_W520, best=median_best),
            _from_kp(_W1030, best=median_best), _from_kp(_W13, "n20_d13_p0_se", 0), _from_kp(_W300, "n300_d3_p0", 0, best=median_best)]


WIDE_PROBLEMS = wide_problems()

_WANT = {}


def base_model(p, T=LD):
    return kr.Model(p.cov_type, p.hyper, p.X, p.y, p.noise, T)


def expected(p, T=LD):
    """({candidate index: Result with P}, {candidate index: value without P}) in the arithmetic of T, once per process"""
    key = (p.name, T)
    if key not in _WANT:
        base = base_model(p, T)
        y_max = float(np.max(np.abs(p.y)))
        P = np.asarray(p.pending, dtype=np.float64).reshape(-1, p.X.shape[1])
        model = kp.PendingModel(base, P) if len(P) else base
        with_p = {i: evaluate_model(model, base, P, p.points[i], p.best, y_max) for i in p.checked}
        without = {i: evaluate_model(base, base, P[:0], p.points[i], p.best, y_max).value for i in p.checked}
        _WANT[key] = (with_p, without)
    return _WANT[key]


# ---- a three-member ensemble: different hyper-parameters, different n on both sides of 128 rows, one list of pending points ----
ENSEMBLE = dict(seed=51, d=3, n=(12, 130, 40), cov=(MATERN, SE, MATERN), factors=(1.0, 1.3, 0.8), p=3, C=6)
# padded dimension 12; n on both sides of 256 and of 512 rows (tri_cols' K slices 64 and 128 beside a member below 128 rows)
ENSEMBLE_WIDE = dict(seed=91, d=10, n=(20, 300, 600), cov=(MATERN, SE, MATERN), factors=(1.0, 1.3, 0.8), p=3, C=6)
EnsembleProblem = collections.namedtuple("EnsembleProblem", "hyper X y noise cov best points pending")


def make_ensemble(e=ENSEMBLE):
    rng = np.random.default_rng(8200 + e["seed"])
    X = rng.uniform(0, 1, size=(max(e["n"]), e["d"]))
    y = 0.3 * rng.normal(size=(max(e["n"]), 1))
    base = np.array([1.3] + [kp.LENGTH_0 + kp.LENGTH_D * math.sqrt(e["d"])] * e["d"])
    hyper = [base * f for f in e["factors"]]
    noise = [[1e-2 * f] for f in e["factors"]]
    best = [float(y[:n].min()) + 0.1 * k for k, n in enumerate(e["n"])]
    points = rng.uniform(0.1, 0.9, size=(e["C"], e["d"]))
    pending = rng.uniform(0, 1, size=(e["p"], e["d"]))
    pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=e["d"])
    return EnsembleProblem(hyper, [X[:n] for n in e["n"]], [y[:n] for n in e["n"]], noise, e["cov"], best, points, pending)


def ensemble_key(ep, pending, T):
    return ("ensemble", ep.points.shape[1], tuple(len(x) for x in ep.X), len(pending), T)


def ensemble_expected(ep, pending, T=LD):
    """per candidate (mean of the members' values, mean of their gradients, the largest member scale), once per process"""
    key = ensemble_key(ep, pending, T)
    if key in _WANT:
        return _WANT[key]
    bases = [kr.Model(ep.cov[k], ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], T) for k in range(len(ep.X))]
    out = _WANT[key] = []
    P = np.asarray(pending, dtype=np.float64).reshape(-1, ep.points.shape[1])
    models = [kp.PendingModel(m, P) if len(P) else m for m in bases]
    for x in ep.points:
        res = [evaluate_model(mm, m, P, x, b, float(np.max(np.abs(y)))) for mm, m, b, y in zip(models, bases, ep.best, ep.y)]
        value, grad = T(0), np.zeros(len(x), dtype=T)
        for r in res:
            value, grad = value + r.value, grad + r.grad
        out.append((value / T(len(res)), grad / T(len(res)), max(r.scale for r in res)))
    return out
