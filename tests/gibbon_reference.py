"""The min-value entropy acquisition GIBBON with pending points, averaged over an ensemble, restated on the CPU (the checker of
tests/test_gpu_gibbon.py) in np.longdouble or float64, on top of tests/kg1_reference.py (Model), tests/kg1_pending_reference.py
(PendingModel) and tests/ei1_deriv_reference.py (DerivModel, DerivPendingModel), all imported unchanged.

The conditioned GP is written out in full -- rows X u P, the whole matrix factored in the arithmetic T -- and nothing of the device's
extension or of its single gradient column appears: var0 comes from the base model, varc from the conditioned one, and the gradient
is A grad mu + B0 grad var0 + Bc grad varc with the three gradients formed separately.  For a candidate x, the member's noise
sigma^2 = noise[0] and its samples m_k of the minimum value (minimisation):
    mu = mean + k(X, x) . kinvy,   var0 = k(x, x) - |L^-1 k(X, x)|^2,   varc = k(x, x) - |L'^-1 k(X', x)|^2   (latent: no noise added)
    s0 = max(DBL_MIN, var0), sc likewise,  sigma0 = sqrt(s0),  rho^2 = s0 / (s0 + sigma^2),  gamma_k = (mu - m_k) / sigma0
    r = phi(gamma) / Phi(gamma),  q = clamp(r (gamma + r), 0, 1),  G = -1/2 log1p(-min(rho^2 q, 1 - DBL_EPSILON))
    alpha = [p > 0] 1/2 (log(sc + sigma^2) - log(s0 + sigma^2)) + mean_k G_k
    gradient: include/moe_hip.h's (moe_gibbon_mcmc), with max(150 eps^2, .) for both floors
In long double r is phi / Phi directly, Phi through erfc on the side of gamma's sign (kr.normal_cdf_diff); in float64 it is the
device's expression sqrt(2 / pi) / erfcx(-gamma / sqrt 2).  scale = max(1, max |y|, max |m|, sqrt(alpha)).
"""
import collections
import math

import numpy as np
import scipy.special

import ei1_deriv_reference as ed
import ei1_reference as er
import kg1_pending_reference as kp
import kg1_reference as kr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN
TINY, EPS = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).eps)
MIN_VAR_GRAD = 150.0 * EPS ** 2

Result = collections.namedtuple("Result", "value grad var0 varc sigma0 gammas bracket scale")


def _erfc_nonneg(x, T):
    """erfc(x) for an array x >= 0 in the arithmetic of T: kr._erfc_nonneg's two expressions (below 2.5 one minus the all-positive
    series of erf, from there on the continued fraction), element by element over the array"""
    x = np.asarray(x, dtype=T)
    root_pi = np.sqrt(T(4) * np.arctan(T(1)))
    e = np.exp(-x * x)
    xs = np.minimum(x, T(2.5))
    term, total, n = xs.copy(), xs.copy(), 0
    while True:
        n += 1
        term = term * T(2) * xs * xs / T(2 * n + 1)
        total = total + term
        if np.all(term <= total * T(np.finfo(T).eps) / T(8)):
            break
    series = T(1) - T(2) / root_pi * np.exp(-xs * xs) * total
    xc = np.maximum(x, T(2.5))
    t = xc.copy()
    for k in range(400, 0, -1):
        t = xc + T(k) / T(2) / t
    return np.where(x < T(2.5), series, e / (root_pi * t))


def normal_cdf(x, T):
    """Phi over an array, erfc on the side of x's sign"""
    x = np.asarray(x, dtype=T)
    half = _erfc_nonneg(np.abs(x) / np.sqrt(T(2)), T) / T(2)
    return np.where(x <= 0, half, T(1) - half)


def ratio(gamma, T):
    """(r, q) over an array of gammas in the arithmetic of T"""
    gamma = np.asarray(gamma, dtype=T)
    if T is LD:
        r = np.exp(-gamma * gamma / T(2)) / np.sqrt(T(8) * np.arctan(T(1))) / normal_cdf(gamma, T)
    else:
        with np.errstate(over="ignore"):
            r = math.sqrt(2.0 / math.pi) / scipy.special.erfcx(-gamma / math.sqrt(2.0))
    q = np.minimum(T(1), np.maximum(T(0), r * (gamma + r)))
    return r, q


def information(gamma, rho2, T):
    """G and its two partial derivatives at (gamma [K], rho^2)"""
    r, q = ratio(gamma, T)
    z = np.minimum(rho2 * q, T(1) - T(EPS))
    G = -np.log1p(-z) / T(2)
    dgamma = rho2 * (r - q * (gamma + T(2) * r)) / (T(1) - z) / T(2)
    drho = q / (T(1) - z) / T(2)
    return G, dgamma, drho


def _columns(model, x):
    """(k(rows, x), grad_x k(rows, x) [rows][dim]) of a plain or a derivative-observing model"""
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    if hasattr(model, "rows_cov"):
        kx = model.rows_cov(x, tuple(range(x.shape[1])))
        return np.ascontiguousarray(kx[:, 0]), np.ascontiguousarray(kx[:, 1:])
    return model.cov(model.X, x)[:, 0], model.grad_cov(model.X, x)


def conditioned(base, pending):
    """`base` conditioned on `pending` [p][dim], factored in full (`base` itself without pending points)"""
    P = np.asarray(pending, dtype=np.float64).reshape(-1, base.X.shape[1])
    if not len(P):
        return base
    return ed.DerivPendingModel(base, P) if hasattr(base, "rows_cov") else kp.PendingModel(base, P)


def evaluate(base, model, x, mins, y_max=0.0):
    """GIBBON and its gradient at x: `base` the member's GP, `model` = conditioned(base, pending), mins [K]"""
    T = base.T
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    m = np.asarray(mins, dtype=np.float64).ravel()
    noise = T(base.noise)
    k0, gk0 = _columns(base, x)
    v0 = base.fwd(k0)
    kxx = kr.covariance(base.cov_type, base.alpha, base.lengths, x, x, T)[0, 0]
    mu = T(base.mean) + k0 @ base.kinvy
    var0 = kxx - v0 @ v0
    pending = model is not base
    if pending:
        k, gk = _columns(model, x)
        v = model.fwd(k)
        varc = kxx - v @ v
    else:
        varc = var0
    s0, sc = max(T(TINY), var0), max(T(TINY), varc)
    sigma0, rho2 = np.sqrt(s0), s0 / (s0 + noise)
    mk = m.astype(T)
    gammas = (mu - mk) / sigma0
    value = np.sum(information(gammas, rho2, T)[0]) / T(len(m))
    bracket = (np.log(sc + noise) - np.log(s0 + noise)) / T(2) if pending else T(0)
    value = bracket + value
    # the gradient, with its own floor
    s0g, scg = max(T(MIN_VAR_GRAD), var0), max(T(MIN_VAR_GRAD), varc)
    sg, rho2g = np.sqrt(s0g), s0g / (s0g + noise)
    gg = (mu - mk) / sg
    _, dgamma, drho = information(gg, rho2g, T)
    A = np.sum(dgamma / sg) / T(len(m))
    B0 = np.sum(-gg * dgamma / (T(2) * s0g) + drho * noise / (s0g + noise) ** 2) / T(len(m))
    grad_mu = gk0.T @ base.kinvy
    grad_var0 = T(-2) * (gk0.T @ base.back(v0))
    grad = A * grad_mu + B0 * grad_var0
    if pending:
        grad_varc = T(-2) * (gk.T @ model.back(v))
        grad = grad - grad_var0 / (T(2) * (s0g + noise)) + grad_varc / (T(2) * (scg + noise))
    scale = max(1.0, float(y_max), float(np.max(np.abs(m))), math.sqrt(float(base.alpha)))
    return Result(value, grad, var0, varc, float(sigma0), (float(np.min(gammas)), float(np.max(gammas))), float(bracket), scale)


# ---- min-values: the minima of K seeded joint draws of the float64 base model at 200 uniform points ----
def draw_min_values(base64, K, seed, num_points=200):
    rng = np.random.default_rng(9100 + seed)
    d = base64.X.shape[1]
    Z = rng.uniform(0, 1, size=(num_points, d))
    if hasattr(base64, "rows_cov"):
        kz = base64.rows_cov(Z, ())
    else:
        kz = base64.cov(base64.X, Z)
    V = base64.fwd(kz)
    mu = base64.mean + kz.T @ base64.kinvy
    S = kr.covariance(base64.cov_type, base64.alpha, base64.lengths, Z, Z, np.float64) - V.T @ V
    S[np.arange(num_points), np.arange(num_points)] += 1e-9 * base64.alpha
    L = np.linalg.cholesky(S)
    draws = mu[:, None] + L @ rng.normal(size=(num_points, K))
    return np.ascontiguousarray(draws.min(axis=0))


# ---- the cases of tests/test_gpu_gibbon.py (tests/test_gibbon_reference.py qualifies them on the CPU) ----
Problem = collections.namedtuple("Problem", "name cov_type hyper X y noise derivs points pending mins checked")


def _base(p, T):
    if len(p.derivs):
        return ed.DerivModel(p.cov_type, p.hyper, p.X, p.y, p.noise, p.derivs, T)
    return kr.Model(p.cov_type, p.hyper, p.X, p.y, p.noise, T)


def base_model(p, T=LD):
    return _base(p, T)


# The candidates at which the two movement conditions of tests/test_gibbon_reference.py are asserted, where they are not all of a
# case's: the others lie so far from every pending point, or so far above every min-value (every gamma above about 4.5, up to 22:
# the terms sum to less than 1e-5), that P or the min-values move their value by less than 1e-5 scale whatever the code does.  Value and gradient are compared at EVERY candidate all the same.
_CHECKED = {"n40_d4_A64_p5_se": (0, 1, 2, 4), "n130_d3_A65_p3": (0, 1, 3), "n20_d32_p2": (0, 1, 3, 4), "n5_d2_g2_p1": (0, 1, 3, 4),
            "n44_d3_g2_p3_noise1e-3": (0, 4), "n10_d2_p2_noise_free": (0, 2, 3, 4),
            # the wide cases: P moves the others by less than 1e-5 scale (in 13 dimensions they lie far from both pending points), and in
            # the derivative case every gamma of candidates 2 to 4 lies above 3.6: the min-values move them by less than 6e-6
            "n20_d13_p3_se": (0, 1, 2, 4), "n10_d13_D0_12_p2": (0, 1), "n300_d3_p3_near_the_lowest_K130": (0, 2, 3)}


def _with_mins(name, q, derivs, K, seed):
    p = Problem(name, q.cov_type, q.hyper, q.X, q.y, q.noise, tuple(derivs), q.points, q.pending, None,
                _CHECKED.get(name, tuple(range(len(q.points)))))
    return p._replace(mins=draw_min_values(_base(p, np.float64), K, seed))


_KS = (64, 63, 65, 1, 64, 1024, 64, 65, 63, 64, 1, 64)  # (per case of ei1_reference.PROBLEMS)
NEGATIVE, NOISE_FREE = "n20_d6_p3_gamma_below_0", "n10_d2_p2_noise_free"
G2, ROWS141 = "n5_d2_g2_p1", "n44_d3_g2_p3_noise1e-3"


def _noise_free():
    """a noise-free member (rho^2 = 1, the bracket's logarithms take the latent variances alone); the candidates keep away from X u P"""
    rng = np.random.default_rng(9177)
    n, d = 10, 2
    X = rng.uniform(0, 1, size=(n, d))
    y = 0.3 * rng.normal(size=(n, 1))
    hyper = np.array([1.3, 0.2, 0.2])
    pending = rng.uniform(0.1, 0.9, size=(2, d))
    rows = np.vstack([X, pending])
    points = []
    while len(points) < 5:
        x = rng.uniform(0.05, 0.95, size=d)
        if np.min(np.max(np.abs(rows - x), axis=1)) >= 0.08:
            points.append(x)
    points = np.array(points)
    points[0] = pending[0] + np.array([0.09, -0.08])
    q = er.Problem(NOISE_FREE, MATERN, hyper, X, y, [0.0], points, pending, 0.0, tuple(range(5)))
    return _with_mins(NOISE_FREE, q, (), 64, 77)


def problems():
    out = [_with_mins(q.name, q, (), K, 10 + i) for i, (q, K) in enumerate(zip(er.PROBLEMS, _KS))]
    # one min-value raised above mu at a checked candidate: gamma < 0
    src = [p for p in out if p.name == "n20_d6_p3"][0]
    base = _base(src, np.float64)
    mu1 = float(base.mean + base.cov(base.X, src.points[1:2])[:, 0] @ base.kinvy)
    mins = src.mins.copy()
    mins[0] = mu1 + 0.4
    out.append(src._replace(name=NEGATIVE, mins=mins))
    for name, K, seed in ((G2, 65, 31), (ROWS141, 63, 32)):
        q = [c for c in ed.PROBLEMS if c.name == name][0]
        out.append(_with_mins(name, q, q.derivs, K, seed))
    out.append(_noise_free())
    return out


PROBLEMS = problems()

WIDE_N300 = "n300_d3_p3_near_the_lowest_K130"
# (seeds chosen on the CPU: the min-values move every candidate by >= 2.7e-5 scale, P moves candidates 0, 2 and 3 by >= 4.9e-4)
_G300 = kp.Case("n300_d3_p3", 84, 300, 3, 1, 3, 0, MATERN, 1e-2, 5)


def _near_the_lowest():
    """tests/ei1_reference.py's 300-point inputs with the candidates within 0.05 of the five sampled points of lowest y and pending
    point 0 within 0.05 of candidate 0: with uniform candidates every gamma lies above 2, up to 25, and the min-values move some
    candidates' values by less than 1e-10"""
    q = er._from_kp(_G300)
    rng = np.random.default_rng(9184)
    low = np.argsort(q.y[:, 0])[:5]
    points = np.clip(q.X[low] + rng.uniform(-0.05, 0.05, size=(5, q.X.shape[1])), 0.0, 1.0)
    pending = q.pending.copy()
    pending[0] = np.clip(points[0] + rng.uniform(-0.05, 0.05, size=q.X.shape[1]), 0.0, 1.0)
    return _with_mins(WIDE_N300, q._replace(points=points, pending=pending), (), 130, 84)


def wide_problems():
    """padded dimensions 16 and 24 with K on both sides of 64, derivative rows at padded dimension 16, and 300 rows under 130
    min-values: five 64-row trips of the candidate kernel's chain with N no multiple of 64, a third trip over the min-values"""
    by_name = {q.name: q for q in er.WIDE_PROBLEMS}
    out = [_with_mins(name, by_name[name], (), K, seed) for name, K, seed in (("n20_d13_p3_se", 65, 41), ("n20_d20_p3", 63, 42))]
    q = ed.WIDE_PROBLEMS[0]
    out.append(_with_mins(q.name, q, q.derivs, 64, 44))  # (seed chosen on the CPU: the min-values move candidates 0 and 1 by 3e-5)
    out.append(_near_the_lowest())
    return out


WIDE_PROBLEMS = wide_problems()

_WANT = {}


def expected(p, T=LD):
    """({candidate index: Result with P}, {index: value without P}, {index: value with P and the min-values shifted by -1}) over
    every candidate in the arithmetic of T, once per process"""
    key = (p.name, T)
    if key not in _WANT:
        base = _base(p, T)
        model = conditioned(base, p.pending)
        y_max = float(np.max(np.abs(p.y)))
        with_p = {i: evaluate(base, model, p.points[i], p.mins, y_max) for i in range(len(p.points))}
        without = {i: evaluate(base, base, p.points[i], p.mins, y_max).value for i in range(len(p.points))}
        shifted = {i: evaluate(base, model, p.points[i], p.mins - 1.0, y_max).value for i in range(len(p.points))}
        _WANT[key] = (with_p, without, shifted)
    return _WANT[key]


# ---- ei1_reference's three-member ensembles (N = 12 / 130 / 40; ENSEMBLE_WIDE: 20 / 300 / 600) with min-values of its own per member ----
ENSEMBLE_K = 64


def make_ensemble(e=er.ENSEMBLE):
    ep = er.make_ensemble(e)
    mins = np.array([draw_min_values(kr.Model(ep.cov[k], ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], np.float64), ENSEMBLE_K, 50 + k)
                     for k in range(len(ep.X))])
    return ep, mins


def ensemble_expected(ep, mins, pending, T=LD):
    """per candidate (mean of the members' values, mean of their gradients, the largest member scale)"""
    key = er.ensemble_key(ep, pending, T)
    if key not in _WANT:
        bases = [kr.Model(ep.cov[k], ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], T) for k in range(len(ep.X))]
        models = [conditioned(b, pending) for b in bases]
        out = []
        for x in ep.points:
            res = [evaluate(b, mm, x, mk, float(np.max(np.abs(y)))) for b, mm, mk, y in zip(bases, models, mins, ep.y)]
            value, grad = T(0), np.zeros(len(x), dtype=T)
            for r in res:
                value, grad = value + r.value, grad + r.grad
            out.append((value / T(len(res)), grad / T(len(res)), max(r.scale for r in res)))
        _WANT[key] = out
    return _WANT[key]
