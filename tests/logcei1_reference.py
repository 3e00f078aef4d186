"""The LOG of the constrained expected improvement with pending points, averaged over an ensemble, restated on the CPU (the checker
of tests/test_gpu_logcei1.py) in np.longdouble or float64, on top of tests/cei1_reference.py, whose Member, moments, ensemble,
CASES and make_problem are imported unchanged: the members, their conditioning on the pending points and the believed-feasible
incumbent b' are that file's.

With mu, var the posterior mean and the conditioned latent variance of the GP in question at x and ONE floor,
sigma = sqrt(max(150 eps^2, var)):
    role 0   c = (b' - mu) / sigma, h(c) = c Phi(c) + phi(c):  l = log sigma + log h(c),
             grad l = -(lambda / sigma) grad mu + (kappa / (2 sigma^2)) grad var,  lambda = Phi / h, kappa = phi / h;
             b' = +infinity: l = 0 and a zero gradient
    role k   z = (tau_k - mu) / sigma:  l = log Phi(z),  grad l = -(r / sigma) grad mu - (r z / (2 sigma^2)) grad var,  r = phi / Phi
    L_e = sum of the member's l, g_e of their gradients;  m = max_e L_e, w_e = exp(L_e - m), W = sum_e w_e
    value = m + log W - log E,  grad = (sum_e w_e g_e) / W
The scalars: below -3 Laplace's continued fraction of the Mills ratio with 400 terms, a = -c,
    t2 = a + 2 / (a + 3 / (a + ...)),  t1 = a + 1 / t2:  Phi / phi = 1 / t1,  h / phi = 1 / (t1 t2)
(all terms positive); from -3 on er.normal_cdf, kr.normal_pdf and kr._erfc_nonneg.  tests/test_logcei1_reference.py pins them
against mpmath.
"""
import collections
import copy

import numpy as np

import cei1_reference as cr
import ei1_reference as er
import kg1_reference as kr
from cei1_reference import CASES, WIDE_CASES, Member, ensemble, make_problem, moments  # noqa: F401

LD = cr.LD
FRACTION_BELOW = -3.0
FRACTION_TERMS = 400

Result = collections.namedtuple("Result", "value grad log_factors bprime args")

# (Delta best, Delta tau): every finite incumbent is lowered by the first, every threshold by the second
SHIFTS = ((0.0, 0.0), (3.0, 0.0), (8.0, 2.0))
# cei1_reference.WIDE_CASES run unshifted and at the deepest shift: its reference stays finite and qualified there (c and z down to
# -26.5, float64 within 7e-15 of long double, the pending points moving a checked value by 215)
WIDE_SHIFTS = (SHIFTS[0], SHIFTS[2])


def _half_log_2pi(T):
    return np.log(T(8) * np.arctan(T(1))) / T(2)


def _fraction(a, T):
    """(t1, t2) of the continued fraction at a > 0, bottom-up"""
    a = T(a)
    t = a
    for k in range(FRACTION_TERMS, 1, -1):
        t = a + T(k) / t
    return a + T(1) / t, t


def log_h_parts(c, T):
    """(log h(c), Phi(c) / h(c), phi(c) / h(c)) with h(c) = c Phi(c) + phi(c), in the arithmetic of T"""
    c = T(c)
    if c < T(FRACTION_BELOW):
        t1, t2 = _fraction(-c, T)
        return -c * c / T(2) - _half_log_2pi(T) - np.log(t1 * t2), t2, t1 * t2
    P, p = er.normal_cdf(c, T), kr.normal_pdf(c, T)
    h = c * P + p
    return np.log(h), P / h, p / h


def log_cdf_parts(z, T):
    """(log Phi(z), phi(z) / Phi(z)) in the arithmetic of T"""
    z = T(z)
    if z < T(FRACTION_BELOW):
        t1, _ = _fraction(-z, T)
        return -z * z / T(2) - _half_log_2pi(T) - np.log(t1), t1
    if z < 0:
        P = kr._erfc_nonneg(-z / np.sqrt(T(2)), T) / T(2)
        return np.log(P), kr.normal_pdf(z, T) / P
    q = kr._erfc_nonneg(z / np.sqrt(T(2)), T) / T(2)
    return np.log1p(-q), kr.normal_pdf(z, T) / (T(1) - q)


def role_log(T, mu, var, grad_mu, grad_var, limit, role):
    """(l, grad l, c or z) of one sub-member from its moments; limit: b' (role 0) or tau_k"""
    if role == 0 and np.isinf(limit):
        return T(0), np.zeros(len(grad_mu), dtype=T), T(np.inf)
    sigma = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), var))
    c = (T(limit) - mu) / sigma
    if role == 0:
        log_h, lam, kap = log_h_parts(c, T)
        return np.log(sigma) + log_h, -(lam / sigma) * grad_mu + (kap / (T(2) * sigma * sigma)) * grad_var, c
    log_cdf, r = log_cdf_parts(c, T)
    return log_cdf, -(r / sigma) * grad_mu - (r * c / (T(2) * sigma * sigma)) * grad_var, c


def member_logs(m, x):
    """([l_0 .. l_K], [their gradients], [c, z_1 .. z_K]) of a cr.Member at x"""
    limits = [m.bprime] + [m.T(t) for t in m.taus]
    out = [role_log(m.T, *moments(model, base, x), limit, r)
           for r, (model, base, limit) in enumerate(zip(m.models, m.bases, limits))]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def evaluate(members, x):
    """Result of the ensemble at x"""
    T = members[0].T
    Ls, gs, logs, args = [], [], [], []
    for m in members:
        vals, grads, cz = member_logs(m, x)
        L, g = vals[0], grads[0]
        for v, gr in zip(vals[1:], grads[1:]):
            L, g = L + v, g + gr
        Ls.append(L)
        gs.append(g)
        logs.append(vals)
        args.append([float(a) for a in cz])
    top = max(Ls)
    w = [np.exp(L - top) for L in Ls]
    W, num = w[0], w[0] * gs[0]
    for we, ge in zip(w[1:], gs[1:]):
        W, num = W + we, num + we * ge
    return Result(top + np.log(W) - np.log(T(len(members))), num / W, logs, [m.bprime for m in members], args)


# ---- the problems of tests/test_gpu_logcei1.py (tests/test_logcei1_reference.py qualifies them on the CPU) ----
_MEMBERS = {}


def _members(c, T, constraints=True):
    """the factored members of a case as it stands, once per process"""
    key = (c.name, T, constraints)
    if key not in _MEMBERS:
        p = make_problem(c)
        _MEMBERS[key] = (p, ensemble(p, T, constraints=constraints))
    return _MEMBERS[key]


def relimited(members, best, taus):
    """the same factored members under other incumbents [E] and thresholds [K]: the believed-feasible mask and b' are worked out
    anew, the factorisations are shared"""
    out = []
    for m, b in zip(members, best):
        n = copy.copy(m)
        n.best, n.taus = float(b), list(taus)[:len(m.taus)]
        n.mask = cr.believed_feasible(n.bases, n.P, n.taus)
        n.scale = cr.member_scale(n.gps, n.best)
        bp = n.T(n.best)
        if n.mask.any():
            bp = min(bp, min(cr.mean_at(n.bases[0], n.P[n.mask])))
        n.bprime = bp
        out.append(n)
    return out


def shifted(c, shift, T=LD, constraints=True):
    """(problem, members) of case c with every finite incumbent lowered by shift[0] and every threshold by shift[1]"""
    p, members = _members(c, T, constraints)
    best = [b - shift[0] if np.isfinite(b) else b for b in p.best]
    taus = [t - shift[1] for t in p.thresholds]
    return p._replace(best=best, thresholds=taus), relimited(members, best, taus)


_WANT = {}


def expected(c, shift, T=LD):
    """(problem, [Result per candidate]) of a case under a shift in the arithmetic of T, once per process"""
    key = (c.name, tuple(shift), T)
    if key not in _WANT:
        p, members = shifted(c, shift, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]


# The scalar regimes: one member, K = 1, n = 20, d = 3, six candidates; candidate i is evaluated under an incumbent and a threshold
# of its own, worked out from the float64 moments so that c lands at REGIME_TARGETS[i] and z at REGIME_TARGETS[(i + 3) % 6] -- inside
# each of REGIMES, both sides of every switch of the device's recipe (-6, 0) and of the restatement's (-3).  Both GPs have noise
# 1e-12 and candidate 1 lies REGIME_NEAR from a sampled point, where sigma is small.  Such a point cannot carry c below -1e4 by
# its small sigma alone: with |b' - mu| of the observations' order that needs sigma below 5e-5, the point within 1e-5; but var =
# k(x, x) - |v|^2 is a difference of numbers of order 1 that float64 keeps to about 1e-14 absolutely whatever the code, and the
# float64 restatement parts from long double (value, gradient; relative) by 2.5e-13, 5.1e-13 at 1e-2 (sigma 5e-2), 2.3e-12, 4.7e-12
# at 1e-3, 6.2e-11, 1.3e-10 at 1e-4, 1.8e-7, 3.7e-7 at 1e-5 (sigma 5e-5) and 2.3e-5, 4.5e-5 at 1e-6: the error grows as
# sigma^-2 (tests/test_logcei1_reference.py prints the ladder).  REGIME_NEAR is where float64 keeps a tenth of its bound of
# 2.5e-11, which leaves the device's own rounding of the same difference its room under 1e-10; the regime below -1e4 is reached
# through the incumbent and the threshold.
REGIMES = ((-np.inf, -1e4), (-100.0, -38.0), (-7.0, -6.0), (-6.0, -5.0), (-1.0, 1.0), (3.0, 8.0))
REGIME_TARGETS = (-3e4, -60.0, -6.5, -5.5, 0.3, 5.0)
REGIME_NEAR = 5e-3
REGIME_NOISE = 1e-12
_REGIMES = {}


def regime_inputs(near=REGIME_NEAR):
    """(problem, [(incumbent, threshold) per candidate])"""
    rng = np.random.default_rng(8722)
    n, d = 20, 3
    X = rng.uniform(0, 1, size=(n, d))
    length = cr.LENGTH_0 + cr.LENGTH_D * np.sqrt(d)
    gps = [[cr.GP(cr.MATERN, np.array([1.3] + [length] * d), X, 0.3 * rng.normal(size=(n, 1)), [REGIME_NOISE], ()),
            cr.GP(cr.SE, np.array([1.3] + [length] * d) * 1.15, X, 0.3 * rng.normal(size=(n, 1)), [REGIME_NOISE], ())]]
    points = rng.uniform(0.1, 0.9, size=(len(REGIMES), d))
    points[1] = X[4] + near * np.array([0.6, -0.5, 0.62])
    p = cr.Problem("regimes", gps, [0.0], [0.0], points, np.zeros((0, d)), tuple(range(len(REGIMES))))
    m = ensemble(p, np.float64)[0]
    limits = []
    for i, x in enumerate(points):
        pair = []
        for r, target in ((0, REGIME_TARGETS[i]), (1, REGIME_TARGETS[(i + 3) % len(REGIMES)])):
            mu, var, _, _ = moments(m.models[r], m.bases[r], x)
            pair.append(float(mu + target * np.sqrt(max(er.MIN_VAR_GRAD_EI, var))))
        limits.append(tuple(pair))
    return p, limits


def regime_expected(T=LD, near=REGIME_NEAR):
    """(problem, limits, [Result of candidate i under its own limits]) in the arithmetic of T, once per process"""
    key = (T, near)
    if key not in _REGIMES:
        p, limits = regime_inputs(near)
        members = ensemble(p, T)
        _REGIMES[key] = (p, limits, [evaluate(relimited(members, [b], [tau]), x) for x, (b, tau) in zip(p.points, limits)])
    return _REGIMES[key]


# The stall: problems on which the plain form and its gradient are exactly 0 in float64 at every start -- every incumbent 60 below
# the member's smallest observation -- and the log form climbs.
STALL_CASES = ("e1_k1_d3_n20_p3", "e3_k2_d3_n12_130_40_p3", "e1_k1_d3_n20_p0")
STALL_DROP = 60.0
STALL_GD = (12, 6, 2, 0, 0.7, 1.0, 0.5, 1e-10)
STALL_GAIN = 1.0


def stall_starts(d=3):
    return np.random.default_rng(77).uniform(0.02, 0.98, size=(12, d))


def stall(name, T=np.float64):
    """(problem, members) of a stall problem"""
    c = cr.case(name)
    p, members = _members(c, T)
    best = [float(np.min(row[0].y[:, 0])) - STALL_DROP for row in p.gps]
    return p._replace(best=best), relimited(members, best, p.thresholds)
