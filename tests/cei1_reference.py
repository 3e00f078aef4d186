"""The constrained expected improvement (expected improvement times the probability of feasibility) with pending points, averaged
over an ensemble, restated on the CPU (the checker of tests/test_gpu_cei1.py) in np.longdouble or float64, on top of
tests/kg1_reference.py (Model), tests/kg1_pending_reference.py (PendingModel) and, for GPs with derivative observations,
tests/ei1_deriv_reference.py (DerivModel, DerivPendingModel), all imported unchanged: the (N + p)^2 system of every GP is factored
in full and nothing of the device's extension appears.

Member e is 1 + K GPs: role 0 the objective, role k constraint k, satisfied where c_k(x) <= tau_k.  With mu, var the posterior
mean and the conditioned latent variance of the GP in question at x:
    F_k = Phi(z),  z = (tau_k - mu) / sigma,  sigma = sqrt(max(DBL_MIN, var))
    grad F_k = -(phi(z_g) / sigma_g) grad mu - (phi(z_g) z_g / (2 sigma_g^2)) grad var,  sigma_g = sqrt(max(150 eps^2, var))
    EI: tests/ei1_reference.py's evaluate_model (ei1_deriv_reference's for derivative observations) with the incumbent
        b' = min(b, min over the believed-feasible pending points j of mu_0(P_j)),  P_j believed feasible when mu_k(P_j) <= tau_k
        for every k; while b' is +infinity the factor is exactly 1 and its gradient 0
    A_e = EI F_1 ... F_K,  grad A_e by the product rule;  value = (A_0 + ... + A_{E-1}) / E
scale = max(1, |best| (where finite), max |y|, sqrt(alpha)) over the member's GPs; an ensemble takes its largest member scale.
"""
import collections
import math

import numpy as np

import ei1_deriv_reference as ed
import ei1_reference as er
import kg1_pending_reference as kp
import kg1_reference as kr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN

GP = collections.namedtuple("GP", "cov_type hyper X y noise derivs")
Problem = collections.namedtuple("Problem", "name gps thresholds best points pending checked")
Result = collections.namedtuple("Result", "value grad factors scale bprime")


def base_model(gp, T=LD):
    if gp.derivs:
        return ed.DerivModel(gp.cov_type, gp.hyper, gp.X, gp.y, gp.noise, gp.derivs, T)
    return kr.Model(gp.cov_type, gp.hyper, gp.X, gp.y, gp.noise, T)


def conditioned(base, P):
    if not len(P):
        return base
    return ed.DerivPendingModel(base, P) if isinstance(base, ed.DerivModel) else kp.PendingModel(base, P)


def mean_at(base, P):
    """mu(P_j), the believed function values, in the arithmetic of the model"""
    T = base.T
    k = base.rows_cov(P, ()) if isinstance(base, ed.DerivModel) else base.cov(base.X, P)
    return T(base.mean) + k.T @ base.kinvy


def moments(model, base, x):
    """(mu, var, grad mu, grad var) of the latent function at x under the conditioned model"""
    T = base.T
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    if isinstance(base, ed.DerivModel):
        kx = model.rows_cov(x, tuple(range(x.shape[1])))
        k, gk = np.ascontiguousarray(kx[:, 0]), np.ascontiguousarray(kx[:, 1:])
        kxx = kr.covariance(base.cov_type, base.alpha, base.lengths, x, x, T)[0, 0]
    else:
        k, gk = model.cov(model.X, x)[:, 0], model.grad_cov(model.X, x)
        kxx = model.cov(x, x)[0, 0]
    v = model.fwd(k)
    return T(base.mean) + k @ model.kinvy, kxx - v @ v, gk.T @ model.kinvy, T(-2) * (gk.T @ model.back(v))


def feasibility(model, base, x, tau):
    """(F, grad F) of one constraint GP at x"""
    T = base.T
    mu, var, grad_mu, grad_var = moments(model, base, x)
    t = T(tau) - mu
    sigma = np.sqrt(max(T(er.MIN_VAR_EI), var))
    F = er.normal_cdf(t / sigma, T)
    sg = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), var))
    zg = t / sg
    pg = kr.normal_pdf(zg, T)
    return F, -(pg / sg) * grad_mu - (pg * zg / (T(2) * sg * sg)) * grad_var


def believed_feasible(bases, P, taus):
    """the pending points a member (its 1 + K base models) believes feasible: a boolean mask [p]"""
    ok = np.ones(len(P), dtype=bool)
    for base, tau in zip(bases[1:], taus):
        if len(P):
            ok &= np.array([m <= base.T(tau) for m in mean_at(base, P)], dtype=bool)
    return ok


def member_scale(gps, best):
    s = max([1.0] + [float(np.max(np.abs(np.asarray(g.y, dtype=np.float64).reshape(len(g.X), -1)[:, 0]))) for g in gps] +
            [math.sqrt(float(np.asarray(g.hyper).ravel()[0])) for g in gps])
    return max(s, abs(float(best))) if math.isfinite(float(best)) else s


class Member(object):
    """one member's 1 + K GPs conditioned on P, factored once for every candidate"""

    def __init__(self, gps, taus, best, P, T=LD):
        self.T, self.gps, self.taus, self.best = T, gps, list(taus), float(best)
        self.P = np.asarray(P, dtype=np.float64).reshape(-1, np.asarray(gps[0].X).shape[1])
        self.bases = [base_model(g, T) for g in gps]
        self.models = [conditioned(b, self.P) for b in self.bases]
        self.mask = believed_feasible(self.bases, self.P, self.taus)
        self.scale = member_scale(gps, best)
        b = T(self.best)
        if self.mask.any():
            b = min(b, min(mean_at(self.bases[0], self.P[self.mask])))
        self.bprime = b

    def factors(self, x):
        """([EI, F_1 .. F_K], [their gradients]) at x"""
        T = self.T
        if np.isinf(self.bprime):
            vals, grads = [T(1)], [np.zeros(len(x), dtype=T)]
        else:
            ev = ed.evaluate_model if isinstance(self.bases[0], ed.DerivModel) else er.evaluate_model
            r = ev(self.models[0], self.bases[0], self.P[self.mask], x, self.best)
            vals, grads = [r.value], [r.grad]
        for model, base, tau in zip(self.models[1:], self.bases[1:], self.taus):
            F, gF = feasibility(model, base, x, tau)
            vals.append(F)
            grads.append(gF)
        return vals, grads

    def evaluate(self, x):
        """(A_e, grad A_e, the factors) at x"""
        T = self.T
        vals, grads = self.factors(x)
        a = vals[0]
        for f in vals[1:]:
            a = a * f
        grad = np.zeros(len(x), dtype=T)
        for r in range(len(vals)):
            ex = T(1)
            for q in range(len(vals)):
                if q != r:
                    ex = ex * vals[q]
            grad = grad + ex * grads[r]
        return a, grad, vals


def ensemble(p, T=LD, pending=None, constraints=True):
    """the members of a problem (pending: another list than the problem's; constraints=False: the objective GPs alone)"""
    P = p.pending if pending is None else pending
    K = len(p.thresholds) if constraints else 0
    return [Member(g[:1 + K], p.thresholds[:K], b, P, T) for g, b in zip(p.gps, p.best)]


def evaluate(members, x):
    """Result of the ensemble at x"""
    T = members[0].T
    value, grad, factors = T(0), np.zeros(len(x), dtype=T), []
    for m in members:
        a, g, vals = m.evaluate(x)
        value, grad = value + a, grad + g
        factors.append(vals)
    n = T(len(members))
    return Result(value / n, grad / n, factors, max(m.scale for m in members), [m.bprime for m in members])


# ---- the cases of tests/test_gpu_cei1.py (tests/test_cei1_reference.py qualifies them on the CPU) ----
# Case: E members of 1 + K GPs in dim d; n[e][role] observations; p pending points; derivs: the observed-derivative list of every GP;
# best: "median" / "max" of the member's objective values, or a list with numbers and "inf"; tau [K]; offset[e][k]: the mean level of
# constraint k's observations under member e (observations of spread 0.3 around it, as the objective's around 0); checked: the
# candidates at which tests/test_cei1_reference.py's qualification conditions hold (None: all C), chosen on the CPU -- elsewhere a
# feasibility factor leaves [0.02, 0.98] or a product falls below 1e-3 scale whatever the code under test does.
Case = collections.namedtuple("Case", "name seed E K d n p derivs best tau offset C checked")

LENGTH_0, LENGTH_D = kp.LENGTH_0, kp.LENGTH_D


def _grid(E, K, n):
    return tuple(tuple(n for _ in range(1 + K)) for _ in range(E))


CASES = [
    Case("e1_k1_d3_n20_p0", 1, 1, 1, 3, _grid(1, 1, 20), 0, (), "median", (0.0,), None, 6, None),
    Case("e1_k1_d3_n20_p3", 2, 1, 1, 3, _grid(1, 1, 20), 3, (), "median", (0.0,), None, 6, (0, 2, 3, 4)),
    # n on both sides of tri_cols' 128-row switch, shuffled over the roles: the members' chains do not line up
    Case("e3_k2_d3_n12_130_40_p3", 3, 3, 2, 3, ((12, 130, 40), (130, 40, 12), (40, 12, 130)), 3, (), "median", (0.1, 0.0), None, 6, (2, 3, 4)),
    Case("e1_k1_d10_n20_p2", 4, 1, 1, 10, _grid(1, 1, 20), 2, (), "median", (0.0,), None, 6, None),   # the <12> gradient kernel
    Case("e1_k1_d3_n300_p2", 5, 1, 1, 3, ((300, 40),), 2, (), "median", (0.0,), None, 6, (0, 1, 3)),         # R > 256
    Case("e1_k1_d3_n12_g1_p2", 6, 1, 1, 3, _grid(1, 1, 12), 2, (1,), "median", (0.0,), None, 6, None),  # 1 + g = 2 rows per point
    # pending point 0 lies on a sampled point of the constraint GPs, whose observations sit at -0.5 under member 0 (believed
    # feasible: it lowers b'_0) and at +0.5 under member 1 (believed infeasible: b'_1 stays although mu_0(P_0) < b_1)
    Case("e2_k1_d3_n20_p2_mixed", 7, 2, 1, 3, _grid(2, 1, 20), 2, (), "max", (0.0,), ((-0.5,), (0.5,)), 6, (0, 2, 3, 4, 5)),
    # member 0 has no feasible observation; its pending points are believed infeasible (b'_0 stays +infinity) ...
    Case("e2_k1_d3_n20_p2_inf", 8, 2, 1, 3, _grid(2, 1, 20), 2, (), ("inf", "median"), (0.0,), ((0.5,), (-0.2,)), 6, (0, 1, 2, 3)),
    # ... or pending point 0 is believed feasible and makes b'_0 finite
    Case("e2_k1_d3_n20_p2_inf_feasible", 9, 2, 1, 3, _grid(2, 1, 20), 2, (), ("inf", "median"), (0.0,), ((-0.5,), (-0.2,)), 6, None),
    Case("e1_k8_d3_n20_p1", 10, 1, 8, 3, _grid(1, 8, 20), 1, (), "median", (0.3,) * 8, None, 6, (3, 4, 5)),
]
# The staging of groups of 1 + K sub-members at a wide padded dimension (24) with unequal members: rows (20, 300, 600) shuffled over
# the three roles per member as ENSEMBLE shuffles its own -- a different R per sub-member, three strides of 256 rows
WIDE = Case("e3_k2_d20_n20_300_600_p3", 11, 3, 2, 20, ((20, 300, 600), (300, 600, 20), (600, 20, 300)), 3, (), "median", (0.1, 0.0), None, 6,
            None)
WIDE_CASES = [WIDE]
MIXED, INF, INF_FEASIBLE = "e2_k1_d3_n20_p2_mixed", "e2_k1_d3_n20_p2_inf", "e2_k1_d3_n20_p2_inf_feasible"
ENSEMBLE = "e3_k2_d3_n12_130_40_p3"


def case(name):
    return next(c for c in CASES + WIDE_CASES if c.name == name)


def make_problem(c):
    """the inputs of a case.  The first pending point lies within 0.05 of candidate 0 in every coordinate (conditioning on P moves
    that candidate by far more than the tolerance) -- or, where the case sets constraint levels, on the first sampled point the
    constraint GPs share, so that every member's belief about its feasibility is firm."""
    rng = np.random.default_rng(8600 + c.seed)
    g1 = 1 + len(c.derivs)
    length = LENGTH_0 + LENGTH_D * math.sqrt(c.d)
    Xc = rng.uniform(0, 1, size=(max(max(row) for row in c.n), c.d))  # (the constraint GPs of a case observe nested point lists)
    gps = []
    for e in range(c.E):
        row = []
        for r in range(1 + c.K):
            n = c.n[e][r]
            X = rng.uniform(0, 1, size=(n, c.d)) if r == 0 else Xc[:n]
            level = 0.0 if (r == 0 or c.offset is None) else c.offset[e][r - 1]
            y = level + 0.3 * rng.normal(size=(n, g1))
            f = 1.0 + 0.15 * ((e + 2 * r) % 4)
            hyper = np.array([1.3] + [length] * c.d) * f
            row.append(GP(MATERN if (e + r) % 2 == 0 else SE, hyper, X, y, [1e-2 * f] * g1, tuple(c.derivs)))
        gps.append(row)
    best = []
    for e in range(c.E):
        y0 = gps[e][0].y[:, 0]
        mode = c.best if isinstance(c.best, str) else c.best[e]
        best.append(float("inf") if mode == "inf" else float(np.median(y0)) if mode == "median" else float(y0.max()) if mode == "max"
                    else float(mode))
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    pending = rng.uniform(0, 1, size=(c.p, c.d))
    if c.p:
        pending[0] = Xc[0] if c.offset is not None else points[0] + rng.uniform(-0.05, 0.05, size=c.d)
    checked = tuple(range(c.C)) if c.checked is None else tuple(c.checked)
    return Problem(c.name, gps, list(c.tau), best, points, pending, checked)


_WANT = {}


def expected(c, T=LD):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T)
    if key not in _WANT:
        p = make_problem(c)
        members = ensemble(p, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]
