"""The two-objective expected hypervolume improvement with pending points, averaged over an ensemble, restated on the CPU (the
checker of tests/test_gpu_ehvi.py) in np.longdouble or float64, on top of tests/kg1_reference.py (Model),
tests/kg1_pending_reference.py (PendingModel) and tests/cei1_reference.py (moments, mean_at, base_model, conditioned), all imported
unchanged: the (N + p)^2 system of every GP is factored in full and nothing of the device's extension appears.

Minimisation.  Member e is two GPs, objective 1 and objective 2; r = (r1, r2) the reference point; the front F >= 0 points
(u_i, v_i), u ascending and v descending, strictly inside r; u_0 = -infinity, u_{F+1} = r1, v_0 = r2.  With mu, var the posterior
mean and the conditioned latent variance of the GP in question at x:
    psi(t) = (t - mu) Phi(z) + sigma phi(z),  z = (t - mu) / sigma,  sigma = sqrt(max(DBL_MIN, var)),  psi_1(-infinity) = 0
    A_e = max(0, sum_{i = 0 .. F} [psi_1(u_{i+1}) - psi_1(u_i)] psi_2(v_i)),  the strips added in the order of i
    grad A_e through d psi / d mu = -Phi(z_g), d psi / d var = phi(z_g) / (2 sigma_g), sigma_g = sqrt(max(150 eps^2, var)); 0 where
    the sum is not positive
    value = (A_0 + ... + A_{E-1}) / E
The believed-front rule: the believed outcome (mu_1(P_j), mu_2(P_j)) of pending point j joins the member's own front, in the order
of j, when it lies strictly inside r and no front point (u, v) has u <= a and v <= b; the front points with u >= a and v >= b leave.
scale = max(1, |r1|, |r2|, max |y|, sqrt(alpha)) over the member's two GPs; an ensemble takes its largest member scale.
"""
import collections
import math

import numpy as np

import cei1_reference as cr
import ei1_reference as er
import kg1_pending_reference as kp
import kg1_reference as kr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN
GP = cr.GP

Problem = collections.namedtuple("Problem", "name gps ref front points pending checked")
Result = collections.namedtuple("Result", "value grad members scale means")


def psi(t, mu, var, T):
    """(psi, d psi / d mu, d psi / d var) at the edge t"""
    t, mu, var = T(t), T(mu), T(var)
    sigma = np.sqrt(max(T(er.MIN_VAR_EI), var))
    z = (t - mu) / sigma
    value = (t - mu) * er.normal_cdf(z, T) + sigma * kr.normal_pdf(z, T)
    sg = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), var))
    zg = (t - mu) / sg
    return value, -er.normal_cdf(zg, T), kr.normal_pdf(zg, T) / (T(2) * sg)


def strips(mu1, var1, mu2, var2, front, ref, T=LD):
    """(A, (dA/dmu1, dA/dvar1, dA/dmu2, dA/dvar2)) of one member from its moments, its front [F][2] and r"""
    front = np.asarray(front, dtype=T).reshape(-1, 2)
    F = len(front)
    zero = (T(0), T(0), T(0))
    left = zero
    total, c = T(0), [T(0), T(0), T(0), T(0)]
    for i in range(F + 1):
        right = psi(front[i, 0] if i < F else ref[0], mu1, var1, T)
        q = psi(ref[1] if i == 0 else front[i - 1, 1], mu2, var2, T)
        dP = right[0] - left[0]
        total = total + dP * q[0]
        c[0] = c[0] + (right[1] - left[1]) * q[0]
        c[1] = c[1] + (right[2] - left[2]) * q[0]
        c[2] = c[2] + dP * q[1]
        c[3] = c[3] + dP * q[2]
        left = right
    if not total > 0:
        return T(0), [T(0)] * 4
    return total, c


def believed_front(front, outcomes, ref, T=LD):
    """(the front after the believed outcomes [p][2] have joined in order, a log with one entry per outcome: ("outside", 0),
    ("dominated", 0) or ("joined", the number of front points that left))"""
    f = [(T(u), T(v)) for u, v in np.asarray(front, dtype=T).reshape(-1, 2)]
    log = []
    for a, b in outcomes:
        a, b = T(a), T(b)
        if not (a < T(ref[0]) and b < T(ref[1])):
            log.append(("outside", 0))
            continue
        if any(u <= a and v <= b for u, v in f):
            log.append(("dominated", 0))
            continue
        kept = [(u, v) for u, v in f if not (u >= a and v >= b)]
        log.append(("joined", len(f) - len(kept)))
        f = sorted(kept + [(a, b)], key=lambda uv: uv[0])
    return np.array(f, dtype=T).reshape(-1, 2), log


def member_scale(gps, ref):
    return max([1.0, abs(float(ref[0])), abs(float(ref[1]))] +
               [float(np.max(np.abs(np.asarray(g.y, dtype=np.float64)))) for g in gps] +
               [math.sqrt(float(np.asarray(g.hyper).ravel()[0])) for g in gps])


class Member(object):
    """one member's two GPs conditioned on P and its own front, factored once for every candidate"""

    def __init__(self, gps, ref, front, P, T=LD):
        self.T, self.gps, self.ref = T, gps, (float(ref[0]), float(ref[1]))
        self.P = np.asarray(P, dtype=np.float64).reshape(-1, np.asarray(gps[0].X).shape[1])
        self.bases = [cr.base_model(g, T) for g in gps]
        self.models = [cr.conditioned(b, self.P) for b in self.bases]
        if len(self.P):
            m1, m2 = cr.mean_at(self.bases[0], self.P), cr.mean_at(self.bases[1], self.P)
            self.outcomes = list(zip(m1, m2))
        else:
            self.outcomes = []
        self.front, self.log = believed_front(front, self.outcomes, self.ref, T)
        self.scale = member_scale(gps, ref)

    def evaluate(self, x):
        """(A_e, grad A_e, (mu_1, mu_2)) at x"""
        mo = [cr.moments(m, b, x) for m, b in zip(self.models, self.bases)]
        a, c = strips(mo[0][0], mo[0][1], mo[1][0], mo[1][1], self.front, self.ref, self.T)
        grad = c[0] * mo[0][2] + c[1] * mo[0][3] + c[2] * mo[1][2] + c[3] * mo[1][3]
        return a, grad, (mo[0][0], mo[1][0])


def ensemble(p, T=LD, pending=None, front=None):
    """the members of a problem (pending / front: others than the problem's)"""
    P = p.pending if pending is None else pending
    f = p.front if front is None else front
    return [Member(g, p.ref, f, P, T) for g in p.gps]


def evaluate(members, x):
    T = members[0].T
    value, grad, vals, means = T(0), np.zeros(len(x), dtype=T), [], []
    for m in members:
        a, g, mu = m.evaluate(x)
        value, grad = value + a, grad + g
        vals.append(a)
        means.append(mu)
    n = T(len(members))
    return Result(value / n, grad / n, vals, max(m.scale for m in members), means)


def dominated(front, a, b):
    return any(u <= a and v <= b for u, v in np.asarray(front).reshape(-1, 2))


# ---- the cases of tests/test_gpu_ehvi.py (tests/test_ehvi_reference.py qualifies them on the CPU) ----
# Case: E members of two GPs in dim d; n[e][objective] observations; p pending points; F front points; shift: the level of the
# front's anti-diagonal (the front runs through the cloud of the candidates' mean pairs, so that some are dominated and some are not);
# checked: the candidates at which tests/test_ehvi_reference.py's qualification conditions hold, chosen on the CPU; ld_diff: the
# worst float64-against-long-double difference over the case's candidates in units of scale, as tests/test_ehvi_reference.py measured
# it (value, members' values and gradient; the GPU tolerance is max(1e-10, 4 ld_diff) scale).
Case = collections.namedtuple("Case", "name seed E d n p F shift C checked ld_diff")

REF = (1.5, 1.4)
LENGTH_0, LENGTH_D = kp.LENGTH_0, kp.LENGTH_D

CASES = [
    Case("e1_d3_n20_p3_f0", 1, 1, 3, ((20, 20),), 3, 0, 0.0, 8, None, 4.1e-14),
    Case("e1_d3_n20_p0_f1", 2, 1, 3, ((20, 20),), 0, 1, -0.35, 8, None, 1.8e-14),
    Case("e1_d3_n20_p3_f2", 3, 1, 3, ((20, 20),), 3, 2, -0.7, 8, (1, 2, 3, 4, 5, 6, 7), 2.5e-15),
    Case("e1_d3_n20_p0_f63", 4, 1, 3, ((20, 20),), 0, 63, 0.0, 8, None, 2.8e-15),
    Case("e1_d3_n20_p3_f64", 5, 1, 3, ((20, 20),), 3, 64, 0.0, 8, None, 7.9e-15),
    Case("e1_d3_n20_p0_f65", 6, 1, 3, ((20, 20),), 0, 65, -0.25, 8, None, 1.5e-15),
    # n on both sides of tri_cols' 128-row switch and past 256 rows, shuffled over the roles: the members' chains do not line up
    Case("e3_d3_n20_130_300_p3_f300", 7, 3, 3, ((20, 130), (130, 300), (300, 20)), 3, 300, 0.0, 8, None, 1.7e-13),
    Case("e1_d10_n20_p3_f65", 8, 1, 10, ((20, 20),), 3, 65, 0.55, 8, None, 3.0e-16),   # the <12> gradient kernel
    Case("e3_d10_n20_p0_f2", 9, 3, 10, ((20, 20),) * 3, 0, 2, -0.1, 8, None, 2.1e-16),
]
ENSEMBLE = "e3_d3_n20_130_300_p3_f300"
# the believed-front rule: pending point 0's outcome joins member 0's front and a front point leaves; pending point 1's outcome is
# dominated under member 1; pending point 2 lies on an observation of 2.0 > r1 of every objective-1 GP: outside r
BELIEVED = Case("e2_d3_n20_p3_believed", 21, 2, 3, ((20, 20),) * 2, 3, 4, 0.0, 8, None, 6.0e-15)


# Every instantiation of the gradient kernel that CASES leaves out (padded dimensions 8, 16, 24, 32 with 2, 3, 4 and 0 padded
# coordinates), each with pending points and a front past one sweep; d20: past one 256-row stride at padded dimension 24; the wide
# ensemble: three strides of 256 rows and tri_cols' K slices of 64 and 128 at padded dimension 24 beside GPs of 20 rows (below its
# 128-row switch), the rows shuffled over the roles as in ENSEMBLE
WIDE_CASES = [
    Case("e1_d6_n20_p3_f65", 10, 1, 6, ((20, 20),), 3, 65, 0.0, 8, None, 6.6e-16),
    Case("e1_d13_n20_p3_f65", 11, 1, 13, ((20, 20),), 3, 65, 0.0, 8, None, 3.7e-16),
    Case("e1_d20_n300_20_p3_f65", 12, 1, 20, ((300, 20),), 3, 65, 0.0, 8, None, 1.8e-16),
    Case("e1_d32_n20_p3_f65", 13, 1, 32, ((20, 20),), 3, 65, 0.0, 8, None, 1.6e-16),
    Case("e3_d20_n20_300_520_p3_f65", 14, 3, 20, ((20, 300), (300, 520), (520, 20)), 3, 65, 0.0, 8, None, 3.6e-16),
]
ENSEMBLE_WIDE = "e3_d20_n20_300_520_p3_f65"


def case(name):
    return next(c for c in CASES + WIDE_CASES + [BELIEVED] if c.name == name)


def random_front(rng, F, shift, ref=REF):
    """F points along the anti-diagonal v = shift - u: u ascending, v descending, strictly inside ref"""
    u = np.sort(rng.uniform(-0.8, 0.8, size=F))
    v = np.sort(shift + rng.uniform(-0.8, 0.8, size=F))[::-1]
    if F <= 2:  # (one or two points in the middle of the cloud)
        u = np.array([-0.25] if F == 1 else [-0.2, 0.2][:F])
        v = shift - u
    assert F == 0 or (np.all(np.diff(u) > 0) and np.all(np.diff(v) < 0) and u[-1] < ref[0] and v[0] < ref[1])
    return np.ascontiguousarray(np.stack([u, v], axis=1)).reshape(-1, 2)


def make_problem(c):
    """the inputs of a case.  The GPs of a case observe nested point lists; the first pending point lies within 0.05 of candidate 0
    in every coordinate (conditioning on P moves that candidate by far more than the tolerance)."""
    rng = np.random.default_rng(9700 + c.seed)
    length = LENGTH_0 + LENGTH_D * math.sqrt(c.d)
    Xc = rng.uniform(0, 1, size=(max(max(row) for row in c.n), c.d))
    believed = c.name == BELIEVED.name
    gps = []
    for e in range(c.E):
        row = []
        for r in range(2):
            n = c.n[e][r]
            y = 0.3 * rng.normal(size=(n, 1))
            if believed and r == 0:
                y[0, 0] = 2.0
            f = 1.0 + 0.15 * ((e + 2 * r) % 4)
            hyper = np.array([1.3] + [length] * c.d) * f
            row.append(GP(MATERN if (e + r) % 2 == 0 else SE, hyper, Xc[:n].copy(), y, [1e-2 * f], ()))
        gps.append(row)
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    pending = rng.uniform(0, 1, size=(c.p, c.d))
    if c.p:
        pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=c.d)
    front = random_front(rng, c.F, c.shift)
    if believed:
        pending[2] = Xc[0]
        bases = [[cr.base_model(g, np.float64) for g in row] for row in gps]
        out = [[(float(cr.mean_at(b[0], pending)[j]), float(cr.mean_at(b[1], pending)[j])) for j in range(3)] for b in bases]
        a0, b0 = out[0][0]
        a1, b1 = out[1][1]
        # (a0 + 0.05, b0 + 0.05) leaves under member 0; (a1 - 0.05, b1 - 0.05) dominates member 1's outcome of pending point 1; two
        # far corners keep the front's ends
        pts = [(a0 + 0.05, b0 + 0.05), (a1 - 0.05, b1 - 0.05), (-0.9, 1.3), (1.4, -0.9)]
        front = _front_of(pts)
    checked = tuple(range(c.C)) if c.checked is None else tuple(c.checked)
    return Problem(c.name, gps, REF, front, points, pending, checked)


def _front_of(pts):
    pts = sorted(pts)
    out, best = [], math.inf
    for u, v in pts:
        if v < best:
            out.append((u, v))
            best = v
    return np.array(out, dtype=np.float64).reshape(-1, 2)


_WANT = {}


def expected(c, T=LD):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T)
    if key not in _WANT:
        p = make_problem(c)
        members = ensemble(p, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]
