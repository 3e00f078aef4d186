"""The constrained expected hypervolume improvement for two and for three objectives with pending points, averaged over an
ensemble, restated on the CPU (the checker of tests/test_gpu_cehvi.py) in np.longdouble or float64, on top of
tests/ehvi_reference.py (strips, the two-objective believed-front rule), tests/ehvi3_reference.py (box_sum, box_table, the
three-objective believed-front rule) and tests/cei1_reference.py (base_model, conditioned, mean_at, moments, feasibility), all
imported unchanged: the (N + p)^2 system of every GP is factored in full and nothing of the device's extension appears.

Minimisation.  Member e is M + K GPs: roles 0 .. M - 1 the objectives, role M - 1 + k constraint k = 1 .. K, satisfied where
c_k(x) <= tau_k.  With mu, var the posterior mean and the conditioned latent variance of the GP in question at x:
    H_e   the member's expected hypervolume improvement: ehvi_reference.strips (M = 2) or ehvi3_reference.box_sum (M = 3), with
          its 2 M coefficients dH/dmu_r, dH/dvar_r; grad H_e = sum_r dH/dmu_r grad mu_r + dH/dvar_r grad var_r
    F_k   = Phi((tau_k - mu) / sigma) and its gradient: cei1_reference.feasibility
    A_e   = H_e F_1 ... F_K,  grad A_e by the product rule;  value = (A_0 + ... + A_{E-1}) / E
THE BELIEVED-FEASIBLE FRONT RULE, in plain Python (Member.__init__): the caller's front is that of the feasible observations;
pending point P_j is believed feasible under member e when mu_{e,k}(P_j) <= tau_k for every k; for j = 0, 1, ... in turn the
believed outcome (mu_{e,1}(P_j), ..., mu_{e,M}(P_j)) is offered to member e's own front under the unconstrained join rule ONLY
where member e believes P_j feasible -- a believed-infeasible point is skipped before the join rule and leaves the front as it was.
Every GP's variance is conditioned on every pending point, whichever way the belief falls.
scale = max(1, |r_k|, max |y|, sqrt(alpha)) over the member's M + K GPs; an ensemble takes its largest member scale.
"""
import collections
import math

import numpy as np

import cei1_reference as cr
import ehvi3_reference as h3
import ehvi_reference as hr
import kg1_pending_reference as kp
import kg1_reference as kr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN
GP = cr.GP

Problem = collections.namedtuple("Problem", "name M gps taus ref front points pending checked")
# factors [E][1 + K]: H_e, F_{e,1} .. F_{e,K}; members [E]: A_e; means [E][M]
Result = collections.namedtuple("Result", "value grad factors members scale means")


def believed_feasible(constraint_bases, P, taus):
    """the pending points a member (its K constraint base models) believes feasible: a boolean mask [p], and the constraint means
    [K][p] it was taken from"""
    ok = np.ones(len(P), dtype=bool)
    means = []
    for base, tau in zip(constraint_bases, taus):
        mu = cr.mean_at(base, P) if len(P) else np.zeros(0, dtype=base.T)
        means.append(mu)
        for j, m in enumerate(mu):
            if not m <= base.T(tau):
                ok[j] = False
    return ok, means


class Member(object):
    """one member's M + K GPs conditioned on P, its believed-feasible mask and its own front, factored once for every candidate"""

    def __init__(self, gps, M, taus, ref, front, P, T=LD):
        self.T, self.M, self.gps, self.taus = T, M, gps, [float(t) for t in taus]
        self.K = len(self.taus)
        assert len(gps) == M + self.K and M in (2, 3)
        self.ref = tuple(float(r) for r in ref)
        self.P = np.asarray(P, dtype=np.float64).reshape(-1, np.asarray(gps[0].X).shape[1])
        self.bases = [cr.base_model(g, T) for g in gps]
        self.models = [cr.conditioned(b, self.P) for b in self.bases]  # (all of them, whichever way the belief falls)
        # the rule: which pending points the member believes feasible ...
        self.mask, self.constraint_means = believed_feasible(self.bases[M:], self.P, self.taus)
        # ... the believed outcomes of all of them ...
        if len(self.P):
            self.outcomes = list(zip(*[cr.mean_at(b, self.P) for b in self.bases[:M]]))
        else:
            self.outcomes = []
        # ... and only the believed-feasible ones are offered to the front, in the order of j
        self.offered = [o for o, ok in zip(self.outcomes, self.mask) if ok]
        rule = hr.believed_front if M == 2 else h3.believed_front
        self.front, self.log = rule(front, self.offered, self.ref, T)
        self.table = h3.box_table(self.front) if M == 3 else None
        self.scale = (hr.member_scale if M == 2 else h3.member_scale)(gps, self.ref)

    def evaluate(self, x):
        """(A_e, grad A_e, [H_e, F_1 .. F_K], (mu_1 .. mu_M)) at x"""
        T, M = self.T, self.M
        mo = [cr.moments(m, b, x) for m, b in zip(self.models[:M], self.bases[:M])]
        if M == 2:
            H, c = hr.strips(mo[0][0], mo[0][1], mo[1][0], mo[1][1], self.front, self.ref, T)
        else:
            H, c = h3.box_sum([(m[0], m[1]) for m in mo], self.front, self.ref, T, self.table)
        gH = sum(c[2 * r] * mo[r][2] + c[2 * r + 1] * mo[r][3] for r in range(M))
        vals, grads = [H], [gH + np.zeros(len(x), dtype=T)]
        for model, base, tau in zip(self.models[M:], self.bases[M:], self.taus):
            F, gF = cr.feasibility(model, base, x, tau)
            vals.append(F)
            grads.append(gF)
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
        return a, grad, vals, tuple(m[0] for m in mo)


def ensemble(p, T=LD, pending=None, front=None, constraints=True):
    """the members of a problem (pending / front: others than the problem's; constraints=False: the objective GPs alone)"""
    P = p.pending if pending is None else pending
    f = p.front if front is None else front
    K = len(p.taus) if constraints else 0
    return [Member(g[:p.M + K], p.M, p.taus[:K], p.ref, f, P, T) for g in p.gps]


def evaluate(members, x):
    T = members[0].T
    value, grad, factors, vals, means = T(0), np.zeros(len(x), dtype=T), [], [], []
    for m in members:
        a, g, f, mu = m.evaluate(x)
        value, grad = value + a, grad + g
        factors.append(f)
        vals.append(a)
        means.append(mu)
    n = T(len(members))
    return Result(value / n, grad / n, factors, vals, max(m.scale for m in members), means)


def host_value(factors):
    """the documented rule on the host in float64: factors [E][1 + K][C] -> value [C], every member's product formed left to right,
    the members added in member order and divided once"""
    E, G, n = factors.shape
    out = np.zeros(n)
    for i in range(n):
        total = 0.0
        for e in range(E):
            a = float(factors[e, 0, i])
            for k in range(1, G):
                a = a * float(factors[e, k, i])
            total = a if e == 0 else total + a
        out[i] = total / float(E)
    return out


def join_margin(front, offered, ref, M):
    """the smallest distance, over the joins of `offered` in order, between a coordinate of an outcome and the same coordinate of a
    front point it is compared with (the front as the outcome meets it) or of the reference point: no decision of the join rule
    within that distance of flipping"""
    rule = hr.believed_front if M == 2 else h3.believed_front
    worst = math.inf
    for j, o in enumerate(offered):
        before, _ = rule(front, offered[:j], ref, np.float64)
        o = [float(x) for x in o]
        worst = min([worst] + [abs(o[k] - float(ref[k])) for k in range(M)] +
                    [abs(o[k] - float(q[k])) for q in np.asarray(before, dtype=np.float64).reshape(-1, M) for k in range(M)])
    return worst


# ---- the cases of tests/test_gpu_cehvi.py (tests/test_cehvi_reference.py qualifies them on the CPU) ----
# Case: M objectives, E members of M + K GPs in dim d; n[e][role] observations; p pending points; F front points; tau [K]; C
# candidates; checked: the candidates at which tests/test_cehvi_reference.py's qualification conditions hold (None: all C), chosen
# on the CPU; ld_diff: the worst float64-against-long-double difference over the case's candidates in units of scale, as
# tests/test_cehvi_reference.py measured it (value, factors, members' values and gradient; the GPU tolerance is max(1e-10, 4 ld_diff)
# scale).
Case = collections.namedtuple("Case", "name seed M E K d n p F tau C checked ld_diff")

REF2, REF3 = hr.REF, h3.REF
LENGTH_0, LENGTH_D = kp.LENGTH_0, kp.LENGTH_D
TAUS = {1: (0.0,), 2: (0.1, 0.0), 8: (0.3,) * 8}


def _grid(E, G, n):
    return tuple(tuple(n for _ in range(G)) for _ in range(E))


def _small(M, K, F, seed, checked, ld_diff):
    return Case("m%d_e1_k%d_d3_n20_p3_f%d" % (M, K, F), seed, M, 1, K, 3, _grid(1, M + K, 20), 3, F, TAUS[K], 8, checked, ld_diff)


CASES = [
    # K in {1, 2, 8} against an empty front, a front of two points and one past a sweep of 64 strips (M = 2) ...
    _small(2, 1, 0, 1, None, 1.4e-14),
    _small(2, 1, 2, 2, (1, 2, 3, 4, 5, 6, 7), 1.2e-15),
    _small(2, 1, 65, 3, (0, 1, 2, 3, 5, 6, 7), 1.0e-15),
    _small(2, 2, 0, 4, None, 4.6e-15),
    _small(2, 2, 2, 105, None, 2.3e-15),
    _small(2, 2, 65, 6, None, 3.5e-15),
    _small(2, 8, 0, 7, (0, 1, 2, 3, 4, 6, 7), 1.3e-14),
    _small(2, 8, 2, 108, None, 2.0e-15),
    _small(2, 8, 65, 209, (0, 1, 2, 4, 5, 6, 7), 3.2e-15),
    # ... and a table of 20 points (M = 3)
    _small(3, 1, 0, 11, None, 2.6e-14),
    _small(3, 1, 2, 12, None, 3.2e-14),
    _small(3, 1, 20, 13, (1, 2, 3, 4, 5, 6, 7), 2.3e-14),
    _small(3, 2, 0, 14, None, 1.5e-14),
    _small(3, 2, 2, 15, (0, 2, 3, 4, 5, 6, 7), 4.9e-14),
    _small(3, 2, 20, 16, None, 1.7e-15),
    _small(3, 8, 0, 17, None, 4.5e-14),
    _small(3, 8, 2, 18, (0, 2, 3, 4, 5, 6, 7), 2.8e-14),
    _small(3, 8, 20, 19, None, 5.2e-15),
    # n on both sides of tri_cols' 128-row switch and past 256 rows, shuffled over objective AND constraint roles: the chains of a
    # member's sub-members do not line up, nor do those of one role across the members
    Case("m2_e3_k1_d3_n20_130_300_p3_f65", 21, 2, 3, 1, 3, ((20, 130, 300), (130, 300, 20), (300, 20, 130)), 3, 65, TAUS[1], 8,
         (0, 1, 2, 3, 5, 6, 7), 1.2e-13),
    Case("m3_e3_k1_d3_n20_130_300_p3_f20", 122, 3, 3, 1, 3, ((20, 130, 300, 130), (130, 300, 20, 300), (300, 20, 130, 20)), 3, 20,
         TAUS[1], 8, None, 1.9e-13),
    # the <12> gradient kernel
    Case("m2_e1_k1_d10_n20_p3_f2", 23, 2, 1, 1, 10, _grid(1, 3, 20), 3, 2, TAUS[1], 8, (0, 1, 3, 4, 5, 6, 7), 2.7e-16),
]
ENSEMBLE2, ENSEMBLE3 = "m2_e3_k1_d3_n20_130_300_p3_f65", "m3_e3_k1_d3_n20_130_300_p3_f20"
# The believed-feasible front rule, E = 2, K = 1, tau = 0, three pending points that lie on sampled points all GPs share, where the
# observations are set by hand (make_problem): pending point 0 is believed feasible under member 0 and its outcome joins member 0's
# front (the front point at the origin leaves); pending point 1 is believed INFEASIBLE under member 1, where its outcome would have
# joined and evicted the origin; pending point 2 is believed feasible under both members and dominated.
BELIEVED2 = Case("m2_e2_k1_d3_n20_p3_believed", 31, 2, 2, 1, 3, _grid(2, 3, 20), 3, 3, (0.0,), 8, None, 2.1e-15)
BELIEVED3 = Case("m3_e2_k1_d3_n20_p3_believed", 32, 3, 2, 1, 3, _grid(2, 4, 20), 3, 4, (0.0,), 8, None, 5.5e-15)
BELIEVED = {2: BELIEVED2, 3: BELIEVED3}
MARGIN = 0.05
# objective observations at the three shared points per member (every objective the same), and the constraint's
_BELIEVED_OBJECTIVE = ((-0.3, 0.7, 0.5), (0.25, -0.4, 0.6))
_BELIEVED_CONSTRAINT = ((-0.5, -0.5, -0.5), (-0.5, 0.5, -0.5))

ALL_CASES = CASES + [BELIEVED2, BELIEVED3]


def case(name):
    return next(c for c in ALL_CASES if c.name == name)


def make_problem(c):
    """the inputs of a case.  The GPs of a case observe nested point lists; the first pending point lies within 0.05 of candidate 0
    in every coordinate (conditioning on P moves that candidate by far more than the tolerance).  The constraints' observations have
    the objectives' spread of 0.3 about 0."""
    rng = np.random.default_rng(12400 + c.seed)
    length = LENGTH_0 + LENGTH_D * math.sqrt(c.d)
    Xc = rng.uniform(0, 1, size=(max(max(row) for row in c.n), c.d))
    believed = c.name in (BELIEVED2.name, BELIEVED3.name)
    gps = []
    for e in range(c.E):
        row = []
        for r in range(c.M + c.K):
            n = c.n[e][r]
            y = 0.3 * rng.normal(size=(n, 1))
            if believed:
                y[:3, 0] = _BELIEVED_OBJECTIVE[e] if r < c.M else _BELIEVED_CONSTRAINT[e]
            f = 1.0 + 0.15 * ((e + 2 * r) % 4)
            hyper = np.array([1.3] + [length] * c.d) * f
            row.append(GP(MATERN if (e + r) % 2 == 0 else SE, hyper, Xc[:n].copy(), y, [1e-2 * f], ()))
        gps.append(row)
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    pending = rng.uniform(0, 1, size=(c.p, c.d))
    if c.p:
        pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=c.d)
    if believed:
        pending = Xc[:3].copy()
        corners = [(-0.9, 1.3), (0.0, 0.0), (1.4, -0.9)] if c.M == 2 else [(-0.9, 1.3, 1.2), (0.0, 0.0, 0.0), (1.4, -0.9, 1.2),
                                                                            (1.4, 1.3, -0.9)]
        front = np.array(sorted(corners), dtype=np.float64) if c.M == 2 else h3.canonical(np.array(corners, dtype=np.float64))
    elif c.M == 2:
        front = hr.random_front(rng, c.F, 0.0 if c.F > 2 else -0.5)
    else:
        front = h3.random_front(rng, c.F)
    checked = tuple(range(c.C)) if c.checked is None else tuple(c.checked)
    return Problem(c.name, c.M, gps, list(c.tau), REF2 if c.M == 2 else REF3, np.ascontiguousarray(front), points, pending, checked)


_WANT = {}


def expected(c, T=LD):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T)
    if key not in _WANT:
        p = make_problem(c)
        members = ensemble(p, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]
