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
import copy
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

# E >= 2 members and K >= 2 constraints TOGETHER, so that no [e][k] stride collapses (with E = 1 the term e K vanishes, with K = 1
# it equals e): row counts that differ per role and member, the padded-16 gradient kernel (d = 13), thresholds that are all
# distinct.  tests/test_cehvi_reference.py asserts that exchanging two constraint GPs within a member, the two members' GPs of one
# constraint, or two thresholds each moves the value by at least SWAP_MOVES scale at every checked candidate.
EDGE_TAUS = {2: (0.1, -0.05), 8: (0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55)}
MIXED2 = Case("m2_e2_k2_d13_n20_130_40_p3_f10", 541, 2, 2, 2, 13, ((20, 130, 40, 20), (130, 20, 20, 40)), 3, 10, EDGE_TAUS[2], 8,
              None, 2.6e-16)
MIXED3 = Case("m3_e2_k2_d13_n20_130_40_p3_f20", 542, 3, 2, 2, 13, ((20, 130, 40, 20, 130), (130, 20, 20, 40, 20)), 3, 20, EDGE_TAUS[2], 8,
              None, 9.7e-16)
MIXED2_K8 = Case("m2_e2_k8_d3_n20_p3_f10", 1543, 2, 2, 8, 3, _grid(2, 10, 20), 3, 10, EDGE_TAUS[8], 8, (0, 1, 2, 3, 4, 5, 6), 1.8e-15)
MIXED = {2: MIXED2, 3: MIXED3}
SWAP_MOVES = 1e-6       # (10^4 times the GPU bound)
FACTORS_APART = 1e-3
# The constraint roles' variance floors, E = 1, K = 2: constraint 1's GP is noise free and candidates 0 and 1 lie on two of its
# sampled points, whose observations are set by hand FLOOR_GAP below and above tau_1 -- there F_1 is exactly 1 and exactly 0 (the
# value floor DBL_MIN under a mean FLOOR_GAP from tau) and its gradient exactly 0 (the gradient floor 150 eps^2).  Candidate 1,
# whose value is 0, is the one candidate the qualification leaves out.
FLOOR2 = Case("m2_e1_k2_d3_n20_p3_f2_floor", 51, 2, 1, 2, 3, _grid(1, 4, 20), 3, 2, TAUS[2], 8, (0, 2, 3, 4, 5, 6, 7), 4.3e-15)
FLOOR3 = Case("m3_e1_k2_d3_n20_p3_f2_floor", 52, 3, 1, 2, 3, _grid(1, 5, 20), 3, 2, TAUS[2], 8, (0, 2, 3, 4, 5, 6, 7), 1.3e-14)
FLOOR = {2: FLOOR2, 3: FLOOR3}
FLOOR_ROWS, FLOOR_GAP = {2: (16, 12), 3: (5, 0)}, 0.2  # (rows whose float64 variance comes out under the floor)

EDGE_CASES = [MIXED2, MIXED3, MIXED2_K8, FLOOR2, FLOOR3]
ALL_CASES = CASES + [BELIEVED2, BELIEVED3] + EDGE_CASES


def case(name):
    return next(c for c in ALL_CASES if c.name == name)


def swapped(p):
    """the problems that part from p by ONE exchange, as (what, problem): two constraint GPs within a member (neighbours k, k + 1,
    cyclically), the two members' GPs of one constraint, two thresholds (neighbours, cyclically)"""
    M, K, out = p.M, len(p.taus), []
    pairs = [(k, (k + 1) % K) for k in range(K if K > 2 else 1)]
    for e in range(len(p.gps)):
        for a, b in pairs:
            gps = [list(row) for row in p.gps]
            gps[e][M + a], gps[e][M + b] = gps[e][M + b], gps[e][M + a]
            out.append(("member %d: constraint GPs %d and %d" % (e, a, b), p._replace(gps=gps)))
    for k in range(K):
        gps = [list(row) for row in p.gps]
        gps[0][M + k], gps[1][M + k] = gps[1][M + k], gps[0][M + k]
        out.append(("constraint %d: the members' GPs" % k, p._replace(gps=gps)))
    for a, b in pairs:
        taus = list(p.taus)
        taus[a], taus[b] = taus[b], taus[a]
        out.append(("thresholds %d and %d" % (a, b), p._replace(taus=taus)))
    return out


def make_problem(c):
    """the inputs of a case.  The GPs of a case observe nested point lists; the first pending point lies within 0.05 of candidate 0
    in every coordinate (conditioning on P moves that candidate by far more than the tolerance).  The constraints' observations have
    the objectives' spread of 0.3 about 0."""
    rng = np.random.default_rng(12400 + c.seed)
    length = LENGTH_0 + LENGTH_D * math.sqrt(c.d)
    Xc = rng.uniform(0, 1, size=(max(max(row) for row in c.n), c.d))
    believed = c.name in (BELIEVED2.name, BELIEVED3.name)
    floor = c.name in (FLOOR2.name, FLOOR3.name)
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
            noise = 1e-2 * f
            if floor and r == c.M:
                y[FLOOR_ROWS[c.M][0], 0], y[FLOOR_ROWS[c.M][1], 0], noise = c.tau[0] - FLOOR_GAP, c.tau[0] + FLOOR_GAP, 0.0
            row.append(GP(MATERN if (e + r) % 2 == 0 else SE, hyper, Xc[:n].copy(), y, [noise], ()))
        gps.append(row)
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    if floor:
        points[0], points[1] = Xc[FLOOR_ROWS[c.M][0]], Xc[FLOOR_ROWS[c.M][1]]
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


# A belief that CHANGES along a greedy batch, E = 2, K = 1, tau = 0: member 0's constraint GP observes values about -0.6 (it believes
# every point feasible); member 1's observes CHANGING_SLOPE (0.5 - x_0) under length scales that span the cube, so that its mean
# falls through tau at x_0 = 0.5 -- it believes a point infeasible to the left and feasible to the right.  The one pending point
# lies on the left, the starts in two clusters, one on each side.  Each pick's mask word is written at another relative index and
# must be worked out anew: a device that kept the pending point's word for every pick computes `stale`'s value.
CHANGING = {2: Case("m2_e2_k1_d3_n20_p1_f3_changing", 71, 2, 2, 1, 3, _grid(2, 3, 20), 1, 3, (0.0,), 8, None, 0.0),
            3: Case("m3_e2_k1_d3_n20_p1_f4_changing", 72, 3, 2, 1, 3, _grid(2, 4, 20), 1, 4, (0.0,), 8, None, 0.0)}
CHANGING_SLOPE, CHANGING_Q = 3.0, {2: 4, 3: 3}


def changing_problem(M):
    """(problem, starts [12][3]) of CHANGING[M]"""
    c = CHANGING[M]
    p = make_problem(c._replace(name=BELIEVED[M].name))  # (BELIEVED's front and observations at the three shared points)
    rng = np.random.default_rng(12400 + c.seed)
    gps = []
    for e, row in enumerate(p.gps):
        con = row[M]
        X = np.asarray(con.X)
        if e == 0:
            y = -0.6 + 0.05 * rng.normal(size=(len(X), 1))
            gps.append(list(row[:M]) + [GP(con.cov_type, con.hyper, con.X, y, con.noise, ())])
        else:
            y = CHANGING_SLOPE * (0.5 - X[:, :1]) + 0.01 * rng.normal(size=(len(X), 1))
            gps.append(list(row[:M]) + [GP(SE, np.array([2.0, 1.5, 3.0, 3.0]), con.X, y, [1e-3], ())])
    pending = np.array([[0.2, 0.5, 0.5]])
    starts = np.vstack([rng.uniform([0.08, 0.1, 0.1], [0.32, 0.9, 0.9], size=(6, 3)), rng.uniform([0.68, 0.1, 0.1], [0.92, 0.9, 0.9], size=(6, 3))])
    return p._replace(name=c.name, gps=gps, pending=pending), starts


def remasked(m, mask, front):
    """member m under ANOTHER believed-feasibility mask [p] than its own, from the caller's front: what its front would be under
    the other decisions"""
    n = copy.copy(m)
    n.mask = np.asarray(mask, dtype=bool)
    n.offered = [o for o, ok in zip(n.outcomes, n.mask) if ok]
    n.front, n.log = (hr.believed_front if m.M == 2 else h3.believed_front)(front, n.offered, n.ref, n.T)
    n.table = h3.box_table(n.front) if m.M == 3 else None
    return n


# Sixty-four pending points under a MIXED mask, E = 5, K = 1, tau = 0: cehvi_believed_kernel over 5 x 64 threads (a second
# workgroup) with a mask row of 64 words, and the front kernels' masked `continue` in front of evictions past index 64 and, for
# M = 3, of a table rebuild.  The pending points lie on the line x_0 = 0.1 .. 0.9 through the middle of the cube and every GP
# observes about 20 points scattered 0.02 about that line: objective 1 rises and objective 2 falls along it, both carry a common
# wave g (where g < 0 the believed outcome lies below the caller's front u + v = 0 and evicts the points about it, where g > 0 it
# is dominated; on g's rising flanks an outcome dominates the ones that follow it); each member's constraint observes a wave of
# another period whose phase moves with the member, so that the members skip different outcomes.  Not among ALL_CASES (p = 64).
MASKED = {2: Case("m2_e5_k1_d3_n20_p64_f200_masked", 81, 2, 5, 1, 3, ((20, 19, 21), (21, 20, 19), (19, 21, 20), (20, 21, 19), (19, 20, 21)),
                  64, 200, (0.0,), 8, None, 8.3e-15),
          3: Case("m3_e5_k1_d3_n20_p64_f100_masked", 82, 3, 5, 1, 3, ((20, 19, 21, 20), (21, 20, 19, 21), (19, 21, 20, 19), (20, 21, 19, 20),
                  (19, 20, 21, 21)), 64, 100, (0.0,), 8, None, 2.1e-14)}


MASKED_WAVE = {2: 0.06, 3: 0.12}  # (M = 2: the members' fronts keep 130 to 160 of the 200 points, three sweeps of strips)


def masked_problem(M):
    c = MASKED[M]
    rng = np.random.default_rng(12400 + c.seed)
    wave = lambda x0, e: MASKED_WAVE[M] * np.sin(2.0 * np.pi * 4.0 * x0 + 0.3 * e)  # noqa: E731
    gps = []
    for e in range(c.E):
        row = []
        for r in range(M + 1):
            n = c.n[e][r]
            X = np.stack([np.linspace(0.02, 0.98, n) + 0.01 * rng.normal(size=n), 0.5 + 0.02 * rng.normal(size=n),
                          0.5 + 0.02 * rng.normal(size=n)], axis=1)
            x0 = X[:, 0]
            if r == 0:
                y = (x0 - 0.5) + wave(x0, e)
            elif r == 1:
                y = -(x0 - 0.5) + wave(x0, e)
            elif r < M:
                y = 0.3 * (x0 - 0.5) + 0.02 * np.cos(2.0 * np.pi * 2.0 * x0 + e)  # (rising, so that an outcome can dominate a later one)
            else:
                y = 0.5 * np.sin(2.0 * np.pi * 2.5 * x0 + 2.0 * np.pi * e / c.E)
            f = 1.0 + 0.1 * ((e + 2 * r) % 4)
            row.append(GP(MATERN if (e + r) % 2 == 0 else SE, np.array([1.0 * f, 0.1 * f, 1.0, 1.0]), X, y.reshape(-1, 1), [1e-3 * f], ()))
        gps.append(row)
    pending = np.full((c.p, 3), 0.5)
    pending[:, 0] = np.linspace(0.1, 0.9, c.p)
    u = np.linspace(-0.55, 0.55, c.F) + rng.uniform(-0.001, 0.001, size=c.F)
    if M == 2:
        front = np.stack([u, -u], axis=1)
    else:
        front = h3.canonical(np.stack([u, -u, rng.uniform(-0.3, 0.3, size=c.F)], axis=1))
    points = np.stack([rng.uniform(0.1, 0.9, size=c.C), rng.uniform(0.2, 0.8, size=c.C), rng.uniform(0.2, 0.8, size=c.C)], axis=1)
    return Problem(c.name, M, gps, list(c.tau), REF2 if M == 2 else REF3, np.ascontiguousarray(front), points, pending, tuple(range(c.C)))


def dominates(a, b):
    return all(float(x) <= float(y) for x, y in zip(a, b))


def mask_effects(m, caller_front):
    """what member m's mask does to its front, for the qualification of MASKED: (the offered outcomes that evict a front point whose
    index, in the front as they meet it, is 64 or more; the skipped outcomes j that would have joined the front as it stood when
    their turn came and that dominate an outcome offered after them)"""
    rule = hr.believed_front if m.M == 2 else h3.believed_front
    evicting, missed = [], []
    offered_before = []
    for j, (o, ok) in enumerate(zip(m.outcomes, m.mask)):
        before, _ = rule(caller_front, offered_before, m.ref, m.T)
        before = np.asarray(before, dtype=np.float64).reshape(-1, m.M)
        joins = all(float(o[k]) < m.ref[k] for k in range(m.M)) and not any(dominates(q, o) for q in before)
        if ok:
            if joins and any(dominates(o, q) for q in before[64:]):
                evicting.append(j)
            offered_before.append(o)
        elif joins and any(m.mask[t] and dominates(o, m.outcomes[t]) for t in range(j + 1, len(m.outcomes))):
            missed.append(j)
    return evicting, missed


# E (M + K) = 1024 exactly, the limit: 128 members of 2 + 6 GPs, the hyper-parameters moving with the member and the role so that
# no two members agree; six distinct thresholds.  Not one of ALL_CASES (C = 4, p = 1): tests/test_cehvi_reference.py and
# tests/test_log_ehvi_reference.py measure its float64-against-long-double differences for the plain and the log form.
LIMIT = Case("m2_e128_k6_d2_n6_p1_f2_limit", 61, 2, 128, 6, 2, _grid(128, 8, 6), 1, 2, (0.25, 0.3, 0.35, 0.4, 0.45, 0.5), 4, None, 2.9e-14)
LIMIT_MEMBERS = (0, 63, 127)


def limit_problem(c=LIMIT):
    rng = np.random.default_rng(12400 + c.seed)
    X = rng.uniform(0, 1, size=(c.n[0][0], c.d))
    ys = [0.3 * rng.normal(size=(len(X), 1)) for _ in range(c.M + c.K)]
    gps = [[GP(MATERN if (e + r) % 2 == 0 else SE, np.array([1.0 + 0.1 * r + 0.003 * e, 0.35 + 0.001 * e, 0.6 - 0.0007 * e]), X.copy(),
               ys[r], [1e-2], ()) for r in range(c.M + c.K)] for e in range(c.E)]
    front = np.array([(-0.4, 0.2), (0.1, -0.3)])
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    pending = rng.uniform(0.1, 0.9, size=(c.p, c.d))
    return Problem(c.name, c.M, gps, list(c.tau), REF2, front, points, pending, tuple(range(c.C)))


_WANT = {}


def expected(c, T=LD):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T)
    if key not in _WANT:
        if c.name == LIMIT.name:
            p = limit_problem(c)
        elif c.name in (MASKED[2].name, MASKED[3].name):
            p = masked_problem(c.M)
        else:
            p = make_problem(c)
        members = ensemble(p, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]
