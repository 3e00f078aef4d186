"""The three-objective expected hypervolume improvement with pending points, averaged over an ensemble, restated on the CPU (the
checker of tests/test_gpu_ehvi3.py) in np.longdouble or float64, on top of tests/kg1_reference.py (Model),
tests/kg1_pending_reference.py (PendingModel), tests/cei1_reference.py (moments, mean_at, base_model, conditioned) and
tests/ehvi_reference.py (psi), all imported unchanged: the (N + p)^2 system of every GP is factored in full and nothing of the
device's extension appears.

Minimisation.  Member e is three GPs, one per objective; r = (r1, r2, r3) the reference point; the front n >= 0 mutually
non-dominated points (u_i, v_i, w_i) strictly inside r in the canonical order: w ascending, ties by u, then by v.  w_0 = -infinity,
w_{n+1} = r3.  Between w_k and w_{k+1} the non-dominated cross-section is the two-dimensional non-dominated region of the first k
points' (u, v) projections, so with psi of ehvi_reference.py
    S2_k = sum over the strips of the staircase of points 1 .. k in (u, v) of [psi_1(right) - psi_1(left)] psi_2(height)
    A_e  = max(0, sum_{k = 0 .. n} S2_k [psi_3(w_{k+1}) - psi_3(w_k)]),  the boxes added slab by slab, a slab's strips in ascending u
    grad A_e through the six coefficients dA/dmu_k, dA/dvar_k; 0 where the sum is not positive
    value = (A_0 + ... + A_{E-1}) / E
The table (box_table) names a box by four indices into the member's edge lists -- 0: -infinity, 1 .. n: the points, n + 1: the
reference point -- the u edge on its left, the u edge on its right, the v edge of its height and its slab k, slab-major.
The believed-front rule: the believed outcome (mu_1, mu_2, mu_3)(P_j) of pending point j joins the member's own front, in the order
of j, when it is finite, strictly inside r and no front point is <= it in all three objectives; the front points >= it in all three
leave; the canonical order is kept.
scale = max(1, |r1|, |r2|, |r3|, max |y|, sqrt(alpha)) over the member's three GPs; an ensemble takes its largest member scale.
"""
import collections
import math

import numpy as np

import cei1_reference as cr
import ehvi_reference as hr
import kg1_pending_reference as kp
import kg1_reference as kr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN
GP = cr.GP
psi = hr.psi

Problem = collections.namedtuple("Problem", "name gps ref front points pending checked")
Result = collections.namedtuple("Result", "value grad members scale means")


def canonical(points):
    """points [n][3] in the canonical order"""
    f = np.asarray(points).reshape(-1, 3)
    return f[np.lexsort((f[:, 1], f[:, 0], f[:, 2]))]


def staircase(front, k):
    """the indices (into front) of the staircase of the first k points' (u, v) projections, in ascending u: the projections no
    other is <= to in both; of equal projections the first"""
    order = sorted(range(k), key=lambda i: (front[i][0], front[i][1], i))
    out, best = [], None
    for i in order:
        if best is None or front[i][1] < best:
            out.append(i)
            best = front[i][1]
    return out


def box_table(front):
    """the member's boxes [B][4] (left u edge, right u edge, v edge of the height, slab), slab-major, strips in ascending u"""
    n = len(front)
    boxes = []
    for k in range(n + 1):
        st = staircase(front, k)
        m = len(st)
        for s in range(m + 1):
            left = 0 if s == 0 else st[s - 1] + 1
            right = n + 1 if s == m else st[s] + 1
            height = n + 1 if s == 0 else left
            boxes.append((left, right, height, k))
    return np.array(boxes, dtype=np.int64).reshape(-1, 4)


def box_sum(moments3, front, ref, T=LD, table=None):
    """(A, [dA/dmu_1, dA/dvar_1, dA/dmu_2, dA/dvar_2, dA/dmu_3, dA/dvar_3]) of one member from its three (mu, var), its front
    [n][3] and r, the boxes added in the table's order"""
    front = np.asarray(front, dtype=T).reshape(-1, 3)
    n = len(front)
    table = box_table(front) if table is None else table
    e = np.zeros((3, 3, n + 2), dtype=T)  # [objective][psi, d / d mu, d / d var][edge]; edge 0: psi(-infinity) = 0
    for k in range(3):
        mu, var = moments3[k]
        for i in range(1, n + 2):
            e[k, :, i] = psi(front[i - 1, k] if i <= n else ref[k], mu, var, T)
    uL, uR, vH, sl = table[:, 0], table[:, 1], table[:, 2], table[:, 3]
    P = e[0][:, uR] - e[0][:, uL]
    Q = e[1][:, vH]
    W = e[2][:, sl + 1] - e[2][:, sl]
    terms = [P[0] * Q[0] * W[0], P[1] * Q[0] * W[0], P[2] * Q[0] * W[0], P[0] * Q[1] * W[0], P[0] * Q[2] * W[0], P[0] * Q[0] * W[1],
             P[0] * Q[0] * W[2]]
    sums = []
    for t in terms:
        acc = T(0)
        for x in t:
            acc = acc + x
        sums.append(acc)
    total, c = sums[0], sums[1:]
    if not total > 0:
        return T(0), [T(0)] * 6
    return total, c


def believed_front(front, outcomes, ref, T=LD):
    """(the front after the believed outcomes [p][3] have joined in order, a log with one entry per outcome: ("outside", 0, False),
    ("dominated", 0, False) or ("joined", the number of front points that left, whether a front point that stays ties it in w))"""
    f = [tuple(T(x) for x in row) for row in np.asarray(front, dtype=T).reshape(-1, 3)]
    log = []
    for o in outcomes:
        o = tuple(T(x) for x in o)
        if not (all(np.isfinite(x) for x in o) and all(o[k] < T(ref[k]) for k in range(3))):
            log.append(("outside", 0, False))
            continue
        if any(all(q[k] <= o[k] for k in range(3)) for q in f):
            log.append(("dominated", 0, False))
            continue
        kept = [q for q in f if not all(q[k] >= o[k] for k in range(3))]
        log.append(("joined", len(f) - len(kept), any(q[2] == o[2] for q in kept)))
        f = sorted(kept + [o], key=lambda q: (q[2], q[0], q[1]))
    return np.array(f, dtype=T).reshape(-1, 3), log


def member_scale(gps, ref):
    return max([1.0] + [abs(float(r)) for r in ref] +
               [float(np.max(np.abs(np.asarray(g.y, dtype=np.float64)))) for g in gps] +
               [math.sqrt(float(np.asarray(g.hyper).ravel()[0])) for g in gps])


class Member(object):
    """one member's three GPs conditioned on P and its own front with its table, factored once for every candidate"""

    def __init__(self, gps, ref, front, P, T=LD):
        self.T, self.gps, self.ref = T, gps, tuple(float(r) for r in ref)
        self.P = np.asarray(P, dtype=np.float64).reshape(-1, np.asarray(gps[0].X).shape[1])
        self.bases = [cr.base_model(g, T) for g in gps]
        self.models = [cr.conditioned(b, self.P) for b in self.bases]
        if len(self.P):
            self.outcomes = list(zip(*[cr.mean_at(b, self.P) for b in self.bases]))
        else:
            self.outcomes = []
        self.front, self.log = believed_front(front, self.outcomes, self.ref, T)
        self.table = box_table(self.front)
        self.scale = member_scale(gps, ref)

    def evaluate(self, x):
        """(A_e, grad A_e, (mu_1, mu_2, mu_3)) at x"""
        mo = [cr.moments(m, b, x) for m, b in zip(self.models, self.bases)]
        a, c = box_sum([(m[0], m[1]) for m in mo], self.front, self.ref, self.T, self.table)
        grad = sum(c[2 * k] * mo[k][2] + c[2 * k + 1] * mo[k][3] for k in range(3))
        return a, grad, tuple(m[0] for m in mo)


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


# ---- the cases of tests/test_gpu_ehvi3.py ----
# Case: E members of three GPs in dim d; n[e][objective] observations; p pending points; F front points of the kind `kind`; B: the
# boxes of the caller's front; ld_diff: the worst float64-against-long-double difference over the case's candidates in units of
# scale, as tests/test_ehvi3_reference.py measured it (value, members' values and gradient; the GPU tolerance is max(1e-10, 4
# ld_diff) scale).
Case = collections.namedtuple("Case", "name seed E d n p F kind B C ld_diff")

REF = (1.5, 1.4, 1.3)
LENGTH_0, LENGTH_D = kp.LENGTH_0, kp.LENGTH_D


def _grid(E, n):
    return tuple((n, n, n) for _ in range(E))


CASES = [
    Case("e1_d3_n20_p0_f0", 1, 1, 3, _grid(1, 20), 0, 0, "random", 1, 8, 2.7e-14),
    Case("e1_d3_n20_p3_f1", 2, 1, 3, _grid(1, 20), 3, 1, "random", 3, 8, 2.0e-14),
    Case("e1_d3_n20_p0_f5", 3, 1, 3, _grid(1, 20), 0, 5, "random", None, 8, 1.1e-14),
    # B = (F + 1)(F + 2) / 2 on either side of one wavefront's sweep of 64 boxes and of the workgroup's sweep of 256
    Case("e1_d3_n20_p0_stair9", 4, 1, 3, _grid(1, 20), 0, 9, "stair", 55, 8, 1.8e-14),
    Case("e1_d3_n20_p3_stair10", 5, 1, 3, _grid(1, 20), 3, 10, "stair", 66, 8, 2.3e-14),
    Case("e1_d3_n20_p0_stair21", 6, 1, 3, _grid(1, 20), 0, 21, "stair", 253, 8, 7.0e-15),
    Case("e1_d3_n20_p3_stair22", 7, 1, 3, _grid(1, 20), 3, 22, "stair", 276, 8, 3.8e-14),
    # one surviving point per slab: 2 F + 1 boxes in F + 1 slabs
    Case("e1_d3_n20_p0_descend70", 8, 1, 3, _grid(1, 20), 0, 70, "descend", 141, 8, 1.2e-14),
    # F - 1 slabs of zero thickness
    Case("e1_d3_n20_p0_flat12", 9, 1, 3, _grid(1, 20), 0, 12, "flat", 91, 8, 1.8e-14),
    # n on both sides of tri_cols' 128-row switch and past 256 rows, shuffled over the roles: the members' chains do not line up
    Case("e3_d3_n20_130_300_p3_f60", 10, 3, 3, ((20, 130, 300), (130, 300, 20), (300, 20, 130)), 3, 60, "random", None, 8, 3.3e-13),
    # the <24> gradient kernel, three 256-row strides, tri_cols' K slices, groups of three
    Case("e2_d20_n20_300_520_p2_f30", 11, 2, 20, ((20, 300, 520), (520, 20, 300)), 2, 30, "random", None, 8, 1.0e-15),
]
FLAT = "e1_d3_n20_p0_flat12"
ENSEMBLE = "e3_d3_n20_130_300_p3_f60"
WIDE = "e2_d20_n20_300_520_p2_f30"
# the believed-front rule, each branch under some member (tests/test_ehvi3_reference.py asserts which): member 0's outcome of
# pending point 0 joins and two front points leave, its outcome of pending point 1 is dominated; pending point 2 lies on an
# observation of 2.0 > r1 of every objective-1 GP: outside r; member 1's third objective has observed zeros only, so every outcome
# it believes has w = 0 exactly, on the device as here, and ties the front point placed at w = 0
BELIEVED = Case("e2_d3_n20_p5_believed", 21, 2, 3, _grid(2, 20), 5, None, "believed", None, 8, 1.8e-14)


def case(name):
    return next(c for c in CASES + [BELIEVED] if c.name == name)


def staircase_front(F, w_flat=None):
    """u ascending, v descending, w ascending (or all w_flat): every slab k keeps all its k points, B = (F + 1)(F + 2) / 2"""
    u = np.linspace(-0.8, 0.8, F) if F > 1 else np.array([0.0])
    w = np.linspace(-0.6, 0.6, F) if F > 1 else np.array([0.0])
    if w_flat is not None:
        w = np.full(F, float(w_flat))
    return np.ascontiguousarray(np.stack([u, 0.1 - u, w], axis=1))


def descending_front(F):
    """u and v descending as w ascends: slab k keeps point k alone"""
    return np.ascontiguousarray(np.stack([np.linspace(0.8, -0.6, F), np.linspace(0.7, -0.7, F), np.linspace(-0.7, 0.7, F)], axis=1))


def random_front(rng, F, shift=0.0):
    """F mutually non-dominated points about the plane u + v + w = shift, in the canonical order"""
    if F == 0:
        return np.zeros((0, 3))
    from cornell_moe_amd import expected_hypervolume_improvement as ehvi
    while True:
        uv = rng.uniform(-0.8, 0.8, size=(6 * F + 8, 2))
        w = shift - uv[:, 0] - uv[:, 1] + rng.uniform(-0.25, 0.25, size=len(uv))
        f = ehvi.pareto_front_3(np.column_stack([uv, np.clip(w, -0.9, 0.9)]), REF)
        if len(f) >= F:
            keep = np.sort(rng.choice(len(f), size=F, replace=False))
            return np.ascontiguousarray(f[keep])


def make_problem(c):
    """the inputs of a case.  The GPs of a case observe nested point lists; the first pending point lies within 0.05 of candidate 0
    in every coordinate (conditioning on P moves that candidate by far more than the tolerance)."""
    rng = np.random.default_rng(9900 + c.seed)
    length = LENGTH_0 + LENGTH_D * math.sqrt(c.d)
    Xc = rng.uniform(0, 1, size=(max(max(row) for row in c.n), c.d))
    believed = c.kind == "believed"
    gps = []
    for e in range(c.E):
        row = []
        for r in range(3):
            n = c.n[e][r]
            y = 0.3 * rng.normal(size=(n, 1))
            if believed and r == 0:
                y[0, 0] = 2.0
            if believed and r == 2 and e == 1:
                y[:] = 0.0
            f = 1.0 + 0.15 * ((e + 2 * r) % 4)
            hyper = np.array([1.3] + [length] * c.d) * f
            row.append(GP(MATERN if (e + r) % 2 == 0 else SE, hyper, Xc[:n].copy(), y, [1e-2 * f], ()))
        gps.append(row)
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    pending = rng.uniform(0, 1, size=(c.p, c.d))
    if c.p:
        pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=c.d)
    if c.kind == "stair":
        front = staircase_front(c.F)
    elif c.kind == "descend":
        front = descending_front(c.F)
    elif c.kind == "flat":
        front = staircase_front(c.F, w_flat=0.1)
    elif believed:
        pending[2] = Xc[0]
        bases = [[cr.base_model(g, np.float64) for g in row] for row in gps]
        out = [[tuple(float(cr.mean_at(b, pending)[j]) for b in row) for j in range(c.p)] for row in bases]
        o00, o01, o13 = np.array(out[0][0]), np.array(out[0][1]), np.array(out[1][3])
        pts = [o00 + (0.05, 0.05, 0.05), o00 + (0.03, 0.08, 0.06), o01 - (0.05, 0.05, 0.05), (o13[0] - 0.1, o13[1] + 0.1, 0.0),
               (-0.9, 1.3, 1.2), (1.4, -0.9, 1.2), (1.4, 1.3, -0.9)]
        from cornell_moe_amd import expected_hypervolume_improvement as ehvi
        front = ehvi.pareto_front_3(np.array(pts, dtype=np.float64), REF)
    else:
        front = random_front(rng, c.F)
    return Problem(c.name, gps, REF, front, points, pending, tuple(range(c.C)))


_WANT = {}


def expected(c, T=LD):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T)
    if key not in _WANT:
        p = make_problem(c)
        members = ensemble(p, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]
