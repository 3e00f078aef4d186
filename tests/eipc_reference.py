"""The LOG of the constrained expected improvement PER UNIT COST with pending points, averaged over an ensemble, restated on the CPU
(the checker of tests/test_gpu_eipc.py) in np.longdouble or float64, on top of tests/cei1_reference.py (Member, moments,
make_problem, Case) and tests/logcei1_reference.py (role_log, member_logs, relimited, SHIFTS), imported unchanged.

Member e is 2 + K GPs: cei1_reference's 1 + K (the objective, the constraints) and, as one more GP of the row, a GP of the LOG of
the evaluation cost.  A cr.Case with K + 1 in the place of K gives the same generator, seeds and nesting; the last GP of every row
is split off as the cost GP and the last threshold of the case is not used.  With mu_c, var_c the posterior mean and the latent
variance of the cost GP at x, conditioned on the pending points as every GP of the member is, and v_c = max(150 eps^2, var_c):
    l_c = -(alpha (mu_c + v_c / 2)),   grad l_c = -alpha grad mu_c - (alpha / 2) grad var_c   (the second term 0 below the floor)
    L_e = ((l_0 + l_1) + ... + l_K) + l_c with logcei1_reference's l_0 .. l_K, g_e likewise
    m = max_e L_e, w_e = exp(L_e - m), W = sum_e w_e:  value = m + log W - log E,  grad = (sum_e w_e g_e) / W
The believed-feasible incumbent b' is cr.Member's over the 1 + K GPs; the cost GP takes no part in it.
"""
import collections
import copy

import numpy as np

import cei1_reference as cr
import ei1_reference as er
import logcei1_reference as lr

LD = cr.LD
Result = lr.Result  # value grad log_factors bprime args


class Member(object):
    """a cr.Member over the row's first 1 + K GPs with the row's last GP as the cost GP, conditioned on the same pending points"""

    def __init__(self, gps, taus, best, P, alpha, T=LD):
        self.T, self.alpha = T, float(alpha)
        self.inner = cr.Member(gps[:-1], list(taus)[:len(gps) - 2], best, P, T)
        self.cost_gp = gps[-1]
        self.cost_base = cr.base_model(gps[-1], T)
        self.cost_model = cr.conditioned(self.cost_base, self.inner.P)

    @property
    def bprime(self):
        return self.inner.bprime

    def cost_log(self, x):
        """(l_c, grad l_c) at x"""
        T, a = self.T, self.T(self.alpha)
        mu, var, grad_mu, grad_var = cr.moments(self.cost_model, self.cost_base, x)
        floor = T(er.MIN_VAR_GRAD_EI)
        v = max(floor, var)
        g = -a * grad_mu
        if not var < floor:
            g = g - (a / T(2)) * grad_var
        return -(a * (mu + v / T(2))), g

    def logs(self, x):
        """([l_0 .. l_K, l_c], their gradients, [c, z_1 .. z_K]) at x"""
        vals, grads, cz = lr.member_logs(self.inner, x)
        lc, gc = self.cost_log(x)
        return vals + [lc], grads + [gc], cz


def ensemble(p, alpha, T=LD, pending=None):
    """the members of a problem made from a K + 1 case"""
    P = p.pending if pending is None else pending
    return [Member(g, p.thresholds[:len(g) - 2], b, P, alpha, T) for g, b in zip(p.gps, p.best)]


def with_exponent(members, alpha):
    """the same factored members under another exponent"""
    out = []
    for m in members:
        n = copy.copy(m)
        n.alpha = float(alpha)
        out.append(n)
    return out


def relimited(members, best, taus):
    """the same factored members under other incumbents [E] and thresholds [K] (lr.relimited on the 1 + K GPs)"""
    inner = lr.relimited([m.inner for m in members], best, taus)
    out = []
    for m, i in zip(members, inner):
        n = copy.copy(m)
        n.inner = i
        out.append(n)
    return out


def evaluate(members, x):
    """Result of the ensemble at x; log_factors [E][2 + K], the cost's last"""
    T = members[0].T
    Ls, gs, logs, args = [], [], [], []
    for m in members:
        vals, grads, cz = m.logs(x)
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


# ---- the cases of tests/test_gpu_eipc.py (tests/test_eipc_reference.py qualifies them on the CPU) ----
# cr.Case with K + 1 in the place of K: n[e] has 2 + K entries, tau and offset K + 1 (the last of each belongs to the cost GP's slot:
# the threshold is unused, the offset is the level of the log cost's observations).
def _grid(E, G, n):
    return tuple(tuple(n for _ in range(G)) for _ in range(E))


def _rotated(rows, E):
    return tuple(tuple(rows[(r + e) % len(rows)] for r in range(len(rows))) for e in range(E))


SMALLEST = cr.Case("eipc_e1_k0_d3_n20_p0", 61, 1, 1, 3, _grid(1, 2, 20), 0, (), "median", (0.0,), None, 6, None)
SECOND = cr.Case("eipc_e1_k1_d3_n20_p3", 62, 1, 2, 3, _grid(1, 3, 20), 3, (), "median", (0.0, 0.0), None, 6, None)
# rows on both sides of tri_cols' 128-row switch and one R > 256, rotated over the four roles: the chains do not line up and the cost
# GP has 300, 12 and 130 rows under members 0, 1, 2
ENSEMBLE = cr.Case("eipc_e3_k2_d3_n12_130_40_300_p3", 63, 3, 3, 3, _rotated((12, 130, 40, 300), 3), 3, (), "median", (0.1, 0.0, 0.0),
                   None, 6, None)
D10 = cr.Case("eipc_e1_k1_d10_n20_p2", 64, 1, 2, 10, _grid(1, 3, 20), 2, (), "median", (0.0, 0.0), None, 6, None)
DERIV = cr.Case("eipc_e1_k1_d3_n12_g1_p2", 65, 1, 2, 3, _grid(1, 3, 12), 2, (1,), "median", (0.0, 0.0), None, 6, None)
# member 0 has no feasible observation and believes its pending points infeasible (b'_0 stays +infinity) beside a finite member
INF = cr.Case("eipc_e2_k1_d3_n20_p2_inf", 66, 2, 2, 3, _grid(2, 3, 20), 2, (), ("inf", "median"), (0.0, 0.0), ((0.5, 0.0), (-0.2, 0.0)),
              6, None)
K8 = cr.Case("eipc_e1_k8_d3_n20_p1", 67, 1, 9, 3, _grid(1, 10, 20), 1, (), "median", (0.3,) * 9, None, 6, None)
WIDE = cr.Case("eipc_e3_k2_d20_n20_300_600_40_p3", 68, 3, 3, 20, _rotated((20, 300, 600, 40), 3), 3, (), "median", (0.1, 0.0, 0.0),
               None, 6, None)
K0_ENSEMBLE = cr.Case("eipc_e3_k0_d3_n40_130_p2", 69, 3, 1, 3, ((40, 130), (130, 12), (12, 40)), 2, (), "median", (0.0,), None, 6, None)
CASES = [SMALLEST, SECOND, ENSEMBLE, D10, DERIV, INF, K8, WIDE]
DEEPEST = lr.SHIFTS[-1]
# (case, shift, alpha) of the comparison with long double
RUNS = [(c, lr.SHIFTS[0], 1.0) for c in CASES] + [(SECOND, DEEPEST, 1.0), (WIDE, DEEPEST, 1.0), (SECOND, lr.SHIFTS[0], 0.5),
                                                 (SECOND, lr.SHIFTS[0], 2.0)]
RUN_IDS = ["%s-b%g-t%g-a%g" % (c.name, s[0], s[1], a) for c, s, a in RUNS]


def make_problem(c):
    """cr.make_problem of the K + 1 case: rows of 2 + K GPs, the cost GP last; thresholds [K]"""
    p = cr.make_problem(c)
    return p._replace(thresholds=list(p.thresholds)[:c.K - 1])


_MEMBERS, _WANT = {}, {}


def members_of(c, T=LD):
    """(problem, members at alpha = 1) of a case as it stands, factored once per process"""
    key = (c.name, T)
    if key not in _MEMBERS:
        p = make_problem(c)
        _MEMBERS[key] = (p, ensemble(p, 1.0, T))
    return _MEMBERS[key]


def shifted(c, shift, alpha, T=LD):
    """(problem, members) with every finite incumbent lowered by shift[0], every threshold by shift[1], at exponent alpha"""
    p, members = members_of(c, T)
    best = [b - shift[0] if np.isfinite(b) else b for b in p.best]
    taus = [t - shift[1] for t in p.thresholds]
    return p._replace(best=best, thresholds=taus), with_exponent(relimited(members, best, taus), alpha)


def expected(c, shift, alpha, T=LD):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, tuple(shift), float(alpha), T)
    if key not in _WANT:
        p, members = shifted(c, shift, alpha, T)
        _WANT[key] = (p, [evaluate(members, x) for x in p.points])
    return _WANT[key]


def without_cost(p):
    """the problem's objective and constraint GPs alone: what logcei1_reference and api.log_ei_constrained_ensemble take"""
    return p._replace(gps=[row[:-1] for row in p.gps])


# ---- the two-basin problem: cost changes the answer ----
# d = 2, one member, K = 0.  The objective GP is observed at 12 points and their mirror images x0 -> 1 - x0 with equal values, so its
# posterior is mirror-symmetric; its observed values have their minima near x0 = 0.2 and x0 = 0.8.  The cost GP is observed at the same
# 24 points with log cost 2 x0 under noise 1e-4: the basin at x0 = 0.2 is the cheaper.  16 starts, 8 of them the mirrors of the
# other 8.  At alpha = 0 a point and its mirror image have the same value; at alpha = 1 they differ by about 2 (1 - 2 x0).
TwoBasin = collections.namedtuple("TwoBasin", "problem starts bounds gd")


def mirrored(x):
    x = np.array(x, dtype=np.float64, copy=True)
    x[..., 0] = 1.0 - x[..., 0]
    return x


def two_basin():
    rng = np.random.default_rng(8811)
    half = np.column_stack([rng.uniform(0.03, 0.47, size=12), rng.uniform(0.05, 0.95, size=12)])
    X = np.vstack([half, mirrored(half)])
    f = 40.0 * ((X[:, 0] - 0.5) ** 2 - 0.09) ** 2 + 0.5 * (X[:, 1] - 0.5) ** 2
    hyper = np.array([1.0, 0.25, 0.4])
    obj = cr.GP(cr.SE, hyper, X, f.reshape(-1, 1), [1e-4], ())
    cost = cr.GP(cr.SE, np.array([1.5, 0.6, 0.8]), X, (2.0 * X[:, 0]).reshape(-1, 1), [1e-4], ())
    s = np.column_stack([rng.uniform(0.05, 0.45, size=8), rng.uniform(0.1, 0.9, size=8)])
    starts = np.vstack([s, mirrored(s)])
    best = float(np.min(f))
    p = cr.Problem("eipc_two_basin", [[obj, cost]], [], [best], starts, np.zeros((0, 2)), tuple(range(16)))
    return TwoBasin(p, starts, np.array([[0.0, 1.0]] * 2), lr.STALL_GD)


_BASIN = {}


def two_basin_margin():
    """(the margin, the restatement's best start, the long-double difference there): the difference of the alpha = 1 value at the
    restatement's best start and at its mirror image, halved"""
    if not _BASIN:
        tb = two_basin()
        members = ensemble(tb.problem, 1.0, LD)
        vals = [evaluate(members, x).value for x in tb.starts]
        s = int(np.argmax(vals))
        diff = float(vals[s] - evaluate(members, mirrored(tb.starts[s])).value)
        _BASIN["m"] = (0.5 * diff, s, diff)
    return _BASIN["m"]
