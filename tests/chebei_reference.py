"""The Chebyshev-scalarised expected improvement for 2 to 8 objectives with pending points, averaged over an ensemble, restated on
the CPU (the checker of tests/test_gpu_chebei.py) in np.longdouble or float64, on top of tests/kg1_reference.py (Model),
tests/kg1_pending_reference.py (PendingModel), tests/cei1_reference.py (moments, mean_at), tests/ei1_reference.py (normal_cdf, the
floor) and kg1_reference.normal_pdf, all imported unchanged: the (N + p)^2 system of every GP is factored in full and nothing of
the device's extension appears.

Member e is M GPs.  With mu_j, var_j the posterior mean and the conditioned latent variance of GP j at x, ONE floor for value and
gradient, sigma_j = sqrt(max(150 eps^2, var_j)), and a scalarisation a_j > 0, b_j:
    s_j = a_j mu_j + b_j,  tau_j = a_j sigma_j,  L = max_j (s_j - 38 tau_j),  z_j(t) = (t - s_j) / tau_j
    A_e = integral over L <= t <= g*_e of prod_j Phi(z_j);  0 with zero coefficients where g*_e <= L
    dA/dmu_j = -a_j integral phi(z_j) / tau_j prod_{k != j} Phi(z_k),  dA/dvar_j = -(a_j / (2 sigma_j)) integral z_j phi(z_j) / tau_j ...
    g*_e = min(best_e, min_i max_j (a_j mu_{e,j}(P_i) + b_j)) over the pending points whose scalarised outcome is finite
    value = (A_0 + ... + A_{E-1}) / E
by the FIXED quadrature of csrc/chebei1.hip: the same 14 M + 2 breakpoints, sort, 8-point Gauss-Legendre nodes and node order (lane
l of sweep s owns node 64 s + l, sweeps ascend, the lanes are summed by the butterfly xor 32 .. 1), the products without j from
prefix and suffix products.  cdf_many / pdf_many are ei1_reference.normal_cdf / kg1_reference.normal_pdf over an array, the same
operations element by element (tests/test_chebei_reference.py holds them to the scalar functions bit for bit).
scale = max(1, |best|, |b_j|, a_j max |y_j|, a_j sqrt(alpha_j)) over the member's GPs; an ensemble takes its largest member scale.
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

BREAKS = (-38, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8)
GL8_X = tuple(float.fromhex(h) for h in (
    "-0x1.ebab1cb0acc67p-1", "-0x1.97e4ab249f41ep-1", "-0x1.0d129583284b4p-1", "-0x1.77ac94f3c7345p-3",
    "0x1.77ac94f3c7345p-3", "0x1.0d129583284b4p-1", "0x1.97e4ab249f41ep-1", "0x1.ebab1cb0acc67p-1"))
GL8_W = tuple(float.fromhex(h) for h in (
    "0x1.9ea1d04ca0374p-4", "0x1.c76fb531d2b96p-3", "0x1.413c50a255615p-2", "0x1.736360b199343p-2",
    "0x1.736360b199343p-2", "0x1.413c50a255615p-2", "0x1.c76fb531d2b96p-3", "0x1.9ea1d04ca0374p-4"))

Problem = collections.namedtuple("Problem", "name M gps scal best points pending checked")
Result = collections.namedtuple("Result", "value grad members scale")
Integral = collections.namedtuple("Integral", "A IM IV L breaks")


# ---- Phi and phi over arrays: kg1_reference._erfc_nonneg's operations, element by element ----
def _erfc_nonneg_many(x, T):
    x = np.asarray(x, dtype=T)
    out = np.zeros(x.shape, dtype=T)
    root_pi = np.sqrt(T(4) * np.arctan(T(1)))
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        e = np.exp(-x * x)
        low = x < T(2.5)
        if low.any():
            xs, es = x[low], e[low]
            term, total = xs.copy(), xs.copy()
            live = np.ones(xs.shape, dtype=bool)
            n = 0
            while live.any():
                n += 1
                nt = term * T(2) * xs * xs / T(2 * n + 1)
                term = np.where(live, nt, term)
                total = np.where(live, total + term, total)
                live = live & ~(term <= total * T(np.finfo(T).eps) / T(8))
            out[low] = T(1) - T(2) / root_pi * es * total
        high = ~low & np.isfinite(x)
        if high.any():
            xs = x[high]
            t = xs.copy()
            for k in range(400, 0, -1):
                t = xs + T(k) / T(2) / t
            out[high] = e[high] / (root_pi * t)
    return out


def cdf_many(z, T):
    """Phi(z) element by element: erfc on the side of z's sign (kg1_reference.normal_cdf_diff from -infinity)"""
    z = np.asarray(z, dtype=T)
    r = T(1) / np.sqrt(T(2))
    neg = z <= 0
    out = np.empty(z.shape, dtype=T)
    # normal_cdf_diff(-inf, z): z <= 0 -> (erfc(-z r) - erfc(inf)) / 2; z > 0 -> (1 - erfc(inf) / 2) - erfc(z r) / 2
    out[neg] = (_erfc_nonneg_many(-z[neg] * r, T) - T(0)) / T(2)
    out[~neg] = (T(1) - T(0) / T(2)) - _erfc_nonneg_many(z[~neg] * r, T) / T(2)
    return out


def pdf_many(z, T):
    z = np.asarray(z, dtype=T)
    with np.errstate(under="ignore"):
        return np.exp(-z * z / T(2)) / np.sqrt(T(8) * np.arctan(T(1)))


# ---- the scalarisation ----
def scalarisation(weights, ideal, nadir):
    w, lo, hi = (np.asarray(v, dtype=np.float64).ravel() for v in (weights, ideal, nadir))
    a = w / (hi - lo)
    return np.concatenate([a, -a * lo])


def split(scal):
    scal = np.asarray(scal, dtype=np.float64).ravel()
    M = scal.size // 2
    return scal[:M], scal[M:]


def sigma_of(var, T):
    return np.sqrt(max(T(er.MIN_VAR_GRAD_EI), T(var)))


def scalarised_moments(a, b, mus, variances, T):
    """(s [M], tau [M], sigma [M]), product and sum each rounded"""
    s, tau, sg = [], [], []
    for j in range(len(a)):
        sig = sigma_of(variances[j], T)
        s.append(T(a[j]) * T(mus[j]) + T(b[j]))
        tau.append(T(a[j]) * sig)
        sg.append(sig)
    return s, tau, sg


def breakpoints(s, tau, g, T):
    """(L, the 14 M + 2 breakpoints sorted ascending, ties by position)"""
    L = max(s[j] + T(-38) * tau[j] for j in range(len(s)))
    raw = []
    for j in range(len(s)):
        for c in BREAKS:
            raw.append(min(max(s[j] + T(c) * tau[j], L), T(g)))
    raw += [L, T(g)]
    order = sorted(range(len(raw)), key=lambda k: (raw[k], k))
    return L, [raw[k] for k in order]


def integrand(t, s, tau, T, want_grad=True):
    """at the nodes t [n]: (prod_j Phi(z_j) [n], [phi(z_j) / tau_j prod_{k != j} Phi(z_k)] [M][n], the same times z_j [M][n])"""
    M = len(s)
    z = [(t - s[j]) / tau[j] for j in range(M)]
    cdf = [cdf_many(z[j], T) for j in range(M)]
    P = cdf[0].copy()
    for j in range(1, M):
        P = P * cdf[j]
    if not want_grad:
        return P, None, None
    others, run = [], np.ones(t.shape, dtype=T)
    for j in range(M):
        others.append(run)
        run = run * cdf[j]
    run = np.ones(t.shape, dtype=T)
    for j in range(M - 1, -1, -1):
        others[j] = others[j] * run
        run = run * cdf[j]
    dens = [pdf_many(z[j], T) / tau[j] * others[j] for j in range(M)]
    return P, dens, [z[j] * dens[j] for j in range(M)]


def _wavefront_sum(terms, T):
    """the device's order: lane l adds terms l, l + 64, ... in ascending sweeps, then the butterfly xor 32, 16, 8, 4, 2, 1"""
    n = len(terms)
    padded = np.zeros(((n + 63) // 64) * 64, dtype=T)
    padded[:n] = terms
    acc = np.zeros(64, dtype=T)
    for row in padded.reshape(-1, 64):
        acc = acc + row
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ off]
    return acc[0]


def integral(s, tau, g, T=LD, want_grad=True):
    """the fixed quadrature: Integral(A, [integral of dens_j], [integral of z_j dens_j], L, the sorted breakpoints)"""
    M = len(s)
    L, bp = breakpoints(s, tau, g, T)
    zero = [T(0)] * M
    if not T(g) > L:
        return Integral(T(0), zero, zero, L, bp)
    lo, hi = np.array(bp[:-1], dtype=T), np.array(bp[1:], dtype=T)
    half = T(0.5) * (hi - lo)
    mid = T(0.5) * (lo + hi)
    x, w = np.array(GL8_X, dtype=T), np.array(GL8_W, dtype=T)
    t = (mid[:, None] + half[:, None] * x[None, :]).ravel()
    wt = (half[:, None] * w[None, :]).ravel()
    live = wt > 0
    P, dens, zdens = integrand(t[live], s, tau, T, want_grad)

    def total(values):
        terms = np.zeros(t.shape, dtype=T)
        terms[live] = wt[live] * values
        return _wavefront_sum(terms, T)

    A = total(P)
    if not want_grad:
        return Integral(A, zero, zero, L, bp)
    return Integral(A, [total(d) for d in dens], [total(d) for d in zdens], L, bp)


def coefficients(a, sg, I, T):
    """[dA/dmu_0, dA/dvar_0, ..., dA/dmu_{M-1}, dA/dvar_{M-1}]"""
    out = []
    for j in range(len(a)):
        out += [-T(a[j]) * I.IM[j], -(T(a[j]) / (T(2) * sg[j])) * I.IV[j]]
    return out


def value_at_moments(a, b, mus, variances, g, T=LD, want_grad=True):
    """(A, the 2 M coefficients) of one member from its M (mu, var), the scalarisation and the incumbent"""
    s, tau, sg = scalarised_moments(a, b, mus, variances, T)
    I = integral(s, tau, g, T, want_grad)
    return I.A, coefficients(a, sg, I, T)


def refined_value(a, b, mus, variances, g, T=LD, nodes=32):
    """the same integral by an independent evaluation: every panel halved, a rule of `nodes` points per half (numpy's leggauss,
    the nodes polished by Newton's iteration in T), added in plain order"""
    s, tau, sg = scalarised_moments(a, b, mus, variances, T)
    L, bp = breakpoints(s, tau, g, T)
    if not T(g) > L:
        return T(0)
    x0, _ = np.polynomial.legendre.leggauss(nodes)
    x = np.array(x0, dtype=T)
    for _ in range(3):
        p0, p1 = np.ones(nodes, dtype=T), x.copy()
        for k in range(2, nodes + 1):
            p0, p1 = p1, (T(2 * k - 1) * x * p1 - T(k - 1) * p0) / T(k)
        dp = T(nodes) * (x * p1 - p0) / (x * x - T(1))
        x = x - p1 / dp
    p0, p1 = np.ones(nodes, dtype=T), x.copy()
    for k in range(2, nodes + 1):
        p0, p1 = p1, (T(2 * k - 1) * x * p1 - T(k - 1) * p0) / T(k)
    dp = T(nodes) * (x * p1 - p0) / (x * x - T(1))
    w = T(2) / ((T(1) - x * x) * dp * dp)
    total = T(0)
    for lo, hi in zip(bp[:-1], bp[1:]):
        if not hi > lo:
            continue
        m = T(0.5) * (lo + hi)
        for u, v in ((lo, m), (m, hi)):
            half, mid = T(0.5) * (v - u), T(0.5) * (u + v)
            P, _, _ = integrand(mid + half * x, s, tau, T, want_grad=False)
            total = total + half * np.sum(w * P)
    return total


def analytic_ei(mu, sigma, best, T=LD):
    """E[(best - Y)^+] for Y ~ N(mu, sigma^2)"""
    z = (T(best) - T(mu)) / T(sigma)
    return (T(best) - T(mu)) * er.normal_cdf(z, T) + T(sigma) * kr.normal_pdf(z, T)


# ---- the believed-incumbent rule ----
def scalarised_outcomes(a, b, outcomes, T):
    """max_j (a_j mu_j(P_i) + b_j) per pending point, outcomes [M][p]; an outcome that is not finite gives +infinity"""
    out = []
    for i in range(len(outcomes[0]) if len(outcomes) else 0):
        vals = [T(a[j]) * T(outcomes[j][i]) + T(b[j]) for j in range(len(a))]
        out.append(max(vals) if all(np.isfinite(v) for v in vals) else T(np.inf))
    return out


def incumbent(a, b, outcomes, best, T=LD):
    g = T(best)
    for v in scalarised_outcomes(a, b, outcomes, T):
        if np.isfinite(v):
            g = min(g, v)
    return g


def member_scale(gps, a, b, best):
    s = [1.0, abs(float(best))]
    for j, g in enumerate(gps):
        s += [abs(float(b[j])), float(a[j]) * float(np.max(np.abs(np.asarray(g.y, dtype=np.float64)))),
              float(a[j]) * math.sqrt(float(np.asarray(g.hyper).ravel()[0]))]
    return max(s)


class Member(object):
    """one member's M GPs conditioned on P and the outcomes it believes, factored once for every candidate and scalarisation"""

    def __init__(self, gps, P, T=LD):
        self.T, self.gps = T, gps
        self.P = np.asarray(P, dtype=np.float64).reshape(-1, np.asarray(gps[0].X).shape[1])
        self.bases = [cr.base_model(g, T) for g in gps]
        self.models = [cr.conditioned(b, self.P) for b in self.bases]
        self.outcomes = [cr.mean_at(b, self.P) for b in self.bases] if len(self.P) else []

    def incumbent(self, scal, best):
        a, b = split(scal)
        return incumbent(a, b, self.outcomes, best, self.T)

    def moments(self, x):
        return [cr.moments(m, b, x) for m, b in zip(self.models, self.bases)]

    def evaluate(self, x, scal, best, want_grad=True):
        """(A_e, grad A_e) at x under the scalarisation and the member's own incumbent"""
        T = self.T
        a, b = split(scal)
        mo = self.moments(x)
        g = self.incumbent(scal, best)
        A, c = value_at_moments(a, b, [m[0] for m in mo], [m[1] for m in mo], g, T, want_grad)
        grad = np.zeros(len(x), dtype=T)
        if want_grad:
            for j in range(len(a)):
                grad = grad + (c[2 * j] * mo[j][2] + c[2 * j + 1] * mo[j][3])
        return A, grad


def ensemble(p, T=LD, pending=None, members=None):
    """the members of a problem (pending: others than the problem's; members: a subset of the member indices)"""
    P = p.pending if pending is None else pending
    idx = range(len(p.gps)) if members is None else members
    return [Member(p.gps[e], P, T) for e in idx]


def evaluate(members, x, scal, best, scales, want_grad=True):
    T = members[0].T
    value, grad, vals = T(0), np.zeros(len(x), dtype=T), []
    for m, bst in zip(members, best):
        A, g = m.evaluate(x, scal, bst, want_grad)
        value, grad = value + A, grad + g
        vals.append(A)
    n = T(len(members))
    return Result(value / n, grad / n, vals, max(scales))


def scales_of(p, r=0):
    a, b = split(p.scal[r])
    return [member_scale(g, a, b, p.best[r][e]) for e, g in enumerate(p.gps)]


# ---- the cases of tests/test_gpu_chebei.py ----
# Case: E members of M GPs in dim d; n[e][j] observations; p pending points; C candidates; kind: how the problem is made; ld_diff:
# the worst float64-against-long-double difference over the case's candidates in units of scale, as tests/test_chebei_reference.py
# measured it (value, members' values and gradient; the GPU tolerance is max(1e-10, 4 ld_diff) scale).
Case = collections.namedtuple("Case", "name seed M E d n p C kind ld_diff")

LENGTH_0, LENGTH_D = kp.LENGTH_0, kp.LENGTH_D
IDEAL, NADIR = -1.0, 1.0


def _grid(E, M, n):
    return tuple(tuple(n for _ in range(M)) for _ in range(E))


CASES = [
    Case("m2_e1_d3_n20_p0", 1, 2, 1, 3, _grid(1, 2, 20), 0, 8, "plain", 1.8e-15),   # 29 panels, 232 nodes: a last sweep of 40 lanes
    Case("m3_e1_d3_n20_p2", 2, 3, 1, 3, _grid(1, 3, 20), 2, 8, "plain", 5.1e-16),
    Case("m5_e1_d3_n20_p2", 3, 5, 1, 3, _grid(1, 5, 20), 2, 8, "plain", 1.8e-16),
    Case("m8_e1_d3_n20_p0", 4, 8, 1, 3, _grid(1, 8, 20), 0, 8, "plain", 4.1e-17),   # 904 nodes: a last sweep of 8 lanes
    # objective 1 is ONE noise-free observation with alpha = 4: at candidate 0, that observation's point, its variance is 0 in every
    # arithmetic and sigma the floor; objectives 0 and 2 carry weights so small that all 28 of their breakpoints clamp to L
    Case("m3_e1_d3_floor", 5, 3, 1, 3, ((20, 1, 20),), 0, 8, "floor", 2.7e-16),
    Case("m4_e1_d3_n20_decades", 6, 4, 1, 3, _grid(1, 4, 20), 0, 8, "decades", 8.4e-16),  # a_j = 1e-5, 1e-3, 1e-1, 10
    Case("m3_e1_d3_n20_below", 7, 3, 1, 3, _grid(1, 3, 20), 0, 8, "below", 0.0),        # g* below L: exact zeros
    Case("m3_e1_d3_n20_above", 8, 3, 1, 3, _grid(1, 3, 20), 0, 8, "above", 7.2e-15),      # g* above every s_j + 8 tau_j
    # n on both sides of tri_cols' 128-row switch and past 256 rows, shuffled over the roles, both covariance types
    Case("m3_e3_d3_n20_130_300_p3", 9, 3, 3, 3, ((20, 130, 300), (130, 300, 20), (300, 20, 130)), 3, 8, "plain", 1.3e-14),
    # the <24> gradient kernel, tri_cols' K slices
    Case("m2_e1_d20_n300_520_p2", 10, 2, 1, 20, ((300, 520),), 2, 8, "plain", 3.0e-17),
]
ENSEMBLE = "m3_e3_d3_n20_130_300_p3"
FLOOR = "m3_e1_d3_floor"
# the believed rule, E = 2, p = 4: (a) an outcome lowers member 0's incumbent and not member 1's; (b) no outcome lowers any; (c) a
# second scalarisation under which ANOTHER pending point is member 0's incumbent
BELIEVED = [
    Case("m2_e2_d3_n20_p4_believed_one", 21, 2, 2, 3, _grid(2, 2, 20), 4, 8, "believed_one", 1.9e-15),
    Case("m2_e2_d3_n20_p4_believed_none", 21, 2, 2, 3, _grid(2, 2, 20), 4, 8, "believed_none", 1.9e-15),
    Case("m2_e2_d3_n20_p4_believed_other", 21, 2, 2, 3, _grid(2, 2, 20), 4, 8, "believed_other", 2.6e-15),
]
# the limit of 1024 GPs, value only (tests/test_gpu_chebei.py holds members 0, 63 and 127 to long double)
MANY = Case("m8_e128_d3_n4_p0", 31, 8, 128, 3, _grid(128, 8, 4), 0, 2, "plain", 1.9e-18)
ALL_CASES = CASES + BELIEVED
# ---- the cases of tests/test_gpu_chebei_edges.py ----
# M = 6 and M = 7 (86 and 100 breakpoints, 680 and 792 nodes: last sweeps of 40 and 24 lanes), M = 7 with n on both sides of
# tri_cols' 128-row switch, alternating over the roles and the members
M6, M7 = "m6_e1_d3_n20_p2", "m7_e2_d3_n20_130_p2"
M6_ABOVE, M7_ABOVE = "m6_e1_d3_n20_p0_above", "m7_e1_d3_n20_p0_above"
# mixed: member 0's incumbent lies below L at every candidate (exact zeros, zero coefficients) beside a live member 1
MIXED = "m3_e2_d3_n20_p0_mixed"
# p64: 64 pending points, every incumbent above every believed outcome, ordered so that member 0's lowest believed scalarised
# outcome is point 63 and member 1's is point 40, each at least P64_MARGIN below the member's runner-up
P64 = "m3_e2_d3_n20_p64"
P64_MARGIN = 1e-3
P64_SLOTS = ((0, 0, 63), (1, 0, 40))  # (member, rank among the member's outcomes from the lowest, the pending point's index)
EDGE_CASES = [
    Case(M6, 51, 6, 1, 3, _grid(1, 6, 20), 2, 6, "plain", 7.8e-17),
    Case(M7, 52, 7, 2, 3, ((20, 130, 20, 130, 20, 130, 20), (130, 20, 130, 20, 130, 20, 130)), 2, 6, "plain", 3.6e-15),
    # With an observed incumbent most breakpoints clamp to g*, the panels at the top have no width and the last, partly filled sweep
    # adds exact zeros (tests/test_chebei_reference.py asserts it of M6 and M7).  With g* above every s_j + 8 tau_j every panel has
    # a width and the last sweep carries nearly all of the value.
    Case(M6_ABOVE, 55, 6, 1, 3, _grid(1, 6, 20), 0, 6, "above", 1.1e-15),
    Case(M7_ABOVE, 56, 7, 1, 3, _grid(1, 7, 20), 0, 6, "above", 3.5e-15),
    Case(MIXED, 53, 3, 2, 3, _grid(2, 3, 20), 0, 6, "mixed", 2.0e-16),
    Case(P64, 54, 3, 2, 3, _grid(2, 3, 20), 64, 2, "p64", 8.7e-17),
]


def case(name):
    return next(c for c in ALL_CASES + EDGE_CASES + [MANY] if c.name == name)


def _random_gps(rng, c):
    length = LENGTH_0 + LENGTH_D * math.sqrt(c.d)
    nmax = max(max(row) for row in c.n)
    Xc = rng.uniform(0, 1, size=(nmax, c.d))
    gps = []
    for e in range(c.E):
        row = []
        for j in range(c.M):
            n = c.n[e][j]
            f = 1.0 + 0.15 * ((e + 2 * j) % 4)
            hyper = np.array([1.3 * f] + [length * f] * c.d)
            y = 0.3 * rng.normal(size=(n, 1)) + 0.1 * (j % 3)
            row.append(GP(MATERN if (e + j) % 2 == 0 else SE, hyper, Xc[:n].copy(), y, [1e-2 * f], ()))
        gps.append(row)
    return gps


def observed_best(gps, scal):
    """per member the smallest scalarised observation over the rows all its GPs share"""
    a, b = split(scal)
    out = []
    for row in gps:
        n = min(len(g.X) for g in row)
        y = np.stack([np.asarray(g.y, dtype=np.float64).ravel()[:n] for g in row], axis=1)
        out.append(float(np.min(np.max(a[None, :] * y + b[None, :], axis=1))))
    return out


def _float64_outcomes(gps, pending, scal):
    """G[e][i]: member e's scalarised believed outcome of pending point i, in float64"""
    a, b = split(scal)
    return [[float(v) for v in scalarised_outcomes(a, b, Member(row, pending, np.float64).outcomes, np.float64)] for row in gps]


def place_pending(rng, gps, scal, p, d, slots):
    """p pending points, drawn until they can be ordered as `slots` asks: for every (member, rank, index) the member's rank-th
    lowest believed scalarised outcome (float64) is point `index`, the slots name different points, and each of these outcomes
    and the member's next one lie at least 2 P64_MARGIN apart (the outcomes are the unconditioned means: an order of the points
    changes none)"""
    top = {}
    for e, r, _ in slots:
        top[e] = max(top.get(e, 0), r)
    while True:
        pending = rng.uniform(0, 1, size=(p, d))
        G = _float64_outcomes(gps, pending, scal)
        order = [np.argsort(g) for g in G]
        clear = all(G[e][order[e][k + 1]] - G[e][order[e][k]] >= 2.0 * P64_MARGIN for e, r in top.items() for k in range(r + 1))
        chosen = [int(order[e][r]) for e, r, _ in slots]
        if clear and len(set(chosen)) == len(chosen):
            break
    perm = [None] * p
    for src, (_, _, index) in zip(chosen, slots):
        perm[index] = src
    rest = iter(i for i in range(p) if i not in chosen)
    return np.ascontiguousarray(pending[[next(rest) if v is None else v for v in perm]])


def make_problem(c):
    rng = np.random.default_rng(9700 + c.seed)
    gps = _random_gps(rng, c)
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    pending = rng.uniform(0, 1, size=(c.p, c.d))
    if c.p:
        pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=c.d)
    w = rng.exponential(size=c.M) + 0.2
    scal = scalarisation(w / w.sum(), [IDEAL] * c.M, [NADIR] * c.M)
    best = observed_best(gps, scal)
    scals, bests = [scal], [best]
    if c.kind == "floor":
        X1 = points[0:1].copy()
        gps[0][1] = GP(MATERN, np.array([4.0] + [0.5] * c.d), X1, np.array([[0.4]]), [0.0], ())
        scals = [scalarisation([0.05, 0.9, 0.05], [IDEAL] * 3, [NADIR] * 3)]
        bests = [[0.45 * 1.4 + 0.3]]
    elif c.kind == "decades":
        a = np.array([1e-5, 1e-3, 1e-1, 10.0])
        scals, bests = [np.concatenate([a, np.full(4, 0.5)])], [[0.6]]
    elif c.kind == "below":
        bests = [[-1e3]]
    elif c.kind == "above":
        bests = [[50.0]]
    elif c.kind == "mixed":
        bests = [[-1e3] + best[1:]]
    elif c.kind == "p64":
        pending = place_pending(rng, gps, scal, c.p, c.d, P64_SLOTS)
        bests = [[max(max(row) for row in _float64_outcomes(gps, pending, scal)) + 0.05] * c.E]
    elif c.kind.startswith("believed"):
        G = _float64_outcomes(gps, pending, scal)
        if c.kind == "believed_one":
            bests = [[min(G[0]) + 0.05, min(G[1]) - 0.05]]
        elif c.kind == "believed_none":
            bests = [[min(G[0]) - 0.05, min(G[1]) - 0.05]]
        else:
            first = int(np.argmin(G[0]))
            while True:  # weights under which another pending point is member 0's incumbent, by a clear margin
                w = rng.exponential(size=c.M) + 0.05
                other = scalarisation(w / w.sum(), [IDEAL] * c.M, [NADIR] * c.M)
                H = _float64_outcomes(gps, pending, other)
                order = np.argsort(H[0])
                if int(order[0]) != first and H[0][order[1]] - H[0][order[0]] > 1e-3:
                    break
            scals = [other]
            bests = [[min(H[0]) + 0.05, min(H[1]) + 0.05]]
    return Problem(c.name, c.M, gps, [np.asarray(s, dtype=np.float64) for s in scals], [list(map(float, b)) for b in bests], points,
                   np.ascontiguousarray(pending), tuple(range(c.C)))


_WANT = {}


def expected(c, T=LD, members=None):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T, members)
    if key not in _WANT:
        p = make_problem(c)
        ms = ensemble(p, T, members=members)
        idx = range(len(p.gps)) if members is None else members
        best = [p.best[0][e] for e in idx]
        sc = scales_of(p)
        _WANT[key] = (p, [evaluate(ms, x, p.scal[0], best, [sc[e] for e in idx]) for x in p.points])
    return _WANT[key]


def ld_difference(c):
    """the worst float64-against-long-double difference of a case in units of scale: value, members' values, gradient"""
    _, hi = expected(c, LD)
    _, lo = expected(c, np.float64)
    worst = 0.0
    for h, l in zip(hi, lo):
        worst = max(worst, abs(float(h.value - LD(l.value))) / h.scale)
        worst = max(worst, max(abs(float(x - LD(y))) for x, y in zip(h.members, l.members)) / h.scale)
        gs = min(h.scale, max(1.0, float(np.max(np.abs(h.grad)))))
        worst = max(worst, float(np.max(np.abs(h.grad - l.grad.astype(LD)))) / gs)
    return worst
