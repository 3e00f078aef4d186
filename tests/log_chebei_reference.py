"""The LOG of the Chebyshev-scalarised expected improvement for 2 to 8 objectives with 0 to 8 constraints and pending points, under an
ensemble's log-sum-exp, restated on the CPU (the checker of tests/test_gpu_log_chebei.py) in np.longdouble or float64, on top of
tests/chebei_reference.py (the scalarisation, the moments, the 14 M breakpoints, the Gauss-Legendre constants, the incumbent rule,
the problems), tests/logcei1_reference.py (log_cdf_parts, role_log), tests/log_ehvi_reference.py (host_value) and
tests/cehvi_reference.py (believed_feasible), all imported unchanged.

Member e is M + K GPs.  With chebei_reference's s_j, tau_j, sigma_j, L and the member's incumbent g (finite):
    z_j(t) = (t - s_j) / tau_j,  (log Phi_j, r_j) = log_cdf_parts(z_j),  log f(t) = sum_j log Phi_j in the order of j
    d_j    = g - s_j (rounded once),  u = g - t the OFFSET below the incumbent,  z_j = (d_j - u) / tau_j
    ell    = min(1 / sum_j (r_j(g) / tau_j), max_j tau_j)      the decay length of f below g, capped where f does not decay at g
    U      = max(min_j (d_j + 38 tau_j), 40 ell) = g - Lambda,  Lambda = min(L, g - 40 ell)
    LA     = log integral over 0 <= u <= U of f
    dLA/dmu_j = -a_j <r_j / tau_j>,  dLA/dvar_j = -(a_j / (2 sigma_j)) <z_j r_j / tau_j>,  <.> the f-weighted mean over [Lambda, g]
by the FIXED quadrature of csrc/logchebei1.hip, formed in offsets so that no node is lost where ell is below an ulp of g:
position 14 j + i holds d_j - c_i tau_j, position 14 M + i holds kappa_i ell (LADDER), all clamped to [0, U]; then U, then 0;
sorted ascending, ties by position; 8 Gauss-Legendre nodes per panel;
lane l of sweep s owns node 64 s + l and keeps a running-maximum record (m, W, S[2 M]) of the terms log(weight) + log f; the 64
records merge by the butterfly xor 32 .. 1.  The pending points a member believes feasible (every constraint mean <= its threshold)
are the ones whose scalarised outcome may lower its incumbent.
    LL_e = LA_e + log F_{e,1} + ... + log F_{e,K},  value = m + log sum_e exp(LL_e - m) - log E,  m = max_e LL_e
"""
import collections

import numpy as np

import cehvi_reference as cv
import cei1_reference as cr
import chebei_reference as ch
import kg1_reference as kr
import log_ehvi_reference as lh
import logcei1_reference as lr

LD = ch.LD
# the ladder below the incumbent, in decay lengths: 14 rungs whose steps widen from a half to five
LADDER = (0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 8.0, 10.5, 13.0, 16.0, 20.0, 24.0, 29.0, 34.0)
REACH = 40.0
assert 14 * 8 + len(LADDER) + 2 <= 128

LogIntegral = collections.namedtuple("LogIntegral", "LA SM SV SVabs U ell breaks")
Result = collections.namedtuple("Result", "value grad log_factors members_grad incumbents")

host_value = lh.host_value


# ---- log Phi and phi / Phi over arrays: logcei1_reference.log_cdf_parts' operations, element by element ----
def log_cdf_parts_many(z, T):
    z = np.asarray(z, dtype=T)
    out_l, out_r = np.empty(z.shape, dtype=T), np.empty(z.shape, dtype=T)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        far = z < T(lr.FRACTION_BELOW)
        if far.any():
            a = -z[far]
            t = a.copy()
            for k in range(lr.FRACTION_TERMS, 1, -1):
                t = a + T(k) / t
            t1 = a + T(1) / t
            out_l[far] = -z[far] * z[far] / T(2) - lr._half_log_2pi(T) - np.log(t1)
            out_r[far] = t1
        neg = ~far & (z < 0)
        if neg.any():
            P = ch._erfc_nonneg_many(-z[neg] / np.sqrt(T(2)), T) / T(2)
            out_l[neg] = np.log(P)
            out_r[neg] = ch.pdf_many(z[neg], T) / P
        pos = ~far & ~neg
        if pos.any():
            q = ch._erfc_nonneg_many(z[pos] / np.sqrt(T(2)), T) / T(2)
            out_l[pos] = np.log1p(-q)
            out_r[pos] = ch.pdf_many(z[pos], T) / (T(1) - q)
    return out_l, out_r


def offsets(s, tau, g, T):
    """d_j = g - s_j, each rounded once: everything below is formed from these, never from g or s_j again"""
    return [T(g) - s[j] for j in range(len(s))]


def decay_rate(d, tau, T):
    """sum_j r_j(g) / tau_j in the order of j: the rate at which log f falls below g"""
    total = None
    for j in range(len(d)):
        _, r = lr.log_cdf_parts(d[j] / tau[j], T)
        term = r / tau[j]
        total = term if total is None else total + term
    return total


def decay_length(d, tau, T):
    """ell: f(t) <= f(g) exp((t - g) / (1 / sum_j r_j(g) / tau_j)) below g, f being log-concave; capped at the largest tau_j
    (where every r_j(g) underflows the rate is exactly 0 and 1 / 0 = infinity yields to the cap)"""
    with np.errstate(divide="ignore"):
        return min(T(1) / decay_rate(d, tau, T), max(tau))


def log_breakpoints(s, tau, g, T):
    """(U, ell, the 14 M + len(LADDER) + 2 breakpoints as OFFSETS u = g - t below the incumbent, sorted ascending, ties by
    position, the offsets d_j).  U = max(min_j (d_j + 38 tau_j), 40 ell) is g - Lambda."""
    d = offsets(s, tau, g, T)
    ell = decay_length(d, tau, T)
    U = max(min(d[j] + T(38) * tau[j] for j in range(len(d))), T(REACH) * ell)
    raw = []
    for j in range(len(d)):
        for c in ch.BREAKS:
            raw.append(min(max(d[j] + T(-c) * tau[j], T(0)), U))
    for kappa in LADDER:
        raw.append(min(max(T(kappa) * ell, T(0)), U))
    raw += [U, T(0)]
    order = sorted(range(len(raw)), key=lambda k: (raw[k], k))
    return U, ell, [raw[k] for k in order], d


def log_integrand(u, d, tau, T):
    """at the offsets u [n]: (log f [n], r_j / tau_j [M][n], z_j r_j / tau_j [M][n]) with z_j = (d_j - u) / tau_j"""
    logf, dm, dv = None, [], []
    for j in range(len(d)):
        z = (d[j] - u) / tau[j]
        l, r = log_cdf_parts_many(z, T)
        logf = l if logf is None else logf + l
        q = r / tau[j]
        dm.append(q)
        dv.append(z * q)
    return logf, dm, dv


def _nodes(bp, T):
    lo, hi = np.array(bp[:-1], dtype=T), np.array(bp[1:], dtype=T)
    half = T(0.5) * (hi - lo)
    mid = T(0.5) * (lo + hi)
    x, w = np.array(ch.GL8_X, dtype=T), np.array(ch.GL8_W, dtype=T)
    return (mid[:, None] + half[:, None] * x[None, :]).ravel(), (half[:, None] * w[None, :]).ravel()


def _merge(m, W, S, off):
    """one butterfly step over the 64 records (record_join: a record without a term yields to the other)"""
    lanes = np.arange(64)
    mb, Wb, Sb = m[lanes ^ off], W[lanes ^ off], S[:, lanes ^ off]
    with np.errstate(invalid="ignore", under="ignore"):
        top = np.maximum(m, mb)
        ea, eb = np.exp(m - top), np.exp(mb - top)
        both = np.isfinite(m) & np.isfinite(mb)
        only_b = ~np.isfinite(m) & np.isfinite(mb)
        Wn = np.where(both, W * ea + Wb * eb, np.where(only_b, Wb, W))
        Sn = np.where(both[None, :], S * ea[None, :] + Sb * eb[None, :], np.where(only_b[None, :], Sb, S))
        mn = np.where(both, top, np.where(only_b, mb, m))
    return mn, Wn, Sn


def log_integral(s, tau, g, T=LD):
    """the fixed quadrature in the device's order: LogIntegral(LA, <r_j / tau_j> [M], <z_j r_j / tau_j> [M], <|z_j| r_j / tau_j>
    [M] (the scale of the signed sum, by plain sums), U, ell, the sorted breakpoints)"""
    M = len(s)
    U, ell, bp, d = log_breakpoints(s, tau, g, T)
    t, wt = _nodes(bp, T)
    n = len(t)
    live = wt > 0
    logf, dm, dv = log_integrand(t[live], d, tau, T)
    with np.errstate(divide="ignore"):
        l_all = np.full(n, -np.inf, dtype=T)
        l_all[live] = np.log(wt[live]) + logf
    live = live & (l_all > -np.inf)
    d_all = np.zeros((2 * M, n), dtype=T)
    pos = np.flatnonzero(wt > 0)
    for j in range(M):
        d_all[2 * j, pos] = dm[j]
        d_all[2 * j + 1, pos] = dv[j]
    pad = ((n + 63) // 64) * 64
    l_pad, live_pad, d_pad = np.full(pad, -np.inf, dtype=T), np.zeros(pad, dtype=bool), np.zeros((2 * M, pad), dtype=T)
    l_pad[:n], live_pad[:n], d_pad[:, :n] = l_all, live, d_all
    m, W, S = np.full(64, -np.inf, dtype=T), np.zeros(64, dtype=T), np.zeros((2 * M, 64), dtype=T)
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        for row in range(pad // 64):
            sl = slice(64 * row, 64 * row + 64)
            l, on, dl = l_pad[sl], live_pad[sl], d_pad[:, sl]
            new = on & (l > m)
            old = on & ~new
            sc = np.where(new, np.exp(m - l), T(0))
            w = np.where(old, np.exp(l - m), T(0))
            W = np.where(new, W * sc + T(1), np.where(old, W + w, W))
            S = np.where(new[None, :], S * sc[None, :] + dl, np.where(old[None, :], S + w[None, :] * dl, S))
            m = np.where(new, l, m)
    for off in (32, 16, 8, 4, 2, 1):
        m, W, S = _merge(m, W, S, off)
    # the scale of the signed sums, by plain sums
    top = np.max(l_all[live])
    wts = np.exp(l_all[live] - top)
    keep = live[pos]
    scale = [np.sum(wts * np.abs(dv[j][keep])) / np.sum(wts) for j in range(M)]
    return LogIntegral(m[0] + np.log(W[0]), [S[2 * j, 0] / W[0] for j in range(M)], [S[2 * j + 1, 0] / W[0] for j in range(M)],
                       scale, U, ell, bp)


def log_coefficients(a, sg, I, T):
    """[dLA/dmu_0, dLA/dvar_0, ..., dLA/dmu_{M-1}, dLA/dvar_{M-1}]"""
    out = []
    for j in range(len(a)):
        out += [-T(a[j]) * I.SM[j], -(T(a[j]) / (T(2) * sg[j])) * I.SV[j]]
    return out


def log_value_at_moments(a, b, mus, variances, g, T=LD):
    """(LA, the 2 M coefficients, the LogIntegral) of one member from its M (mu, var), the scalarisation and the incumbent"""
    s, tau, sg = ch.scalarised_moments(a, b, mus, variances, T)
    I = log_integral(s, tau, g, T)
    return I.LA, log_coefficients(a, sg, I, T), I


_RULES = {}


def _gauss_legendre(nodes, T):
    """numpy's leggauss polished by Newton's iteration in T (chebei_reference.refined_value's)"""
    if (nodes, T) not in _RULES:
        x = np.array(np.polynomial.legendre.leggauss(nodes)[0], dtype=T)
        for it in range(4):
            p0, p1 = np.ones(nodes, dtype=T), x.copy()
            for k in range(2, nodes + 1):
                p0, p1 = p1, (T(2 * k - 1) * x * p1 - T(k - 1) * p0) / T(k)
            dp = T(nodes) * (x * p1 - p0) / (x * x - T(1))
            if it < 3:
                x = x - p1 / dp
        _RULES[(nodes, T)] = (x, T(2) / ((T(1) - x * x) * dp * dp))
    return _RULES[(nodes, T)]


def refined_log_value(a, b, mus, variances, g, T=LD, nodes=32):
    """the same quantities by an independent evaluation: every panel halved, a rule of `nodes` points per half, one plain
    max-shifted sum.  (LA, the 2 M coefficients, [the scale of each: |coefficient| for mu, the unsigned sum's for var])"""
    s, tau, sg = ch.scalarised_moments(a, b, mus, variances, T)
    _, _, bp, d = log_breakpoints(s, tau, g, T)
    x, w = _gauss_legendre(nodes, T)
    ts, ws = [], []
    for lo, hi in zip(bp[:-1], bp[1:]):
        if not hi > lo:
            continue
        mid = T(0.5) * (lo + hi)
        for u, v in ((lo, mid), (mid, hi)):
            half, c = T(0.5) * (v - u), T(0.5) * (u + v)
            if half > 0:
                ts.append(c + half * x)
                ws.append(half * w)
    t, wt = np.concatenate(ts), np.concatenate(ws)
    logf, dm, dv = log_integrand(t, d, tau, T)
    l = np.log(wt) + logf
    top = np.max(l)
    e = np.exp(l - top)
    W = np.sum(e)
    coef, scale = [], []
    for j in range(len(a)):
        cm = -T(a[j]) * (np.sum(e * dm[j]) / W)
        k = T(a[j]) / (T(2) * sg[j])
        coef += [cm, -k * (np.sum(e * dv[j]) / W)]
        scale += [abs(cm), k * (np.sum(e * np.abs(dv[j])) / W)]
    return top + np.log(W), coef, scale


# ---- members ----
class Member(object):
    """one member's M + K GPs conditioned on P, the pending points it believes feasible and their believed outcomes"""

    def __init__(self, gps, M, taus, P, T=LD):
        self.T, self.M, self.gps, self.taus = T, M, gps, [float(t) for t in taus]
        self.K = len(self.taus)
        assert len(gps) == M + self.K
        self.P = np.asarray(P, dtype=np.float64).reshape(-1, np.asarray(gps[0].X).shape[1])
        self.bases = [cr.base_model(g, T) for g in gps]
        self.models = [cr.conditioned(b, self.P) for b in self.bases]
        self.mask, self.constraint_means = cv.believed_feasible(self.bases[M:], self.P, self.taus)
        self.outcomes = [cr.mean_at(b, self.P) for b in self.bases[:M]] if len(self.P) else []

    def incumbent(self, scal, best):
        a, b = ch.split(scal)
        g = self.T(best)
        for v, ok in zip(ch.scalarised_outcomes(a, b, self.outcomes, self.T), self.mask):
            if ok and np.isfinite(v):
                g = min(g, v)
        return g

    def evaluate(self, x, scal, best):
        """([LA_e, log F_1 .. log F_K], g_e, the 2 M coefficients, the incumbent) at x"""
        T, M = self.T, self.M
        a, b = ch.split(scal)
        mo = [cr.moments(m, bs, x) for m, bs in zip(self.models, self.bases)]
        g = self.incumbent(scal, best)
        LA, c, _ = log_value_at_moments(a, b, [m[0] for m in mo[:M]], [m[1] for m in mo[:M]], g, T)
        grad = np.zeros(len(x), dtype=T)
        for j in range(M):
            grad = grad + (c[2 * j] * mo[j][2] + c[2 * j + 1] * mo[j][3])
        vals = [LA]
        for k, tau in enumerate(self.taus):
            l, gl, _ = lr.role_log(T, *mo[M + k], tau, 1 + k)
            vals.append(l)
            grad = grad + gl
        return vals, grad, c, g


def ensemble(gps, M, taus, P, T=LD):
    return [Member(row[:M + len(taus)], M, taus, P, T) for row in gps]


def evaluate(members, x, scal, best):
    T = members[0].T
    Ls, gs, logs, incs = [], [], [], []
    for m, bst in zip(members, best):
        vals, g, _, inc = m.evaluate(x, scal, bst)
        L = vals[0]
        for v in vals[1:]:
            L = L + v
        Ls.append(L)
        gs.append(g)
        logs.append(vals)
        incs.append(inc)
    top = max(Ls)
    w = [np.exp(L - top) for L in Ls]
    W, num = w[0], w[0] * gs[0]
    for we, ge in zip(w[1:], gs[1:]):
        W, num = W + we, num + we * ge
    return Result(top + np.log(W) - np.log(T(len(members))), num / W, logs, gs, incs)


# ---- what an entry point refuses before a handle is touched, in the header's order ----
def refusal(M, K, E, scal, thresholds, best):
    """None, or (error, payload index) of the first refusal of moe_log_ei_chebyshev_constrained_mcmc's value checks"""
    if not 2 <= M <= 8:
        return ("bounds", "num_objectives")
    if not 0 <= K <= 8:
        return ("bounds", "num_constraints")
    if E < 1 or E * (M + K) > 1024:
        return ("bounds", "num_mcmc")
    scal = np.asarray(scal, dtype=np.float64).reshape(-1, 2 * M)
    for r, row in enumerate(scal):
        for k, v in enumerate(row):
            if not np.isfinite(v) or (k < M and not v > 0):
                return ("invalid", r * 2 * M + k)
    for k, v in enumerate(np.asarray(thresholds, dtype=np.float64).ravel()):
        if not np.isfinite(v):
            return ("invalid", k)
    for i, v in enumerate(np.asarray(best, dtype=np.float64).ravel()):
        if not np.isfinite(v):
            return ("invalid", i)
    return None


# ---- the problems of tests/test_gpu_log_chebei.py ----
# Case: chebei_reference's fields and K constraints with thresholds taus; drop: every incumbent is lowered by that much; far: the
# first threshold is lowered by that many prior deviations; ld_diff: the worst float64-against-long-double difference of LA, LL,
# the value (absolute: they are logs) and of the gradient relative to its largest entry, as tests/test_log_chebei_reference.py
# measured it
Case = collections.namedtuple("Case", "name seed M E K d n p C kind taus drop far ld_diff")
Problem = collections.namedtuple("Problem", "name M K gps taus scal best points pending")
TAUS = {0: (), 1: (0.0,), 2: (0.1, 0.0), 8: (0.3,) * 8}
STALL_DROP = 60.0
STALL_FAR = 40.0
# The ascent has no line search: step i moves by pre_mult (i + 1)^-gamma grad, capped at half the distance to the bound, and climbs
# for certain only where pre_mult is below 1 / L, L the largest curvature of the objective (log_ehvi3_reference.STALL_GD's argument).
# Here LA behaves like -sum_j z_j^2 / 2 with z_j = (Delta / a_j) / sigma_j(x): Delta = 60 and a_j = w_j / 2 of order 0.15 give 400 /
# sigma_j, so the curvature along x is about 3 (400^2 / sigma^4) |grad sigma|^2 per objective -- sigma from 0.5, |grad sigma| of
# order 1 and three objectives give L of order 2e7.  pre_mult = 1e-8 lies a factor 5 below 1 / L; test_gpu_cei1.py's 1.0 would make
# every step the cap, whatever the gradient.
STALL_GD = (12, 6, 2, 0, 0.7, 1e-8, 0.5, 1e-10)


def _grid(E, G, n):
    return tuple(tuple(n for _ in range(G)) for _ in range(E))


CASES = [
    Case("log_m2_e1_k0_d3_n20_p0", 1, 2, 1, 0, 3, _grid(1, 2, 20), 0, 8, "plain", TAUS[0], 0.0, 0.0, 4.3e-14),
    Case("log_m3_e1_k0_d3_n20_p2", 2, 3, 1, 0, 3, _grid(1, 3, 20), 2, 8, "plain", TAUS[0], 0.0, 0.0, 8.1e-13),
    Case("log_m5_e1_k0_d3_n20_p2", 3, 5, 1, 0, 3, _grid(1, 5, 20), 2, 8, "plain", TAUS[0], 0.0, 0.0, 7.9e-15),
    Case("log_m8_e1_k0_d3_n20_p0", 4, 8, 1, 0, 3, _grid(1, 8, 20), 0, 8, "plain", TAUS[0], 0.0, 0.0, 1.4e-14),
    Case("log_m4_e1_k2_d3_n20_p2", 11, 4, 1, 2, 3, _grid(1, 6, 20), 2, 8, "plain", TAUS[2], 0.0, 0.0, 2.6e-14),
    Case("log_m8_e2_k8_d3_n20_p2", 12, 8, 2, 8, 3, _grid(2, 16, 20), 2, 8, "plain", TAUS[8], 0.0, 0.0, 6.1e-14),
    # the exact-zero regime: the plain form is 0 with a zero gradient at every candidate
    Case("log_m3_e1_k0_d3_n20_p0_stall", 7, 3, 1, 0, 3, _grid(1, 3, 20), 0, 8, "plain", TAUS[0], STALL_DROP, 0.0, 1.6e-9),
    Case("log_m3_e1_k1_d3_n20_p0_stall_far", 7, 3, 1, 1, 3, _grid(1, 4, 20), 0, 8, "plain", TAUS[1], STALL_DROP, STALL_FAR, 3.8e-9),
    Case("log_m3_e1_k0_d3_floor", 5, 3, 1, 0, 3, ((20, 1, 20),), 0, 8, "floor", TAUS[0], 0.0, 0.0, 4.1e-14),
    Case("log_m4_e1_k0_d3_n20_decades", 6, 4, 1, 0, 3, _grid(1, 4, 20), 0, 8, "decades", TAUS[0], 0.0, 0.0, 3.7e-15),
    Case("log_m3_e3_k0_d3_n20_130_300_p3", 9, 3, 3, 0, 3, ((20, 130, 300), (130, 300, 20), (300, 20, 130)), 3, 8, "plain", TAUS[0], 0.0,
         0.0, 8.6e-13),
    Case("log_m2_e1_k0_d20_n300_p2", 10, 2, 1, 0, 20, ((300, 300),), 2, 8, "plain", TAUS[0], 0.0, 0.0, 3.1e-15),
]
ENSEMBLE = "log_m3_e3_k0_d3_n20_130_300_p3"
STALL = "log_m3_e1_k0_d3_n20_p0_stall"
STALL_FAR_CASE = "log_m3_e1_k1_d3_n20_p0_stall_far"
BATCH_K2 = "log_m4_e1_k2_d3_n20_p2"
# the believed-and-feasible rule, E = 2, p = 4, K = 1: member 0 believes pending point 0 infeasible and point 1 feasible (the
# constraint GP's observations say so), both lie below its observed incumbent; member 1 believes both feasible
BELIEVED = Case("log_m2_e2_k1_d3_n20_p4_believed", 21, 2, 2, 1, 3, _grid(2, 3, 20), 4, 8, "believed", TAUS[1], 0.0, 0.0, 1.3e-14)
# the floor case with every incumbent 0.5 lower: at candidate 0, the noise-free observation's own point, sigma_1 is the floor and
# s_1 = 0.63 lies ABOVE the incumbent 0.43, so that z_1(g) is about -1.7e14, ell about 1e-29 and LA about -1e28 -- a candidate on
# a noise-free observation or on a pick of a greedy batch.  Formed as g - kappa ell, every breakpoint would round to g.
FLOOR_ABOVE = Case("log_m3_e1_k0_d3_floor_above", 5, 3, 1, 0, 3, ((20, 1, 20),), 0, 8, "floor", TAUS[0], 0.5, 0.0, 0.0)
MANY = Case("log_m8_e64_k8_d3_n4_p0", 31, 8, 64, 8, 3, _grid(64, 16, 4), 0, 2, "plain", TAUS[8], 0.0, 0.0, 0.0)
ALL_CASES = CASES + [BELIEVED]
# ---- the cases of tests/test_gpu_chebei_edges.py ----
TAUS.update({3: (0.1, 0.0, 0.2), 5: (0.1, 0.0, 0.2, -0.1, 0.3)})
# M = 6 and M = 7 (100 and 114 breakpoints, 792 and 904 nodes; LogStripRecord<12> and <14>), K = 3 and K = 5, an odd dimension
# under two members
M67 = [
    Case("log_m6_e2_k3_d7_n20_p3", 51, 6, 2, 3, 7, _grid(2, 9, 20), 3, 6, "plain", TAUS[3], 0.0, 0.0, 4.4e-14),
    Case("log_m7_e2_k5_d3_n20_p2", 52, 7, 2, 5, 3, _grid(2, 12, 20), 2, 6, "plain", TAUS[5], 0.0, 0.0, 3.1e-14),
    Case("log_m6_e1_k0_d3_n20_p0", 53, 6, 1, 0, 3, _grid(1, 6, 20), 0, 6, "plain", TAUS[0], 0.0, 0.0, 8.3e-14),
    Case("log_m7_e1_k0_d3_n20_p0", 54, 7, 1, 0, 3, _grid(1, 7, 20), 0, 6, "plain", TAUS[0], 0.0, 0.0, 1.5e-14),
]
# the incumbent 50 above the observed one: every r_j(g) underflows, the rate is exactly 0 and ell is the cap max_j tau_j
ABOVE_RAISE = 50.0
ABOVE = [
    Case("log_m3_e1_k0_d3_n20_p0_above", 55, 3, 1, 0, 3, _grid(1, 3, 20), 0, 6, "plain", TAUS[0], -ABOVE_RAISE, 0.0, 6.4e-14),
    Case("log_m6_e1_k0_d3_n20_p0_above", 56, 6, 1, 0, 3, _grid(1, 6, 20), 0, 6, "plain", TAUS[0], -ABOVE_RAISE, 0.0, 2.8e-14),
]
# a live member beside one whose incumbent is lowered by STALL_DROP (kind mixed: member 1; mixed_swapped: the same two members in
# the other order): the stalled member's weight exp(LL - m) is exactly 0.  ld_diff covers the stalled member's LA, of order -1e6;
# MIXED_LIVE[name] is the same figure without that member's group values, which is what the value, the gradient and the live
# member's group values are held to
MIXED = [
    Case("log_m3_e2_k0_d3_n20_p0_mixed", 57, 3, 2, 0, 3, _grid(2, 3, 20), 0, 6, "mixed", TAUS[0], STALL_DROP, 0.0, 8.5e-9),
    Case("log_m3_e2_k0_d3_n20_p0_mixed_swapped", 57, 3, 2, 0, 3, _grid(2, 3, 20), 0, 6, "mixed_swapped", TAUS[0], STALL_DROP, 0.0, 8.5e-9),
    Case("log_m3_e2_k1_d3_n20_p0_mixed", 58, 3, 2, 1, 3, _grid(2, 4, 20), 0, 6, "mixed", TAUS[1], STALL_DROP, 0.0, 1.7e-9),
    Case("log_m3_e2_k1_d3_n20_p0_mixed_swapped", 58, 3, 2, 1, 3, _grid(2, 4, 20), 0, 6, "mixed_swapped", TAUS[1], STALL_DROP, 0.0, 1.7e-9),
]
MIXED_LIVE = {"log_m3_e2_k0_d3_n20_p0_mixed": 7.2e-15, "log_m3_e2_k0_d3_n20_p0_mixed_swapped": 7.2e-15,
              "log_m3_e2_k1_d3_n20_p0_mixed": 2.4e-15, "log_m3_e2_k1_d3_n20_p0_mixed_swapped": 2.4e-15}


def stalled_member(c):
    return {"mixed": 1, "mixed_swapped": 0}[c.kind]


# 64 pending points: member 0 believes its lowest believed outcome, point 62, infeasible, so that its incumbent is its second
# lowest, point 63; member 1 believes all feasible and its lowest is point 40; every incumbent lies above every believed outcome
P64 = Case("log_m3_e2_k1_d3_n20_p64", 59, 3, 2, 1, 3, _grid(2, 4, 20), 64, 2, "p64", TAUS[1], 0.0, 0.0, 3.3e-12)
P64_SLOTS = ((0, 0, 62), (0, 1, 63), (1, 0, 40))
# the believed-and-feasible rule inside a greedy batch: member 0's constraint GP observes +0.5 on one half of the box and -0.5 on
# the other, member 1's -0.5 everywhere; every incumbent is HIGH_BEST, above every outcome a member can believe, so that what a
# member believes feasible among the pending points and the picks decides its incumbent
HALF = Case("log_m2_e2_k1_d3_n20_p2_half", 60, 2, 2, 1, 3, _grid(2, 3, 20), 2, 4, "half", TAUS[1], 0.0, 0.0, 5.6e-14)
HIGH_BEST = 2.0
EDGE_CASES = M67 + ABOVE + MIXED + [P64, HALF]


def case(name):
    return next(c for c in ALL_CASES + EDGE_CASES + [MANY, FLOOR_ABOVE] if c.name == name)


def make_problem(c):
    """chebei_reference's problem of the same seed and kind over M + K GPs per member; the GPs behind the first M are the
    constraints"""
    base = ch.Case(c.name, c.seed, c.M + c.K, c.E, c.d, c.n, c.p, c.C, c.kind if c.kind in ("floor", "decades") else "plain", 0.0)
    if c.kind in ("floor", "decades"):
        p = ch.make_problem(base._replace(M=c.M))
        gps, scal, best = p.gps, p.scal[0], list(p.best[0])
    else:
        rng = np.random.default_rng(9700 + c.seed)
        gps = ch._random_gps(rng, base)
        p = ch.make_problem(base)
        w = np.random.default_rng(4100 + c.seed).exponential(size=c.M) + 0.2
        scal = ch.scalarisation(w / w.sum(), [ch.IDEAL] * c.M, [ch.NADIR] * c.M)
        best = ch.observed_best([row[:c.M] for row in gps], scal)
    taus = list(c.taus)
    if c.far:
        taus[0] = taus[0] - c.far * float(np.sqrt(np.asarray(gps[0][c.M].hyper).ravel()[0]))
    if c.kind.startswith("mixed"):
        best = [best[0]] + [v - c.drop for v in best[1:]]
    else:
        best = [v - c.drop for v in best]
    pending = p.pending
    if c.kind == "believed":
        pending, gps, best = _believed(c, gps, p, scal)
    elif c.kind == "mixed_swapped":
        gps, best = gps[::-1], best[::-1]
    elif c.kind == "p64":
        placed = ch.place_pending(rng, [row[:c.M] for row in gps], scal, c.p, c.d, P64_SLOTS)
        pending, gps, best = _believed(c, gps, p._replace(pending=placed), scal)
    elif c.kind == "half":
        gps, best = _believed_half(c, gps, p.pending, scal), [HIGH_BEST] * c.E
    return Problem(c.name, c.M, c.K, gps, tuple(taus), np.asarray(scal, dtype=np.float64), [float(v) for v in best], p.points,
                   np.ascontiguousarray(pending))


def _believed(c, gps, p, scal):
    """member 0's constraint GP observes +0.5 at the pending point whose believed outcome is its lowest and -0.5 at the others,
    member 1's -0.5 at all four; the incumbents lie above every believed outcome, so that what a member believes feasible decides
    its incumbent"""
    pending = np.ascontiguousarray(p.pending)
    gps = [list(row) for row in gps]
    out = [ch.scalarised_outcomes(*ch.split(scal), ch.Member(row[:c.M], pending, np.float64).outcomes, np.float64) for row in gps]
    for e in range(c.E):
        g = gps[e][c.M]
        y = np.full((c.p, 1), -0.5)
        if e == 0:
            y[int(np.argmin(out[0])), 0] = 0.5
        gps[e][c.M] = ch.GP(g.cov_type, g.hyper, pending.copy(), y, [1e-6], ())
    best = [float(max(max(o) for o in out)) + 0.05] * c.E
    return pending, gps, best


def half_region(c, gps, pending, scal):
    """(k, upper): the half of the box, cut at 0.5 along coordinate k, that member 0 of the `half` problem believes infeasible.
    It is the half that holds, deepest inside it, the best of 64 probe points under the objectives alone (K = 0, float64, the
    problem's pending points, every incumbent HIGH_BEST): where the first picks of a batch go"""
    probes = np.random.default_rng(7300 + c.seed).uniform(0.05, 0.95, size=(64, c.d))
    ms = ensemble([row[:c.M] for row in gps], c.M, (), pending, np.float64)
    x = probes[int(np.argmax([float(evaluate(ms, q, scal, [HIGH_BEST] * c.E).value) for q in probes]))]
    k = int(np.argmax(np.abs(x - 0.5)))
    return k, bool(x[k] > 0.5)


def _believed_half(c, gps, pending, scal):
    """member 0's constraint GP observes +0.5 at its points inside half_region and -0.5 at the others, member 1's -0.5 at all;
    both with lengths of 0.6, so that the believed mean is a smooth step across the box"""
    k, upper = half_region(c, gps, pending, scal)
    gps = [list(row) for row in gps]
    for e in range(c.E):
        g = gps[e][c.M]
        X = np.asarray(g.X, dtype=np.float64)
        inside = (X[:, k] > 0.5) == upper
        y = np.where(inside & (e == 0), 0.5, -0.5).reshape(-1, 1)
        gps[e][c.M] = ch.GP(g.cov_type, np.array([float(np.asarray(g.hyper).ravel()[0])] + [0.6] * c.d), X.copy(), y, [1e-2], ())
    return gps


def batch_rounds(p, q):
    """q scalarisations, the problem's own first, and the incumbents [q][E] of the `half` problem's batch"""
    rng = np.random.default_rng(8805)
    rows = [p.scal]
    for _ in range(q - 1):
        w = rng.exponential(size=p.M) + 0.2
        rows.append(ch.scalarisation(w / w.sum(), [ch.IDEAL] * p.M, [ch.NADIR] * p.M))
    return np.array(rows), np.full((q, len(p.gps)), HIGH_BEST)


_WANT = {}


def expected(c, T=LD, members=None):
    """(problem, [Result per candidate]) in the arithmetic of T, once per process"""
    key = (c.name, T, members)
    if key not in _WANT:
        p = make_problem(c)
        idx = range(len(p.gps)) if members is None else members
        ms = ensemble([p.gps[e] for e in idx], p.M, p.taus, p.pending, T)
        _WANT[key] = (p, [evaluate(ms, x, p.scal, [p.best[e] for e in idx]) for x in p.points])
    return _WANT[key]


def ld_difference(c, without=None):
    """the worst float64-against-long-double difference of a case: the value and every group value (absolute; `without`: but
    those of that member), the gradient relative to its largest entry"""
    _, hi = expected(c, LD)
    _, lo = expected(c, np.float64)
    worst = 0.0
    for h, l in zip(hi, lo):
        worst = max(worst, abs(float(h.value - LD(l.value))))
        worst = max(worst, max(abs(float(x - LD(y))) for e, (hv, lv) in enumerate(zip(h.log_factors, l.log_factors)) if e != without
                               for x, y in zip(hv, lv)))
        worst = max(worst, float(np.max(np.abs(h.grad - l.grad.astype(LD)))) / float(np.max(np.abs(h.grad))))
    return worst
