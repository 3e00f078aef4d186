"""The LOG of the two-objective constrained expected hypervolume improvement with pending points, averaged over an ensemble, restated
on the CPU (the checker of tests/test_gpu_log_ehvi.py) in np.longdouble or float64, on top of tests/cehvi_reference.py (Member,
ensemble, make_problem, the M = 2 CASES, BELIEVED2: the members, their conditioning on the pending points, the believed-feasibility
mask and the join rule are that file's) and tests/logcei1_reference.py (log_h_parts, log_cdf_parts, role_log), all imported
unchanged.

With mu_r, var_r the posterior mean and the conditioned latent variance of objective r's GP at x and ONE floor,
sigma = sqrt(max(150 eps^2, var)); a member's front u_1 < ... < u_F' < r1, r2 > v_1 > ... > v_F', u_0 = -inf, u_{F'+1} = r1, v_0 = r2:
    lambda_r(t) = log sigma_r + log h(z),  z = (t - mu_r) / sigma_r,  (log h, lam, kap) = log_h_parts(z);  lambda_1(-inf) = -inf
    strip i:  D = lambda_1(u_i) - lambda_1(u_{i+1}), rho = exp(D);  log Delta = lambda_1(u_{i+1}) + log(1 - rho)  (log1p(-rho) for
              rho <= 1/2, log(-expm1(D)) above);  l_i = log Delta + lambda_2(v_i)
              dl/dmu_1 = -(lam_b - rho lam_a) / (sigma_1 (1 - rho)),  dl/dvar_1 = (kap_b - rho kap_a) / (2 sigma_1^2 (1 - rho)),
              dl/dmu_2 = -lam(v_i) / sigma_2,  dl/dvar_2 = kap(v_i) / (2 sigma_2^2)
              a strip that does not give D < 0 (rho = 1) carries weight 0 and is skipped
    L_e = m + log W,  m = max_i l_i,  w_i = exp(l_i - m),  W = sum_i w_i;  coefficients (sum_i w_i dl_i/d.) / W
    log F_k and its gradient: logcei1_reference.role_log with role k
    LL_e = L_e + log F_1 + ... + log F_K;  g_e = ((c_mu1 grad mu_1 + c_var1 grad var_1) + c_mu2 grad mu_2) + c_var2 grad var_2 + ...
    value = m + log W - log E over the members (m = max_e LL_e, w_e = exp(LL_e - m)),  grad = (sum_e w_e g_e) / W
A SHIFT (s, t) lowers the reference point and every point of the caller's front by s in both objectives and every threshold by t;
the members' factorisations are shared between the shifts, their masks and fronts are worked out anew (a believed outcome that the
lowered reference point leaves outside does not join).
"""
import collections
import copy
import math

import numpy as np

import cehvi_reference as ch
import cei1_reference as cr
import ehvi_reference as hr
import ei1_reference as er
import logcei1_reference as lr

LD = ch.LD
Result = collections.namedtuple("Result", "value grad log_factors coef args skipped")

SHIFTS = ((0.0, 0.0), (3.0, 0.0), (8.0, 2.0))


def log_strips(mu1, var1, mu2, var2, front, ref, T=LD):
    """(L, [dL/dmu1, dL/dvar1, dL/dmu2, dL/dvar2], the lowest z met, the strips skipped at rho = 1) of one member from its moments,
    its front [F][2] and r"""
    front = np.asarray(front, dtype=T).reshape(-1, 2)
    F = len(front)
    s1 = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), T(var1)))
    s2 = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), T(var2)))
    la, lam_a, kap_a = T(-np.inf), T(0), T(0)
    ls, ds, low, skipped = [], [], math.inf, 0
    for i in range(F + 1):
        zb = ((front[i, 0] if i < F else T(ref[0])) - T(mu1)) / s1
        lh, lam_b, kap_b = lr.log_h_parts(zb, T)
        lb = np.log(s1) + lh
        zq = ((T(ref[1]) if i == 0 else front[i - 1, 1]) - T(mu2)) / s2
        lh, lam_q, kap_q = lr.log_h_parts(zq, T)
        lq = np.log(s2) + lh
        low = min(low, float(zb), float(zq))
        D = la - lb
        if D < 0:
            rho = np.exp(D)
            if rho <= T(0.5):
                om, lom = T(1) - rho, np.log1p(-rho)
            else:
                om = -np.expm1(D)
                lom = np.log(om)
            ls.append((lb + lom) + lq)
            ds.append((-(lam_b - rho * lam_a) / (s1 * om), (kap_b - rho * kap_a) / (T(2) * (s1 * s1) * om), -lam_q / s2,
                       kap_q / (T(2) * (s2 * s2))))
        else:
            skipped += 1
        la, lam_a, kap_a = lb, lam_b, kap_b
    m = max(ls)
    w = [np.exp(l - m) for l in ls]
    W = sum(w[1:], w[0])
    c = [sum((wi * d[q] for wi, d in zip(w[1:], ds[1:])), w[0] * ds[0][q]) / W for q in range(4)]
    return m + np.log(W), c, low, skipped


def lane_replay(mu1, var1, mu2, var2, front, ref):
    """logehvi1_strip_kernel's reduction order replayed in float64 for one member and candidate: strip i belongs to lane i mod 64,
    the sweeps ascend, a lane's record (m, W) takes its strips by record_take's two branches, and the 64 records merge by the fixed
    butterfly (xor 32, 16, 8, 4, 2, 1; every pair counted once).  Returns the counts of what ran -- which branch decides nothing
    about the value, so nothing but such a count shows that a branch was reached:
        rho_low / rho_high / rho_one   strips with rho <= 1/2, above, and skipped at rho = 1 (with their indices in `skipped_at`)
        first / rescales / below       record_take: a lane's first strip; later strips above its running maximum (W and S are
                                       scaled by exp(m - l)); later strips at or below it (weight exp(l - m))
        later_sweeps                   (rescales, below) counted over the strips of the second and later sweeps alone -- a lane
                                       whose strip of the first sweep was skipped meets its FIRST strip there, which counts in neither
        won_low / won_high / empty     merges whose maximum is the lower lane's (ties included) / the upper lane's; merges in which
                                       a record holds no strip
        lane_spread / merge_spread     the largest |l - m| a record_take met after a lane's first strip, the largest |m_a - m_b| a
                                       merge of two records met
        zero_weights                   the scalings exp(.) of record_take and of the merges that came out exactly 0
        L                              m + log W of lane 0 at the end: the kernel's value in this order"""
    T = np.float64
    front = np.asarray(front, dtype=T).reshape(-1, 2)
    F = len(front)
    s1, s2 = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), T(var1))), np.sqrt(max(T(er.MIN_VAR_GRAD_EI), T(var2)))
    out = dict(rho_low=0, rho_high=0, rho_one=0, skipped_at=[], first=0, rescales=0, below=0, later_sweeps=[0, 0], won_low=0,
               won_high=0, empty=0, lane_spread=0.0, merge_spread=0.0, zero_weights=0)
    m, W = [-math.inf] * 64, [0.0] * 64
    la = T(-np.inf)
    with np.errstate(over="ignore", under="ignore"):
        for i in range(F + 1):
            lb = np.log(s1) + lr.log_h_parts(((front[i, 0] if i < F else T(ref[0])) - T(mu1)) / s1, T)[0]
            lq = np.log(s2) + lr.log_h_parts(((T(ref[1]) if i == 0 else front[i - 1, 1]) - T(mu2)) / s2, T)[0]
            D = la - lb
            la = lb
            if not D < 0:
                out["rho_one"] += 1
                out["skipped_at"].append(i)
                continue
            rho = np.exp(D)
            out["rho_low" if rho <= 0.5 else "rho_high"] += 1
            l = float((lb + (np.log1p(-rho) if rho <= 0.5 else np.log(-np.expm1(D)))) + lq)
            lane = i % 64
            if m[lane] == -math.inf:
                out["first"] += 1
                m[lane], W[lane] = l, 1.0
                continue
            out["lane_spread"] = max(out["lane_spread"], abs(l - m[lane]))
            if l > m[lane]:
                sc = math.exp(m[lane] - l)
                out["rescales"] += 1
                out["later_sweeps"][0] += i >= 64
                m[lane], W[lane] = l, W[lane] * sc + 1.0
            else:
                sc = math.exp(l - m[lane])
                out["below"] += 1
                out["later_sweeps"][1] += i >= 64
                W[lane] = W[lane] + sc
            out["zero_weights"] += sc == 0.0
    for off in (32, 16, 8, 4, 2, 1):
        nm, nW = list(m), list(W)
        for a in range(64):
            b = a ^ off
            if a > b:
                continue
            if m[a] == -math.inf or m[b] == -math.inf:
                out["empty"] += 1
                k = b if m[a] == -math.inf else a
                nm[a] = nm[b] = m[k]
                nW[a] = nW[b] = W[k]
                continue
            top = max(m[a], m[b])
            out["won_low" if m[a] >= m[b] else "won_high"] += 1
            out["merge_spread"] = max(out["merge_spread"], abs(m[a] - m[b]))
            ea, eb = math.exp(m[a] - top), math.exp(m[b] - top)
            out["zero_weights"] += (ea == 0.0) + (eb == 0.0)
            nm[a] = nm[b] = top
            nW[a] = nW[b] = W[a] * ea + W[b] * eb
        m, W = nm, nW
    out["later_sweeps"] = tuple(out["later_sweeps"])
    out["L"] = m[0] + math.log(W[0])
    return out


def member_replay(m, x):
    """lane_replay of a float64 ch.Member (M = 2) at x"""
    assert m.T is np.float64
    mo = [cr.moments(model, base, x) for model, base in zip(m.models[:2], m.bases[:2])]
    return lane_replay(mo[0][0], mo[0][1], mo[1][0], mo[1][1], m.front, m.ref)


def member_logs(m, x):
    """([L_e, log F_1 .. log F_K], g_e, the four coefficients, the lowest z or strip argument, strips skipped) of a ch.Member (M = 2)
    at x"""
    T = m.T
    mo = [cr.moments(model, base, x) for model, base in zip(m.models[:2], m.bases[:2])]
    L, c, low, skipped = log_strips(mo[0][0], mo[0][1], mo[1][0], mo[1][1], m.front, m.ref, T)
    g = ((c[0] * mo[0][2] + c[1] * mo[0][3]) + c[2] * mo[1][2]) + c[3] * mo[1][3]
    vals = [L]
    for k, (model, base, tau) in enumerate(zip(m.models[2:], m.bases[2:], m.taus)):
        l, gl, z = lr.role_log(T, *cr.moments(model, base, x), tau, 1 + k)
        vals.append(l)
        g = g + gl
        low = min(low, float(z))
    return vals, g, c, low, skipped


def evaluate(members, x):
    """Result of the ensemble at x"""
    T = members[0].T
    Ls, gs, logs, coefs, lows, skipped = [], [], [], [], [], 0
    for m in members:
        vals, g, c, low, sk = member_logs(m, x)
        L = vals[0]
        for v in vals[1:]:
            L = L + v
        Ls.append(L)
        gs.append(g)
        logs.append(vals)
        coefs.append(c)
        lows.append(low)
        skipped += sk
    top = max(Ls)
    w = [np.exp(L - top) for L in Ls]
    W, num = w[0], w[0] * gs[0]
    for we, ge in zip(w[1:], gs[1:]):
        W, num = W + we, num + we * ge
    return Result(top + np.log(W) - np.log(T(len(members))), num / W, logs, coefs, lows, skipped)


def host_value(log_factors):
    """the documented rule on the host in float64: log_factors [E][1 + K][C] -> value [C]"""
    E, G, n = log_factors.shape
    out = np.zeros(n)
    for i in range(n):
        Ls = []
        for e in range(E):
            L = float(log_factors[e, 0, i])
            for k in range(1, G):
                L = L + float(log_factors[e, k, i])
            Ls.append(L)
        m = max(Ls)
        W = math.exp(Ls[0] - m)
        for L in Ls[1:]:
            W = W + math.exp(L - m)
        out[i] = m + math.log(W) - math.log(float(E))
    return out


# ---- the cases of tests/test_gpu_log_ehvi.py (tests/test_log_ehvi_reference.py qualifies them on the CPU) ----
Case = ch.Case
_grid = ch._grid


def _own(K, F, seed, p=3, C=5, d=3):
    return Case("log_e1_k%d_d%d_n20_p%d_f%d" % (K, d, p, F), seed, 2, 1, K, d, _grid(1, 2 + K, 20), p, F, ch.TAUS[K] if K else (), C, None, 0.0)


# a sweep of 64 strips filled exactly (F = 63) and the next one started (F = 64: 65 strips); no constraints at F in {0, 2, 65}
OWN_CASES = [_own(1, 63, 301), _own(1, 64, 302), _own(0, 0, 303), _own(0, 2, 304), _own(0, 65, 305)]
# F = 960 and 64 pending points whose believed outcomes all join without evicting: cap 1024, 1025 strips at shift 0 (a lowered
# reference point leaves the outcomes outside: 961 strips).  Two candidates: 1025 strips of 400-term fractions each.
FULL = Case("log_e1_k0_d3_n20_p64_f960", 306, 2, 1, 0, 3, _grid(1, 2, 20), 64, 960, (), 2, None, 0.0)
# a front of three whose middle u exceeds its neighbour by one unit in the last place: the rho = 1 strip
ULP = Case("log_e1_k1_d3_n20_p0_f3_ulp", 307, 2, 1, 1, 3, _grid(1, 3, 20), 0, 3, ch.TAUS[1], 5, None, 0.0)
# candidates 0 and 1 on sampled points of the noise-free GP of objective 1: the floor
FLOOR = Case("log_e1_k1_d3_n20_p0_f2_floor", 308, 2, 1, 1, 3, _grid(1, 3, 20), 0, 2, ch.TAUS[1], 5, None, 0.0)
# At a sampled point of a noise-free GP below a lowered reference point every edge lies 1e14 floored deviations BELOW the mean: the
# value is of order -1e28 and dl/dvar of order 1e57 multiplies a grad var that is 0 up to rounding, which float64 and long double
# round differently -- such a case-shift does not qualify.  The floor case runs under shifts that keep the reference point above
# the means instead (every threshold still lowered).
FLOOR_SHIFTS = ((0.0, 0.0), (0.3, 0.0), (0.6, 2.0))

M2_CASES = [c for c in ch.CASES if c.M == 2]  # (E = 3 with n = (20, 130, 300) at F = 65, K = 1 and d = 10 at F = 2 among them)
# cehvi_reference.EDGE_CASES, named one by one: E = 2 with K = 2 (d = 13, rows that differ per role and member) and with K = 8,
# the thresholds all distinct -- tests/test_log_ehvi_reference.py qualifies them against exchanges of GPs and thresholds
MIXED = [ch.MIXED2, ch.MIXED2_K8]
# candidate 0 on a sampled point of the noise-free GP of constraint 1 whose observation lies 0.2 BELOW tau_1: logehvi1_feas_kernel's
# floor, log F_1 = 0 there.  It is cehvi_reference.FLOOR2 without its candidate on the infeasible side, where the mean lies 1e14
# floored deviations above tau and log F_1 is of order -1e28 with a derivative by var of order 1e57 against a grad var that is 0
# up to rounding: float64 and long double do not agree there and the candidate does not qualify (FLOOR_SHIFTS' reason).  A lowered
# threshold would put candidate 0 on that side, so this case's shifts lower the reference point and the front alone.
CFLOOR = ch.FLOOR2._replace(name="log_e1_k2_d3_n20_p3_f2_constraint_floor", checked=None, ld_diff=0.0)
CFLOOR_SHIFTS = ((0.0, 0.0), (3.0, 0.0), (8.0, 0.0))
# The log-strip kernel's per-lane branches (lane_replay counts them; tests/test_log_ehvi_reference.py asserts the counts), E = 2,
# K = 1.  LANES: F = 200 and three pending points, four sweeps of a front that differs per member; the objective GPs observe with
# noise 1e-6 and candidates 0 and 1 lie 0.01 from sampled points, where the deviations are so small that under shift 8 the strips'
# logs spread by far more than 745 (exp of the difference is exactly 0) within a lane and across a merge.  ULP64: a front of 70
# whose points 63 and 64 are a unit in the last place apart in u -- the rho = 1 strip is strip 64, lane 0 of the second sweep,
# whose left edge comes through the carry.  ULP_LAST: F = 64 and u_63 a unit in the last place below r1 -- the rho = 1 strip is the
# last one, the second sweep's only strip.
LANES = Case("log_e2_k1_d3_n20_p3_f200_lanes", 311, 2, 2, 1, 3, _grid(2, 3, 20), 3, 200, ch.TAUS[1], 5, None, 0.0)
ULP64 = Case("log_e2_k1_d3_n20_p0_f70_ulp64", 312, 2, 2, 1, 3, _grid(2, 3, 20), 0, 70, ch.TAUS[1], 5, None, 0.0)
ULP_LAST = Case("log_e2_k1_d3_n20_p0_f64_ulp_last", 313, 2, 2, 1, 3, _grid(2, 3, 20), 0, 64, ch.TAUS[1], 5, None, 0.0)
LANE_CASES = [LANES, ULP64, ULP_LAST]
LANES_NOISE, LANES_OFFSET, LANES_ROWS = 1e-6, 0.01, (3, 7)
# A member whose weight underflows, E = 2, K = 1: member 1's constraint GP observes values HOPELESS_LEVEL above tau with noise 1e-2
# under length scales that span the cube, so that its log feasibility lies more than 800 below member 0's total at every candidate
# and exp(LL_1 - m) is exactly 0 in logehvi1_combine_kernel's member log-sum-exp.
HOPELESS = Case("log_e2_k1_d3_n20_p3_f2_hopeless", 314, 2, 2, 1, 3, _grid(2, 3, 20), 3, 2, ch.TAUS[1], 5, None, 0.0)
HOPELESS_LEVEL, HOPELESS_GAP = 3.0, -800.0
EDGE_CASES = MIXED + [CFLOOR] + LANE_CASES + [HOPELESS]
ALL_CASES = M2_CASES + OWN_CASES + [FULL, ULP, FLOOR] + EDGE_CASES
BELIEVED2 = ch.BELIEVED2


def shifts_of(c):
    return {FLOOR.name: FLOOR_SHIFTS, CFLOOR.name: CFLOOR_SHIFTS}.get(c.name, SHIFTS)


CASE_SHIFTS = [(c, s) for c in ALL_CASES for s in shifts_of(c)]


def case(name):
    return next(c for c in ALL_CASES + [BELIEVED2] if c.name == name)


def _full_problem(c):
    """objectives that rise and fall along the first coordinate, 64 pending points along it whose believed outcomes are mutually
    non-dominated, and 15 front points strictly between every two neighbouring outcomes (and 15 in front of the first): 960"""
    rng = np.random.default_rng(12400 + c.seed)
    length = 1.0  # (long enough for posterior means that follow the observations' slope from one end of the cube to the other)
    X = rng.uniform(0, 1, size=(20, c.d))
    gps = [[ch.GP(ch.MATERN if r == 0 else ch.SE, np.array([1.3] + [length] * c.d) * (1.0 + 0.15 * r), X.copy(),
                  ((1.0 - 2.0 * r) * (X[:, :1] - 0.5) + 0.01 * rng.normal(size=(20, 1))), [1e-2], ()) for r in range(2)]]
    pending = np.full((c.p, c.d), 0.5)
    pending[:, 0] = np.linspace(0.1, 0.9, c.p)
    bases = [cr.base_model(g, np.float64) for g in gps[0]]
    a = np.asarray(cr.mean_at(bases[0], pending), dtype=np.float64)
    b = np.asarray(cr.mean_at(bases[1], pending), dtype=np.float64)
    assert np.all(np.diff(a) > 1e-4) and np.all(np.diff(b) < -1e-4)
    pts = []
    per = c.F // c.p
    for j in range(c.p):
        lo_u, hi_u = (a[0] - 0.2, a[0]) if j == 0 else (a[j - 1], a[j])
        lo_v, hi_v = (b[0], b[0] + 0.2) if j == 0 else (b[j], b[j - 1])
        t = (np.arange(per) + 1.0) / (per + 1.0)
        pts.extend(zip(lo_u + t * (hi_u - lo_u), hi_v - t * (hi_v - lo_v)))
    front = np.array(pts, dtype=np.float64).reshape(-1, 2)
    assert len(front) == c.F and np.all(np.diff(front[:, 0]) > 0) and np.all(np.diff(front[:, 1]) < 0)
    points = rng.uniform(0.1, 0.9, size=(c.C, c.d))
    return ch.Problem(c.name, 2, gps, [], ch.REF2, np.ascontiguousarray(front), points, pending, tuple(range(c.C)))


def _one_ulp(c, front, ref):
    """the front of ULP64 / ULP_LAST with its two neighbouring edges a unit in the last place apart (again, after a shift)"""
    if c.name == ULP64.name:
        front[64, 0] = np.nextafter(front[63, 0], np.inf)
        assert front[63, 0] < front[64, 0] < front[65, 0]
    else:
        front[63, 0] = np.nextafter(ref[0], -np.inf)
        assert front[62, 0] < front[63, 0] < ref[0]
    return np.ascontiguousarray(front)


def make_problem(c):
    """ch.make_problem, with the constructions of this file"""
    if c.name == FULL.name:
        return _full_problem(c)
    if c.name == CFLOOR.name:
        p = ch.make_problem(ch.FLOOR2)
        points = p.points.copy()
        points[1] = 0.5 * (points[2] + points[3])  # (an ordinary point in place of the infeasible side's)
        return p._replace(name=c.name, points=points, checked=tuple(range(c.C)))
    p = ch.make_problem(c)
    if c.name == ULP.name:
        front = np.array([(-0.2, 0.4), (np.nextafter(-0.2, 1.0), 0.1), (0.3, -0.3)])
        p = p._replace(front=np.ascontiguousarray(front))
    if c.name in (ULP64.name, ULP_LAST.name):
        p = p._replace(front=_one_ulp(c, p.front.copy(), p.ref))
    if c.name == HOPELESS.name:
        rng = np.random.default_rng(c.seed)
        g = p.gps[1][2]
        y = p.taus[0] + HOPELESS_LEVEL + 0.01 * rng.normal(size=np.asarray(g.y).shape)
        far = ch.GP(ch.SE, np.array([1.3, 3.0, 3.0, 3.0]), g.X, y, [1e-2], ())
        p = p._replace(gps=[p.gps[0], list(p.gps[1][:2]) + [far]])
    if c.name == LANES.name:
        gps = [[ch.GP(g.cov_type, g.hyper, g.X, g.y, [LANES_NOISE], ()) for g in row[:2]] + list(row[2:]) for row in p.gps]
        points = p.points.copy()
        X = p.gps[0][0].X
        points[0], points[1] = X[LANES_ROWS[0]] + LANES_OFFSET, X[LANES_ROWS[1]] - LANES_OFFSET
        p = p._replace(gps=gps, points=points)
    if c.name == FLOOR.name:
        row = list(p.gps[0])
        g = row[0]
        row[0] = ch.GP(g.cov_type, g.hyper, g.X, g.y, [0.0], ())
        points = p.points.copy()
        points[0], points[1] = g.X[3], g.X[7]
        p = p._replace(gps=[row], points=points)
    return p


_MEMBERS = {}


def _members(c, T):
    """the factored members of a case as it stands, once per process"""
    key = (c.name, T)
    if key not in _MEMBERS:
        p = make_problem(c)
        _MEMBERS[key] = (p, ch.ensemble(p, T))
    return _MEMBERS[key]


def reshifted(members, ref, front, taus):
    """the same factored members under another reference point, caller's front and thresholds: the believed-feasibility mask and the
    member's own front are worked out anew (ch.Member.__init__'s rule), the factorisations are shared"""
    out = []
    for m in members:
        n = copy.copy(m)
        n.taus = [float(t) for t in taus][:m.K]
        n.ref = tuple(float(r) for r in ref)
        n.mask, n.constraint_means = ch.believed_feasible(n.bases[2:], n.P, n.taus)
        n.offered = [o for o, ok in zip(n.outcomes, n.mask) if ok]
        n.caller_front = np.asarray(front, dtype=np.float64).reshape(-1, 2)
        n.front, n.log = hr.believed_front(n.caller_front, n.offered, n.ref, n.T)
        out.append(n)
    return out


def shifted(c, shift, T=LD):
    """(problem, members) of case c with the reference point and the front lowered by shift[0] and every threshold by shift[1]"""
    p, members = _members(c, T)
    ref = tuple(r - shift[0] for r in p.ref)
    front = np.ascontiguousarray(np.asarray(p.front, dtype=np.float64).reshape(-1, 2) - shift[0])
    if c.name == ULP.name:  # (the lowered neighbours would round to one number: one unit in the last place apart again)
        front[1, 0] = np.nextafter(front[0, 0], np.inf)
    if c.name in (ULP64.name, ULP_LAST.name):
        front = _one_ulp(c, front, ref)
    taus = [t - shift[1] for t in p.taus]
    return p._replace(ref=ref, front=front, taus=taus), reshifted(members, ref, front, taus)


_WANT = {}


def expected(c, shift, T=LD):
    """(problem, members, [Result per candidate]) of a case under a shift in the arithmetic of T, once per process"""
    key = (c.name, tuple(shift), T)
    if key not in _WANT:
        p, members = shifted(c, shift, T)
        _WANT[key] = (p, members, [evaluate(members, x) for x in p.points])
    return _WANT[key]


# The stall: the reference point 60 below the smallest observation of either objective, the front empty or two points at offsets
# -0.5 and -0.8 from that reference point, K = 1, 12 Latin-hypercube starts.  The plain form and its gradient are exactly 0 in
# float64 at every start; the log form is finite with a gradient that is not 0.
STALL_CASE = "m2_e1_k1_d3_n20_p3_f0"
STALL_DROP = 60.0
STALL_FRONTS = ("empty", "two")
STALL_GD = (12, 6, 2, 0, 0.7, 1.0, 0.5, 1e-10)


def stall_starts(d=3, n=12):
    """n Latin-hypercube starts in the unit cube: one per stratum and coordinate"""
    rng = np.random.default_rng(77)
    return np.stack([(rng.permutation(n) + rng.uniform(0.02, 0.98, size=n)) / n for _ in range(d)], axis=1)


def stall(front_kind, T=np.float64):
    """(problem, members) of a stall problem"""
    c = ch.case(STALL_CASE)
    p, members = _members(c, T)
    ref = tuple(float(np.min(p.gps[0][r].y[:, 0])) - STALL_DROP for r in range(2))
    front = np.zeros((0, 2)) if front_kind == "empty" else np.array([(ref[0] - 0.8, ref[1] - 0.5), (ref[0] - 0.5, ref[1] - 0.8)])
    return p._replace(ref=ref, front=front), reshifted(members, ref, front, p.taus)


def remasked(m, mask):
    """member m with ANOTHER believed-feasibility mask [p] than its own: what its front would be under the other decisions"""
    n = copy.copy(m)
    n.mask = np.asarray(mask, dtype=bool)
    n.offered = [o for o, ok in zip(n.outcomes, n.mask) if ok]
    n.front, n.log = hr.believed_front(np.asarray(m.caller_front), n.offered, n.ref, n.T)
    return n
