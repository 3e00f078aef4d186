"""The LOG of the three-objective constrained expected hypervolume improvement with pending points, averaged over an ensemble,
restated on the CPU (the checker of tests/test_gpu_log_ehvi3.py) in np.longdouble or float64, on top of tests/ehvi3_reference.py
(box_table, believed_front), tests/cehvi_reference.py (Member, ensemble, make_problem, BELIEVED3, MASKED[3]: the members, their
conditioning on the pending points, the believed-feasibility mask and the join rule are that file's), tests/logcei1_reference.py
(log_h_parts, role_log) and tests/log_ehvi_reference.py (SHIFTS, host_value), all imported unchanged.

With mu_r, var_r the posterior mean and the conditioned latent variance of objective r's GP at x and ONE floor,
sigma = sqrt(max(150 eps^2, var)); a member's front n points (u_i, v_i, w_i) in the canonical order, its table ehvi3_reference.box_table's
(left, right, height, slab; edge 0 -inf, 1 .. n the points, n + 1 the reference point):
    lambda_r(t) = log sigma_r + log h(z),  z = (t - mu_r) / sigma_r,  (log h, lam, kap) = log_h_parts(z);  lambda_r(-inf) = -inf
    difference rule, edges a < b of objective r:  D = lambda_r(a) - lambda_r(b), rho = exp(D);  log[psi(b) - psi(a)] = lambda_r(b) +
              log(1 - rho)  (log1p(-rho) for rho <= 1/2, log(-expm1(D)) above);  d/dmu = -(lam_b - rho lam_a) / (sigma (1 - rho)),
              d/dvar = (kap_b - rho kap_a) / (2 sigma^2 (1 - rho));  a pair that does not give D < 0 (rho = 1) carries weight 0
    box b:    l_b = ((log P) + lambda_2(height)) + log W_k, log P by the rule from objective 1 at (left, right), log W_k from objective
              3 at (w_k, w_{k+1});  dl/dmu_2 = -lam(height) / sigma_2,  dl/dvar_2 = kap(height) / (2 sigma_2^2);  a box whose P or W
              carries weight 0 is skipped
    L_e = m + log W,  m = max_b l_b,  w_b = exp(l_b - m),  W = sum_b w_b;  coefficients (sum_b w_b dl_b/d.) / W
    log F_k and its gradient: logcei1_reference.role_log with role k
    LL_e = L_e + log F_1 + ... + log F_K;  g_e = the six coefficient terms in the order mu_1, var_1, mu_2, var_2, mu_3, var_3, then
    the constraints';  value = m + log W - log E over the members (m = max_e LL_e, w_e = exp(LL_e - m)),  grad = (sum_e w_e g_e) / W
A SHIFT (s, t) lowers the reference point and every point of the caller's front by s in all three objectives and every threshold by
t; the members' factorisations are shared between the shifts, their masks, fronts and tables are worked out anew.
"""
import collections
import copy
import math

import numpy as np

import cehvi_reference as ch
import cei1_reference as cr
import ehvi3_reference as h3
import ei1_reference as er
import log_ehvi_reference as lh
import logcei1_reference as lr

LD = ch.LD
Result = collections.namedtuple("Result", "value grad log_factors coef skipped")
SHIFTS = lh.SHIFTS
host_value = lh.host_value


def edge_logs(moments3, front, ref, T=LD):
    """(lam [3][3][n + 2]: lambda, lam, kap of every edge of the three objectives, sigma [3])"""
    front = np.asarray(front, dtype=T).reshape(-1, 3)
    n = len(front)
    e = np.zeros((3, 3, n + 2), dtype=T)
    sd = []
    for k in range(3):
        mu, var = moments3[k]
        s = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), T(var)))
        sd.append(s)
        e[k, 0, 0] = T(-np.inf)
        for i in range(1, n + 2):
            t = front[i - 1, k] if i <= n else T(ref[k])
            lhh, lam, kap = lr.log_h_parts((t - T(mu)) / s, T)
            e[k, :, i] = (np.log(s) + lhh, lam, kap)
    return e, sd


def _difference(ea, eb, s, T):
    """the difference rule over arrays of edges: (weight > 0 [B], log difference, d/dmu, d/dvar), the last three 0 where not"""
    with np.errstate(all="ignore"):
        D = ea[0] - eb[0]
        ok = D < 0
        D = np.where(ok, D, T(-1))
        rho = np.exp(D)
        low = rho <= T(0.5)
        om = np.where(low, T(1) - rho, -np.expm1(D))
        lom = np.where(low, np.log1p(-np.where(low, rho, T(0))), np.log(om))
        ld = eb[0] + lom
        dmu = -(eb[1] - rho * ea[1]) / (s * om)
        dvar = (eb[2] - rho * ea[2]) / (T(2) * (s * s) * om)
    z = T(0)
    return ok, np.where(ok, ld, z), np.where(ok, dmu, z), np.where(ok, dvar, z), np.where(ok, rho, T(1))


def log_boxes(moments3, front, ref, T=LD, table=None):
    """(L, [dL/dmu_1, dL/dvar_1, dL/dmu_2, dL/dvar_2, dL/dmu_3, dL/dvar_3], the boxes skipped at rho = 1) of one member from its
    three (mu, var), its front [n][3] and r, walking over ehvi3_reference.box_table"""
    front = np.asarray(front, dtype=T).reshape(-1, 3)
    table = h3.box_table(front) if table is None else table
    e, sd = edge_logs(moments3, front, ref, T)
    uL, uR, vH, sl = table[:, 0], table[:, 1], table[:, 2], table[:, 3]
    okP, lp, p_mu, p_var, _ = _difference(e[0][:, uL], e[0][:, uR], sd[0], T)
    okW, lw, w_mu, w_var, _ = _difference(e[2][:, sl], e[2][:, sl + 1], sd[2], T)
    keep = okP & okW
    l = ((lp + e[1][0][vH]) + lw)[keep]
    dl = [p_mu, p_var, -e[1][1][vH] / sd[1], e[1][2][vH] / (T(2) * (sd[1] * sd[1])), w_mu, w_var]
    m = np.max(l)
    w = np.exp(l - m)
    W = np.sum(w)
    c = [np.sum(w * d[keep]) / W for d in dl]
    return m + np.log(W), c, int(np.sum(~keep))


def thread_replay(moments3, front, ref, table=None):
    """logehvi3_box_kernel's reduction order replayed in float64 for one member and candidate: box b belongs to thread b mod 256,
    the sweeps ascend, a thread's record (m, W, S[6]) takes its boxes by record_take's two branches, the 64 records of a wavefront
    merge by the fixed butterfly (xor 32, 16, 8, 4, 2, 1; every pair counted once) and the four wavefronts' records as
    (0 + 1) + (2 + 3).  Returns the counts of what ran -- which branch decides nothing about the value, so nothing but such a count
    shows that a branch was reached:
        p_low / p_high / p_one         boxes whose P has rho <= 1/2, above, and skipped at rho = 1
        w_low / w_high / w_one         slabs likewise;  w_skipped: the boxes skipped because their slab carries weight 0
        first / rescales / below       record_take: a thread's first box; later boxes above its running maximum; at or below it
        later_sweeps                   the boxes taken with b >= 256
        won_low / won_high / empty     butterfly merges whose maximum is the lower lane's (ties included) / the upper lane's;
                                       merges in which a record holds no box
        wave_empty                     merges of wavefronts' records in which one holds no box
        L, c                           m + log W and S / W of the last merge: the kernel's value and coefficients in this order"""
    T = np.float64
    front = np.asarray(front, dtype=T).reshape(-1, 3)
    table = h3.box_table(front) if table is None else table
    n = len(front)
    with np.errstate(all="ignore"):
        e, sd = edge_logs(moments3, front, ref, T)
    e = e.astype(np.float64)
    sd = [float(s) for s in sd]
    out = dict(p_low=0, p_high=0, p_one=0, w_low=0, w_high=0, w_one=0, w_skipped=0, first=0, rescales=0, below=0, later_sweeps=0,
               won_low=0, won_high=0, empty=0, wave_empty=0, boxes=len(table))

    def rule(a, b, r, kind):
        la, lb = float(e[r, 0, a]), float(e[r, 0, b])
        D = la - lb
        if not D < 0.0:
            out[kind + "_one"] += 1
            return None
        rho = math.exp(D)
        out[kind + ("_low" if rho <= 0.5 else "_high")] += 1
        if rho <= 0.5:
            om, lom = 1.0 - rho, math.log1p(-rho)
        else:
            om = -math.expm1(D)
            lom = math.log(om)
        return (lb + lom, -(float(e[r, 1, b]) - rho * float(e[r, 1, a])) / (sd[r] * om),
                (float(e[r, 2, b]) - rho * float(e[r, 2, a])) / (2.0 * (sd[r] * sd[r]) * om))

    slabs = [rule(k, k + 1, 2, "w") for k in range(n + 1)]
    rec = [[-math.inf, 0.0, [0.0] * 6] for _ in range(256)]
    for b, (uL, uR, vH, k) in enumerate(table):
        if slabs[k] is None:
            out["w_skipped"] += 1
            continue
        P = rule(int(uL), int(uR), 0, "p")
        if P is None:
            continue
        l = (P[0] + float(e[1, 0, vH])) + slabs[k][0]
        dl = [P[1], P[2], -float(e[1, 1, vH]) / sd[1], float(e[1, 2, vH]) / (2.0 * (sd[1] * sd[1])), slabs[k][1], slabs[k][2]]
        r = rec[b % 256]
        out["later_sweeps"] += b >= 256
        if r[0] == -math.inf:
            out["first"] += 1
        elif l > r[0]:
            out["rescales"] += 1
        else:
            out["below"] += 1
        if l > r[0]:
            sc = math.exp(r[0] - l)
            r[1] = r[1] * sc + 1.0
            r[2] = [s * sc + d for s, d in zip(r[2], dl)]
            r[0] = l
        else:
            w = math.exp(l - r[0])
            r[1] = r[1] + w
            r[2] = [s + w * d for s, d in zip(r[2], dl)]

    def join(a, b, name):
        if a[0] == -math.inf or b[0] == -math.inf:
            out[name] += 1
            return list(b if a[0] == -math.inf else a)
        top = max(a[0], b[0])
        if name == "empty":
            out["won_low" if a[0] >= b[0] else "won_high"] += 1
        ea, eb = math.exp(a[0] - top), math.exp(b[0] - top)
        return [top, a[1] * ea + b[1] * eb, [sa * ea + sb * eb for sa, sb in zip(a[2], b[2])]]

    waves = []
    for v in range(4):
        lanes = rec[64 * v:64 * v + 64]
        for off in (32, 16, 8, 4, 2, 1):
            nxt = list(lanes)
            for a in range(64):
                b = a ^ off
                if a < b:
                    nxt[a] = nxt[b] = join(lanes[a], lanes[b], "empty")
            lanes = nxt
        waves.append(lanes[0])
    total = join(join(waves[0], waves[1], "wave_empty"), join(waves[2], waves[3], "wave_empty"), "wave_empty")
    out["L"] = total[0] + math.log(total[1])
    out["c"] = [s / total[1] for s in total[2]]
    return out


def member_moments(m, x):
    return [cr.moments(model, base, x) for model, base in zip(m.models[:3], m.bases[:3])]


def member_logs(m, x):
    """([L_e, log F_1 .. log F_K], g_e, the six coefficients, boxes skipped) of a ch.Member (M = 3) at x"""
    T = m.T
    mo = member_moments(m, x)
    L, c, skipped = log_boxes([(q[0], q[1]) for q in mo], m.front, m.ref, T, m.table)
    g = c[0] * mo[0][2] + c[1] * mo[0][3]
    for r in (1, 2):
        g = (g + c[2 * r] * mo[r][2]) + c[2 * r + 1] * mo[r][3]
    vals = [L]
    for k, (model, base, tau) in enumerate(zip(m.models[3:], m.bases[3:], m.taus)):
        l, gl, _ = lr.role_log(T, *cr.moments(model, base, x), tau, 1 + k)
        vals.append(l)
        g = g + gl
    return vals, g, c, skipped


def evaluate(members, x):
    """Result of the ensemble at x"""
    T = members[0].T
    Ls, gs, logs, coefs, skipped = [], [], [], [], 0
    for m in members:
        vals, g, c, sk = member_logs(m, x)
        L = vals[0]
        for v in vals[1:]:
            L = L + v
        Ls.append(L)
        gs.append(g)
        logs.append(vals)
        coefs.append(c)
        skipped += sk
    top = max(Ls)
    w = [np.exp(L - top) for L in Ls]
    W, num = w[0], w[0] * gs[0]
    for we, ge in zip(w[1:], gs[1:]):
        W, num = W + we, num + we * ge
    return Result(top + np.log(W) - np.log(T(len(members))), num / W, logs, coefs, skipped)


# ---- the cases of tests/test_gpu_log_ehvi3.py (tests/test_log_ehvi3_reference.py qualifies them on the CPU) ----
Case = ch.Case
ROWS = (20, 26, 33)  # the members' observations: E = 3 members of different n
KS, FS = (0, 1, 2, 8), (0, 1, 2, 22, 45)


def _case(K, F):
    n = tuple(tuple(r for _ in range(3 + K)) for r in ROWS)
    return Case("log3_e3_k%d_d3_n20_26_33_p3_f%d" % (K, F), 700 + 10 * K + FS.index(F), 3, 3, K, 3, n, 3, F, ch.TAUS[K] if K else (), 8,
                None, 0.0)


# F in {0, 1, 2}: one sweep, wavefronts and lanes without a box, and the believed outcomes of the three pending points join or not
# as each member believes, so the members' fronts differ; F = 22: the caller's front a full staircase of 276 boxes, a second sweep in
# some threads; F = 45: 1 081 boxes, a second sweep in every wavefront.  The staircases lie STAIR_DROP below
# ehvi3_reference.staircase_front's, under the believed outcomes: an outcome that joins evicts none of their points, so that every
# member's table keeps at least the caller's boxes.
STAIR_DROP = 0.3
CASES = [_case(K, F) for K in KS for F in FS]
CASE_SHIFTS = [(c, s) for c in CASES for s in SHIFTS]
# a front of three where two points share w exactly: the slab between them has zero thickness and its boxes carry weight 0
TIE = Case("log3_e1_k1_d3_n20_p0_f3_tie", 771, 3, 1, 1, 3, ((20,) * 4,), 0, 3, ch.TAUS[1], 8, None, 0.0)
TIE_FRONT = np.array([(0.2, -0.4, -0.3), (-0.3, 0.1, 0.2), (-0.1, -0.2, 0.2)])
# a front of three whose staircase has two neighbouring u edges a unit in the last place apart
ULP = Case("log3_e1_k1_d3_n20_p0_f3_ulp", 772, 3, 1, 1, 3, ((20,) * 4,), 0, 3, ch.TAUS[1], 8, None, 0.0)
EDGE_CASES = [TIE, ULP]


def ulp_front(shift=0.0):
    a = -0.2 - shift
    return np.array([(a, 0.4 - shift, -0.3 - shift), (np.nextafter(a, np.inf), 0.1 - shift, 0.0 - shift), (0.3 - shift, -0.3 - shift, 0.2 - shift)])


def case(name):
    return next(c for c in CASES + EDGE_CASES if c.name == name)


def make_problem(c):
    """ch.make_problem with this file's fronts: the lowered staircase from 22 points on"""
    p = ch.make_problem(c)
    if c.name == TIE.name:
        p = p._replace(front=np.ascontiguousarray(TIE_FRONT))
    elif c.name == ULP.name:
        p = p._replace(front=np.ascontiguousarray(ulp_front()))
    elif c.F >= 22:
        p = p._replace(front=np.ascontiguousarray(h3.staircase_front(c.F) - STAIR_DROP))
    return p


_MEMBERS = {}


def _members(c, T):
    key = (c.name, T)
    if key not in _MEMBERS:
        p = make_problem(c)
        _MEMBERS[key] = (p, ch.ensemble(p, T))
    return _MEMBERS[key]


def reshifted(members, ref, front, taus):
    """the same factored members (M = 3) under another reference point, caller's front and thresholds: the believed-feasibility mask,
    the member's own front and its table are worked out anew (ch.Member.__init__'s rule), the factorisations are shared"""
    out = []
    for m in members:
        n = copy.copy(m)
        n.taus = [float(t) for t in taus][:m.K]
        n.ref = tuple(float(r) for r in ref)
        n.mask, n.constraint_means = ch.believed_feasible(n.bases[3:], n.P, n.taus)
        n.offered = [o for o, ok in zip(n.outcomes, n.mask) if ok]
        n.caller_front = np.asarray(front, dtype=np.float64).reshape(-1, 3)
        n.front, n.log = h3.believed_front(n.caller_front, n.offered, n.ref, n.T)
        n.table = h3.box_table(n.front)
        out.append(n)
    return out


def shifted_problem(p, c, shift):
    ref = tuple(r - shift[0] for r in p.ref)
    front = np.ascontiguousarray(np.asarray(p.front, dtype=np.float64).reshape(-1, 3) - shift[0])
    if c is not None and c.name == ULP.name:  # (the lowered neighbours would round to one number: an ulp apart again)
        front = np.ascontiguousarray(ulp_front(shift[0]))
    return p._replace(ref=ref, front=front, taus=[t - shift[1] for t in p.taus])


def shifted(c, shift, T=LD):
    """(problem, members) of case c with the reference point and the front lowered by shift[0] and every threshold by shift[1]"""
    p, members = _members(c, T)
    q = shifted_problem(p, c, shift)
    return q, reshifted(members, q.ref, q.front, q.taus)


_WANT = {}


def expected(c, shift, T=LD):
    """(problem, members, [Result per candidate]) of a case under a shift in the arithmetic of T, once per process"""
    key = (c.name, tuple(shift), T)
    if key not in _WANT:
        p, members = shifted(c, shift, T)
        _WANT[key] = (p, members, [evaluate(members, x) for x in p.points])
    return _WANT[key]


def remasked(m, mask):
    """member m with ANOTHER believed-feasibility mask [p] than its own (from its caller's front)"""
    return ch.remasked(m, mask, np.asarray(m.caller_front))


# The stall: the reference point STALL_DROP below the smallest observation of one objective ("one": the first, the other two
# coordinates stay ch.REF3's) or of all three ("all"), the front empty, K = 1, 12 Latin-hypercube starts.  The plain form and its
# gradient are exactly 0 in float64 at every start; the log form is finite with a gradient that is not 0.  "far": the reference point
# as it stands and the one constraint's threshold STALL_FAR posterior deviations below the lowest constraint mean over the starts.
STALL_CASE = "m3_e1_k1_d3_n20_p3_f0"
STALL_DROP = 60.0
STALL_KINDS = ("one", "all", "far")
STALL_FAR = 40.0
# The ascent has no line search: step i moves by pre_mult (i + 1)^-gamma grad, capped at half the distance to the bound, and climbs
# for certain only where pre_mult is below 1 / L, L the largest curvature of the objective.  Here the log value behaves like
# -z^2 / 2 with z = Delta / sigma(x) the number of deviations that underflows the plain form, so its curvature along x is about
# 3 (Delta^2 / sigma^4) |grad sigma|^2: Delta = 60 (or z up to 200 in "far"), sigma from 0.3 near the observations, |grad sigma|
# of order 1 give L of order 1e6, three times that with all three objectives lowered.  pre_mult = 1e-7 lies a factor 3 to 8 below
# 1 / L; log_ehvi_reference.STALL_GD's 1.0 would make every step the cap, whatever the gradient.
STALL_GD = (12, 6, 2, 0, 0.7, 1e-7, 0.5, 1e-10)
stall_starts = lh.stall_starts


def stall_problem(kind):
    p = ch.make_problem(ch.case(STALL_CASE))
    if kind == "far":
        members = ch.ensemble(p, np.float64)
        model, base = members[0].models[3], members[0].bases[3]
        mo = [cr.moments(model, base, x) for x in stall_starts()]
        return p._replace(taus=[min(float(q[0]) - STALL_FAR * math.sqrt(float(q[1])) for q in mo)])
    lows = [float(np.min(p.gps[0][r].y[:, 0])) - STALL_DROP for r in range(3)]
    ref = (lows[0], p.ref[1], p.ref[2]) if kind == "one" else tuple(lows)
    return p._replace(ref=ref, front=np.zeros((0, 3)))
