"""Posterior function paths by pathwise conditioning (moe_gp_paths_evaluate / moe_gp_paths_minimize, csrc/paths.hip) restated on the
host on top of kg1_reference.Model, in np.longdouble (the checker of tests/test_gpu_paths.py) or in plain float64 (its twin of the
same algebra; tests/test_paths_reference.py holds the two against each other).  NumPy only.

Member (Model: alpha, lengths l, noise s^2, mean m, K + s^2 I = L L^T) and its path s, from the tables frequencies Om [M][d], phases
b [M], weights w [S][M], noise normals z [S][n]:
    om_i = Om_i / l,   g_s(x) = sqrt(2 alpha / M) sum_i w_si cos(om_i . x + b_i)
    v_s = K^-1 (y - m - g_s(X) - s z_s),   f_s(x) = m + g_s(x) + sum_j v_sj k(x, X_j)
The descent is pm_members_reference.one_step / descend / run's algebra with PathObjective in the place of the member's mean, so every
decision carries its margin.
"""
import numpy as np

import kg1_reference as k1
import pm_members_reference as pr
import recommend_reference as rr
import sampling_reference as sr

LD = sr.LD
SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
MAIN_INNER, LONG_INNER = pr.MAIN_INNER, pr.LONG_INNER


def draw_tables(cov_type, d, n, E, M, S, seed):
    """the tables of a call from numpy's generator: frequencies for the covariance type (Matern-5/2: a multivariate t with 5 degrees
    of freedom), phases in [0, 2 pi), weights [E][S][M], noise normals [E][S][n]"""
    rng = np.random.default_rng(seed)
    freq = rng.standard_normal((M, d))
    if int(cov_type) == MATERN:
        freq = freq / np.sqrt(rng.chisquare(5, size=M) / 5.0)[:, None]
    return dict(frequencies=freq, phases=rng.uniform(0.0, 2.0 * np.pi, size=M), weights=rng.standard_normal((E, S, M)),
                noise_normals=rng.standard_normal((E, S, n)))


class Paths(object):
    """the S paths of one member in the arithmetic of model.T"""

    def __init__(self, model, y, frequencies, phases, weights, noise_normals):
        T = self.t = model.T
        self.m, self.size = model, model.X.shape[1]
        freq = np.asarray(frequencies, dtype=np.float64).reshape(-1, self.size)
        M = freq.shape[0]
        self.om = freq.astype(T) / np.asarray(model.lengths, dtype=np.float64).astype(T)[None, :]
        self.b = np.asarray(phases, dtype=np.float64).astype(T)
        self.w = np.asarray(weights, dtype=np.float64).reshape(-1, M).astype(T)
        self.scale = np.sqrt(T(2) * T(model.alpha) / T(M))
        self.sigma = np.sqrt(T(model.noise))
        self.z = np.asarray(noise_normals, dtype=np.float64).reshape(self.w.shape[0], -1).astype(T)
        self.y = np.asarray(y, dtype=np.float64).ravel()[:model.X.shape[0]].astype(T)
        r = (self.y - T(model.mean))[None, :] - self.prior(model.X) - self.sigma * self.z
        self.v = model.back(model.fwd(np.ascontiguousarray(r.T))).T  # [S][n]

    def _args(self, P):
        P = np.asarray(P, dtype=np.float64).reshape(-1, self.size).astype(self.t)
        return P @ self.om.T + self.b[None, :]  # [C][M]

    def prior(self, P):
        """g_s(P_c) [S][C]"""
        return self.scale * (self.w @ np.cos(self._args(P)).T)

    def values(self, P):
        """f_s(P_c) [S][C]"""
        P = np.asarray(P, dtype=np.float64).reshape(-1, self.size)
        return self.t(self.m.mean) + self.prior(P) + self.v @ self.m.cov(self.m.X, P)

    def grads(self, P):
        """d f_s / d x at P_c [S][C][d]"""
        P = np.asarray(P, dtype=np.float64).reshape(-1, self.size)
        sn = np.sin(self._args(P))  # [C][M]
        out = np.zeros((self.w.shape[0], P.shape[0], self.size), dtype=self.t)
        for c in range(P.shape[0]):
            out[:, c, :] = -self.scale * ((self.w * sn[c][None, :]) @ self.om) + self.v @ self.m.grad_cov(self.m.X, P[c])
        return out


class PathObjective(object):
    """f = -f_s and its gradient: pm_members_reference.Objective's interface"""

    def __init__(self, paths, s):
        self.p, self.s, self.t, self.size = paths, int(s), paths.t, paths.size

    def mu(self, pts):
        return self.p.values(np.asarray(pts, dtype=np.float64).reshape(-1, self.size))[self.s]

    def f(self, x):
        return -self.p.values(np.asarray(x, dtype=self.t).astype(np.float64).reshape(1, self.size))[self.s, 0]

    def f_grad(self, x):
        x = np.asarray(x, dtype=self.t).astype(np.float64).reshape(1, self.size)
        return -self.p.values(x)[self.s, 0], -self.p.grads(x)[self.s, 0]


def run(paths, s, gd, bounds, candidates):
    """pm_members_reference.run for path s: screen, numpy.argmin, descend, keep or fall back, with every margin"""
    obj = PathObjective(paths, s)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, obj.size)
    vals = obj.mu(cand)
    start = int(np.argmin(vals))
    order = np.sort(vals)
    gap_ = float(order[1] - order[0]) if len(order) > 1 else np.inf
    margins = [("argmin", gap_)] if len(order) > 1 else []
    end, steps, m2 = pr.descend(obj, gd, bounds, cand[start])
    margins += m2
    mu_end, mu_start = -obj.f(end), vals[start]
    margins.append(("keep", abs(float(mu_end - mu_start))))
    fell_back = bool(mu_end > mu_start)
    best = cand[start].astype(obj.t) if fell_back else end
    path = [cand[start].astype(obj.t)] + [st.x for _, _, st in steps]
    return pr.Result(vals, start, gap_, path, steps, end, mu_end, mu_start, fell_back, best, mu_start if fell_back else mu_end, margins)


# ---- the cases of tests/test_gpu_paths.py ----
# seed, n, d, E, cov_type, M, S, C: values and gradients against long double.  d = 3, 6, 10, 13, 17, 32 pad to 4, 8, 12, 16, 24, 32; n
# on both sides of the 256-thread stride; M on both sides of it and at the limit; S on both sides of the chunk of 8; n = 260 with
# S = 70: more than 64 columns through the split-K side (n >= 128) of the set phase's triangular products
EVAL_CASES = [
    (1, 20, 3, 1, SE, 64, 1, 7),
    (2, 130, 10, 3, MATERN, 100, 3, 5),
    (3, 300, 3, 1, MATERN, 257, 9, 6),
    (4, 20, 17, 1, SE, 1024, 8, 4),
    (5, 20, 32, 3, MATERN, 64, 70, 3),
    (6, 300, 3, 1, SE, 4096, 1, 1),
    (7, 20, 6, 1, SE, 64, 3, 5),
    (8, 20, 13, 3, MATERN, 100, 9, 4),
    (9, 260, 3, 1, MATERN, 64, 70, 3),
]
# seed, n, d, E, cov_type, M, S, C, gd: the minimiser.  tests/test_paths_reference.py asserts that every decision of every path has a
# margin of at least 1e-7: the seeds were chosen on the CPU so that this holds
LONG12 = LONG_INNER[:1] + (12,) + LONG_INNER[2:]
DESCENT_CASES = [
    (1, 20, 3, 1, SE, 64, 3, 30, MAIN_INNER),
    (2, 130, 10, 3, MATERN, 100, 1, 140, MAIN_INNER),
    (3, 20, 17, 1, MATERN, 64, 9, 30, MAIN_INNER),
    (4, 20, 32, 1, SE, 64, 2, 30, MAIN_INNER),
    (20, 300, 3, 1, MATERN, 257, 2, 310, LONG12),
    (5, 20, 6, 1, SE, 64, 3, 30, MAIN_INNER),
    (6, 20, 13, 1, MATERN, 64, 3, 30, MAIN_INNER),
]
# Rows past the evaluator's row cache (csrc/paths.hip keeps the first 3584 covariance entries of a point in LDS and recomputes the
# rows behind them for every chunk of 8 paths): two chunks over 3600 rows at the feature limit, the largest LDS request there is.
# Kept out of EVAL_CASES (gap() stays fast) and checked against the float64 form: CACHE_GAP is the float64-against-long-double
# difference of this very case at cache_problem()'s points, as tests/test_paths_reference.py's measure_cache_gap() found it (value 5.92e-12,
# gradient 2.98e-12; a minute of long-double factorisation, so the figure is recorded, not recomputed); the device's bound is
# max(tolerance(), 4 CACHE_GAP)
ROW_CACHE = 3584
CACHE_CASE = (31, 3600, 3, 1, MATERN, 4096, 9, 5)
CACHE_GAP = 6.0e-12
# Two launches of the point kernels: 16384 points per launch (tests/test_gpu_paths.py asserts the figure by the launches it sees)
PASS = 16384
PASS_CASE = (32, 20, 3, 1, SE, 8, 1, PASS + 3)


def case_problem(case, dtype=LD):
    """(the members' Paths in dtype, the arrays api.DeviceGP takes, the tables, bounds, points): the points are uniform draws followed
    by the sampled points where C > n, uniform draws otherwise"""
    seed, n, d, E, cov, M, S, C_ = case[:8]
    _, a = rr.make_ensemble(seed, n, d, E, cov, (), dtype=np.float64)
    tables = draw_tables(cov, d, n, E, M, S, 9000 + seed)
    members = []
    for e in range(E):
        model = k1.Model(cov, a["hypers"][e], a["X"], a["y"], a["noises"][e], T=dtype)
        members.append(Paths(model, a["y"], tables["frequencies"], tables["phases"], tables["weights"][e], tables["noise_normals"][e]))
    rng = np.random.default_rng(7000 + seed)
    pts = np.vstack([rng.uniform(0.05, 0.95, size=(C_ - n, d)), a["X"]]) if C_ > n else rng.uniform(0.05, 0.95, size=(C_, d))
    return members, a, tables, np.array([[0.0, 1.0]] * d), pts


def cache_problem(dtype=np.float64):
    """case_problem for CACHE_CASE with its points each within 0.02 (per coordinate) of a sampled point behind the row cache"""
    members, a, tables, bounds, _ = case_problem(CACHE_CASE, dtype)
    n, d, C_ = CACHE_CASE[1], CACHE_CASE[2], CACHE_CASE[7]
    rng = np.random.default_rng(7000 + CACHE_CASE[0])
    rows = ROW_CACHE + rng.choice(n - ROW_CACHE, size=C_, replace=False)
    pts = np.clip(a["X"][rows] + rng.uniform(-0.02, 0.02, size=(C_, d)), 0.0, 1.0)
    return members, a, tables, bounds, pts, rows


def tail_rows(paths, P, first=ROW_CACHE):
    """sum_{j >= first} v_sj k(P_c, X_j) [S][C]: what the rows behind the cache add to f_s"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, paths.size)
    return paths.v[:, first:] @ paths.m.cov(paths.m.X[first:], P)


_GAP = {}


def gap():
    """the largest |float64 twin - long double| of a value or a gradient component over EVAL_CASES and the candidates of
    DESCENT_CASES, relative to max(1, |f|) (a gradient: to max(1, its largest component)): what plain double arithmetic with this
    algebra loses; the device's tolerance is derived from it"""
    if "v" not in _GAP:
        worst = 0.0
        for case in EVAL_CASES + DESCENT_CASES:
            mld, _, _, _, pts = case_problem(case, LD)
            m64 = case_problem(case, np.float64)[0]
            for pl, p6 in zip(mld, m64):
                want, got = pl.values(pts), p6.values(pts)
                worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want.astype(np.float64))))))
                wg, gg = pl.grads(pts[:2]), p6.grads(pts[:2])
                worst = max(worst, float(np.max(np.abs(gg - wg)) / max(1.0, float(np.max(np.abs(wg))))))
        _GAP["v"] = worst
    return _GAP["v"]


def tolerance():
    """the device's bound on a value or gradient against long double, relative to the scale: four times what the float64 twin
    loses, floored at the 1e-10 of the library's other evaluators"""
    return max(1e-10, 4.0 * gap())


def end_gap():
    """pm_members_reference.gap() for DESCENT_CASES: the largest |float64 twin - long double| of an end point relative to max(1, |x|)
    over the paths whose decisions agree"""
    if "e" not in _GAP:
        worst = 0.0
        for case in DESCENT_CASES:
            mld, _, _, bounds, cand = case_problem(case, LD)
            m64 = case_problem(case, np.float64)[0]
            for pl, p6 in zip(mld, m64):
                for s in range(case[6]):
                    want, got = run(pl, s, case[8], bounds, cand), run(p6, s, case[8], bounds, cand)
                    if want.start_index != got.start_index or pr.decisions_of(want.steps) != pr.decisions_of(got.steps):
                        continue
                    x = want.end.astype(np.float64)
                    worst = max(worst, float(np.max(np.abs(got.end - want.end) / np.maximum(1.0, np.abs(x)))))
        _GAP["e"] = worst
    return _GAP["e"]
