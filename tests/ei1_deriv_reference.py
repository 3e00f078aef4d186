"""The analytic one-point expected improvement of GPs with derivative observations, with pending points, averaged over an ensemble,
restated on the CPU (the checker of tests/test_gpu_ei1_deriv.py) in np.longdouble or float64.

A member observes at every sampled point the function value and the partial derivatives `derivs` (g of them): N = n (1 + g) rows,
point-major, row i (1 + g) + a with noise[a] on its diagonal.  A pending point P_j is believed to return its value AND those
derivatives: 1 + g more rows with the same noise, the believed observations being the member's posterior means, so that the mean is
left alone and K'^-1 (y' - mean) = [K^-1 (y - mean) ; 0].  DerivPendingModel writes the conditioned GP out in full: rows X u P, the
whole (N + p (1 + g))^2 matrix factored in the arithmetic T -- nothing of the device's row-by-row extension appears.  The candidate
x is a function value:
    mu = mean + k(X', x) . kinvy',   var = k(x, x) - |L'^-1 k(X', x)|^2,   b' = min(b, min_j mu(P_j)) (function values only)
    EI, its two floors and the gradient as in tests/ei1_reference.py, with grad_x k(row, x) of a derivative row the second-derivative
    block of the covariance.
cross() is the covariance of two point lists with their own derivative lists (BuildMixCovarianceMatrix); with all dim derivatives on
x's side its columns 1 .. dim are grad_x cov(row, x).  The function-value block and its gradient are tests/kg1_reference.py's
expressions operation for operation, so that with g = 0 every figure equals tests/ei1_reference.py's to the last bit.
scale = max(1, |b|, max |y|, sqrt(alpha)).
"""
import collections
import math

import numpy as np

import ei1_reference as er
import kg1_reference as kr
import sampling_reference as sr

LD = kr.LD
SE, MATERN = kr.SE, kr.MATERN
Result = er.Result


def cross(cov_type, alpha, lengths, A, da, B, db, T):
    """cov(A_i[a], B_j[b]) [len(A) (1 + ga)][len(B) (1 + gb)], point-major on both sides; a = 0 the value, 1 + m the partial derivative
    da[m]"""
    A = np.asarray(A, dtype=np.float64).reshape(-1, len(lengths))
    B = np.asarray(B, dtype=np.float64).reshape(-1, len(lengths))
    ga1, gb1 = 1 + len(da), 1 + len(db)
    r2, al = kr._r2(A, B, lengths, T), T(alpha)
    out = np.zeros((A.shape[0] * ga1, B.shape[0] * gb1), dtype=T)
    out[0::ga1, 0::gb1] = kr.covariance(cov_type, alpha, lengths, A, B, T)
    if ga1 == 1 and gb1 == 1:
        return out
    if int(cov_type) == SE:
        first = al * np.exp(-r2 / T(2))
        second = first
    else:
        arg = np.sqrt(T(5) * r2)
        first = T(5) / T(3) * al * np.exp(-arg) * (arg + T(1))
        second = T(25) / T(3) * al * np.exp(-arg)
    ell2 = np.asarray(lengths, dtype=np.float64).astype(T) ** 2
    At, Bt = A.astype(T), B.astype(T)
    diff = [At[:, k][:, None] - Bt[:, k][None, :] for k in range(A.shape[1])]  # A - B
    for b_, i2 in enumerate(db):
        out[0::ga1, 1 + b_::gb1] = first * diff[i2] / ell2[i2]
    for a_, i1 in enumerate(da):
        out[1 + a_::ga1, 0::gb1] = -(first * diff[i1] / ell2[i1])
        for b_, i2 in enumerate(db):
            blk = -(diff[i1] / ell2[i1]) * (diff[i2] / ell2[i2]) * second
            if i1 == i2:
                blk = blk + first / ell2[i2]
            out[1 + a_::ga1, 1 + b_::gb1] = blk
    return out


class DerivModel(kr.Model):
    """a GP on values and derivatives y [n][1 + g], noise [1 + g]; K = L L^T and K^-1 (y - mean) in the arithmetic of T"""

    def __init__(self, cov_type, hyper, X, y, noise, derivs, T=LD):
        hyper = np.asarray(hyper, dtype=np.float64).ravel()
        self.T, self.cov_type, self.alpha, self.lengths = T, int(cov_type), hyper[0], hyper[1:]
        self.X = np.asarray(X, dtype=np.float64)
        self.derivs = tuple(int(v) for v in derivs)
        self.row_derivs = self.derivs  # (the observations behind the model's rows, point by point)
        n, g1 = self.X.shape[0], 1 + len(self.derivs)
        self.noise_all = np.asarray(noise, dtype=np.float64).ravel()[:g1]
        self.noise = float(self.noise_all[0])
        self.points = self.X
        K = self.rows_cov(self.X, self.derivs)
        N = n * g1
        K[np.arange(N), np.arange(N)] += np.tile(self.noise_all.astype(T), n)
        self.L = sr.cholesky_spd(K) if T is LD else np.linalg.cholesky(K)
        Y = np.asarray(y, dtype=np.float64).reshape(n, g1)
        self.mean = sr.constant_mean(Y[:, 0])
        yc = Y.astype(T)
        yc[:, 0] -= T(self.mean)
        self.kinvy = self.back(self.fwd(yc.ravel()))

    def rows_cov(self, B, db):
        """cov(rows of the model, B with derivatives db) [rows][len(B) (1 + len(db))]"""
        return cross(self.cov_type, self.alpha, self.lengths, self.points, self.row_derivs, B, db, self.T)


class DerivPendingModel(DerivModel):
    """`base` conditioned on the pending points: rows X u P, the P rows carrying pending_derivs (default: the model's own list) and
    noise[a] of their observation kind, factored in full"""

    def __init__(self, base, pending, pending_derivs=None):
        T = base.T
        self.T, self.cov_type, self.alpha, self.lengths = T, base.cov_type, base.alpha, base.lengths
        self.noise, self.noise_all, self.mean, self.base, self.derivs = base.noise, base.noise_all, base.mean, base, base.derivs
        P = np.asarray(pending, dtype=np.float64).reshape(-1, base.X.shape[1])
        dp_ = base.derivs if pending_derivs is None else tuple(pending_derivs)
        self.X = np.vstack([base.X, P])
        kind = [0] + [1 + base.derivs.index(i) for i in dp_]  # (which noise a pending row takes)
        c = lambda A, da, B, db: cross(self.cov_type, self.alpha, self.lengths, A, da, B, db, T)  # noqa: E731
        K = np.block([[c(base.X, base.derivs, base.X, base.derivs), c(base.X, base.derivs, P, dp_)],
                      [c(P, dp_, base.X, base.derivs), c(P, dp_, P, dp_)]])
        rows = K.shape[0]
        diag = np.concatenate([np.tile(base.noise_all, base.X.shape[0]), np.tile(base.noise_all[kind], P.shape[0])])
        K[np.arange(rows), np.arange(rows)] += diag.astype(T)
        self.L = sr.cholesky_spd(K) if T is LD else np.linalg.cholesky(K)
        self.kinvy = np.concatenate([base.kinvy, np.zeros(P.shape[0] * len(kind), dtype=T)])
        self._parts = ((base.X, base.derivs), (P, dp_))

    def rows_cov(self, B, db):
        return np.vstack([cross(self.cov_type, self.alpha, self.lengths, A, da, B, db, self.T) for A, da in self._parts])


def believed_best(base, pending, best):
    """b' = min(best, min_j mu(P_j)): the believed function values alone"""
    T = base.T
    b = T(best)
    P = np.asarray(pending, dtype=np.float64).reshape(-1, base.X.shape[1])
    if len(P):
        mu = T(base.mean) + base.rows_cov(P, ()).T @ base.kinvy
        b = min(b, min(mu))
    return b


def evaluate(base, pending, x, best, y_max=0.0, pending_derivs=None):
    """EI and its gradient at x for the model `base` conditioned on `pending` [p][dim] (may be empty)"""
    T = base.T
    dim = base.X.shape[1]
    P = np.asarray(pending, dtype=np.float64).reshape(-1, dim)
    model = DerivPendingModel(base, P, pending_derivs) if len(P) else base
    return evaluate_model(model, base, P, x, best, y_max)


def evaluate_model(model, base, P, x, best, y_max=0.0):
    T = base.T
    dim = base.X.shape[1]
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    kx = model.rows_cov(x, tuple(range(dim)))  # [rows][1 + dim]: the value column and grad_x cov(row, x)
    k = np.ascontiguousarray(kx[:, 0])
    gk = np.ascontiguousarray(kx[:, 1:])
    v = model.fwd(k)
    mu = T(base.mean) + k @ model.kinvy
    var = kr.covariance(base.cov_type, base.alpha, base.lengths, x, x, T)[0, 0] - v @ v
    bp = believed_best(base, P, best)
    t = bp - mu
    sigma = np.sqrt(max(T(er.MIN_VAR_EI), var))
    c = t / sigma
    value = max(T(0), t * er.normal_cdf(c, T) + sigma * kr.normal_pdf(c, T))
    sg = np.sqrt(max(T(er.MIN_VAR_GRAD_EI), var))
    cg = t / sg
    grad_mu = gk.T @ model.kinvy
    grad_var = T(-2) * (gk.T @ model.back(v))
    grad = -er.normal_cdf(cg, T) * grad_mu + kr.normal_pdf(cg, T) * grad_var / (T(2) * sg)
    scale = max(1.0, abs(float(best)), float(y_max), math.sqrt(float(base.alpha)))
    return Result(value, grad, float(sigma), float(c), float(bp), scale)


def conditioned_variance(model, x):
    """var of the latent function at x under `model` (a DerivModel or DerivPendingModel)"""
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    v = model.fwd(np.ascontiguousarray(model.rows_cov(x, ())[:, 0]))
    return kr.covariance(model.cov_type, model.alpha, model.lengths, x, x, model.T)[0, 0] - v @ v


# ---- the cases of tests/test_gpu_ei1_deriv.py (tests/test_ei1_deriv_reference.py qualifies them on the CPU) ----
Case = collections.namedtuple("Case", "name seed n d derivs p cov_type noise0 C near best_is_max")
Problem = collections.namedtuple("Problem", "name cov_type hyper X y noise derivs points pending best checked")

LENGTH_0, LENGTH_D = 0.05, 0.1
CASES = [
    Case("n5_d2_g2_p1", 1, 5, 2, (0, 1), 1, MATERN, 1e-2, 5, False, False),
    Case("n20_d3_D1_p2", 2, 20, 3, (1,), 2, MATERN, 1e-2, 5, False, False),
    Case("n40_d4_D023_p5_se", 3, 40, 4, (0, 2, 3), 5, SE, 1e-2, 5, False, False),          # 160 rows: the split-K side of tri_cols
    Case("n44_d3_g2_p3_noise1e-3", 4, 44, 3, (0, 2), 3, MATERN, 1e-3, 5, False, False),    # 132 rows
    Case("n12_d2_g2_p21", 5, 12, 2, (0, 1), 21, MATERN, 1e-2, 5, False, False),            # 63 extension rows
    Case("n20_d6_D05_p3", 6, 20, 6, (0, 5), 3, MATERN, 1e-2, 5, False, False),             # the DP = 8 gradient kernel
    Case("n10_d32_D0_31_p2", 7, 10, 32, (0, 31), 2, MATERN, 1e-2, 5, True, False),         # the DP = 32 gradient kernel
    Case("n9_d12_g12_p2", 8, 9, 12, tuple(range(12)), 2, MATERN, 1e-2, 5, False, False),   # 13 rows per point
    Case("n30_d3_g3_p4_bprime", 9, 30, 3, (0, 1, 2), 4, MATERN, 1e-2, 5, False, True),     # best = max(y): b' binds
]
BPRIME = "n30_d3_g3_p4_bprime"


def smooth(X, seed):
    """a smooth function of spread ~ 0.3 and its gradient: (f [n], grad f [n][d])"""
    X = np.asarray(X, dtype=np.float64)
    rng = np.random.default_rng(900 + seed)
    d = X.shape[1]
    w1, w2 = rng.normal(size=d) * 3.0 / math.sqrt(d), rng.normal(size=d) * 2.0 / math.sqrt(d)
    ph = rng.uniform(0, 2 * math.pi)
    f = 0.3 * (np.sin(X @ w1 + ph) + np.cos(X @ w2))
    grad = 0.3 * (np.cos(X @ w1 + ph)[:, None] * w1[None, :] - np.sin(X @ w2)[:, None] * w2[None, :])
    return f, grad


def noise_of(noise0, g):
    """distinct noise per observation kind: a device that took noise[0] for a derivative row would fail"""
    return np.array([noise0 * (1.0 + a / 2.0) for a in range(1 + g)])


def observe(X, derivs, noise, seed, rng):
    f, grad = smooth(X, seed)
    y = np.column_stack([f] + [grad[:, i] for i in derivs])
    return y + rng.normal(size=y.shape) * np.sqrt(noise)[None, :]


def make_problem(case, p=None):
    """the inputs of a case (p: that many of its pending points).  Candidate 0 lies within 0.05 of pending point 0 in every
    coordinate.  `near`: the candidates lie within 0.08 of sampled points and pending points 0, 1 within 0.05 of candidates 0, 1 (in
    32 dimensions a uniform candidate is far from everything and neither derivative rows nor P move its value)."""
    rng = np.random.default_rng(8300 + case.seed)
    X = rng.uniform(0, 1, size=(case.n, case.d))
    noise = noise_of(case.noise0, len(case.derivs))
    y = observe(X, case.derivs, noise, case.seed, rng)
    hyper = np.array([1.3] + [LENGTH_0 + LENGTH_D * math.sqrt(case.d)] * case.d)
    if case.near:
        points = np.clip(X[:case.C] + rng.uniform(-0.08, 0.08, size=(case.C, case.d)), 0.0, 1.0)
    else:
        points = rng.uniform(0.1, 0.9, size=(case.C, case.d))
    pending = rng.uniform(0, 1, size=(case.p, case.d))
    pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=case.d)
    if case.near and case.p > 1:
        pending[1] = points[1] + rng.uniform(-0.05, 0.05, size=case.d)
    best = float(y[:, 0].max()) if case.best_is_max else float(y[:, 0].min())
    pending = pending if p is None else pending[:p]
    name = case.name if p is None else "%s_first%d" % (case.name, p)
    return Problem(name, case.cov_type, hyper, X, y, noise, case.derivs, points, pending, best, tuple(range(case.C)))


PROBLEMS = [make_problem(c) for c in CASES]
PROBLEMS_P0 = [make_problem(c, 0) for c in CASES]

# padded dimensions 16 and 24 of ei1_grad_g_kernel (12 is reached above without a padded coordinate), and more than 256 points: a
# second trip of its loop over the points, 520 rows (tri_cols' K slice 128).  From 256 points on the best value is the median of the
# observed values (tests/ei1_reference.py: with the minimum EI and its gradient vanish and a 1e-10 test is empty).
WIDE_CASES = [
    # (seed chosen on the CPU for tests/gibbon_reference.py, which takes this case: candidates 0 and 1 lie low enough for gamma near 3)
    Case("n10_d13_D0_12_p2", 30, 10, 13, (0, 12), 2, MATERN, 1e-2, 5, True, False),    # DP = 16, three padded coordinates
    Case("n10_d20_D3_19_p2_se", 22, 10, 20, (3, 19), 2, SE, 1e-2, 5, True, False),      # DP = 24, four padded coordinates
    Case("n260_d3_D1_p2", 23, 260, 3, (1,), 2, MATERN, 1e-2, 5, False, False),          # 260 points, 520 rows
]


def make_wide_problem(case, p=None):
    q = make_problem(case, p)
    return q._replace(best=float(np.median(q.y[:, 0]))) if case.n >= 256 else q


WIDE_PROBLEMS = [make_wide_problem(c) for c in WIDE_CASES]
WIDE_PROBLEMS_P0 = [make_wide_problem(c, 0) for c in WIDE_CASES]

_WANT = {}


def base_model(p, T=LD):
    return DerivModel(p.cov_type, p.hyper, p.X, p.y, p.noise, p.derivs, T)


def expected(p, T=LD):
    """{candidate index: Result} of a problem in the arithmetic of T, computed once per process"""
    key = (p.name, T)
    if key not in _WANT:
        base = base_model(p, T)
        y_max = float(np.max(np.abs(p.y)))
        P = np.asarray(p.pending, dtype=np.float64).reshape(-1, p.X.shape[1])
        model = DerivPendingModel(base, P) if len(P) else base
        _WANT[key] = {i: evaluate_model(model, base, P, p.points[i], p.best, y_max) for i in p.checked}
    return _WANT[key]


def expected_variants(p):
    """long-double values of the checked candidates with something dropped: (without P, P's rows value-only, X's derivative
    observations dropped: the GP on y[:, 0] alone with the same pending points)"""
    key = (p.name, "variants")
    if key not in _WANT:
        base = base_model(p, LD)
        P = np.asarray(p.pending, dtype=np.float64).reshape(-1, p.X.shape[1])
        plain = kr.Model(p.cov_type, p.hyper, p.X, p.y[:, :1], p.noise[:1], LD)
        value_only = DerivPendingModel(base, P, ()) if len(P) else base
        out = ({}, {}, {})
        for i in p.checked:
            out[0][i] = evaluate_model(base, base, P[:0], p.points[i], p.best).value
            out[1][i] = evaluate_model(value_only, base, P, p.points[i], p.best).value
            out[2][i] = er.evaluate(plain, P, p.points[i], p.best).value
        _WANT[key] = out
    return _WANT[key]


# ---- a three-member ensemble: one derivative list, different hyper-parameters and noise, n on both sides of 128 rows ----
ENSEMBLE = dict(seed=61, d=3, derivs=(0, 2), n=(12, 50, 30), cov=(MATERN, SE, MATERN), factors=(1.0, 1.3, 0.8), p=3, C=6)
EnsembleProblem = collections.namedtuple("EnsembleProblem", "hyper X y noise cov derivs best points pending")


def make_ensemble():
    e = ENSEMBLE
    rng = np.random.default_rng(8300 + e["seed"])
    nmax, g = max(e["n"]), len(e["derivs"])
    X = rng.uniform(0, 1, size=(nmax, e["d"]))
    noise0 = noise_of(1e-2, g)
    y = observe(X, e["derivs"], noise0, e["seed"], rng)
    base = np.array([1.3] + [LENGTH_0 + LENGTH_D * math.sqrt(e["d"])] * e["d"])
    hyper = [base * f for f in e["factors"]]
    noise = [noise0 * f for f in e["factors"]]
    best = [float(y[:n, 0].min()) + 0.1 * k for k, n in enumerate(e["n"])]
    points = rng.uniform(0.1, 0.9, size=(e["C"], e["d"]))
    pending = rng.uniform(0, 1, size=(e["p"], e["d"]))
    pending[0] = points[0] + rng.uniform(-0.05, 0.05, size=e["d"])
    return EnsembleProblem(hyper, [X[:n] for n in e["n"]], [y[:n] for n in e["n"]], noise, e["cov"], e["derivs"], best, points, pending)


def ensemble_expected(ep, pending, T=LD):
    """per candidate (mean of the members' values, mean of their gradients, the largest member scale)"""
    key = ("ensemble", len(pending), T)
    if key not in _WANT:
        bases = [DerivModel(ep.cov[k], ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], ep.derivs, T) for k in range(len(ep.X))]
        P = np.asarray(pending, dtype=np.float64).reshape(-1, ep.points.shape[1])
        models = [DerivPendingModel(m, P) if len(P) else m for m in bases]
        out = []
        for x in ep.points:
            res = [evaluate_model(mm, m, P, x, b, float(np.max(np.abs(y)))) for mm, m, b, y in zip(models, bases, ep.best, ep.y)]
            value, grad = T(0), np.zeros(len(x), dtype=T)
            for r in res:
                value, grad = value + r.value, grad + r.grad
            out.append((value / T(len(res)), grad / T(len(res)), max(r.scale for r in res)))
        _WANT[key] = out
    return _WANT[key]
