"""The exact discretised one-point knowledge gradient restated on the CPU, in np.longdouble (the checker of tests/test_gpu_kg1.py)
or in plain float64 (tests/test_kg1_reference.py holds the two against each other), on top of tests/sampling_reference.py.

For a GP without derivative observations with posterior mean mu_n and covariance Sigma_n, observation noise sigma^2, a candidate x
[dim], x^ = x with its last num_fidelity coordinates set to 1 and a discrete set A [A][dim - num_fidelity] padded the same way:
    s^2 = Sigma_n(x, x) + sigma^2,   Z = {x^} u A (x^ first),   a_z = mu_n(z),   b_z = Sigma_n(z, x) / s
    KG_A(x) = min(best, mu_n(x^)) - E[min_z (a_z + b_z Z)],  Z ~ N(0, 1)
the fantasy of gpp_knowledge_gradient_optimization.cpp:83-107, :298-316 conditioned on with noise sigma^2.  Lines ordered by
(slope descending, intercept ascending, index ascending); of equal slopes the first survives; a stack scan leaves the lower
envelope j = 1 .. k with breakpoints c_0 = -inf < c_1 < ... < c_k = inf, and
    E[min] = sum_j a_j P_j + b_j w_j,   P_j = Phi(c_j) - Phi(c_j-1),   w_j = phi(c_j-1) - phi(c_j)
    grad E[min] = sum_j P_j grad a_j + w_j grad b_j      (envelope theorem: the breakpoints' terms cancel)
    grad b_j = grad_x Sigma_n(z_j, x) / s - Sigma_n(z_j, x) grad(s^2) / (2 s^3)
with grad a_j non-zero only for x^'s line (grad mu_n on the free coordinates) and x^'s own slope depending on x through both
arguments.  grad KG = [mu_n(x^) < best] grad mu_n(x^) - grad E[min].

Decision margins (Result.margins): (the smallest relative gap by which a line enters or misses the envelope,
|mu_n(x^) - best| / scale), with scale = max(1, max |a|, sqrt(alpha)).  A stack decision asks whether the top line t lies below the
lines u (under it on the stack) and i (the new one) where those two cross, at Z* = (a_i - a_u) / (b_u - b_i); its gap is the
vertical distance there, |(a_t + b_t Z*) - (a_u + b_u Z*)| / scale = |lhs - rhs| / ((b_u - b_i) scale) for the two products
lhs = (a_i - a_u)(b_u - b_t), rhs = (a_t - a_u)(b_u - b_i) the scan compares.  (Errors of eps scale in the a and b move that distance
by about 2 eps scale (1 + |Z*|): crossings far out in the tails, between lines of nearly equal slope, are the sensitive ones.)
"""
import collections
import math

import numpy as np

import sampling_reference as sr

LD = sr.LD

Result = collections.namedtuple("Result", "value emin grad num_active hull a b s2 margins scale")


def _erfc_nonneg(x, T):
    """erfc(x) for x >= 0 in the arithmetic of T: below 2.5 one minus the all-positive series
    erf = 2/sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 ... (2n+1)), from there on the continued fraction."""
    x = T(x)
    if x == T(np.inf):
        return T(0)
    root_pi = np.sqrt(T(4) * np.arctan(T(1)))
    e = np.exp(-x * x)
    if x < T(2.5):
        term, total, n = x, x, 0
        while True:
            n += 1
            term = term * T(2) * x * x / T(2 * n + 1)
            total = total + term
            if term <= total * T(np.finfo(T).eps) / T(8):
                break
        return T(1) - T(2) / root_pi * e * total
    t = x
    for k in range(400, 0, -1):
        t = x + T(k) / T(2) / t
    return e / (root_pi * t)


def normal_cdf_diff(lo, hi, T):
    """Phi(hi) - Phi(lo), lo < hi, erfc on the side of the common sign"""
    r = T(1) / np.sqrt(T(2))
    if hi <= 0:
        return (_erfc_nonneg(-hi * r, T) - _erfc_nonneg(-lo * r, T)) / T(2)
    if lo >= 0:
        return (_erfc_nonneg(lo * r, T) - _erfc_nonneg(hi * r, T)) / T(2)
    return (T(1) - _erfc_nonneg(-lo * r, T) / T(2)) - _erfc_nonneg(hi * r, T) / T(2)


def normal_pdf(x, T):
    if abs(x) == T(np.inf):
        return T(0)
    return np.exp(-x * x / T(2)) / np.sqrt(T(8) * np.arctan(T(1)))


def _r2(A, B, lengths, T):
    A, B = np.asarray(A, dtype=np.float64).astype(T), np.asarray(B, dtype=np.float64).astype(T)
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=T)
    for i in range(A.shape[1]):
        diff = (A[:, i][:, None] - B[:, i][None, :]) / T(lengths[i])
        r2 += diff * diff
    return r2


def covariance(cov_type, alpha, lengths, A, B, T):
    r2, alpha = _r2(A, B, lengths, T), T(alpha)
    if int(cov_type) == sr.COV_SQUARE_EXPONENTIAL:
        return alpha * np.exp(-r2 / T(2))
    arg = np.sqrt(T(5) * r2)
    return alpha * (T(1) + arg + T(5) * r2 / T(3)) * np.exp(-arg)


def grad_covariance(cov_type, alpha, lengths, P, x, T):
    """d cov(P_r, x) / d x [len(P)][dim]"""
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    r2, alpha = _r2(P, x, lengths, T)[:, 0], T(alpha)
    if int(cov_type) == sr.COV_SQUARE_EXPONENTIAL:
        first = alpha * np.exp(-r2 / T(2))
    else:
        arg = np.sqrt(T(5) * r2)
        first = T(5) / T(3) * alpha * np.exp(-arg) * (arg + T(1))
    ell2 = np.asarray(lengths, dtype=np.float64).astype(T) ** 2
    diff = np.asarray(P, dtype=np.float64).astype(T) - x.astype(T)
    return first[:, None] * diff / ell2[None, :]


class Model(object):
    """K = L L^T, K^-1 (y - mean) and the solves, in the arithmetic of T (np.longdouble or np.float64)"""

    def __init__(self, cov_type, hyper, X, y, noise, T=LD):
        hyper = np.asarray(hyper, dtype=np.float64).ravel()
        self.T, self.cov_type, self.alpha, self.lengths = T, int(cov_type), hyper[0], hyper[1:]
        self.X = np.asarray(X, dtype=np.float64)
        self.noise = float(np.asarray(noise, dtype=np.float64).ravel()[0])
        n = self.X.shape[0]
        K = self.cov(self.X, self.X)
        K[np.arange(n), np.arange(n)] += T(self.noise)
        self.L = sr.cholesky_spd(K) if T is LD else np.linalg.cholesky(K)
        self.mean = sr.constant_mean(y)
        yc = np.asarray(y, dtype=np.float64).ravel()[:n].astype(T) - T(self.mean)
        self.kinvy = self.back(self.fwd(yc))

    def cov(self, A, B):
        return covariance(self.cov_type, self.alpha, self.lengths, A, B, self.T)

    def grad_cov(self, P, x):
        return grad_covariance(self.cov_type, self.alpha, self.lengths, P, x, self.T)

    def fwd(self, B):
        """L^-1 B"""
        if self.T is LD:
            return sr.forward_solve(self.L, B)
        return _substitute(self.L, np.array(B, dtype=np.float64))

    def back(self, B):
        """L^-T B (the forward substitution of the factor with both axes reversed)"""
        B = np.array(B, dtype=self.T)
        R = self.L[::-1, ::-1].T
        if self.T is LD:
            return sr.forward_solve(np.ascontiguousarray(R), B[::-1])[::-1]
        return _substitute(np.ascontiguousarray(R), B[::-1])[::-1]


def _substitute(L, B):
    """forward substitution in float64, row by row"""
    X = np.array(B, dtype=np.float64)
    for k in range(L.shape[0]):
        X[k] = (X[k] - L[k, :k] @ X[:k]) / L[k, k]
    return X


def pad(points, dim, num_fidelity):
    """points [.][dim - num_fidelity] with the fidelity coordinates appended as ones"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, dim - num_fidelity)
    return np.hstack([points, np.ones((points.shape[0], num_fidelity))])


class DiscreteSet(object):
    """what depends on the set alone: k(X, A) and a_A = mu_n(A)"""

    def __init__(self, model, discrete, num_fidelity):
        self.model, self.nf = model, int(num_fidelity)
        self.points = pad(discrete, model.X.shape[1], self.nf)
        self.kA = model.cov(model.X, self.points)  # [N][A]
        self.a = model.T(model.mean) + self.kA.T @ model.kinvy


def lower_envelope(a, b, scale, T):
    """(hull: indices into a / b in slope order, the smallest gap of a stack decision)"""
    idx = np.arange(len(a))
    order = np.lexsort((idx, a, -b))
    stack, margin, prev_b = [], np.inf, None
    for i in order:
        if prev_b is not None and b[i] == prev_b:
            continue
        prev_b = b[i]
        while len(stack) >= 2:
            t, u = stack[-1], stack[-2]
            lhs, rhs = (a[i] - a[u]) * (b[u] - b[t]), (a[t] - a[u]) * (b[u] - b[i])
            margin = min(margin, float(abs(lhs - rhs) / ((b[u] - b[i]) * T(scale))))
            if lhs <= rhs:
                stack.pop()
            else:
                break
        stack.append(int(i))
    return stack, margin


def expected_minimum(a, b, hull, T):
    """(E[min], P [k], w [k]) of the envelope's lines"""
    k = len(hull)
    P, w = np.zeros(k, dtype=T), np.zeros(k, dtype=T)
    cuts = [T(-np.inf)] + [(a[hull[j + 1]] - a[hull[j]]) / (b[hull[j]] - b[hull[j + 1]]) for j in range(k - 1)] + [T(np.inf)]
    total = T(0)
    for j in range(k):
        P[j] = normal_cdf_diff(cuts[j], cuts[j + 1], T)
        w[j] = normal_pdf(cuts[j], T) - normal_pdf(cuts[j + 1], T)
        total += a[hull[j]] * P[j] + b[hull[j]] * w[j]
    return total, P, w


def lines(dset, x):
    """(a [A + 1], b [A + 1], s^2, and what the gradient reuses) of the candidate x [dim]; line 0 is x^'s"""
    m, T = dset.model, dset.model.T
    x = np.asarray(x, dtype=np.float64).ravel()
    dim = x.size
    xh = x.copy()
    if dset.nf:
        xh[dim - dset.nf:] = 1.0
    kx, kh = m.cov(m.X, x[None, :])[:, 0], m.cov(m.X, xh[None, :])[:, 0]
    kinv_kx, kinv_kh = m.back(m.fwd(kx)), m.back(m.fwd(kh))
    s2 = T(m.alpha) - kx @ kinv_kx + T(m.noise)
    s = np.sqrt(s2)
    a = np.concatenate([[T(m.mean) + kh @ m.kinvy], dset.a])
    Z = np.vstack([xh[None, :], dset.points])
    num = m.cov(Z, x[None, :])[:, 0] - np.concatenate([[kh @ kinv_kx], dset.kA.T @ kinv_kx])  # Sigma_n(z, x)
    return a, num / s, s2, (x, xh, Z, num, kinv_kx, kinv_kh)


def evaluate(dset, x, best, want_grad=True):
    m, T = dset.model, dset.model.T
    a, b, s2, (x, xh, Z, num, kinv_kx, kinv_kh) = lines(dset, x)
    dim, free = x.size, x.size - dset.nf
    scale = max(1.0, float(np.max(np.abs(a))), math.sqrt(m.alpha))
    hull, margin = lower_envelope(a, b, scale, T)
    emin, P, w = expected_minimum(a, b, hull, T)
    value = min(T(best), a[0]) - emin
    margins = (margin, float(abs(a[0] - T(best))) / scale)
    grad = None
    if want_grad:
        s = np.sqrt(s2)
        gX_x, gX_h = m.grad_cov(m.X, x), m.grad_cov(m.X, xh)  # [N][dim]
        grad_mu = np.zeros(dim, dtype=T)
        grad_mu[:free] = (m.kinvy @ gX_h)[:free]
        grad_s2 = -T(2) * (kinv_kx @ gX_x)
        g = np.zeros(dim, dtype=T)
        for j, z in enumerate(hull):
            kinv_kz = kinv_kh if z == 0 else m.back(m.fwd(dset.kA[:, z - 1]))
            grad_num = m.grad_cov(Z[z][None, :], x)[0] - kinv_kz @ gX_x  # the second argument of Sigma_n(z, x)
            if z == 0:  # x^ moves with x on the free coordinates: the first argument (d k(x^, x) / d x^ is zero there)
                first_arg = -(kinv_kx @ gX_h)
                grad_num[:free] += first_arg[:free]
                g += P[j] * grad_mu
            g += w[j] * (grad_num / s - num[z] * grad_s2 / (T(2) * s * s2))
        grad = (grad_mu if a[0] < T(best) else T(0) * grad_mu) - g
    return Result(value, emin, grad, len(hull), hull, a, b, s2, margins, scale)


def two_line_emin(a0, b0, a1, b1, T=LD):
    """E[min(a0 + b0 Z, a1 + b1 Z)] in closed form: with b0 > b1 and the crossing c = (a1 - a0) / (b0 - b1),
    a0 Phi(c) + a1 (1 - Phi(c)) - (b0 - b1) phi(c)"""
    a0, b0, a1, b1 = T(a0), T(b0), T(a1), T(b1)
    if b0 == b1:
        return min(a0, a1)
    if b0 < b1:
        a0, b0, a1, b1 = a1, b1, a0, b0
    cut = (a1 - a0) / (b0 - b1)
    r = T(1) / np.sqrt(T(2))
    Phi = (T(1) - _erfc_nonneg(cut * r, T) / T(2)) if cut >= 0 else _erfc_nonneg(-cut * r, T) / T(2)
    return a0 * Phi + a1 * (T(1) - Phi) - (b0 - b1) * normal_pdf(cut, T)


# ---- the cases of tests/test_gpu_kg1.py (tests/test_kg1_reference.py holds the float64 restatement to them on the CPU) ----
Case = collections.namedtuple("Case", "name seed n d A cov_type noise nf C")
SE, MATERN = sr.COV_SQUARE_EXPONENTIAL, sr.COV_MATERN_NU_2P5
GPU_CASES = [
    Case("n5_d2_A1", 1, 5, 2, 1, MATERN, 1e-2, 0, 7),
    Case("n20_d3_A63_fid", 2, 20, 3, 63, MATERN, 1e-2, 1, 7),
    Case("n70_d4_A64", 3, 70, 4, 64, MATERN, 1e-2, 0, 1),
    Case("n70_d4_A64_se", 4, 70, 4, 64, SE, 1e-2, 0, 7),
    Case("n70_d4_A65", 5, 70, 4, 65, MATERN, 1e-2, 0, 7),
    Case("n5_d2_A255", 6, 5, 2, 255, MATERN, 1e-2, 0, 7),
    Case("n8_d2_A4000", 7, 8, 2, 4000, MATERN, 1e-3, 0, 1),
    Case("n40_d8_A300_fid", 8, 40, 8, 300, MATERN, 1e-2, 1, 7),
    Case("n150_d6_A1000", 9, 150, 6, 1000, MATERN, 1e-2, 0, 7),
    # padded dimensions 12 (with a fidelity coordinate), 16, 24 and 32, each with and without fidelity coordinates: every
    # instantiation of the gradient kernel the cases above leave out; A = 63 / 64 / 65 around a wavefront of lines
    Case("n20_d12_A63_fid", 45, 20, 12, 63, MATERN, 1e-2, 1, 7),
    Case("n20_d16_A63", 41, 20, 16, 63, MATERN, 1e-2, 0, 7),
    Case("n20_d17_A64_fid", 42, 20, 17, 64, SE, 1e-2, 1, 7),
    Case("n24_d24_A65_fid2", 43, 24, 24, 65, MATERN, 1e-2, 2, 7),
    Case("n20_d32_A63_fid", 44, 20, 32, 63, MATERN, 1e-2, 1, 7),
    Case("n20_d18_A64", 46, 20, 18, 64, MATERN, 1e-2, 0, 7),  # (24 and 32 without a fidelity coordinate, d below the padded dimension)
    Case("n20_d25_A65", 47, 20, 25, 65, SE, 1e-2, 0, 7),
    Case("n20_d14_A63_fid", 48, 20, 14, 63, MATERN, 1e-2, 1, 7),  # (16 with a fidelity coordinate)
    # (the last case stays last: tests/test_gpu_kg1.py takes it by position)
    Case("n300_d12_A4095", 10, 300, 12, 4095, MATERN, 1e-2, 0, 1027),  # passes of 1024 candidates: C straddles one
]

Problem = collections.namedtuple("Problem", "case hyper X y noise discrete points best checked")


def make_problem(case):
    """the inputs of a case; `checked`: the candidates held against this module (all of them up to 7, else both sides of the pass
    boundary)"""
    rng = np.random.default_rng(7000 + case.seed)
    X = rng.uniform(0, 1, size=(case.n, case.d))
    y = rng.normal(size=(case.n, 1))
    hyper = np.array([1.3] + [0.1 + 0.25 * math.sqrt(case.d)] * case.d)
    discrete = rng.uniform(0, 1, size=(case.A, case.d - case.nf))
    points = rng.uniform(0, 1, size=(case.C, case.d))
    checked = tuple(range(case.C)) if case.C <= 7 else (0, 1023, 1024, case.C - 1)
    return Problem(case, hyper, X, y, [case.noise], discrete, points, float(y.min()), checked)


_WANT = {}


def expected(case, T=LD):
    """(problem, {candidate index: Result}) of a case in the arithmetic of T, computed once per process"""
    key = (case.name, T)
    if key not in _WANT:
        p = make_problem(case)
        dset = DiscreteSet(Model(case.cov_type, p.hyper, p.X, p.y, p.noise, T), p.discrete, case.nf)
        _WANT[key] = (p, {i: evaluate(dset, p.points[i], p.best) for i in p.checked})
    return _WANT[key]
