"""Joint posterior draws of a GP without derivative observations in extended precision (np.longdouble, 64-bit mantissa): the
checker of tests/test_gpu_sampling_edges.py, itself held to the reference's recorded results by tests/test_sampling_reference.py.

Written from the formulas (SamplePointsFromGP, gpp_math.cpp:1800-1848, states them):
    K        = cov(X, X) + noise I,  K = L L^T
    mean     = the arithmetic mean of y, summed in observation order IN DOUBLE as the reference forms it
    mu       = mean + K*^T K^-1 (y - mean),   K* = cov(X, U)
    Var      = cov(U, U) - K*^T K^-1 K* = cov(U, U) - V^T V,  V = L^-1 K*
    Var      = F F^T by the outer-product algorithm with the pivot rule `pivot > 1e-16` (ComputeCholeskyFactorL,
               gpp_linear_algebra.cpp:109-148); on a failing pivot either stop there (the reference: the columns before it factored,
               the Schur complement left in the lower triangle behind it, return code pivot + 1) or zero that column and go on
    y_d      = mu + tril(F) z_d;  argmin: best = y[0], index -1, replaced on a strictly smaller value
covariances: square exponential alpha exp(-r2 / 2), Matern nu = 5/2 alpha (1 + sqrt(5 r2) + 5 r2 / 3) exp(-sqrt(5 r2)), with
r2 = sum_i (x_i - x'_i)^2 / length_i^2.

Only the result is rounded to double.  Cost: N^3 / 3 + N^2 C + N C^2 extended multiply-adds at ~2e8 / s (N = 1500, C = 300: ~10 s).
"""
import numpy as np

LD = np.longdouble

# The x87 80-bit format on the x86 hosts this suite runs on.  Anything narrower (longdouble == double on some platforms) would make
# this module no better than the code it checks: refuse loudly.
assert np.finfo(LD).eps < 1e-18, (
    "tests/sampling_reference.py needs an extended-precision np.longdouble (eps %.3g found, < 1e-18 wanted): on this platform "
    "longdouble is no wider than the arithmetic under test" % float(np.finfo(LD).eps))

COV_SQUARE_EXPONENTIAL, COV_MATERN_NU_2P5 = 0, 1
PIVOT_MIN = LD("1e-16")
_BLOCK = 64


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def covariance(cov_type, alpha, lengths, A, B):
    """cov(A, B) [len(A)][len(B)] in extended precision."""
    A, B, ell = _ld(A), _ld(B), _ld(lengths).ravel()
    alpha = LD(float(alpha))
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for i in range(A.shape[1]):
        diff = (A[:, i][:, None] - B[:, i][None, :]) / ell[i]
        r2 += diff * diff
    if int(cov_type) == COV_SQUARE_EXPONENTIAL:
        return alpha * np.exp(-r2 / LD(2))
    if int(cov_type) != COV_MATERN_NU_2P5:
        raise ValueError("cov_type %r" % (cov_type,))
    arg = np.sqrt(LD(5) * r2)
    return alpha * (LD(1) + arg + LD(5) * r2 / LD(3)) * np.exp(-arg)


def cholesky_spd(a):
    """Lower factor of a positive definite matrix (blocked, left-looking).  No pivot rule: for K, which is regular by its noise."""
    a = np.array(a, dtype=LD)
    n = a.shape[0]
    for j in range(0, n, _BLOCK):
        je = min(n, j + _BLOCK)
        if j:
            a[j:, j:je] -= a[j:, :j] @ a[j:je, :j].T
        for k in range(j, je):
            if not a[k, k] > 0:
                raise np.linalg.LinAlgError("pivot %d of K is not positive" % k)
            a[k, k] = np.sqrt(a[k, k])
            a[k + 1:, k] /= a[k, k]
            if k + 1 < je:
                a[k + 1:, k + 1:je] -= np.outer(a[k + 1:, k], a[k + 1:je, k])
    return np.tril(a)


def forward_solve(L, B):
    """L^-1 B for a lower-triangular L (blocked forward substitution)."""
    X = np.array(B, dtype=LD)
    if X.ndim == 1:
        return forward_solve(L, X[:, None])[:, 0]
    n = L.shape[0]
    for j in range(0, n, _BLOCK):
        je = min(n, j + _BLOCK)
        if j:
            X[j:je] -= L[j:je, :j] @ X[:j]
        for k in range(j, je):
            X[k] /= L[k, k]
            if k + 1 < je:
                X[k + 1:je] -= np.outer(L[k + 1:je, k], X[k])
    return X


def outer_product_cholesky(var, stop_at_failure=True):
    """ComputeCholeskyFactorL's algorithm on the lower triangle of var, in the arithmetic of var's dtype.

    Returns (rc, F): rc = 0, or the first failing pivot + 1.  F is the lower triangle the draws use: with stop_at_failure the
    factored columns followed by the untouched Schur complement (what the reference goes on to multiply with), otherwise the
    factor of the positive semi-definite matrix with every failing column zeroed."""
    a = np.array(var)
    n = a.shape[0]
    floor = a.dtype.type(PIVOT_MIN)
    rc = 0
    for k in range(n):
        if a[k, k] > floor:
            a[k, k] = np.sqrt(a[k, k])
            a[k + 1:, k] /= a[k, k]
            if k + 1 < n:
                a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k + 1:, k])
        else:
            if rc == 0:
                rc = k + 1
            if stop_at_failure:
                break
            a[k:, k] = 0
    return rc, np.tril(a)


def reference_argmin(y):
    """SamplePointsFromGP's scan: the first index of the minimum, -1 when y[0] is a minimum."""
    y = np.asarray(y)
    i = int(np.argmin(y))  # (numpy: the first occurrence)
    return i if y[i] < y[0] else -1


def constant_mean(y):
    """The mean of the observed values, accumulated in double in observation order (the value the reference subtracts)."""
    total = 0.0
    for v in np.asarray(y, dtype=np.float64).ravel():
        total += float(v)
    return total / np.asarray(y).size


class Posterior(object):
    """The GP's side of the computation (K, its factor, K^-1 (y - mean)): built once, queried for many candidate sets."""

    def __init__(self, cov_type, hyper, X, y, noise):
        hyper = np.asarray(hyper, dtype=np.float64).ravel()
        self.cov_type, self.alpha, self.lengths = int(cov_type), hyper[0], hyper[1:]
        self.X = np.asarray(X, dtype=np.float64)
        n = self.X.shape[0]
        K = covariance(self.cov_type, self.alpha, self.lengths, self.X, self.X)
        K[np.arange(n), np.arange(n)] += LD(float(np.asarray(noise, dtype=np.float64).ravel()[0]))
        self.L = cholesky_spd(K)
        self.mean = constant_mean(y)
        self.v_y = forward_solve(self.L, _ld(y).ravel() - LD(self.mean))  # L^-1 (y - mean)

    def mu_var(self, pts):
        """(mu [C], Var [C][C]) in extended precision."""
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, self.X.shape[1])
        V = forward_solve(self.L, covariance(self.cov_type, self.alpha, self.lengths, self.X, pts))
        mu = LD(self.mean) + V.T @ self.v_y
        var = covariance(self.cov_type, self.alpha, self.lengths, pts, pts) - V.T @ V
        return mu, var

    def draws(self, pts, normals, stop_at_failure=True):
        mu, var = self.mu_var(pts)
        return draws_from(mu, var, normals, stop_at_failure) + (mu, var)


def draws_from(mu, var, normals, stop_at_failure=True):
    """(values [D][C] double, argmin [D], rc, F extended) from a mean and a covariance given in any precision."""
    mu, var = np.asarray(mu).astype(LD), np.asarray(var).astype(LD)
    rc, F = outer_product_cholesky(var, stop_at_failure)
    Z = _ld(normals).reshape(-1, mu.shape[0])
    values = (mu[None, :] + Z @ F.T).astype(np.float64)
    return values, np.array([reference_argmin(v) for v in values], dtype=np.int32), rc, F


def sample(cov_type, hyper, X, y, noise, pts, normals, stop_at_failure=True):
    """values [D][C] (rounded to double), argmin [D], rc -- the whole operation for one candidate set."""
    values, argmin, rc = Posterior(cov_type, hyper, X, y, noise).draws(pts, normals, stop_at_failure)[:3]
    return values, argmin, rc
