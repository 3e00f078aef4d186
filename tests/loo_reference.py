"""Host restatement of the leave-one-out (LOO) objective, numpy only (nothing imported from the product).

With K = K(X, X) + diag(noise + 1e-6) over the N = n (1 + g) scalar observations (row i (1 + g) + a: observation kind a of point i,
0 = the function value, 1 + m = the partial derivative derivs[m]), yc = the values centred on the mean of the function values:

  closed_form   alpha = K^-1 yc, kappa = diag K^-1:  mu_i = yc_i - alpha_i / kappa_i, var_i = 1 / kappa_i,
                L_LOO = sum_i 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi, and its gradient
                sum_ab (u_a alpha_b - M_ab) dK_ab with u = K^-1 (alpha / kappa), M = K^-1 diag(e) K^-1,
                e_i = 1/2 (1 + alpha_i^2 / kappa_i) / kappa_i.  dK / d(alpha, lengths) in the boundary's convention: the
                function-value block only.
  brute_force   row and column i of K deleted, row i predicted from the rest, for every i: no algebra shared with the above.

Everything in np.longdouble by default (dtype=np.float64 gives the same code in double: the gap between the two is what the
device's gradient is allowed ten times of).  The Cholesky factorisation and the triangular solves are written out.
"""
import functools

import numpy as np

SE, MATERN = 0, 1
LOG_2PI = np.longdouble("1.837877066409345483560659472811235279722794947275566825634")


def covariance(cov_type, X, derivs, alpha, lengths, dtype):
    """K(X, X) [N][N] with derivative observations, N = n (1 + g)."""
    X = np.asarray(X, dtype=dtype)
    n, d = X.shape
    g1 = 1 + len(derivs)
    il2 = 1.0 / np.asarray(lengths, dtype=dtype) ** 2
    diff = X[:, None, :] - X[None, :, :]          # x1 - x2
    r2 = np.sum(diff * diff * il2, axis=2)
    alpha = dtype(alpha)
    if cov_type == SE:
        base = alpha * np.exp(-r2 / 2)
        first = second = base
    else:
        a = np.sqrt(5 * r2)
        e = np.exp(-a)
        base = alpha * e * (1 + a + dtype(5) / 3 * r2)
        first = dtype(5) / 3 * alpha * e * (a + 1)
        second = dtype(25) / 3 * alpha * e
    K = np.zeros((n * g1, n * g1), dtype=dtype)
    K[0::g1, 0::g1] = base
    for a_, i1 in enumerate(derivs):
        u = -diff[:, :, i1] * il2[i1]
        K[1 + a_::g1, 0::g1] = first * u
        K[0::g1, 1 + a_::g1] = first * (diff[:, :, i1] * il2[i1])
        for b_, i2 in enumerate(derivs):
            v = diff[:, :, i2] * il2[i2]
            blk = u * v * second
            if i1 == i2:
                blk = blk + first * il2[i2]
            K[1 + a_::g1, 1 + b_::g1] = blk
    return K


def hyper_grad_blocks(cov_type, X, alpha, lengths, dtype):
    """dK_ff / d alpha [n][n] and dK_ff / d l_k [d][n][n] of the function-value block."""
    X = np.asarray(X, dtype=dtype)
    lengths = np.asarray(lengths, dtype=dtype)
    il2 = 1.0 / lengths ** 2
    diff = X[:, None, :] - X[None, :, :]
    d2 = diff * diff
    r2 = np.sum(d2 * il2, axis=2)
    alpha = dtype(alpha)
    if cov_type == SE:
        base = alpha * np.exp(-r2 / 2)
        first = base
    else:
        a = np.sqrt(5 * r2)
        e = np.exp(-a)
        base = alpha * e * (1 + a + dtype(5) / 3 * r2)
        first = dtype(5) / 3 * alpha * e * (a + 1)
    return base / alpha, np.array([first * d2[:, :, k] / lengths[k] ** 3 for k in range(X.shape[1])])


def cholesky(A):
    """Lower factor of a symmetric positive definite matrix, column by column; None if a pivot is not positive."""
    L = np.array(A, copy=True)
    N = L.shape[0]
    for j in range(N):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            return None
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return np.tril(L)


def solve_lower(L, B):
    Y = np.array(B, copy=True)
    for j in range(L.shape[0]):
        Y[j] = Y[j] / L[j, j]
        Y[j + 1:] -= np.multiply.outer(L[j + 1:, j], Y[j]) if Y.ndim > 1 else L[j + 1:, j] * Y[j]
    return Y


def solve_upper_t(L, B):
    """L^T Z = B"""
    Z = np.array(B, copy=True)
    for j in range(L.shape[0] - 1, -1, -1):
        Z[j] = Z[j] / L[j, j]
        Z[:j] -= np.multiply.outer(L[j, :j], Z[j]) if Z.ndim > 1 else L[j, :j] * Z[j]
    return Z


def _system(X, y, derivs, hyper, cov_type, dtype):
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    g1 = 1 + len(derivs)
    hyper = np.asarray(hyper, dtype=dtype)
    K = covariance(cov_type, X, derivs, hyper[0], hyper[1:1 + d], dtype)
    noise = hyper[1 + d:1 + d + g1] + dtype(1.0e-6)   # (the double 1e-6, as the device adds it)
    K[np.diag_indices(n * g1)] += np.tile(noise, n)
    Y = np.asarray(y, dtype=np.float64).reshape(n, g1)
    mean = dtype(np.sum(Y[:, 0]) / n)   # centred in double, as the data reach the device
    yc = Y.astype(dtype)
    yc[:, 0] -= mean
    return K, yc.ravel(), mean


def closed_form(X, y, derivs, hyper, cov_type, dtype=np.longdouble, want_grad=True):
    """-> (value, grad [1 + d + 1 + g] or None, mu [n][1 + g] in the caller's units, var [n][1 + g]); value -inf if K is singular."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    g1 = 1 + len(derivs)
    N = n * g1
    K, yc, mean = _system(X, y, derivs, hyper, cov_type, dtype)
    L = cholesky(K)
    if L is None:
        return -np.inf, None, None, None
    Kinv = solve_upper_t(L, solve_lower(L, np.eye(N, dtype=dtype)))
    alpha = Kinv @ yc
    kappa = np.diag(Kinv).copy()
    mu = yc - alpha / kappa
    var = 1 / kappa
    value = np.sum(np.log(kappa) / 2 - alpha * alpha / kappa / 2) - dtype(N) * dtype(LOG_2PI) / 2
    mu_out = mu.reshape(n, g1).copy()
    mu_out[:, 0] += mean
    grad = None
    if want_grad:
        c = alpha / kappa
        e = (1 + alpha * alpha / kappa) / kappa / 2
        u = Kinv @ c
        M = (Kinv * e) @ Kinv
        Wt = np.multiply.outer(u, alpha) - M
        dKa, dKl = hyper_grad_blocks(cov_type, X, np.asarray(hyper, dtype=dtype)[0], np.asarray(hyper, dtype=dtype)[1:1 + d], dtype)
        Wff = Wt[0::g1, 0::g1]
        grad = np.zeros(1 + d + g1, dtype=dtype)
        grad[0] = np.sum(Wff * dKa)
        for k in range(d):
            grad[1 + k] = np.sum(Wff * dKl[k])
        dg = np.diag(Wt)
        for a in range(g1):
            grad[1 + d + a] = np.sum(dg[a::g1])
    return value, grad, mu_out, var.reshape(n, g1)


def brute_force(X, y, derivs, hyper, cov_type, dtype=np.longdouble):
    """-> (value, mu [n][1 + g], var [n][1 + g]): every row predicted from the N - 1 others."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    g1 = 1 + len(derivs)
    N = n * g1
    K, yc, mean = _system(X, y, derivs, hyper, cov_type, dtype)
    mu, var = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    for i in range(N):
        keep = np.r_[0:i, i + 1:N]
        if keep.size == 0:
            mu[i], var[i] = 0, K[i, i]
            continue
        L = cholesky(K[np.ix_(keep, keep)])
        ki = K[keep, i]
        w = solve_upper_t(L, solve_lower(L, ki))
        mu[i] = w @ yc[keep]
        var[i] = K[i, i] - w @ ki
    value = np.sum(-np.log(var) / 2 - (yc - mu) ** 2 / var / 2) - dtype(N) * dtype(LOG_2PI) / 2
    mu_out = mu.reshape(n, g1).copy()
    mu_out[:, 0] += mean
    return value, mu_out, var.reshape(n, g1)


# ---- the problems of tests/test_gpu_loo.py (here so that the CPU suite checks the restatement on the same inputs) ----
# (cov_type, n, d, g): N = n (1 + g) in {1, 2, 63, 64, 65, 129, 257} -- the 64-column and 256-row block edges of the gradient's
# contraction and the 64-wide blocks of the factor and of its inverse; (d, g) in {(1,0), (3,0), (5,0), (3,2), (12,3)} -- padded
# dimensions 4, 8, 12; both kernels where g = 0.  (Padded dimensions 16, 24, 32: WIDE_CASES below.)
CASES = [
    (MATERN, 1, 1, 0), (SE, 1, 3, 0), (SE, 2, 3, 0), (MATERN, 2, 5, 0),
    (MATERN, 21, 3, 2), (SE, 63, 5, 0), (MATERN, 63, 1, 0),
    (MATERN, 16, 12, 3), (MATERN, 64, 1, 0), (SE, 64, 3, 0),
    (SE, 65, 3, 0), (MATERN, 65, 5, 0),
    (MATERN, 43, 3, 2), (SE, 129, 1, 0), (MATERN, 129, 5, 0),
    (MATERN, 257, 3, 0), (SE, 257, 5, 0),
]
SE_DERIV_CASE = (SE, 21, 3, 2)   # value and predictions only: the gradient with derivative observations is Matern-5/2's
# Padded dimensions 16, 24 and 32, at both ends of each (d = 13 / 16, 17 / 24, 25 / 32); N = 20, 30, 36 and 70 (a second 64-column
# block at d = 32).  A list of its own: grad_gap() below, the bound of the device's gradient, stays a maximum over CASES alone.
WIDE_CASES = [
    (MATERN, 20, 13, 0), (SE, 20, 16, 0), (MATERN, 20, 17, 0), (SE, 30, 24, 0),
    (MATERN, 12, 25, 2), (SE, 20, 32, 0), (MATERN, 70, 32, 0),
]


def case_id(case):
    return "%s_n%d_d%d_g%d" % ("se" if case[0] == SE else "matern", case[1], case[2], case[3])


def make_problem(case, num_sets=1):
    """Points uniform in the unit cube, smooth values + noise, hyper-parameters with lengths in [0.3, 1] and noise >= 1e-2 (the
    restatement alone stays within 1e-12 of the brute force there).  -> X, y, derivs, hyper [num_sets][1 + d + 1 + g]"""
    cov_type, n, d, g = case
    rng = np.random.RandomState(1000 * n + 10 * d + g + 7 * cov_type)
    X = rng.uniform(size=(n, d))
    y = np.zeros((n, 1 + g))
    y[:, 0] = np.sin(3.0 * X[:, 0]) + 0.5 * np.cos(2.0 * X.sum(axis=1)) + 0.05 * rng.standard_normal(n) + 0.7
    derivs = list(range(g))
    for j, k in enumerate(derivs):
        y[:, 1 + j] = -np.sin(2.0 * X.sum(axis=1)) + (3.0 * np.cos(3.0 * X[:, 0]) if k == 0 else 0.0) + 0.05 * rng.standard_normal(n)
    hyper = np.c_[rng.uniform(0.5, 1.5, size=(num_sets, 1)), rng.uniform(0.3, 1.0, size=(num_sets, d)),
                  rng.uniform(1.0e-2, 1.0e-1, size=(num_sets, 1 + g))]
    return X, y, derivs, hyper


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's first hyper-parameter set through both restatements, computed once: dict(X, y, derivs, hyper, value, grad, mu,
    var (closed form, longdouble), grad64 (closed form, float64), bf_value, bf_mu, bf_var (brute force))."""
    X, y, derivs, hyper = make_problem(case)
    value, grad, mu, var = closed_form(X, y, derivs, hyper[0], case[0])
    _, grad64, _, _ = closed_form(X, y, derivs, hyper[0], case[0], dtype=np.float64)
    bf_value, bf_mu, bf_var = brute_force(X, y, derivs, hyper[0], case[0])
    return dict(X=X, y=y, derivs=derivs, hyper=hyper[0], value=value, grad=grad, mu=mu, var=var, grad64=grad64, bf_value=bf_value,
                bf_mu=bf_mu, bf_var=bf_var)


def grad_gap():
    """max over CASES and components of |grad (float64) - grad (longdouble)| / max(1, |grad (longdouble)|): what the same algebra
    loses in double on these inputs."""
    gap = 0.0
    for case in CASES:
        r = reference(case)
        gap = max(gap, float(np.max(np.abs(r["grad64"].astype(np.longdouble) - r["grad"]) / np.maximum(1, np.abs(r["grad"])))))
    return gap


# ---- the sampler problems (n = 20, d = 2, W = 12, 6 steps); the seeds are checked by tests/test_loo_reference.py ----
MCMC_CASES = [(MATERN, 20, 2, 0, 311), (MATERN, 20, 2, 1, 312)]


def mcmc_problem(case):
    """-> dict(cov_type, X, y, derivs, table, p0, tables, lnpost): default prior table, 12 walkers, 6 steps; lnpost is the log posterior
    of tests/hyper_mcmc_reference.py with the closed form above as its likelihood."""
    import hyper_mcmc_reference as hm
    cov_type, n, d, g, seed = case
    X, y, derivs = hm.make_problem(n, d, g, seed)
    nh = 1 + d + 1 + g
    table = hm.default_prior_table(nh, 1 + g)
    rng = np.random.RandomState(seed + 1000)
    p0 = hm.start_walkers(rng, 12, d, g, table)
    tables = hm.stretch_tables(rng, 6, 12)

    def lnpost(theta):
        if not np.all(np.abs(theta) <= hm.BOX):
            return -np.inf
        lp = hm.log_prior(table, theta, True)
        if lp == -np.inf:
            return -np.inf
        return lp + float(closed_form(X, y, derivs, np.exp(theta), cov_type, want_grad=False)[0])

    return dict(cov_type=cov_type, X=X, y=y, derivs=derivs, table=table, p0=p0, tables=tables, lnpost=lnpost)
