"""q,p-EI by Monte Carlo, value and gradient, of a GP without derivative observations in extended precision (np.longdouble, 64-bit
mantissa): the checker of tests/test_gpu_ei_edges.py, itself held to the reference's recorded results and to the double-precision
oracle by tests/test_ei_reference.py.

Written from the formulas (the header comment of csrc/ei.hip states them; K, its factor and the constant mean as
tests/sampling_reference.py builds them):
    U        = [points_to_sample (q); points_being_sampled (p)],  u = q + p
    K        = cov(X, X) + noise I,  a = K^-1 (y - mean),  A = K^-1 K*,  K* = cov(X, U)
    mu       = mean + K*^T a,   Var = cov(U, U) - K*^T A,   V = Var + 1e-6 I = L L^T
    y_s      = mu + L z_s,  t_sj = best - y_sj,  w_s = the first index of max_j t_sj,  I_s = max(0, t_{s, w_s})
    EI       = sum_s I_s / M
    grad EI[k, :] = -(1 / M) sum_{s: I_s > 0} ( [w_s == k] grad mu_k + sum_{j <= w_s} dL[w_s][j] / dU_k z_sj ),   k < q
    grad mu_k     = (d K*_k / dU_k)^T a
    dV / dU_{k, i}: row and column k only -- entry (k, j), j != k: d cov(U_k, U_j) / dU_{k, i} - (d K*_k / dU_{k, i})^T A_j;
                    entry (k, k): -2 (d K*_k / dU_{k, i})^T A_k  (cov(x, x) = alpha is constant)
    dL from dV by Smith's recursion, the derivative of the outer-product Cholesky algorithm column by column:
        dL_kk = dV_kk / (2 L_kk);  dL_jk = (dV_jk - L_jk dL_kk) / L_kk;  dV_ij -= dL_ik L_jk + L_ik dL_jk   (i, j > k)
covariances and their derivatives in the first argument, r2 = sum_i (x_i - x'_i)^2 / length_i^2:
    square exponential  alpha exp(-r2 / 2),                 d / dx_i = -alpha exp(-r2 / 2) (x_i - x'_i) / length_i^2
    Matern nu = 5/2     alpha (1 + s + s^2 / 3) exp(-s),    d / dx_i = -(5 / 3) alpha (1 + s) exp(-s) (x_i - x'_i) / length_i^2,  s = sqrt(5 r2)

Besides EI and its gradient an evaluation returns, per sample, the two margins its decisions were taken with: |t_{s, w_s}| (the sign
decides whether the sample counts) and the gap between the largest and the second largest t_sj (it decides w_s).  A device result
can be held to this module at a rounding-sized tolerance only where no margin is rounding-sized; tests/test_ei_reference.py asserts
that for every shape the device tests use.

K^-1 B: through the extended Cholesky factor (sampling_reference.cholesky_spd, N^3 / 3 extended multiply-adds at ~2e8 / s) up to
DIRECT_MAX_N rows; above, by iterative refinement -- x += K64^-1 (B - K x) with the residual in extended precision and K64^-1 from
LAPACK -- which converges by cond(K) 2^-53 per step to the same cond(K) 2^-64 accuracy, at N^2 extended multiply-adds per column and
step (N = 2632: 2 s instead of 30).  The refinement stops when its correction\nno longer shrinks -- the rounding floor of the extended residual -- refuses a floor above 1e-13 of max |x|, and is held to the direct\nsolve by the CPU test.
"""
import numpy as np

import sampling_reference as sr
from sampling_reference import COV_MATERN_NU_2P5, COV_SQUARE_EXPONENTIAL, LD  # noqa: F401  (re-exported)

JITTER = LD("1e-6")
DIRECT_MAX_N = 400


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def grad_covariance(cov_type, alpha, lengths, A, B):
    """d cov(A_k, B_j) / d A_{k, i} as [len(A)][dim][len(B)] in extended precision."""
    A, B, ell = _ld(A), _ld(B), _ld(lengths).ravel()
    alpha = LD(float(alpha))
    diff = (A[:, :, None] - B.T[None, :, :]) / (ell * ell)[None, :, None]      # (x_i - x'_i) / length_i^2
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for i in range(A.shape[1]):
        t = (A[:, i][:, None] - B[:, i][None, :]) / ell[i]
        r2 += t * t
    if int(cov_type) == COV_SQUARE_EXPONENTIAL:
        radial = -alpha * np.exp(-r2 / LD(2))
    elif int(cov_type) == COV_MATERN_NU_2P5:
        s = np.sqrt(LD(5) * r2)
        radial = -(LD(5) / LD(3)) * alpha * (LD(1) + s) * np.exp(-s)
    else:
        raise ValueError("cov_type %r" % (cov_type,))
    return radial[:, None, :] * diff


def backward_solve(L, B):
    """L^-T B for a lower-triangular L: the forward substitution of the index-reversed system."""
    return sr.forward_solve(L[::-1, ::-1].T, np.asarray(B, dtype=LD)[::-1])[::-1]


def smith_factor_derivative(L, dV):
    """dL [B][u][u] (lower triangles) of the factor L of V for B symmetric perturbations dV [B][u][u], by Smith's recursion."""
    L = np.asarray(L, dtype=LD)
    dV = np.array(dV, dtype=LD)
    u = L.shape[0]
    dL = np.zeros_like(dV)
    for k in range(u):
        dL[:, k, k] = dV[:, k, k] / (LD(2) * L[k, k])
        if k + 1 == u:
            break
        col, below = L[k + 1:, k], dL[:, k + 1:, k]
        below[...] = (dV[:, k + 1:, k] - col[None, :] * dL[:, k, k][:, None]) / L[k, k]
        dV[:, k + 1:, k + 1:] -= below[:, :, None] * col[None, None, :] + col[None, :, None] * below[:, None, :]
    return dL


class Evaluation(object):
    """ei, grad [q][dim] or None (extended precision; round with float() / .astype), and per sample zero_margin = |t_{s, w_s}|,
    winner_margin = largest minus second largest t_sj (inf for u = 1), with scale = max(1, |best|, max |y|) to measure them against."""

    def near_ties(self, band=1e-9):
        lim = LD(band) * self.scale
        return int(np.count_nonzero((self.zero_margin <= lim) | (self.winner_margin <= lim)))


class EiReference(object):
    """The GP's side (K, a = K^-1 (y - mean)): built once, queried for many point sets."""

    def __init__(self, cov_type, hyper, X, y, noise, refine=None):
        hyper = np.asarray(hyper, dtype=np.float64).ravel()
        self.cov_type, self.alpha, self.lengths = int(cov_type), hyper[0], hyper[1:]
        self.X = np.asarray(X, dtype=np.float64)
        n = self.X.shape[0]
        self.K = sr.covariance(self.cov_type, self.alpha, self.lengths, self.X, self.X)
        self.K[np.arange(n), np.arange(n)] += LD(float(np.asarray(noise, dtype=np.float64).ravel()[0]))
        self.mean = sr.constant_mean(np.asarray(y, dtype=np.float64).reshape(n, -1)[:, 0])
        self.refine = (n > DIRECT_MAX_N) if refine is None else bool(refine)
        if self.refine:
            self.K64_inv = np.linalg.inv(self.K.astype(np.float64))
        else:
            self.L = sr.cholesky_spd(self.K)
        self.a = self.k_inverse_times(_ld(np.asarray(y).reshape(n, -1)[:, 0]) - LD(self.mean))

    def k_inverse_times(self, B):
        B = np.asarray(B, dtype=LD)
        if not self.refine:
            return backward_solve(self.L, sr.forward_solve(self.L, B))
        x = (self.K64_inv @ B.astype(np.float64)).astype(LD)
        last = None
        for _ in range(12):
            dx = (self.K64_inv @ (B - self.K @ x).astype(np.float64)).astype(LD)
            x = x + dx
            step = np.abs(dx).max() / np.abs(x).max()
            if step <= LD(2) ** -56 or (last is not None and step > last / 4):   # converged, or at the rounding floor of the residual
                break
            last = step
        if step > LD("1e-13"):
            raise np.linalg.LinAlgError("refinement of K^-1 B stalled at a correction of %.3g" % float(step))
        return x

    def state(self, Xq, Xp, want_grad=True):
        """(mu [u], L [u][u], grad_mu [q][dim], dL [q][dim][u][u]); the last two None without want_grad."""
        d = self.X.shape[1]
        Xq = np.asarray(Xq, dtype=np.float64).reshape(-1, d)
        q = Xq.shape[0]
        U = Xq if Xp is None or np.size(Xp) == 0 else np.vstack([Xq, np.asarray(Xp, dtype=np.float64).reshape(-1, d)])
        u = U.shape[0]
        cov = (self.cov_type, self.alpha, self.lengths)
        Ks = sr.covariance(*cov, self.X, U)                                  # [N][u]
        A = self.k_inverse_times(Ks)
        mu = LD(self.mean) + Ks.T @ self.a
        V = sr.covariance(*cov, U, U) - Ks.T @ A
        V = (V + V.T) / LD(2)
        V[np.arange(u), np.arange(u)] += JITTER
        L = sr.cholesky_spd(V)
        if not want_grad:
            return mu, L, None, None
        dKs = grad_covariance(*cov, Xq, self.X)                               # [q][dim][N]
        grad_mu = dKs @ self.a
        T = dKs @ A                                                           # [q][dim][u]
        dss = grad_covariance(*cov, Xq, U)                                    # [q][dim][u]; zero at j = k
        dV = np.zeros((q, d, u, u), dtype=LD)
        for k in range(q):
            row = dss[k] - T[k]
            row[:, k] = -LD(2) * T[k][:, k]
            dV[k, :, k, :] = row
            dV[k, :, :, k] = row
        dL = smith_factor_derivative(L, dV.reshape(q * d, u, u)).reshape(q, d, u, u)
        return mu, L, grad_mu, dL

    def ei(self, Xq, Xp, best_so_far, normals, want_grad=True):
        mu, L, grad_mu, dL = self.state(Xq, Xp, want_grad)
        u = mu.shape[0]
        Z = _ld(normals).reshape(-1, u)
        M = Z.shape[0]
        best = LD(float(best_so_far))
        Y = mu[None, :] + Z @ L.T
        T = best - Y
        w = np.argmax(T, axis=1)                                              # (numpy: the first occurrence)
        top = T[np.arange(M), w]
        counts = top > 0
        out = Evaluation()
        out.ei = np.where(counts, top, LD(0)).sum() / LD(M)
        out.zero_margin = np.abs(top)
        if u > 1:
            rest = T.copy()
            rest[np.arange(M), w] = -np.inf
            out.winner_margin = top - rest.max(axis=1)
        else:
            out.winner_margin = np.full(M, np.inf, dtype=LD)
        out.scale = max(LD(1), abs(best), np.abs(Y).max())
        out.improving = int(np.count_nonzero(counts))
        out.grad = None
        if want_grad:
            q = grad_mu.shape[0]
            zsum = np.zeros((u, u), dtype=LD)                                 # zsum[w] = sum of z_s over the counting samples won by w
            wins = np.zeros(u, dtype=LD)
            for j in np.unique(w[counts]):
                sel = counts & (w == j)
                zsum[j] = Z[sel].sum(axis=0)
                wins[j] = np.count_nonzero(sel)
            out.grad = -(wins[:q, None] * grad_mu + (dL * zsum[None, None, :, :]).sum(axis=(2, 3))) / LD(M)
        return out
