"""Batch lower-confidence-bound selection (cpp_wrappers/lower_confidence_bound.py: lower_confidence_bound_optimization) restated
twice, as the checkers of tests/test_gpu_lcb.py; tests/test_lcb_reference.py holds the two to each other and to the reference's own
function.

  literal(gp_like, candidates, q)   the reference's steps, one by one, over any object with
                                        mean(pts) -> [k],  chol_var(pt [1][dim]) -> flat factor (entry 0 = sqrt(var)),
                                        with_point(pt) -> the same GP rebuilt with pt added as a zero-valued observation;
                                    OrcLike wraps oracle.orc.OrcGP that way (any derivative observations);
  extended(post, noise, cand, q)    the same selection in extended precision on tests/sampling_reference.py's Posterior (no
                                    derivative observations, both covariances): the picks extend the factor row by row instead of
                                    rebuilding it -- var_t(c) = var_{t-1}(c) - w_t(c)^2,
                                    w_t(c) = [k(c, s) - V_c . V_s] / sqrt(k(s, s) + noise - |V_s|^2) with V carrying the earlier rows.

Both return a Selection: index [q], mean [C], var [C], kept (the size of {i : target_i <= min ucb}), margins.  The margins are what
an exact comparison of indices rests on: the gap between winner and runner-up of every argmin / argmax (q of them), and the smallest
|target_i - min(ucb)| over candidates other than the ucb minimiser (for that one the gap is 2 std by construction)."""
import collections

import numpy as np

from oracle import orc
from sampling_reference import LD, covariance, forward_solve

Selection = collections.namedtuple("Selection", "index mean var kept margins")


def _gap(values, largest):
    """winner minus runner-up (as a positive number) of an argmax / argmin over values; inf for a single value"""
    v = np.sort(np.asarray(values, dtype=np.float64))
    if v.size < 2:
        return np.inf
    return float(v[-1] - v[-2]) if largest else float(v[1] - v[0])


def _keep_margin(target, ucb):
    """smallest |target_i - min ucb| over i other than the ucb minimiser"""
    j = int(np.argmin(ucb))
    others = np.delete(np.abs(np.asarray(target, dtype=np.float64) - float(ucb[j])), j)
    return float(others.min()) if others.size else np.inf


class OrcLike(object):
    """oracle.orc.OrcGP behind the three methods literal() needs."""

    def __init__(self, cov_type, hyper, X, y, noise, derivs=()):
        self.args = (int(cov_type), np.asarray(hyper, dtype=np.float64), np.asarray(X, dtype=np.float64),
                     np.asarray(y, dtype=np.float64).reshape(len(X), 1 + len(derivs)), np.asarray(noise, dtype=np.float64),
                     tuple(derivs))
        cov_type, hyper, X, y, noise, derivs = self.args
        self.gp = orc.OrcGP(cov_type, hyper[0], hyper[1:], X, y, noise, list(derivs))

    def mean(self, pts):
        return self.gp.mean(pts)

    def chol_var(self, pt):
        return self.gp.chol_var(pt)

    def with_point(self, pt):
        cov_type, hyper, X, y, noise, derivs = self.args
        return OrcLike(cov_type, hyper, np.vstack([X, np.reshape(pt, (1, -1))]), np.vstack([y, np.zeros((1, y.shape[1]))]), noise,
                       derivs)


def literal(gp_like, candidates, q):
    """lower_confidence_bound.py:52-79, step for step (the GP handed in is not modified: every round rebuilds)."""
    cand = np.asarray(candidates, dtype=np.float64)
    mean = np.asarray(gp_like.mean(cand), dtype=np.float64)
    std = np.array([np.ravel(gp_like.chol_var(cand[[i], :]))[0] for i in range(cand.shape[0])])
    target, ucb = mean - std, mean + std
    index = [int(np.argmin(target))]
    margins = [_gap(target, False), _keep_margin(target, ucb)]
    condition = target <= np.min(ucb)
    kept_idx = np.flatnonzero(condition)
    kept_pts = cand[condition, :]
    for _ in range(1, q):
        gp_like = gp_like.with_point(cand[index[-1]])
        cstd = np.array([np.ravel(gp_like.chol_var(kept_pts[[j], :]))[0] for j in range(kept_pts.shape[0])])
        index.append(int(kept_idx[int(np.argmax(cstd))]))
        margins.append(_gap(cstd, True))
    return Selection(np.array(index), mean, std * std, int(kept_idx.size), margins)


def extended(post, noise, candidates, q):
    """The selection in extended precision over a sampling_reference.Posterior; only comparisons' inputs are rounded to double."""
    cand = np.asarray(candidates, dtype=np.float64)
    ctype, alpha, ell = post.cov_type, post.alpha, post.lengths
    V = forward_solve(post.L, covariance(ctype, alpha, ell, post.X, cand))  # [N][C]
    mean = LD(post.mean) + V.T @ post.v_y
    kcc = covariance(ctype, alpha, ell, cand[:1], cand[:1])[0, 0]  # k(c, c) = alpha for every c
    var = kcc - (V * V).sum(axis=0)
    std = np.sqrt(var)
    target, ucb = (mean - std).astype(np.float64), (mean + std).astype(np.float64)
    index = [int(np.argmin(target))]
    margins = [_gap(target, False), _keep_margin(target, ucb)]
    kept_idx = np.flatnonzero(target <= np.min(ucb))
    Vk, cvar = V[:, kept_idx], var[kept_idx].copy()
    noise = LD(float(np.ravel(noise)[0]))
    for _ in range(1, q):
        s = index[-1]
        pos = int(np.flatnonzero(kept_idx == s)[0])  # (every pick is a kept candidate)
        vs = Vk[:, pos]
        pivot = kcc + noise - vs @ vs
        if not pivot > LD("1e-16"):
            raise np.linalg.LinAlgError("conditioning pivot %g" % float(pivot))
        w = (covariance(ctype, alpha, ell, cand[kept_idx], cand[[s]])[:, 0] - Vk.T @ vs) / np.sqrt(pivot)
        Vk = np.vstack([Vk, w[None, :]])
        cvar = cvar - w * w
        cstd = np.sqrt(np.maximum(cvar, 0)).astype(np.float64)
        index.append(int(kept_idx[int(np.argmax(cstd))]))
        margins.append(_gap(cstd, True))
    return Selection(np.array(index), mean.astype(np.float64), var.astype(np.float64), int(kept_idx.size), margins)
