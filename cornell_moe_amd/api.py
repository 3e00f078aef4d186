"""numpy-level wrappers over the C ABI (include/moe_hip.h).  Thin: argument marshalling + error mapping only.

Exceptions mirror the reference's Python-visible classes (gpp_python.cpp:71-124, 285-379):
OptimalLearningException, BoundsException(value, min, max), InvalidValueException(value, truth, tolerance),
SingularMatrixException(num_rows, leading_minor_index).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp, ip


class OptimalLearningException(Exception):
    pass


class BoundsException(OptimalLearningException):
    def __init__(self, message, value=0.0, min=0.0, max=0.0):  # noqa: A002  (names follow gpp_python.cpp:315-317)
        super(BoundsException, self).__init__(message)
        self.value, self.min, self.max = value, min, max


class InvalidValueException(OptimalLearningException):
    def __init__(self, message, value=0.0, truth=0.0, tolerance=0.0):
        super(InvalidValueException, self).__init__(message)
        self.value, self.truth, self.tolerance = value, truth, tolerance


class SingularMatrixException(OptimalLearningException):
    def __init__(self, message, num_rows=0, leading_minor_index=0):
        super(SingularMatrixException, self).__init__(message)
        self.num_rows, self.leading_minor_index = int(num_rows), int(leading_minor_index)


def _raise(err):
    msg = err.message.decode("utf-8", "replace")
    p = list(err.payload)
    if err.code == _lib.MOE_ERR_BOUNDS:
        raise BoundsException(msg, p[0], p[1], p[2])
    if err.code == _lib.MOE_ERR_INVALID_VALUE:
        raise InvalidValueException(msg, p[0], p[1], p[2])
    if err.code == _lib.MOE_ERR_SINGULAR:
        raise SingularMatrixException(msg, p[0], p[1])
    raise OptimalLearningException(msg)


def _check(rc, err):
    if rc != 0:
        _raise(err)


def _d(a):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(dp)


def fp64_rate(device=0):
    """moe_debug_fp64_rate: sustained FP64 FMA rate of the chip in TFLOP/s."""
    v = C.c_double(0.0)
    err = _lib.MoeError()
    _check(_lib.load().moe_debug_fp64_rate(int(device), C.byref(v), C.byref(err)), err)
    return v.value


def kxx_build_probe(log=None, device=0):
    """bench.py's `roofline_cov_build_kxx`: the GP's own covariance assembly where SURVEY 8(d) says it is the meaningful HBM
    measurement -- K(X, X) with derivative-observation rows at C5 (n = 2000, d = 12, g = 3: N = 8000, 512 MB) and at C5 with all
    12 partial derivatives observed (N = 26 000, 5.4 GB) -- against the 8 TB/s HBM peak."""
    from .workloads import make_workload
    out = {"bound": "hbm", "peak": 8000.0, "unit": "GB/s", "kernel": "cov_build_points_kernel (GpDev::rebuild's launch)", "cases": []}
    for derivs in ((0, 1, 2), tuple(range(12))):
        w = make_workload("C5", M=2, derivs=derivs)
        G = DeviceGP(w.hyperparameters, w.X, w.y, w.noise, w.derivs, device=device)
        ms, nbytes = G.kxx_build_probe(repeat=5 if len(derivs) > 3 else 20)
        gbs = nbytes / (ms * 1e-3) / 1e9
        out["cases"].append({"n": w.n, "d": w.d, "g": w.g, "N": w.n * (1 + w.g), "avg_launch_ms": ms, "bytes_per_launch": nbytes,
                             "achieved": gbs, "frac": gbs / 8000.0})
        if log:
            log("K(X,X) build N=%d: %.3f ms, %.0f GB/s" % (w.n * (1 + w.g), ms, gbs))
        G.close()
    out["achieved"] = out["cases"][0]["achieved"]
    out["frac"] = out["cases"][0]["frac"]
    return out


def pool_held_bytes():
    """moe_pool_held_bytes: device bytes the library's pool holds (released by destroyed objects, not yet reused)."""
    return int(_lib.load().moe_pool_held_bytes())


def pool_trim():
    """moe_pool_trim: give every pooled device / pinned buffer back to the runtime."""
    _lib.load().moe_pool_trim()


def multistart_trace():
    """moe_multistart_trace: rows (kind 0 values / 1 gradients, items, ms) of the last outer optimisation of this process."""
    L = _lib.load()
    n = L.moe_multistart_trace(None, 0)
    out = np.zeros((max(n, 1), 3))
    L.moe_multistart_trace(out.ctypes.data_as(dp), n)
    return out[:n]


def set_reference_quirks(on):
    """moe_set_reference_quirks: 1 = the multistart drivers reproduce the reference's execution, defects included (default);
    0 = the drivers as the reference intends them (fresh states, all q points move); -1 = follow MOE_REFERENCE_QUIRKS."""
    _lib.load().moe_set_reference_quirks(int(on))


def get_reference_quirks():
    return bool(_lib.load().moe_get_reference_quirks())


def set_ensemble_launches(on):
    """moe_set_ensemble_launches: 1 = the MCMC-averaged KG evaluators issue every kernel once for all ensemble members (default),
    0 = member by member, -1 = follow MOE_ENS_LAUNCH.  Same bits either way."""
    _lib.load().moe_set_ensemble_launches(int(on))


def ensemble_launch_stats():
    """(merged evaluations, member-by-member fall-backs, launches issued by merged evaluations, member launches they stand for)"""
    import ctypes
    out = (ctypes.c_longlong * 4)()
    _lib.load().moe_ensemble_launch_stats(out)
    return tuple(int(v) for v in out)


def normal_draws(seed, count):
    out = np.empty(int(count), dtype=np.float64)
    _lib.load().moe_normal_draws(C.c_uint(int(seed) & 0xFFFFFFFF), int(count), out.ctypes.data_as(dp))
    return out


def latin_hypercube(seed, bounds, num_points):
    """moe_latin_hypercube: [num_points][dim] points, one per slice of every edge (gpp_random.cpp:173-194)."""
    bounds, bp = _d(bounds)
    dim = bounds.size // 2
    out = np.zeros((int(num_points), dim))
    _lib.load().moe_latin_hypercube(C.c_uint(int(seed) & 0xFFFFFFFF), bp, dim, int(num_points), out.ctypes.data_as(dp))
    return out


def debug_cholesky(a, device=0):
    """Device Cholesky + inverse factor of an SPD matrix (parity probe); returns (L, Linv) as [row, col] arrays."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    flat = np.ascontiguousarray(a.T).ravel()
    chol = np.zeros(n * n)
    inv = np.zeros(n * n)
    info = C.c_int(0)
    err = _lib.MoeError()
    _check(_lib.load().moe_debug_cholesky(n, flat.ctypes.data_as(dp), int(device), chol.ctypes.data_as(dp),
                                          inv.ctypes.data_as(dp), C.byref(info), C.byref(err)), err)
    return chol.reshape(n, n).T.copy(), inv.reshape(n, n).T.copy()


def debug_math(x, device=0):
    """(exp(-x), sqrt(x)) evaluated by the device fast-math routines, x >= 0."""
    x, xp = _d(x)
    e = np.zeros(x.size)
    r = np.zeros(x.size)
    err = _lib.MoeError()
    _check(_lib.load().moe_debug_math(x.size, xp, int(device), e.ctypes.data_as(dp), r.ctypes.data_as(dp), C.byref(err)), err)
    return e, r


class DeviceGP(object):
    """Device-resident GP: handle around moe_gp_t (replaces the reference's C_GP.GaussianProcess object)."""

    def __init__(self, hyperparameters, X, y, noise_variance, derivatives=(), cov_type=_lib.COV_MATERN_NU_2P5, device=0):
        L = _lib.load()
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise BoundsException("points_sampled must be 2-D [num_sampled][dim]")
        self.n, self.d = X.shape
        self.derivatives = [int(v) for v in derivatives]
        self.g = len(self.derivatives)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(self.n, 1 + self.g)
        hyper, hp = _d(hyperparameters)
        noise, npn = _d(noise_variance)
        if hyper.size != 1 + self.d:
            raise InvalidValueException("hyperparameters must be [alpha, lengths...]", hyper.size, 1 + self.d, 0)
        if noise.size != 1 + self.g:
            raise InvalidValueException("noise_variance must have 1 + num_derivatives entries", noise.size, 1 + self.g, 0)
        dv = np.ascontiguousarray(self.derivatives, dtype=np.int32)
        self._h = C.c_void_p(None)
        err = _lib.MoeError()
        rc = L.moe_gp_create(hp, int(cov_type), X.ctypes.data_as(dp), y.ctypes.data_as(dp), npn,
                             dv.ctypes.data_as(ip) if self.g else None, self.g, self.d, self.n, int(device),
                             C.byref(self._h), C.byref(err))
        _check(rc, err)
        self.device = device
        self.cov_type = int(cov_type)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().moe_gp_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- bookkeeping ----
    @property
    def N(self):
        return self.n * (1 + self.g)

    def add_points(self, pts, vals):
        pts, pp = _d(pts)
        vals, vp = _d(vals)
        k = pts.reshape(-1, self.d).shape[0]
        err = _lib.MoeError()
        try:
            _check(_lib.load().moe_gp_add_points(self._h, pp, vp, k, C.byref(err)), err)
        finally:  # a failed append rolls the handle back: always mirror what the device holds
            self.n = int(_lib.load().moe_gp_num_sampled(self._h))

    def get_factor(self):
        N = self.N
        K = np.zeros(N * N)
        kiy = np.zeros(N)
        mean = C.c_double(0.0)
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_get_factor(self._h, K.ctypes.data_as(dp), kiy.ctypes.data_as(dp), C.byref(mean),
                                             C.byref(err)), err)
        return K.reshape(N, N).T.copy(), kiy, mean.value

    # ---- posterior queries (raw column-major outputs, flat) ----
    def _q(self, fn, pts, size, *extra):
        pts, pp = _d(pts)
        k = pts.reshape(-1, self.d).shape[0]
        out = np.zeros(size(k))
        err = _lib.MoeError()
        _check(fn(self._h, pp, k, *extra, out.ctypes.data_as(dp), C.byref(err)), err)
        return out

    def mean(self, pts):
        return self._q(_lib.load().moe_gp_mean, pts, lambda k: k)

    def additional_mean(self, pts):
        return self._q(_lib.load().moe_gp_additional_mean, pts, lambda k: k)

    def grad_mean(self, pts):
        return self._q(_lib.load().moe_gp_grad_mean, pts, lambda k: self.d * k * (1 + self.g))

    def variance(self, pts):
        return self._q(_lib.load().moe_gp_variance, pts, lambda k: (k * (1 + self.g)) ** 2)

    def cholesky_variance(self, pts):
        return self._q(_lib.load().moe_gp_cholesky_variance, pts, lambda k: (k * (1 + self.g)) ** 2)

    def grad_variance(self, pts, num_derivs):
        return self._q(_lib.load().moe_gp_grad_variance, pts, lambda k: self.d * (k * (1 + self.g)) ** 2 * num_derivs,
                       int(num_derivs))

    def grad_cholesky_variance(self, pts, num_derivs):
        return self._q(_lib.load().moe_gp_grad_cholesky_variance, pts,
                       lambda k: self.d * (k * (1 + self.g)) ** 2 * num_derivs, int(num_derivs))

    def sample_points(self, pts, normals):
        """moe_gp_sample_points: joint posterior draws of the function values at pts [C][dim], one per row of normals [D][C].
        Returns (values [D][C] = mu + L z, argmin [D] by the reference's rule (-1: candidate 0 is the minimum), failed_pivot: 0 or
        the failing pivot + 1 -- a failed factorisation is handled as include/moe_hip.h describes, not raised)."""
        pts, pp = _d(pts)
        C_ = pts.reshape(-1, self.d).shape[0]
        normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, C_)
        D = normals.shape[0]
        values = np.zeros((D, C_))
        argmin = np.zeros(D, dtype=np.int32)
        failed = C.c_int(0)
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_sample_points(self._h, pp, C_, normals.ctypes.data_as(dp), D, values.ctypes.data_as(dp),
                                                argmin.ctypes.data_as(ip), C.byref(failed), C.byref(err)), err)
        return values, argmin, failed.value

    def sample_global_optima(self, candidates, normals):
        """moe_gp_sample_global_optima: candidates [E][C][dim], normals [E][C] (one draw per set), all sets in one batch.
        Returns (points [E][dim], index [E] (-1: candidate 0, which is then the point), failed_pivot [E])."""
        cand = np.ascontiguousarray(candidates, dtype=np.float64)
        E, C_ = cand.shape[0], cand.shape[1]
        normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(E, C_)
        points = np.zeros((E, self.d))
        index = np.zeros(E, dtype=np.int32)
        failed = np.zeros(E, dtype=np.int32)
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_sample_global_optima(self._h, cand.ctypes.data_as(dp), C_, E, normals.ctypes.data_as(dp),
                                                       points.ctypes.data_as(dp), index.ctypes.data_as(ip),
                                                       failed.ctypes.data_as(ip), C.byref(err)), err)
        return points, index, failed

    def mean_std(self, pts):
        """moe_gp_mean_std: marginal posterior (mean [C], std [C]) of the function value at pts [C][dim]; the C x C covariance is
        never formed.  SingularMatrixException(1, i) for the first candidate i whose variance fails the pivot rule."""
        pts, pp = _d(pts)
        C_ = pts.reshape(-1, self.d).shape[0]
        mean = np.zeros(C_)
        std = np.zeros(C_)
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_mean_std(self._h, pp, C_, mean.ctypes.data_as(dp), std.ctypes.data_as(dp), C.byref(err)), err)
        return mean, std

    def lcb_select(self, candidates, q, want_surface=False):
        """moe_gp_lcb_select: batch lower-confidence-bound selection of q of the candidates [C][dim] on the device; this GP is not
        modified.  Returns (index [q], points [q][dim], num_kept), with want_surface also (mean [C], std [C]) behind them."""
        cand, cp = _d(candidates)
        C_ = cand.reshape(-1, self.d).shape[0]
        q = int(q)
        index = np.zeros(max(q, 1), dtype=np.int32)
        points = np.zeros((max(q, 1), self.d))
        mean = np.zeros(C_) if want_surface else None
        std = np.zeros(C_) if want_surface else None
        kept = C.c_int(0)
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_lcb_select(self._h, cp, C_, q, index.ctypes.data_as(ip), points.ctypes.data_as(dp),
                                             mean.ctypes.data_as(dp) if want_surface else None,
                                             std.ctypes.data_as(dp) if want_surface else None, C.byref(kept), C.byref(err)), err)
        if want_surface:
            return index, points, kept.value, mean, std
        return index, points, kept.value

    def kg_discrete(self, discrete, points, best_so_far, num_fidelity=0, want_grad=True, want_active=False,
                    points_being_sampled=None):
        """moe_gp_kg_discrete: the exact discretised one-point knowledge gradient of points [C][dim] over the discrete set
        [A][dim - num_fidelity] (a lower bound of the continuous knowledge gradient), for a GP without derivative observations.
        Returns kg [C], with want_grad (kg, grad [C][dim]), with want_active the number of lines on the envelope [C] behind them.
        SingularMatrixException(1, i) for the first candidate i with Sigma_n(x, x) + noise <= 1e-16.
        points_being_sampled [p][dim] (None or empty: the call and bits of before): the posterior covariance is conditioned on these
        pending points, the posterior mean is not (moe_kg_discrete_mcmc_pending with this GP as an ensemble of one;
        SingularMatrixException(0, j) for a pending point j that makes the conditioned covariance singular)."""
        if _num_pending(points_being_sampled, self.d):
            res = kg_discrete_ensemble(self, [discrete], points, [best_so_far], num_fidelity=num_fidelity, want_grad=want_grad,
                                       points_being_sampled=points_being_sampled)
            out = (res if want_grad else (res,))
            if want_active:
                C_ = out[0].shape[0]
                active = np.zeros(C_, dtype=np.int32)
                err = _lib.MoeError()
                _check(_lib.load().moe_gp_kg_discrete_last_active(self._h, C_, active.ctypes.data_as(ip), C.byref(err)), err)
                out = tuple(out) + (active,)
            return out[0] if len(out) == 1 else tuple(out)
        nf = int(num_fidelity)
        size = self.d - nf
        if not 0 < size <= self.d:
            size = self.d  # (the library refuses num_fidelity; the shapes only have to be readable)
        disc, dcp = _d(discrete)
        pts, pp = _d(points)
        A = disc.reshape(-1, size).shape[0]
        C_ = pts.reshape(-1, self.d).shape[0]
        kg = np.zeros(max(C_, 1))
        grad = np.zeros((max(C_, 1), self.d)) if want_grad else None
        active = np.zeros(max(C_, 1), dtype=np.int32) if want_active else None
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_kg_discrete(self._h, nf, dcp, A, pp, C_, float(best_so_far), 1 if want_grad else 0,
                                              kg.ctypes.data_as(dp), grad.ctypes.data_as(dp) if want_grad else None,
                                              active.ctypes.data_as(ip) if want_active else None, C.byref(err)), err)
        out = (kg,) + ((grad,) if want_grad else ()) + ((active,) if want_active else ())
        return out[0] if len(out) == 1 else out

    def mix_covariance(self, pts, derivs2=()):
        pts, pp = _d(pts)
        k = pts.reshape(-1, self.d).shape[0]
        g2 = len(derivs2)
        dv = np.ascontiguousarray(list(derivs2), dtype=np.int32)
        out = np.zeros(self.N * k * (1 + g2))
        err = _lib.MoeError()
        _check(_lib.load().moe_gp_mix_covariance(self._h, pp, k, dv.ctypes.data_as(ip) if g2 else None, g2,
                                                 out.ctypes.data_as(dp), C.byref(err)), err)
        return out.reshape(k * (1 + g2), self.N).T.copy()

    def cov_build_probe(self, pts, repeat=10):
        pts, pp = _d(pts)
        k = pts.reshape(-1, self.d).shape[0]
        ms, nbytes = C.c_double(0.0), C.c_double(0.0)
        err = _lib.MoeError()
        _check(_lib.load().moe_cov_build_probe(self._h, pp, k, int(repeat), C.byref(ms), C.byref(nbytes), C.byref(err)), err)
        return ms.value, nbytes.value

    def kxx_build_probe(self, repeat=10):
        """moe_kxx_build_probe: (average ms per launch, algorithmic bytes per launch) of the GP's own K(X, X) assembly."""
        ms, nbytes = C.c_double(0.0), C.c_double(0.0)
        err = _lib.MoeError()
        _check(_lib.load().moe_kxx_build_probe(self._h, int(repeat), C.byref(ms), C.byref(nbytes), C.byref(err)), err)
        return ms.value, nbytes.value

    def posterior_mean(self, point, num_fidelity=0, want_grad=True):
        point, pp = _d(point)
        val = C.c_double(0.0)
        grad = np.zeros(self.d - num_fidelity)
        err = _lib.MoeError()
        _check(_lib.load().moe_posterior_mean(self._h, int(num_fidelity), pp, C.byref(val),
                                              grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
        return val.value, (grad if want_grad else None)

    # ---- acquisition functions ----
    def ei(self, Xq, Xp, num_mc, best_so_far, normals, want_grad=True, want_value=True):
        Xq, qp = _d(Xq)
        q = Xq.reshape(-1, self.d).shape[0]
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        normals, npn = _d(normals)
        if normals.size < num_mc * (q + p):
            raise InvalidValueException("normal table too small", normals.size, num_mc * (q + p), 0)
        ei = C.c_double(0.0)
        grad = np.zeros(q * self.d)
        err = _lib.MoeError()
        _check(_lib.load().moe_ei(self._h, qp, ppp, q, p, int(num_mc), float(best_so_far), npn,
                                  C.byref(ei) if want_value else None, grad.ctypes.data_as(dp) if want_grad else None,
                                  C.byref(err)), err)
        return (ei.value if want_value else None), (grad.reshape(q, self.d) if want_grad else None)

    def ei_batch(self, Xq_all, Xp, num_mc, best_so_far, normals, want_grad=True):
        """moe_ei_batch: Xq_all [E][q][dim] -> (ei [E], grad [E][q][dim] or None)."""
        Xq_all = np.ascontiguousarray(Xq_all, dtype=np.float64)
        E, q, _ = Xq_all.shape
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        normals, npn = _d(normals)
        if normals.size < num_mc * (q + p):
            raise InvalidValueException("normal table too small", normals.size, num_mc * (q + p), 0)
        ei = np.zeros(E)
        grad = np.zeros(E * q * self.d)
        err = _lib.MoeError()
        _check(_lib.load().moe_ei_batch(self._h, Xq_all.ctypes.data_as(dp), E, ppp, q, p, int(num_mc), float(best_so_far), npn,
                                        ei.ctypes.data_as(dp), grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)),
               err)
        return ei, (grad.reshape(E, q, self.d) if want_grad else None)

    def ei_analytic_batch(self, points, best_so_far, want_grad=True):
        """moe_ei_analytic_batch: points [E][dim] -> (ei [E], grad [E][dim] or None)."""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.d)
        E = points.shape[0]
        ei = np.zeros(E)
        grad = np.zeros((E, self.d))
        err = _lib.MoeError()
        _check(_lib.load().moe_ei_analytic_batch(self._h, points.ctypes.data_as(dp), E, float(best_so_far),
                                                 ei.ctypes.data_as(dp), grad.ctypes.data_as(dp) if want_grad else None,
                                                 C.byref(err)), err)
        return ei, (grad if want_grad else None)

    def ei_multistart(self, outer_params, bounds, starts, Xp, num_mc, best_so_far, normals, gradient_ascent=True):
        """moe_ei_multistart: starts [S][q][dim] -> (best_points [q][dim], best_ei, found)."""
        go = self._gd(outer_params)
        bounds, bp = _d(bounds)
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        S, q, _ = starts.shape
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        npn = None
        if normals is not None:
            normals, npn = _d(normals)
            if normals.size < num_mc * (q + p):
                raise InvalidValueException("normal table too small", normals.size, num_mc * (q + p), 0)
        best = np.zeros(q * self.d)
        best_ei = C.c_double(0.0)
        found = C.c_int(0)
        err = _lib.MoeError()
        _check(_lib.load().moe_ei_multistart(self._h, C.byref(go), bp, starts.ctypes.data_as(dp), S, ppp, q, p, int(num_mc),
                                             float(best_so_far), npn, 1 if gradient_ascent else 0, best.ctypes.data_as(dp),
                                             C.byref(best_ei), C.byref(found), C.byref(err)), err)
        return best.reshape(q, self.d), best_ei.value, bool(found.value)

    @staticmethod
    def _gd(params):
        if isinstance(params, _lib.GdParams):
            return params
        g = _lib.GdParams()
        (g.num_multistarts, g.max_num_steps, g.max_num_restarts, g.num_steps_averaged) = [int(v) for v in params[:4]]
        (g.gamma, g.pre_mult, g.max_relative_change, g.tolerance) = [float(v) for v in params[4:8]]
        g.domain_type = int(params[8]) if len(params) > 8 else 0   # (outer optimisers: 1 = simplex intersection, moe_hip.h)
        return g

    def kg(self, inner_params, bounds, discrete, Xq, Xp, num_mc, best_so_far, normals, want_grad=True, num_fidelity=0,
           first_sample=0, num_local=None, want_best_points=False):
        """One KG evaluation (or an even-aligned MC shard of it).  Returns dict(kg_sum, grad_sum, kg, grad, stats, ...);
        `kg`/`grad` are the normalised values assuming this call covered all num_mc samples."""
        L = _lib.load()
        gd = self._gd(inner_params)
        bounds, bp = _d(bounds)
        discrete, dpp = _d(discrete)
        if not 0 <= num_fidelity < self.d:
            raise BoundsException("num_fidelity out of range", num_fidelity, 0, self.d - 1)
        P = discrete.reshape(-1, self.d - num_fidelity).shape[0]
        Xq, qp = _d(Xq)
        q = Xq.reshape(-1, self.d).shape[0]
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        m = (q + p) * (1 + self.g)
        normals, npn = _d(normals)
        if normals.size < ((num_mc + 1) // 2) * m:
            raise InvalidValueException("normal table too small", normals.size, ((num_mc + 1) // 2) * m, 0)
        if num_local is None:
            num_local = num_mc - first_sample
        kg_sum = C.c_double(0.0)
        grad = np.zeros(q * self.d)
        best = np.zeros(num_local * self.d) if want_best_points else None
        stats = _lib.KgStats()
        err = _lib.MoeError()
        rc = L.moe_kg(self._h, int(num_fidelity), C.byref(gd), bp, dpp, P, qp, ppp, q, p, int(num_mc), float(best_so_far),
                      npn, int(first_sample), int(num_local), 1 if want_grad else 0, C.byref(kg_sum),
                      grad.ctypes.data_as(dp), best.ctypes.data_as(dp) if want_best_points else None, C.byref(stats),
                      C.byref(err))
        _check(rc, err)
        out = dict(kg_sum=kg_sum.value, grad_sum=grad.reshape(q, self.d) if want_grad else None,
                   kg=kg_sum.value / num_mc, grad=(grad.reshape(q, self.d) / num_mc) if want_grad else None,
                   mean_evals=stats.posterior_mean_evals, grad_evals=stats.posterior_grad_evals,
                   ms_state=stats.ms_state, ms_mc=stats.ms_mc, ms_tail=stats.ms_tail)
        if want_best_points:
            out["best_point"] = best.reshape(num_local, self.d)
        return out

    def kg_batch(self, inner_params, bounds, discrete, Xq_all, Xp, num_mc, best_so_far, normals, want_grad=True,
                 num_fidelity=0, first_sample=0, num_local=None):
        L = _lib.load()
        gd = self._gd(inner_params)
        bounds, bp = _d(bounds)
        discrete, dpp = _d(discrete)
        if not 0 <= num_fidelity < self.d:
            raise BoundsException("num_fidelity out of range", num_fidelity, 0, self.d - 1)
        P = discrete.reshape(-1, self.d - num_fidelity).shape[0]
        Xq_all = np.ascontiguousarray(Xq_all, dtype=np.float64)
        R, q, _ = Xq_all.shape
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        normals, npn = _d(normals)
        if num_local is None:
            num_local = num_mc - first_sample
        kg_sum = np.zeros(R)
        grad = np.zeros(R * q * self.d)
        stats = _lib.KgStats()
        err = _lib.MoeError()
        rc = L.moe_kg_batch(self._h, int(num_fidelity), C.byref(gd), bp, dpp, P, Xq_all.ctypes.data_as(dp), R, ppp, q, p,
                            int(num_mc), float(best_so_far), npn, int(first_sample), int(num_local),
                            1 if want_grad else 0, kg_sum.ctypes.data_as(dp), grad.ctypes.data_as(dp), C.byref(stats),
                            C.byref(err))
        _check(rc, err)
        return dict(kg_sum=kg_sum, grad_sum=grad.reshape(R, q, self.d), mean_evals=stats.posterior_mean_evals,
                    grad_evals=stats.posterior_grad_evals, ms_state=stats.ms_state, ms_mc=stats.ms_mc, ms_tail=stats.ms_tail)

    def kg_multistart(self, outer_params, inner_params, bounds, discrete, starts, Xp, num_mc, best_so_far, normals,
                      gradient_ascent=True, num_fidelity=0, comm=None):
        """moe_kg_multistart: starts [S][q][dim] -> (best_points [q][dim], best_kg, found).  comm (r5: a dist.Exchange, or None):
        moe_kg_multistart_comm -- the restarts of every batched evaluation are dealt to the ranks, one all-gather each; every rank
        returns the single-rank result bit for bit."""
        L = _lib.load()
        go, gi = self._gd(outer_params), self._gd(inner_params)
        bounds, bp = _d(bounds)
        discrete, dpp = _d(discrete)
        if not 0 <= num_fidelity < self.d:
            raise BoundsException("num_fidelity out of range", num_fidelity, 0, self.d - 1)
        P = discrete.reshape(-1, self.d - num_fidelity).shape[0]
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        S, q, _ = starts.shape
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        normals, npn = _d(normals)
        best = np.zeros(q * self.d)
        best_kg = C.c_double(0.0)
        found = C.c_int(0)
        err = _lib.MoeError()
        if comm is not None and comm.world > 1:
            rc = L.moe_kg_multistart_comm(self._h, C.byref(comm.c_struct), int(num_fidelity), C.byref(go), C.byref(gi), bp, dpp, P,
                                          starts.ctypes.data_as(dp), S, ppp, q, p, int(num_mc), float(best_so_far), npn,
                                          1 if gradient_ascent else 0, best.ctypes.data_as(dp), C.byref(best_kg), C.byref(found),
                                          C.byref(err))
            comm.reraise()  # (an exception inside the exchange callback cannot cross the C frames: it is kept and raised here)
            _check(rc, err)
        else:
            _check(L.moe_kg_multistart(self._h, int(num_fidelity), C.byref(go), C.byref(gi), bp, dpp, P, starts.ctypes.data_as(dp), S,
                                       ppp, q, p, int(num_mc), float(best_so_far), npn, 1 if gradient_ascent else 0,
                                       best.ctypes.data_as(dp), C.byref(best_kg), C.byref(found), C.byref(err)), err)
        return best.reshape(q, self.d), best_kg.value, bool(found.value)

    def posterior_mean_optimize(self, params, bounds, initial_guess, num_fidelity=0):
        g = self._gd(params)
        bounds, bp = _d(bounds)
        x0, xp = _d(initial_guess)
        out = np.zeros(self.d - num_fidelity)
        val = C.c_double(0.0)
        err = _lib.MoeError()
        _check(_lib.load().moe_posterior_mean_optimize(self._h, int(num_fidelity), C.byref(g), bp, xp, out.ctypes.data_as(dp),
                                                       C.byref(val), C.byref(err)), err)
        return out, val.value

    def last_kernel_ms(self):
        out = np.zeros(5)
        _lib.load().moe_last_kernel_ms(self._h, out.ctypes.data_as(dp))
        return dict(mc=out[0], cov_build=out[1], tail=out[2], state=out[3], total=out[4])


    def last_kernel_info(self):
        out = (C.c_int * 8)()
        _lib.load().moe_last_kernel_info(self._h, out)
        keys = ("variant", "xlds", "waves", "tr", "weight_table", "fused_tail", "blocks", "prep")
        info = dict(zip(keys, [int(v) for v in out]))
        info["far_frame"], info["wide_frame"], info["lane"] = (info["xlds"] >> 1) & 1, (info["xlds"] >> 2) & 1, (info["xlds"] >> 3) & 1
        info["start_table"] = (info["xlds"] >> 4) & 1
        info["xlds"] &= 1
        return info

    def last_kg_moves(self):
        """moe_last_kg_moves: how often a workgroup of the last KG call's MC kernel moved to another evaluation."""
        out = C.c_longlong(0)
        if _lib.load().moe_last_kg_moves(self._h, C.byref(out)):
            raise RuntimeError("moe_last_kg_moves failed")
        return int(out.value)

    def last_kg_best_points(self):
        """moe_last_kg_best_points: the inner optimisations' end points of the last KG call, [evaluations][samples][dim]."""
        L = _lib.load()
        E, M = C.c_int(0), C.c_int(0)
        if L.moe_last_kg_best_points(self._h, C.byref(E), C.byref(M), None, 0):
            raise RuntimeError("moe_last_kg_best_points failed")
        out = np.zeros((E.value, M.value, self.d))
        if out.size and L.moe_last_kg_best_points(self._h, C.byref(E), C.byref(M), out.ctypes.data_as(dp), out.size):
            raise RuntimeError("moe_last_kg_best_points failed")
        return out


def kg_batch_multi(gps, shard, inner_params, bounds, discrete, Xq_all, Xp, num_mc, best_so_far, normals, want_grad=True,
                   num_fidelity=0):
    """moe_kg_batch_multi: the same GP on several devices (`gps`: DeviceGP objects built with device = 0 .. W-1), one host
    thread per device inside the library; shard = "restarts" (evaluation e on handle e % W) or "mc" (every handle takes an
    even-aligned slice of the samples, host-side fixed-order sum).  Returns the dict kg_batch returns."""
    L = _lib.load()
    g0 = gps[0]
    gd = DeviceGP._gd(inner_params)
    bounds, bp = _d(bounds)
    discrete, dpp = _d(discrete)
    P = discrete.reshape(-1, g0.d - num_fidelity).shape[0]
    Xq_all = np.ascontiguousarray(Xq_all, dtype=np.float64)
    R, q, _ = Xq_all.shape
    if Xp is None or np.size(Xp) == 0:
        p, ppp = 0, None
    else:
        Xp, ppp = _d(Xp)
        p = Xp.reshape(-1, g0.d).shape[0]
    normals, npn = _d(normals)
    arr = (C.c_void_p * len(gps))(*[g._h.value for g in gps])
    kg = np.zeros(R)
    grad = np.zeros(R * q * g0.d)
    stats = _lib.KgStats()
    err = _lib.MoeError()
    _check(L.moe_kg_batch_multi(arr, len(gps), {"restarts": 0, "mc": 1}[shard], int(num_fidelity), C.byref(gd), bp, dpp, P,
                                Xq_all.ctypes.data_as(dp), R, ppp, q, p, int(num_mc), float(best_so_far), npn,
                                1 if want_grad else 0, kg.ctypes.data_as(dp), grad.ctypes.data_as(dp), C.byref(stats),
                                C.byref(err)), err)
    return dict(kg_sum=kg, grad_sum=grad.reshape(R, q, g0.d) if want_grad else None, mean_evals=stats.posterior_mean_evals,
                grad_evals=stats.posterior_grad_evals)


class DeviceGPMCMC(object):
    """num_mcmc device GPs over the same data, one per hyper-parameter sample (replaces C_GP.GaussianProcessMCMC,
    gpp_knowledge_gradient_mcmc_optimization.cpp:24-49: Matern-5/2, hypers [num_mcmc][1 + dim] = (alpha, lengths),
    noises [num_mcmc][1 + num_derivatives]).  `members` restricts construction to a subset of the GP indices (the GP-index
    shard of a multi-GPU run); the MCMC-averaged evaluators below then return that subset's share."""

    def __init__(self, hypers, noises, X, y, derivatives=(), device=0, members=None):
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.n, self.d = X.shape
        self.derivatives = [int(v) for v in derivatives]
        self.g = len(self.derivatives)
        hypers = np.ascontiguousarray(hypers, dtype=np.float64).reshape(-1, self.d + 1)
        noises = np.ascontiguousarray(noises, dtype=np.float64).reshape(-1, 1 + self.g)
        self.total_num_mcmc = hypers.shape[0]
        self.members = list(range(self.total_num_mcmc)) if members is None else [int(i) for i in members]
        self.gps = [DeviceGP(hypers[i], X, y, noises[i], self.derivatives, cov_type=_lib.COV_MATERN_NU_2P5, device=device)
                    for i in self.members]
        self._arr = (C.c_void_p * max(len(self.gps), 1))(*[gp._h.value for gp in self.gps])

    num_mcmc = property(lambda self: len(self.gps))

    def _common(self, Xq_all, Xp):
        Xq_all = np.ascontiguousarray(Xq_all, dtype=np.float64)
        E, q, _ = Xq_all.shape
        if Xp is None or np.size(Xp) == 0:
            p, ppp = 0, None
        else:
            Xp, ppp = _d(Xp)
            p = Xp.reshape(-1, self.d).shape[0]
        return Xq_all, E, q, Xp, p, ppp

    def _local(self, per_gp):
        """Rows of a per-GP array [total_num_mcmc][...] that belong to this object's members."""
        a = np.asarray(per_gp, dtype=np.float64).reshape(self.total_num_mcmc, -1)
        return np.ascontiguousarray(a[self.members])

    def kg_batch(self, inner_params, bounds, discrete_all, Xq_all, Xp, num_mc, best_so_far, normals, want_grad=True,
                 num_fidelity=0, finalize=True):
        """moe_kg_mcmc_batch: Xq_all [E][q][dim], discrete_all [total_num_mcmc][P][dim - f], best_so_far [total_num_mcmc]
        -> (kg [E], grad [E][q][dim] or None).  finalize=False returns this object's members' plain sums."""
        Xq_all, E, q, Xp, p, ppp = self._common(Xq_all, Xp)
        g = DeviceGP._gd(inner_params)
        bounds, bp = _d(bounds)
        disc = self._local(discrete_all)
        if not 0 <= num_fidelity < self.d:
            raise BoundsException("num_fidelity out of range", num_fidelity, 0, self.d - 1)
        P = disc.shape[1] // (self.d - num_fidelity)
        best = self._local(best_so_far).ravel()
        normals, npn = _d(normals)
        m = (q + p) * (1 + self.g)
        if normals.size < ((num_mc + 1) // 2) * m:
            raise InvalidValueException("normal table too small", normals.size, ((num_mc + 1) // 2) * m, 0)
        kg = np.zeros(E)
        grad = np.zeros((E, q, self.d))
        err = _lib.MoeError()
        _check(_lib.load().moe_kg_mcmc_batch(self._arr, len(self.gps), int(num_fidelity), C.byref(g), bp, disc.ctypes.data_as(dp),
                                             P, Xq_all.ctypes.data_as(dp), E, ppp, q, p, int(num_mc), best.ctypes.data_as(dp),
                                             npn, 1 if finalize else 0, self.total_num_mcmc, kg.ctypes.data_as(dp),
                                             grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
        return kg, (grad if want_grad else None)

    def kg_finalize(self, kg_sum, grad_sum, Xq_all, num_fidelity=0):
        """moe_kg_mcmc_finalize on all-reduced sums: mean over total_num_mcmc, fidelity cost and its gradient term."""
        Xq_all = np.ascontiguousarray(Xq_all, dtype=np.float64)
        E, q, _ = Xq_all.shape
        kg = np.array(kg_sum, dtype=np.float64, copy=True).reshape(E)
        grad = None if grad_sum is None else np.array(grad_sum, dtype=np.float64, copy=True).reshape(E, q, self.d)
        rc = _lib.load().moe_kg_mcmc_finalize(kg.ctypes.data_as(dp), grad.ctypes.data_as(dp) if grad is not None else None,
                                              Xq_all.ctypes.data_as(dp), E, q, self.d, int(num_fidelity), self.total_num_mcmc)
        if rc:
            raise BoundsException("moe_kg_mcmc_finalize: bad argument", rc, 0, 0)
        return kg, grad

    def ei_batch(self, Xq_all, Xp, num_mc, best_so_far, normals, want_grad=True, analytic=False):
        """moe_ei_mcmc_batch: (ei [E], grad [E][q][dim] or None), averaged over this object's members."""
        Xq_all, E, q, Xp, p, ppp = self._common(Xq_all, Xp)
        best = self._local(best_so_far).ravel()
        npn = None
        if not analytic:
            normals, npn = _d(normals)
            if normals.size < num_mc * (q + p):
                raise InvalidValueException("normal table too small", normals.size, num_mc * (q + p), 0)
        ei = np.zeros(E)
        grad = np.zeros((E, q, self.d))
        err = _lib.MoeError()
        _check(_lib.load().moe_ei_mcmc_batch(self._arr, len(self.gps), Xq_all.ctypes.data_as(dp), E, ppp, q, p, int(num_mc),
                                             best.ctypes.data_as(dp), npn, 1 if analytic else 0, ei.ctypes.data_as(dp),
                                             grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
        return ei, (grad if want_grad else None)

    def kg_multistart(self, outer_params, inner_params, bounds, discrete_all, starts, Xp, num_mc, best_so_far, normals,
                      gradient_ascent=True, num_fidelity=0, comm=None):
        """moe_kg_mcmc_multistart: starts [S][q][dim] -> (best_points [q][dim], best_kg, found).  comm (r5: a dist.Exchange):
        moe_kg_mcmc_multistart_comm -- this object holds members rank, rank + world, ... (DeviceGPMCMC(members=dist.shard_members(...)));
        discrete_all / best_so_far are the WHOLE ensemble's, the local rows are picked here; the per-member values of every batched
        evaluation are exchanged and added in global member order: the single-rank result bit for bit."""
        starts, S, q, Xp, p, ppp = self._common(starts, Xp)
        go, gi = DeviceGP._gd(outer_params), DeviceGP._gd(inner_params)
        bounds, bp = _d(bounds)
        disc = self._local(discrete_all)
        if not 0 <= num_fidelity < self.d:
            raise BoundsException("num_fidelity out of range", num_fidelity, 0, self.d - 1)
        P = disc.shape[1] // (self.d - num_fidelity)
        best = self._local(best_so_far).ravel()
        normals, npn = _d(normals)
        out = np.zeros(q * self.d)
        val = C.c_double(0.0)
        found = C.c_int(0)
        err = _lib.MoeError()
        if comm is not None and comm.world > 1:
            if self.members != list(range(comm.rank, self.total_num_mcmc, comm.world)):
                raise InvalidValueException("member-sharded optimisation: this rank must hold members rank, rank + world, ...",
                                            len(self.members), 0, 0)
            rc = _lib.load().moe_kg_mcmc_multistart_comm(self._arr, len(self.gps), self.total_num_mcmc, C.byref(comm.c_struct),
                                                         int(num_fidelity), C.byref(go), C.byref(gi), bp, disc.ctypes.data_as(dp), P,
                                                         starts.ctypes.data_as(dp), S, ppp, q, p, int(num_mc),
                                                         best.ctypes.data_as(dp), npn, 1 if gradient_ascent else 0,
                                                         out.ctypes.data_as(dp), C.byref(val), C.byref(found), C.byref(err))
            comm.reraise()
            _check(rc, err)
            return out.reshape(q, self.d), val.value, bool(found.value)
        _check(_lib.load().moe_kg_mcmc_multistart(self._arr, len(self.gps), int(num_fidelity), C.byref(go), C.byref(gi), bp,
                                                  disc.ctypes.data_as(dp), P, starts.ctypes.data_as(dp), S, ppp, q, p, int(num_mc),
                                                  best.ctypes.data_as(dp), npn, 1 if gradient_ascent else 0,
                                                  out.ctypes.data_as(dp), C.byref(val), C.byref(found), C.byref(err)), err)
        return out.reshape(q, self.d), val.value, bool(found.value)

    def ei_multistart(self, outer_params, bounds, starts, Xp, num_mc, best_so_far, normals, gradient_ascent=True):
        """moe_ei_mcmc_multistart: starts [S][q][dim] -> (best_points [q][dim], best_ei, found)."""
        starts, S, q, Xp, p, ppp = self._common(starts, Xp)
        go = DeviceGP._gd(outer_params)
        bounds, bp = _d(bounds)
        best = self._local(best_so_far).ravel()
        npn = None
        if normals is not None:
            normals, npn = _d(normals)
        out = np.zeros(q * self.d)
        val = C.c_double(0.0)
        found = C.c_int(0)
        err = _lib.MoeError()
        _check(_lib.load().moe_ei_mcmc_multistart(self._arr, len(self.gps), C.byref(go), bp, starts.ctypes.data_as(dp), S, ppp, q, p,
                                                  int(num_mc), best.ctypes.data_as(dp), npn, 1 if gradient_ascent else 0,
                                                  out.ctypes.data_as(dp), C.byref(val), C.byref(found), C.byref(err)), err)
        return out.reshape(q, self.d), val.value, bool(found.value)


def _ensemble_handles(gps):
    """(ctypes array of handles, count, dim) of an MCMC ensemble: a DeviceGPMCMC or a sequence of DeviceGP over the same data."""
    members = list(gps.gps) if isinstance(gps, DeviceGPMCMC) else list(gps)
    arr = (C.c_void_p * max(len(members), 1))(*[g._h.value for g in members])
    return arr, len(members), (members[0].d if members else 0), members


def posterior_mean_mcmc(gps, points, num_fidelity=0, want_grad=False):
    """moe_posterior_mean_mcmc_batch: f = -(mean over the members of the posterior mean), fidelity coordinates pinned to 1, at
    points [P][dim - num_fidelity] in one device call.  Returns value [P], with want_grad (value, grad [P][dim - num_fidelity])."""
    arr, E, d, keep = _ensemble_handles(gps)
    size = d - int(num_fidelity)
    if E > 0 and not 0 < size <= d:
        raise BoundsException("num_fidelity out of range", num_fidelity, 0, d - 1)
    points, pp = _d(points)
    P = points.reshape(-1, max(size, 1)).shape[0]
    value = np.zeros(P)
    grad = np.zeros((P, max(size, 1))) if want_grad else None
    err = _lib.MoeError()
    _check(_lib.load().moe_posterior_mean_mcmc_batch(arr, E, int(num_fidelity), pp, P, value.ctypes.data_as(dp),
                                                     grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
    return (value, grad) if want_grad else value


def kg_discrete_mcmc(gps, discrete_all, points, best_so_far_all, num_fidelity=0, want_grad=True):
    """The ensemble average of DeviceGP.kg_discrete, every member with its own discrete set discrete_all[e] [A_e][dim - num_fidelity]
    and best value best_so_far_all[e], as KG-MCMC averages its members: the members' results are added in member order and divided
    by their number.  Returns kg [C], with want_grad (kg, grad [C][dim])."""
    members = list(gps.gps) if isinstance(gps, DeviceGPMCMC) else list(gps)
    if not members or len(discrete_all) != len(members) or len(best_so_far_all) != len(members):
        raise BoundsException("one discrete set and one best value per ensemble member", len(discrete_all), len(members), len(members))
    kg = grad = None
    for g, disc, best in zip(members, discrete_all, best_so_far_all):
        res = g.kg_discrete(disc, points, best, num_fidelity=num_fidelity, want_grad=want_grad)
        k, gr = res if want_grad else (res, None)
        kg = k if kg is None else kg + k
        if want_grad:
            grad = gr if grad is None else grad + gr
    kg = kg / len(members)
    return (kg, grad / len(members)) if want_grad else kg


def _num_pending(points_being_sampled, d):
    """the number of pending points [p][dim] (0 for None or an empty array)"""
    if points_being_sampled is None:
        return 0
    return int(np.asarray(points_being_sampled, dtype=np.float64).size // max(int(d), 1))


def _kg_discrete_members(gps, discrete_all, best_so_far_all, num_fidelity):
    """(handles, count, dim, members kept alive, sets back to back, their sizes, best values) of the ensemble forms of kg_discrete;
    a single DeviceGP counts as a list of one"""
    if isinstance(gps, DeviceGP):
        gps = [gps]
    arr, E, d, keep = _ensemble_handles(gps)
    if E == 0 or len(discrete_all) != E or len(best_so_far_all) != E:
        raise BoundsException("one discrete set and one best value per ensemble member", len(discrete_all), E, E)
    size = d - int(num_fidelity)
    if not 0 < size <= d:
        size = d  # (the library refuses num_fidelity; the shapes only have to be readable)
    sets = [np.ascontiguousarray(s, dtype=np.float64).reshape(-1, size) for s in discrete_all]
    disc = np.ascontiguousarray(np.vstack(sets))
    counts = np.ascontiguousarray([s.shape[0] for s in sets], dtype=np.int32)
    best = np.ascontiguousarray(best_so_far_all, dtype=np.float64).ravel()
    return arr, E, d, keep, disc, counts, best


def _acq1_pending(points_being_sampled, d):
    """(array kept alive, ctypes pointer or None, p) of the pending points [p][dim] of an ensemble one-point acquisition"""
    p = _num_pending(points_being_sampled, d)
    pend, pendp = _d(points_being_sampled) if p else (None, None)
    return pend, pendp, p


def _acq1_evaluate(fn, pre, post, d, points, want_grad, points_being_sampled, extra_shape=None, want_extra=False, fn_without=None):
    """The evaluate-at-points shape of the ensemble one-point acquisitions: fn(*pre, *post, pending, p, points, C, want_grad, value,
    grad[, extra], err).  pre / post: the objective's own arguments, those before and behind (gd_params, bounds) in the other two
    shapes.  extra_shape: the symbol has a trailing per-member output of that shape with [C] appended, filled with want_extra and
    NULL without.  fn_without: the symbol without the pending arguments, called when there are no pending points.  Returns value
    [C], with want_grad (value, grad [C][dim]), with want_extra the extra output last."""
    pts, pp = _d(points)
    C_ = pts.reshape(-1, d).shape[0]
    value = np.zeros(max(C_, 1))
    grad = np.zeros((max(C_, 1), d)) if want_grad else None
    extra = np.zeros(tuple(extra_shape) + (max(C_, 1),)) if want_extra else None
    pend, pendp, p = _acq1_pending(points_being_sampled, d)
    err = _lib.MoeError()
    if fn_without is not None and not p:
        fn, pending = fn_without, ()
    else:
        pending = (pendp, p)
    args = tuple(pre) + tuple(post) + pending + (pp, C_, 1 if want_grad else 0, value.ctypes.data_as(dp),
                                                 grad.ctypes.data_as(dp) if want_grad else None)
    if extra_shape is not None:
        args += (extra.ctypes.data_as(dp) if want_extra else None,)
    _check(fn(*(args + (C.byref(err),))), err)
    out = (value, grad) if want_grad else (value,)
    if extra is not None:
        out = out + (extra,)
    return out if len(out) > 1 else out[0]


def _acq1_multistart(fn, pre, post, d, gd_params, bounds, starts, gradient_ascent, want_path, points_being_sampled, fn_without=None):
    """The multistart shape: fn(*pre, gd_params, bounds, *post, pending, p, starts, S, gradient_ascent, the nine outputs, err);
    fn_without as in _acq1_evaluate.  Returns the dict of kg_discrete_multistart."""
    g = DeviceGP._gd(gd_params)
    bounds, bp = _d(bounds)
    starts, sp = _d(starts)
    S = starts.reshape(-1, d).shape[0]
    K = max(min(S, 20), 1)
    rows = max(g.max_num_restarts, 0) * max(g.max_num_steps, 0) + 1
    point = np.zeros(d)
    start_values = np.zeros(max(S, 1))
    kept = np.zeros(K, dtype=np.int32)
    ends, end_values = np.zeros((K, d)), np.zeros(K)
    steps = np.zeros(K, dtype=np.int32)
    path = np.zeros((K, rows, d)) if (want_path and gradient_ascent) else None
    value, found = C.c_double(0.0), C.c_int(0)
    pend, pendp, p = _acq1_pending(points_being_sampled, d)
    err = _lib.MoeError()
    if fn_without is not None and not p:
        fn, pending = fn_without, ()
    else:
        pending = (pendp, p)
    _check(fn(*(tuple(pre) + (C.byref(g), bp) + tuple(post) + pending + (
        sp, S, 1 if gradient_ascent else 0, point.ctypes.data_as(dp), C.byref(value), C.byref(found), start_values.ctypes.data_as(dp),
        kept.ctypes.data_as(ip), ends.ctypes.data_as(dp), end_values.ctypes.data_as(dp),
        path.ctypes.data_as(dp) if path is not None else None, steps.ctypes.data_as(ip), C.byref(err)))), err)
    out = {"point": point, "value": value.value, "found": bool(found.value), "start_values": start_values,
           "kept_index": kept if gradient_ascent else None, "end_points": ends if gradient_ascent else None,
           "end_values": end_values if gradient_ascent else None, "steps_taken": steps if gradient_ascent else None}
    if want_path:
        out["path"] = path
    return out


def _acq1_suggest(fn, pre, post, d, gd_params, bounds, starts, num_to_sample, gradient_ascent, points_being_sampled):
    """The greedy-batch shape: fn(*pre, gd_params, bounds, *post, pending, p, starts, S, gradient_ascent, q, points, values, found,
    err).  Returns a dict: points [q][dim], values [q], found [q]."""
    g = DeviceGP._gd(gd_params)
    bounds, bp = _d(bounds)
    starts, sp = _d(starts)
    S = starts.reshape(-1, d).shape[0]
    q = int(num_to_sample)
    pend, pendp, p = _acq1_pending(points_being_sampled, d)
    points, values = np.zeros((max(q, 1), d)), np.zeros(max(q, 1))
    found = np.zeros(max(q, 1), dtype=np.int32)
    err = _lib.MoeError()
    _check(fn(*(tuple(pre) + (C.byref(g), bp) + tuple(post) + (
        pendp, p, sp, S, 1 if gradient_ascent else 0, q, points.ctypes.data_as(dp), values.ctypes.data_as(dp), found.ctypes.data_as(ip),
        C.byref(err)))), err)
    return {"points": points, "values": values, "found": found.astype(bool)}


def kg_discrete_ensemble(gps, discrete_all, points, best_so_far_all, num_fidelity=0, want_grad=True, points_being_sampled=None):
    """moe_kg_discrete_mcmc: what kg_discrete_mcmc returns, bit for bit, in one device call for the whole ensemble (one upload, one
    stream, one wait; every kernel launched once for all members where their launches line up).  gps: a DeviceGPMCMC, a list of
    DeviceGP (they need not share their sampled points) or one DeviceGP.  Returns kg [C], with want_grad (kg, grad [C][dim]).
    SingularMatrixException(e, i): member e, candidate i.
    points_being_sampled [p][dim] (None or empty: the symbol and bits of before): moe_kg_discrete_mcmc_pending -- every member's
    posterior covariance conditioned on the pending points, its mean left alone; SingularMatrixException(e, j) for pending point j."""
    arr, E, d, keep, disc, counts, best = _kg_discrete_members(gps, discrete_all, best_so_far_all, num_fidelity)
    pre, post = (arr, E, int(num_fidelity)), (disc.ctypes.data_as(dp), counts.ctypes.data_as(ip), best.ctypes.data_as(dp))
    lib = _lib.load()
    return _acq1_evaluate(lib.moe_kg_discrete_mcmc_pending, pre, post, d, points, want_grad, points_being_sampled,
                          fn_without=lib.moe_kg_discrete_mcmc)


def kg_discrete_multistart(gps, gd_params, bounds, discrete_all, best_so_far_all, starts, num_fidelity=0, gradient_ascent=True,
                           want_path=False, points_being_sampled=None):
    """moe_kg_discrete_mcmc_multistart: one suggestion by the ensemble-averaged discretised knowledge gradient -- the value at
    every start [S][dim], the 20 best kept, restarted gradient ascent on all of them on the device, the value at every end point,
    the best one returned.  Returns a dict: point [dim], value, found, start_values [S], and with gradient_ascent kept_index [K],
    end_points [K][dim], end_values [K], steps_taken [K] (None without), with want_path path [K][restarts steps + 1][dim].
    points_being_sampled [p][dim] (None or empty: the symbol and bits of before): moe_kg_discrete_mcmc_multistart_pending, the same
    ascent on the knowledge gradient conditioned on the pending points."""
    arr, E, d, keep, disc, counts, best = _kg_discrete_members(gps, discrete_all, best_so_far_all, num_fidelity)
    pre, post = (arr, E, int(num_fidelity)), (disc.ctypes.data_as(dp), counts.ctypes.data_as(ip), best.ctypes.data_as(dp))
    lib = _lib.load()
    return _acq1_multistart(lib.moe_kg_discrete_mcmc_multistart_pending, pre, post, d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled, fn_without=lib.moe_kg_discrete_mcmc_multistart)


def kg_discrete_suggest(gps, gd_params, bounds, discrete_all, best_so_far_all, starts, num_to_sample, num_fidelity=0,
                        gradient_ascent=True, points_being_sampled=None):
    """moe_kg_discrete_mcmc_suggest: num_to_sample points greedily by the ensemble-averaged discretised knowledge gradient -- round t
    is kg_discrete_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None)
    followed by the points of the rounds before, bit for bit, in one device call: the set phase runs once and a round appends one
    row to every member's extension.  p + num_to_sample - 1 <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    arr, E, d, keep, disc, counts, best = _kg_discrete_members(gps, discrete_all, best_so_far_all, num_fidelity)
    pre, post = (arr, E, int(num_fidelity)), (disc.ctypes.data_as(dp), counts.ctypes.data_as(ip), best.ctypes.data_as(dp))
    return _acq1_suggest(_lib.load().moe_kg_discrete_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _ei_analytic_members(gps, best_so_far):
    """(handles, count, dim, members kept alive, best values [E]) of the ensemble forms of the analytic expected improvement; a single
    DeviceGP counts as a list of one"""
    if isinstance(gps, DeviceGP):
        gps = [gps]
    arr, E, d, keep = _ensemble_handles(gps)
    best = np.ascontiguousarray(best_so_far, dtype=np.float64).ravel()
    if E == 0 or best.size != E:
        raise BoundsException("one best value per ensemble member", best.size, E, E)
    return arr, E, d, keep, best


def ei_analytic_ensemble(gps, points, best_so_far, points_being_sampled=None, want_grad=True):
    """moe_ei_analytic_mcmc: the analytic one-point expected improvement averaged over the ensemble at points [C][dim], in one device
    call (one upload, one stream, one wait), member e against best_so_far[e].  points_being_sampled [p][dim] (None or empty: none):
    every member's posterior covariance is conditioned on the pending points, its mean left alone, and the believed values join the
    member's best value.  gps: a DeviceGPMCMC, a list of DeviceGP or one DeviceGP.  The members may observe derivatives (one list
    for all of them, InvalidValueException otherwise): a pending point is then believed to return its value and those g derivatives,
    1 + g rows with noise_variance[a] on row a, and p (1 + g) <= 64 (BoundsException(p, 0, 64 // (1 + g))).  Returns ei [C], with
    want_grad (ei, grad [C][dim]).  SingularMatrixException(e, j): member e, pending point j; a candidate never raises."""
    arr, E, d, keep, best = _ei_analytic_members(gps, best_so_far)
    pre, post = (arr, E), (best.ctypes.data_as(dp),)
    return _acq1_evaluate(_lib.load().moe_ei_analytic_mcmc, pre, post, d, points, want_grad, points_being_sampled)


def ei_analytic_multistart(gps, gd_params, bounds, best_so_far, starts, gradient_ascent=True, want_path=False,
                           points_being_sampled=None):
    """moe_ei_analytic_mcmc_multistart: one suggestion by the ensemble-averaged analytic expected improvement -- the value at every
    start [S][dim], the 20 best kept, restarted gradient ascent on all of them on the device, the value at every end point, the best
    one returned.  The dict of kg_discrete_multistart: point [dim], value, found, start_values [S], and with gradient_ascent
    kept_index [K], end_points [K][dim], end_values [K], steps_taken [K] (None without), with want_path path [K][restarts steps +
    1][dim].  Members with derivative observations as in ei_analytic_ensemble."""
    arr, E, d, keep, best = _ei_analytic_members(gps, best_so_far)
    pre, post = (arr, E), (best.ctypes.data_as(dp),)
    return _acq1_multistart(_lib.load().moe_ei_analytic_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent, want_path,
                            points_being_sampled)


def ei_analytic_suggest(gps, gd_params, bounds, best_so_far, starts, num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_ei_analytic_mcmc_suggest: num_to_sample points greedily by the ensemble-averaged analytic expected improvement -- round t
    is ei_analytic_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None)
    followed by the points of the rounds before, bit for bit, in one device call.  p + num_to_sample - 1 <= 64; with g observed
    derivatives per point (p + num_to_sample - 1) (1 + g) <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    arr, E, d, keep, best = _ei_analytic_members(gps, best_so_far)
    pre, post = (arr, E), (best.ctypes.data_as(dp),)
    return _acq1_suggest(_lib.load().moe_ei_analytic_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample, gradient_ascent,
                         points_being_sampled)


def _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far):
    """(objective handles, E, dim, GPs kept alive, constraint handles [K][E] flat or None, K, thresholds [K], best values [E]) of the
    ensemble forms of the constrained expected improvement.  constraint_gps: K ensembles, each shaped like gps (a DeviceGPMCMC, a
    list of DeviceGP or one DeviceGP), E members each; best values may be +inf."""
    arr, E, d, keep, best = _ei_analytic_members(gps, best_so_far)
    cons = [] if constraint_gps is None else list(constraint_gps)
    K = len(cons)
    tau = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    if tau.size != K:
        raise BoundsException("one threshold per constraint", tau.size, K, K)
    flat = []
    for c in cons:
        members = [c] if isinstance(c, DeviceGP) else (list(c.gps) if isinstance(c, DeviceGPMCMC) else list(c))
        if len(members) != E:
            raise BoundsException("one constraint GP per ensemble member and constraint", len(members), E, E)
        flat.extend(members)
    carr = (C.c_void_p * max(len(flat), 1))(*[g._h.value for g in flat]) if K else None
    return arr, E, d, (keep, flat), carr, K, tau, best


def ei_constrained_ensemble(gps, constraint_gps, thresholds, points, best_so_far, points_being_sampled=None, want_grad=True,
                            want_factors=False):
    """moe_ei_constrained_mcmc: expected improvement times the probability of feasibility, averaged over the ensemble at points
    [C][dim], in one device call.  Member e is the objective GP gps[e] and the constraint GPs constraint_gps[k][e], constraint k
    satisfied where c_k(x) <= thresholds[k] (0 <= K <= 8; K = 0 with finite best values is ei_analytic_ensemble bit for bit).
    best_so_far [E] is the best FEASIBLE value per member and may be +inf (no feasible observation yet: the member's acquisition is
    its probability of feasibility).  points_being_sampled [p][dim] condition every GP's covariance; a pending point joins member
    e's incumbent where the member believes it feasible.  Returns value [C], with want_grad (value, grad [C][dim]), and with
    want_factors additionally factors [E][1 + K][C] (the improvement factor, then the K feasibility factors) as the last item.
    SingularMatrixException(e (1 + K) + role, j): the GP, counted flat, and the pending point; a candidate never raises."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None), (best.ctypes.data_as(dp),)
    return _acq1_evaluate(_lib.load().moe_ei_constrained_mcmc, pre, post, d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 1 + K), want_extra=want_factors)


def ei_constrained_multistart(gps, constraint_gps, thresholds, gd_params, bounds, best_so_far, starts, gradient_ascent=True,
                              want_path=False, points_being_sampled=None):
    """moe_ei_constrained_mcmc_multistart: one suggestion by the ensemble-averaged constrained expected improvement --
    ei_analytic_multistart's screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None), (best.ctypes.data_as(dp),)
    return _acq1_multistart(_lib.load().moe_ei_constrained_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent, want_path,
                            points_being_sampled)


def ei_constrained_suggest(gps, constraint_gps, thresholds, gd_params, bounds, best_so_far, starts, num_to_sample,
                           gradient_ascent=True, points_being_sampled=None):
    """moe_ei_constrained_mcmc_suggest: num_to_sample points greedily by the ensemble-averaged constrained expected improvement --
    round t is ei_constrained_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be
    None) followed by the points of the rounds before, bit for bit, in one device call.  (p + num_to_sample - 1) (1 + g) <= 64.
    Returns a dict: points [q][dim], values [q], found [q]."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None), (best.ctypes.data_as(dp),)
    return _acq1_suggest(_lib.load().moe_ei_constrained_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample, gradient_ascent,
                         points_being_sampled)


def log_ei_constrained_ensemble(gps, constraint_gps, thresholds, points, best_so_far, points_being_sampled=None, want_grad=True,
                                want_log_factors=False):
    """moe_log_ei_constrained_mcmc: the LOG of what ei_constrained_ensemble returns, computed so that it stays finite with a useful
    gradient where that value and its gradient are exactly 0 in float64 (an incumbent dozens of posterior standard deviations below
    the mean, a constraint far from feasible).  Arguments as there; constraint_gps=None / thresholds=None is K = 0, the log of the
    ensemble-averaged analytic expected improvement.  Returns value [C], with want_grad (value, grad [C][dim]), and with
    want_log_factors additionally log_factors [E][1 + K][C] (the log improvement factor, then the K log feasibility factors) as
    the last item; the value is the log-mean-exp over e of the members' sums.  SingularMatrixException as there."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None), (best.ctypes.data_as(dp),)
    return _acq1_evaluate(_lib.load().moe_log_ei_constrained_mcmc, pre, post, d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 1 + K), want_extra=want_log_factors)


def log_ei_constrained_multistart(gps, constraint_gps, thresholds, gd_params, bounds, best_so_far, starts, gradient_ascent=True,
                                  want_path=False, points_being_sampled=None):
    """moe_log_ei_constrained_mcmc_multistart: one suggestion by the log of the ensemble-averaged constrained expected improvement
    -- ei_constrained_multistart's screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict,
    on an objective whose screening values do not tie at 0 and whose gradient does not vanish."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None), (best.ctypes.data_as(dp),)
    return _acq1_multistart(_lib.load().moe_log_ei_constrained_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled)


def log_ei_constrained_suggest(gps, constraint_gps, thresholds, gd_params, bounds, best_so_far, starts, num_to_sample,
                               gradient_ascent=True, points_being_sampled=None):
    """moe_log_ei_constrained_mcmc_suggest: num_to_sample points greedily by the log of the ensemble-averaged constrained expected
    improvement -- round t is log_ei_constrained_multistart from the same starts [S][dim] with the pending points
    points_being_sampled [p][dim] (may be None) followed by the points of the rounds before, bit for bit, in one device call.
    (p + num_to_sample - 1) (1 + g) <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None), (best.ctypes.data_as(dp),)
    return _acq1_suggest(_lib.load().moe_log_ei_constrained_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _ei_per_cost_members(gps, constraint_gps, thresholds, cost_gps, cost_exponent, best_so_far):
    """_ei_constrained_members' tuple with (cost handles [E], the exponent as a C double) behind the thresholds, of the ensemble
    forms of the log expected improvement per unit cost.  cost_gps: an ensemble shaped like gps (a DeviceGPMCMC, a list of DeviceGP or
    one DeviceGP) of GPs of the LOG of the evaluation cost, E members; cost_exponent finite and >= 0."""
    arr, E, d, keep, carr, K, tau, best = _ei_constrained_members(gps, constraint_gps, thresholds, best_so_far)
    if cost_gps is None:
        raise BoundsException("one cost GP per ensemble member", 0, E, E)
    costs = [cost_gps] if isinstance(cost_gps, DeviceGP) else (list(cost_gps.gps) if isinstance(cost_gps, DeviceGPMCMC) else list(cost_gps))
    if len(costs) != E:
        raise BoundsException("one cost GP per ensemble member", len(costs), E, E)
    alpha = float(cost_exponent)
    if not np.isfinite(alpha) or alpha < 0.0:
        raise InvalidValueException("cost_exponent must be finite and not negative", alpha, 0.0, 0.0)
    costarr = (C.c_void_p * E)(*[g._h.value for g in costs])
    return arr, E, d, (keep, costs), carr, K, tau, costarr, C.c_double(alpha), best


def _ei_per_cost_args(gps, constraint_gps, thresholds, cost_gps, cost_exponent, best_so_far):
    """(pre, post, E, K, dim, what must stay alive) of the three shapes below"""
    arr, E, d, keep, carr, K, tau, costarr, alpha, best = _ei_per_cost_members(gps, constraint_gps, thresholds, cost_gps, cost_exponent,
                                                                               best_so_far)
    pre, post = (arr, E, carr, K, tau.ctypes.data_as(dp) if K else None, costarr, alpha), (best.ctypes.data_as(dp),)
    return pre, post, E, K, d, (keep, tau, best)


def log_ei_per_cost_ensemble(gps, constraint_gps, thresholds, cost_gps, cost_exponent, points, best_so_far, points_being_sampled=None,
                             want_grad=True, want_log_factors=False):
    """moe_log_ei_per_cost_mcmc: the log of the constrained expected improvement per unit cost, log_ei_constrained_ensemble's member
    log plus -cost_exponent (mu_c + var_c / 2) from cost_gps[e], a GP of the LOG of the evaluation cost (the log of
    E[cost]^-cost_exponent under a log-normal cost).  The other arguments as there; every GP's covariance, the cost GP's too, is
    conditioned on points_being_sampled.  Returns value [C], with want_grad (value, grad [C][dim]), and with want_log_factors
    additionally log_factors [E][2 + K][C] (the cost row last) as the last item.  cost_exponent = 0 is log_ei_constrained_ensemble
    bit for bit.  SingularMatrixException(e (2 + K) + role, j): the GP, counted flat, and the pending point."""
    pre, post, E, K, d, keep = _ei_per_cost_args(gps, constraint_gps, thresholds, cost_gps, cost_exponent, best_so_far)
    return _acq1_evaluate(_lib.load().moe_log_ei_per_cost_mcmc, pre, post, d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 2 + K), want_extra=want_log_factors)


def log_ei_per_cost_multistart(gps, constraint_gps, thresholds, cost_gps, cost_exponent, gd_params, bounds, best_so_far, starts,
                               gradient_ascent=True, want_path=False, points_being_sampled=None):
    """moe_log_ei_per_cost_mcmc_multistart: one suggestion by log_ei_per_cost_ensemble's objective --
    log_ei_constrained_multistart's screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict."""
    pre, post, E, K, d, keep = _ei_per_cost_args(gps, constraint_gps, thresholds, cost_gps, cost_exponent, best_so_far)
    return _acq1_multistart(_lib.load().moe_log_ei_per_cost_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled)


def log_ei_per_cost_suggest(gps, constraint_gps, thresholds, cost_gps, cost_exponent, gd_params, bounds, best_so_far, starts,
                            num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_log_ei_per_cost_mcmc_suggest: num_to_sample points greedily by log_ei_per_cost_ensemble's objective -- round t is
    log_ei_per_cost_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None)
    followed by the points of the rounds before, bit for bit, in one device call.  (p + num_to_sample - 1) (1 + g) <= 64.
    Returns a dict: points [q][dim], values [q], found [q]."""
    pre, post, E, K, d, keep = _ei_per_cost_args(gps, constraint_gps, thresholds, cost_gps, cost_exponent, best_so_far)
    return _acq1_suggest(_lib.load().moe_log_ei_per_cost_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _ehvi_members(gps, gps2, reference_point, front):
    """(objective-1 handles, objective-2 handles, E, dim, GPs kept alive, reference point [2], front [F][2] or None, F) of the
    ensemble forms of the expected hypervolume improvement; gps and gps2 shaped alike (a DeviceGPMCMC, a list of DeviceGP or one
    DeviceGP), E members each"""
    if isinstance(gps, DeviceGP):
        gps = [gps]
    if isinstance(gps2, DeviceGP):
        gps2 = [gps2]
    arr, E, d, keep = _ensemble_handles(gps)
    arr2, E2, d2, keep2 = _ensemble_handles(gps2)
    if E == 0 or E2 != E:
        raise BoundsException("one GP per ensemble member and objective", E2, E, E)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    if ref.size != 2:
        raise BoundsException("the reference point has two coordinates", ref.size, 2, 2)
    fr = np.ascontiguousarray([] if front is None else front, dtype=np.float64).reshape(-1, 2)
    F = fr.shape[0]
    return arr, arr2, E, d, (keep, keep2), ref, (fr if F else None), F


def ehvi_ensemble(gps, gps2, reference_point, front, points, points_being_sampled=None, want_grad=True, want_member_values=False):
    """moe_ehvi_mcmc: the two-objective expected hypervolume improvement (minimisation) averaged over the ensemble at points [C][dim],
    in one device call.  Member e is gps[e] (objective 1) and gps2[e] (objective 2), without derivative observations.
    reference_point [2]; front [F][2] (None or empty: none; F <= 960) sorted by the first objective ascending, mutually non-dominated
    and strictly inside the reference point (pareto_front of expected_hypervolume_improvement.py returns that form).
    points_being_sampled [p][dim] condition both GPs' covariances, and their believed outcomes join every member's own front.
    Returns value [C], with want_grad (value, grad [C][dim]), and with want_member_values additionally the members' values [E][C] as
    the last item.  SingularMatrixException(2 e + objective - 1, j): the GP, counted flat, and the pending point."""
    arr, arr2, E, d, keep, ref, fr, F = _ehvi_members(gps, gps2, reference_point, front)
    pre, post = (arr, arr2, E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F), ()
    return _acq1_evaluate(_lib.load().moe_ehvi_mcmc, pre, post, d, points, want_grad, points_being_sampled,
                          extra_shape=(E,), want_extra=want_member_values)


def ehvi_multistart(gps, gps2, reference_point, front, gd_params, bounds, starts, gradient_ascent=True, want_path=False,
                    points_being_sampled=None):
    """moe_ehvi_mcmc_multistart: one suggestion by the ensemble-averaged expected hypervolume improvement -- ei_analytic_multistart's
    screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict."""
    arr, arr2, E, d, keep, ref, fr, F = _ehvi_members(gps, gps2, reference_point, front)
    pre, post = (arr, arr2, E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F), ()
    return _acq1_multistart(_lib.load().moe_ehvi_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent, want_path,
                            points_being_sampled)


def ehvi_suggest(gps, gps2, reference_point, front, gd_params, bounds, starts, num_to_sample, gradient_ascent=True,
                 points_being_sampled=None):
    """moe_ehvi_mcmc_suggest: num_to_sample points greedily by the ensemble-averaged expected hypervolume improvement -- round t is
    ehvi_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None) followed by
    the points of the rounds before, bit for bit, in one device call.  p + num_to_sample - 1 <= 64.  Returns a dict: points
    [q][dim], values [q], found [q]."""
    arr, arr2, E, d, keep, ref, fr, F = _ehvi_members(gps, gps2, reference_point, front)
    pre, post = (arr, arr2, E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F), ()
    return _acq1_suggest(_lib.load().moe_ehvi_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample, gradient_ascent,
                         points_being_sampled)


def _ehvi3_members(gps, gps2, gps3, reference_point, front):
    """(the three objectives' handles, E, dim, GPs kept alive, reference point [3], front [F][3] or None, F) of the ensemble forms
    of the three-objective expected hypervolume improvement; gps, gps2 and gps3 shaped alike (a DeviceGPMCMC, a list of DeviceGP or
    one DeviceGP), E members each"""
    arrs, keeps, E, d = [], [], None, None
    for g in (gps, gps2, gps3):
        arr, Ek, dk, keep = _ensemble_handles([g] if isinstance(g, DeviceGP) else g)
        if E is None:
            E, d = Ek, dk
        if E == 0 or Ek != E:
            raise BoundsException("one GP per ensemble member and objective", Ek, E, E)
        arrs.append(arr)
        keeps.append(keep)
    ref = np.ascontiguousarray(reference_point, dtype=np.float64).ravel()
    if ref.size != 3:
        raise BoundsException("the reference point has three coordinates", ref.size, 3, 3)
    fr = np.ascontiguousarray([] if front is None else front, dtype=np.float64).reshape(-1, 3)
    F = fr.shape[0]
    return arrs, E, d, keeps, ref, (fr if F else None), F


def ehvi3_ensemble(gps, gps2, gps3, reference_point, front, points, points_being_sampled=None, want_grad=True,
                   want_member_values=False):
    """moe_ehvi3_mcmc: the three-objective expected hypervolume improvement (minimisation) averaged over the ensemble at points
    [C][dim], in one device call.  Member e is gps[e], gps2[e] and gps3[e] (objectives 1, 2, 3), without derivative observations.
    reference_point [3]; front [F][3] (None or empty: none; F <= 192) mutually non-dominated, strictly inside the reference point
    and in the canonical order: the third objective ascending, ties by the first, then by the second (pareto_front_3 of
    expected_hypervolume_improvement.py returns that form).  points_being_sampled [p][dim] condition the three GPs' covariances, and
    their believed outcomes join every member's own front.  Returns value [C], with want_grad (value, grad [C][dim]), and with
    want_member_values additionally the members' values [E][C] as the last item.  SingularMatrixException(3 e + objective - 1, j):
    the GP, counted flat, and the pending point."""
    arrs, E, d, keep, ref, fr, F = _ehvi3_members(gps, gps2, gps3, reference_point, front)
    pre, post = (arrs[0], arrs[1], arrs[2], E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F), ()
    return _acq1_evaluate(_lib.load().moe_ehvi3_mcmc, pre, post, d, points, want_grad, points_being_sampled,
                          extra_shape=(E,), want_extra=want_member_values)


def ehvi3_multistart(gps, gps2, gps3, reference_point, front, gd_params, bounds, starts, gradient_ascent=True, want_path=False,
                     points_being_sampled=None):
    """moe_ehvi3_mcmc_multistart: one suggestion by the ensemble-averaged three-objective expected hypervolume improvement --
    ei_analytic_multistart's screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict."""
    arrs, E, d, keep, ref, fr, F = _ehvi3_members(gps, gps2, gps3, reference_point, front)
    pre, post = (arrs[0], arrs[1], arrs[2], E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F), ()
    return _acq1_multistart(_lib.load().moe_ehvi3_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent, want_path,
                            points_being_sampled)


def ehvi3_suggest(gps, gps2, gps3, reference_point, front, gd_params, bounds, starts, num_to_sample, gradient_ascent=True,
                  points_being_sampled=None):
    """moe_ehvi3_mcmc_suggest: num_to_sample points greedily by the ensemble-averaged three-objective expected hypervolume
    improvement -- round t is ehvi3_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim]
    (may be None) followed by the points of the rounds before, bit for bit, in one device call.  p + num_to_sample - 1 <= 64.
    Returns a dict: points [q][dim], values [q], found [q]."""
    arrs, E, d, keep, ref, fr, F = _ehvi3_members(gps, gps2, gps3, reference_point, front)
    pre, post = (arrs[0], arrs[1], arrs[2], E, ref.ctypes.data_as(dp), fr.ctypes.data_as(dp) if F else None, F), ()
    return _acq1_suggest(_lib.load().moe_ehvi3_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample, gradient_ascent,
                         points_being_sampled)


def _ei_chebyshev_call(objective_gps, scalarisations, best_so_far, num_rounds):
    """(the arguments in front of the shape's own, E, dim, what must stay alive) of the ensemble forms of the Chebyshev-scalarised
    expected improvement.  objective_gps: M ensembles shaped alike (a DeviceGPMCMC, a list of DeviceGP or one DeviceGP), E members
    each; scalarisations [R][2 M] (a, then b); best_so_far [R][E] (one row [E] or one number is spread over the rounds and members)."""
    objs = list(objective_gps)
    M = len(objs)
    members, E, d = [], None, 0
    for g in objs:
        arr, Ek, dk, keep = _ensemble_handles([g] if isinstance(g, DeviceGP) else g)
        if E is None:
            E, d = Ek, dk
        if E == 0 or Ek != E:
            raise BoundsException("one GP per ensemble member and objective", Ek, E, E)
        members.append(keep)
    if E is None:
        raise BoundsException("num_objectives must be between 2 and 8", 0, 2, 8)
    flat = [members[j][e] for e in range(E) for j in range(M)]
    arr = (C.c_void_p * max(len(flat), 1))(*[g._h.value for g in flat])
    R = max(int(num_rounds), 1)
    scal = np.ascontiguousarray(scalarisations, dtype=np.float64).reshape(-1)
    if scal.size != R * 2 * M:
        raise BoundsException("a scalarisation is 2 num_objectives numbers per round", scal.size, R * 2 * M, R * 2 * M)
    best = np.asarray(best_so_far, dtype=np.float64)
    if best.size == R * E:
        best = best.reshape(R, E)
    elif best.size == 1:
        best = np.full((R, E), float(best.ravel()[0]))
    elif best.size == E:
        best = np.broadcast_to(best.reshape(1, E), (R, E))
    else:
        raise BoundsException("one incumbent per round and ensemble member", best.size, R * E, R * E)
    best = np.ascontiguousarray(best, dtype=np.float64)
    return (arr, M, E, scal.ctypes.data_as(dp), best.ctypes.data_as(dp)), E, d, (flat, scal, best)


def ei_chebyshev_ensemble(objective_gps, scalarisation, best_so_far, points, points_being_sampled=None, want_grad=True,
                          want_member_values=False):
    """moe_ei_chebyshev_mcmc: the expected improvement of the weighted Chebyshev scalarisation max_j (a_j Y_j + b_j) of 2 <= M <= 8
    objectives (minimisation) averaged over the ensemble at points [C][dim], in one device call: a fixed quadrature of a product of
    normal CDFs, exact to rounding.  Member e is objective_gps[j][e], j = 0 .. M - 1, without derivative observations; E M <= 1024.
    scalarisation [2 M]: a > 0, then b (chebyshev_scalarisation of expected_scalarised_improvement.py returns that pair);
    best_so_far [E] (or one number): the members' smallest scalarised values so far.  points_being_sampled [p][dim] condition all M
    GPs' covariances, and a member's incumbent is lowered to the smallest scalarised outcome it believes of them.  Returns value
    [C], with want_grad (value, grad [C][dim]), and with want_member_values additionally the members' values [E][C] as the last
    item.  SingularMatrixException(e M + j, i): the GP, counted flat, and the pending point."""
    pre, E, d, keep = _ei_chebyshev_call(objective_gps, scalarisation, best_so_far, 1)
    return _acq1_evaluate(_lib.load().moe_ei_chebyshev_mcmc, pre, (), d, points, want_grad, points_being_sampled,
                          extra_shape=(E,), want_extra=want_member_values)


def ei_chebyshev_multistart(objective_gps, scalarisation, best_so_far, gd_params, bounds, starts, gradient_ascent=True,
                            want_path=False, points_being_sampled=None):
    """moe_ei_chebyshev_mcmc_multistart: one suggestion by the ensemble-averaged Chebyshev-scalarised expected improvement --
    ei_analytic_multistart's screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict."""
    pre, E, d, keep = _ei_chebyshev_call(objective_gps, scalarisation, best_so_far, 1)
    return _acq1_multistart(_lib.load().moe_ei_chebyshev_mcmc_multistart, pre, (), d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled)


def ei_chebyshev_suggest(objective_gps, scalarisations, best_so_far, gd_params, bounds, starts, num_to_sample, gradient_ascent=True,
                         points_being_sampled=None):
    """moe_ei_chebyshev_mcmc_suggest: num_to_sample points greedily, point t under scalarisations[t] [2 M] and the incumbents
    best_so_far[t] [E] -- round t is ei_chebyshev_multistart with that scalarisation from the same starts [S][dim] with the pending
    points points_being_sampled [p][dim] (may be None) followed by the points of the rounds before, bit for bit, in one device
    call.  p + num_to_sample - 1 <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    pre, E, d, keep = _ei_chebyshev_call(objective_gps, scalarisations, best_so_far, num_to_sample)
    return _acq1_suggest(_lib.load().moe_ei_chebyshev_mcmc_suggest, pre, (), d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _log_ei_chebyshev_call(objective_gps, constraint_gps, thresholds, scalarisations, best_so_far, num_rounds):
    """(the arguments in front of the shape's own, E, dim, K, what must stay alive) of the log forms of the Chebyshev-scalarised
    expected improvement: _ei_chebyshev_call's with constraint_gps, K ensembles shaped like the objectives' (None: K = 0), passed
    flat as [K][E], and thresholds [K] behind the objectives."""
    pre, E, d, keep = _ei_chebyshev_call(objective_gps, scalarisations, best_so_far, num_rounds)
    cons = [] if constraint_gps is None else list(constraint_gps)
    K = len(cons)
    tau = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    if tau.size != K:
        raise BoundsException("one threshold per constraint", tau.size, K, K)
    flat = []
    for c in cons:
        members = [c] if isinstance(c, DeviceGP) else (list(c.gps) if isinstance(c, DeviceGPMCMC) else list(c))
        if len(members) != E:
            raise BoundsException("one constraint GP per ensemble member and constraint", len(members), E, E)
        flat += members  # [K][E]
    carr = (C.c_void_p * max(len(flat), 1))(*[g._h.value for g in flat]) if K else None
    arr, M, E_, scal, best = pre
    return (arr, M, carr, K, tau.ctypes.data_as(dp) if K else None, E_, scal, best), E, d, K, (keep, flat, tau, carr)


def log_ei_chebyshev_constrained_ensemble(objective_gps, constraint_gps, thresholds, scalarisation, best_so_far, points,
                                          points_being_sampled=None, want_grad=True, want_factors=False):
    """moe_log_ei_chebyshev_constrained_mcmc: the LOG of ei_chebyshev_ensemble's member value times the probabilities of feasibility,
    under the ensemble's log-sum-exp, at points [C][dim] in one device call -- finite with a useful gradient where the plain form
    and its gradient are exactly 0.  objective_gps, scalarisation and best_so_far as there (every incumbent finite, that of the
    FEASIBLE observations); member e's constraint GPs are constraint_gps[k][e], constraint k satisfied where c_k(x) <=
    thresholds[k] (0 <= K <= 8; None: K = 0); E (M + K) <= 1024.  points_being_sampled [p][dim] condition every GP's covariance; a
    pending point's scalarised outcome lowers member e's incumbent only where the member believes the point feasible.  Returns
    value [C], with want_grad (value, grad [C][dim]), and with want_factors additionally log_factors [E][1 + K][C] (LA_e, then log
    F_{e,1..K}) as the last item.  SingularMatrixException(e (M + K) + role, j): the GP, counted flat, and the pending point."""
    pre, E, d, K, keep = _log_ei_chebyshev_call(objective_gps, constraint_gps, thresholds, scalarisation, best_so_far, 1)
    return _acq1_evaluate(_lib.load().moe_log_ei_chebyshev_constrained_mcmc, pre, (), d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 1 + K), want_extra=want_factors)


def log_ei_chebyshev_constrained_multistart(objective_gps, constraint_gps, thresholds, scalarisation, best_so_far, gd_params, bounds,
                                            starts, gradient_ascent=True, want_path=False, points_being_sampled=None):
    """moe_log_ei_chebyshev_constrained_mcmc_multistart: one suggestion by log_ei_chebyshev_constrained_ensemble's objective --
    ei_analytic_multistart's screening, 20 kept starts, restarted ascent on the device and end-point selection, and its dict."""
    pre, E, d, K, keep = _log_ei_chebyshev_call(objective_gps, constraint_gps, thresholds, scalarisation, best_so_far, 1)
    return _acq1_multistart(_lib.load().moe_log_ei_chebyshev_constrained_mcmc_multistart, pre, (), d, gd_params, bounds, starts,
                            gradient_ascent, want_path, points_being_sampled)


def log_ei_chebyshev_constrained_suggest(objective_gps, constraint_gps, thresholds, scalarisations, best_so_far, gd_params, bounds,
                                         starts, num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_log_ei_chebyshev_constrained_mcmc_suggest: num_to_sample points greedily, point t under scalarisations[t] [2 M] and the
    incumbents best_so_far[t] [E] -- round t is log_ei_chebyshev_constrained_multistart with that scalarisation from the same starts
    with points_being_sampled followed by the points of the rounds before, bit for bit, in one device call.  p + num_to_sample - 1
    <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    pre, E, d, K, keep = _log_ei_chebyshev_call(objective_gps, constraint_gps, thresholds, scalarisations, best_so_far, num_to_sample)
    return _acq1_suggest(_lib.load().moe_log_ei_chebyshev_constrained_mcmc_suggest, pre, (), d, gd_params, bounds, starts,
                         num_to_sample, gradient_ascent, points_being_sampled)


def _ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front):
    """(which entry points: "ehvi" or "ehvi3", the arguments in front of the shape's own, E, dim, K, what must stay alive) of the
    ensemble forms of the constrained expected hypervolume improvement.  objective_gps: 2 or 3 ensembles shaped alike (a
    DeviceGPMCMC, a list of DeviceGP or one DeviceGP), E members each; constraint_gps: K ensembles of the same shape (None: K = 0)."""
    objs = list(objective_gps)
    M = len(objs)
    if M == 2:
        arr, arr2, E, d, keep, ref, fr, F = _ehvi_members(objs[0], objs[1], reference_point, front)
        arrs, stem = [arr, arr2], "moe_ehvi_constrained_mcmc"
    elif M == 3:
        arrs, E, d, keep, ref, fr, F = _ehvi3_members(objs[0], objs[1], objs[2], reference_point, front)
        stem = "moe_ehvi3_constrained_mcmc"
    else:
        raise BoundsException("two or three objectives", M, 2, 3)
    cons = [] if constraint_gps is None else list(constraint_gps)
    K = len(cons)
    tau = np.ascontiguousarray([] if thresholds is None else thresholds, dtype=np.float64).ravel()
    if tau.size != K:
        raise BoundsException("one threshold per constraint", tau.size, K, K)
    per = []
    for c in cons:
        members = [c] if isinstance(c, DeviceGP) else (list(c.gps) if isinstance(c, DeviceGPMCMC) else list(c))
        if len(members) != E:
            raise BoundsException("one constraint GP per ensemble member and constraint", len(members), E, E)
        per.append(members)
    flat = [per[k][e] for e in range(E) for k in range(K)]  # [E][K]
    carr = (C.c_void_p * max(len(flat), 1))(*[g._h.value for g in flat]) if K else None
    pre = tuple(arrs) + (carr, K, tau.ctypes.data_as(dp) if K else None, E, ref.ctypes.data_as(dp),
                         fr.ctypes.data_as(dp) if F else None, F)
    return stem, pre, E, d, K, (keep, flat, tau, ref, fr, carr)


def ehvi_constrained_ensemble(objective_gps, constraint_gps, thresholds, reference_point, front, points, points_being_sampled=None,
                              want_grad=True, want_factors=False):
    """moe_ehvi_constrained_mcmc / moe_ehvi3_constrained_mcmc: the expected hypervolume improvement times the probability of
    feasibility (minimisation), averaged over the ensemble at points [C][dim], in one device call.  objective_gps: 2 or 3 ensembles
    (the number decides which); member e is objective_gps[r][e] and the constraint GPs constraint_gps[k][e], constraint k satisfied
    where c_k(x) <= thresholds[k] (0 <= K <= 8; K = 0 is ehvi_ensemble / ehvi3_ensemble bit for bit).  reference_point and front as
    there, the front that of the FEASIBLE observations (feasible_pareto_front of expected_hypervolume_improvement_constrained.py).
    points_being_sampled [p][dim] condition every GP's covariance; a pending point's believed outcome is offered to member e's front
    only where the member believes it feasible.  Returns value [C], with want_grad (value, grad [C][dim]), and with want_factors
    additionally factors [E][1 + K][C] (the hypervolume term, then the K feasibility factors) as the last item.
    SingularMatrixException(e (M + K) + role, j): the GP, counted flat, and the pending point; a candidate never raises."""
    stem, pre, E, d, K, keep = _ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_evaluate(getattr(_lib.load(), stem), pre, (), d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 1 + K), want_extra=want_factors)


def ehvi_constrained_multistart(objective_gps, constraint_gps, thresholds, reference_point, front, gd_params, bounds, starts,
                                gradient_ascent=True, want_path=False, points_being_sampled=None):
    """moe_ehvi_constrained_mcmc_multistart / moe_ehvi3_constrained_mcmc_multistart: one suggestion by the ensemble-averaged
    constrained expected hypervolume improvement -- ei_analytic_multistart's screening, 20 kept starts, restarted ascent on the
    device and end-point selection, and its dict."""
    stem, pre, E, d, K, keep = _ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_multistart(getattr(_lib.load(), stem + "_multistart"), pre, (), d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled)


def ehvi_constrained_suggest(objective_gps, constraint_gps, thresholds, reference_point, front, gd_params, bounds, starts,
                             num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_ehvi_constrained_mcmc_suggest / moe_ehvi3_constrained_mcmc_suggest: num_to_sample points greedily -- round t is
    ehvi_constrained_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None)
    followed by the points of the rounds before, bit for bit, in one device call.  p + num_to_sample - 1 <= 64.  Returns a dict:
    points [q][dim], values [q], found [q]."""
    stem, pre, E, d, K, keep = _ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_suggest(getattr(_lib.load(), stem + "_suggest"), pre, (), d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _log_ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front):
    """_ehvi_constrained_call for the log form, which is built for two objectives"""
    objs = list(objective_gps)
    if len(objs) != 2:
        raise BoundsException("the log expected hypervolume improvement takes two objectives", len(objs), 2, 2)
    stem, pre, E, d, K, keep = _ehvi_constrained_call(objs, constraint_gps, thresholds, reference_point, front)
    return "moe_log_ehvi_constrained_mcmc", pre, E, d, K, keep


def log_ehvi_constrained_ensemble(objective_gps, constraint_gps, thresholds, reference_point, front, points,
                                  points_being_sampled=None, want_grad=True, want_log_factors=False):
    """moe_log_ehvi_constrained_mcmc: the LOG of what ehvi_constrained_ensemble returns for two objectives, computed so that it
    stays finite with a useful gradient where that value and its gradient are exactly 0 in float64 (a mean dozens of posterior
    standard deviations above the reference point in either objective, a constraint far from feasible).  Arguments as there;
    constraint_gps=None / thresholds=None is K = 0, the log of ehvi_ensemble's value.  Returns value [C], with want_grad (value,
    grad [C][dim]), and with want_log_factors additionally log_factors [E][1 + K][C] (the log hypervolume term, then the K log
    feasibility factors) as the last item; the value is the log-mean-exp over e of the members' sums.  SingularMatrixException as
    there."""
    stem, pre, E, d, K, keep = _log_ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_evaluate(getattr(_lib.load(), stem), pre, (), d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 1 + K), want_extra=want_log_factors)


def log_ehvi_constrained_multistart(objective_gps, constraint_gps, thresholds, reference_point, front, gd_params, bounds, starts,
                                    gradient_ascent=True, want_path=False, points_being_sampled=None):
    """moe_log_ehvi_constrained_mcmc_multistart: one suggestion by the log of the ensemble-averaged constrained expected
    hypervolume improvement -- ehvi_constrained_multistart's screening, 20 kept starts, restarted ascent on the device and end-point
    selection, and its dict, on an objective whose screening values do not tie at 0 and whose gradient does not vanish."""
    stem, pre, E, d, K, keep = _log_ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_multistart(getattr(_lib.load(), stem + "_multistart"), pre, (), d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled)


def log_ehvi_constrained_suggest(objective_gps, constraint_gps, thresholds, reference_point, front, gd_params, bounds, starts,
                                 num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_log_ehvi_constrained_mcmc_suggest: num_to_sample points greedily -- round t is log_ehvi_constrained_multistart from the
    same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None) followed by the points of the rounds
    before, bit for bit, in one device call.  p + num_to_sample - 1 <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    stem, pre, E, d, K, keep = _log_ehvi_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_suggest(getattr(_lib.load(), stem + "_suggest"), pre, (), d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _log_ehvi3_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front):
    """_ehvi_constrained_call for the three-objective log form"""
    objs = list(objective_gps)
    if len(objs) != 3:
        raise BoundsException("the three-objective log expected hypervolume improvement takes three objectives", len(objs), 3, 3)
    stem, pre, E, d, K, keep = _ehvi_constrained_call(objs, constraint_gps, thresholds, reference_point, front)
    return "moe_log_ehvi3_constrained_mcmc", pre, E, d, K, keep


def log_ehvi3_constrained_ensemble(objective_gps, constraint_gps, thresholds, reference_point, front, points,
                                   points_being_sampled=None, want_grad=True, want_log_factors=False):
    """moe_log_ehvi3_constrained_mcmc: the LOG of what ehvi_constrained_ensemble returns for three objectives, computed so that it
    stays finite with a useful gradient where that value and its gradient are exactly 0 in float64 (a mean dozens of posterior
    standard deviations above the reference point in any one objective, a constraint far from feasible).  Arguments as there, the
    front [F][3] in the canonical order; constraint_gps=None / thresholds=None is K = 0, the log of ehvi3_ensemble's value.  Returns
    value [C], with want_grad (value, grad [C][dim]), and with want_log_factors additionally log_factors [E][1 + K][C] (the log
    hypervolume term, then the K log feasibility factors) as the last item; the value is the log-mean-exp over e of the members'
    sums.  SingularMatrixException as there."""
    stem, pre, E, d, K, keep = _log_ehvi3_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_evaluate(getattr(_lib.load(), stem), pre, (), d, points, want_grad, points_being_sampled,
                          extra_shape=(E, 1 + K), want_extra=want_log_factors)


def log_ehvi3_constrained_multistart(objective_gps, constraint_gps, thresholds, reference_point, front, gd_params, bounds, starts,
                                     gradient_ascent=True, want_path=False, points_being_sampled=None):
    """moe_log_ehvi3_constrained_mcmc_multistart: one suggestion by the log of the ensemble-averaged three-objective constrained
    expected hypervolume improvement -- ehvi_constrained_multistart's screening, 20 kept starts, restarted ascent on the device and
    end-point selection, and its dict, on an objective whose screening values do not tie at 0 and whose gradient does not vanish."""
    stem, pre, E, d, K, keep = _log_ehvi3_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_multistart(getattr(_lib.load(), stem + "_multistart"), pre, (), d, gd_params, bounds, starts, gradient_ascent,
                            want_path, points_being_sampled)


def log_ehvi3_constrained_suggest(objective_gps, constraint_gps, thresholds, reference_point, front, gd_params, bounds, starts,
                                  num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_log_ehvi3_constrained_mcmc_suggest: num_to_sample points greedily -- round t is log_ehvi3_constrained_multistart from the
    same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None) followed by the points of the rounds
    before, bit for bit, in one device call.  p + num_to_sample - 1 <= 64.  Returns a dict: points [q][dim], values [q], found [q]."""
    stem, pre, E, d, K, keep = _log_ehvi3_constrained_call(objective_gps, constraint_gps, thresholds, reference_point, front)
    return _acq1_suggest(getattr(_lib.load(), stem + "_suggest"), pre, (), d, gd_params, bounds, starts, num_to_sample,
                         gradient_ascent, points_being_sampled)


def _gibbon_members(gps, min_values):
    """(handles, count, dim, members kept alive, min-values [E][K], K) of the ensemble forms of the min-value entropy acquisition; a
    single DeviceGP counts as a list of one"""
    if isinstance(gps, DeviceGP):
        gps = [gps]
    arr, E, d, keep = _ensemble_handles(gps)
    mins = np.ascontiguousarray(min_values, dtype=np.float64)
    if E == 0 or mins.size % E != 0 or (mins.ndim > 1 and mins.shape[0] != E):
        raise BoundsException("one row of min-values per ensemble member", mins.shape[0] if mins.ndim else 0, E, E)
    mins = mins.reshape(E, -1)
    return arr, E, d, keep, mins, mins.shape[1]


def gibbon_ensemble(gps, points, min_values, points_being_sampled=None, want_grad=True):
    """moe_gibbon_mcmc: the min-value entropy acquisition GIBBON (for minimisation) averaged over the ensemble at points [C][dim], in
    one device call, member e against its samples of the global minimum value min_values[e] ([E][K], 1 <= K <= 1024, all finite:
    BoundsException(K, 1, 1024), InvalidValueException(value, member, index)).  points_being_sampled [p][dim] (None or empty: none):
    every member's covariance is conditioned on the pending points and the value gains 1/2 log of the conditioned over the
    unconditioned predictive variance, the exact greedy increment of GIBBON's batch term.  gps, derivative observations and the row
    limit as in ei_analytic_ensemble.  Returns value [C], with want_grad (value, grad [C][dim]).  SingularMatrixException(e, j):
    member e, pending point j; a candidate never raises."""
    arr, E, d, keep, mins, K = _gibbon_members(gps, min_values)
    pre, post = (arr, E), (mins.ctypes.data_as(dp), K)
    return _acq1_evaluate(_lib.load().moe_gibbon_mcmc, pre, post, d, points, want_grad, points_being_sampled)


def gibbon_multistart(gps, gd_params, bounds, min_values, starts, gradient_ascent=True, want_path=False, points_being_sampled=None):
    """moe_gibbon_mcmc_multistart: one suggestion by the ensemble-averaged min-value entropy acquisition -- ei_analytic_multistart's
    screening, kept starts, restarted ascent on the device and end-point selection, and its dict."""
    arr, E, d, keep, mins, K = _gibbon_members(gps, min_values)
    pre, post = (arr, E), (mins.ctypes.data_as(dp), K)
    return _acq1_multistart(_lib.load().moe_gibbon_mcmc_multistart, pre, post, d, gd_params, bounds, starts, gradient_ascent, want_path,
                            points_being_sampled)


def gibbon_suggest(gps, gd_params, bounds, min_values, starts, num_to_sample, gradient_ascent=True, points_being_sampled=None):
    """moe_gibbon_mcmc_suggest: num_to_sample points greedily by the ensemble-averaged min-value entropy acquisition -- round t is
    gibbon_multistart from the same starts [S][dim] with the pending points points_being_sampled [p][dim] (may be None) followed by
    the points of the rounds before, bit for bit, in one device call; the limits of ei_analytic_suggest.  Returns a dict: points
    [q][dim], values [q], found [q]."""
    arr, E, d, keep, mins, K = _gibbon_members(gps, min_values)
    pre, post = (arr, E), (mins.ctypes.data_as(dp), K)
    return _acq1_suggest(_lib.load().moe_gibbon_mcmc_suggest, pre, post, d, gd_params, bounds, starts, num_to_sample, gradient_ascent,
                         points_being_sampled)


def recommend(gps, candidates, gd_params, domain_bounds, num_fidelity=0, num_starts=1, want_values=False, want_path=False):
    """moe_posterior_mean_mcmc_recommend: screen the candidates [C][dim - num_fidelity] on the ensemble-averaged posterior mean,
    descend from the num_starts best (the reference's Python gradient descent, on the device), keep the screened candidate unless
    the descent did at least as well.  Returns a dict: point [size], value, screened_index, refined, end_points [num_starts][size],
    and with want_values candidate_values [C], with want_path path [num_starts][max_num_steps + 1][size]."""
    arr, E, d, keep = _ensemble_handles(gps)
    size = d - int(num_fidelity)
    if E > 0 and not 0 < size <= d:
        raise BoundsException("num_fidelity out of range", num_fidelity, 0, d - 1)
    g = DeviceGP._gd(gd_params)
    cand, cp = _d(candidates)
    C_ = cand.reshape(-1, max(size, 1)).shape[0]
    bounds, bp = _d(domain_bounds)
    S = int(num_starts)
    point = np.zeros(max(size, 1))
    ends = np.zeros((max(S, 1), max(size, 1)))
    values = np.zeros(C_) if want_values else None
    path = np.zeros((max(S, 1), max(g.max_num_steps, 0) + 1, max(size, 1))) if want_path else None
    value, index, refined = C.c_double(0.0), C.c_int(0), C.c_int(0)
    err = _lib.MoeError()
    _check(_lib.load().moe_posterior_mean_mcmc_recommend(arr, E, int(num_fidelity), C.byref(g), bp, cp, C_, S,
                                                         point.ctypes.data_as(dp), C.byref(value), C.byref(index), C.byref(refined),
                                                         values.ctypes.data_as(dp) if want_values else None,
                                                         ends.ctypes.data_as(dp), path.ctypes.data_as(dp) if want_path else None,
                                                         C.byref(err)), err)
    out = dict(point=point, value=value.value, screened_index=index.value, refined=bool(refined.value), end_points=ends)
    if want_values:
        out["candidate_values"] = values
    if want_path:
        out["path"] = path
    return out


TRACE_EXTRA = 6  # trace columns behind the point: f0 | halvings | limiter changed | rejected | stopped by norm | state


def minimize_member_means(gps, candidates, gd, bounds, num_fidelity=0, want_means=False, want_trace=False):
    """moe_posterior_mean_members_minimize: for every member of the ensemble by itself, screen the candidates on the member's
    posterior mean (fidelity coordinates pinned to 1), run ComputeOptimalPosteriorMean's line search from the best on the device,
    keep the start if the search ended worse.  candidates [C][size] (one set for all members) or [E][C][size] (member e's own
    set), size = dim - num_fidelity.  Returns a dict: best_points [E][size], best_values [E], start_index [E], fell_back [E]
    (bool); with want_means means [E][C]; with want_trace trace [E][max_num_restarts][max_num_steps][size + 6] (moe_hip.h)."""
    arr, E, d, keep = _ensemble_handles(gps)
    size = d - int(num_fidelity)
    if E > 0 and not 0 < size <= d:
        raise BoundsException("num_fidelity out of range", num_fidelity, 0, d - 1)
    g = DeviceGP._gd(gd)
    cand = np.ascontiguousarray(candidates, dtype=np.float64)
    per_member = cand.ndim == 3
    if per_member and cand.shape[0] != E:
        raise InvalidValueException("per-member candidates need one set per member", cand.shape[0], E, 0)
    C_ = cand.reshape(-1, max(size, 1)).shape[0] // (max(E, 1) if per_member else 1)
    bounds, bp = _d(bounds)
    En, R, T = max(E, 1), max(g.max_num_restarts, 0), max(g.max_num_steps, 0)
    points = np.zeros((En, max(size, 1)))
    values = np.zeros(En)
    index = np.zeros(En, dtype=np.int32)
    fell = np.zeros(En, dtype=np.int32)
    means = np.zeros((En, max(C_, 1))) if want_means else None
    trace = np.zeros((En, R, T, max(size, 1) + TRACE_EXTRA)) if want_trace else None
    err = _lib.MoeError()
    _check(_lib.load().moe_posterior_mean_members_minimize(arr, E, int(num_fidelity), C.byref(g), bp, cand.ctypes.data_as(dp), C_,
                                                           1 if per_member else 0, points.ctypes.data_as(dp),
                                                           values.ctypes.data_as(dp), index.ctypes.data_as(_lib.ip),
                                                           fell.ctypes.data_as(_lib.ip),
                                                           means.ctypes.data_as(dp) if want_means else None,
                                                           trace.ctypes.data_as(dp) if want_trace else None, C.byref(err)), err)
    out = dict(best_points=points, best_values=values, start_index=index.astype(np.int64), fell_back=fell.astype(bool))
    if want_means:
        out["means"] = means
    if want_trace:
        out["trace"] = trace
    return out


def _path_tables(E, d, n, frequencies, phases, weights, noise_normals):
    """the tables of a paths call as contiguous doubles, and (M, S)"""
    freq = np.ascontiguousarray(frequencies, dtype=np.float64).reshape(-1, max(d, 1))
    M = freq.shape[0]
    ph = np.ascontiguousarray(phases, dtype=np.float64).ravel()
    w = np.ascontiguousarray(weights, dtype=np.float64)
    z = np.ascontiguousarray(noise_normals, dtype=np.float64)
    if ph.size != M or w.ndim != 3 or w.shape[0] != max(E, 1) or w.shape[2] != M:
        raise InvalidValueException("the tables must be frequencies [M][dim], phases [M], weights [E][S][M]", ph.size, M, 0)
    S = w.shape[1]
    if z.shape != (max(E, 1), S, n):
        raise InvalidValueException("noise_normals must be [E][S][num_sampled]", z.size, max(E, 1) * S * n, 0)
    return freq, ph, w, z, M, S


def paths_evaluate(gps, frequencies, phases, weights, noise_normals, points, want_grad=False):
    """moe_gp_paths_evaluate: the posterior function paths f_s of every member of the ensemble (pathwise conditioning, moe_hip.h) at
    points [C][dim] in one device call.  frequencies [M][dim] (unit scale, drawn for the members' covariance), phases [M], weights
    [E][S][M], noise_normals [E][S][num_sampled].  Returns values [E][S][C], with want_grad (values, grad [E][S][C][dim])."""
    arr, E, d, keep = _ensemble_handles(gps)
    n = keep[0].n if keep else 0
    freq, ph, w, z, M, S = _path_tables(E, d, n, frequencies, phases, weights, noise_normals)
    pts, pp = _d(points)
    C_ = pts.reshape(-1, max(d, 1)).shape[0]
    values = np.zeros((max(E, 1), S, max(C_, 1)))
    grad = np.zeros((max(E, 1), S, max(C_, 1), max(d, 1))) if want_grad else None
    err = _lib.MoeError()
    _check(_lib.load().moe_gp_paths_evaluate(arr, E, freq.ctypes.data_as(dp), ph.ctypes.data_as(dp), M, w.ctypes.data_as(dp),
                                             z.ctypes.data_as(dp), S, pp, C_, 1 if want_grad else 0, values.ctypes.data_as(dp),
                                             grad.ctypes.data_as(dp) if want_grad else None, C.byref(err)), err)
    return (values, grad) if want_grad else values


def paths_minimize(gps, frequencies, phases, weights, noise_normals, gd, bounds, candidates, want_screened=False, want_trace=False):
    """moe_gp_paths_minimize: every path of every member screened at candidates [C][dim], minimised by minimize_member_means' line
    search from its best candidate on the device, the start kept if the search ended worse.  The tables as in paths_evaluate.
    Returns a dict: best_points [E][S][dim], best_values, start_index, fell_back (bool) [E][S]; with want_screened screened
    [E][S][C]; with want_trace trace [E][S][max_num_restarts][max_num_steps][dim + 6] (moe_hip.h)."""
    arr, E, d, keep = _ensemble_handles(gps)
    n = keep[0].n if keep else 0
    freq, ph, w, z, M, S = _path_tables(E, d, n, frequencies, phases, weights, noise_normals)
    g = DeviceGP._gd(gd)
    cand, cp = _d(candidates)
    C_ = cand.reshape(-1, max(d, 1)).shape[0]
    bounds, bp = _d(bounds)
    En, R, T = max(E, 1), max(g.max_num_restarts, 0), max(g.max_num_steps, 0)
    points = np.zeros((En, S, max(d, 1)))
    values = np.zeros((En, S))
    index = np.zeros((En, S), dtype=np.int32)
    fell = np.zeros((En, S), dtype=np.int32)
    screened = np.zeros((En, S, max(C_, 1))) if want_screened else None
    trace = np.zeros((En, S, R, T, max(d, 1) + TRACE_EXTRA)) if want_trace else None
    err = _lib.MoeError()
    _check(_lib.load().moe_gp_paths_minimize(arr, E, freq.ctypes.data_as(dp), ph.ctypes.data_as(dp), M, w.ctypes.data_as(dp),
                                             z.ctypes.data_as(dp), S, C.byref(g), bp, cp, C_, points.ctypes.data_as(dp),
                                             values.ctypes.data_as(dp), index.ctypes.data_as(_lib.ip), fell.ctypes.data_as(_lib.ip),
                                             screened.ctypes.data_as(dp) if want_screened else None,
                                             trace.ctypes.data_as(dp) if want_trace else None, C.byref(err)), err)
    out = dict(best_points=points, best_values=values, start_index=index.astype(np.int64), fell_back=fell.astype(bool))
    if want_screened:
        out["screened"] = screened
    if want_trace:
        out["trace"] = trace
    return out


def kg_multistart_multi(gps, outer_params, inner_params, bounds, discrete, starts, Xp, num_mc, best_so_far, normals,
                        gradient_ascent=True, num_fidelity=0):
    """moe_kg_multistart_multi (r5): the outer optimiser with its restarts dealt to `gps` -- DeviceGP objects holding the same GP on
    devices 0 .. W-1 -- one host thread per handle, the exchange in shared memory.  (best_points [q][dim], best_kg, found): bit for
    bit DeviceGP.kg_multistart's."""
    g0 = gps[0]
    go, gi = DeviceGP._gd(outer_params), DeviceGP._gd(inner_params)
    bounds, bp = _d(bounds)
    discrete, dpp = _d(discrete)
    P = discrete.reshape(-1, g0.d - num_fidelity).shape[0]
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    S, q, _ = starts.shape
    if Xp is None or np.size(Xp) == 0:
        p, ppp = 0, None
    else:
        Xp, ppp = _d(Xp)
        p = Xp.reshape(-1, g0.d).shape[0]
    normals, npn = _d(normals)
    arr = (C.c_void_p * len(gps))(*[g._h.value for g in gps])
    best = np.zeros(q * g0.d)
    val, found, err = C.c_double(0.0), C.c_int(0), _lib.MoeError()
    _check(_lib.load().moe_kg_multistart_multi(arr, len(gps), int(num_fidelity), C.byref(go), C.byref(gi), bp, dpp, P,
                                               starts.ctypes.data_as(dp), S, ppp, q, p, int(num_mc), float(best_so_far), npn,
                                               1 if gradient_ascent else 0, best.ctypes.data_as(dp), C.byref(val), C.byref(found),
                                               C.byref(err)), err)
    return best.reshape(q, g0.d), val.value, bool(found.value)


def kg_mcmc_multistart_multi(mcmc, num_workers, outer_params, inner_params, bounds, discrete_all, starts, Xp, num_mc, best_so_far,
                             normals, gradient_ascent=True, num_fidelity=0):
    """moe_kg_mcmc_multistart_multi (r5): `mcmc` = a DeviceGPMCMC holding the WHOLE ensemble (member g built on device
    g % num_workers by the caller); worker k -- a host thread -- takes members k, k + num_workers, ...  Result: bit for bit
    DeviceGPMCMC.kg_multistart's."""
    starts, S, q, Xp, p, ppp = mcmc._common(starts, Xp)
    go, gi = DeviceGP._gd(outer_params), DeviceGP._gd(inner_params)
    bounds, bp = _d(bounds)
    disc = mcmc._local(discrete_all)
    P = disc.shape[1] // (mcmc.d - num_fidelity)
    best = mcmc._local(best_so_far).ravel()
    normals, npn = _d(normals)
    out = np.zeros(q * mcmc.d)
    val, found, err = C.c_double(0.0), C.c_int(0), _lib.MoeError()
    _check(_lib.load().moe_kg_mcmc_multistart_multi(mcmc._arr, len(mcmc.gps), int(num_workers), int(num_fidelity), C.byref(go),
                                                    C.byref(gi), bp, disc.ctypes.data_as(dp), P, starts.ctypes.data_as(dp), S, ppp,
                                                    q, p, int(num_mc), best.ctypes.data_as(dp), npn, 1 if gradient_ascent else 0,
                                                    out.ctypes.data_as(dp), C.byref(val), C.byref(found), C.byref(err)), err)
    return out.reshape(q, mcmc.d), val.value, bool(found.value)


class LogLikelihood(object):
    """Log likelihood of fixed data under varying hyper-parameters (moe_ll_*): the evaluator a hyper-parameter
    sampler calls thousands of times (LogMarginalLikelihoodEvaluator, gpp_model_selection.cpp:540-612).  objective:
    _lib.LL_LOG_MARGINAL (the default) or _lib.LL_LEAVE_ONE_OUT -- what evaluate, grad, ascend, multistart and mcmc compute."""

    def __init__(self, X, y, derivatives=(), cov_type=_lib.COV_MATERN_NU_2P5, device=0, objective=_lib.LL_LOG_MARGINAL):
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.n, self.d = X.shape
        self.derivatives = [int(v) for v in derivatives]
        self.g = len(self.derivatives)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(self.n, 1 + self.g)
        dv = np.ascontiguousarray(self.derivatives, dtype=np.int32)
        self._h = C.c_void_p(None)
        err = _lib.MoeError()
        _check(_lib.load().moe_ll_create(int(cov_type), X.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                         dv.ctypes.data_as(ip) if self.g else None, self.g, self.d, self.n, int(device),
                                         C.byref(self._h), C.byref(err)), err)
        if int(objective) != _lib.LL_LOG_MARGINAL:
            self.set_objective(objective)

    @property
    def objective(self):
        return int(_lib.load().moe_ll_get_objective(self._h))

    def set_objective(self, objective):
        """moe_ll_set_objective: _lib.LL_LOG_MARGINAL or _lib.LL_LEAVE_ONE_OUT (BoundsException otherwise)."""
        err = _lib.MoeError()
        _check(_lib.load().moe_ll_set_objective(self._h, int(objective), C.byref(err)), err)

    def loo_predict(self, hyperparameters):
        """moe_ll_loo_predict: the leave-one-out predictive (mean, var), each [n][1 + g], of every observation at one
        hyper-parameter set [1 + dim + 1 + g], whatever the handle's objective."""
        h = np.ascontiguousarray(hyperparameters, dtype=np.float64).reshape(1 + self.d + 1 + self.g)
        mean, var = np.zeros((self.n, 1 + self.g)), np.zeros((self.n, 1 + self.g))
        err = _lib.MoeError()
        _check(_lib.load().moe_ll_loo_predict(self._h, h.ctypes.data_as(dp), mean.ctypes.data_as(dp), var.ctypes.data_as(dp),
                                              C.byref(err)), err)
        return mean, var

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.load().moe_ll_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, hyperparameters_all):
        """hyperparameters_all [num_sets][1 + dim + 1 + g] = (alpha, lengths, noise variances) -> values [num_sets]
        (-inf where K + noise is singular)."""
        h = np.ascontiguousarray(hyperparameters_all, dtype=np.float64).reshape(-1, 1 + self.d + 1 + self.g)
        out = np.zeros(h.shape[0])
        err = _lib.MoeError()
        _check(_lib.load().moe_ll_evaluate(self._h, h.ctypes.data_as(dp), h.shape[0], out.ctypes.data_as(dp), C.byref(err)), err)
        return out

    def multistart(self, gd_params, domain_log10, initial_guesses):
        """moe_ll_multistart: maximum-likelihood hyper-parameters by restarted gradient ascent from initial_guesses [S][1 + dim + 1 + g]
        (linear space) inside domain_log10 [n_hyper][2] (log-10 space) -> (best [n_hyper], best log likelihood, found)."""
        nh = 1 + self.d + 1 + self.g
        g = DeviceGP._gd(gd_params)
        dom, dpp = _d(domain_log10)
        x0 = np.ascontiguousarray(initial_guesses, dtype=np.float64).reshape(-1, nh)
        out = np.zeros(nh)
        val, found, err = C.c_double(0.0), C.c_int(0), _lib.MoeError()
        _check(_lib.load().moe_ll_multistart(self._h, C.byref(g), dpp, x0.ctypes.data_as(dp), x0.shape[0], out.ctypes.data_as(dp),
                                             C.byref(val), C.byref(found), C.byref(err)), err)
        return out, val.value, bool(found.value)

    def ascend(self, gd_params, domain_log10, x0):
        """moe_ll_ascend: the end point of the restarted gradient ascent from x0 [1 + dim + 1 + g] (linear space)."""
        nh = 1 + self.d + 1 + self.g
        g = DeviceGP._gd(gd_params)
        dom, dpp = _d(domain_log10)
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(nh)
        out = np.zeros(nh)
        err = _lib.MoeError()
        _check(_lib.load().moe_ll_ascend(self._h, C.byref(g), dpp, x0.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(err)), err)
        return out

    def grad(self, hyperparameters):
        """d log p / d (alpha, lengths, noise variances) at one hyper-parameter set [1 + dim + 1 + g] (moe_ll_grad)."""
        h = np.ascontiguousarray(hyperparameters, dtype=np.float64).reshape(1 + self.d + 1 + self.g)
        out = np.zeros(h.size)
        err = _lib.MoeError()
        _check(_lib.load().moe_ll_grad(self._h, h.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(err)), err)
        return out

    def mcmc(self, priors, p0, u_stretch, partner, u_accept, stretch_a=2.0, diagnostics=True):
        """moe_ll_mcmc on this handle: see ll_mcmc."""
        return ll_mcmc(self, priors, p0, u_stretch, partner, u_accept, stretch_a=stretch_a, diagnostics=diagnostics)


def stretch_tables(rng, num_steps, num_walkers):
    """The random tables of a stretch-move chain from a numpy.random.RandomState: per half-step W/2 uniforms for z, W/2
    partner indices in [0, W/2), W/2 uniforms for the accept -- in that order.  Returns (u_stretch, partner, u_accept), each
    [num_steps][2][W/2]."""
    T, H = int(num_steps), int(num_walkers) // 2
    u_stretch, partner, u_accept = np.zeros((T, 2, H)), np.zeros((T, 2, H), dtype=np.int32), np.zeros((T, 2, H))
    for t in range(T):
        for h in range(2):
            u_stretch[t, h] = rng.rand(H)
            partner[t, h] = rng.randint(H, size=H)
            u_accept[t, h] = rng.rand(H)
    return u_stretch, partner, u_accept


def ll_mcmc(ll, priors, p0, u_stretch, partner, u_accept, stretch_a=2.0, diagnostics=True):
    """moe_ll_mcmc: the stretch-move ensemble sampler over log-space hyper-parameters, the whole chain on the device.
    ll: a LogLikelihood; priors: nh rows (kind, a, b) (_lib.PRIOR_*); p0 [W][nh]; the tables [T][2][W/2] (stretch_tables).
    Returns a dict: chain [T][W][nh], lnprob [T][W], lnprob0 [W] and, with diagnostics, proposal_lnprob [T][W], accepted [T][W]."""
    nh = 1 + ll.d + 1 + ll.g
    table = [(int(k), float(a), float(b)) for k, a, b in priors]
    if len(table) != nh:
        raise BoundsException("the prior table needs one row per hyper-parameter", len(table), nh, nh)
    p0 = np.ascontiguousarray(p0, dtype=np.float64)
    if p0.ndim != 2 or p0.shape[1] != nh:
        raise BoundsException("p0 must be [num_walkers][%d]" % nh, p0.shape[-1] if p0.ndim else 0, nh, nh)
    W = p0.shape[0]
    u_stretch = np.ascontiguousarray(u_stretch, dtype=np.float64)
    u_accept = np.ascontiguousarray(u_accept, dtype=np.float64)
    partner = np.ascontiguousarray(partner, dtype=np.int32)
    T = u_stretch.shape[0] if u_stretch.ndim == 3 else 0
    for name, a in (("u_stretch", u_stretch), ("partner", partner), ("u_accept", u_accept)):
        if a.shape != (T, 2, W // 2):
            raise BoundsException("%s must be [num_steps][2][num_walkers / 2]" % name, a.size, T * 2 * (W // 2), T * 2 * (W // 2))
    pr = (_lib.Prior * nh)(*[_lib.Prior(k, a, b) for k, a, b in table])
    chain, lnprob, lnprob0 = np.zeros((T, W, nh)), np.zeros((T, W)), np.zeros(W)
    prop = np.zeros((T, W)) if diagnostics else None
    acc = np.zeros((T, W), dtype=np.int32) if diagnostics else None
    err = _lib.MoeError()
    _check(_lib.load().moe_ll_mcmc(ll._h, pr, W, T, float(stretch_a), p0.ctypes.data_as(dp), u_stretch.ctypes.data_as(dp),
                                   partner.ctypes.data_as(ip), u_accept.ctypes.data_as(dp), chain.ctypes.data_as(dp),
                                   lnprob.ctypes.data_as(dp), lnprob0.ctypes.data_as(dp),
                                   prop.ctypes.data_as(dp) if diagnostics else None,
                                   acc.ctypes.data_as(ip) if diagnostics else None, C.byref(err)), err)
    out = dict(chain=chain, lnprob=lnprob, lnprob0=lnprob0)
    if diagnostics:
        out.update(proposal_lnprob=prop, accepted=acc)
    return out
