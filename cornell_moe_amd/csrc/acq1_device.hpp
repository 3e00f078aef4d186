// cornell_moe_amd/csrc/acq1_device.hpp -- the device pieces the candidate kernels of the one-point acquisitions share (ei1.hip,
// gibbon1.hip, cei1.hip, ehvi1.hip, logcei1.hip; kg1.hip takes the density): one definition each, inlined into every kernel that
// uses it.
#pragma once
#include <cfloat>

#include <hip/hip_runtime.h>

namespace moe {

// The reference's two variance floors: the value's (gpp_math.hpp:1316) and the gradient's (gpp_math.hpp:1323).
constexpr double kMinVarEI = DBL_MIN;
constexpr double kMinVarGradEI = 150.0 * DBL_EPSILON * DBL_EPSILON;

__device__ __forceinline__ double normal_pdf(double x) { return 0.3989422804014326779399460599343818684759 * exp(-0.5 * x * x); }
// Phi through erfc on the side of x's sign: no cancellation in either tail
__device__ __forceinline__ double normal_cdf(double x) {
  const double r = 0.7071067811865475244008443621048490392848;
  return (x <= 0.0) ? 0.5 * erfc(-x * r) : 1.0 - 0.5 * erfc(x * r);
}

// The log forms (logcei1.hip).  With h(c) = c Phi(c) + phi(c), so that EI = sigma h(c): log h(c), lambda = Phi(c) / h(c) and
// kappa = phi(c) / h(c), finite for every finite c.
//   c >= 0        the direct expressions
//   -6 <= c < 0   h / phi = 1 + c sqrt(pi / 2) erfcx(-c / sqrt 2) = q:  log h = log phi + log q, kappa = 1 / q, lambda = (Phi / phi) / q
//   c < -6        Laplace's continued fraction of the Mills ratio, bottom-up, a = -c:  t2 = a + 2 / (a + 3 / (a + ... 20 / a)),
//                 t1 = a + 1 / t2,  Phi / phi = 1 / t1,  h / phi = 1 / (t1 t2): all terms positive, nothing cancels
//                 log h = log phi - log(t1 t2), lambda = t2, kappa = t1 t2
// (q loses digits as c falls, 1.4e-14 in lambda and kappa at -6, where the fraction has converged to 7e-16: DESIGN 5.22).
constexpr double kLogSqrt2Pi = 0.9189385332046727417803297364056176398614;
constexpr double kLogEiSwitch = -6.0;
constexpr int kLogEiFractionTerms = 20;
__device__ __forceinline__ void log_h_parts(double c, double& log_h, double& lambda, double& kappa) {
  if (c >= 0.0) {
    const double P = normal_cdf(c), p = normal_pdf(c);
    const double h = c * P + p;
    log_h = log(h);
    lambda = P / h;
    kappa = p / h;
    return;
  }
  const double log_phi = -0.5 * c * c - kLogSqrt2Pi;
  if (c >= kLogEiSwitch) {
    const double mills = 1.2533141373155002512078826424055226265035 * erfcx(-c * 0.7071067811865475244008443621048490392848);
    const double q = 1.0 + c * mills;
    log_h = log_phi + log(q);
    lambda = mills / q;
    kappa = 1.0 / q;
    return;
  }
  const double a = -c;
  double t2 = a;
  for (int k = kLogEiFractionTerms; k >= 2; --k) t2 = a + (double)k / t2;
  const double t1 = a + 1.0 / t2;
  const double tt = t1 * t2;
  log_h = log_phi - log(tt);
  lambda = t2;
  kappa = tt;
}

// log Phi(z) and r = phi(z) / Phi(z), finite for every finite z: through erfcx below 0 (gibbon1.hip's ratio), directly above.
__device__ __forceinline__ void log_cdf_parts(double z, double& log_cdf, double& ratio) {
  const double r2 = 0.7071067811865475244008443621048490392848;
  if (z < 0.0) {
    const double e = erfcx(-z * r2);
    log_cdf = -0.5 * z * z + log(0.5 * e);
    ratio = 0.7978845608028653558798921198687637369517 / e;
    return;
  }
  const double q = 0.5 * erfc(z * r2);
  log_cdf = log1p(-q);
  ratio = normal_pdf(z) / (1.0 - q);
}

// ss + sum of v_r^2 over the rows r0 <= r < r1 as ONE fused multiply-add chain in row order, for a whole wavefront: the lanes load
// 64 rows at a time and every lane runs the whole chain on the broadcast entries, so every lane returns the same bits; rows past
// r1 add exact zeros.  A chain carried on over a second range (gibbon1.hip taps it after the member's own rows) is two calls.
__device__ __forceinline__ double row_chain(const double* __restrict__ v, int r0, int r1, int lane, double ss) {
  for (int r = r0; r < r1; r += 64) {
    const double x = (r + lane < r1) ? v[r + lane] : 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const double xi = __shfl(x, i, 64);
      ss = fma(xi, xi, ss);
    }
  }
  return ss;
}

}  // namespace moe
