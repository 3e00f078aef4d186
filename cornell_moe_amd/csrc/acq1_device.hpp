// cornell_moe_amd/csrc/acq1_device.hpp -- the device pieces the candidate kernels of the one-point acquisitions share (ei1.hip,
// gibbon1.hip, cei1.hip, ehvi1.hip; kg1.hip takes the density): one definition each, inlined into every kernel that uses it.
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
