// cornell_moe_amd/csrc/logehvi1.hpp -- what the two log forms of the expected hypervolume improvement share (logehvi1.hip: two
// objectives, the strips of a front; logehvi3.hip: three objectives, the boxes of a table): the log-sum-exp record with its take and
// merge rules, templated on the number of weighted derivative sums (4 or 6), the log-feasibility kernel over groups of M + K
// sub-members and a member's LL_e.  Device code only; every unit that includes it compiles its own copy of the kernel.
#pragma once
#include <cmath>

#include "acq1_device.hpp"
#include "cehvi1.hpp"

namespace moe {

namespace {

// a thread's log-sum-exp over the terms it has seen: their maximum, the weights' sum and the N weighted derivative sums
template <int N>
struct LogStripRecord {
  double m, W, S[N];
};

// the record takes a term of log l with derivatives dl: a term above the maximum rescales (W, S) by exp(m - l) and enters with
// weight 1, one at or below it enters with weight exp(l - m)
template <int N>
__device__ __forceinline__ void record_take(LogStripRecord<N>& a, double l, const double* dl, bool wg) {
#pragma clang fp contract(off)
  if (l > a.m) {
    const double sc = exp(a.m - l);  // (exp(-infinity) = 0 for the first term, W and S being 0)
    a.W = a.W * sc + 1.0;
    if (wg) {
#pragma unroll
      for (int q = 0; q < N; ++q) a.S[q] = a.S[q] * sc + dl[q];
    }
    a.m = l;
  } else {
    const double w = exp(l - a.m);
    a.W = a.W + w;
    if (wg) {
#pragma unroll
      for (int q = 0; q < N; ++q) a.S[q] = a.S[q] + w * dl[q];
    }
  }
}

// a becomes the merge of a and b: the merged maximum is the larger one, the two records are scaled by exp(m_a - m) and exp(m_b - m),
// multiplied out first and then added (a and b exchanged give the same bits); a record that holds no term (m = -infinity) yields
// to the other
template <int N>
__device__ __forceinline__ void record_join(LogStripRecord<N>& a, const LogStripRecord<N>& b, bool wg) {
#pragma clang fp contract(off)
  if (b.m == -INFINITY) return;
  if (a.m == -INFINITY) {
    a = b;
    return;
  }
  const double m = fmax(a.m, b.m);
  const double ea = exp(a.m - m), eb = exp(b.m - m);
  const double wa = a.W * ea, wb = b.W * eb;
  a.W = wa + wb;
  if (wg) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const double sa = a.S[q] * ea, sb = b.S[q] * eb;
      a.S[q] = sa + sb;
    }
  }
  a.m = m;
}

// one butterfly step: the lane's record and its partner's become their merge, the same bits in both lanes
template <int N>
__device__ __forceinline__ void record_merge(LogStripRecord<N>& a, int off, bool wg) {
  LogStripRecord<N> b;
  b.m = __shfl_xor(a.m, off, 64);
  b.W = __shfl_xor(a.W, off, 64);
#pragma unroll
  for (int q = 0; q < N; ++q) b.S[q] = __shfl_xor(a.S[q], off, 64);
  record_join(a, b, wg);
}

// One thread per (member, constraint, candidate): log F and, with want_grad, its derivatives by mu and var (logehvi1.hip's header
// forms) from the constraint sub-member's [mu Cs | var Cs].  kg: the E (M + K) sub-members'; feas [E][K][Cs][3].
__global__ __launch_bounds__(256) void logehvi1_feas_kernel(const double* const* __restrict__ kg, int E, int M, int K, const CehviTau tau, int C, int Cs, int want_grad, double* __restrict__ feas) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)E * K * C) return;
  const int c = (int)(i % C);
  const int ek = (int)(i / C), k = ek % K, e = ek / K;
  const double* src = kg[(size_t)e * (M + K) + M + k];
  const double mu = src[c], var = src[(size_t)Cs + c];
  const double sigma = sqrt(fmax(kMinVarGradEI, var));
  const double z = (tau.t[k] - mu) / sigma;
  double l, ratio;
  log_cdf_parts(z, l, ratio);
  double* out = feas + 3 * ((size_t)ek * Cs + c);
  out[0] = l;
  if (want_grad == 0) return;
  out[1] = -(ratio / sigma);
  out[2] = -(ratio * z) / (2.0 * (sigma * sigma));
}

// candidate c's LL_e: L_e and the K log feasibilities added in the order k = 1 .. K
__device__ __forceinline__ double logehvi1_member_log(const double* __restrict__ hv, const double* __restrict__ feas, int e, int K, int Cs, long c) {
#pragma clang fp contract(off)
  double L = hv[(size_t)e * Cs + c];
  for (int k = 0; k < K; ++k) L = L + feas[3 * (((size_t)e * K + k) * Cs + c)];
  return L;
}

}  // namespace

}  // namespace moe
