// cornell_moe_amd/csrc/logcei1.hip -- the LOG of the constrained expected improvement averaged over a hyper-parameter ensemble
// (Ament, Daulton, Eriksson, Balandat & Bakshy, "Unexpected improvements to expected improvement", NeurIPS 2023), with pending
// points, its multistart ascent and greedy q-point batches, on the device (moe_log_ei_constrained_mcmc,
// moe_log_ei_constrained_mcmc_multistart, moe_log_ei_constrained_mcmc_suggest): the sixth client of kg1_ascent.hip's staging, ascent
// and drivers.  The members, their pass, the gradient's tail and the believed-feasible incumbent are cei1.hip's and ei1.hip's
// (cei1.hpp, ei1.hpp); this file keeps the candidate kernel with its two roles, the combine kernel and the description of the call.
//
// Why.  cei1.hip's factors are Phi and phi in float64: from c = (b' - mu) / sigma below about -38 both are exactly 0, every start of
// an ascent ties at 0 with a zero gradient, and one constraint whose Phi(z) underflows zeroes the whole product.  The log of the
// same quantity is finite with a useful gradient for every finite input.
//
// A call is cei1.hip's: E joint hyper-samples, K constraints (0 <= K <= 8), the E (1 + K) GPs the sub-members of one Kg1Ensemble
// ordered [e][role], every GP's covariance conditioned on the pending points.  With var the conditioned latent variance of the
// sub-member at x and ONE floor for value and gradient, sigma = sqrt(max(150 eps^2, var)) (the value's DBL_MIN floor would let c^2
// overflow at a sampled point of a noise-free GP; with the gradient's the value is finite and the gradient is the value's wherever
// var lies above the floor):
//   role 0   t = b'_e - mu(x), c = t / sigma, h(c) = c Phi(c) + phi(c):   l = log sigma + log h(c)
//            grad l = -(lambda / sigma) grad mu + (kappa / (2 sigma^2)) grad var,  lambda = Phi(c) / h(c), kappa = phi(c) / h(c)
//            b'_e = +infinity: l = 0 and a zero gradient (cei1.hip's factor 1)
//   role k   z = (tau_k - mu(x)) / sigma:   l = log Phi(z),  r = phi(z) / Phi(z)
//            grad l = -(r / sigma) grad mu - (r z / (2 sigma^2)) grad var
// -- ei1.hip's gradient form, grad = -s grad mu + (w / 2) grad var, with (s, w) = (lambda / sigma, kappa / sigma^2) and
// (r / sigma, -r z / sigma^2): the candidate kernel leaves s in dScal and the column w v'_x in dT, ei1_grad_tail serves.  The scalars
// are acq1_device.hpp's log_h_parts and log_cdf_parts; none of them is the log of a float64 Phi or phi that could have underflowed.
//   L_e = l_{e,0} + l_{e,1} + ... + l_{e,K},  g_e = grad l_{e,0} + ... + grad l_{e,K}       added in the order objective, k = 1 .. K
//   m = max_e L_e,  w_e = exp(L_e - m),  W = w_0 + ... + w_{E-1}                             members in member order
//   value = m + log W - log E,   grad = (w_0 g_0 + ... + w_{E-1} g_{E-1}) / W
// every operation rounded by itself, no atomics (logcei1_combine_kernel, in the place of kg1_ascent.hip's mean of the members, at
// K = 0 too: Kg1Objective::combine_single_groups).  With E = 1, K = 0 that is the member's own l and gradient bit for bit (w = 1, W = 1,
// log 1 = 0).  The members' own values of an evaluation are the sub-members' l [E (1 + K)][C].
//
// Bits.  The variance is ei1_cand_kernel's ONE fused multiply-add chain over the rows in order; a candidate's bits do not depend on
// who shares its pass, on want_grad or on ensemble-wide launches.  A candidate never raises; only a pending point whose Schur pivot
// fails does, payload (the flat index e (1 + K) + role of the GP, the pending point).
#include <algorithm>
#include <cmath>

#include "acq1_device.hpp"
#include "cei1.hpp"
#include "device_cov.hpp"
#include "ei1.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

// One wavefront per candidate: ei1_cand_kernel's chain for the variance (row_chain), then the scalars of the sub-member's role,
// the same in every lane (twenty divisions beside the 2 N^2 of the triangular products; lane 0 writes them).  *best is b' (role 0)
// or tau_k (role k); val_out takes l, and with want_grad s_out the scalar s and T the column w v'_x.
struct logcei1_cand_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int R, int ld, int ncols, int col0, const CovParams& cp, int want_grad, int role, const double* __restrict__ best, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ s_out, double* __restrict__ T) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const double* v = Vx + (size_t)c * ld;
    const double ss = row_chain(v, 0, R, lane, 0.0);
    const double var = radial_scalars(cp.type, cp.alpha, 0.0).base - ss;
    const double b = *best;
    double* tc = T + (size_t)c * ld;
    if (role == 0 && b == INFINITY) {  // no feasible incumbent: the improvement factor is 1, its log 0, and does not move
      if (lane == 0) val_out[col0 + c] = 0.0;
      if (want_grad == 0) return;
      if (lane == 0) s_out[c] = 0.0;
      for (int r = lane; r < R; r += 64) tc[r] = 0.0;
      return;
    }
    const double sigma = sqrt(fmax(kMinVarGradEI, var));
    const double cc = (b - mu[c]) / sigma;
    double l, s, w;
    if (role == 0) {
      double log_h, lambda, kappa;
      log_h_parts(cc, log_h, lambda, kappa);
      l = log(sigma) + log_h;
      s = lambda / sigma;
      w = kappa / (sigma * sigma);
    } else {
      double ratio;
      log_cdf_parts(cc, l, ratio);
      s = ratio / sigma;
      w = -(ratio * cc) / (sigma * sigma);
    }
    if (lane == 0) val_out[col0 + c] = l;
    if (want_grad == 0) return;
    if (lane == 0) s_out[c] = s;
    for (int r = lane; r < R; r += 64) tc[r] = w * v[r];
  }
};
__global__ __launch_bounds__(256) void logcei1_cand_kernel(int R, int ld, int ncols, int col0, const CovParams cp, int want_grad, int role, const double* __restrict__ best, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ s_out, double* __restrict__ T) {
  logcei1_cand_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, R, ld, ncols, col0, cp, want_grad, role, best, mu, Vx, val_out, s_out, T);
}

// candidate c's L_e: member e's G logs added in the order objective, k = 1 .. K
__device__ __forceinline__ double logcei1_member_log(const double* const* __restrict__ f, int G, long c) {
#pragma clang fp contract(off)
  double L = f[0][c];
  for (int q = 1; q < G; ++q) L = L + f[q][c];
  return L;
}

// The log-sum-exp over the members, one thread per output element.  vals / grads: the E G sub-members' logs [C] and gradients
// [C][d], ordered [e][role].  Element i < nv of value_out (NULL: nv = 0) is candidate i's value; the elements behind are grad_out's
// (c, j).  Every sum in the header's order, each operation rounded by itself.  A thread works out every member's L_e twice (once
// for the maximum, once for the weights) and each of a candidate's d gradient threads repeats its whole log-sum-exp: deliberate --
// nothing is kept between threads, so no scratch, no barrier and no second launch, and E (1 + K) loads and E exponentials per
// element are small beside the members' chains (0.17 ms of a 15.6 ms suggestion at K = 0).
__global__ __launch_bounds__(256) void logcei1_combine_kernel(int E, int G, long C, int d, const double* const* __restrict__ vals, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  const long k = i - nv, c = (i < nv) ? i : k / d;
  double m = logcei1_member_log(vals, G, c);
  for (int e = 1; e < E; ++e) m = fmax(m, logcei1_member_log(vals + (size_t)e * G, G, c));
  double W = 0.0, sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double w = exp(logcei1_member_log(vals + (size_t)e * G, G, c) - m);
    W = (e == 0) ? w : W + w;
    if (i < nv) continue;
    double g = grads[(size_t)e * G][k];
    for (int q = 1; q < G; ++q) g = g + grads[(size_t)e * G + q][k];
    const double term = w * g;
    sum = (e == 0) ? term : sum + term;
  }
  if (i < nv)
    value_out[i] = m + log(W) - log((double)E);
  else
    grad_out[k] = sum / W;
}

// ei1.hip's pass with logcei1_cand_kernel in the place of ei1_cand_kernel (dScal holds s)
void cand_step(const Kg1Member& m, int nc, int c0, bool with_grad, hipStream_t s) {
  launch_kernel_ens<logcei1_cand_kernel_body, 256>(logcei1_cand_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, m.gp->N + m.p, m.ld,
                                                   nc, c0, m.gp->cp, with_grad ? 1 : 0, m.role, (const double*)m.dBp,
                                                   (const double*)m.dMuh, (const double*)m.dVx, m.dKg, m.dScal, m.dT);
}

void logcei1_eval_points(const Kg1Member& m, const double* Px, const double*, int C, bool with_grad, hipStream_t s) {
  ei1_eval_passes(m, Px, C, with_grad, s, "logcei1_eval_pass", cand_step, ei1_grad_tail);
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  const long n = (value_out != nullptr ? (long)C : 0) + (grad_out != nullptr ? (long)C * T.d : 0);
  if (n == 0) return;
  MOE_LAUNCH_NOW(logcei1_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, T.E / T.group, T.group, (long)C, T.d,
                 T.dKgTab, T.dGradTab, value_out, grad_out);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

// cei1_call's description with the log kernels and the log-sum-exp, taken at K = 0 too.  The call keeps the sub-members' limits
// [E (1 + K)].
Kg1Call logcei1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* best_so_far) {
  const int E = num_mcmc, K = num_constraints;
  Kg1Call call;
  call.doubles.resize((size_t)E * (1 + K));
  for (int e = 0; e < E; ++e) {
    call.doubles[(size_t)e * (1 + K)] = best_so_far[e];
    for (int k = 0; k < K; ++k) call.doubles[(size_t)e * (1 + K) + 1 + k] = thresholds[k];
  }
  call.o.best_so_far = call.doubles.data();
  call.o.member = cei1_member;
  call.o.eval_points = logcei1_eval_points;
  call.o.all_extended = cei1_all_extended;
  call.o.pick_appended = cei1_pick_appended;
  call.o.group = 1 + K;
  call.o.combine = combine;
  call.o.combine_single_groups = true;
  call.check_members = ei1_check_members;
  return call;
}

}  // namespace moe
