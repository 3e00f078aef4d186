// cornell_moe_amd/csrc/gibbon1.hip -- the min-value entropy acquisition GIBBON (Moss, Leslie, Gonzalez & Rayson, JMLR 2021: the
// max-value entropy search of Wang & Jegelka 2017 made right under observation noise and for batches), for minimisation, averaged over
// a hyper-parameter ensemble, with pending points, its multistart ascent and greedy q-point batches, on the device (moe_gibbon_mcmc,
// moe_gibbon_mcmc_multistart, moe_gibbon_mcmc_suggest): a client of kg1_ascent.hip's staging, ascent and drivers.  The pending-row
// extension is kg1_pending.hip's, the member's layout, the members' check, the pass and the gradient's tail are ei1.hip's (ei1.hpp);
// this file keeps the candidate kernel and the description of the call (gibbon1_call).
//
// Member e: posterior mean mu, noise sigma^2 = noise_variance[0], K samples m_k of the global minimum VALUE (the caller's), pending
// points P (the member's noise on P's diagonal, the mean left alone; 1 + g rows per point under derivative observations).  With
// v_x = L^-1 k(X, x) and r_x the extension's rows under it:
//   var0 = k(x, x) - |v_x|^2 (latent, unconditioned),  varc = var0 - |r_x|^2 (conditioned on P),  s0 = max(DBL_MIN, var0), sc likewise
//   sigma0 = sqrt(s0),  rho^2 = s0 / (s0 + sigma^2),  gamma_k = (mu(x) - m_k) / sigma0
//   r(gamma) = phi(gamma) / Phi(gamma) = sqrt(2 / pi) / erfcx(-gamma / sqrt 2)            (one expression for every gamma)
//   q_k = clamp(r_k (gamma_k + r_k), 0, 1),   G_k = -1/2 log1p(-min(rho^2 q_k, 1 - DBL_EPSILON))
//   alpha_e(x) = [p > 0] 1/2 (log(sc + sigma^2) - log(s0 + sigma^2)) + (1 / K) sum_k G_k
// 1 - rho^2 q is Var(y | f >= m) / Var(y) of the noisy observation y = f + eps: G_k is the information the event "the minimum is m_k"
// carries about y (GIBBON's moment-matched lower bound).  The bracket is the exact greedy increment of GIBBON's batch term 1/2 log
// |R_B|, R the correlation matrix of the batch's noisy predictive outputs: |R_{B u x}| / |R_B| is the Schur complement of x over its
// marginal, (varc + sigma^2) / (var0 + sigma^2).  It tends to -infinity at a noise-free pick, so a greedy batch never re-picks.
//
// Gradient (P and m do not move with x; unclamped like EI's), with s0g = max(150 eps^2, var0), scg likewise, in every denominator
// and in the gamma and rho^2 of the derivative factors:
//   dG/dgamma = 1/2 rho^2 (r - q (gamma + 2 r)) / (1 - rho^2 q),   dG/drho^2 = 1/2 q / (1 - rho^2 q)       (r' = -q)
//   A  = (1 / K) sum_k dG/dgamma_k / sigma0g
//   B0 = -[p > 0] / (2 (s0g + sigma^2)) + (1 / K) sum_k [-gamma_k dG/dgamma_k / (2 s0g) + dG/drho^2_k sigma^2 / (s0g + sigma^2)^2]
//   Bc = [p > 0] / (2 (scg + sigma^2))
//   grad alpha = A grad mu + B0 grad var0 + Bc grad varc
// grad var0 = -2 sum_{rows X} (L^-T v_x)_r grad_x k(X_r, x), grad varc = -2 sum_{rows X u P} (L'^-T [v_x ; r_x])_r grad_x k(row_r, x),
// and L'^-T [a ; 0] = [L^-T a ; 0] (L' = [[L, 0], [B, L_P]]: the pending block of the solution is L_P^-T 0 = 0), so both ride ONE column:
//   grad alpha = sum_r coef_r grad_x k(row_r, x),  coef_r = A [K^-1 (y - mean) ; 0]_r - (L'^-T [2 (B0 + Bc) v_x ; 2 Bc r_x])_r
// -- EI's coefficient with -A where EI has Phi(c_g) and this column where EI has (phi(c_g) / sigma_g) v'_x: ei1_grad_tail serves.
//
// Per pass of ei1_pass_size(N) candidates (recordable; nothing waits): launch_cov_build, tri_cols ('N'), launch_mean,
// kg1_pending_rows (p > 0), gibbon1_cand_kernel, ei1_grad_tail.  There is no believed best: nothing follows the extension.
//
// Bits.  The variance is ONE fused multiply-add chain over the member's rows in row order (tapped: var0) and then the extension's
// rows (tapped: varc): at p = 0 var0 is ei1_cand_kernel's var bit for bit.  Lane l adds the terms k = l, l + 64, ... in order, then a
// fixed butterfly over the 64 lanes; lanes past K add exact zeros.  A candidate's bits do not depend on who shares its pass, on
// want_grad or on ensemble-wide launches.  A candidate never raises; only a pending point whose Schur pivot fails does.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "device_cov.hpp"
#include "ei1.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

// r = phi / Phi at gamma and q = clamp(r (gamma + r), 0, 1).  erfcx overflows to +infinity from gamma ~ 37 on: r = q = 0 exactly.
__device__ __forceinline__ void gibbon1_ratio(double gamma, double& r, double& q) {
  r = 0.7978845608028653558798921198687637369517 / erfcx(-gamma * 0.7071067811865475244008443621048490392848);
  q = fmin(1.0, fmax(0.0, r * (gamma + r)));
}

// One wavefront per candidate.  The chain over the rows is ei1_cand_kernel's (row_chain; rows past a part's end add exact zeros),
// run over the member's N rows, tapped, and carried on over the extension's rows.  Then the K terms: lane l takes k = l, l + 64,
// ..., the four running sums go through one butterfly, lane 0 writes the value and -A, all lanes write the column
// [2 (B0 + Bc) v_x ; 2 Bc r_x].
struct gibbon1_cand_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int R, int ld, int ncols, int col0, const CovParams& cp, int want_grad, double noise, int K, const double* __restrict__ mins, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ na_out, double* __restrict__ T) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const double* v = Vx + (size_t)c * ld;
    double ss = row_chain(v, 0, N, lane, 0.0);
    const double base = radial_scalars(cp.type, cp.alpha, 0.0).base;
    const double var0 = base - ss;
    ss = row_chain(v, N, R, lane, ss);
    const double varc = base - ss;
    const bool pending = R > N;
    const double s0 = fmax(kMinVarEI, var0), sc = fmax(kMinVarEI, varc);
    const double s0g = fmax(kMinVarGradEI, var0), scg = fmax(kMinVarGradEI, varc);
    const double sigma0 = sqrt(s0), rho2 = s0 / (s0 + noise);
    const double sigma0g = sqrt(s0g), rho2g = s0g / (s0g + noise);
    const bool floored = s0g != s0;  // (the gradient's factors then take their own gamma and rho^2)
    const double m = mu[c];
    double sG = 0.0, sDg = 0.0, sGDg = 0.0, sDr = 0.0;
    for (int k = lane; k < K; k += 64) {
      const double t = m - mins[k];
      double gamma = t / sigma0, r, q;
      gibbon1_ratio(gamma, r, q);
      double z = fmin(rho2 * q, 1.0 - DBL_EPSILON);
      sG += -0.5 * log1p(-z);
      if (want_grad != 0) {
        if (floored) {
          gamma = t / sigma0g;
          gibbon1_ratio(gamma, r, q);
          z = fmin(rho2g * q, 1.0 - DBL_EPSILON);
        }
        const double dg = 0.5 * rho2g * (r - q * (gamma + 2.0 * r)) / (1.0 - z);
        sDg += dg;
        sGDg = fma(gamma, dg, sGDg);
        sDr += 0.5 * q / (1.0 - z);
      }
    }
  #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sG += __shfl_xor(sG, off, 64);
      sDg += __shfl_xor(sDg, off, 64);
      sGDg += __shfl_xor(sGDg, off, 64);
      sDr += __shfl_xor(sDr, off, 64);
    }
    const double nK = (double)K;
    if (lane == 0) {
      double value = sG / nK;
      if (pending) value = 0.5 * (log(sc + noise) - log(s0 + noise)) + value;
      val_out[col0 + c] = value;
    }
    if (want_grad == 0) return;
    const double a = (sDg / nK) / sigma0g;
    const double t0 = s0g + noise;
    double b0 = (-sGDg / (2.0 * s0g) + sDr * (noise / (t0 * t0))) / nK, bc = 0.0;
    if (pending) {
      b0 = -1.0 / (2.0 * t0) + b0;
      bc = 1.0 / (2.0 * (scg + noise));
    }
    if (lane == 0) na_out[c] = -a;
    const double w0 = 2.0 * (b0 + bc), wc = 2.0 * bc;
    double* tc = T + (size_t)c * ld;
    for (int r = lane; r < R; r += 64) tc[r] = (r < N ? w0 : wc) * v[r];
  }
};
__global__ __launch_bounds__(256) void gibbon1_cand_kernel(int N, int R, int ld, int ncols, int col0, const CovParams cp, int want_grad, double noise, int K, const double* __restrict__ mins, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ na_out, double* __restrict__ T) {
  gibbon1_cand_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, R, ld, ncols, col0, cp, want_grad, noise, K, mins, mu, Vx, val_out, na_out, T);
}

// ei1.hip's pass with gibbon1_cand_kernel in the place of ei1_cand_kernel (dScal holds -A)
void cand_step(const Kg1Member& m, int nc, int c0, bool with_grad, hipStream_t s) {
  const GpDev& gp = *m.gp;
  launch_kernel_ens<gibbon1_cand_kernel_body, 256>(gibbon1_cand_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, gp.N, gp.N + m.p,
                                                   m.ld, nc, c0, gp.cp, with_grad ? 1 : 0, gp.noise[0], m.nExtra, m.dExtra,
                                                   (const double*)m.dMuh, (const double*)m.dVx, m.dKg, m.dScal, m.dT);
}

void gibbon1_eval_points(const Kg1Member& m, const double* Px, const double*, int C, bool with_grad, hipStream_t s) {
  if (C > 0 && (m.dExtra == nullptr || m.nExtra < 1))  // (the staging has not laid out the member's min-values)
    throw Error(MOE_ERR_RUNTIME, "gibbon1_eval_pass: the pass does not fit the member's buffers");
  ei1_eval_passes(m, Px, C, with_grad, s, "gibbon1_eval_pass", cand_step, ei1_grad_tail);
}

// EI's layout (an empty set, no best value); the staging adds the address of the member's min-values (Kg1Member::dExtra)
Kg1Member member(const Kg1Objective&, GpDev& gp, int, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  return ei1_member(gp, C, 0.0, with_grad, fail, pcap * (1 + gp.g), fail_pending);  // (pcap points: 1 + g rows each)
}

// a pick joins every member's extension, inside device memory; the min-values stay as they are over the batch
void pick_appended(Kg1Ensemble& T) {
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
}

}  // namespace

// No sets, no fidelity coordinates and no believed best: the upload is [value pointers E | grad pointers E | bounds 2 d | points
// C dp | pending points pcap dp | min-values E K].
Kg1Call gibbon1_call(const double* min_values, int num_min_values) {
  Kg1Call call;
  call.o.member = member;
  call.o.eval_points = gibbon1_eval_points;
  call.o.pick_appended = pick_appended;
  call.o.member_extra = min_values;
  call.o.num_member_extra = num_min_values;
  call.check_members = ei1_check_members;
  return call;
}

void check_gibbon_min_values(const double* min_values, int num_mcmc, int num_min_values) {
  if (num_min_values < 1 || num_min_values > kGibbonMaxMinValues)
    throw Error(MOE_ERR_BOUNDS, "num_min_values must be between 1 and 1024", num_min_values, 1, kGibbonMaxMinValues);
  for (int e = 0; e < num_mcmc; ++e)
    for (int k = 0; k < num_min_values; ++k) {
      const double v = min_values[(size_t)e * num_min_values + k];
      if (!std::isfinite(v)) throw Error(MOE_ERR_INVALID_VALUE, "min_values must be finite", v, e, k);
    }
}

}  // namespace moe
