// cornell_moe_amd/csrc/cei1.hip -- the constrained expected improvement (expected improvement times the probability of feasibility:
// Schonlau, Welch & Jones 1998; Gardner et al. 2014; Gelbart, Snoek & Adams 2014) averaged over a hyper-parameter ensemble, with
// pending points, its multistart ascent and greedy q-point batches, on the device (moe_ei_constrained_mcmc,
// moe_ei_constrained_mcmc_multistart, moe_ei_constrained_mcmc_suggest): a client of kg1_ascent.hip's staging, ascent and drivers.
// The pending-row extension is kg1_pending.hip's, the layout, the members' check, the pass and the gradient's tail are ei1.hip's
// (ei1.hpp); this file keeps the candidate kernel with its two roles, the combine kernel, the believed-feasible incumbent and the
// description of the call (cei1_call).  The sub-member's layout and the incumbent's hooks are lent to logcei1.hip (cei1.hpp).
//
// A call takes E joint hyper-samples and K constraints, 0 <= K <= 8.  Member e is 1 + K GPs: the objective GP and the constraint GPs
// c_1 .. c_K, constraint k satisfied where c_k(x) <= tau_k.  The E (1 + K) GPs are the SUB-MEMBERS of one Kg1Ensemble, ordered
// [e][role] (role 0: the objective): each runs ei1.hip's chain and leaves its factor and that factor's gradient in its own dKg / dGrad.
// Every GP's covariance is conditioned on the pending points P as in ei1.hip (its own noise on P's diagonal, the mean left alone,
// 1 + g rows per point under derivative observations).  With var the conditioned latent variance of the sub-member at x,
// sigma = sqrt(max(DBL_MIN, var)), sigma_g = sqrt(max(150 eps^2, var)):
//   role 0   t = b'_e - mu(x):   EI = max(0, t Phi(t / sigma) + sigma phi(t / sigma)),  grad as in ei1.hip;
//            b'_e = +infinity ("no feasible observation yet"): the factor is exactly 1 and its gradient 0
//   role k   t = tau_k - mu(x):  F = Phi(z), z = t / sigma;  z_g = t / sigma_g,
//            grad F = -(phi(z_g) / sigma_g) grad mu - (phi(z_g) z_g / (2 sigma_g^2)) grad var
// -- ei1.hip's gradient form, grad = -s grad mu + (w / 2) grad var, with (s, w) = (phi(z_g) / sigma_g, -phi(z_g) z_g / sigma_g^2)
// where EI has (Phi(c_g), phi(c_g) / sigma_g): the candidate kernel leaves s in dScal and the column w v'_x in dT, ei1_grad_tail serves.
//   b'_e = min(b_e, min over the believed-feasible pending points j of mu_{e,0}(P_j)),
//   P_j believed feasible under member e when mu_{e,k}(P_j) <= tau_k for every k
// (a believed-infeasible pick must not lower the incumbent, and without the join a greedy batch re-picks its own point).
//   A_e = EI_e F_{e,1} ... F_{e,K}                       multiplied left to right
//   grad A_e = sum_r (prod_{q != r} f_q) grad f_r        each excluded product by the same multiplication with its factor skipped,
//                                                        the terms added in the order objective, k = 1 .. K
//   value = (A_0 + ... + A_{E-1}) / E, the gradient likewise: members added in member order and divided once, no contraction
// (cei1_combine_kernel, in the place of kg1_ascent.hip's mean of the members).  With K = 0 there is one GP per member, the drivers
// take the mean of the members as they always did, and the call is moe_ei_analytic_mcmc bit for bit while every b_e is finite.
//
// Bits.  The variance is ei1_cand_kernel's ONE fused multiply-add chain over the rows in order; a candidate's bits do not depend on
// who shares its pass, on want_grad or on ensemble-wide launches.  A candidate never raises; only a pending point whose Schur pivot
// fails does, payload (the flat index e (1 + K) + role of the GP, the pending point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "cei1.hpp"
#include "device_cov.hpp"
#include "ei1.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

// One wavefront per candidate: ei1_cand_kernel's chain for the variance (row_chain), then the scalars of the sub-member's role.
// *best is b' (role 0) or tau_k (role k); val_out takes the factor, and with want_grad s_out the scalar s and T the column w v'_x.
struct cei1_cand_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int R, int ld, int ncols, int col0, const CovParams& cp, int want_grad, int role, const double* __restrict__ best, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ s_out, double* __restrict__ T) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const double* v = Vx + (size_t)c * ld;
    const double ss = row_chain(v, 0, R, lane, 0.0);
    const double var = radial_scalars(cp.type, cp.alpha, 0.0).base - ss;
    const double b = *best;
    double* tc = T + (size_t)c * ld;
    if (role == 0 && b == INFINITY) {  // no feasible incumbent: the improvement factor is 1 and does not move
      if (lane == 0) val_out[col0 + c] = 1.0;
      if (want_grad == 0) return;
      if (lane == 0) s_out[c] = 0.0;
      for (int r = lane; r < R; r += 64) tc[r] = 0.0;
      return;
    }
    const double t = b - mu[c];
    if (lane == 0) {
      const double sigma = sqrt(fmax(kMinVarEI, var));
      const double cc = t / sigma;
      if (role == 0)
        val_out[col0 + c] = fmax(0.0, t * normal_cdf(cc) + sigma * normal_pdf(cc));
      else
        val_out[col0 + c] = normal_cdf(cc);
    }
    if (want_grad == 0) return;
    const double sg = sqrt(fmax(kMinVarGradEI, var));
    const double cg = t / sg;
    const double pg = normal_pdf(cg) / sg;
    double w;
    if (role == 0) {
      w = pg;
      if (lane == 0) s_out[c] = normal_cdf(cg);
    } else {
      w = -(pg * cg) / sg;
      if (lane == 0) s_out[c] = pg;
    }
    for (int r = lane; r < R; r += 64) tc[r] = w * v[r];
  }
};
__global__ __launch_bounds__(256) void cei1_cand_kernel(int R, int ld, int ncols, int col0, const CovParams cp, int want_grad, int role, const double* __restrict__ best, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ s_out, double* __restrict__ T) {
  cei1_cand_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, R, ld, ncols, col0, cp, want_grad, role, best, mu, Vx, val_out, s_out, T);
}

// The product rule and the ensemble mean, one thread per output element.  vals / grads: the E G sub-members' factor values [C] and
// gradients [C][d], ordered [e][role].  Element i < nv of value_out (NULL: nv = 0) is candidate i's value; the elements behind are
// grad_out's (c, j).  Every product and sum in the header's order, each operation rounded by itself.
__global__ __launch_bounds__(256) void cei1_combine_kernel(int E, int G, long C, int d, const double* const* __restrict__ vals, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  if (i < nv) {
    double sum = 0.0;
    for (int e = 0; e < E; ++e) {
      double a = vals[(size_t)e * G][i];
      for (int q = 1; q < G; ++q) a = a * vals[(size_t)e * G + q][i];
      sum = (e == 0) ? a : sum + a;
    }
    value_out[i] = sum / (double)E;
    return;
  }
  const long k = i - nv, c = k / d;
  double sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double* const* f = vals + (size_t)e * G;
    double a = 0.0;
    for (int r = 0; r < G; ++r) {
      double ex = 1.0;
      bool started = false;
      for (int q = 0; q < G; ++q) {
        if (q == r) continue;
        const double fq = f[q][c];
        ex = started ? ex * fq : fq;
        started = true;
      }
      const double term = ex * grads[(size_t)e * G + r][k];
      a = (r == 0) ? term : a + term;
    }
    sum = (e == 0) ? a : sum + a;
  }
  grad_out[k] = sum / (double)E;
}

// One member's believed-feasible incumbent and its constraints' thresholds in device memory.  mu[r]: mu_{e,r} at `count` pending
// points; lim[r]: b_e (r = 0) and tau_r; out[r]: the sub-members' dBp.  first != 0: b_e is the incumbent as it stands and the
// thresholds are written; otherwise the incumbent so far is out[0]'s (a greedy batch's next pick joins).
struct Cei1Best {
  const double* mu[1 + kCeiMaxConstraints];
  double* out[1 + kCeiMaxConstraints];
  double lim[1 + kCeiMaxConstraints];
};
__global__ void cei1_best_kernel(Cei1Best a, int G, int first, int count) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double v = first != 0 ? a.lim[0] : *a.out[0];
  for (int j = 0; j < count; ++j) {
    bool feasible = true;
    for (int r = 1; r < G; ++r) feasible = feasible && (a.mu[r][j] <= a.lim[r]);
    if (feasible) v = fmin(v, a.mu[0][j]);
  }
  *a.out[0] = v;
  if (first != 0)
    for (int r = 1; r < G; ++r) *a.out[r] = a.lim[r];
}

// ei1.hip's pass with cei1_cand_kernel in the place of ei1_cand_kernel (dScal holds s)
void cand_step(const Kg1Member& m, int nc, int c0, bool with_grad, hipStream_t s) {
  launch_kernel_ens<cei1_cand_kernel_body, 256>(cei1_cand_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, m.gp->N + m.p, m.ld, nc,
                                                c0, m.gp->cp, with_grad ? 1 : 0, m.role, (const double*)m.dBp, (const double*)m.dMuh,
                                                (const double*)m.dVx, m.dKg, m.dScal, m.dT);
}

void cei1_eval_points(const Kg1Member& m, const double* Px, const double*, int C, bool with_grad, hipStream_t s) {
  ei1_eval_passes(m, Px, C, with_grad, s, "cei1_eval_pass", cand_step, ei1_grad_tail);
}

}  // namespace

// mu of every sub-member at P_j0 .. j0 + count - 1 (the function values alone), then every member's believed-feasible incumbent
void cei1_join_believed_feasible(Kg1Ensemble& T, int j0, int count, bool first) {
  const int G = std::max(T.group, 1);
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  for (int e = 0; e < T.E; e += G) {
    Cei1Best a = {};
    for (int r = 0; r < G; ++r) {
      a.mu[r] = T.mem[e + r].dAA;
      a.out[r] = T.mem[e + r].dBp;
      a.lim[r] = T.mem[e + r].best;
    }
    MOE_LAUNCH_NOW(cei1_best_kernel, dim3(1), dim3(64), 0, T.z, a, G, first ? 1 : 0, count);
  }
  MOE_HIP_CHECK(hipGetLastError());
}

// EI's layout; o.best_so_far holds the sub-members' limits [E G]: b_e for role 0, tau_k for role k
Kg1Member cei1_member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  Kg1Member m = ei1_member(gp, C, o.best_so_far[e], with_grad, fail, pcap * (1 + gp.g), fail_pending);  // (pcap points: 1 + g rows each)
  m.role = e % std::max(o.group, 1);
  return m;
}

void cei1_all_extended(Kg1Ensemble& T, int p) { cei1_join_believed_feasible(T, 0, p, true); }

// a pick joins every sub-member's extension, then the members' incumbents under the feasibility test, inside device memory
void cei1_pick_appended(Kg1Ensemble& T) {
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
  cei1_join_believed_feasible(T, T.p, 1, false);
}

namespace {

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  const long n = (value_out != nullptr ? (long)C : 0) + (grad_out != nullptr ? (long)C * T.d : 0);
  if (n == 0) return;
  MOE_LAUNCH_NOW(cei1_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, T.E / T.group, T.group, (long)C, T.d, T.dKgTab,
                 T.dGradTab, value_out, grad_out);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

// No sets, no fidelity coordinates; groups of 1 + K sub-members under the product rule (K = 0: one GP per member and the mean).
// The call keeps the sub-members' limits [E (1 + K)].
Kg1Call cei1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* best_so_far) {
  const int E = num_mcmc, K = num_constraints;
  Kg1Call call;
  call.doubles.resize((size_t)E * (1 + K));
  for (int e = 0; e < E; ++e) {
    call.doubles[(size_t)e * (1 + K)] = best_so_far[e];
    for (int k = 0; k < K; ++k) call.doubles[(size_t)e * (1 + K) + 1 + k] = thresholds[k];
  }
  call.o.best_so_far = call.doubles.data();
  call.o.member = cei1_member;
  call.o.eval_points = cei1_eval_points;
  call.o.all_extended = cei1_all_extended;
  call.o.pick_appended = cei1_pick_appended;
  call.o.group = 1 + K;
  call.o.combine = combine;
  call.check_members = ei1_check_members;
  return call;
}

void check_ei_constrained_shapes(int num_mcmc, int num_constraints, const void* constraint_gps, const double* thresholds,
                                 const double* best_so_far) {
  if (num_constraints < 0 || num_constraints > kCeiMaxConstraints)
    throw Error(MOE_ERR_BOUNDS, "num_constraints must be between 0 and 8", num_constraints, 0, kCeiMaxConstraints);
  if ((long)num_mcmc * (1 + num_constraints) > 1024)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc (1 + num_constraints) must be at most 1024", num_mcmc, 1, 1024 / (1 + num_constraints));
  if (num_constraints > 0 && (constraint_gps == nullptr || thresholds == nullptr))
    throw Error(MOE_ERR_RUNTIME, "constraint_gps and thresholds must not be NULL with num_constraints > 0");
  for (int k = 0; k < num_constraints; ++k)
    if (!std::isfinite(thresholds[k])) throw Error(MOE_ERR_INVALID_VALUE, "thresholds must be finite", thresholds[k], k, 0);
  for (int e = 0; e < num_mcmc; ++e)
    if (std::isnan(best_so_far[e]) || best_so_far[e] == -INFINITY)
      throw Error(MOE_ERR_INVALID_VALUE, "best_so_far must be finite or +infinity (no feasible observation yet)", best_so_far[e], e, 0);
}

}  // namespace moe
