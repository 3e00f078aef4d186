// cornell_moe_amd/csrc/logeipc1.hip -- the LOG of the constrained expected improvement PER UNIT COST averaged over a hyper-parameter
// ensemble ("EI per second": Snoek, Larochelle & Adams, NeurIPS 2012, the log of the cost modelled by a GP of its own; the exponent
// of cost-cooling: Lee, Perrone, Archambeau & Seeger 2020), with pending points, its multistart ascent and greedy q-point batches, on
// the device (moe_log_ei_per_cost_mcmc, moe_log_ei_per_cost_mcmc_multistart, moe_log_ei_per_cost_mcmc_suggest): the fourteenth client
// of kg1_ascent.hip's staging, ascent and drivers.  The sub-member's layout, the members' check, the pass and the gradient's tail are
// cei1.hip's and ei1.hip's (cei1.hpp, ei1.hpp); this file keeps the candidate kernel with its three roles, the combine kernel, the
// believed-feasible incumbent over the roles that take part in it and the description of the call.
//
// A call takes E joint hyper-samples, K constraints (0 <= K <= 8) and an exponent alpha >= 0.  Member e is 2 + K GPs, the E (2 + K)
// GPs the sub-members of one Kg1Ensemble ordered [e][role]: role 0 the objective, roles 1 .. K the constraints (satisfied where
// c_k(x) <= tau_k), role K + 1 a GP of the LOG of the evaluation cost.  Every GP's covariance, the cost GP's too, is conditioned on
// the pending points (the Kriging-believer extension, the mean left alone): one staging serves every sub-member, so the variance
// term of the cost is the conditioned one -- a pending point is believed to return the cost's posterior mean as it returns the
// objective's.  All 2 + K GPs of a call carry ONE observed-derivative list (ei1_check_members over the flat list, as cei1.hip
// requires): a pending point is 1 + g extension rows of at most 64.  With var the conditioned latent variance of the sub-member at
// x and ONE floor for value and gradient, v = max(150 eps^2, var), sigma = sqrt(v):
//   role 0      l = log sigma + log h(c), c = (b'_e - mu) / sigma      exactly logcei1.hip's role 0 (b'_e = +infinity: l = 0, gradient 0)
//   role k      l = log Phi(z), z = (tau_k - mu) / sigma               exactly its role k
//   cost role   l = -(alpha (mu + v / 2))                              the log of E[cost]^-alpha under a log-normal cost
//               grad l = -alpha grad mu - (alpha / 2) grad var         where var lies below the floor the second term is 0
// -- ei1.hip's gradient form, grad = -s grad mu + (w / 2) grad var, with (s, w) = (alpha, -alpha): the candidate kernel leaves s in
// dScal and the column w v'_x in dT, ei1_grad_tail serves unchanged.
//   L_e = ((l_{e,0} + l_{e,1}) + ... + l_{e,K}) + l_{e,cost},  g_e likewise                 added in that order
//   m = max_e L_e,  w_e = exp(L_e - m),  W = w_0 + ... + w_{E-1}                              members in member order
//   value = m + log W - log E,   grad = (w_0 g_0 + ... + w_{E-1} g_{E-1}) / W
// every operation rounded by itself, no fused multiply-add in these rules, no atomics.  With alpha = 0 the cost role's l is a zero
// and its gradient zeros, and the call is moe_log_ei_constrained_mcmc on the objective and constraint GPs bit for bit.  The members'
// own values of an evaluation are the sub-members' l [E (2 + K)][C], the cost row last.
//
// The believed-feasible incumbent b'_e is cei1.hip's (the same kernel arithmetic in the same order) over roles 0 .. K; the cost GP
// takes no part in it.  cei1.hip's hook walks a whole group and its table holds 1 + 8 roles, so a group of 2 + K has a join of
// its own here, which also spares the cost GP's mean at the pending points.  The cost sub-member's limit is alpha.
//
// Bits.  The variance is ei1_cand_kernel's ONE fused multiply-add chain over the rows in order; a candidate's bits do not depend on
// who shares its pass, on want_grad or on ensemble-wide launches.  A candidate never raises; only a pending point whose Schur pivot
// fails does, payload (the flat index e (2 + K) + role of the GP, the pending point).
#include <algorithm>
#include <cmath>

#include "acq1_device.hpp"
#include "cei1.hpp"
#include "device_cov.hpp"
#include "ei1.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

constexpr int kCostRole = -1;  // Kg1Member::role of the cost sub-member (the last of its group)

// the cost role's log, each operation rounded by itself
__device__ __forceinline__ double logeipc1_cost_log(double alpha, double mu, double v) {
#pragma clang fp contract(off)
  const double half = 0.5 * v;
  const double mean_log = mu + half;
  const double scaled = alpha * mean_log;
  return -scaled;
}

// One wavefront per candidate: ei1_cand_kernel's chain for the variance (row_chain), then the scalars of the sub-member's role,
// the same in every lane (lane 0 writes them).  *best is b' (role 0), tau_k (role k) or alpha (the cost role); val_out takes l, and
// with want_grad s_out the scalar s and T the column w v'_x.  Roles 0 .. K are logcei1_cand_kernel's statements.
struct logeipc1_cand_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int R, int ld, int ncols, int col0, const CovParams& cp, int want_grad, int role, const double* __restrict__ best, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ s_out, double* __restrict__ T) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const double* v = Vx + (size_t)c * ld;
    const double ss = row_chain(v, 0, R, lane, 0.0);
    const double var = radial_scalars(cp.type, cp.alpha, 0.0).base - ss;
    const double b = *best;
    double* tc = T + (size_t)c * ld;
    if (role == kCostRole) {  // b is alpha
      if (lane == 0) val_out[col0 + c] = logeipc1_cost_log(b, mu[c], fmax(kMinVarGradEI, var));
      if (want_grad == 0) return;
      if (lane == 0) s_out[c] = b;
      const double wc = (var < kMinVarGradEI) ? 0.0 : -b;
      for (int r = lane; r < R; r += 64) tc[r] = wc * v[r];
      return;
    }
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
__global__ __launch_bounds__(256) void logeipc1_cand_kernel(int R, int ld, int ncols, int col0, const CovParams cp, int want_grad, int role, const double* __restrict__ best, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ val_out, double* __restrict__ s_out, double* __restrict__ T) {
  logeipc1_cand_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, R, ld, ncols, col0, cp, want_grad, role, best, mu, Vx, val_out, s_out, T);
}

// candidate c's L_e: member e's G logs added in the order objective, k = 1 .. K, cost
__device__ __forceinline__ double logeipc1_member_log(const double* const* __restrict__ f, int G, long c) {
#pragma clang fp contract(off)
  double L = f[0][c];
  for (int q = 1; q < G; ++q) L = L + f[q][c];
  return L;
}

// The log-sum-exp over the members, one thread per output element (logcei1_combine_kernel's shape and rule over groups of G = 2 + K).
// vals / grads: the E G sub-members' logs [C] and gradients [C][d], ordered [e][role].  Element i < nv of value_out (NULL: nv = 0)
// is candidate i's value; the elements behind are grad_out's (c, j).  Every sum in the header's order, each operation rounded by
// itself; nothing is kept between threads.
__global__ __launch_bounds__(256) void logeipc1_combine_kernel(int E, int G, long C, int d, const double* const* __restrict__ vals, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  const long k = i - nv, c = (i < nv) ? i : k / d;
  double m = logeipc1_member_log(vals, G, c);
  for (int e = 1; e < E; ++e) m = fmax(m, logeipc1_member_log(vals + (size_t)e * G, G, c));
  double W = 0.0, sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double w = exp(logeipc1_member_log(vals + (size_t)e * G, G, c) - m);
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

// One member's believed-feasible incumbent and its sub-members' limits in device memory: cei1_best_kernel over the F = 1 + K roles
// that take part (mu[r]: mu_{e,r} at `count` pending points), with the limits of all G = 2 + K roles written at first != 0 (lim: b_e,
// tau_1 .. tau_K, alpha; out: the sub-members' dBp).
struct Logeipc1Best {
  const double* mu[1 + kCeiMaxConstraints];
  double* out[2 + kCeiMaxConstraints];
  double lim[2 + kCeiMaxConstraints];
};
__global__ void logeipc1_best_kernel(Logeipc1Best a, int F, int G, int first, int count) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double v = first != 0 ? a.lim[0] : *a.out[0];
  for (int j = 0; j < count; ++j) {
    bool feasible = true;
    for (int r = 1; r < F; ++r) feasible = feasible && (a.mu[r][j] <= a.lim[r]);
    if (feasible) v = fmin(v, a.mu[0][j]);
  }
  *a.out[0] = v;
  if (first != 0)
    for (int r = 1; r < G; ++r) *a.out[r] = a.lim[r];
}

// mu of the objective and constraint sub-members at P_j0 .. j0 + count - 1, then every member's believed-feasible incumbent
void join_believed_feasible(Kg1Ensemble& T, int j0, int count, bool first) {
  const int G = T.group, F = G - 1;
  if (G < 2 || G > 2 + kCeiMaxConstraints) throw Error(MOE_ERR_RUNTIME, "logeipc1: a member is 2 + K GPs, 0 <= K <= 8");
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0 && m.role != kCostRole)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  for (int e = 0; e < T.E; e += G) {
    Logeipc1Best a = {};
    for (int r = 0; r < G; ++r) {
      if (r < F) a.mu[r] = T.mem[e + r].dAA;
      a.out[r] = T.mem[e + r].dBp;
      a.lim[r] = T.mem[e + r].best;
    }
    MOE_LAUNCH_NOW(logeipc1_best_kernel, dim3(1), dim3(64), 0, T.z, a, F, G, first ? 1 : 0, count);
  }
  MOE_HIP_CHECK(hipGetLastError());
}

// cei1.hip's layout; o.best_so_far holds the sub-members' limits [E G]: b_e, tau_1 .. tau_K, alpha.  The last of a group is the cost.
Kg1Member member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  Kg1Member m = cei1_member(o, gp, e, C, with_grad, fail, pcap, fail_pending);
  if (m.role == o.group - 1) m.role = kCostRole;
  return m;
}

void all_extended(Kg1Ensemble& T, int p) { join_believed_feasible(T, 0, p, true); }

// a pick joins every sub-member's extension, the cost GP's too, then the members' incumbents under the feasibility test
void pick_appended(Kg1Ensemble& T) {
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
  join_believed_feasible(T, T.p, 1, false);
}

// ei1.hip's pass with logeipc1_cand_kernel in the place of ei1_cand_kernel (dScal holds s)
void cand_step(const Kg1Member& m, int nc, int c0, bool with_grad, hipStream_t s) {
  launch_kernel_ens<logeipc1_cand_kernel_body, 256>(logeipc1_cand_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, m.gp->N + m.p,
                                                    m.ld, nc, c0, m.gp->cp, with_grad ? 1 : 0, m.role, (const double*)m.dBp,
                                                    (const double*)m.dMuh, (const double*)m.dVx, m.dKg, m.dScal, m.dT);
}

void logeipc1_eval_points(const Kg1Member& m, const double* Px, const double*, int C, bool with_grad, hipStream_t s) {
  ei1_eval_passes(m, Px, C, with_grad, s, "logeipc1_eval_pass", cand_step, ei1_grad_tail);
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  const long n = (value_out != nullptr ? (long)C : 0) + (grad_out != nullptr ? (long)C * T.d : 0);
  if (n == 0) return;
  MOE_LAUNCH_NOW(logeipc1_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, T.E / T.group, T.group, (long)C, T.d,
                 T.dKgTab, T.dGradTab, value_out, grad_out);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

// Groups of 2 + K sub-members under the log-sum-exp.  The call keeps the sub-members' limits [E (2 + K)]; the members' own values
// of an evaluation are the sub-members' logs, which the drivers gather from the members' tables themselves (no group_values: the
// groups' rows ARE the members' rows).
Kg1Call logeipc1_call(int num_mcmc, int num_constraints, const double* thresholds, double cost_exponent, const double* best_so_far) {
  const int E = num_mcmc, K = num_constraints, G = 2 + K;
  Kg1Call call;
  call.doubles.resize((size_t)E * G);
  for (int e = 0; e < E; ++e) {
    call.doubles[(size_t)e * G] = best_so_far[e];
    for (int k = 0; k < K; ++k) call.doubles[(size_t)e * G + 1 + k] = thresholds[k];
    call.doubles[(size_t)e * G + 1 + K] = cost_exponent;
  }
  call.o.best_so_far = call.doubles.data();
  call.o.member = member;
  call.o.eval_points = logeipc1_eval_points;
  call.o.all_extended = all_extended;
  call.o.pick_appended = pick_appended;
  call.o.group = G;
  call.o.combine = combine;
  call.o.combine_single_groups = true;
  call.check_members = ei1_check_members;
  return call;
}

void check_log_ei_per_cost_shapes(int num_mcmc, int num_constraints, const void* constraint_gps, const double* thresholds,
                                  double cost_exponent, const double* best_so_far) {
  if (num_constraints < 0 || num_constraints > kCeiMaxConstraints)
    throw Error(MOE_ERR_BOUNDS, "num_constraints must be between 0 and 8", num_constraints, 0, kCeiMaxConstraints);
  if ((long)num_mcmc * (2 + num_constraints) > 1024)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc (2 + num_constraints) must be at most 1024", num_mcmc, 1, 1024 / (2 + num_constraints));
  check_ei_constrained_shapes(num_mcmc, num_constraints, constraint_gps, thresholds, best_so_far);
  if (!std::isfinite(cost_exponent) || cost_exponent < 0.0)
    throw Error(MOE_ERR_INVALID_VALUE, "cost_exponent must be finite and not negative", cost_exponent, 0, 0);
}

}  // namespace moe
