// cornell_moe_amd/csrc/logehvi3.hip -- the LOG of the three-objective expected hypervolume improvement, with 0 to 8 constraints (the
// log of cehvi1.hip's M = 3 quantity, in the way of Ament, Daulton, Eriksson, Balandat & Bakshy, "Unexpected improvements to expected
// improvement", NeurIPS 2023), averaged over a hyper-parameter ensemble, with pending points, its multistart ascent and greedy
// q-point batches, on the device (moe_log_ehvi3_constrained_mcmc, moe_log_ehvi3_constrained_mcmc_multistart,
// moe_log_ehvi3_constrained_mcmc_suggest): the eleventh client of kg1_ascent.hip's staging, ascent and drivers.  The sub-member's
// chain, layout and check are ehvi1.hip's (ehvi1.hpp); the fronts kept per member in device memory, the box tables, the join rule,
// the believed-feasibility mask, the pending-row extension and the greedy batch's hand-over of a pick are ehvi3.hip's and
// cehvi1.hip's (ehvi3.hpp, cehvi1.hpp), K = 0 included: no front, table, believed or objectives kernel is touched.  The log-sum-exp
// record and the log-feasibility kernel are logehvi1.hip's (logehvi1.hpp); this file keeps the log-box kernel, the combine kernel
// and the description of the call (logehvi3_call).
//
// Why.  A member's plain value is a sum of products of three psi factors times K probabilities of feasibility in float64: it is
// exactly 0, with a zero gradient, wherever the candidate's mean lies a few dozen deviations above the reference point in any one
// objective or one constraint is far from feasible -- with three factors sooner than with two -- and every start of an ascent then
// ties at 0.  The log is finite with a useful gradient for every finite input.
//
// Minimisation.  E joint hyper-samples; member e is 3 + K GPs (roles 0 .. 2 the objectives, role 2 + k constraint k, satisfied
// where c_k(x) <= tau_k), 0 <= K <= 8, the E (3 + K) GPs the SUB-MEMBERS of one Kg1Ensemble ordered [e][role].  r = (r1, r2, r3);
// a member's front is n points (u_i, v_i, w_i) in ehvi3.hip's canonical order and its boxes are ehvi3_table_kernel's: box b is
// (left u edge, right u edge, v edge of the height, slab k), edge index 0 -infinity, 1 .. n the points, n + 1 the reference point;
// slab k lies between w_k and w_{k+1}.  ONE variance floor for value and gradient, sigma = sqrt(max(150 eps^2, var))
// (logehvi1.hip's).  For objective role r and an edge t:
//   z = (t - mu_r) / sigma_r,  (log h, lam, kap) = log_h_parts(z),  lambda_r(t) = log sigma_r + log h = log psi_r(t)
//   lambda_r(-infinity) = -infinity with lam = kap = 0
// The DIFFERENCE RULE for an objective r and edges a < b (logehvi1.hip's strip rule):
//   D = lambda_r(a) - lambda_r(b),  rho = exp(D) in [0, 1]
//   one_minus = 1 - rho (rho <= 1/2) or -expm1(D) (above);  log[psi_r(b) - psi_r(a)] = lambda_r(b) + log1p(-rho) or + log(-expm1(D))
//   d/dmu_r = -(lam_b - rho lam_a) / (sigma_r one_minus),  d/dvar_r = (kap_b - rho kap_a) / (2 sigma_r^2 one_minus)
//   edges that do not give D < 0 in float64 (rho = 1: a slab of zero thickness, neighbours an ulp apart) carry weight 0
// Box b:  log P by the rule from objective 1 at (left, right), log W_k by the rule from objective 3 at (w_k, w_{k+1}),
//   l_b = ((log P) + lambda_2(height)) + log W_k,  every term of the plain sum being P Q W with P, Q, W >= 0 (psi increases in its
//   edge): no signed terms.  Its six derivatives are the rule's for objectives 1 and 3 and (-lam / sigma_2, kap / (2 sigma_2^2)) at
//   the height for objective 2.  A box whose P or W has weight 0 is skipped, not evaluated: no 0 / 0.  The box of slab 0 has left
//   edge -infinity and lower w edge -infinity, so it always counts and a member's sum is positive.
// Member:  L_e = log sum_b exp l_b, its six coefficients c = (sum_b w_b dl_b/d.) / W_e.  L_e is never clipped.
//   log F_{e,k} and its derivatives: logehvi1.hip's (logehvi1_feas_kernel over groups of 3 + K)
//   LL_e = L_e + log F_{e,1} + ... + log F_{e,K}                                                      added in that order
//   g_e  = ((((c_mu1 grad mu_1 + c_var1 grad var_1) + c_mu2 grad mu_2) + c_var2 grad var_2) + c_mu3 grad mu_3) + c_var3 grad var_3,
//          then + grad log F_{e,k}, k = 1 .. K                                                      (ehvi3_combine_kernel's order)
// Ensemble (logehvi1_combine_kernel's rule):
//   m = max_e LL_e,  w_e = exp(LL_e - m),  W = w_0 + ... + w_{E-1} in member order
//   value = m + log W - log E,  grad = (w_0 g_0 + ... + w_{E-1} g_{E-1}) / W
// every operation rounded by itself, no atomics.  With E = 1 the value is LL_0 bit for bit.
//
// Log-box kernel and its REDUCTION ORDER.  ehvi3_box_kernel's grid: one workgroup of four wavefronts per (candidate, member).
//   Phase 1  the threads form (lambda, lam, kap) at every edge of the three objectives, 3 (n + 2) log_h_parts in all, into LDS
//            [3][3][258]; edge 0 is (-infinity, 0, 0).
//   Phase 2  thread k forms slab k's log W_k and the two derivative pieces of objective 3 into LDS [3][257] (log W_k = -infinity
//            marks weight 0): n + 1 exp and log1p instead of one per box.  The three rows lie apart, not interleaved: a wavefront's
//            64 boxes are neighbours in a slab-major table, so they read one or two slabs and every row's read is a broadcast,
//            whichever way the rows lie; kept apart, phase 2's stores are unit-stride.
//   Phase 3  thread t of sweep s owns box b = 256 s + t.  It applies the rule to objective 1, adds up l_b with contraction off and
//            takes the box into its own running-maximum record (m, W, S[6]) (record_take), sweep after sweep in ascending s.
//   Phase 4  a wavefront's 64 records merge by the fixed butterfly (xor 32, 16, 8, 4, 2, 1; record_merge); the four wavefronts'
//            records pass through LDS and merge as (0 + 1) + (2 + 3) by the same rule (record_join).  Thread 0 writes
//            L_e = m + log W and S / W.
// LDS: 18 576 + 6 168 + 256 bytes, six workgroups to a CU's 160 KiB.  The order depends on the member's table alone: not on the
// candidates that share the launch (one workgroup each), not on want_grad (m and W do not see the flag), not on the pass boundary,
// not on ensemble-wide launches (the box, feasibility and combine kernels are never recorded).  With n = 0 the one box gives
// (lambda_1(r1) + lambda_2(r2)) + lambda_3(r3): log1p(-0) = 0 and W = 1.
//
// The group values of the evaluator are [E][1 + K][C]: L_e, log F_{e,1} .. log F_{e,K}, from which the value is the rule above.
//
// Limits: the plain M = 3 form's -- F <= 192 and at most 64 pending points, so cap <= 256 and B <= 33 153; K <= 8, E <= 341 and
// E (3 + K) <= 1024; no derivative observations; tensor-product domains.  A candidate never raises; only a pending point whose
// Schur pivot fails does, payload (the flat index e (3 + K) + role, the point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "cehvi1.hpp"
#include "ehvi1.hpp"
#include "ehvi3.hpp"
#include "kg1_ascent.hpp"
#include "logehvi1.hpp"

namespace moe {

namespace {

constexpr int kLogEhvi3Cap = kEhvi3MaxFront + kKg1MaxPending;  // a member's front at its largest
constexpr int kLogEhvi3Edges = kLogEhvi3Cap + 2;               // -infinity, the points, the reference point
static_assert(kLogEhvi3Cap == 256, "phase 2 gives every slab but the last a thread of its own");

// the header's difference rule from (lambda, lam, kap) at the edges a < b of an objective with deviation s: false where the pair
// carries weight 0 (nothing is written); otherwise log[psi(b) - psi(a)] and, with wg, the two derivative pieces
__device__ __forceinline__ bool log_difference(double la, double lama, double kapa, double lb, double lamb, double kapb, double s, bool wg, double& log_diff, double& dmu, double& dvar) {
#pragma clang fp contract(off)
  const double D = la - lb;
  if (!(D < 0.0)) return false;
  const double rho = exp(D);
  double one_minus, log_one_minus;
  if (rho <= 0.5) {
    one_minus = 1.0 - rho;
    log_one_minus = log1p(-rho);
  } else {
    one_minus = -expm1(D);
    log_one_minus = log(one_minus);
  }
  log_diff = lb + log_one_minus;
  if (wg) {
    dmu = -(lamb - rho * lama) / (s * one_minus);
    dvar = (kapb - rho * kapa) / (2.0 * (s * s) * one_minus);
  }
  return true;
}

// The log box sums (the header's reduction order).  Grid (C, E), four wavefronts; kg: the objective sub-members' [mu Cs | var Cs]
// ordered [e][3]; fronts / counts as ehvi3_front_kernel leaves them, tables / nbox as ehvi3_table_kernel does; vals [E][Cs] takes
// L_e and, with want_grad, coef [E][Cs][6] takes dL/dmu_1, dL/dvar_1, dL/dmu_2, dL/dvar_2, dL/dmu_3, dL/dvar_3.
__global__ __launch_bounds__(256) void logehvi3_box_kernel(int Cs, const double* const* __restrict__ kg, const double* __restrict__ fronts, int cap, const int* __restrict__ counts, const ushort4* __restrict__ tables, size_t tstride, const int* __restrict__ nbox, double r1, double r2, double r3, int want_grad, double* __restrict__ vals, double* __restrict__ coef) {
#pragma clang fp contract(off)
  __shared__ double s_e[3][3][kLogEhvi3Edges];    // [objective][lambda, lam, kap][edge]
  __shared__ double s_w[3][kLogEhvi3Cap + 1];     // [log W, dl/dmu_3, dl/dvar_3][slab]
  __shared__ double s_rec[4][8];                  // the wavefronts' records (m, W, S[6])
  const int c = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
  const int n = min(counts[e], min(cap, kLogEhvi3Cap));
  const int B = min(nbox[e], (n + 1) * (n + 2) / 2);
  const bool wg = want_grad != 0;
  const double* pts = fronts + (size_t)e * 3 * cap;
  double sd[3], mu[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mu[k] = kg[3 * e + k][c];
    sd[k] = sqrt(fmax(kMinVarGradEI, kg[3 * e + k][(size_t)Cs + c]));
  }
  // phase 1: the edges
  const int edges = n + 2;
  for (int idx = tid; idx < 3 * edges; idx += 256) {
    const int k = idx / edges, i = idx - k * edges;
    double lambda = -INFINITY, lam = 0.0, kap = 0.0;  // edge 0
    if (i > 0) {
      const double t = i <= n ? pts[(size_t)k * cap + i - 1] : (k == 0 ? r1 : (k == 1 ? r2 : r3));
      const double m = k == 0 ? mu[0] : (k == 1 ? mu[1] : mu[2]), s = k == 0 ? sd[0] : (k == 1 ? sd[1] : sd[2]);
      double lh;
      log_h_parts((t - m) / s, lh, lam, kap);
      lambda = log(s) + lh;
    }
    s_e[k][0][i] = lambda;
    s_e[k][1][i] = lam;
    s_e[k][2][i] = kap;
  }
  __syncthreads();
  // phase 2: the slabs
  for (int k = tid; k <= n; k += 256) {
    double lw = -INFINITY, dm = 0.0, dv = 0.0;
    log_difference(s_e[2][0][k], s_e[2][1][k], s_e[2][2][k], s_e[2][0][k + 1], s_e[2][1][k + 1], s_e[2][2][k + 1], sd[2], wg, lw, dm, dv);
    s_w[0][k] = lw;
    s_w[1][k] = dm;
    s_w[2][k] = dv;
  }
  __syncthreads();
  // phase 3: the boxes
  const ushort4* tab = tables + (size_t)e * tstride;
  LogStripRecord<6> rec = {-INFINITY, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
  for (int b = tid; b < B; b += 256) {
    const ushort4 bx = tab[b];
    const int uL = min((int)bx.x, n + 1), uR = min((int)bx.y, n + 1), vH = min((int)bx.z, n + 1), k = min((int)bx.w, n);
    const double lw = s_w[0][k];
    if (lw == -INFINITY) continue;  // (W carries weight 0)
    double lp, dl[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!log_difference(s_e[0][0][uL], s_e[0][1][uL], s_e[0][2][uL], s_e[0][0][uR], s_e[0][1][uR], s_e[0][2][uR], sd[0], wg, lp, dl[0], dl[1]))
      continue;  // (P carries weight 0)
    const double l = (lp + s_e[1][0][vH]) + lw;
    if (wg) {
      dl[2] = -s_e[1][1][vH] / sd[1];
      dl[3] = s_e[1][2][vH] / (2.0 * (sd[1] * sd[1]));
      dl[4] = s_w[1][k];
      dl[5] = s_w[2][k];
    }
    record_take(rec, l, dl, wg);
  }
  // phase 4: the merge
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) record_merge(rec, off, wg);
  if ((tid & 63) == 0) {
    double* r = s_rec[tid >> 6];
    r[0] = rec.m;
    r[1] = rec.W;
#pragma unroll
    for (int q = 0; q < 6; ++q) r[2 + q] = rec.S[q];
  }
  __syncthreads();
  if (tid != 0) return;
  LogStripRecord<6> w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i].m = s_rec[i][0];
    w[i].W = s_rec[i][1];
#pragma unroll
    for (int q = 0; q < 6; ++q) w[i].S[q] = s_rec[i][2 + q];
  }
  record_join(w[0], w[1], wg);
  record_join(w[2], w[3], wg);
  record_join(w[0], w[2], wg);
  const size_t o = (size_t)e * Cs + c;
  vals[o] = w[0].m + log(w[0].W);
  if (wg) {
#pragma unroll
    for (int q = 0; q < 6; ++q) coef[6 * o + q] = w[0].S[q] / w[0].W;
  }
}

// The log-sum-exp over the members, one thread per output element (logehvi1_combine_kernel's shape and rule with six hypervolume
// terms in ehvi3_combine_kernel's order): element i < nv of value_out (NULL: nv = 0) is candidate i's value, the elements behind
// are grad_out's (c, j).  hv [E][Cs] and coef [E][Cs][6]: the log-box kernel's; feas: logehvi1_feas_kernel's; grads: the E (3 + K)
// sub-members' [grad mu Cs d | grad var Cs d].  A value thread also leaves its candidate's group values in factors [E][1 + K][Cs].
// Every operation rounded by itself, in the header's order; a thread works out every member's LL_e twice and nothing is kept
// between threads.
__global__ __launch_bounds__(256) void logehvi3_combine_kernel(int E, int K, long C, int Cs, int d, const double* __restrict__ hv, const double* __restrict__ coef, const double* __restrict__ feas, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out, double* __restrict__ factors) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  const long k = i - nv, c = (i < nv) ? i : k / d;
  const int G = 3 + K;
  const size_t gv = (size_t)Cs * d;
  double m = logehvi1_member_log(hv, feas, 0, K, Cs, c);
  for (int e = 1; e < E; ++e) m = fmax(m, logehvi1_member_log(hv, feas, e, K, Cs, c));
  double W = 0.0, sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double w = exp(logehvi1_member_log(hv, feas, e, K, Cs, c) - m);
    W = (e == 0) ? w : W + w;
    if (i < nv) {
      factors[(size_t)e * (1 + K) * Cs + c] = hv[(size_t)e * Cs + c];
      for (int q = 0; q < K; ++q) factors[((size_t)e * (1 + K) + 1 + q) * Cs + c] = feas[3 * (((size_t)e * K + q) * Cs + c)];
      continue;
    }
    const double* co = coef + 6 * ((size_t)e * Cs + c);
    double g = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double* gr = grads[(size_t)e * G + r];
      const double tm = co[2 * r] * gr[k];
      g = (r == 0) ? tm : g + tm;
      const double tv = co[2 * r + 1] * gr[gv + k];
      g = g + tv;
    }
    for (int q = 0; q < K; ++q) {
      const double* f = feas + 3 * (((size_t)e * K + q) * Cs + c);
      const double* gq = grads[(size_t)e * G + 3 + q];
      const double tm = f[1] * gq[k];
      const double tv = f[2] * gq[gv + k];
      const double gF = tm + tv;
      g = g + gF;
    }
    const double term = w * g;
    sum = (e == 0) ? term : sum + term;
  }
  if (i < nv)
    value_out[i] = m + log(W) - log((double)E);
  else
    grad_out[k] = sum / W;
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  if (value_out == nullptr && grad_out == nullptr) return;
  const CehviCall& k = *static_cast<const CehviCall*>(T.client);
  const CehviLayout l = cehvi_layout(T);
  if (C < 1 || C > l.C) throw Error(MOE_ERR_RUNTIME, "logehvi3: more candidates than the call was staged for");
  double* base = T.gps[0]->ehviD.p;
  const double* const* obj = reinterpret_cast<const double* const*>(base + l.oObj);
  const bool wg = grad_out != nullptr;
  MOE_LAUNCH_NOW(logehvi3_box_kernel, dim3((unsigned)C, (unsigned)l.E), dim3(256), 0, T.z, l.C, obj, (const double*)(base + l.l3.oFront),
                 l.l3.cap, reinterpret_cast<const int*>(base + l.l3.oCount), reinterpret_cast<const ushort4*>(base + l.l3.oTable),
                 l.l3.tstride, reinterpret_cast<const int*>(base + l.l3.oNbox), k.c3.r1, k.c3.r2, k.c3.r3, wg ? 1 : 0, base + l.l3.oVals,
                 base + l.l3.oCoef);
  if (l.K > 0) {
    const long nf = (long)l.E * l.K * C;
    MOE_LAUNCH_NOW(logehvi1_feas_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, T.z, T.dKgTab, l.E, 3, l.K, k.tau, C,
                   l.C, wg ? 1 : 0, base + l.oFeas);
  }
  const long n = (value_out != nullptr ? (long)C : 0) + (wg ? (long)C * T.d : 0);
  MOE_LAUNCH_NOW(logehvi3_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, l.E, l.K, (long)C, l.C, T.d,
                 (const double*)(base + l.l3.oVals), (const double*)(base + l.l3.oCoef), (const double*)(base + l.oFeas), T.dGradTab,
                 value_out, grad_out, base + l.oFactors);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

Kg1Call logehvi3_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                      int num_front) {
  CehviCall c = cehvi_constraints_of(3, num_constraints, thresholds);
  c.c3 = Ehvi3Call{front, num_front, reference_point[0], reference_point[1], reference_point[2]};
  return cehvi_call_combined_by(num_mcmc, c, combine);
}

}  // namespace moe
