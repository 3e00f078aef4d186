// cornell_moe_amd/csrc/logchebei1.hip -- the LOG of the Chebyshev-scalarised expected improvement for 2 to 8 objectives, with 0 to 8
// constraints (the log of chebei1.hip's quantity times the probabilities of feasibility, in the way of Ament, Daulton, Eriksson,
// Balandat & Bakshy, "Unexpected improvements to expected improvement", NeurIPS 2023), under a hyper-parameter ensemble's
// log-sum-exp, with pending points, its multistart ascent and greedy q-point batches with a scalarisation per point, on the device
// (moe_log_ei_chebyshev_constrained_mcmc, _multistart, _suggest): the thirteenth client of kg1_ascent.hip's staging, ascent and
// drivers.  The sub-member's chain and the members' check are ehvi1.hip's (ehvi1.hpp); the quadrature's constants are chebei1.hip's
// (chebei1.hpp); the running-maximum record, its merge, the log-feasibility kernel and a member's LL_e are logehvi1.hip's
// (logehvi1.hpp); this file keeps the outcome kernel with the believed-feasibility mask, the log-node kernel, the combine kernel
// and the description of the call (logchebei1_call).
//
// Why.  chebei1.hip's member value is exactly 0, with zero coefficients, wherever the incumbent lies at or below L = max_j (s_j - 38
// tau_j), and long before that the product of M normal CDFs is so small that every start of an ascent ties at 0 -- with M factors
// sooner than with one, and most of all late in a run.  The log is finite with a useful gradient for every finite input.
//
// Minimisation.  E joint hyper-samples; member e is M + K GPs (roles 0 .. M - 1 the objectives, role M - 1 + k constraint k,
// satisfied where c_k(x) <= thresholds[k - 1]), the E (M + K) GPs the SUB-MEMBERS of one Kg1Ensemble ordered [e][role].  With
// chebei1.hip's a_j, b_j, sigma_j = sqrt(max(150 eps^2, var_j)), s_j = a_j mu_j + b_j, tau_j = a_j sigma_j, L and the member's
// incumbent g (finite):
//   z_j(t) = (t - s_j) / tau_j,  (log Phi_j, r_j) = log_cdf_parts(z_j),  log f(t) = sum_j log Phi_j    added in the order of j
//   OFFSETS: d_j = g - s_j is formed once and everything below g is measured as u = g - t >= 0, z_j = (d_j - u) / tau_j.  ell can
//            lie far below an ulp of g (a floored sigma_j under an s_j above the incumbent: ell of order 1e-29 at g of order 1);
//            formed as g - kappa ell every breakpoint would round to g and no node would be left.  In offsets the panels below
//            the incumbent always have width, and the rounding of a node's position is relative to d_j, not to g.
//   ell    = min(1 / sum_j (r_j(g) / tau_j), max_j tau_j)
//            f is log-concave, so f(t) <= f(g) exp((t - g) sum_j r_j(g) / tau_j) below g: the first term is the decay length of
//            that bound.  The cap binds only where f does not decay at g (every z_j(g) above about -0.3), and keeps ell finite.
//   Lambda = min(L, g - 40 ell):  what lies below is under e^-40 of the bound's integral, or, below L, under 1e-300 absolutely
//   LA_e   = log integral over Lambda <= t <= g of f                       there is no `g <= L -> 0` branch
//   dLA/dmu_j  = -a_j <r_j / tau_j>,  dLA/dvar_j = -(a_j / (2 sigma_j)) <z_j r_j / tau_j>,  <.> the f-weighted mean over [Lambda, g]
//            (z_j r_j changes sign with z_j: the means are signed sums of scaled terms, never logs).  Lambda and the breakpoints
//            are constants in the gradient: the integral is exact to rounding and Lambda's boundary term is below e^-40 relative.
//   log F_{e,k} and its derivatives: logehvi1.hip's (logehvi1_feas_kernel over groups of M + K)
//   LL_e  = LA_e + log F_{e,1} + ... + log F_{e,K}                                                      added in that order
//   g_e   = sum_j (c_mu_j grad mu_j + c_var_j grad var_j) in the order of j, mu before var, then + grad log F_{e,k}, k = 1 .. K
//   value = m + log(sum_e exp(LL_e - m)) - log E,  m = max_e LL_e,  grad = sum_e w_e g_e / sum_e w_e    (logehvi1_combine_kernel's
//           rule; with E = 1 the value is LL_0 bit for bit)
//
// The quadrature is FIXED.  Breakpoints, as offsets: position 14 j + i holds d_j - c_i tau_j (chebei1.hip's c: the offset of
// s_j + c_i tau_j), position 14 M + i holds kappa_i ell, kappa = {1/2, 1, 2, 3, 4.5, 6, 8, 10.5, 13, 16, 20, 24, 29, 34} (the
// LADDER: below every s_j - 8 tau_j the plain breakpoints leave one panel in which f falls by hundreds of orders of magnitude,
// while the mass lies within a few ell of g), all clamped to [0, U], U = max(min_j (d_j + 38 tau_j), 40 ell) = g - Lambda > 0;
// position 14 M + 14 holds U, position 14 M + 15 holds 0.  Sorted ascending in the offset, ties by position: 14 M + 16 <= 128
// points.  Per panel chebei1.hip's 8 Gauss-Legendre nodes; a panel of zero width is skipped; the first rung's panel never is.
//
// Outcomes.  chebei1.hip's rule with cehvi1.hip's mask: every member keeps the believed outcomes mu_{e,j}(P_i) [M][pcap] and a word
// per pending point, 1 where mu_{e,c_k}(P_i) <= thresholds[k] for every k; the round's incumbent is
//   g_e = min(best_so_far[t][e], min_i max_j (a_{t,j} mu_{e,j}(P_i) + b_{t,j}))
// over the pending points in use whose word is 1 and whose scalarised outcome is finite.  Every sub-member's variance is conditioned
// on every pending point, whichever way the belief falls.  K = 0: every word is 1 and the rule is chebei1.hip's bit for bit.
//
// Log-node kernel and its REDUCTION ORDER.  One wavefront per (candidate, member), instantiated per M.  Every lane forms the d_j, ell
// and U; the lanes form the breakpoints in LDS, two per lane at most, and rank them by counting.  Lane l of sweep s owns node
// 64 s + l; at most 16 sweeps.  Per node M log_cdf_parts, log f with contraction off, and the term log(weight) + log f goes into
// the lane's own running-maximum record (m, W, S[2 M]) with the ratios r_j / tau_j and z_j r_j / tau_j (record_take).  Sweeps
// ascend.  The 64 records merge by the fixed butterfly (xor 32, 16, 8, 4, 2, 1; record_merge).  Lane 0 writes LA_e = m + log W and
// the coefficients -a_j (S / W), -(a_j / (2 sigma_j)) (S / W).  The order depends on M alone: not on the candidates that share the
// launch, not on want_grad (m and W do not see the flag), not on the pass boundary, not on ensemble-wide launches (the outcome,
// node, feasibility and combine kernels are never recorded).
//
// The group values of the evaluator are [E][1 + K][C]: LA_e, log F_{e,1} .. log F_{e,K}.
//
// Limits: 2 <= M <= 8, 0 <= K <= 8, E (M + K) <= 1024, at most 64 pending points, no derivative observations; every incumbent
// finite (a caller without a feasible observation passes a finite cap of its own: the integral's upper limit must be finite).  A
// candidate never raises; only a pending point whose Schur pivot fails does, payload (the flat index e (M + K) + role, the point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "cehvi1.hpp"
#include "chebei1.hpp"
#include "ehvi1.hpp"
#include "kg1_ascent.hpp"
#include "logehvi1.hpp"

namespace moe {

namespace {

constexpr int kLogChebLadder = 14;  // rungs below the incumbent
constexpr double kLogChebReach = 40.0;

__constant__ double kLogChebKappa[kLogChebLadder] = {0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 8.0, 10.5, 13.0, 16.0, 20.0, 24.0, 29.0, 34.0};

// the call's record: the caller's arrays and the round in use (a greedy batch's pick moves it on)
struct LogChebCall {
  int M, K, R;
  CehviTau tau;
  const double* scal;  // [R][2 M]
  const double* best;  // [R][E]
  mutable int round;
};

// where the call's own device memory lies inside the first GP's ehviD, in doubles: E members of M + K GPs, R rounds, room for cap
// pending points, C staged candidates; the believed-feasibility words are integers
struct LogChebLayout {
  int E, M, K, R, cap, C;
  size_t oScal, oBest, oMeans, oMask, oInc, oVals, oCoef, oFeas, oFactors, total;
};

LogChebLayout layout_of(const Kg1Ensemble& T) {
  const LogChebCall& k = *static_cast<const LogChebCall*>(T.client);
  LogChebLayout l;
  l.M = k.M;
  l.K = k.K;
  l.R = k.R;
  l.E = T.E / (k.M + k.K);
  l.cap = std::max(1, T.pcap);
  l.C = T.mem[0].C;
  l.oScal = 0;
  l.oBest = l.oScal + 2 * (size_t)l.R * l.M;
  l.oMeans = l.oBest + (size_t)l.R * l.E;
  l.oMask = l.oMeans + (size_t)l.E * l.M * l.cap;
  l.oInc = l.oMask + ((size_t)l.E * l.cap + 1) / 2;
  l.oVals = l.oInc + (size_t)l.E;
  l.oCoef = l.oVals + (size_t)l.E * l.C;
  l.oFeas = l.oCoef + 2 * (size_t)l.M * l.E * l.C;
  l.oFactors = l.oFeas + 3 * (size_t)l.E * l.K * l.C;
  l.total = l.oFactors + (size_t)l.E * (1 + l.K) * l.C;
  return l;
}

// chebei1_outcome_kernel with the mask.  One wavefront per member (blockIdx.x).  kg: the E (M + K) sub-members' dKg, their mu at
// `count` pending points `aa` doubles behind; the objectives' go to places j0 .. j0 + count - 1 of the member's outcomes means
// [E][M][cap], and the member's belief about each of those points to mask [E][cap] (1 where every constraint's mean is <= its
// threshold; a NaN mean leaves 0).  Then the incumbent of the round whose scalarisation scal [2 M] and incumbents best [E] are
// given, over the first `total` <= 64 outcomes whose word is 1, into inc [E].
__global__ __launch_bounds__(64) void logchebei1_outcome_kernel(const double* const* __restrict__ kg, size_t aa, int M, int K, const CehviTau tau, int cap, int j0, int count, int total, const double* __restrict__ scal, const double* __restrict__ best, double* __restrict__ means, int* __restrict__ mask, double* __restrict__ inc) {
#pragma clang fp contract(off)
  const int e = blockIdx.x, lane = threadIdx.x, G = M + K;
  double* mine = means + (size_t)e * M * cap;
  int* words = mask + (size_t)e * cap;
  for (int idx = lane; idx < M * count; idx += 64) {
    const int j = idx / count, i = idx - j * count;
    if (j0 + i < cap) mine[(size_t)j * cap + j0 + i] = kg[(size_t)e * G + j][aa + i];
  }
  for (int i = lane; i < count; i += 64) {
    int ok = 1;
    for (int k = 0; k < K; ++k) ok &= (kg[(size_t)e * G + M + k][aa + i] <= tau.t[k]) ? 1 : 0;
    if (j0 + i < cap) words[j0 + i] = ok;
  }
  __syncthreads();
  double g = INFINITY;
  if (lane < total && lane < cap) {
    double mx = -INFINITY;
    bool ok = words[lane] != 0;
    for (int j = 0; j < M; ++j) {
      const double prod = scal[j] * mine[(size_t)j * cap + lane];
      const double v = prod + scal[M + j];
      ok = ok && isfinite(v);
      mx = fmax(mx, v);
    }
    if (ok) g = mx;
  }
  for (int off = 32; off > 0; off >>= 1) g = fmin(g, __shfl_xor(g, off, 64));
  if (lane == 0) inc[e] = fmin(best[e], g);
}

// The log node sums (the header's reduction order).  Grid (C, E), one wavefront; kg: the E G sub-members' [mu Cs | var Cs], the
// objectives the first M of every G; scal [2 M] the round's scalarisation, inc [E] its incumbents; vals [E][Cs] takes LA_e and,
// with want_grad, coef [E][Cs][2 M] takes dLA/dmu_0, dLA/dvar_0, ..., dLA/dmu_{M-1}, dLA/dvar_{M-1}.
template <int M>
__global__ __launch_bounds__(64) void logchebei1_node_kernel(int Cs, int G, const double* const* __restrict__ kg, const double* __restrict__ scal, const double* __restrict__ inc, int want_grad, double* __restrict__ vals, double* __restrict__ coef) {
#pragma clang fp contract(off)
  constexpr int NP = kChebBreaks * M;           // the objectives' breakpoints
  constexpr int NB = NP + kLogChebLadder + 2;   // breakpoints
  constexpr int NODES = 8 * (NB - 1);
  static_assert(NB <= 128, "a lane ranks two breakpoints at most");
  __shared__ double s_raw[128], s_sorted[128];
  const int c = blockIdx.x, e = blockIdx.y, lane = threadIdx.x;
  const bool wg = want_grad != 0;
  const size_t o = (size_t)e * Cs + c;
  const double g = inc[e];
  double a[M], dg[M], tau[M], sg[M];  // dg: the offsets g - s_j, each rounded once
  double U = INFINITY, tmax = 0.0, rate = 0.0;
  #pragma unroll
  for (int j = 0; j < M; ++j) {
    const double* r = kg[(size_t)e * G + j];
    const double mu = r[c], var = r[(size_t)Cs + c];
    a[j] = scal[j];
    sg[j] = sqrt(fmax(kMinVarGradEI, var));
    const double s = a[j] * mu + scal[M + j];
    tau[j] = a[j] * sg[j];
    dg[j] = g - s;
    U = fmin(U, dg[j] + 38.0 * tau[j]);  // g - L
    tmax = fmax(tmax, tau[j]);
    double lc, ratio;
    log_cdf_parts(dg[j] / tau[j], lc, ratio);
    const double term = ratio / tau[j];
    rate = (j == 0) ? term : rate + term;
  }
  const double ell = fmin(1.0 / rate, tmax);  // (1 / 0 = infinity yields to the cap)
  U = fmax(U, kLogChebReach * ell);           // g - Lambda > 0
  for (int k = lane; k < NB; k += 64) {
    double v = (k == NB - 2) ? U : 0.0;
    if (k < NP) {
      const int j = k / kChebBreaks, i = k - kChebBreaks * j;
      double dj = 0.0, tj = 0.0;
  #pragma unroll
      for (int q = 0; q < M; ++q) {  // (a select per objective: the offsets and tau stay in registers)
        dj = (q == j) ? dg[q] : dj;
        tj = (q == j) ? tau[q] : tj;
      }
      v = dj + -kChebC[i] * tj;
      v = fmin(fmax(v, 0.0), U);
    } else if (k < NB - 2) {
      v = kLogChebKappa[k - NP] * ell;
      v = fmin(fmax(v, 0.0), U);
    }
    s_raw[k] = v;
  }
  __syncthreads();
  for (int k = lane; k < NB; k += 64) {
    const double v = s_raw[k];
    int rank = 0;
    for (int i = 0; i < NB; ++i) {
      const double u = s_raw[i];
      rank += (u < v || (u == v && i < k)) ? 1 : 0;
    }
    s_sorted[min(rank, NB - 1)] = v;
  }
  __syncthreads();
  LogStripRecord<2 * M> rec;
  rec.m = -INFINITY;
  rec.W = 0.0;
  #pragma unroll
  for (int q = 0; q < 2 * M; ++q) rec.S[q] = 0.0;
  for (int s0 = 0; s0 < NODES; s0 += 64) {
    const int idx = s0 + lane;
    if (idx >= NODES) continue;
    const int panel = idx >> 3, node = idx & 7;
    const double lo = s_sorted[panel], hi = s_sorted[panel + 1];
    const double half = 0.5 * (hi - lo);
    if (!(half > 0.0)) continue;
    const double mid = 0.5 * (lo + hi);
    const double u = mid + half * kChebX[node];
    const double wt = half * kChebW[node];
    double logf = 0.0, dl[2 * M];
  #pragma unroll
    for (int j = 0; j < M; ++j) {
      const double z = (dg[j] - u) / tau[j];
      double lc, ratio;
      log_cdf_parts(z, lc, ratio);
      logf = (j == 0) ? lc : logf + lc;
      const double q = ratio / tau[j];
      dl[2 * j] = q;
      dl[2 * j + 1] = z * q;
    }
    const double l = log(wt) + logf;
    if (!(l > -INFINITY)) continue;  // (a term of weight 0 in float64; a NaN never enters)
    record_take(rec, l, dl, wg);
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) record_merge(rec, off, wg);
  if (lane != 0) return;
  vals[o] = rec.m + log(rec.W);
  if (wg) {
  #pragma unroll
    for (int j = 0; j < M; ++j) {
      coef[2 * M * o + 2 * j] = -a[j] * (rec.S[2 * j] / rec.W);
      coef[2 * M * o + 2 * j + 1] = -(a[j] / (2.0 * sg[j])) * (rec.S[2 * j + 1] / rec.W);
    }
  }
}

// The log-sum-exp over the members, one thread per output element (logehvi3_combine_kernel's shape and rule with 2 M terms,
// instantiated per M): element i < nv of value_out (NULL: nv = 0) is candidate i's value, the elements behind are grad_out's
// (c, j).  la [E][Cs] and coef [E][Cs][2 M]: the log-node kernel's; feas: logehvi1_feas_kernel's; grads: the E (M + K)
// sub-members' [grad mu Cs d | grad var Cs d].  A value thread also leaves its candidate's group values in factors [E][1 + K][Cs].
// Every operation rounded by itself, in the header's order.
template <int M>
__global__ __launch_bounds__(256) void logchebei1_combine_kernel(int E, int K, long C, int Cs, int d, const double* __restrict__ la, const double* __restrict__ coef, const double* __restrict__ feas, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out, double* __restrict__ factors) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  const long k = i - nv, c = (i < nv) ? i : k / d;
  const int G = M + K;
  const size_t gv = (size_t)Cs * d;
  double m = logehvi1_member_log(la, feas, 0, K, Cs, c);
  for (int e = 1; e < E; ++e) m = fmax(m, logehvi1_member_log(la, feas, e, K, Cs, c));
  double W = 0.0, sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double w = exp(logehvi1_member_log(la, feas, e, K, Cs, c) - m);
    W = (e == 0) ? w : W + w;
    if (i < nv) {
      factors[(size_t)e * (1 + K) * Cs + c] = la[(size_t)e * Cs + c];
      for (int q = 0; q < K; ++q) factors[((size_t)e * (1 + K) + 1 + q) * Cs + c] = feas[3 * (((size_t)e * K + q) * Cs + c)];
      continue;
    }
    const double* co = coef + 2 * (size_t)M * ((size_t)e * Cs + c);
    double g = 0.0;
  #pragma unroll
    for (int r = 0; r < M; ++r) {
      const double* gr = grads[(size_t)e * G + r];
      const double tm = co[2 * r] * gr[k];
      g = (r == 0) ? tm : g + tm;
      const double tv = co[2 * r + 1] * gr[gv + k];
      g = g + tv;
    }
    for (int q = 0; q < K; ++q) {
      const double* f = feas + 3 * (((size_t)e * K + q) * Cs + c);
      const double* gq = grads[(size_t)e * G + M + q];
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

// the node kernel over C candidates, then the combine kernel, both instantiated for M (the feasibility kernel has run)
template <int M>
void launch_node_and_combine(const Kg1Ensemble& T, const LogChebLayout& l, double* base, int round, int C, double* value_out, double* grad_out) {
  const bool wg = grad_out != nullptr;
  MOE_LAUNCH_NOW(logchebei1_node_kernel<M>, dim3((unsigned)C, (unsigned)l.E), dim3(64), 0, T.z, l.C, l.M + l.K, T.dKgTab,
                 (const double*)(base + l.oScal + 2 * (size_t)round * l.M), (const double*)(base + l.oInc), wg ? 1 : 0, base + l.oVals,
                 base + l.oCoef);
  const long n = (value_out != nullptr ? (long)C : 0) + (wg ? (long)C * T.d : 0);
  MOE_LAUNCH_NOW(logchebei1_combine_kernel<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, l.E, l.K, (long)C, l.C, T.d,
                 (const double*)(base + l.oVals), (const double*)(base + l.oCoef), (const double*)(base + l.oFeas), T.dGradTab,
                 value_out, grad_out, base + l.oFactors);
}

Kg1Member member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  return ehvi1_member(gp, e % o.group, C, with_grad, fail, pcap, fail_pending);
}

// mu of every sub-member at P_j0 .. j0 + count - 1; the objectives' join the members' outcomes and the constraints' decide the
// members' beliefs; then the incumbents of the round in use over the first j0 + count outcomes
void gather_outcomes(Kg1Ensemble& T, int j0, int count) {
  const LogChebCall& k = *static_cast<const LogChebCall*>(T.client);
  const LogChebLayout l = layout_of(T);
  if (j0 + count > l.cap && count > 0) throw Error(MOE_ERR_RUNTIME, "logchebei1: more pending points than the call has room for");
  double* base = T.gps[0]->ehviD.p;
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  const size_t aa = (size_t)(T.mem[0].dAA - T.mem[0].dKg);  // (one layout for every sub-member: ei1_member's, from C, d and with_grad)
  MOE_LAUNCH_NOW(logchebei1_outcome_kernel, dim3((unsigned)l.E), dim3(64), 0, T.z, T.dKgTab, aa, l.M, l.K, k.tau, l.cap, j0, count,
                 j0 + count, (const double*)(base + l.oScal + 2 * (size_t)k.round * l.M),
                 (const double*)(base + l.oBest + (size_t)k.round * l.E), base + l.oMeans, reinterpret_cast<int*>(base + l.oMask),
                 base + l.oInc);
  MOE_HIP_CHECK(hipGetLastError());
}

// every sub-member's extension stands: the call's own device memory, the caller's scalarisations and incumbents, then the believed
// outcomes of the caller's pending points, the members' beliefs and round 0's incumbents
void all_extended(Kg1Ensemble& T, int p) {
  const LogChebCall& k = *static_cast<const LogChebCall*>(T.client);
  const LogChebLayout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  g0.ehviD.reserve(l.total);
  copy_async(g0.ehviD.p + l.oScal, k.scal, sizeof(double) * 2 * (size_t)l.R * l.M, hipMemcpyHostToDevice, T.z);
  copy_async(g0.ehviD.p + l.oBest, k.best, sizeof(double) * (size_t)l.R * l.E, hipMemcpyHostToDevice, T.z);
  T.dGroupVals = g0.ehviD.p + l.oFactors;
  k.round = 0;
  gather_outcomes(T, 0, p);
}

// a pick joins every sub-member's extension, then its believed outcomes and the beliefs about it every member's list, and the next
// round's scalarisation and incumbents come into use, inside device memory
void pick_appended(Kg1Ensemble& T) {
  const LogChebCall& k = *static_cast<const LogChebCall*>(T.client);
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
  if (k.round + 1 >= k.R) throw Error(MOE_ERR_RUNTIME, "logchebei1: more rounds than scalarisations");
  k.round += 1;
  gather_outcomes(T, T.p, 1);
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  if (value_out == nullptr && grad_out == nullptr) return;
  const LogChebCall& k = *static_cast<const LogChebCall*>(T.client);
  const LogChebLayout l = layout_of(T);
  if (C < 1 || C > l.C) throw Error(MOE_ERR_RUNTIME, "logchebei1: more candidates than the call was staged for");
  double* base = T.gps[0]->ehviD.p;
  if (l.K > 0) {
    const long nf = (long)l.E * l.K * C;
    MOE_LAUNCH_NOW(logehvi1_feas_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, T.z, T.dKgTab, l.E, l.M, l.K, k.tau, C, l.C,
                   grad_out != nullptr ? 1 : 0, base + l.oFeas);
  }
  switch (l.M) {
    case 2: launch_node_and_combine<2>(T, l, base, k.round, C, value_out, grad_out); break;
    case 3: launch_node_and_combine<3>(T, l, base, k.round, C, value_out, grad_out); break;
    case 4: launch_node_and_combine<4>(T, l, base, k.round, C, value_out, grad_out); break;
    case 5: launch_node_and_combine<5>(T, l, base, k.round, C, value_out, grad_out); break;
    case 6: launch_node_and_combine<6>(T, l, base, k.round, C, value_out, grad_out); break;
    case 7: launch_node_and_combine<7>(T, l, base, k.round, C, value_out, grad_out); break;
    case 8: launch_node_and_combine<8>(T, l, base, k.round, C, value_out, grad_out); break;
    default: throw Error(MOE_ERR_RUNTIME, "logchebei1: no kernels for this number of objectives");
  }
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

// No sets, no fidelity coordinates; the drivers' own incumbents are zeros kept by the call (the rounds' incumbents are the
// client's); groups of M + K sub-members under the header's rule, K = 0 included; the groups' own values 1 + K rows each
Kg1Call logchebei1_call(int num_mcmc, int num_objectives, int num_constraints, const double* thresholds, int num_rounds,
                        const double* scalarisations, const double* best_so_far) {
  const int G = num_objectives + num_constraints;
  LogChebCall c = {};
  c.M = num_objectives;
  c.K = num_constraints;
  c.R = num_rounds;
  for (int k = 0; k < num_constraints; ++k) c.tau.t[k] = thresholds[k];
  c.scal = scalarisations;
  c.best = best_so_far;
  Kg1Call call;
  call.doubles.assign((size_t)G * (size_t)num_mcmc, 0.0);
  call.client = std::make_shared<const LogChebCall>(c);
  call.o.best_so_far = call.doubles.data();
  call.o.member = member;
  call.o.eval_points = ehvi1_eval_points;
  call.o.all_extended = all_extended;
  call.o.pick_appended = pick_appended;
  call.o.group = G;
  call.o.combine = combine;
  call.o.client = call.client.get();
  call.o.group_values = true;
  call.o.group_value_rows = 1 + num_constraints;
  call.check_members = ehvi1_check_members;
  return call;
}

void check_logchebei_shapes(int num_objectives, int num_constraints, int num_mcmc) {
  if (num_objectives < kChebMinObjectives || num_objectives > kChebMaxObjectives)
    throw Error(MOE_ERR_BOUNDS, "num_objectives must be between 2 and 8", num_objectives, kChebMinObjectives, kChebMaxObjectives);
  if (num_constraints < 0 || num_constraints > kCeiMaxConstraints)
    throw Error(MOE_ERR_BOUNDS, "num_constraints must be between 0 and 8", num_constraints, 0, kCeiMaxConstraints);
  const int G = num_objectives + num_constraints;
  if (num_mcmc < 1 || (long)num_mcmc * G > 1024)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc must be positive and num_mcmc (num_objectives + num_constraints) at most 1024", num_mcmc, 1,
                1024 / G);
}

void check_logchebei_values(int num_objectives, int num_constraints, int num_mcmc, int num_rounds, const double* scalarisations,
                            const double* thresholds, const double* best_so_far) {
  const int M = num_objectives, R = std::max(num_rounds, 1);
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < 2 * M; ++k) {
      const double v = scalarisations[(size_t)r * 2 * M + k];
      if (!std::isfinite(v) || (k < M && !(v > 0.0)))
        throw Error(MOE_ERR_INVALID_VALUE, "a scalarisation's a_j must be positive and finite, its b_j finite", v, (double)(r * 2 * M + k),
                    0);
    }
  for (int k = 0; k < num_constraints; ++k)
    if (!std::isfinite(thresholds[k])) throw Error(MOE_ERR_INVALID_VALUE, "thresholds must be finite", thresholds[k], k, 2);
  for (int i = 0; i < R * num_mcmc; ++i)
    if (!std::isfinite(best_so_far[i]))
      throw Error(MOE_ERR_INVALID_VALUE, "best_so_far must be finite: the log form's integral needs a finite upper limit", best_so_far[i],
                  (double)i, 1);
}

}  // namespace moe
