// cornell_moe_amd/csrc/chebei1.hip -- the Chebyshev-scalarised expected improvement for 2 to 8 objectives (ParEGO, Knowles 2006; the
// one-point analytic form of qParEGO, Daulton, Balandat & Bakshy 2020) averaged over a hyper-parameter ensemble, with pending points,
// its multistart ascent and greedy q-point batches with a scalarisation per point, on the device (moe_ei_chebyshev_mcmc,
// moe_ei_chebyshev_mcmc_multistart, moe_ei_chebyshev_mcmc_suggest): the twelfth client of kg1_ascent.hip's staging, ascent and
// drivers.  The sub-member's chain and the members' check are ehvi1.hip's (ehvi1.hpp); this file keeps the outcome kernel, the node
// kernel, the combine kernel and the description of the call (chebei1_call).
//
// Minimisation.  A call takes E joint hyper-samples; member e is M GPs, one per objective, the E M GPs being the SUB-MEMBERS of one
// Kg1Ensemble ordered [e][objective].  A scalarisation is a_j > 0 and b_j, j = 0 .. M - 1.  With mu_j, var_j the posterior mean and
// the conditioned latent variance of GP j at x and ONE floor for value and gradient (logcei1.hip's), sigma_j = sqrt(max(150 eps^2,
// var_j)):
//   s_j = a_j mu_j + b_j (product and sum each rounded),  tau_j = a_j sigma_j,  L = max_j (s_j - 38 tau_j),  z_j(t) = (t - s_j) / tau_j
//   A_e   = E[(g*_e - max_j (a_j Y_j + b_j))^+] = integral over L <= t <= g*_e of prod_j Phi(z_j);  0 with zero coefficients where
//           g*_e <= L (below L the integrand is under 1e-300: L is a constant in the gradient)
//   dA/dmu_j  = -a_j integral phi(z_j) / tau_j prod_{k != j} Phi(z_k)
//   dA/dvar_j = -(a_j / (2 sigma_j)) integral z_j phi(z_j) / tau_j prod_{k != j} Phi(z_k)
//   value = (A_0 + ... + A_{E-1}) / E
//   grad  = (1 / E) sum_e sum_j [ dA/dmu_j grad mu_j + dA/dvar_j grad var_j ]
//
// The quadrature is FIXED.  Breakpoints: position 14 j + i holds s_j + c_i tau_j (product and sum each rounded) clamped to
// [L, g*_e], c = {-38, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8}; position 14 M holds L, position 14 M + 1 holds g*_e.  They are
// sorted ascending, ties by position: 14 M + 2 points, 14 M + 1 panels.  Panel [lo, hi] has half = (hi - lo) / 2, mid = (lo + hi) / 2
// and the 8 nodes t = mid + half x_k (product and sum each rounded) with the weights half w_k of the Gauss-Legendre rule; a panel
// with half = 0 is skipped, an exact 0.
//
// Outcomes.  Every member keeps the believed outcomes mu_{e,j}(P_i) [M][pcap] of the pending points in device memory -- not a scalar,
// because the scalarisation changes from round to round of a greedy batch.  chebei1_outcome_kernel (one wavefront per member) gathers
// the means the set phase or a pick has left behind the sub-members' results and forms the round's incumbent
//   g*_e = min(best_so_far[t][e], min_i max_j (a_{t,j} mu_{e,j}(P_i) + b_{t,j}))
// over the pending points in use whose scalarised outcome is finite (product and sum each rounded; the minimum by the fixed
// butterfly).  No host round trip.
//
// Node kernel and its REDUCTION ORDER.  One wavefront per (candidate, member), instantiated per M so that everything indexed by j
// lives in registers.  The lanes form the 14 M + 2 breakpoints in LDS, two per lane at most, and rank them by counting.  Lane l of
// sweep s owns node 64 s + l: panel (64 s + l) / 8, node (64 s + l) mod 8; at most 15 sweeps.  Per node the lane computes M erfc,
// the product of the Phi_j in the order of j, and adds weight x product to its own accumulator of A by fused multiply-add; with a
// gradient also M exp, the prefix and suffix products, and 2 M more fused accumulations.  Sweeps ascend; lanes past the last node
// add nothing.  The 1 + 2 M accumulators are summed by the fixed butterfly (xor 32, 16, 8, 4, 2, 1).  The order depends on M alone:
// not on the candidates that share the launch (one wavefront each), not on want_grad (the value's accumulator does not see the
// flag), not on the pass boundary, not on ensemble-wide launches (the outcome, node and combine kernels are never recorded).
// The combine kernel then forms, with contraction off, sum_j (c_mu_j g_mu_j + c_var_j g_var_j) in the order of j, mu before var,
// per member and coordinate, adds the members in member order and divides once; the value likewise.
//
// Limits: 2 <= M <= 8, E M <= 1024, at most 64 pending points, no derivative observations.  A candidate never raises; only a
// pending point whose Schur pivot fails does, payload (the flat index e M + j, the point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "chebei1.hpp"
#include "ehvi1.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

// the call's record: the caller's arrays and the round in use (a greedy batch's pick moves it on)
struct ChebCall {
  int M, R;
  const double* scal;  // [R][2 M]
  const double* best;  // [R][E]
  mutable int round;
};

// where the call's own device memory lies inside the first GP's ehviD, in doubles: E members of M GPs, R rounds, room for pcap
// pending points, C staged candidates
struct ChebLayout {
  int E, M, R, cap, C;
  size_t oScal, oBest, oMeans, oInc, oVals, oCoef, total;
};

ChebLayout layout_of(const Kg1Ensemble& T) {
  const ChebCall& k = *static_cast<const ChebCall*>(T.client);
  ChebLayout l;
  l.M = k.M;
  l.R = k.R;
  l.E = T.E / k.M;
  l.cap = std::max(1, T.pcap);
  l.C = T.mem[0].C;
  l.oScal = 0;
  l.oBest = l.oScal + 2 * (size_t)l.R * l.M;
  l.oMeans = l.oBest + (size_t)l.R * l.E;
  l.oInc = l.oMeans + (size_t)l.E * l.M * l.cap;
  l.oVals = l.oInc + (size_t)l.E;
  l.oCoef = l.oVals + (size_t)l.E * l.C;
  l.total = l.oCoef + 2 * (size_t)l.M * l.E * l.C;
  return l;
}

// One wavefront per member (blockIdx.x).  kg: the sub-members' dKg, their mu at `count` pending points `aa` doubles behind; they go
// to places j0 .. j0 + count - 1 of the member's outcomes means [E][M][cap].  Then the incumbent of the round whose scalarisation
// scal [2 M] and incumbents best [E] are given, over the first `total` <= 64 outcomes, into inc [E].
__global__ __launch_bounds__(64) void chebei1_outcome_kernel(const double* const* __restrict__ kg, size_t aa, int M, int cap, int j0, int count, int total, const double* __restrict__ scal, const double* __restrict__ best, double* __restrict__ means, double* __restrict__ inc) {
#pragma clang fp contract(off)
  const int e = blockIdx.x, lane = threadIdx.x;
  double* mine = means + (size_t)e * M * cap;
  for (int idx = lane; idx < M * count; idx += 64) {
    const int j = idx / count, i = idx - j * count;
    if (j0 + i < cap) mine[(size_t)j * cap + j0 + i] = kg[(size_t)e * M + j][aa + i];
  }
  __syncthreads();
  double g = INFINITY;
  if (lane < total && lane < cap) {
    double mx = -INFINITY;
    bool ok = true;
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

// The node sums (the header's reduction order).  Grid (C, E), one wavefront; kg: the sub-members' [mu Cs | var Cs]; scal [2 M] the
// round's scalarisation, inc [E] its incumbents; vals [E][Cs] takes A_e and, with want_grad, coef [E][Cs][2 M] takes dA/dmu_0,
// dA/dvar_0, ..., dA/dmu_{M-1}, dA/dvar_{M-1}.
template <int M>
__global__ __launch_bounds__(64) void chebei1_node_kernel(int Cs, const double* const* __restrict__ kg, const double* __restrict__ scal, const double* __restrict__ inc, int want_grad, double* __restrict__ vals, double* __restrict__ coef) {
  constexpr int NB = kChebBreaks * M + 2;  // breakpoints
  constexpr int NODES = 8 * (NB - 1);
  static_assert(NB <= 128, "a lane ranks two breakpoints at most");
  __shared__ double s_raw[128], s_sorted[128];
  const int c = blockIdx.x, e = blockIdx.y, lane = threadIdx.x;
  const bool wg = want_grad != 0;
  const size_t o = (size_t)e * Cs + c;
  double a[M], s[M], tau[M], sg[M];
  double L = -INFINITY;
  #pragma unroll
  for (int j = 0; j < M; ++j) {
    const double* r = kg[(size_t)e * M + j];
    const double mu = r[c], var = r[(size_t)Cs + c];
    a[j] = scal[j];
    sg[j] = sqrt(fmax(kMinVarGradEI, var));
    s[j] = radd(rmul(a[j], mu), scal[M + j]);
    tau[j] = rmul(a[j], sg[j]);
    L = fmax(L, radd(s[j], rmul(-38.0, tau[j])));
  }
  const double g = inc[e];
  if (!(g > L)) {  // (the same for every lane)
    if (lane == 0) vals[o] = 0.0;
    if (wg && lane < 2 * M) coef[2 * M * o + lane] = 0.0;
    return;
  }
  for (int k = lane; k < NB; k += 64) {
    double v = (k == kChebBreaks * M) ? L : g;
    if (k < kChebBreaks * M) {
      const int j = k / kChebBreaks, i = k - kChebBreaks * j;
      double sj = 0.0, tj = 0.0;
  #pragma unroll
      for (int q = 0; q < M; ++q) {  // (a select per objective: s and tau stay in registers)
        sj = (q == j) ? s[q] : sj;
        tj = (q == j) ? tau[q] : tj;
      }
      v = radd(sj, rmul(kChebC[i], tj));
      v = fmin(fmax(v, L), g);
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
  double accA = 0.0, accM[M], accV[M];
  #pragma unroll
  for (int j = 0; j < M; ++j) {
    accM[j] = 0.0;
    accV[j] = 0.0;
  }
  for (int s0 = 0; s0 < NODES; s0 += 64) {
    const int idx = s0 + lane;
    if (idx >= NODES) continue;
    const int panel = idx >> 3, node = idx & 7;
    const double lo = s_sorted[panel], hi = s_sorted[panel + 1];
    const double half = rmul(0.5, radd(hi, -lo));
    if (!(half > 0.0)) continue;
    const double mid = rmul(0.5, radd(lo, hi));
    const double t = radd(mid, rmul(half, kChebX[node]));
    const double wt = rmul(half, kChebW[node]);
    double z[M], cdf[M];
  #pragma unroll
    for (int j = 0; j < M; ++j) {
      z[j] = (t - s[j]) / tau[j];
      cdf[j] = normal_cdf(z[j]);
    }
    double P = cdf[0];
  #pragma unroll
    for (int j = 1; j < M; ++j) P = rmul(P, cdf[j]);
    accA = fma(wt, P, accA);
    if (wg) {
      double others[M];  // prod_{k != j} Phi(z_k): the prefix times the suffix
      double run = 1.0;
  #pragma unroll
      for (int j = 0; j < M; ++j) {
        others[j] = run;
        run = rmul(run, cdf[j]);
      }
      run = 1.0;
  #pragma unroll
      for (int j = M - 1; j >= 0; --j) {
        others[j] = rmul(others[j], run);
        run = rmul(run, cdf[j]);
      }
  #pragma unroll
      for (int j = 0; j < M; ++j) {
        const double dens = rmul(normal_pdf(z[j]) / tau[j], others[j]);
        accM[j] = fma(wt, dens, accM[j]);
        accV[j] = fma(wt, rmul(z[j], dens), accV[j]);
      }
    }
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    accA += __shfl_xor(accA, off, 64);
  #pragma unroll
    for (int j = 0; j < M; ++j) {
      accM[j] += __shfl_xor(accM[j], off, 64);
      accV[j] += __shfl_xor(accV[j], off, 64);
    }
  }
  if (lane != 0) return;
  vals[o] = accA;
  if (wg) {
  #pragma unroll
    for (int j = 0; j < M; ++j) {
      coef[2 * M * o + 2 * j] = rmul(-a[j], accM[j]);
      coef[2 * M * o + 2 * j + 1] = rmul(-(a[j] / (2.0 * sg[j])), accV[j]);
    }
  }
}

// The ensemble's value and gradient from the members' A_e and coefficients, one thread per output element (ehvi3_combine_kernel's
// shape with 2 M terms, instantiated per M so that a member's 2 M loads are issued together): element i < nv of value_out (NULL: nv = 0) is candidate i's value, the elements behind are grad_out's
// (c, j).  grads: the sub-members' [grad mu Cs d | grad var Cs d].  Every operation rounded by itself, in the header's order.
template <int M>
__global__ __launch_bounds__(256) void chebei1_combine_kernel(int E, long C, int Cs, int d, const double* __restrict__ vals, const double* __restrict__ coef, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  if (i < nv) {
    double sum = 0.0;
    for (int e = 0; e < E; ++e) {
      const double a = vals[(size_t)e * Cs + i];
      sum = (e == 0) ? a : sum + a;
    }
    value_out[i] = sum / (double)E;
    return;
  }
  const long k = i - nv, c = k / d;
  const size_t gv = (size_t)Cs * d;
  double sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double* co = coef + 2 * (size_t)M * ((size_t)e * Cs + c);
    double a = 0.0;
  #pragma unroll
    for (int r = 0; r < M; ++r) {
      const double* g = grads[(size_t)e * M + r];
      const double tm = co[2 * r] * g[k];
      a = (r == 0) ? tm : a + tm;
      const double tv = co[2 * r + 1] * g[gv + k];
      a = a + tv;
    }
    sum = (e == 0) ? a : sum + a;
  }
  grad_out[k] = sum / (double)E;
}

// the node kernel over C candidates, then the combine kernel, both instantiated for M
template <int M>
void launch_node_and_combine(const Kg1Ensemble& T, const ChebLayout& l, double* base, int round, int C, double* value_out, double* grad_out) {
  const bool want_grad = grad_out != nullptr;
  MOE_LAUNCH_NOW(chebei1_node_kernel<M>, dim3((unsigned)C, (unsigned)l.E), dim3(64), 0, T.z, l.C, T.dKgTab,
                 (const double*)(base + l.oScal + 2 * (size_t)round * l.M), (const double*)(base + l.oInc), want_grad ? 1 : 0,
                 base + l.oVals, base + l.oCoef);
  const long n = (value_out != nullptr ? (long)C : 0) + (want_grad ? (long)C * T.d : 0);
  MOE_LAUNCH_NOW(chebei1_combine_kernel<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, l.E, (long)C, l.C, T.d,
                 (const double*)(base + l.oVals), (const double*)(base + l.oCoef), T.dGradTab, value_out, grad_out);
}

Kg1Member member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  const ChebCall& k = *static_cast<const ChebCall*>(o.client);
  return ehvi1_member(gp, e % k.M, C, with_grad, fail, pcap, fail_pending);
}

// mu of every sub-member at P_j0 .. j0 + count - 1 joins the members' outcomes; then the incumbents of the round in use over the
// first j0 + count outcomes
void gather_outcomes(Kg1Ensemble& T, int j0, int count) {
  const ChebCall& k = *static_cast<const ChebCall*>(T.client);
  const ChebLayout l = layout_of(T);
  double* base = T.gps[0]->ehviD.p;
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  const size_t aa = (size_t)(T.mem[0].dAA - T.mem[0].dKg);  // (one layout for every sub-member: ei1_member's, from C, d and with_grad)
  MOE_LAUNCH_NOW(chebei1_outcome_kernel, dim3((unsigned)l.E), dim3(64), 0, T.z, T.dKgTab, aa, l.M, l.cap, j0, count, j0 + count,
                 (const double*)(base + l.oScal + 2 * (size_t)k.round * l.M), (const double*)(base + l.oBest + (size_t)k.round * l.E),
                 base + l.oMeans, base + l.oInc);
  MOE_HIP_CHECK(hipGetLastError());
}

// every sub-member's extension stands: the call's own device memory, the caller's scalarisations and incumbents, then the believed
// outcomes of the caller's pending points and round 0's incumbents
void all_extended(Kg1Ensemble& T, int p) {
  const ChebCall& k = *static_cast<const ChebCall*>(T.client);
  const ChebLayout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  g0.ehviD.reserve(l.total);
  copy_async(g0.ehviD.p + l.oScal, k.scal, sizeof(double) * 2 * (size_t)l.R * l.M, hipMemcpyHostToDevice, T.z);
  copy_async(g0.ehviD.p + l.oBest, k.best, sizeof(double) * (size_t)l.R * l.E, hipMemcpyHostToDevice, T.z);
  T.dGroupVals = g0.ehviD.p + l.oVals;
  k.round = 0;
  gather_outcomes(T, 0, p);
}

// a pick joins every sub-member's extension, then its believed outcomes every member's list, and the next round's scalarisation
// and incumbents come into use, inside device memory
void pick_appended(Kg1Ensemble& T) {
  const ChebCall& k = *static_cast<const ChebCall*>(T.client);
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
  if (k.round + 1 >= k.R) throw Error(MOE_ERR_RUNTIME, "chebei1: more rounds than scalarisations");
  k.round += 1;
  gather_outcomes(T, T.p, 1);
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  if (value_out == nullptr && grad_out == nullptr) return;
  const ChebCall& k = *static_cast<const ChebCall*>(T.client);
  const ChebLayout l = layout_of(T);
  if (C < 1 || C > l.C) throw Error(MOE_ERR_RUNTIME, "chebei1: more candidates than the call was staged for");
  double* base = T.gps[0]->ehviD.p;
  switch (l.M) {
    case 2: launch_node_and_combine<2>(T, l, base, k.round, C, value_out, grad_out); break;
    case 3: launch_node_and_combine<3>(T, l, base, k.round, C, value_out, grad_out); break;
    case 4: launch_node_and_combine<4>(T, l, base, k.round, C, value_out, grad_out); break;
    case 5: launch_node_and_combine<5>(T, l, base, k.round, C, value_out, grad_out); break;
    case 6: launch_node_and_combine<6>(T, l, base, k.round, C, value_out, grad_out); break;
    case 7: launch_node_and_combine<7>(T, l, base, k.round, C, value_out, grad_out); break;
    case 8: launch_node_and_combine<8>(T, l, base, k.round, C, value_out, grad_out); break;
    default: throw Error(MOE_ERR_RUNTIME, "chebei1: no kernels for this number of objectives");
  }
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

// No sets, no fidelity coordinates; the drivers' own incumbents are zeros kept by the call (the rounds' incumbents are the
// client's); groups of M sub-members under the quadrature, the members' own values kept
Kg1Call chebei1_call(int num_mcmc, int num_objectives, int num_rounds, const double* scalarisations, const double* best_so_far) {
  Kg1Call call;
  call.doubles.assign((size_t)num_objectives * (size_t)num_mcmc, 0.0);
  call.client = std::make_shared<const ChebCall>(ChebCall{num_objectives, num_rounds, scalarisations, best_so_far, 0});
  call.o.best_so_far = call.doubles.data();
  call.o.member = member;
  call.o.eval_points = ehvi1_eval_points;
  call.o.all_extended = all_extended;
  call.o.pick_appended = pick_appended;
  call.o.group = num_objectives;
  call.o.combine = combine;
  call.o.client = call.client.get();
  call.o.group_values = true;
  call.check_members = ehvi1_check_members;
  return call;
}

void check_chebei_objectives(int num_objectives, int num_mcmc) {
  if (num_objectives < kChebMinObjectives || num_objectives > kChebMaxObjectives)
    throw Error(MOE_ERR_BOUNDS, "num_objectives must be between 2 and 8", num_objectives, kChebMinObjectives, kChebMaxObjectives);
  if (num_mcmc < 1 || (long)num_mcmc * num_objectives > 1024)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc must be positive and num_mcmc num_objectives at most 1024", num_mcmc, 1,
                1024 / num_objectives);
}

void check_chebei_values(int num_objectives, int num_mcmc, int num_rounds, const double* scalarisations, const double* best_so_far) {
  const int M = num_objectives, R = std::max(num_rounds, 1);
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < 2 * M; ++k) {
      const double v = scalarisations[(size_t)r * 2 * M + k];
      if (!std::isfinite(v) || (k < M && !(v > 0.0)))
        throw Error(MOE_ERR_INVALID_VALUE, "a scalarisation's a_j must be positive and finite, its b_j finite", v, (double)(r * 2 * M + k),
                    0);
    }
  for (int i = 0; i < R * num_mcmc; ++i)
    if (!std::isfinite(best_so_far[i]))
      throw Error(MOE_ERR_INVALID_VALUE, "best_so_far must be finite", best_so_far[i], (double)i, 1);
}

}  // namespace moe
