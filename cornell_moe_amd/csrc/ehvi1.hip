// cornell_moe_amd/csrc/ehvi1.hip -- the two-objective expected hypervolume improvement (Emmerich, Giannakoglou & Naujoks 2006;
// Emmerich, Deutz & Klinkenberg 2011; Yang et al. 2019) averaged over a hyper-parameter ensemble, with pending points, its
// multistart ascent and greedy q-point batches, on the device (moe_ehvi_mcmc, moe_ehvi_mcmc_multistart, moe_ehvi_mcmc_suggest): a
// client of kg1_ascent.hip's staging, ascent and drivers.  The pending-row extension is kg1_pending.hip's, the
// layout and the pass are ei1.hip's (ei1.hpp); this file keeps a sub-member's candidate kernel and the two-sum gradient kernel
// with its tail, the front kernel, the strip kernel, the combine kernel, the members' check and the description of the call
// (ehvi1_call).  ehvi3.hip, the three-objective form, takes the sub-member's chain, the members' check and psi from here (ehvi1.hpp);
// cehvi1.hip, the constrained form, also the layout and the launches of the front kernel (with its mask) and the strip kernel.
//
// Minimisation.  A call takes E joint hyper-samples; member e is two GPs, objective 1 and objective 2, the 2 E GPs being the
// SUB-MEMBERS of one Kg1Ensemble ordered [e][role].  r = (r1, r2) is the reference point, the front F >= 0 points (u_i, v_i) with
// u_1 < ... < u_F < r1 and r2 > v_1 > ... > v_F; u_0 = -infinity, u_{F+1} = r1, v_0 = r2.  With mu_r, var_r the posterior mean and
// the conditioned latent variance of objective r's GP at x, sigma = sqrt(max(DBL_MIN, var)), sigma_g = sqrt(max(150 eps^2, var)):
//   psi(t) = (t - mu) Phi(z) + sigma phi(z),  z = (t - mu) / sigma,  psi_1(-infinity) = 0
//   d psi / d mu = -Phi(z_g),  d psi / d var = phi(z_g) / (2 sigma_g),  z_g = (t - mu) / sigma_g
//   S_e = sum_{i = 0 .. F} [psi_1(u_{i+1}) - psi_1(u_i)] psi_2(v_i)          strip i: left edge u_i, right edge u_{i+1}, height v_i
//   A_e = max(0, S_e);  where S_e <= 0 the member's four coefficients are 0
//   value = (A_0 + ... + A_{E-1}) / E
//   grad  = (1 / E) sum_e [ dA/dmu_1 grad mu_1 + dA/dvar_1 grad var_1 + dA/dmu_2 grad mu_2 + dA/dvar_2 grad var_2 ]
//
// Sub-member chain (per pass of ei1_pass_size(N) candidates, recordable): ei1.hip's K(X, x), V_x = L^-1 K(X, x), mu(x), the pending
// rows, then ehvi1_cand_kernel -- ei1_cand_kernel's ONE fused multiply-add chain for var -- which leaves mu and var in the member's
// dKg [2][C] and, with a gradient, the column v'_x itself; L'^-T of it (kg1_pending_back, tri_cols 'T') gives w, and
// ehvi1_grad_kernel<DP> walks the rows once with two accumulators, grad mu = sum_r kinvy_r grad_x k(row_r, x) and
// grad var = -2 sum_r w_r grad_x k(row_r, x), into dGrad [2][C][d] (ei1_grad_kernel's reduction: threads stride the rows, the fixed
// butterfly, the four wavefronts' sums as (0 + 1) + (2 + 3)).
//
// Fronts.  Every member keeps its own front in device memory, u [cap] and v [cap] with cap = F + the call's pending room, and its
// count.  ehvi1_front_kernel (one wavefront per member) copies the caller's front and inserts the believed outcomes
// (mu_{e,1}(P_j), mu_{e,2}(P_j)) in the order of j: an outcome joins when it lies strictly inside r and no front point (u, v) has
// u <= a and v <= b; the front points with u >= a and v >= b leave.  A greedy batch's pick joins the same way, inside device memory.
//
// Strip kernel and its REDUCTION ORDER.  One workgroup of four wavefronts per (four candidates, member): the member's front goes to
// LDS once, a wavefront serves one candidate.  Lane l of sweep s owns strip i = 64 s + l: it computes psi_1 and its two derivatives at
// the strip's RIGHT edge once and takes the left edge's from lane l - 1 (lane 0: from lane 63 of the sweep before; zeros for strip
// 0), computes psi_2 and its derivatives at v_i, and adds its strip's five products to five accumulators of its own by fused
// multiply-add, sweep after sweep in ascending s.  Lanes past strip F add nothing.  Then the five accumulators are summed across the
// lanes by the fixed butterfly (xor 32, 16, 8, 4, 2, 1).  The order depends on F alone: not on the candidates that share the launch,
// not on want_grad (the value's accumulator does not see the flag), not on ensemble-wide launches (the kernel is never recorded).
// The combine kernel then forms, with contraction off, ((c_mu1 g_mu1 + c_var1 g_var1) + c_mu2 g_mu2) + c_var2 g_var2 per member and
// coordinate, adds the members in member order and divides once; the value likewise.
//
// Limits: F <= 960 and at most 64 pending points, so cap <= 1024; E <= 512, so 2 E <= 1024; no derivative observations.
// A candidate never raises; only a pending point whose Schur pivot fails does, payload (the flat index 2 e + role, the point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "device_cov.hpp"
#include "ehvi1.hpp"
#include "ei1.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

constexpr int kEhviCap = kEhviMaxFront + kKg1MaxPending;  // a member's front at its largest

Ehvi1Layout layout_of(const Kg1Ensemble& T) {
  const Ehvi1Call& k = *static_cast<const Ehvi1Call*>(T.client);
  return ehvi1_layout(T.E / 2, k.F, T.pcap, T.mem[0].C);
}

// One wavefront per candidate: ei1_cand_kernel's chain for the variance (rows past R add exact zeros).  out [2][Cs]: mu and var of
// candidate col0 + c; with want_grad T takes the column v'_x as it stands.
struct ehvi1_cand_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int R, int ld, int ncols, int col0, int Cs, const CovParams& cp, int want_grad, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ out, double* __restrict__ T) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const double* v = Vx + (size_t)c * ld;
    const double ss = row_chain(v, 0, R, lane, 0.0);
    const double var = radial_scalars(cp.type, cp.alpha, 0.0).base - ss;
    if (lane == 0) {
      out[col0 + c] = mu[c];
      out[(size_t)Cs + col0 + c] = var;
    }
    if (want_grad == 0) return;
    double* tc = T + (size_t)c * ld;
    for (int r = lane; r < R; r += 64) tc[r] = v[r];
  }
};
__global__ __launch_bounds__(256) void ehvi1_cand_kernel(int R, int ld, int ncols, int col0, int Cs, const CovParams cp, int want_grad, const double* __restrict__ mu, const double* __restrict__ Vx, double* __restrict__ out, double* __restrict__ T) {
  ehvi1_cand_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, R, ld, ncols, col0, Cs, cp, want_grad, mu, Vx, out, T);
}

// One workgroup per candidate, ei1_grad_kernel's walk over the R rows of X u P with TWO accumulators: grad mu = sum_r kinvy_r
// grad_x k(row_r, x) and grad var = -2 sum_r u_r grad_x k(row_r, x), u = L'^-T v'_x.  grad [2][Cs][d].
template <int DP>
struct ehvi1_grad_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int R, int ld, int d, int col0, int Cs, const CovParams& cp, const double* __restrict__ X, const double* __restrict__ kinvy, const double* __restrict__ Px, const double* __restrict__ U, double* __restrict__ grad) {
    __shared__ double s_part[2][4][DP];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double* u = U + (size_t)c * ld;
    double x[DP], gm[DP], gv[DP];
  #pragma unroll
    for (int i = 0; i < DP; ++i) {
      x[i] = Px[(size_t)c * DP + i];
      gm[i] = 0.0;
      gv[i] = 0.0;
    }
    for (int r = tid; r < R; r += 256) {
      const double* xr = X + (size_t)r * DP;
      double e[DP], r2 = 0.0;
  #pragma unroll
      for (int i = 0; i < DP; ++i) {
        const double diff = xr[i] - x[i];
        r2 = fma(diff * diff, cp.inv_l2[i], r2);
        e[i] = diff * cp.inv_l2[i];
      }
      const double first = radial_scalars(cp.type, cp.alpha, r2).first;
      const double fm = first * kinvy[r], fv = first * u[r];
  #pragma unroll
      for (int i = 0; i < DP; ++i) {
        gm[i] = fma(fm, e[i], gm[i]);
        gv[i] = fma(fv, e[i], gv[i]);
      }
    }
  #pragma unroll
    for (int i = 0; i < DP; ++i) {
  #pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        gm[i] += __shfl_xor(gm[i], off, 64);
        gv[i] += __shfl_xor(gv[i], off, 64);
      }
    }
    if ((tid & 63) == 0) {
  #pragma unroll
      for (int i = 0; i < DP; ++i) {
        s_part[0][tid >> 6][i] = gm[i];
        s_part[1][tid >> 6][i] = gv[i];
      }
    }
    __syncthreads();
    if (tid < d) {
      const size_t o = (size_t)(col0 + c) * d + tid;
      grad[o] = (s_part[0][0][tid] + s_part[0][1][tid]) + (s_part[0][2][tid] + s_part[0][3][tid]);
      grad[(size_t)Cs * d + o] = -2.0 * ((s_part[1][0][tid] + s_part[1][1][tid]) + (s_part[1][2][tid] + s_part[1][3][tid]));
    }
  }
};
template <int DP>
__global__ __launch_bounds__(256) void ehvi1_grad_kernel(int R, int ld, int d, int col0, int Cs, const CovParams cp, const double* __restrict__ X, const double* __restrict__ kinvy, const double* __restrict__ Px, const double* __restrict__ U, double* __restrict__ grad) {
  ehvi1_grad_kernel_body<DP>::run(MOE_VBLOCK, MOE_VGRID, nullptr, R, ld, d, col0, Cs, cp, X, kinvy, Px, U, grad);
}

// One wavefront per member (blockIdx.x).  kg: the sub-members' dKg, their mu at the pending points `aa` doubles behind.  first != 0:
// the member's front is the caller's [F][2]; otherwise the front as it stands.  Then the believed outcomes of `count` pending points
// join in order under the header's rule.  fronts: [E][2][cap], counts [E].  mask (NULL: every outcome is offered): member e offers
// pending point j only where mask[e mask_ld + j] != 0 (cehvi1.hip's believed feasibility).
__global__ __launch_bounds__(64) void ehvi1_front_kernel(const double* const* __restrict__ kg, size_t aa, const double* __restrict__ caller, int F, double r1, double r2, double* __restrict__ fronts, int cap, int* __restrict__ counts, int first, int count, const int* __restrict__ mask, int mask_ld) {
  const int e = blockIdx.x, lane = threadIdx.x;
  double* u = fronts + (size_t)e * 2 * cap;
  double* v = u + cap;
  int n;
  if (first != 0) {
    for (int i = lane; i < F; i += 64) {
      u[i] = caller[2 * i];
      v[i] = caller[2 * i + 1];
    }
    n = F;
  } else {
    n = counts[e];
  }
  __syncthreads();
  const double* mu1 = kg[2 * e] + aa;
  const double* mu2 = kg[2 * e + 1] + aa;
  for (int j = 0; j < count; ++j) {
    if (mask != nullptr && mask[(size_t)e * mask_ld + j] == 0) continue;  // (the same word for every lane)
    const double a = mu1[j], b = mu2[j];
    if (!(a < r1 && b < r2)) continue;  // (not strictly inside r; NaN included)
    int lo = 0, ev = 0, dom = 0;
    for (int i = lane; i < n; i += 64) {
      const double ui = u[i], vi = v[i];
      lo += (ui < a) ? 1 : 0;
      ev += (ui >= a && vi >= b) ? 1 : 0;
      dom |= (ui <= a && vi <= b) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
      lo += __shfl_xor(lo, off, 64);
      ev += __shfl_xor(ev, off, 64);
      dom |= __shfl_xor(dom, off, 64);
    }
    if (dom != 0) continue;
    // sorted and mutually non-dominated: the points that leave are lo .. lo + ev - 1; those behind move by 1 - ev
    const int shift = 1 - ev, from = lo + ev;
    if (n + shift > cap) continue;  // (cannot happen: cap counts the caller's front and every pending point)
    if (shift != 0) {
      double ru[kEhviCap / 64], rv[kEhviCap / 64];
  #pragma unroll
      for (int k = 0; k < kEhviCap / 64; ++k) {
        const int i = lane + 64 * k;
        const bool mine = i >= from && i < n;
        ru[k] = mine ? u[i] : 0.0;
        rv[k] = mine ? v[i] : 0.0;
      }
      __syncthreads();
  #pragma unroll
      for (int k = 0; k < kEhviCap / 64; ++k) {
        const int i = lane + 64 * k;
        if (i >= from && i < n) {
          u[i + shift] = ru[k];
          v[i + shift] = rv[k];
        }
      }
    }
    if (lane == 0) {
      u[lo] = a;
      v[lo] = b;
    }
    n += shift;
    __syncthreads();
  }
  if (lane == 0) counts[e] = n;
}

// The strip sums (the header's reduction order).  Grid (ceil(C / 4), E), four wavefronts, one candidate each; kg: the sub-members'
// [mu Cs | var Cs]; fronts / counts as ehvi1_front_kernel leaves them; vals [E][Cs] takes A_e and, with want_grad, coef [E][Cs][4]
// takes dA/dmu_1, dA/dvar_1, dA/dmu_2, dA/dvar_2.
__global__ __launch_bounds__(256) void ehvi1_strip_kernel(int C, int Cs, const double* const* __restrict__ kg, const double* __restrict__ fronts, int cap, const int* __restrict__ counts, double r1, double r2, int want_grad, double* __restrict__ vals, double* __restrict__ coef) {
  __shared__ double s_u[kEhviCap], s_v[kEhviCap];
  const int e = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int n = min(counts[e], min(cap, kEhviCap));
  const double* fu = fronts + (size_t)e * 2 * cap;
  const double* fv = fu + cap;
  for (int i = tid; i < n; i += 256) {
    s_u[i] = fu[i];
    s_v[i] = fv[i];
  }
  __syncthreads();
  const int c = blockIdx.x * 4 + (tid >> 6);
  if (c >= C) return;
  const bool wg = want_grad != 0;
  const double mu1 = kg[2 * e][c], var1 = kg[2 * e][(size_t)Cs + c];
  const double mu2 = kg[2 * e + 1][c], var2 = kg[2 * e + 1][(size_t)Cs + c];
  const double sd1 = sqrt(fmax(kMinVarEI, var1)), sg1 = sqrt(fmax(kMinVarGradEI, var1));
  const double sd2 = sqrt(fmax(kMinVarEI, var2)), sg2 = sqrt(fmax(kMinVarGradEI, var2));
  double accA = 0.0, accM1 = 0.0, accV1 = 0.0, accM2 = 0.0, accV2 = 0.0;
  double carryP = 0.0, carryM = 0.0, carryV = 0.0;  // the left edge of strip 0: psi_1(-infinity) = 0
  for (int s0 = 0; s0 <= n; s0 += 64) {
    const int i = s0 + lane;
    const bool active = i <= n;
    double P = 0.0, Pm = 0.0, Pv = 0.0, Q = 0.0, Qm = 0.0, Qv = 0.0;
    if (active) {
      ehvi1_edge(i < n ? s_u[i] : r1, mu1, sd1, sg1, wg, P, Pm, Pv);
      ehvi1_edge(i == 0 ? r2 : s_v[i - 1], mu2, sd2, sg2, wg, Q, Qm, Qv);
    }
    double Lp = __shfl_up(P, 1, 64), Lm = __shfl_up(Pm, 1, 64), Lv = __shfl_up(Pv, 1, 64);
    if (lane == 0) {
      Lp = carryP;
      Lm = carryM;
      Lv = carryV;
    }
    carryP = __shfl(P, 63, 64);
    carryM = __shfl(Pm, 63, 64);
    carryV = __shfl(Pv, 63, 64);
    if (active) {
      const double dP = P - Lp;
      accA = fma(dP, Q, accA);
      if (wg) {
        accM1 = fma(Pm - Lm, Q, accM1);
        accV1 = fma(Pv - Lv, Q, accV1);
        accM2 = fma(dP, Qm, accM2);
        accV2 = fma(dP, Qv, accV2);
      }
    }
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    accA += __shfl_xor(accA, off, 64);
    accM1 += __shfl_xor(accM1, off, 64);
    accV1 += __shfl_xor(accV1, off, 64);
    accM2 += __shfl_xor(accM2, off, 64);
    accV2 += __shfl_xor(accV2, off, 64);
  }
  if (lane != 0) return;
  const bool pos = accA > 0.0;
  const size_t o = (size_t)e * Cs + c;
  vals[o] = pos ? accA : 0.0;
  if (wg) {
    coef[4 * o] = pos ? accM1 : 0.0;
    coef[4 * o + 1] = pos ? accV1 : 0.0;
    coef[4 * o + 2] = pos ? accM2 : 0.0;
    coef[4 * o + 3] = pos ? accV2 : 0.0;
  }
}

// The ensemble's value and gradient from the members' A_e and coefficients, one thread per output element (cei1_combine_kernel's
// shape): element i < nv of value_out (NULL: nv = 0) is candidate i's value, the elements behind are grad_out's (c, j).  grads: the
// sub-members' [grad mu Cs d | grad var Cs d].  Every operation rounded by itself, in the header's order.
__global__ __launch_bounds__(256) void ehvi1_combine_kernel(int E, long C, int Cs, int d, const double* __restrict__ vals, const double* __restrict__ coef, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out) {
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
    const double* co = coef + 4 * ((size_t)e * Cs + c);
    const double* g1 = grads[2 * e];
    const double* g2 = grads[2 * e + 1];
    double a = co[0] * g1[k];
    const double t1 = co[1] * g1[gv + k];
    a = a + t1;
    const double t2 = co[2] * g2[k];
    a = a + t2;
    const double t3 = co[3] * g2[gv + k];
    a = a + t3;
    sum = (e == 0) ? a : sum + a;
  }
  grad_out[k] = sum / (double)E;
}

// ei1.hip's pass with ehvi1_cand_kernel and, in the place of ei1_grad_tail, the two-sum gradient kernel behind the same L'^-T
void cand_step(const Kg1Member& m, int nc, int c0, bool with_grad, hipStream_t s) {
  launch_kernel_ens<ehvi1_cand_kernel_body, 256>(ehvi1_cand_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, m.gp->N + m.p, m.ld,
                                                 nc, c0, m.C, m.gp->cp, with_grad ? 1 : 0, (const double*)m.dMuh, (const double*)m.dVx,
                                                 m.dKg, m.dT);
}

void grad_tail(const Kg1Member& m, const double* Px, int nc, int c0, hipStream_t s) {
  GpDev& gp = *m.gp;
  const int d = gp.d, R = gp.N + m.p, ld = m.ld;
  const double* Xr = m.p > 0 ? m.dXe : gp.dX.p;
  const double* Kr = m.p > 0 ? m.dKe : gp.dKinvY.p;
  if (m.p > 0) kg1_pending_back(m, nc, s);
  tri_cols(gp, 'T', nc, m.dT, ld, m.dU, ld, s);
  dispatch_dp(gp.dp, [&](auto DP) {
    launch_kernel_ens<ehvi1_grad_kernel_body<DP>, 256>(ehvi1_grad_kernel<DP>, dim3((unsigned)nc), dim3(256), 0, s, R, ld, d, c0, m.C, gp.cp,
                                                       Xr, Kr, Px, (const double*)m.dU, m.dGrad);
  });
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

Ehvi1Layout ehvi1_layout(int E, int F, int pcap, int C) {
  Ehvi1Layout l;
  l.E = E;
  l.F = F;
  l.cap = std::max(1, F + pcap);
  l.C = C;
  l.oCaller = 0;
  l.oFront = l.oCaller + 2 * (size_t)std::max(1, F);
  l.oCount = l.oFront + 2 * (size_t)l.E * l.cap;
  l.oVals = l.oCount + (size_t)l.E;  // (the counts are integers in the front halves of E doubles' room)
  l.oCoef = l.oVals + (size_t)l.E * l.C;
  l.total = l.oCoef + 4 * (size_t)l.E * l.C;
  return l;
}

void ehvi1_launch_front(const Ehvi1Call& k, const Ehvi1Layout& l, double* base, const double* const* kg, size_t aa, const int* mask,
                        int mask_ld, bool first, int count, hipStream_t s) {
  MOE_LAUNCH_NOW(ehvi1_front_kernel, dim3((unsigned)l.E), dim3(64), 0, s, kg, aa, (const double*)(base + l.oCaller), l.F, k.r1, k.r2,
                 base + l.oFront, l.cap, reinterpret_cast<int*>(base + l.oCount), first ? 1 : 0, count, mask, mask_ld);
  MOE_HIP_CHECK(hipGetLastError());
}

void ehvi1_launch_strip(const Ehvi1Call& k, const Ehvi1Layout& l, double* base, const double* const* kg, int C, bool want_grad,
                        hipStream_t s) {
  MOE_LAUNCH_NOW(ehvi1_strip_kernel, dim3((unsigned)((C + 3) / 4), (unsigned)l.E), dim3(256), 0, s, C, l.C, kg,
                 (const double*)(base + l.oFront), l.cap, reinterpret_cast<const int*>(base + l.oCount), k.r1, k.r2, want_grad ? 1 : 0,
                 base + l.oVals, base + l.oCoef);
}

void ehvi1_eval_points(const Kg1Member& m, const double* Px, const double*, int C, bool with_grad, hipStream_t s) {
  ei1_eval_passes(m, Px, C, with_grad, s, "ehvi1_eval_pass", cand_step, grad_tail);
}

Kg1Member ehvi1_member(GpDev& gp, int role, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  Kg1Member m = ei1_member(gp, C, 0.0, with_grad, fail, pcap, fail_pending, 2);
  m.role = role;
  return m;
}

namespace {

Kg1Member member(const Kg1Objective&, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  return ehvi1_member(gp, e % 2, C, with_grad, fail, pcap, fail_pending);
}

// mu of every sub-member at P_j0 .. j0 + count - 1, then every member's front takes the believed outcomes
void join_believed_outcomes(Kg1Ensemble& T, int j0, int count, bool first) {
  const Ehvi1Call& k = *static_cast<const Ehvi1Call*>(T.client);
  const Ehvi1Layout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  const size_t aa = (size_t)(T.mem[0].dAA - T.mem[0].dKg);  // (one layout for every sub-member: ei1_member's, from C, d and with_grad)
  ehvi1_launch_front(k, l, g0.ehviD.p, T.dKgTab, aa, nullptr, 0, first, count, T.z);
}

// every sub-member's extension stands: the call's own device memory, the caller's front, then the members' fronts
void all_extended(Kg1Ensemble& T, int p) {
  const Ehvi1Call& k = *static_cast<const Ehvi1Call*>(T.client);
  const Ehvi1Layout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  g0.ehviD.reserve(l.total);
  if (k.F > 0) copy_async(g0.ehviD.p + l.oCaller, k.front, sizeof(double) * 2 * (size_t)k.F, hipMemcpyHostToDevice, T.z);
  T.dGroupVals = g0.ehviD.p + l.oVals;
  join_believed_outcomes(T, 0, p, true);
}

// a pick joins every sub-member's extension, then its believed outcome every member's front, inside device memory
void pick_appended(Kg1Ensemble& T) {
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
  join_believed_outcomes(T, T.p, 1, false);
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  if (value_out == nullptr && grad_out == nullptr) return;
  const Ehvi1Call& k = *static_cast<const Ehvi1Call*>(T.client);
  const Ehvi1Layout l = layout_of(T);
  if (C < 1 || C > l.C) throw Error(MOE_ERR_RUNTIME, "ehvi1: more candidates than the call was staged for");
  double* base = T.gps[0]->ehviD.p;
  ehvi1_launch_strip(k, l, base, T.dKgTab, C, grad_out != nullptr, T.z);
  const long n = (value_out != nullptr ? (long)C : 0) + (grad_out != nullptr ? (long)C * T.d : 0);
  MOE_LAUNCH_NOW(ehvi1_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, l.E, (long)C, l.C, T.d,
                 (const double*)(base + l.oVals), (const double*)(base + l.oCoef), T.dGradTab, value_out, grad_out);
  MOE_HIP_CHECK(hipGetLastError());
}

void check_member(const GpDev& g, const GpDev&, size_t e, int) {
  if (g.g != 0)
    throw Error(MOE_ERR_INVALID_VALUE, "the expected hypervolume improvement takes GPs without derivative observations", g.g, 0,
                (double)e);
}

}  // namespace

void ehvi1_check_members(const Kg1Objective&, const std::vector<GpDev*>& gps, int pending_room) {
  kg1_check_members(gps, 0, check_member);
  if (pending_room > kKg1MaxPending)
    throw Error(MOE_ERR_BOUNDS, "pending points (num_being_sampled + num_to_sample - 1) must fit 64 extension rows", pending_room, 0,
                kKg1MaxPending);
}

// No sets, no fidelity coordinates, no incumbents (the members' best values are zeros, kept by the call); groups of two sub-members
// under the strip rule, the members' own values kept
Kg1Call ehvi1_call(int num_mcmc, const double* reference_point, const double* front, int num_front) {
  Kg1Call call;
  call.doubles.assign(2 * (size_t)num_mcmc, 0.0);
  call.client = std::make_shared<const Ehvi1Call>(Ehvi1Call{front, num_front, reference_point[0], reference_point[1]});
  call.o.best_so_far = call.doubles.data();
  call.o.member = member;
  call.o.eval_points = ehvi1_eval_points;
  call.o.all_extended = all_extended;
  call.o.pick_appended = pick_appended;
  call.o.group = 2;
  call.o.combine = combine;
  call.o.client = call.client.get();
  call.o.group_values = true;
  call.check_members = ehvi1_check_members;
  return call;
}

void check_ehvi_num_mcmc(int num_mcmc) {
  if (num_mcmc < 1 || num_mcmc > kEhviMaxMembers)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc must be between 1 and 512 (two GPs per member)", num_mcmc, 1, kEhviMaxMembers);
}

void check_ehvi_front(const double* reference_point, const double* front, int num_front) {
  if (num_front < 0 || num_front > kEhviMaxFront)
    throw Error(MOE_ERR_BOUNDS, "num_front must be between 0 and 960", num_front, 0, kEhviMaxFront);
  if (num_front > 0 && front == nullptr) throw Error(MOE_ERR_RUNTIME, "front is NULL with num_front > 0");
  for (int r = 0; r < 2; ++r)
    if (!std::isfinite(reference_point[r]))
      throw Error(MOE_ERR_INVALID_VALUE, "reference_point must be finite", reference_point[r], r, 0);
  for (int i = 0; i < num_front; ++i) {
    const double u = front[2 * i], v = front[2 * i + 1];
    const bool ok = std::isfinite(u) && std::isfinite(v) && u < reference_point[0] && v < reference_point[1] &&
                    (i == 0 || (front[2 * i - 2] < u && front[2 * i - 1] > v));
    if (!ok)
      throw Error(MOE_ERR_INVALID_VALUE,
                  "front must be finite, strictly inside reference_point, sorted by the first objective ascending and mutually "
                  "non-dominated (the second objective descending)",
                  i, 0, 0);
  }
}

}  // namespace moe
