// cornell_moe_amd/csrc/ehvi3.hip -- the three-objective expected hypervolume improvement averaged over a hyper-parameter ensemble,
// with pending points, its multistart ascent and greedy q-point batches, on the device (moe_ehvi3_mcmc, moe_ehvi3_mcmc_multistart,
// moe_ehvi3_mcmc_suggest): the seventh client of kg1_ascent.hip's staging, ascent and drivers.  The sub-member's chain, the members'
// check and psi are ehvi1.hip's (ehvi1.hpp); this file keeps the front kernel, the table kernel, the box kernel, the combine kernel
// and the description of the call (ehvi3_call).  cehvi1.hip, the constrained form, takes the layout and the launches of the front
// kernel (with its mask), the table kernel and the box kernel from here (ehvi3.hpp).
//
// Minimisation.  A call takes E joint hyper-samples; member e is three GPs, one per objective, the 3 E GPs being the SUB-MEMBERS of
// one Kg1Ensemble ordered [e][objective].  r = (r1, r2, r3) is the reference point, the member's front n >= 0 mutually non-dominated
// points (u_i, v_i, w_i) strictly inside r in the CANONICAL ORDER: w ascending, ties by u, then by v.  psi_k, sigma, sigma_g and both
// variance floors are ehvi1.hip's.  With w_0 = -infinity and w_{n+1} = r3, the non-dominated part of (-infinity, r] between w_k and
// w_{k+1} has the two-dimensional non-dominated region of the first k points' (u, v) projections as its cross-section:
//   S2_k  = sum over the strips of the staircase of points 1 .. k in (u, v) of [psi_1(right) - psi_1(left)] psi_2(height)
//   S_e   = sum_{k = 0 .. n} S2_k [psi_3(w_{k+1}) - psi_3(w_k)]
//   A_e   = max(0, S_e);  where S_e <= 0 the member's six coefficients are 0
//   value = (A_0 + ... + A_{E-1}) / E
//   grad  = (1 / E) sum_e sum_k [ dA/dmu_k grad mu_k + dA/dvar_k grad var_k ]
// A slab of zero thickness (w_k = w_{k+1}) keeps its boxes and contributes an exact 0.
//
// Fronts.  Every member keeps u [cap], v [cap], w [cap] and a count in device memory, cap = F + the call's pending room.
// ehvi3_front_kernel (one wavefront per member) copies the caller's front and inserts the believed outcomes (mu_{e,1}, mu_{e,2},
// mu_{e,3})(P_j) in the order of j: an outcome joins when it is finite, strictly inside r, and no front point is <= it in all three
// objectives; the front points >= it in all three leave; the canonical order is kept.  A greedy batch's pick joins the same way.
//
// Table.  ehvi3_table_kernel (one workgroup per member) runs after every change of the fronts -- once in the set phase, once per
// greedy round, never per ascent step -- and writes the member's boxes SLAB-MAJOR: slab k = 0 .. n in turn, inside a slab the
// staircase's strips in ascending u.  A box is four 16-bit indices (8 bytes) into the member's edge lists, where index 0 is
// -infinity, 1 .. n the member's points and n + 1 the reference point: the u edge on its left, the u edge on its right, the v edge
// of its height, and its slab k (whose w edges are k and k + 1).  B <= (n + 1)(n + 2) / 2.  The staircase of slab k is that of slab
// k - 1 with point k added (it leaves as it came if a projection before it is <= it in both u and v, otherwise the projections it
// is <= to leave), its order a count per point: O(cap^2) per thread-parallel slab, O(cap^3) in all.
//
// Box kernel and its REDUCTION ORDER.  One workgroup of four wavefronts per (candidate, member).  The threads first form psi_k and
// its two derivatives at every edge of the three objectives -- one erfc and one exp each, 3 (n + 2) in all -- and leave them in LDS
// (3 x 3 x 258 doubles).  Then thread t of sweep s owns box b = 256 s + t of the table: with P = psi_1(right) - psi_1(left),
// Q = psi_2(height), W = psi_3(w_{k+1}) - psi_3(w_k) it adds fma(P Q, W, .) to its own accumulator of A, the product P Q rounded by
// itself, and likewise the six coefficients' terms ((dP Q) W, (P dQ) W, (P Q) dW), sweep after sweep in ascending s.  Threads past
// B add nothing.  The seven accumulators are summed across each wavefront by the fixed butterfly (xor 32, 16, 8, 4, 2, 1) and the
// four wavefronts' sums as (0 + 1) + (2 + 3).  The order depends on the member's table alone: not on the candidates that share the
// launch (one workgroup each), not on want_grad (the value's accumulator does not see the flag), not on the pass boundary, not on
// ensemble-wide launches (the front, table, box and combine kernels are never recorded).  With n = 0 the one box gives
// (psi_1(r1) psi_2(r2)) psi_3(r3), each product rounded once.  The combine kernel then forms, with contraction off,
//   ((((c_mu1 g_mu1 + c_var1 g_var1) + c_mu2 g_mu2) + c_var2 g_var2) + c_mu3 g_mu3) + c_var3 g_var3
// per member and coordinate, adds the members in member order and divides once; the value likewise.
//
// Limits: F <= 192 and at most 64 pending points, so cap <= 256 and B <= 33 153; E <= 341, so 3 E <= 1024; no derivative
// observations.  A candidate never raises; only a pending point whose Schur pivot fails does, payload (the flat index 3 e +
// objective - 1, the point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "ehvi1.hpp"
#include "ehvi3.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

constexpr int kEhvi3Cap = kEhvi3MaxFront + kKg1MaxPending;  // a member's front at its largest: one thread per point
constexpr int kEhvi3Edges = kEhvi3Cap + 2;                  // -infinity, the points, the reference point
static_assert(kEhvi3Cap == 256, "the table kernel gives every point a thread, the front kernel every lane four points");

size_t max_boxes(int cap) { return (size_t)(cap + 1) * (size_t)(cap + 2) / 2; }

Ehvi3Layout layout_of(const Kg1Ensemble& T) {
  const Ehvi3Call& k = *static_cast<const Ehvi3Call*>(T.client);
  return ehvi3_layout(T.E / 3, k.F, T.pcap, T.mem[0].C);
}

// One wavefront per member (blockIdx.x).  kg: the sub-members' dKg, their mu at the pending points `aa` doubles behind.  first != 0:
// the member's front is the caller's [F][3]; otherwise the front as it stands.  Then the believed outcomes of `count` pending points
// join in order under the header's rule.  fronts: [E][3][cap], counts [E].  mask (NULL: every outcome is offered): member e offers
// pending point j only where mask[e mask_ld + j] != 0 (cehvi1.hip's believed feasibility).
__global__ __launch_bounds__(64) void ehvi3_front_kernel(const double* const* __restrict__ kg, size_t aa, const double* __restrict__ caller, int F, double r1, double r2, double r3, double* __restrict__ fronts, int cap, int* __restrict__ counts, int first, int count, const int* __restrict__ mask, int mask_ld) {
  __shared__ double s_u[kEhvi3Cap], s_v[kEhvi3Cap], s_w[kEhvi3Cap];
  __shared__ int s_keep[kEhvi3Cap];
  const int e = blockIdx.x, lane = threadIdx.x;
  const int room = min(cap, kEhvi3Cap);
  double* gu = fronts + (size_t)e * 3 * cap;
  double* gv = gu + cap;
  double* gw = gv + cap;
  int n;
  if (first != 0) {
    n = min(F, room);
    for (int i = lane; i < n; i += 64) {
      s_u[i] = caller[3 * i];
      s_v[i] = caller[3 * i + 1];
      s_w[i] = caller[3 * i + 2];
    }
  } else {
    n = min(counts[e], room);
    for (int i = lane; i < n; i += 64) {
      s_u[i] = gu[i];
      s_v[i] = gv[i];
      s_w[i] = gw[i];
    }
  }
  __syncthreads();
  const double* mu1 = kg[3 * e] + aa;
  const double* mu2 = kg[3 * e + 1] + aa;
  const double* mu3 = kg[3 * e + 2] + aa;
  for (int j = 0; j < count; ++j) {
    if (mask != nullptr && mask[(size_t)e * mask_ld + j] == 0) continue;  // (the same word for every lane)
    const double a = mu1[j], b = mu2[j], c = mu3[j];
    if (!(isfinite(a) && isfinite(b) && isfinite(c) && a < r1 && b < r2 && c < r3)) continue;  // (not finite or not strictly inside r)
    int dom = 0, kept = 0, before = 0;
    for (int i = lane; i < n; i += 64) {
      const double ui = s_u[i], vi = s_v[i], wi = s_w[i];
      dom |= (ui <= a && vi <= b && wi <= c) ? 1 : 0;
      const int keep = (ui >= a && vi >= b && wi >= c) ? 0 : 1;
      const bool ahead = wi < c || (wi == c && (ui < a || (ui == a && vi < b)));  // the point sorts before the outcome
      s_keep[i] = keep;
      kept += keep;
      before += (keep != 0 && ahead) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
      dom |= __shfl_xor(dom, off, 64);
      kept += __shfl_xor(kept, off, 64);
      before += __shfl_xor(before, off, 64);
    }
    if (dom != 0) continue;
    if (kept + 1 > room) continue;  // (cannot happen: cap counts the caller's front and every pending point)
    __syncthreads();
    // the kept points stay in order: the first `before` of them where they rank, the others one further
    double ru[kEhvi3Cap / 64], rv[kEhvi3Cap / 64], rw[kEhvi3Cap / 64];
    int pos[kEhvi3Cap / 64];
  #pragma unroll
    for (int k = 0; k < kEhvi3Cap / 64; ++k) {
      const int i = lane + 64 * k;
      pos[k] = -1;
      ru[k] = 0.0;
      rv[k] = 0.0;
      rw[k] = 0.0;
      if (i < n && s_keep[i] != 0) {
        int rank = 0;
        for (int q = 0; q < i; ++q) rank += s_keep[q];
        pos[k] = rank < before ? rank : rank + 1;
        ru[k] = s_u[i];
        rv[k] = s_v[i];
        rw[k] = s_w[i];
      }
    }
    __syncthreads();
  #pragma unroll
    for (int k = 0; k < kEhvi3Cap / 64; ++k) {
      if (pos[k] >= 0) {
        s_u[pos[k]] = ru[k];
        s_v[pos[k]] = rv[k];
        s_w[pos[k]] = rw[k];
      }
    }
    if (lane == 0) {
      s_u[before] = a;
      s_v[before] = b;
      s_w[before] = c;
    }
    n = kept + 1;
    __syncthreads();
  }
  for (int i = lane; i < n; i += 64) {
    gu[i] = s_u[i];
    gv[i] = s_v[i];
    gw[i] = s_w[i];
  }
  if (lane == 0) counts[e] = n;
}

// One workgroup per member (blockIdx.x), thread j for point j: the member's boxes in the header's order into tables [E][tstride],
// their number into nbox [E].
__global__ __launch_bounds__(256) void ehvi3_table_kernel(const double* __restrict__ fronts, int cap, const int* __restrict__ counts, ushort4* __restrict__ tables, size_t tstride, int* __restrict__ nbox) {
  __shared__ double s_u[kEhvi3Cap], s_v[kEhvi3Cap];
  __shared__ int s_surv[kEhvi3Cap], s_order[kEhvi3Cap];
  const int e = blockIdx.x, j = threadIdx.x;
  const int n = min(counts[e], min(cap, kEhvi3Cap));
  const double* gu = fronts + (size_t)e * 3 * cap;
  const double* gv = gu + cap;
  s_u[j] = j < n ? gu[j] : 0.0;
  s_v[j] = j < n ? gv[j] : 0.0;
  s_surv[j] = 0;
  __syncthreads();
  ushort4* tab = tables + (size_t)e * tstride;
  const unsigned short top = (unsigned short)(n + 1);
  if (j == 0) tab[0] = make_ushort4(0, top, top, 0);  // slab 0: the whole of (-infinity, r1] x (-infinity, r2]
  int off = 1;
  const double uj = s_u[j], vj = s_v[j];
  for (int k = 1; k <= n; ++k) {
    const int q = k - 1;  // the point that joins the staircase
    const double uq = s_u[q], vq = s_v[q];
    const int covered = __syncthreads_or((j < q && uj <= uq && vj <= vq) ? 1 : 0);
    if (covered == 0) {
      if (j < q && uq <= uj && vq <= vj) s_surv[j] = 0;
      if (j == q) s_surv[j] = 1;
    }
    __syncthreads();
    int m = 0, rank = 0;
    for (int i = 0; i < k; ++i) {
      const int sv = s_surv[i];
      m += sv;
      rank += (sv != 0 && s_u[i] < uj) ? 1 : 0;
    }
    if (j < k && s_surv[j] != 0) s_order[rank] = j;
    __syncthreads();
    // m surviving points, m + 1 strips; k <= 256 and thread 0 writes the last strip where m = 256
    for (int s = j; s <= m; s += 256) {
      const unsigned short left = s == 0 ? 0 : (unsigned short)(s_order[s - 1] + 1);
      const unsigned short right = s == m ? top : (unsigned short)(s_order[s] + 1);
      const unsigned short height = s == 0 ? top : left;
      tab[off + s] = make_ushort4(left, right, height, (unsigned short)k);
    }
    off += m + 1;
    __syncthreads();
  }
  if (j == 0) nbox[e] = off;
}

// The box sums (the header's reduction order).  Grid (C, E), four wavefronts; kg: the sub-members' [mu Cs | var Cs]; fronts / counts
// as ehvi3_front_kernel leaves them, tables / nbox as ehvi3_table_kernel does; vals [E][Cs] takes A_e and, with want_grad, coef
// [E][Cs][6] takes dA/dmu_1, dA/dvar_1, dA/dmu_2, dA/dvar_2, dA/dmu_3, dA/dvar_3.
__global__ __launch_bounds__(256) void ehvi3_box_kernel(int Cs, const double* const* __restrict__ kg, const double* __restrict__ fronts, int cap, const int* __restrict__ counts, const ushort4* __restrict__ tables, size_t tstride, const int* __restrict__ nbox, double r1, double r2, double r3, int want_grad, double* __restrict__ vals, double* __restrict__ coef) {
  __shared__ double s_e[3][3][kEhvi3Edges];  // [objective][psi, d / d mu, d / d var][edge]
  __shared__ double s_part[7][4];
  const int c = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
  const int n = min(counts[e], min(cap, kEhvi3Cap));
  const int B = min(nbox[e], (n + 1) * (n + 2) / 2);
  const bool wg = want_grad != 0;
  const double* pts = fronts + (size_t)e * 3 * cap;
  const int edges = n + 2;
  for (int idx = tid; idx < 3 * edges; idx += 256) {
    const int k = idx / edges, i = idx - k * edges;
    double psi = 0.0, dm = 0.0, dv = 0.0;  // edge 0: psi(-infinity) = 0
    if (i > 0) {
      const double t = i <= n ? pts[(size_t)k * cap + i - 1] : (k == 0 ? r1 : (k == 1 ? r2 : r3));
      const double mu = kg[3 * e + k][c], var = kg[3 * e + k][(size_t)Cs + c];
      const double sd = sqrt(fmax(kMinVarEI, var)), sg = sqrt(fmax(kMinVarGradEI, var));
      ehvi1_edge(t, mu, sd, sg, wg, psi, dm, dv);
    }
    s_e[k][0][i] = psi;
    s_e[k][1][i] = dm;
    s_e[k][2][i] = dv;
  }
  __syncthreads();
  const ushort4* tab = tables + (size_t)e * tstride;
  double accA = 0.0, accM1 = 0.0, accV1 = 0.0, accM2 = 0.0, accV2 = 0.0, accM3 = 0.0, accV3 = 0.0;
  for (int b = tid; b < B; b += 256) {
    const ushort4 bx = tab[b];
    const int uL = min((int)bx.x, n + 1), uR = min((int)bx.y, n + 1), vH = min((int)bx.z, n + 1), k = min((int)bx.w, n);
    const double P = s_e[0][0][uR] - s_e[0][0][uL];
    const double Q = s_e[1][0][vH];
    const double W = s_e[2][0][k + 1] - s_e[2][0][k];
    const double PQ = P * Q;
    accA = fma(PQ, W, accA);
    if (wg) {
      const double Pm = s_e[0][1][uR] - s_e[0][1][uL], Pv = s_e[0][2][uR] - s_e[0][2][uL];
      const double Qm = s_e[1][1][vH], Qv = s_e[1][2][vH];
      const double Wm = s_e[2][1][k + 1] - s_e[2][1][k], Wv = s_e[2][2][k + 1] - s_e[2][2][k];
      const double PmQ = Pm * Q, PvQ = Pv * Q, PQm = P * Qm, PQv = P * Qv;
      accM1 = fma(PmQ, W, accM1);
      accV1 = fma(PvQ, W, accV1);
      accM2 = fma(PQm, W, accM2);
      accV2 = fma(PQv, W, accV2);
      accM3 = fma(PQ, Wm, accM3);
      accV3 = fma(PQ, Wv, accV3);
    }
  }
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    accA += __shfl_xor(accA, off, 64);
    accM1 += __shfl_xor(accM1, off, 64);
    accV1 += __shfl_xor(accV1, off, 64);
    accM2 += __shfl_xor(accM2, off, 64);
    accV2 += __shfl_xor(accV2, off, 64);
    accM3 += __shfl_xor(accM3, off, 64);
    accV3 += __shfl_xor(accV3, off, 64);
  }
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    s_part[0][w] = accA;
    s_part[1][w] = accM1;
    s_part[2][w] = accV1;
    s_part[3][w] = accM2;
    s_part[4][w] = accV2;
    s_part[5][w] = accM3;
    s_part[6][w] = accV3;
  }
  __syncthreads();
  if (tid >= 7) return;
  const double total = (s_part[tid][0] + s_part[tid][1]) + (s_part[tid][2] + s_part[tid][3]);
  const double A = (s_part[0][0] + s_part[0][1]) + (s_part[0][2] + s_part[0][3]);
  const bool pos = A > 0.0;
  const size_t o = (size_t)e * Cs + c;
  if (tid == 0) {
    vals[o] = pos ? total : 0.0;
  } else if (wg) {
    coef[6 * o + tid - 1] = pos ? total : 0.0;
  }
}

// The ensemble's value and gradient from the members' A_e and coefficients, one thread per output element (ehvi1_combine_kernel's
// shape with six terms): element i < nv of value_out (NULL: nv = 0) is candidate i's value, the elements behind are grad_out's
// (c, j).  grads: the sub-members' [grad mu Cs d | grad var Cs d].  Every operation rounded by itself, in the header's order.
__global__ __launch_bounds__(256) void ehvi3_combine_kernel(int E, long C, int Cs, int d, const double* __restrict__ vals, const double* __restrict__ coef, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out) {
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
    const double* co = coef + 6 * ((size_t)e * Cs + c);
    double a = 0.0;
    for (int r = 0; r < 3; ++r) {
      const double* g = grads[3 * e + r];
      const double tm = co[2 * r] * g[k];
      a = (r == 0) ? tm : a + tm;
      const double tv = co[2 * r + 1] * g[gv + k];
      a = a + tv;
    }
    sum = (e == 0) ? a : sum + a;
  }
  grad_out[k] = sum / (double)E;
}

}  // namespace

Ehvi3Layout ehvi3_layout(int E, int F, int pcap, int C) {
  Ehvi3Layout l;
  l.E = E;
  l.F = F;
  l.cap = std::min(kEhvi3Cap, std::max(1, F + pcap));
  l.C = C;
  l.tstride = max_boxes(l.cap);
  l.oCaller = 0;
  l.oFront = l.oCaller + 3 * (size_t)std::max(1, F);
  l.oCount = l.oFront + 3 * (size_t)l.E * l.cap;
  l.oNbox = l.oCount + (size_t)l.E;  // (the counts are integers in the front halves of E doubles' room, the box counts likewise)
  l.oTable = l.oNbox + (size_t)l.E;
  l.oVals = l.oTable + (size_t)l.E * l.tstride;
  l.oCoef = l.oVals + (size_t)l.E * l.C;
  l.total = l.oCoef + 6 * (size_t)l.E * l.C;
  return l;
}

void ehvi3_launch_front(const Ehvi3Call& k, const Ehvi3Layout& l, double* base, const double* const* kg, size_t aa, const int* mask,
                        int mask_ld, bool first, int count, hipStream_t s) {
  int* counts = reinterpret_cast<int*>(base + l.oCount);
  MOE_LAUNCH_NOW(ehvi3_front_kernel, dim3((unsigned)l.E), dim3(64), 0, s, kg, aa, (const double*)(base + l.oCaller), l.F, k.r1, k.r2,
                 k.r3, base + l.oFront, l.cap, counts, first ? 1 : 0, count, mask, mask_ld);
  MOE_LAUNCH_NOW(ehvi3_table_kernel, dim3((unsigned)l.E), dim3(256), 0, s, (const double*)(base + l.oFront), l.cap, (const int*)counts,
                 reinterpret_cast<ushort4*>(base + l.oTable), l.tstride, reinterpret_cast<int*>(base + l.oNbox));
  MOE_HIP_CHECK(hipGetLastError());
}

void ehvi3_launch_box(const Ehvi3Call& k, const Ehvi3Layout& l, double* base, const double* const* kg, int C, bool want_grad,
                      hipStream_t s) {
  MOE_LAUNCH_NOW(ehvi3_box_kernel, dim3((unsigned)C, (unsigned)l.E), dim3(256), 0, s, l.C, kg, (const double*)(base + l.oFront), l.cap,
                 reinterpret_cast<const int*>(base + l.oCount), reinterpret_cast<const ushort4*>(base + l.oTable), l.tstride,
                 reinterpret_cast<const int*>(base + l.oNbox), k.r1, k.r2, k.r3, want_grad ? 1 : 0, base + l.oVals, base + l.oCoef);
}

namespace {

Kg1Member member(const Kg1Objective&, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  return ehvi1_member(gp, e % 3, C, with_grad, fail, pcap, fail_pending);
}

// mu of every sub-member at P_j0 .. j0 + count - 1, then every member's front takes the believed outcomes and its table is rebuilt
void join_believed_outcomes(Kg1Ensemble& T, int j0, int count, bool first) {
  const Ehvi3Call& k = *static_cast<const Ehvi3Call*>(T.client);
  const Ehvi3Layout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  const size_t aa = (size_t)(T.mem[0].dAA - T.mem[0].dKg);  // (one layout for every sub-member: ei1_member's, from C, d and with_grad)
  ehvi3_launch_front(k, l, g0.ehviD.p, T.dKgTab, aa, nullptr, 0, first, count, T.z);
}

// every sub-member's extension stands: the call's own device memory, the caller's front, then the members' fronts and tables
void all_extended(Kg1Ensemble& T, int p) {
  const Ehvi3Call& k = *static_cast<const Ehvi3Call*>(T.client);
  const Ehvi3Layout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  g0.ehviD.reserve(l.total);
  if (k.F > 0) copy_async(g0.ehviD.p + l.oCaller, k.front, sizeof(double) * 3 * (size_t)k.F, hipMemcpyHostToDevice, T.z);
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
  const Ehvi3Call& k = *static_cast<const Ehvi3Call*>(T.client);
  const Ehvi3Layout l = layout_of(T);
  if (C < 1 || C > l.C) throw Error(MOE_ERR_RUNTIME, "ehvi3: more candidates than the call was staged for");
  double* base = T.gps[0]->ehviD.p;
  ehvi3_launch_box(k, l, base, T.dKgTab, C, grad_out != nullptr, T.z);
  const long n = (value_out != nullptr ? (long)C : 0) + (grad_out != nullptr ? (long)C * T.d : 0);
  MOE_LAUNCH_NOW(ehvi3_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, l.E, (long)C, l.C, T.d,
                 (const double*)(base + l.oVals), (const double*)(base + l.oCoef), T.dGradTab, value_out, grad_out);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

// No sets, no fidelity coordinates, no incumbents (the members' best values are zeros, kept by the call); groups of three
// sub-members under the box rule, the members' own values kept
Kg1Call ehvi3_call(int num_mcmc, const double* reference_point, const double* front, int num_front) {
  Kg1Call call;
  call.doubles.assign(3 * (size_t)num_mcmc, 0.0);
  call.client = std::make_shared<const Ehvi3Call>(Ehvi3Call{front, num_front, reference_point[0], reference_point[1], reference_point[2]});
  call.o.best_so_far = call.doubles.data();
  call.o.member = member;
  call.o.eval_points = ehvi1_eval_points;
  call.o.all_extended = all_extended;
  call.o.pick_appended = pick_appended;
  call.o.group = 3;
  call.o.combine = combine;
  call.o.client = call.client.get();
  call.o.group_values = true;
  call.check_members = ehvi1_check_members;
  return call;
}

void check_ehvi3_num_mcmc(int num_mcmc) {
  if (num_mcmc < 1 || num_mcmc > kEhvi3MaxMembers)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc must be between 1 and 341 (three GPs per member)", num_mcmc, 1, kEhvi3MaxMembers);
}

void check_ehvi3_front(const double* reference_point, const double* front, int num_front) {
  if (num_front < 0 || num_front > kEhvi3MaxFront)
    throw Error(MOE_ERR_BOUNDS, "num_front must be between 0 and 192", num_front, 0, kEhvi3MaxFront);
  if (num_front > 0 && front == nullptr) throw Error(MOE_ERR_RUNTIME, "front is NULL with num_front > 0");
  for (int r = 0; r < 3; ++r)
    if (!std::isfinite(reference_point[r]))
      throw Error(MOE_ERR_INVALID_VALUE, "reference_point must be finite", reference_point[r], r, 0);
  for (int i = 0; i < num_front; ++i) {
    const double* a = front + 3 * (size_t)i;
    bool ok = std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && a[0] < reference_point[0] &&
              a[1] < reference_point[1] && a[2] < reference_point[2];
    if (ok && i > 0) {  // behind its predecessor: w ascending, ties by u, then by v; equal points are refused
      const double* b = a - 3;
      ok = b[2] < a[2] || (b[2] == a[2] && (b[0] < a[0] || (b[0] == a[0] && b[1] < a[1])));
    }
    for (int j = 0; ok && j < i; ++j) {  // (in this order only a point before it can be <= it in all three)
      const double* b = front + 3 * (size_t)j;
      if (b[0] <= a[0] && b[1] <= a[1] && b[2] <= a[2]) ok = false;
    }
    if (!ok)
      throw Error(MOE_ERR_INVALID_VALUE,
                  "front must be finite, strictly inside reference_point, in the canonical order (the third objective ascending, ties "
                  "by the first, then by the second) and mutually non-dominated (equal points count as dominated)",
                  i, 0, 0);
  }
}

}  // namespace moe
