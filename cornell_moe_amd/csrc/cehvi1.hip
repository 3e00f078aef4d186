// cornell_moe_amd/csrc/cehvi1.hip -- the constrained expected hypervolume improvement (the expected hypervolume improvement times
// the probability of feasibility: Emmerich, Giannakoglou & Naujoks 2006 with the constraint handling of Schonlau, Welch & Jones 1998
// and Gardner et al. 2014) for two and for three objectives, averaged over a hyper-parameter ensemble, with pending points, its
// multistart ascent and greedy q-point batches, on the device (moe_ehvi_constrained_mcmc*, moe_ehvi3_constrained_mcmc*): the eighth
// and ninth client of kg1_ascent.hip's staging, ascent and drivers.  The sub-member's chain, layout and check are ehvi1.hip's
// (ehvi1.hpp); the fronts, the strip kernel (M = 2) and the table and box kernels (M = 3) are ehvi1.hip's and ehvi3.hip's, launched
// through ehvi1.hpp / ehvi3.hpp over a table of the objective sub-members alone; this file keeps the believed-feasibility kernel,
// the feasibility kernel, the combine kernel and the description of the call (cehvi1_call, cehvi3_call).  logehvi1.hip and
// logehvi3.hip, the log forms for two and for three objectives, take the call's record, its layout and the same description under
// another combine hook (cehvi1.hpp).
//
// Minimisation.  A call takes E joint hyper-samples, M in {2, 3} objectives and K constraints, 1 <= K <= 8 here (K = 0 is the
// unconstrained client itself).  Member e is M + K GPs, the E (M + K) GPs being the SUB-MEMBERS of one Kg1Ensemble ordered
// [e][role]: roles 0 .. M - 1 the objectives, role M - 1 + k constraint k = 1 .. K, satisfied where c_k(x) <= tau_k.  Every
// sub-member runs ehvi1_eval_points and leaves [mu | var] in its dKg and [grad mu | grad var] in its dGrad.  With mu, var of a
// constraint sub-member at x, sigma = sqrt(max(DBL_MIN, var)), sigma_g = sqrt(max(150 eps^2, var)):
//   H_e      ehvi1.hip's A_e (M = 2) or ehvi3.hip's (M = 3) with its 4 or 6 coefficients: the same kernels, the same bits
//   F_{e,k}  = Phi(z), z = (tau_k - mu) / sigma;  z_g = (tau_k - mu) / sigma_g,
//              dF/dmu = -phi(z_g) / sigma_g,  dF/dvar = -phi(z_g) z_g / (2 sigma_g^2)                  (cei1.hip's role-k form)
//   A_e      = H_e F_{e,1} ... F_{e,K}                                  multiplied left to right
//   grad A_e = (F_1 ... F_K) grad H_e + sum_k (H_e prod_{q != k} F_q) grad F_k
//              each excluded product by the same left-to-right multiplication with its factor skipped, the terms added in the
//              order H, k = 1 .. K; grad H_e from its coefficients in ehvi1_combine_kernel's order (ehvi3.hip's for M = 3);
//              grad F_k = (dF/dmu) grad mu + (dF/dvar) grad var
//   value    = (A_0 + ... + A_{E-1}) / E, the gradient likewise: members added in member order and divided once, no contraction
//
// Fronts.  The caller's front is that of the FEASIBLE observations.  A pending point P_j is believed feasible under member e when
// mu_{e,k}(P_j) <= tau_k for every k (cehvi_believed_kernel, a word per (member, point)); the front kernels offer P_j's believed
// outcome to member e's front only where the word is set, so that a believed-infeasible pick does not shrink the non-dominated
// region.  Every sub-member's variance is conditioned on every pending point, whichever way the belief falls.  A greedy batch's
// pick joins the same way, inside device memory.
//
// Bits.  The strip and box kernels are never recorded and neither are the three kernels here; the feasibility kernel gives every
// (member, constraint, candidate) a thread and the combine kernel every output element one: a candidate's bits do not depend on who
// shares its pass, on want_grad or on ensemble-wide launches.  The evaluator's group values are [E][1 + K][C]: H_e, F_{e,1} ..
// F_{e,K}, from which the value is the rule above bit for bit.
//
// Limits: the unconstrained client's for the front and the pending points; E (M + K) <= 1024; no derivative observations.  A
// candidate never raises; only a pending point whose Schur pivot fails does, payload (the flat index e (M + K) + role, the point).
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "acq1_device.hpp"
#include "cehvi1.hpp"
#include "ehvi1.hpp"
#include "ehvi3.hpp"
#include "kg1_ascent.hpp"

namespace moe {

namespace {

CehviLayout layout_of(const Kg1Ensemble& T) {
  const CehviCall& k = *static_cast<const CehviCall*>(T.client);
  CehviLayout l = {};
  l.M = k.M;
  l.K = k.K;
  l.E = T.E / (k.M + k.K);
  l.C = T.mem[0].C;
  l.mask_ld = std::max(1, T.pcap);
  size_t inner;
  if (k.M == 2) {
    l.l2 = ehvi1_layout(l.E, k.c2.F, T.pcap, l.C);
    inner = l.l2.total;
  } else {
    l.l3 = ehvi3_layout(l.E, k.c3.F, T.pcap, l.C);
    inner = l.l3.total;
  }
  l.oObj = inner;
  l.oMask = l.oObj + (size_t)l.E * l.M;
  l.oFeas = l.oMask + ((size_t)l.E * l.mask_ld + 1) / 2;
  l.oFactors = l.oFeas + 3 * (size_t)l.E * l.K * l.C;
  l.total = l.oFactors + (size_t)l.E * (1 + l.K) * l.C;
  return l;
}

// obj [E][M]: the objective sub-members' entries of kg [E][G]
__global__ __launch_bounds__(256) void cehvi_objectives_kernel(const double* const* __restrict__ kg, int E, int M, int G, const double** __restrict__ obj) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * M) return;
  const int e = i / M, r = i - e * M;
  obj[i] = kg[(size_t)e * G + r];
}

// One thread per (member, pending point): the word of point j < count under member e is 1 where every constraint sub-member's
// mean at the point (aa doubles behind its dKg, launch_mean's block) is <= its threshold; a NaN mean leaves 0.  mask [E][mask_ld].
__global__ __launch_bounds__(256) void cehvi_believed_kernel(const double* const* __restrict__ kg, size_t aa, int E, int M, int K, const CehviTau tau, int count, int* __restrict__ mask, int mask_ld) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= E * count) return;
  const int e = i / count, j = i - e * count;
  int ok = 1;
  for (int k = 0; k < K; ++k) {
    const double mu = kg[(size_t)e * (M + K) + M + k][aa + j];
    ok &= (mu <= tau.t[k]) ? 1 : 0;
  }
  mask[(size_t)e * mask_ld + j] = ok;
}

// One thread per (member, constraint, candidate): F and, with want_grad, dF/dmu and dF/dvar (the header's forms) from the
// constraint sub-member's [mu Cs | var Cs].  feas [E][K][Cs][3].
__global__ __launch_bounds__(256) void cehvi_feas_kernel(const double* const* __restrict__ kg, int E, int M, int K, const CehviTau tau, int C, int Cs, int want_grad, double* __restrict__ feas) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)E * K * C) return;
  const int c = (int)(i % C);
  const int ek = (int)(i / C), k = ek % K, e = ek / K;
  const double* src = kg[(size_t)e * (M + K) + M + k];
  const double mu = src[c], var = src[(size_t)Cs + c];
  const double t = tau.t[k] - mu;
  const double sigma = sqrt(fmax(kMinVarEI, var));
  double* out = feas + 3 * ((size_t)ek * Cs + c);
  out[0] = normal_cdf(t / sigma);
  if (want_grad == 0) return;
  const double sg = sqrt(fmax(kMinVarGradEI, var));
  const double zg = t / sg;
  const double pg = normal_pdf(zg) / sg;
  out[1] = -pg;
  out[2] = -(pg * zg) / sg * 0.5;
}

// The product rule and the ensemble mean, one thread per output element (cei1_combine_kernel's shape): element i < nv of value_out
// (NULL: nv = 0) is candidate i's value, the elements behind are grad_out's (c, j).  hv [E][Cs] and coef [E][Cs][2 M]: the strip or
// box kernel's; feas: cehvi_feas_kernel's; grads: the E (M + K) sub-members' [grad mu Cs d | grad var Cs d].  A value thread also
// leaves its candidate's group values in factors [E][1 + K][Cs].  Every operation rounded by itself, in the header's order.
__global__ __launch_bounds__(256) void cehvi_combine_kernel(int E, int M, int K, long C, int Cs, int d, const double* __restrict__ hv, const double* __restrict__ coef, const double* __restrict__ feas, const double* const* __restrict__ grads, double* __restrict__ value_out, double* __restrict__ grad_out, double* __restrict__ factors) {
#pragma clang fp contract(off)
  const long nv = value_out != nullptr ? C : 0, ng = grad_out != nullptr ? C * d : 0;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv + ng) return;
  if (i < nv) {
    double sum = 0.0;
    for (int e = 0; e < E; ++e) {
      const double H = hv[(size_t)e * Cs + i];
      double a = H;
      factors[(size_t)e * (1 + K) * Cs + i] = H;
      for (int k = 0; k < K; ++k) {
        const double f = feas[3 * (((size_t)e * K + k) * Cs + i)];
        a = a * f;
        factors[((size_t)e * (1 + K) + 1 + k) * Cs + i] = f;
      }
      sum = (e == 0) ? a : sum + a;
    }
    value_out[i] = sum / (double)E;
    return;
  }
  const long k = i - nv, c = k / d;
  const size_t gv = (size_t)Cs * d;
  const int G = M + K;
  double sum = 0.0;
  for (int e = 0; e < E; ++e) {
    const double* co = coef + 2 * (size_t)M * ((size_t)e * Cs + c);
    const double* fe = feas + 3 * ((size_t)e * K * Cs + c);  // constraint q's three lie 3 q Cs further
    double gH = 0.0;
    for (int r = 0; r < M; ++r) {
      const double* g = grads[(size_t)e * G + r];
      const double tm = co[2 * r] * g[k];
      gH = (r == 0) ? tm : gH + tm;
      const double tv = co[2 * r + 1] * g[gv + k];
      gH = gH + tv;
    }
    double ex = fe[0];
    for (int q = 1; q < K; ++q) ex = ex * fe[3 * (size_t)q * Cs];
    double a = ex * gH;
    const double H = hv[(size_t)e * Cs + c];
    for (int r = 0; r < K; ++r) {
      ex = H;
      for (int q = 0; q < K; ++q) {
        if (q == r) continue;
        ex = ex * fe[3 * (size_t)q * Cs];
      }
      const double* f = fe + 3 * (size_t)r * Cs;
      const double* g = grads[(size_t)e * G + M + r];
      const double tm = f[1] * g[k];
      const double tv = f[2] * g[gv + k];
      const double gF = tm + tv;
      const double term = ex * gF;
      a = a + term;
    }
    sum = (e == 0) ? a : sum + a;
  }
  grad_out[k] = sum / (double)E;
}

Kg1Member member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  return ehvi1_member(gp, e % o.group, C, with_grad, fail, pcap, fail_pending);
}

// mu of every sub-member at P_j0 .. j0 + count - 1, the members' beliefs about those points, then every member's front takes the
// believed outcomes it believes feasible (M = 3: and its table is rebuilt)
void join_believed_outcomes(Kg1Ensemble& T, int j0, int count, bool first) {
  const CehviCall& k = *static_cast<const CehviCall*>(T.client);
  const CehviLayout l = layout_of(T);
  for (Kg1Member& m : T.mem) {
    GpDev& gp = *m.gp;
    if (count > 0)
      launch_mean(gp.cp, gp.dX.p, gp.n, gp.derivs, gp.dKinvY.p, T.dPending + (size_t)j0 * T.dp, count, gp.mean, false, m.dAA, T.z);
  }
  double* base = T.gps[0]->ehviD.p;
  const size_t aa = (size_t)(T.mem[0].dAA - T.mem[0].dKg);  // (one layout for every sub-member: ei1_member's, from C, d and with_grad)
  int* mask = reinterpret_cast<int*>(base + l.oMask);
  const double* const* obj = reinterpret_cast<const double* const*>(base + l.oObj);
  if (count > 0) {
    if (count > l.mask_ld) throw Error(MOE_ERR_RUNTIME, "cehvi1: more pending points than the call has room for");
    MOE_LAUNCH_NOW(cehvi_believed_kernel, dim3((unsigned)((l.E * count + 255) / 256)), dim3(256), 0, T.z, T.dKgTab, aa, l.E, l.M, l.K,
                   k.tau, count, mask, l.mask_ld);
  }
  if (l.M == 2)
    ehvi1_launch_front(k.c2, l.l2, base, obj, aa, mask, l.mask_ld, first, count, T.z);
  else
    ehvi3_launch_front(k.c3, l.l3, base, obj, aa, mask, l.mask_ld, first, count, T.z);
}

// every sub-member's extension stands: the call's own device memory, the caller's front, the objectives' table, then the members'
// fronts
void all_extended(Kg1Ensemble& T, int p) {
  const CehviCall& k = *static_cast<const CehviCall*>(T.client);
  const CehviLayout l = layout_of(T);
  GpDev& g0 = *T.gps[0];
  g0.ehviD.reserve(l.total);
  double* base = g0.ehviD.p;
  if (l.M == 2) {
    if (k.c2.F > 0) copy_async(base + l.l2.oCaller, k.c2.front, sizeof(double) * 2 * (size_t)k.c2.F, hipMemcpyHostToDevice, T.z);
  } else {
    if (k.c3.F > 0) copy_async(base + l.l3.oCaller, k.c3.front, sizeof(double) * 3 * (size_t)k.c3.F, hipMemcpyHostToDevice, T.z);
  }
  MOE_LAUNCH_NOW(cehvi_objectives_kernel, dim3((unsigned)((l.E * l.M + 255) / 256)), dim3(256), 0, T.z, T.dKgTab, l.E, l.M, l.M + l.K,
                 reinterpret_cast<const double**>(base + l.oObj));
  T.dGroupVals = base + l.oFactors;
  join_believed_outcomes(T, 0, p, true);
}

// a pick joins every sub-member's extension, then its believed outcome the fronts of the members that believe it feasible
void pick_appended(Kg1Ensemble& T) {
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, false, T.z);
  join_believed_outcomes(T, T.p, 1, false);
}

void combine(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) {
  if (value_out == nullptr && grad_out == nullptr) return;
  const CehviCall& k = *static_cast<const CehviCall*>(T.client);
  const CehviLayout l = layout_of(T);
  if (C < 1 || C > l.C) throw Error(MOE_ERR_RUNTIME, "cehvi1: more candidates than the call was staged for");
  double* base = T.gps[0]->ehviD.p;
  const double* const* obj = reinterpret_cast<const double* const*>(base + l.oObj);
  const bool wg = grad_out != nullptr;
  const double *hv, *coef;
  if (l.M == 2) {
    ehvi1_launch_strip(k.c2, l.l2, base, obj, C, wg, T.z);
    hv = base + l.l2.oVals;
    coef = base + l.l2.oCoef;
  } else {
    ehvi3_launch_box(k.c3, l.l3, base, obj, C, wg, T.z);
    hv = base + l.l3.oVals;
    coef = base + l.l3.oCoef;
  }
  const long nf = (long)l.E * l.K * C;
  MOE_LAUNCH_NOW(cehvi_feas_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, T.z, T.dKgTab, l.E, l.M, l.K, k.tau, C, l.C,
                 wg ? 1 : 0, base + l.oFeas);
  const long n = (value_out != nullptr ? (long)C : 0) + (wg ? (long)C * T.d : 0);
  MOE_LAUNCH_NOW(cehvi_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, l.E, l.M, l.K, (long)C, l.C, T.d, hv, coef,
                 (const double*)(base + l.oFeas), T.dGradTab, value_out, grad_out, base + l.oFactors);
  MOE_HIP_CHECK(hipGetLastError());
}

// No sets, no fidelity coordinates, no incumbents (the sub-members' best values are zeros, kept by the call); groups of M + K
// sub-members under the header's rule, the groups' own values 1 + K rows each
Kg1Call constrained_call(int num_mcmc, CehviCall c) {
  const int G = c.M + c.K;
  Kg1Call call;
  call.doubles.assign((size_t)G * num_mcmc, 0.0);
  call.client = std::make_shared<const CehviCall>(c);
  call.o.best_so_far = call.doubles.data();
  call.o.member = member;
  call.o.eval_points = ehvi1_eval_points;
  call.o.all_extended = all_extended;
  call.o.pick_appended = pick_appended;
  call.o.group = G;
  call.o.combine = combine;
  call.o.client = call.client.get();
  call.o.group_values = true;
  call.o.group_value_rows = 1 + c.K;
  call.check_members = ehvi1_check_members;
  return call;
}

CehviCall constraints_of(int M, int num_constraints, const double* thresholds) {
  CehviCall c = {};
  c.M = M;
  c.K = num_constraints;
  for (int k = 0; k < num_constraints; ++k) c.tau.t[k] = thresholds[k];
  return c;
}

}  // namespace

// what logehvi1.hip and logehvi3.hip take (cehvi1.hpp)
CehviLayout cehvi_layout(const Kg1Ensemble& T) { return layout_of(T); }

CehviCall cehvi_constraints_of(int M, int num_constraints, const double* thresholds) { return constraints_of(M, num_constraints, thresholds); }

Kg1Call cehvi_call_combined_by(int num_mcmc, const CehviCall& c, void (*combine_by)(const Kg1Ensemble& T, int C, double* value_out, double* grad_out)) {
  Kg1Call call = constrained_call(num_mcmc, c);
  call.o.combine = combine_by;
  return call;
}

Kg1Call cehvi1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                    int num_front) {
  if (num_constraints == 0) return ehvi1_call(num_mcmc, reference_point, front, num_front);
  CehviCall c = constraints_of(2, num_constraints, thresholds);
  c.c2 = Ehvi1Call{front, num_front, reference_point[0], reference_point[1]};
  return constrained_call(num_mcmc, c);
}

Kg1Call cehvi3_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                    int num_front) {
  if (num_constraints == 0) return ehvi3_call(num_mcmc, reference_point, front, num_front);
  CehviCall c = constraints_of(3, num_constraints, thresholds);
  c.c3 = Ehvi3Call{front, num_front, reference_point[0], reference_point[1], reference_point[2]};
  return constrained_call(num_mcmc, c);
}

void check_ehvi_constrained_shapes(int num_objectives, int num_mcmc, int num_constraints, const void* constraint_gps,
                                   const double* thresholds) {
  const int G = num_objectives + (num_constraints > 0 ? num_constraints : 0);
  if (num_constraints < 0 || num_constraints > kCeiMaxConstraints)
    throw Error(MOE_ERR_BOUNDS, "num_constraints must be between 0 and 8", num_constraints, 0, kCeiMaxConstraints);
  if ((long)num_mcmc * G > 1024)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc (num_objectives + num_constraints) must be at most 1024", num_mcmc, 1, 1024 / G);
  if (num_constraints > 0 && (constraint_gps == nullptr || thresholds == nullptr))
    throw Error(MOE_ERR_RUNTIME, "constraint_gps and thresholds must not be NULL with num_constraints > 0");
  for (int k = 0; k < num_constraints; ++k)
    if (!std::isfinite(thresholds[k])) throw Error(MOE_ERR_INVALID_VALUE, "thresholds must be finite", thresholds[k], k, 0);
}

}  // namespace moe
