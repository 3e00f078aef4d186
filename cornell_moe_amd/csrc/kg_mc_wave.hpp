// cornell_moe_amd/csrc/kg_mc_wave.hpp -- the wave-per-sample q-KG / d-KG Monte-Carlo kernel kg_mc_kernel (gfx950) over the
// shared core kg_mc.hpp: its evaluator WaveEval, the frame line search line_search_frame, one sample (kg_sample), the kernel and
// its launchers.  Streamed tables from 16 coordinate rows on take WideEval / line_search_lds (kg_mc_lds.hpp) instead.
// Instantiated by kg_mc_dp{4,8,12,16,24,32}.hip.
#pragma once
#include "kg_mc.hpp"
#include "kg_mc_lds.hpp"

namespace moe {
namespace mc {

// Evaluator of the wave-per-sample kernel: one pass = eval_pass over the LDS tables.
template <int DP, int G, bool SMALL, bool XL>
struct WaveEval {
  const double* __restrict__ xs;
  const double* __restrict__ aw;
  const double* __restrict__ etab;
  int ntiles, cov_type;
  double mean;
  int lane;
  double* __restrict__ scr;  // per-wave LDS scratch for the gradient sums (DP doubles)
#if MOE_BLOCK_PROF
  unsigned long long c_v = 0, c_g = 0, n_v = 0, n_g = 0;
#endif
  // frame line search: f and its gradient with respect to the FRAME coordinates at the frame point xf; f at the point whose
  // frame coordinates are -q2 / 2
  __device__ __forceinline__ double eval_grad_frame(const double (&xf)[DP], double (&gradf)[DP]) {
#if MOE_BLOCK_PROF
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
    const double f = eval_pass<DP, G, true, SMALL, XL>(xs, aw, etab, ntiles, cov_type, mean, xf, gradf, lane, scr);
#if MOE_BLOCK_PROF
    c_g += __builtin_amdgcn_s_memtime() - t0;
    n_g++;
#endif
    return f;
  }
  // up to kMaxTrials Armijo trials alpha / 2^t in one pass (eval_multi_loop): q-KG on the LDS table only
  static constexpr int kMaxTrials = !SMALL ? 5 : 1;
  // T trials and the reference's sequence of decisions over them (gpp_optimization.hpp:752-769), with compile-time indices
  // (a runtime-sized result array would live in scratch memory): stops at the first accepted trial (done), halves alpha and
  // counts `search` for every rejected one, counts consumed trials only.  Returns false (nothing evaluated, nothing changed)
  // when a trial lies beyond the far radius.
  template <int T>
  __device__ __forceinline__ bool armijo_t(const double (&x2)[DP], const double (&d2)[DP], double f0, double norm, double& alpha_n,
                                           int& search, double& ftrial, bool& done, unsigned long long& n_val) {
    double f[T];
    const bool ok = (cov_type == MOE_COV_SQUARE_EXPONENTIAL)
                        ? eval_multi_loop<DP, MOE_COV_SQUARE_EXPONENTIAL, T, SMALL, XL, G>(xs, aw, etab, ntiles, mean, x2, d2, alpha_n, lane, f)
                        : eval_multi_loop<DP, MOE_COV_MATERN_NU_2P5, T, SMALL, XL, G>(xs, aw, etab, ntiles, mean, x2, d2, alpha_n, lane, f);
    if (!ok) return false;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (!done) {
        ftrial = f[t];
        n_val++;
#if MOE_BLOCK_PROF
        n_v++;
#endif
        if (ftrial - f0 > 0.5 * alpha_n * norm) {
          done = true;
        } else {
          alpha_n *= 0.5;
          if (++search >= 30) done = true;
        }
      }
    }
    return true;
  }
  // one pass over min(want, kMaxTrials) >= 2 trials
  __device__ __forceinline__ bool armijo_batch(int want, const double (&x2)[DP], const double (&d2)[DP], double f0, double norm,
                                               double& alpha_n, int& search, double& ftrial, bool& done,
                                               unsigned long long& n_val) {
    if constexpr (kMaxTrials >= 5) {
#if MOE_BLOCK_PROF
      const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
      bool ok;
      switch (want) {
        case 2: ok = armijo_t<2>(x2, d2, f0, norm, alpha_n, search, ftrial, done, n_val); break;
        case 3: ok = armijo_t<3>(x2, d2, f0, norm, alpha_n, search, ftrial, done, n_val); break;
        case 4: ok = armijo_t<4>(x2, d2, f0, norm, alpha_n, search, ftrial, done, n_val); break;
        default: ok = armijo_t<5>(x2, d2, f0, norm, alpha_n, search, ftrial, done, n_val); break;
      }
#if MOE_BLOCK_PROF
      c_v += __builtin_amdgcn_s_memtime() - t0;
#endif
      return ok;
    } else {
      return false;
    }
  }
  __device__ __forceinline__ double eval_value_q2(const double (&q2)[DP]) {
    double unused[DP];
#if MOE_BLOCK_PROF
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
    const double f = eval_pass<DP, G, false, SMALL, XL>(xs, aw, etab, ntiles, cov_type, mean, q2, unused, lane);
#if MOE_BLOCK_PROF
    c_v += __builtin_amdgcn_s_memtime() - t0;
    n_v++;
#endif
    return f;
  }
};

// The line search of the wave-per-sample kernel, carried out in the FRAME of the tables (x' = (x - c) s per table row, s the
// frame scale): the sequence of decisions of the reference's GradientDescentOptimizerLineSearch::Optimize
// (gpp_optimization.hpp:1242-1283) around GradientDescentOptimizationLineSearch (:708-828) with
// TensorProductDomain::LimitUpdate (gpp_domain.cpp:64-105), as plain nested wave-uniform loops -- every comparison in them is
// invariant under a positive affine map of a coordinate, so no pass converts its point: with g the gradient in the original
// coordinates and gf = g / s the one the evaluator returns,
//     x + alpha g   <->   x' + alpha gf s^2,       |g|^2 = sum (gf s)^2,       |step|^2 = sum (step' / s)^2,
// and the value passes take q2 = -2 (x' + alpha gf s^2) = fma(alpha, d2, x2) directly (eval_loop, value passes).  Every
// posterior-mean value comes from the same dataflow (eval_loop, explicit fma only), so re-evaluating a point reproduces its value
// bit for bit at any call site, which lets the search reuse f(x) where the reference recomputes it.  The per-row
// constants live in an LDS block `cst` (written once per workgroup): [0, DP) frame scale s | [DP, 2DP) 1 / s (0 in pad rows) |
// [2DP, 3DP) centre c | [3DP, 4DP) lower bound' | [4DP, 5DP) upper bound' (bounds already in the frame) | [5DP, 6DP) the value a
// pinned row holds.  `scr` is 3 DP doubles of per-wave LDS scratch (the restart's starting point | the evaluator's gradient sums |
// the clamped step).  Nothing of KgMcParams' per-row arrays is touched between the first and the last pass of a sample: they used to sit in ~100 SGPRs and
// were spilled to / reloaded from VGPR lanes (v_readlane -- a VALU slot each) around every pass.

template <int DP>
__device__ __forceinline__ void fill_frame_constants(const KgMcParams& P, double* __restrict__ cst) {
  const int r = threadIdx.x;
  if (r < DP) {
    const double sc = P.inv_lp[r];
    cst[r] = sc;
    cst[DP + r] = (sc != 0.0) ? 1.0 / sc : 0.0;
    cst[2 * DP + r] = P.center[r];
    cst[3 * DP + r] = (P.bounds[2 * r] - P.center[r]) * sc;
    cst[4 * DP + r] = (P.bounds[2 * r + 1] - P.center[r]) * sc;
    cst[5 * DP + r] = (P.perm[r] < P.dim) ? 1.0 : 0.0;  // what a pinned row holds: fidelity coordinates 1, pads 0 (.cpp:353-357)
  }
}

template <int DP, int G, class EV>
__device__ __forceinline__ double line_search_frame(const KgMcParams& P, const double* __restrict__ cst, double* __restrict__ scr,
                                                    EV& ev, double (&x)[DP], unsigned long long& n_val,
                                                    unsigned long long& n_grad, const double* __restrict__ start_row = nullptr) {
  typedef const volatile __attribute__((address_space(3))) double* cst_ptr;  // (volatile: read where used, never hoisted)
  cst_ptr C = (cst_ptr)cst;
  const int lane_id = (int)(threadIdx.x & 63u);
  const unsigned int free_mask = P.free_mask;
  const int max_num_steps = P.max_num_steps, max_num_restarts = P.max_num_restarts;
  const double tolerance = P.tolerance;
  if (max_num_restarts <= 0) {
    // reference returns without touching its outputs (.cpp:425-427): value 0, point filled with 1.0 (.cpp:163)
#pragma unroll
    for (int k = 0; k < DP; ++k) x[k] = (k < P.dim) ? 1.0 : 0.0;
    return 0.0;
  }
  const double step_tolerance = tolerance / (double)max_num_steps;
  // entry: table-row order, then into the frame (pinned rows -- fidelity coordinates, pads -- keep their frame value throughout)
  // The point lives twice: xo_l -- lane r holds coordinate r in the ORIGINAL units, advanced by exactly the reference's operations
  // (x += LimitUpdate(alpha grad), TensorProductDomain::LimitUpdate on the original bounds) -- and xf, its image in the frame,
  // which only feeds the evaluator.  LimitUpdate's "would the step leave the domain" test is a knife edge when a step goes to the
  // wall itself (max_relative_change = 1: x + (upper - x) is exactly upper in the original units, by Sterbenz, but can be one
  // ulp beyond the wall's image in the centred frame -- which halves the step): the decisions must be taken where the reference
  // takes them (found by tools/fuzz_parity.py, seed 101 case 93).
  double xf[DP];
  double xo_l = 0.0;
  {
    double xp[DP];
    to_table_order<DP, G>(x, P.perm, xp);
#pragma unroll
    for (int r = 0; r < DP; ++r) {
      xf[r] = (xp[r] - C[2 * DP + r]) * C[r];
      xo_l = (lane_id == r) ? xp[r] : xo_l;
    }
  }
  volatile __attribute__((address_space(3))) double* S = (volatile __attribute__((address_space(3))) double*)scr;
  const int lk = lane_id < DP ? lane_id : 0;
  const double lo_l = P.bounds[2 * lk], hi_l = P.bounds[2 * lk + 1];  // original units, table-row order (once per sample)
  const double s_l = C[lk];
  const bool free_l = lane_id < DP && ((free_mask >> (lane_id & 31)) & 1u);
  double fcur = 0.0;
  double gf[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) gf[k] = 0.0;
  // A clamped step needs f(x + step) before it is accepted (.hpp:771-786), and -- once accepted -- the next iteration starts by
  // evaluating f and grad f at that very point.  While another iteration can follow, that evaluation is therefore done as ONE
  // value + gradient pass and carried over (have_g): a step costs its Armijo trials + one pass instead of + two.  A carried
  // gradient that ends up unused (step rejected, |step| below the tolerance, no further restart) is counted as the value pass
  // it replaced, so the device counters never exceed what was computed.
  bool have_g = false;
  double f_carried = 0.0;
  int pred = 1;  // Armijo trials the previous step consumed (how many the next step evaluates in its first pass)
  for (int restart = 0; restart < max_num_restarts; ++restart) {
#pragma unroll
    for (int k = 0; k < DP; ++k) S[k] = xf[k];  // the restart's starting point (every lane writes the same value)
    for (int istep = 0; istep < max_num_steps;) {
      // ---- f(x), grad f(x) ----
      double f0;
      if (have_g) {
        f0 = f_carried;
        have_g = false;
      } else if (G == 0 && start_row != nullptr && restart == 0 && istep == 0) {
        // the sample's first gradient, at its discretised point: from the start table (beta still sits behind the rows of `scr`)
        const double v = start_from_table<DP>(start_row, S + kMaxM, P.m, lane_id);
        f0 = lane_value(v, DP);
#pragma unroll
        for (int k = 0; k < DP; ++k) gf[k] = lane_value(v, k);
      } else {
        f0 = ev.eval_grad_frame(xf, gf);
      }
      n_grad++;
      fcur = f0;
      // d2 = -2 g s (the trial direction in the frame, pre-multiplied for q2), x2 = -2 x', |g|^2
      double d2[DP], x2[DP];
      double norm = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const double sk = C[k];
        const double g = ((free_mask >> k) & 1u) ? gf[k] * sk : 0.0;  // fidelity / pad coordinates stay pinned
        norm = fma(g, g, norm);
        d2[k] = -2.0 * (g * sk);
        x2[k] = -2.0 * xf[k];
      }
      // pre_mult * (i+1)^-gamma (gpp_optimization.hpp:741); x^-0 == 1 exactly, so gamma == 0 needs no pow()
      double alpha_n = (P.gamma == 0.0) ? P.pre_mult : P.pre_mult * pow((double)(istep + 1), -P.gamma);
      // ---- Armijo back-tracking (.hpp:745-760): unclamped trial points ----
      // The trial step sizes alpha, alpha / 2, alpha / 4, ... are known in advance, so several of them can be evaluated in
      // one pass (EV::eval_value_multi, where the evaluator has it): as many as the previous step of THIS sample consumed
      // (the first step of a sample starts with one; a sample's results therefore depend on nothing but the sample), then
      // in pairs.  The sequence of decisions is the reference's; only consumed trials are counted.
      int search = 0;
      double ftrial = 0.0;
      {
        int batch = pred;
        bool done = false;
        while (!done) {
          bool evaluated = false;
          if (EV::kMaxTrials >= 2 && P.multi_trial != 0) {
            const int want = min(batch, 30 - search);
            if (want >= 2) evaluated = ev.armijo_batch(want, x2, d2, f0, norm, alpha_n, search, ftrial, done, n_val);
          }
          if (!evaluated) {
            double q2[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) q2[k] = fma(alpha_n, d2[k], x2[k]);
            ftrial = ev.eval_value_q2(q2);
            n_val++;
            if (ftrial - f0 > 0.5 * alpha_n * norm) {
              done = true;
            } else {
              alpha_n *= 0.5;
              if (++search >= 30) done = true;
            }
          }
          // (a first trial that fails is usually followed by several halvings: four more at once, then pairs)
          batch = (batch == 1 && search == 1) ? 4 : 2;
        }
        pred = min(search + 1, EV::kMaxTrials);
      }
      // ---- LimitUpdate in the frame, one coordinate per lane, then accept only if f improves (.hpp:762-795) ----
      bool changed, nonzero;
      double step[DP];
      double step_o = 0.0;  // this lane's coordinate of the step, original units
      {
        double g_l = 0.0, d2_l = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          g_l = (lane_id == k) ? gf[k] : g_l;
          d2_l = (lane_id == k) ? d2[k] : d2_l;
        }
        const double want_o = alpha_n * (g_l * s_l);  // alpha grad_r in the original units (grad = frame gradient x scale)
        if (free_l) step_o = limit_update_1d(lo_l, hi_l, P.max_relative_change, xo_l, want_o);
        changed = __ballot(free_l && step_o != want_o) != 0ull;
        nonzero = __ballot(free_l && step_o != 0.0) != 0ull;
        // the step in the frame: the trial point's own offset where the clamp left it alone (its value is reused below)
        const double step_f = changed ? step_o * s_l : (-0.5 * alpha_n) * d2_l;
        if (lane_id < DP) S[2 * DP + lane_id] = free_l ? step_f : 0.0;  // back as wave-uniform values through the scratch
#pragma unroll
        for (int k = 0; k < DP; ++k) step[k] = S[2 * DP + k];
      }
      if (search == 30 || !nonzero) break;  // .hpp:781-785: x restored (a zero step re-evaluates f(x) == f0: rejected)
      double obj2 = ftrial;  // the clamp left the step untouched: f(x + step) is the last trial value
      bool carried = false;
      if (changed) {
        if (istep + 1 < max_num_steps || restart + 1 < max_num_restarts) {
          double xn[DP];
#pragma unroll
          for (int k = 0; k < DP; ++k) xn[k] = xf[k] + step[k];
          obj2 = ev.eval_grad_frame(xn, gf);  // (the old gradient is spent: d2 carries the direction)
          carried = true;
        } else {
          double q2[DP];
#pragma unroll
          for (int k = 0; k < DP; ++k) q2[k] = fma(-2.0, step[k], x2[k]);
          obj2 = ev.eval_value_q2(q2);
          n_val++;
        }
      }
      if (obj2 <= f0) {
        if (carried) n_val++;
        break;
      }
      double ss = 0.0;  // |step|^2 in the original coordinates
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        xf[k] += step[k];
        const double so = step[k] * C[DP + k];
        ss = fma(so, so, ss);
      }
      xo_l += step_o;
      fcur = obj2;
      istep += 1;
      have_g = carried;
      f_carried = obj2;
      if (sqrt(ss) < step_tolerance) break;
    }
    double ds = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const double dk = (S[k] - xf[k]) * C[DP + k];
      ds = fma(dk, dk, ds);
    }
    if (!(sqrt(ds) > tolerance)) break;
  }
  if (have_g) n_val++;  // carried but never used
  // exit: the original-unit state (pinned rows hold what a fidelity coordinate / pad row holds) in the original dimension order
  {
    if (lane_id < DP) S[lane_id] = free_l ? xo_l : C[5 * DP + lk];
    double xo[DP];
#pragma unroll
    for (int r = 0; r < DP; ++r) xo[r] = S[r];
    from_table_order<DP, G>(xo, P.perm, x);
  }
  return fcur;
}

// One MC sample: weights, discretised-set scan, line-search gradient descent.  Called with the whole wave converged.
template <int DP, int G, bool SMALL, bool XL>
__device__ __forceinline__ void kg_sample(const KgMcParams& P, int e, int sl, const double* __restrict__ xs,
                                          double* __restrict__ aw, double* __restrict__ zb,
                                          const double* __restrict__ etab, const double* __restrict__ cst, int lane,
                                          unsigned long long& tot_val, unsigned long long& tot_grad) {
  const int m = P.m, u = P.u, n = P.n, g1 = 1 + P.g;
  const int s = P.first_sample + sl;  // global sample index
  const int size = P.dim - P.f;       // problem size of the inner optimisation
  const double* rec = P.blob + (long)e * P.rec.stride;
  const double* Lsm = rec + P.rec.L;
  const double* We = P.W + (long)e * P.w_stride;

  double zc = 0.0, bc = 0.0;
  MOE_PROF_T(w0);
  const long so0 = (long)e * P.num_local + sl;
  const bool prepped = P.best_j != nullptr;  // beta and the discretised-set winner come from the pre-pass (kg_sample_prep_kernel)
  int best_j = 0;
  if (prepped) {
    bc = (lane < m) ? P.beta[so0 * m + lane] : 0.0;
    best_j = P.best_j[so0];
    zb[kMaxM + lane] = bc;
    __builtin_amdgcn_wave_barrier();
  } else {
    draw_z_beta(P, Lsm, s, lane, zb, zc, bc);
  }
  MOE_PROF_T(w1);
  // ---- per-sample weights (see file header) into this wave's LDS slab ----
  // v(j,a) = KinvY[(j,a)] - sum_c W[(j,a), c] beta_c.
  if (G == 0 && g1 == 1 && m <= 4) {
    // q-KG with up to four fantasy points: the loads of EIGHT tiles (40 independent L2 reads per lane) are issued together, so a
    // sample pays two round trips to L2 instead of one per pair of tiles (the phase is pure latency: 33k of a sample's 316k
    // cycles before).  Same operation order as the general loop below.
    const double b0 = zb[kMaxM], b1 = zb[kMaxM + 1], b2 = zb[kMaxM + 2], b3 = zb[kMaxM + 3];  // 0 beyond m
    const long c1 = (long)min(1, m - 1) * P.N, c2 = (long)min(2, m - 1) * P.N, c3 = (long)min(3, m - 1) * P.N;
    for (int t0 = 0; t0 < P.ntiles; t0 += 8) {
      double ky[8], l0[8], l1[8], l2[8], l3[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const long row = min(min(t0 + i, P.ntiles - 1) * 64 + lane, n - 1);  // clamped: always a valid address
        ky[i] = P.KinvY[row];
        l0[i] = We[row];
        l1[i] = We[row + c1];
        l2[i] = We[row + c2];
        l3[i] = We[row + c3];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int t = t0 + i;
        if (t < P.ntiles) {
          const int j = t * 64 + lane;
          double v = ky[i];
          v = fma(-l0[i], b0, v);
          v = fma(-l1[i], b1, v);
          v = fma(-l2[i], b2, v);
          v = fma(-l3[i], b3, v);
          if (j >= n) v = (j < n + u) ? zb[kMaxM + min(j - n, kMaxM - 1)] : 0.0;
          aw[(long)t * 64 + lane] = v * P.alpha;
        }
      }
    }
  } else {
  // The W loads are issued four columns at a time (column index clamped
  // to m - 1; beta is 0 beyond m) and two tiles per iteration, so ~10 independent L2 loads are in flight per wait
  // instead of one dependent load per fma.
#pragma unroll 2
  for (int t = 0; t < P.ntiles; ++t) {
    const int j = t * 64 + lane;
    double* w = aw + (long)t * (1 + G) * 64 + lane;
#pragma unroll
    for (int a = 0; a < 1 + G; ++a) {
      double v = 0.0;
      if (a < g1) {
        if (j < n) {
          const long row = (long)j * g1 + a;
          v = P.KinvY[row];
          for (int c0 = 0; c0 < m; c0 += 4) {
            const double l0 = We[row + (long)c0 * P.N];
            const double l1 = We[row + (long)min(c0 + 1, m - 1) * P.N];
            const double l2 = We[row + (long)min(c0 + 2, m - 1) * P.N];
            const double l3 = We[row + (long)min(c0 + 3, m - 1) * P.N];
            v = fma(-l0, zb[kMaxM + c0], v);
            v = fma(-l1, zb[kMaxM + min(c0 + 1, kMaxM - 1)], v);
            v = fma(-l2, zb[kMaxM + min(c0 + 2, kMaxM - 1)], v);
            v = fma(-l3, zb[kMaxM + min(c0 + 3, kMaxM - 1)], v);
          }
        } else if (j < n + u) {
          v = zb[kMaxM + (j - n) * g1 + a];
        }
        // fold alpha and, for derivative weights, the -(frame scale) of the derivative row (radial3)
        v *= (a == 0) ? P.alpha : -P.alpha * cst[a > 0 ? a - 1 : 0];
      }
      w[a * 64] = v;
    }
  }
  }
  // (each lane only ever reads back the weight entries it wrote itself -- no cross-lane hazard; zb is read by every lane
  //  but was written before the wave-wide butterflies above/below execute, and LDS ops of one wave complete in order)

  MOE_PROF_T(w2);
  if (!prepped) best_j = discrete_scan(P, rec, zb, lane);
  MOE_PROF_T(w3);

  const double* disc = rec + P.rec.disc;
  double x[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) x[k] = (k < size) ? disc[(long)best_j * size + k] : ((k < P.dim) ? 1.0 : 0.0);

  unsigned long long n_val = 0, n_grad = 0;  // passes over the n + u points (the A-point scan is O(A m), not counted)
  double fcur;
  if constexpr (wide_eval(DP, XL)) {
    double* st = zb + 2 * kMaxM;  // line-search vectors | packed-sum slot: kWideScratch doubles behind the z / beta scratch
    const d2t* xg = reinterpret_cast<const d2t*>(xs) + lane;
    lds_pair_ptr xl = (lds_pair_ptr)(cst + kCstRows * DP) + lane;  // the workgroup's LDS copy of the first tiles (kg_mc_kernel)
    WideEval<DP, G> ev{xg, xl, {(lds_tile_ptr)(aw + lane)}, etab, st + kLsRows * kMaxDimPadded, P.ntiles, P.wide_lds_tiles, P.cov_type, lane, P.mean};
    fcur = line_search_lds<DP, G>(P, ev, st, x, n_val, n_grad);
  } else {
    WaveEval<DP, G, SMALL, XL> ev{xs, aw, etab, P.ntiles, P.cov_type, P.mean, lane, zb + DP};
    // (z / beta scratch is idle by now -- but for beta, which the start table's row is multiplied with before the first pass)
    const double* start_row =
        (G == 0 && XL && P.start_tab != nullptr) ? P.start_tab + (long)e * P.start_stride + (long)best_j * (1 + m) * (DP + 1) : nullptr;
    fcur = line_search_frame<DP, G>(P, cst, zb, ev, x, n_val, n_grad, start_row);
#if MOE_BLOCK_PROF
    {
      const unsigned long long w4 = __builtin_amdgcn_s_memtime();
      if (lane == 0) {  // [0] z/beta [1] weights [2] scan [3] line search | [4] in value passes [5] in gradient passes | counts
        atomicAdd(&P.prof[0], w1 - w0);
        atomicAdd(&P.prof[1], w2 - w1);
        atomicAdd(&P.prof[2], w3 - w2);
        atomicAdd(&P.prof[3], w4 - w3);
        atomicAdd(&P.prof[4], ev.c_v);
        atomicAdd(&P.prof[5], ev.c_g);
        atomicAdd(&P.prof[6], ev.n_v);
        atomicAdd(&P.prof[7], ev.n_g);
        atomicAdd(&P.prof[13], 1ull);
      }
    }
#endif
  }

  const long so = so0;
  if (lane == 0) P.best_value[so] = fcur;
  tot_val += n_val;  // flushed once per wave and evaluation by the caller: 10^4 samples x 2 atomics on one cache line per
  tot_grad += n_grad;  // evaluation serialise in the L2 atomic unit (and delay the sample tickets queued behind them)
  if (lane < DP) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (lane == k) v = x[k];
    P.best_point[so * DP + lane] = v;
  }
  if (!prepped && lane < m) P.beta[so * m + lane] = bc;
}

// SMALL: the many-wavefront instantiation for point sets of a few tiles, where one pass is a short dependent chain (LDS
// read -> ~43 dependent FP64 operations -> wave reduction -> decision) that two wavefronts per SIMD cannot cover: compiled
// for 16 wavefronts per workgroup (<= 128 VGPRs, tile loop not unrolled) so that four wavefronts share each SIMD.
template <int DP, int G, bool XLDS, bool SMALL>
struct kg_mc_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int ntiles = P.ntiles;
    const int tab = ntiles * (DP + 1) * 64;  // LDS copy: the DP coordinate rows + the |x|^2 row per tile (see eval_loop)
    const int wslab = ntiles * (1 + G) * 64 + 2 * kMaxM + (wide_eval(DP, XLDS) ? kWideScratch : 0);
    // LDS: [64] exp table | [kCstRows x DP] per-row constants of the frame line search | [tab] coordinates (if XLDS) | per-wave slabs
    double* cst = smem + kExpTabLen;
    double* coords = cst + kCstRows * DP;
    const int wtab = wide_eval(DP, XLDS) ? P.wide_lds_tiles * DP * 64 : 0;  // streamed table: its leading tiles (paired rows: WideEval)
    double* aw = coords + (XLDS ? tab : wtab) + wave * wslab;
    double* zb = aw + ntiles * (1 + G) * 64;
    if (threadIdx.x < kExpTabLen) smem[threadIdx.x] = kExp2Tab64[threadIdx.x];
    fill_frame_constants<DP>(P, cst);
    if (!XLDS) __syncthreads();
    // (which evaluations this workgroup serves, and in what order: kg_mc.hpp next_evaluation; its LDS word is wave 0's scratch)
    bool moved = false;
    for (int e = first_evaluation(P, blockIdx); e >= 0;
         e = next_evaluation(P, gridDim, e, moved, reinterpret_cast<int*>(coords + (XLDS ? tab : wtab) + ntiles * (1 + G) * 64))) {
      const double* xs = P.XsTab + (long)e * P.tab_stride;
      if (XLDS) {
        __syncthreads();  // previous evaluation's readers are done
        for (int pt = threadIdx.x; pt < ntiles * 64; pt += blockDim.x) {  // one point per thread and step
          const int tl = pt >> 6, l = pt & 63;
          const double* src = xs + (long)tl * DP * 64 + l;
          double* dst = coords + tl * (DP + 1) * 64 + l;
          double xx = 0.0;
  #pragma unroll
          for (int k = 0; k < DP; ++k) {
            const double v = src[k * 64];
            dst[k * 64] = v;
            xx = fma(v, v, xx);
          }
          dst[DP * 64] = xx;
        }
        xs = coords;
        __syncthreads();
      }
      if constexpr (wide_eval(DP, XLDS)) {
        __syncthreads();  // previous evaluation's readers are done
        const d2t* src = reinterpret_cast<const d2t*>(xs);
        d2t* dst = reinterpret_cast<d2t*>(coords);
        for (int i = threadIdx.x; i < wtab / 2; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
      }
      // sample tickets are drawn ONE AHEAD: the atomic's round trip to L2 overlaps the current sample instead of stalling
      // the wave between samples (each wave ends up drawing one ticket it does not use)
      unsigned int ticket = 0;
      unsigned int* next = P.next_sample + (long)e * kTicketStride;  // one cache line per evaluation
      if (lane == 0) ticket = atomicAdd(next, 1u);
      unsigned long long tot_val = 0, tot_grad = 0;
      while (true) {
        const unsigned int sl = (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket);
        if (sl >= (unsigned int)P.num_local) break;
        if (lane == 0) ticket = atomicAdd(next, 1u);
        kg_sample<DP, G, SMALL, XLDS>(P, e, (int)sl, xs, aw, zb, smem, cst, lane, tot_val, tot_grad);
      }
      if (lane == 0 && (tot_val | tot_grad) != 0) {
        atomicAdd(&P.counters[2 * e], tot_val);
        atomicAdd(&P.counters[2 * e + 1], tot_grad);
      }
    }
  }
};
template <int DP, int G, bool XLDS, bool SMALL>
__global__ __launch_bounds__(SMALL ? 1024 : 512) void kg_mc_kernel(KgMcParams P) {
  kg_mc_kernel_body<DP, G, XLDS, SMALL>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P);
}

template <int DP, int G, bool XLDS, bool SMALL>
inline void launch_inst2(const KgMcParams& P, int blocks, int waves, size_t shm, hipStream_t s) {
  auto kern = kg_mc_kernel<DP, G, XLDS, SMALL>;
  launch_kernel_ens<kg_mc_kernel_body<DP, G, XLDS, SMALL>, (SMALL ? 1024 : 512)>(kern, dim3(blocks), dim3(waves * 64), shm, s, P);
  MOE_HIP_CHECK(hipGetLastError());
}

// one derivative-slot count: the LDS coordinate table (padded dimension <= 16 only; waves > 8 selects its many-wavefront
// instantiation) or coordinates streamed from L2
template <int DP, int G>
inline void launch_g(const KgMcParams& P, bool xlds, int blocks, int waves, size_t shm, hipStream_t s) {
  if constexpr (DP <= 16) {
    if (xlds && waves > 8) return launch_inst2<DP, G, true, true>(P, blocks, waves, shm, s);
    if (xlds) return launch_inst2<DP, G, true, false>(P, blocks, waves, shm, s);
  }
  launch_inst2<DP, G, false, false>(P, blocks, waves, shm, s);
}

template <int DP>
void launch_dp(const KgMcParams& P, int G, bool xlds, int blocks, int waves, size_t shm, hipStream_t s) {
  if constexpr (DP > 16) {  // the wide padded dimensions (24, 32) are built for a reduced set: slots {0, 4}, streamed coordinates
    if (xlds || waves > 8) throw Error(MOE_ERR_RUNTIME, "d > 16: the wave-per-sample MC kernel streams coordinates from L2 only");
  }
  switch (G) {
    case 0: return launch_g<DP, 0>(P, xlds, blocks, waves, shm, s);
    case 1: if constexpr (DP <= 16) return launch_g<DP, 1>(P, xlds, blocks, waves, shm, s); break;
    case 2: if constexpr (DP <= 16) return launch_g<DP, 2>(P, xlds, blocks, waves, shm, s); break;
    case 3: if constexpr (DP <= 16) return launch_g<DP, 3>(P, xlds, blocks, waves, shm, s); break;
    case 4: return launch_g<DP, 4>(P, xlds, blocks, waves, shm, s);
  }
  throw Error(MOE_ERR_RUNTIME, "unsupported derivative-slot count in the MC kernel");
}

}  // namespace mc
}  // namespace moe
