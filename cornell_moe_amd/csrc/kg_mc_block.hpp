// cornell_moe_amd/csrc/kg_mc_block.hpp -- the workgroup-per-sample q-KG / d-KG Monte-Carlo kernel kg_mc_block_kernel (gfx950): its
// point terms and weights, the evaluator BlockEval, the kernel and its launchers, over the shared core kg_mc.hpp and the LDS-state
// line search kg_mc_lds.hpp.  Instantiated by kg_mc_dp{4,8,12,16}b.hip and kg_mc_dp{24,32}.hip.
#pragma once
#include "kg_mc.hpp"
#include "kg_mc_lds.hpp"

namespace moe {
namespace mc {

// Workgroup-per-sample variant for training sets whose coordinate table + per-wave weight slabs no longer fit the 160 KB of
// LDS (e.g. d-KG at n = 2000, d = 12, g = 3: 196 KB of coordinates, 80 KB of weights per sample).  ONE sample at a time
// per workgroup of 8 wavefronts; the point tiles are split statically over the waves and over the two on-chip stores:
//   * the first T_L tiles live in LDS (coordinates, loaded once per workgroup, and the current sample's weights), each wave
//     sweeping its share with the same software-pipelined loop as the wave-per-sample kernel;
//   * the last 8 * TR tiles live in REGISTERS: TR tiles per wave, coordinates for the kernel's lifetime and weights per
//     sample (the register file, 512 KB per CU, is the largest on-chip store; at TR = 2, d = 12, g = 3 that is 68 VGPRs).
// The host picks the smallest TR in {0, 2, 4} for which the LDS part fits.  All waves run the same line search in lockstep:
// each pass ends with one wavefront sum per wave, one LDS slot per wave, ONE __syncthreads, and a fixed-order sum of the
// per-wave partials, so every wave takes bit-identical decisions.

// One point's contribution to the accumulators (shared by the LDS-tile loop and the register tiles).
template <int DP, int G, bool WG, int COV>
__device__ __forceinline__ void point_terms(const double (&cx)[DP], const double (&cw)[1 + G], const double (&xq)[DP],
                                            const double* __restrict__ etab, double& accf, double (&accg)[DP],
                                            double (&accd)[G > 0 ? G : 1]) {
  double diff[DP];
  double r2 = 1.0e-300;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    diff[k] = cx[k] - xq[k];
    r2 = fma(diff[k], diff[k], r2);
  }
  double base, first, second;
  radial3<COV, (WG || G > 0), (WG && G > 0)>(r2, etab, base, first, second);
  double sd = 0.0;
  if (G > 0) {
#pragma unroll
    for (int a = 0; a < G; ++a) sd = fma(cw[1 + a], diff[a], sd);
  }
  accf = fma(cw[0], base, accf);
  if (G > 0) accf = fma(first, sd, accf);
  if (WG) {
    double coef = cw[0] * first;
    if (G > 0) {
      coef = fma(second, sd, coef);
#pragma unroll
      for (int a = 0; a < G; ++a) accd[a] = fma(first, cw[1 + a], accd[a]);
    }
#pragma unroll
    for (int k = 0; k < DP; ++k) accg[k] = fma(coef, diff[k], accg[k]);
  }
}

// One point's contribution to T Armijo trial values f(x0 + alpha_t dv), alpha_t = al[t] (frame coordinates; see
// eval_multi_loop for the idea).  With diff0 = x_j - x0:
//   r2_t = |diff0 - alpha_t dv|^2 = A - 2 alpha_t B + alpha_t^2 |dv|^2,   A = |diff0|^2, B = diff0 . dv   (3 DP instructions once),
//   sum_a w_a (diff0 - alpha_t dv)_a = sdA - alpha_t sdB                                                  (2 G once),
// so a trial costs two fmas and a max for its distance instead of 2 DP, and one for its derivative-weight sum instead of G.
// Centred on x0 (the current iterate, inside the domain), so A and B are of the size of the distances themselves.
template <int DP, int G, int COV, int T>
__device__ __forceinline__ void point_terms_multi(const double (&cx)[DP], const double (&cw)[1 + G], const double (&x0)[DP],
                                                  const double (&dv)[DP], const double (&al)[T], double dd,
                                                  const double* __restrict__ etab, double (&acc)[T]) {
  double A = 1.0e-300, B = 0.0, sdA = 0.0, sdB = 0.0;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const double d0 = cx[k] - x0[k];
    A = fma(d0, d0, A);
    B = fma(d0, dv[k], B);
    if (G > 0 && k < G) {
      sdA = fma(cw[1 + (k < G ? k : 0)], d0, sdA);
      sdB = fma(cw[1 + (k < G ? k : 0)], dv[k], sdB);
    }
  }
  const double mB2 = -2.0 * B;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const double r2 = fmax(fma(al[t], fma(al[t], dd, mB2), A), 1.0e-300);
    double base, first, second;
    radial3<COV, (G > 0), false>(r2, etab, base, first, second);
    acc[t] = fma(cw[0], base, acc[t]);
    if (G > 0) acc[t] = fma(first, fma(-al[t], sdB, sdA), acc[t]);
  }
}

template <int DP, int G, int TR>
struct BlockEval {
  double cx[TR > 0 ? TR : 1][DP];     // register tiles: scaled coordinates (resident for the kernel's life)
  double cw[TR > 0 ? TR : 1][1 + G];  // register tiles: weights of the current sample
  const double* __restrict__ xl;      // this wave's LDS tiles: coordinates [ntl][DP][64] (+lane)
  const double* __restrict__ wl;      // this wave's LDS tiles: weights of the current sample [ntl][1+G][64] (+lane)
  int ntl;                            // number of LDS tiles of this wave
  const double* __restrict__ etab;
  double* __restrict__ part;  // LDS [2][kMaxBlockWaves][kPartLen]
  const double* inv_lp;
  double mean;
  int nw, wave, lane, cov_type, par;
#if MOE_BLOCK_PROF
  unsigned long long c_acc = 0, c_red = 0, c_bar = 0, c_post = 0, c_n = 0, c_gtot = 0, c_gn = 0;
  unsigned long long c_tot = 0;        // cycles inside passes (all kinds)
  unsigned long long seg[4] = {0, 0, 0, 0};  // line_search_lds: cycles OUTSIDE the passes, by segment of a step
  unsigned long long seg_last = 0, seg_tot = 0;
  __device__ __forceinline__ void seg_mark(int i) {  // closes segment i: wall clock since the last mark minus pass time since then
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    seg[i] += (now - seg_last) - (c_tot - seg_tot);
    seg_last = now;
    seg_tot = c_tot;
  }
#endif

  template <bool WG, int COV>
  __device__ __forceinline__ void accumulate(const double (&xq)[DP], double& accf, double (&accg)[DP],
                                             double (&accd)[G > 0 ? G : 1]) {
    // ---- LDS tiles: software-pipelined (next tile requested before the current one is consumed) ----
    if (ntl > 0) {
      lds_tile_ptr xt = (lds_tile_ptr)xl;  // single ds_read_b64 each (see lds_tile_ptr)
      lds_tile_ptr wt = (lds_tile_ptr)wl;
      double c0[DP], w0[1 + G];
#pragma unroll
      for (int k = 0; k < DP; ++k) c0[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) w0[a] = wt[a * 64];
#pragma unroll 2
      for (int t = 0; t < ntl; ++t) {
        double c1[DP], w1[1 + G];
        if (t + 1 < ntl) {
          xt += DP * 64;
          wt += (1 + G) * 64;
        }
#pragma unroll
        for (int k = 0; k < DP; ++k) c1[k] = xt[k * 64];
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) w1[a] = wt[a * 64];
        point_terms<DP, G, WG, COV>(c0, w0, xq, etab, accf, accg, accd);
#pragma unroll
        for (int k = 0; k < DP; ++k) c0[k] = c1[k];
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) w0[a] = w1[a];
      }
    }
    // ---- register tiles ----
#pragma unroll
    for (int t = 0; t < TR; ++t) point_terms<DP, G, WG, COV>(cx[t], cw[t], xq, etab, accf, accg, accd);
  }

  // Value of the objective at TWO query points in one sweep over the tiles (the coordinates and weights of a point are
  // loaded once and used for both): the pass costs twice the arithmetic but ONE wave reduction round, one barrier and one
  // decision round -- and in this kernel a pass is dominated by exactly those (see line_search_lds).
  template <int COV>
  __device__ __forceinline__ void accumulate2(const double (&xa)[DP], const double (&xb)[DP], double& fa, double& fb) {
    double dg[DP], dd[G > 0 ? G : 1];  // unused gradient accumulators of the value-only instantiation
    if (ntl > 0) {
      lds_tile_ptr xt = (lds_tile_ptr)xl;  // single ds_read_b64 each (see lds_tile_ptr)
      lds_tile_ptr wt = (lds_tile_ptr)wl;
      double c0[DP], w0[1 + G];
#pragma unroll
      for (int k = 0; k < DP; ++k) c0[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) w0[a] = wt[a * 64];
#pragma unroll 1
      for (int t = 0; t < ntl; ++t) {
        double c1[DP], w1[1 + G];
        if (t + 1 < ntl) {
          xt += DP * 64;
          wt += (1 + G) * 64;
        }
#pragma unroll
        for (int k = 0; k < DP; ++k) c1[k] = xt[k * 64];
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) w1[a] = wt[a * 64];
        point_terms<DP, G, false, COV>(c0, w0, xa, etab, fa, dg, dd);
        point_terms<DP, G, false, COV>(c0, w0, xb, etab, fb, dg, dd);
#pragma unroll
        for (int k = 0; k < DP; ++k) c0[k] = c1[k];
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) w0[a] = w1[a];
      }
    }
#pragma unroll
    for (int t = 0; t < TR; ++t) {
      point_terms<DP, G, false, COV>(cx[t], cw[t], xa, etab, fa, dg, dd);
      point_terms<DP, G, false, COV>(cx[t], cw[t], xb, etab, fb, dg, dd);
    }
  }

  // T trial values along one line in one sweep (point_terms_multi): one set of coordinate / weight loads, one reduction round,
  // one barrier and one decision round per T trials.
  template <int COV, int T>
  __device__ __forceinline__ void accumulateT(const double (&x0)[DP], const double (&dv)[DP], const double (&al)[T], double dd,
                                              double (&acc)[T]) {
    if (ntl > 0) {
      lds_tile_ptr xt = (lds_tile_ptr)xl;  // single ds_read_b64 each (see lds_tile_ptr)
      lds_tile_ptr wt = (lds_tile_ptr)wl;
      double c0[DP], w0[1 + G];
#pragma unroll
      for (int k = 0; k < DP; ++k) c0[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) w0[a] = wt[a * 64];
#pragma unroll 1
      for (int t = 0; t < ntl; ++t) {
        double c1[DP], w1[1 + G];
        if (t + 1 < ntl) {
          xt += DP * 64;
          wt += (1 + G) * 64;
        }
#pragma unroll
        for (int k = 0; k < DP; ++k) c1[k] = xt[k * 64];
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) w1[a] = wt[a * 64];
        point_terms_multi<DP, G, COV, T>(c0, w0, x0, dv, al, dd, etab, acc);
#pragma unroll
        for (int k = 0; k < DP; ++k) c0[k] = c1[k];
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) w0[a] = w1[a];
      }
    }
#pragma unroll
    for (int t = 0; t < TR; ++t) point_terms_multi<DP, G, COV, T>(cx[t], cw[t], x0, dv, al, dd, etab, acc);
  }

  // Up to kMaxTrials Armijo trials x0 + alpha 2^-t dv (frame coordinates) in one pass, followed by the reference's sequence of
  // decisions over them with compile-time indices (gpp_optimization.hpp:752-769; see WaveEval::armijo_t).  The caller has
  // checked that no trial needs clamp_query.
  static constexpr int kMaxTrials = 5;
  template <int T>
  __device__ __forceinline__ void armijo_t(const double* __restrict__ x0p, const double* __restrict__ dvp, double dd, double f0,
                                           double norm, double& alpha_n, int& search, double& ftrial, bool& done,
                                           unsigned long long& n_val) {
    double x0[DP], dv[DP];  // (from the wave's LDS scratch: see line_search_lds)
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      x0[k] = x0p[k];
      dv[k] = dvp[k];
    }
    double al[T], acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      al[t] = (t == 0) ? alpha_n : 0.5 * al[t > 0 ? t - 1 : 0];
      acc[t] = 0.0;
    }
    MOE_PROF_T(t0);
    if (cov_type == MOE_COV_SQUARE_EXPONENTIAL)
      accumulateT<MOE_COV_SQUARE_EXPONENTIAL, T>(x0, dv, al, dd, acc);
    else
      accumulateT<MOE_COV_MATERN_NU_2P5, T>(x0, dv, al, dd, acc);
    MOE_PROF_T(t1);
    double* slot = part + (par * kMaxBlockWaves + wave) * kPartLen;
    wave_sum_packed_store<T>(acc, slot, lane);
    MOE_PROF_T(t2);
    __syncthreads();
    MOE_PROF_T(t3);
    const double* all = part + par * kMaxBlockWaves * kPartLen;
    par ^= 1;
    double f[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      double tot = 0.0;
#pragma unroll
      for (int w = 0; w < kMaxBlockWaves; ++w) tot += (w < nw) ? all[w * kPartLen + t] : 0.0;  // (reads issued together)
      f[t] = -(mean + uniform(tot));
    }
    MOE_PROF_T(t4);
    MOE_PROF_ADD(c_acc, t0, t1);
    MOE_PROF_ADD(c_red, t1, t2);
    MOE_PROF_ADD(c_bar, t2, t3);
    MOE_PROF_ADD(c_post, t3, t4);
    MOE_PROF_ADD(c_tot, t0, t4);
#if MOE_BLOCK_PROF
    c_n++;
#endif
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (!done) {
        ftrial = f[t];
        n_val++;
        if (ftrial - f0 > 0.5 * alpha_n * norm) {
          done = true;
        } else {
          alpha_n *= 0.5;
          if (++search >= 30) done = true;
        }
      }
    }
  }
  __device__ __forceinline__ void armijo_batch(int want, const double* __restrict__ x0, const double* __restrict__ dv, double dd,
                                               double f0, double norm, double& alpha_n, int& search, double& ftrial, bool& done,
                                               unsigned long long& n_val) {
    switch (want) {
      case 2: armijo_t<2>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
      case 3: armijo_t<3>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
      case 4: armijo_t<4>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
      default: armijo_t<5>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
    }
  }

  __device__ __forceinline__ void eval2(const double (&xa_in)[DP], const double (&xb_in)[DP], double& fa_out, double& fb_out) {
    double fa = 0.0, fb = 0.0;
    double xa[DP], xb[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      xa[k] = xa_in[k];
      xb[k] = xb_in[k];
    }
    clamp_query<DP>(xa);
    clamp_query<DP>(xb);
    MOE_PROF_T(t0);
    if (cov_type == MOE_COV_SQUARE_EXPONENTIAL)
      accumulate2<MOE_COV_SQUARE_EXPONENTIAL>(xa, xb, fa, fb);
    else
      accumulate2<MOE_COV_MATERN_NU_2P5>(xa, xb, fa, fb);
    MOE_PROF_T(t1);
    double* slot = part + (par * kMaxBlockWaves + wave) * kPartLen;
    const double sa = wave_sum_uniform(fa), sb = wave_sum_uniform(fb);
    if (lane == 0) {
      slot[0] = sa;
      slot[1] = sb;
    }
    MOE_PROF_T(t2);
    __syncthreads();
    MOE_PROF_T(t3);
    const double* all = part + par * kMaxBlockWaves * kPartLen;
    par ^= 1;
    double ta = 0.0, tb = 0.0;
#pragma unroll
    for (int w = 0; w < kMaxBlockWaves; ++w) {  // fixed trip count: the eight reads are issued together
      ta += (w < nw) ? all[w * kPartLen] : 0.0;
      tb += (w < nw) ? all[w * kPartLen + 1] : 0.0;
    }
    fa_out = -(mean + uniform(ta));
    fb_out = -(mean + uniform(tb));
    MOE_PROF_T(t4);
    MOE_PROF_ADD(c_acc, t0, t1);
    MOE_PROF_ADD(c_red, t1, t2);
    MOE_PROF_ADD(c_bar, t2, t3);
    MOE_PROF_ADD(c_post, t3, t4);
    MOE_PROF_ADD(c_tot, t0, t4);
#if MOE_BLOCK_PROF
    c_n++;
#endif
  }

  // the query read from the wave's LDS scratch (line_search_lds)
  template <bool WG>
  __device__ __forceinline__ double eval_p(const double* __restrict__ xq_ptr, double (&grad)[DP]) {
    double xq[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xq[k] = xq_ptr[k];
    return eval<WG>(xq, grad);
  }
  // value + gradient with the gradient handed back ONE COMPONENT PER LANE (lane k < DP: d f / d x_k in the original units,
  // scale_l = this lane's frame scale): the cross-wave sums are lane-distributed anyway, and fetching them as wave-uniform
  // values cost 2 (1 + DP + G) v_readlane into a scalar file that was already spilling
  __device__ __forceinline__ double eval_p_lane(const double* __restrict__ xq_ptr, double scale_l, double& grad_l) {
    double xq[DP], unused[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xq[k] = xq_ptr[k];
    return eval<true, true>(xq, unused, scale_l, &grad_l);
  }

  template <bool WG, bool LANEOUT = false>
  __device__ __forceinline__ double eval(const double (&xq_in)[DP], double (&grad)[DP], double scale_l = 0.0,
                                         double* grad_l = nullptr) {
    double accf = 0.0, accg[DP], accd[G > 0 ? G : 1];
    double xq[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xq[k] = xq_in[k];
    clamp_query<DP>(xq);
#pragma unroll
    for (int k = 0; k < DP; ++k) accg[k] = 0.0;
#pragma unroll
    for (int a = 0; a < (G > 0 ? G : 1); ++a) accd[a] = 0.0;
    MOE_PROF_T(t0);
    if (cov_type == MOE_COV_SQUARE_EXPONENTIAL)
      accumulate<WG, MOE_COV_SQUARE_EXPONENTIAL>(xq, accf, accg, accd);
    else
      accumulate<WG, MOE_COV_MATERN_NU_2P5>(xq, accf, accg, accd);
    MOE_PROF_T(t1);
    double* slot = part + (par * kMaxBlockWaves + wave) * kPartLen;
    if (WG) {
      double all_sums[1 + DP + (G > 0 ? G : 0)];  // f | gradient sums | derivative-weight sums: one packed reduction
      all_sums[0] = accf;
#pragma unroll
      for (int k = 0; k < DP; ++k) all_sums[1 + k] = accg[k];
      if (G > 0) {
#pragma unroll
        for (int a = 0; a < G; ++a) all_sums[1 + DP + a] = accd[a];
      }
      wave_sum_packed_store<1 + DP + (G > 0 ? G : 0)>(all_sums, slot, lane);
    } else {
      const double sf = wave_sum_uniform(accf);
      if (lane == 0) slot[0] = sf;
    }
    MOE_PROF_T(t2);
    __syncthreads();
    MOE_PROF_T(t3);
    MOE_PROF_ADD(c_acc, t0, t1);
    MOE_PROF_ADD(c_red, t1, t2);
    MOE_PROF_ADD(c_bar, t2, t3);
#if MOE_BLOCK_PROF
    c_n++;
#endif
    const double* all = part + par * kMaxBlockWaves * kPartLen;
    par ^= 1;
    double f;
    if (WG) {
      // One component per LANE: lane l sums slot entry l over the waves (eight independent LDS reads, wave order), then the
      // components come back as wave-uniform values through v_readlane -- instead of (1 + DP + G) x nw dependent
      // broadcast reads, each a full LDS round trip (12k cycles per gradient pass at DP = 12, G = 3).
      double comp = 0.0;
      const int lc = lane < kPartLen ? lane : 0;
#pragma unroll
      for (int w = 0; w < kMaxBlockWaves; ++w) comp += (w < nw) ? all[w * kPartLen + lc] : 0.0;
      auto take = [&](int idx) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(comp), idx);
        const int hi = __builtin_amdgcn_readlane(__double2hiint(comp), idx);
        return __hiloint2double(hi, lo);
      };
      f = take(0);
      if (LANEOUT) {
        auto from_lane = [&](int src) {  // comp of lane `src` (per-lane index): two ds_bpermute_b32
          const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(comp));
          const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(comp));
          return __hiloint2double(hi, lo);
        };
        double v = from_lane(min(lane + 1, 63));
        if (G > 0) {
          const double vd = from_lane(min(lane + 1 + DP, 63));
          if (lane < G) v -= vd;
        }
        *grad_l = -(v * scale_l);
      } else {
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          double v = take(1 + k);
          if (G > 0 && k < G) v -= take(1 + DP + (k < G ? k : 0));
          grad[k] = -(v * inv_lp[k]);
        }
      }
    } else {
      f = 0.0;
#pragma unroll
      for (int w = 0; w < kMaxBlockWaves; ++w) f += (w < nw) ? all[w * kPartLen] : 0.0;
    }
    const double fret = -(mean + uniform(f));
    MOE_PROF_T(t4);
    MOE_PROF_ADD(c_post, t3, t4);
    MOE_PROF_ADD(c_tot, t0, t4);
#if MOE_BLOCK_PROF
    if (WG) {
      c_gtot += t4 - t0;
      c_gn++;
    }
#endif
    return fret;
  }
};

// v(j, a) of the weight block for point j (see file header), alpha and the derivative scaling folded in.  The W loads
// of 16 columns x (1 + G) rows are issued together (64 independent L2 loads per lane and round at G = 3): issued four at a
// time this phase took a quarter of the kernel at m = 16 (latency x 64 rounds per wave and sample).
template <int G>
__device__ __forceinline__ void point_weights(const KgMcParams& P, const double* __restrict__ We, const double* __restrict__ zb,
                                              int j, double (&w)[1 + G]) {
  const int n = P.n, u = P.u, m = P.m, g1 = 1 + P.g;
  double v[1 + G];
#pragma unroll
  for (int a = 0; a < 1 + G; ++a) v[a] = (a < g1 && j < n) ? P.KinvY[(long)j * g1 + a] : 0.0;
  if (j < n) {
    // the 1 + G rows of a point are contiguous in a column of W: with an even row count they are read as 16-byte pairs, so
    // that a wavefront's load covers each cache line once (row by row, a lane stride of (1 + G) doubles touches every line
    // 1 + G times and the phase becomes L2 -> CU bandwidth: 4 MB per sample instead of 1 MB at g = 3)
    typedef double d2 __attribute__((ext_vector_type(2)));
    const bool pairs = (G & 1) == 1 && g1 == 1 + G && (P.N & 1) == 0 && (reinterpret_cast<size_t>(We) & 15) == 0;
    for (int c0 = 0; c0 < m; c0 += 16) {
      double l[1 + G][16];
      if (pairs) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const d2* src = reinterpret_cast<const d2*>(We + (long)j * g1 + (long)min(c0 + i, m - 1) * P.N);
#pragma unroll
          for (int a2 = 0; a2 < (1 + G) / 2; ++a2) {
            const d2 pr = src[a2];
            l[2 * a2][i] = pr.x;
            l[2 * a2 + ((1 + G) > 1 ? 1 : 0)][i] = pr.y;
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {  // column outer: the rows of one point share their cache lines
#pragma unroll
          for (int a = 0; a < 1 + G; ++a)
            l[a][i] = We[(long)j * g1 + (a < g1 ? a : 0) + (long)min(c0 + i, m - 1) * P.N];
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const double beta = zb[kMaxMB + min(c0 + i, kMaxMB - 1)];  // 0 beyond m
#pragma unroll
        for (int a = 0; a < 1 + G; ++a) v[a] = fma(-l[a][i], beta, v[a]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 1 + G; ++a) {
    double t = 0.0;
    if (a < g1) {
      t = v[a];
      if (j >= n) t = (j < n + u) ? zb[kMaxMB + (j - n) * g1 + a] : 0.0;
      // fold alpha and, for derivative weights, the -1/l of (x - X)_{d_a} / l^2 = -diff_scaled[a] / l
      t *= (a == 0) ? P.alpha : -P.alpha * P.inv_lp[a > 0 ? a - 1 : 0];
    }
    w[a] = t;
  }
}

// The same weights read back from the precomputed table V (kg_sample_weights_kernel): Vs = V + sample * N.  Rows of a
// point are contiguous, so with an even row count they travel as 16-byte pairs (see point_weights).
template <int G>
__device__ __forceinline__ void point_weights_pre(const KgMcParams& P, const double* __restrict__ Vs,
                                                  const double* __restrict__ zb, int j, double (&w)[1 + G]) {
  const int n = P.n, u = P.u, g1 = 1 + P.g;
  typedef double d2 __attribute__((ext_vector_type(2)));
  const bool pairs = (G & 1) == 1 && g1 == 1 + G && (P.N & 1) == 0 && (reinterpret_cast<size_t>(Vs) & 15) == 0;
  if (j < n) {
    if (pairs) {
      const d2* src = reinterpret_cast<const d2*>(Vs + (long)j * g1);
#pragma unroll
      for (int a2 = 0; a2 < (1 + G) / 2; ++a2) {
        const d2 pr = src[a2];
        w[2 * a2] = pr.x;
        w[2 * a2 + ((1 + G) > 1 ? 1 : 0)] = pr.y;
      }
    } else {
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) w[a] = (a < g1) ? Vs[(long)j * g1 + a] : 0.0;
    }
  } else {
#pragma unroll
    for (int a = 0; a < 1 + G; ++a) {
      double t = 0.0;
      if (a < g1 && j < n + u) {
        t = zb[kMaxMB + (j - n) * g1 + a];
        t *= (a == 0) ? P.alpha : -P.alpha * P.inv_lp[a > 0 ? a - 1 : 0];
      }
      w[a] = t;
    }
  }
}

template <int DP, int G, int TR>
struct kg_mc_block_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P, int num_lds_tiles) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // LDS: [64] exp table | z / beta scratch of draw_z_beta [0, 2 kMaxM) = [0, kMaxMB), beta of the sample [kMaxMB, 2 kMaxMB) |
    //      partial slots [2][8][kPartLen] | control words (2 doubles) |
    //      line-search state [8][kLsRows kMaxDimPadded] | coordinates of the LDS tiles [T_L][DP][64] | their weights [T_L][1+G][64]
    double* etab = smem;
    double* zb = smem + kExpTabLen;
    double* part = zb + 2 * kMaxMB;
    int* ctl = reinterpret_cast<int*>(part + 2 * kMaxBlockWaves * kPartLen);  // [0] sample index, [1] best discretised point
    double* stw = part + 2 * kMaxBlockWaves * kPartLen + 2 + (threadIdx.x >> 6) * (kLsRows * kMaxDimPadded);
    double* ldsx = smem + kBlockFixed;
    double* ldsw = ldsx + (long)num_lds_tiles * DP * 64;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    const int m = P.m;
    const int size = P.dim - P.f;
    // LDS tiles [0, T_L) are dealt to the waves in contiguous runs; register tiles are T_L + wave * TR + t
    const int TL = num_lds_tiles;
    const int per = (TL + nw - 1) / nw;
    const int tl0 = min(wave * per, TL), tl1 = min(tl0 + per, TL);
    if (threadIdx.x < kExpTabLen) etab[threadIdx.x] = kExp2Tab64[threadIdx.x];
    BlockEval<DP, G, TR> ev;
    ev.xl = ldsx + (long)tl0 * DP * 64 + lane;
    ev.wl = ldsw + (long)tl0 * (1 + G) * 64 + lane;
    ev.ntl = tl1 - tl0;
    ev.etab = etab;
    ev.part = part;
    ev.inv_lp = P.inv_lp;
    ev.mean = P.mean;
    ev.nw = nw;
    ev.wave = wave;
    ev.lane = lane;
    ev.cov_type = P.cov_type;
    ev.par = 0;
    // (which evaluations this workgroup serves, and in what order: kg_mc.hpp next_evaluation; its LDS word is the sample index's)
    bool moved = false;
    for (int e = first_evaluation(P, blockIdx); e >= 0; e = next_evaluation(P, gridDim, e, moved, ctl)) {
      const double* tab = P.XsTab + (long)e * P.tab_stride;
      const double* rec = P.blob + (long)e * P.rec.stride;
      const double* Lsm = rec + P.rec.L;
      const double* We = P.W + (long)e * P.w_stride;
      __syncthreads();  // previous evaluation's readers of the LDS coordinates are done
      if constexpr (DP > 16) {  // (the table of the wide dimensions holds its rows in pairs: WideEval)
        for (int t = threadIdx.x; t < TL * DP * 64; t += blockDim.x) {
          const int l = t & 63, r = (t >> 6) % DP, tile = (t >> 6) / DP;
          ldsx[t] = tab[(((long)tile * (DP / 2) + (r >> 1)) * 64 + l) * 2 + (r & 1)];
        }
      } else {
        for (int t = threadIdx.x; t < TL * DP * 64; t += blockDim.x) ldsx[t] = tab[t];
      }
  #pragma unroll
      for (int t = 0; t < TR; ++t) {
        const int tile = TL + wave * TR + t;
  #pragma unroll
        for (int k = 0; k < DP; ++k) ev.cx[t][k] = (tile < P.ntiles) ? tab[((long)tile * DP + k) * 64 + lane] : 0.0;
      }
  #if MOE_BLOCK_PROF
      unsigned long long p_tick = 0, p_setup = 0, p_w = 0, p_ls = 0, p_zb = 0, p_scan = 0;
  #endif
      while (true) {
        MOE_PROF_T(k0);
        if (threadIdx.x == 0) ctl[0] = (int)atomicAdd(&P.next_sample[(long)e * kTicketStride], 1u);
        __syncthreads();
        const int sl = ctl[0];
        if (sl >= P.num_local) break;
        const int s = P.first_sample + sl;
        double zc = 0.0, bc = 0.0;
        MOE_PROF_T(k1);
        if (wave == 0) {
          MOE_PROF_T(k1a0);
          if (P.best_j != nullptr) {
            // beta and the discretised-set winner depend on z alone: a pre-pass computed them for every sample with the whole
            // chip (here they cost one wavefront 10 % of the sample while seven wait at the barrier)
            const long so0 = (long)e * P.num_local + sl;
            for (int c = lane; c < kMaxMB; c += 64) zb[kMaxMB + c] = (c < m) ? P.beta[so0 * m + c] : 0.0;
            if (lane == 0) ctl[1] = P.best_j[so0];
          } else {  // (m <= 64 only: one lane per component)
            draw_z_beta(P, Lsm, s, lane, zb, zc, bc);
            zb[kMaxMB + lane] = bc;
            zb[kMaxMB + 64 + lane] = 0.0;
            const int bj = discrete_scan(P, rec, zb, lane);
            if (lane == 0) ctl[1] = bj;
          }
          MOE_PROF_T(k1a);
          MOE_PROF_T(k1b);
          (void)zc;
          MOE_PROF_ADD(p_zb, k1a0, k1a);
          MOE_PROF_ADD(p_scan, k1a, k1b);
        }
        __syncthreads();
        MOE_PROF_T(k2);
        // ---- weights of this wave's points for this sample: LDS tiles into the LDS slab, register tiles into registers ----
        {
          double* wdst = ldsw + (long)tl0 * (1 + G) * 64 + lane;
          if (P.V != nullptr) {
            const double* Vs = P.V + ((long)e * P.num_local + sl) * P.v_stride;
  #pragma unroll 2
            for (int t = tl0; t < tl1; ++t) {
              double w[1 + G];
              point_weights_pre<G>(P, Vs, zb, t * 64 + lane, w);
  #pragma unroll
              for (int a = 0; a < 1 + G; ++a) wdst[a * 64] = w[a];  // read back only by this lane
              wdst += (1 + G) * 64;
            }
  #pragma unroll
            for (int t = 0; t < TR; ++t) point_weights_pre<G>(P, Vs, zb, (TL + wave * TR + t) * 64 + lane, ev.cw[t]);
          } else {
  #pragma unroll 1
            for (int t = tl0; t < tl1; ++t) {
              double w[1 + G];
              point_weights<G>(P, We, zb, t * 64 + lane, w);
  #pragma unroll
              for (int a = 0; a < 1 + G; ++a) wdst[a * 64] = w[a];  // read back only by this lane
              wdst += (1 + G) * 64;
            }
  #pragma unroll
            for (int t = 0; t < TR; ++t) point_weights<G>(P, We, zb, (TL + wave * TR + t) * 64 + lane, ev.cw[t]);
          }
        }
        MOE_PROF_T(k3);
        const int best_j = ctl[1];
        const double* disc = rec + P.rec.disc;
        double x[DP];
  #pragma unroll
        for (int k = 0; k < DP; ++k) x[k] = (k < size) ? disc[(long)best_j * size + k] : ((k < P.dim) ? 1.0 : 0.0);
        unsigned long long n_val = 0, n_grad = 0;
        const double fcur = line_search_lds<DP, G>(P, ev, stw, x, n_val, n_grad);
        MOE_PROF_T(k4);
        MOE_PROF_ADD(p_tick, k0, k1);
        MOE_PROF_ADD(p_setup, k1, k2);
        MOE_PROF_ADD(p_w, k2, k3);
        MOE_PROF_ADD(p_ls, k3, k4);
        if (wave == 0) {
          const long so = (long)e * P.num_local + sl;
          if (lane == 0) {
            P.best_value[so] = fcur;
            atomicAdd(&P.counters[2 * e], n_val);
            atomicAdd(&P.counters[2 * e + 1], n_grad);
          }
          if (lane < DP) {
            double v = 0.0;
  #pragma unroll
            for (int k = 0; k < DP; ++k)
              if (lane == k) v = x[k];
            P.best_point[so * DP + lane] = v;
          }
          if (P.best_j == nullptr && lane < m) P.beta[so * m + lane] = bc;  // (the pre-pass already stored it)
        }
      }
  #if MOE_BLOCK_PROF
      if (threadIdx.x == 0) {  // wave 0's view: [0..3] ticket, z/beta/scan, weights, line search; [4..8] inside the passes
        atomicAdd(&P.prof[0], p_tick);
        atomicAdd(&P.prof[1], p_setup);
        atomicAdd(&P.prof[2], p_w);
        atomicAdd(&P.prof[3], p_ls);
        atomicAdd(&P.prof[4], ev.c_acc);
        atomicAdd(&P.prof[5], ev.c_red);
        atomicAdd(&P.prof[6], ev.c_bar);
        atomicAdd(&P.prof[7], ev.c_post);
        atomicAdd(&P.prof[8], ev.c_n);
        atomicAdd(&P.prof[9], ev.c_gtot);
        atomicAdd(&P.prof[10], ev.c_gn);
        atomicAdd(&P.prof[11], p_zb);
        atomicAdd(&P.prof[12], p_scan);
        atomicAdd(&P.prof[13], ev.seg[0]);
        atomicAdd(&P.prof[14], ev.seg[1]);
        atomicAdd(&P.prof[15], ev.seg[2] + ev.seg[3]);
      }
  #endif
    }
  }
};
template <int DP, int G, int TR>
__global__ __launch_bounds__(512) void kg_mc_block_kernel(KgMcParams P, int num_lds_tiles) {
  kg_mc_block_kernel_body<DP, G, TR>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, num_lds_tiles);
}

template <int DP, int G, int TR>
inline void launch_block_inst(const KgMcParams& P, int num_lds_tiles, int blocks, int waves, hipStream_t s) {
  const size_t shm = sizeof(double) * (kBlockFixed + (size_t)num_lds_tiles * (DP + 1 + G) * 64);
  auto kern = kg_mc_block_kernel<DP, G, TR>;
  launch_kernel_ens<kg_mc_block_kernel_body<DP, G, TR>, 512>(kern, dim3(blocks), dim3(waves * 64), shm, s, P, num_lds_tiles);
  MOE_HIP_CHECK(hipGetLastError());
}

// (the wide padded dimensions, 24 and 32, are built for a reduced set: all tiles in LDS, derivative slots {0, 4, 8, 12})
template <int DP, int G>
inline void launch_block_g(const KgMcParams& P, int tr, int num_lds_tiles, int blocks, int waves, hipStream_t s) {
  switch (tr) {
    case 0: return launch_block_inst<DP, G, 0>(P, num_lds_tiles, blocks, waves, s);
    case 2: if constexpr (DP <= 16) return launch_block_inst<DP, G, 2>(P, num_lds_tiles, blocks, waves, s); break;
    case 4: if constexpr (DP <= 16) return launch_block_inst<DP, G, 4>(P, num_lds_tiles, blocks, waves, s); break;
  }
  throw Error(MOE_ERR_RUNTIME, "unsupported register-tile count in the workgroup-per-sample MC kernel");
}

template <int DP>
void launch_block_dp(const KgMcParams& P, int G, int tr, int num_lds_tiles, int blocks, int waves, hipStream_t s) {
  if constexpr (DP > 16) {
    if (tr != 0) throw Error(MOE_ERR_RUNTIME, "d > 16: the workgroup-per-sample MC kernel is built with all tiles in LDS only");
  }
  switch (G) {
    case 0: return launch_block_g<DP, 0>(P, tr, num_lds_tiles, blocks, waves, s);
    case 1: if constexpr (DP <= 16) return launch_block_g<DP, 1>(P, tr, num_lds_tiles, blocks, waves, s); break;
    case 2: if constexpr (DP <= 16) return launch_block_g<DP, 2>(P, tr, num_lds_tiles, blocks, waves, s); break;
    case 3: if constexpr (DP <= 16) return launch_block_g<DP, 3>(P, tr, num_lds_tiles, blocks, waves, s); break;
    case 4: return launch_block_g<DP, 4>(P, tr, num_lds_tiles, blocks, waves, s);
    // more observed derivatives (up to 12: every dimension of C5) run in the next larger slot count, the unused slots
    // carrying zero weights; only this kernel is instantiated for them (the host never sends them to the wave-per-sample one)
    case 8: return launch_block_g<DP, 8>(P, tr, num_lds_tiles, blocks, waves, s);
    case 12: return launch_block_g<DP, 12>(P, tr, num_lds_tiles, blocks, waves, s);
  }
  throw Error(MOE_ERR_RUNTIME, "unsupported derivative-slot count in the MC kernel");
}

}  // namespace mc
}  // namespace moe
