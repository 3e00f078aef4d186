// cornell_moe_amd/csrc/kg_mc_lds.hpp -- the line search with its state in per-wave LDS rows (line_search_lds) and the evaluator of the
// streamed sweeps (WideEval, WeightPtr), shared by three kernel families of the q-KG / d-KG Monte-Carlo phase: the wave-per-sample
// kernel on streamed tables (kg_mc_wave.hpp), the streamed-weights kernel (kg_mc_stream.hpp) and the workgroup-per-sample kernel
// (kg_mc_block.hpp, with its own evaluator BlockEval).  Over the shared core kg_mc.hpp.
#pragma once
#include "kg_mc.hpp"

namespace moe {
namespace mc {

// Armijo trials of the streamed sweeps (line_search_lds, WideEval::kMaxTrials): at most per sweep, in a sample's first sweep, per
// follow-up batch.  (One trial more than the previous step consumed in a step's first sweep: measured slower everywhere -- C5 MC
// 4.22 -> 4.44 ms, d = 16 at n = 1000 0.188 -> 0.197.)
constexpr int kStreamTrials = 8;
constexpr int kStreamFirst = 6;
constexpr int kStreamFollowup = 4;

// The inner optimisation of one MC sample from the start point x (in/out, original dimension order): returns the final objective
// value f = -mu_after(x).  The reference's GradientDescentOptimizerLineSearch::Optimize (gpp_optimization.hpp:1242-1283) around
// GradientDescentOptimizationLineSearch (:708-828) with TensorProductDomain::LimitUpdate (gpp_domain.cpp:64-105), in the original
// units and in TABLE-ROW order (the evaluator works in that order: x is permuted on entry and exit only; free_mask marks the
// optimised coordinates).  Its wave-uniform vectors (x, grad, step, x at restart start, the trial line) are parked in an LDS scratch
// `st` (kLsRows x kMaxDimPadded doubles, private to the wave) between evaluations, for kernels whose registers are better spent on
// point data (workgroup-per-sample variant: the evaluator's __syncthreads is an LDS fence, so nothing is cached across
// passes); uniform LDS reads are broadcasts that do not occupy the VALU.
template <int DP, int G, class EV>
__device__ __forceinline__ double line_search_lds(const KgMcParams& P, EV& ev, double* __restrict__ st, double (&x)[DP],
                                                  unsigned long long& n_val, unsigned long long& n_grad) {
  const double step_tolerance = P.tolerance / (double)P.max_num_steps;
  const int lane_id = (int)(threadIdx.x & 63u);
  const double lo_l = P.bounds[2 * (lane_id < DP ? lane_id : 0)], hi_l = P.bounds[2 * (lane_id < DP ? lane_id : 0) + 1];
  // frame centre and scale of this lane's row (behind the bounds in the blob): the conversions into the frame are done one row
  // per lane and handed over through the wave's LDS scratch -- as wave-uniform arithmetic on KgMcParams' arrays they kept ~50
  // SGPRs live across the whole line search, and the scalar file's spills (v_readlane / v_writelane) were this kernel's most
  // frequent instructions
  const bool free_l = lane_id < DP && ((P.free_mask >> (lane_id & 31)) & 1u);
  const double c_l = P.bounds[2 * kMaxDimPadded + (lane_id < DP ? lane_id : 0)];
  const double s_l = P.bounds[3 * kMaxDimPadded + (lane_id < DP ? lane_id : 0)];
  double* sX = st;
  double* sG = st + kMaxDimPadded;
  double* sS = st + 2 * kMaxDimPadded;
  double* sX0 = st + 3 * kMaxDimPadded;
  double* sF = st + 4 * kMaxDimPadded;  // x0 of the trial line, frame coordinates
  double* sD = st + 5 * kMaxDimPadded;  // its direction dv
  double fcur = 0.0;
  if (P.max_num_restarts <= 0) {
#pragma unroll
    for (int k = 0; k < DP; ++k) x[k] = (k < P.dim) ? 1.0 : 0.0;
    return 0.0;
  }
  double tq[DP], tqp[DP], gp[DP];
  to_table_order<DP, G>(x, P.perm, tq);  // table-row order from here on
#pragma unroll
  for (int k = 0; k < DP; ++k) sX[k] = tq[k];
#pragma unroll
  for (int k = 0; k < DP; ++k) gp[k] = 0.0;
  // Armijo trials the previous step of this sample consumed (>= 2): the size of the next step's first batch.  (A sample's first step:
  // two -- or six where a sweep is bound by the weight stream, the streamed-weights kernel: a bracket there is ~6 trials long.)
  int pred = (EV::kMaxTrials > 5) ? kStreamFirst : 2;
#if MOE_BLOCK_PROF
  ev.seg_last = __builtin_amdgcn_s_memtime();
  ev.seg_tot = ev.c_tot;
#endif
  // A clamped step needs f(x + step) before it is accepted, and -- once accepted -- the next iteration starts with f and grad f at that
  // very point: while another iteration can follow, that evaluation is ONE value + gradient pass carried over (as in
  // line_search_frame: a step costs its Armijo sweeps + one pass instead of + two -- r3: with max_relative_change = 0.1 nearly every
  // step is clamped, so a sample saves five of its ~21 sweeps).  A carried gradient that ends up unused is counted as the value pass it replaced.
  bool have_g = false;
  double f_carried = 0.0, g_carried_l = 0.0;
  for (int restart = 0; restart < P.max_num_restarts; ++restart) {
    if (lane_id < DP) sX0[lane_id] = sX[lane_id];
    for (int istep = 0; istep < P.max_num_steps;) {
      if (lane_id < DP) sF[lane_id] = (sX[lane_id] - c_l) * s_l;  // the iterate in the frame: this pass's query AND the trial line's x0
#if MOE_BLOCK_PROF
      ev.seg_mark(3);  // (3: step end -> this gradient pass, loop control, restart bookkeeping)
#endif
      double g_l;
      double f0;
      if (have_g) {
        f0 = f_carried;
        g_l = g_carried_l;
        have_g = false;
      } else {
        f0 = ev.eval_p_lane(sF, s_l, g_l);
      }
      n_grad++;
      fcur = f0;
      if (lane_id < DP) sG[lane_id] = free_l ? g_l : 0.0;  // fidelity / pad coordinates stay pinned
      double norm = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const double gk = sG[k];
        norm = fma(gk, gk, norm);
      }
      double alpha_n = (P.gamma == 0.0) ? P.pre_mult : P.pre_mult * pow((double)(istep + 1), -P.gamma);
      int search = 0;
      double ftrial;
      // Armijo back-tracking, several trial step sizes per pass (alpha, alpha / 2, alpha / 4, ...: EV::armijo_batch): as many as
      // the previous step of this sample consumed (at least two -- in this kernel a pass is dominated by its fixed cost), then
      // in pairs.  The sequence of decisions is the reference's (gpp_optimization.hpp:752-769): a trial's value is only
      // looked at if all earlier ones failed, and only consumed trials are counted.  A trial that would need clamp_query
      // (millions of length scales away) sends the batch down the two-point path, which clamps.
      {
        // (x0 and dv go to the wave's LDS scratch and are read back inside each pass: as register arrays they stayed live
        //  across the passes of the bracket -- 48 VGPRs of wave-uniform data next to the register tiles -- and the kernel's
        //  scratch-memory spills sat exactly in this code between the passes)
        double dd = 0.0, q0 = 0.0, qa = 0.0;
        if (lane_id < DP) sD[lane_id] = sG[lane_id] * s_l;
#pragma unroll
        for (int r = 0; r < DP; ++r) {
          const double x0r = sF[r];
          const double dvr = sD[r];
          dd = fma(dvr, dvr, dd);
          q0 = fma(x0r, x0r, q0);
          const double xa = fma(alpha_n, dvr, x0r);
          qa = fma(xa, xa, qa);
        }
        // (|x0 + alpha dv|^2 is convex in alpha: the two ends bound every trial of the bracket)
        const bool near = uniform(fmax(q0, qa)) <= kQueryClamp * kQueryClamp;
        int batch = pred;
        bool done = false;
#if MOE_BLOCK_PROF
        ev.seg_mark(0);  // (0: gradient post-processing, norm, trial-line set-up)
#endif
        while (!done) {
          const int want = min(batch, 30 - search);
          if (near && want >= 2) {
            ev.armijo_batch(want, sF, sD, dd, f0, norm, alpha_n, search, ftrial, done, n_val);
          } else {
            const double a1 = alpha_n, a2 = 0.5 * alpha_n;
            double tqb[DP], f1, f2;
#pragma unroll
            for (int r = 0; r < DP; ++r) {
              tqp[r] = to_frame(P, fma(a1, sG[r], sX[r]), r);
              tqb[r] = to_frame(P, fma(a2, sG[r], sX[r]), r);
            }
            ev.eval2(tqp, tqb, f1, f2);
            ftrial = f1;
            n_val++;
            if (f1 - f0 > 0.5 * a1 * norm) break;
            alpha_n = a2;
            if (++search >= 30) break;
            if (want >= 2) {  // (want == 1: the 30th trial -- the second value is not consumed)
              ftrial = f2;
              n_val++;
              if (f2 - f0 > 0.5 * a2 * norm) break;
              alpha_n = 0.5 * a2;
              if (++search >= 30) break;
            }
          }
          // follow-up batches: pairs -- or fours where a sweep is bound by the weight stream, not by its trials (streamed-weights
          // kernel: kMaxTrials > 5), so that a bracket longer than predicted costs one more sweep, not two or three
          batch = (EV::kMaxTrials > 5) ? kStreamFollowup : 2;
        }
        pred = max(2, min(search + 1, EV::kMaxTrials));
#if MOE_BLOCK_PROF
        ev.seg_mark(1);  // (1: the Armijo loop outside its passes: dispatch, decisions)
#endif
      }
      // LimitUpdate with one coordinate per lane (the state already lives in per-wave LDS arrays, so lane k simply reads
      // entry k): one clamp instead of DP wave-uniform copies
      bool changed, nonzero;
      {
        const int lk = lane_id < DP ? lane_id : 0;
        const double want_l = alpha_n * sG[lk];
        double step_l = 0.0;
        if (free_l) step_l = limit_update_1d(lo_l, hi_l, P.max_relative_change, sX[lk], want_l);
        if (P.simplex != 0) {  // (the bounds are the box clipped to the unit hypercube, max_relative_change carries the reference's tweak)
          if (lane_id < DP) sS[lane_id] = step_l;
          __builtin_amdgcn_wave_barrier();
          double relaxed, vnorm;
          if (simplex_limit(P, sX, sS, relaxed, vnorm)) step_l = free_l ? relaxed * (step_l / vnorm) : 0.0;
          __builtin_amdgcn_wave_barrier();
        }
        changed = __ballot(free_l && step_l != want_l) != 0ull;
        nonzero = __ballot(free_l && step_l != 0.0) != 0ull;
        if (lane_id < DP) sS[lane_id] = step_l;  // read back below by every lane of this wave (in-order LDS, same wave)
      }
      if (search == 30 || !nonzero) break;
      double obj2 = ftrial;
      bool carried = false;
      double gn_l = 0.0;
      if (changed) {
        if (lane_id < DP) sF[lane_id] = ((sX[lane_id] + sS[lane_id]) - c_l) * s_l;
        if (istep + 1 < P.max_num_steps || restart + 1 < P.max_num_restarts) {
          obj2 = ev.eval_p_lane(sF, s_l, gn_l);
          carried = true;
        } else {
          obj2 = ev.template eval_p<false>(sF, gp);
          n_val++;
        }
      }
#if MOE_BLOCK_PROF
      ev.seg_mark(2);  // (2: LimitUpdate, clamped re-evaluation set-up)
#endif
      if (obj2 <= f0) {
        if (carried) n_val++;
        break;
      }
      // x += step one row per lane (as a wave-uniform loop the read-modify-writes of sX were twelve dependent LDS round trips:
      // most of the 2.8 k cycles per pass this kernel spent between its passes); |step|^2 from the step row alone, in k order
      if (lane_id < DP) sX[lane_id] = sX[lane_id] + sS[lane_id];
      double ss = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const double sk = sS[k];
        ss = fma(sk, sk, ss);
      }
      fcur = obj2;
      istep += 1;
      have_g = carried;
      f_carried = obj2;
      g_carried_l = gn_l;
      if (sqrt(ss) < step_tolerance) break;
    }
    double ds = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const double dk = sX0[k] - sX[k];
      ds = fma(dk, dk, ds);
    }
    if (!(sqrt(ds) > P.tolerance)) break;
  }
  if (have_g) n_val++;  // carried but never used
#pragma unroll
  for (int k = 0; k < DP; ++k) tq[k] = sX[k];
  from_table_order<DP, G>(tq, P.perm, x);
  return fcur;
}

// Evaluator of the wave-per-sample kernel for the WIDE padded dimensions (d = 17 .. 32), used with line_search_lds.
// At 24 / 32 coordinate rows WaveEval (kg_mc_wave.hpp) needs x2, d2, x0, dv, the current and the prefetched tile -- 6 DP doubles, 384
// VGPRs at DP = 32 -- inside its tile loop and compiled to 2.3 KB of scratch per lane with the spills in the loop (r3: d = 32
// ran 15x slower than d = 16, d = 24 5x).  Here the line-search state lives in the wave's LDS scratch and a pass keeps only what
// its loop needs:
//   value passes (T trials along one line):   x0, dv (2 DP) + a ring of PF rows + T accumulators  -- 80 + T doubles at DP = 32
//   gradient pass:                            xq, grad sums (2 DP) + the tile's rows (DP)          -- 96 doubles at DP = 32; the
//     gradient is accumulated as sum_j coef_j x_j - q sum_j coef_j (the centred frame keeps both terms of the size of the
//     gradient), so a row is dead -- and refilled from the next tile -- right after its fma.
// The table of the wide dimensions holds the rows in PAIRS, [tile][DP / 2][64][2]: a lane fetches rows 2i, 2i + 1 of its point
// with one 16-byte load (8-byte loads run at 0.54 - 0.70x the 16-byte rate out of L2, and these passes are bound by exactly
// that stream: ~200 KB per sweep and wave at n = 1000, d = 24).  The first `ntl` tiles are served from an LDS copy shared by
// the workgroup's waves (whatever the weight slabs leave of the 160 KB), the rest from L2; a sweep is the same loop over the
// two segments (the ring's slot indices are static: PF divides DP).
// Same arithmetic as BlockEval (direct differences about x0); queries beyond kQueryClamp are pulled back (clamp_query).
typedef double d2t __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) d2t* lds_pair_ptr;

// Where a sweep takes the 1 + G weights of a lane's point from: the wave's LDS slab [tile][1 + G][64] (+ lane), or the sample's row of
// the weight table in global memory, [point][1 + G] (+ lane (1 + G)) -- the rows of a point travel as 16-byte pairs when there is an
// even number of them.
template <int G, bool WS>
struct WeightPtr {
  lds_tile_ptr p;
  __device__ __forceinline__ void load(double (&cw)[1 + G]) const {
#pragma unroll
    for (int a = 0; a < 1 + G; ++a) cw[a] = p[a * 64];
  }
  __device__ __forceinline__ void next() { p += (1 + G) * 64; }
};
template <int G>
struct WeightPtr<G, true> {
  const double* __restrict__ p;
  __device__ __forceinline__ void load(double (&cw)[1 + G]) const {
    if constexpr (((1 + G) & 1) == 0) {
      const d2t* q = reinterpret_cast<const d2t*>(p);
#pragma unroll
      for (int a2 = 0; a2 < (1 + G) / 2; ++a2) {
        const d2t v = q[a2];
        cw[2 * a2] = v.x;
        cw[2 * a2 + ((1 + G) > 1 ? 1 : 0)] = v.y;
      }
    } else {
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) cw[a] = p[a];
    }
  }
  __device__ __forceinline__ void next() { p += 64 * (1 + G); }
};

template <int DP, int G, bool WS = false>
struct WideEval {
  const d2t* __restrict__ xg;   // coordinate table of this evaluation in global memory (one tile of padding behind), + lane
  lds_pair_ptr xl;              // LDS copy of its first `ntl` tiles, + lane
  WeightPtr<G, WS> w0;              // this sample's weights, first tile (see WeightPtr)
  const double* __restrict__ etab;
  double* __restrict__ red;         // kPartLen doubles of LDS, private to the wave: packed sums of a gradient pass
  int ntiles, ntl, cov_type, lane;
  double mean;
  // Armijo trials per sweep: with the weights streamed from the table a sweep is bound by that stream (64 KB per sample and sweep at
  // C5), so a step's whole bracket goes into ONE sweep whenever the previous step's bracket predicts up to eight trials.
  // (the L2-streamed sweeps of 16 / 24 rows gain too -- n = 1000: d = 16 0.257 -> 0.230 ms, d = 24 0.306 -> 0.296; at 32 rows the eight
  //  accumulators cost more registers than the saved sweeps give back: 0.403 -> 0.429 -- r3, `profiles/r03_dim_sweep_after.txt`)
  static constexpr int kMaxTrials = (WS || DP <= 24) ? kStreamTrials : 5;
  static constexpr int HP = DP / 2;                        // row pairs per tile
  static constexpr int PF2 = (HP <= 8) ? HP : ((HP % 8 == 0) ? 8 : 6);  // ring depth in row pairs
  static_assert(HP % PF2 == 0 && PF2 <= HP, "ring slots must be static");
#if MOE_BLOCK_PROF
  unsigned long long c_tot = 0, seg_last = 0, seg_tot = 0;
  __device__ __forceinline__ void seg_mark(int) {}
#endif

  // one segment (LDS or L2 tiles) of a T-trial value sweep; `wt` walks on through the weight slab
  template <int COV, int T, class PP>
  __device__ __forceinline__ void segT(PP xt, WeightPtr<G, WS>& wt, int nt, const double (&x0)[DP], const double (&dv)[DP],
                                       const double (&al)[T], double dd, double (&acc)[T]) {
    if (nt <= 0) return;
    d2t ring[PF2];
    double cw[1 + G];
#pragma unroll
    for (int i = 0; i < PF2; ++i) ring[i] = xt[i * 64];
    wt.load(cw);
#pragma unroll 1
    for (int tile = 0; tile < nt; ++tile) {
      double A = 1.0e-300, B = 0.0, sdA = 0.0, sdB = 0.0;
#pragma unroll
      for (int i = 0; i < HP; ++i) {
        const d2t c = ring[i % PF2];
        ring[i % PF2] = xt[(i + PF2) * 64];  // pair i + PF2 of the stream (runs into the next tile; behind the segment: unused)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = 2 * i + h;
          const double d0 = (h == 0 ? c.x : c.y) - x0[k];
          A = fma(d0, d0, A);
          B = fma(d0, dv[k], B);
          if (G > 0 && k < G) {
            sdA = fma(cw[1 + (k < G ? k : 0)], d0, sdA);
            sdB = fma(cw[1 + (k < G ? k : 0)], dv[k], sdB);
          }
        }
      }
      xt += HP * 64;
      wt.next();
      double nw[1 + G];
      wt.load(nw);  // (the last tile's prefetch reads one tile past the sample's weights: padded / the next sample's, unused)
      const double mB2 = -2.0 * B;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const double r2 = fmax(fma(al[t], fma(al[t], dd, mB2), A), 1.0e-300);
        double base, first, second;
        radial3<COV, (G > 0), false>(r2, etab, base, first, second);
        acc[t] = fma(cw[0], base, acc[t]);
        if (G > 0) acc[t] = fma(first, fma(-al[t], sdB, sdA), acc[t]);
      }
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) cw[a] = nw[a];
    }
  }

  template <int T>
  __device__ __forceinline__ void values(const double (&x0)[DP], const double (&dv)[DP], const double (&al)[T], double dd,
                                         double (&f)[T]) {
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    WeightPtr<G, WS> wt = w0;
    if (cov_type == MOE_COV_SQUARE_EXPONENTIAL) {
      segT<MOE_COV_SQUARE_EXPONENTIAL, T>(xl, wt, ntl, x0, dv, al, dd, acc);
      segT<MOE_COV_SQUARE_EXPONENTIAL, T>(xg + (long)ntl * HP * 64, wt, ntiles - ntl, x0, dv, al, dd, acc);
    } else {
      segT<MOE_COV_MATERN_NU_2P5, T>(xl, wt, ntl, x0, dv, al, dd, acc);
      segT<MOE_COV_MATERN_NU_2P5, T>(xg + (long)ntl * HP * 64, wt, ntiles - ntl, x0, dv, al, dd, acc);
    }
    double sum[T];
    constexpr int T4 = T / 4 * 4;
#pragma unroll
    for (int t = 0; t < T4; t += 4) {
      double o[4];
      wave_sum4_uniform(acc[t], acc[t + 1], acc[t + 2], acc[t + 3], o);
      sum[t] = o[0];
      sum[t + 1] = o[1];
      sum[t + 2] = o[2];
      sum[t + 3] = o[3];
    }
    if constexpr (T - T4 >= 2) wave_sum2_uniform(acc[T4], acc[T4 + 1], sum[T4], sum[T4 + 1]);
    if constexpr (((T - T4) & 1) != 0) sum[T - 1] = wave_sum_uniform(acc[T - 1]);
#pragma unroll
    for (int t = 0; t < T; ++t) f[t] = -(mean + sum[t]);
  }

  // up to kMaxTrials Armijo trials x0 + alpha 2^-t dv in one pass and the reference's decisions over them (see BlockEval::armijo_t)
  template <int T>
  __device__ __forceinline__ void armijo_t(const double* __restrict__ x0p, const double* __restrict__ dvp, double dd, double f0,
                                           double norm, double& alpha_n, int& search, double& ftrial, bool& done,
                                           unsigned long long& n_val) {
    double x0[DP], dv[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      x0[k] = x0p[k];
      dv[k] = dvp[k];
    }
    double al[T], f[T];
#pragma unroll
    for (int t = 0; t < T; ++t) al[t] = (t == 0) ? alpha_n : 0.5 * al[t > 0 ? t - 1 : 0];
    values<T>(x0, dv, al, dd, f);
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
      case 5: armijo_t<5>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
      default:
        if constexpr (kMaxTrials > 5) {
          switch (want) {
            case 6: armijo_t<6>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
            case 7: armijo_t<7>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
            default: armijo_t<8>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val); break;
          }
        } else {
          armijo_t<5>(x0, dv, dd, f0, norm, alpha_n, search, ftrial, done, n_val);
        }
        break;
    }
  }

  // f at one point: a one-trial sweep along the zero direction
  __device__ __forceinline__ double value_at(const double (&xq_in)[DP]) {
    double xq[DP], dv[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      xq[k] = xq_in[k];
      dv[k] = 0.0;
    }
    clamp_query<DP>(xq);
    const double al[1] = {0.0};
    double f[1];
    values<1>(xq, dv, al, 0.0, f);
    return f[0];
  }
  __device__ __forceinline__ void eval2(const double (&xa)[DP], const double (&xb)[DP], double& fa, double& fb) {
    fa = value_at(xa);
    fb = value_at(xb);
  }
  template <bool WG>
  __device__ __forceinline__ double eval_p(const double* __restrict__ xq_ptr, double (&)[DP]) {
    static_assert(!WG, "gradient passes of the wide evaluator go through eval_p_lane");
    double xq[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xq[k] = xq_ptr[k];
    return value_at(xq);
  }

  // one segment of a gradient sweep
  template <int COV, class PP>
  __device__ __forceinline__ void segG(PP xt, WeightPtr<G, WS>& wt, int nt, const double (&xq)[DP], double& accf, double& accs,
                                       double (&accg)[DP], double (&accd)[G > 0 ? G : 1]) {
    if (nt <= 0) return;
    d2t cx[HP];
    double cw[1 + G];
#pragma unroll
    for (int i = 0; i < HP; ++i) cx[i] = xt[i * 64];
    wt.load(cw);
#pragma unroll 1
    for (int tile = 0; tile < nt; ++tile) {
      double r2 = 1.0e-300, sd = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const double d0 = ((k & 1) ? cx[k / 2].y : cx[k / 2].x) - xq[k];
        r2 = fma(d0, d0, r2);
        if (G > 0 && k < G) sd = fma(cw[1 + (k < G ? k : 0)], d0, sd);
      }
      double base, first, second;
      radial3<COV, true, (G > 0)>(r2, etab, base, first, second);
      const double w0 = cw[0];
      accf = fma(w0, base, accf);
      double coef = w0 * first;
      if (G > 0) {
        accf = fma(first, sd, accf);
        coef = fma(second, sd, coef);
#pragma unroll
        for (int a = 0; a < G; ++a) accd[a] = fma(first, cw[1 + a], accd[a]);
      }
      accs += coef;
      xt += HP * 64;
      wt.next();
#pragma unroll
      for (int i = 0; i < HP; ++i) {
        accg[2 * i] = fma(coef, cx[i].x, accg[2 * i]);
        accg[2 * i + 1] = fma(coef, cx[i].y, accg[2 * i + 1]);
        cx[i] = xt[i * 64];  // the pair's slot is free: the next tile's rows (behind the segment: unused)
      }
      wt.load(cw);
    }
  }

  // value + gradient, the gradient handed back one component per lane in the original units (scale_l = this lane's frame scale)
  __device__ __forceinline__ double eval_p_lane(const double* __restrict__ xq_ptr, double scale_l, double& grad_l) {
    constexpr int NS = 2 + DP + (G > 0 ? G : 0);
    static_assert(NS <= kPartLen, "packed sums of a gradient pass exceed the wave's scratch");
    double xq[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xq[k] = xq_ptr[k];
    clamp_query<DP>(xq);
    double q_l = 0.0;  // this lane's (clamped) query coordinate
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (lane == k) q_l = xq[k];
    double accf = 0.0, accs = 0.0, accg[DP], accd[G > 0 ? G : 1];
#pragma unroll
    for (int k = 0; k < DP; ++k) accg[k] = 0.0;
#pragma unroll
    for (int a = 0; a < (G > 0 ? G : 1); ++a) accd[a] = 0.0;
    WeightPtr<G, WS> wt = w0;
    if (cov_type == MOE_COV_SQUARE_EXPONENTIAL) {
      segG<MOE_COV_SQUARE_EXPONENTIAL>(xl, wt, ntl, xq, accf, accs, accg, accd);
      segG<MOE_COV_SQUARE_EXPONENTIAL>(xg + (long)ntl * HP * 64, wt, ntiles - ntl, xq, accf, accs, accg, accd);
    } else {
      segG<MOE_COV_MATERN_NU_2P5>(xl, wt, ntl, xq, accf, accs, accg, accd);
      segG<MOE_COV_MATERN_NU_2P5>(xg + (long)ntl * HP * 64, wt, ntiles - ntl, xq, accf, accs, accg, accd);
    }
    double sums[NS];
    sums[0] = accf;
#pragma unroll
    for (int k = 0; k < DP; ++k) sums[1 + k] = accg[k];
    sums[1 + DP] = accs;
    if (G > 0) {
#pragma unroll
      for (int a = 0; a < G; ++a) sums[2 + DP + a] = accd[a];
    }
    wave_sum_packed_store<NS>(sums, red, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    volatile __attribute__((address_space(3))) double* R = (volatile __attribute__((address_space(3))) double*)red;
    const double f = R[0];
    const double ss = R[1 + DP];
    double v = R[1 + (lane < DP ? lane : 0)];
    v = fma(-q_l, ss, v);  // sum coef x_k - q_k sum coef
    if (G > 0) {
      const double vd = R[2 + DP + (lane < G ? lane : 0)];
      if (lane < G) v -= vd;
    }
    grad_l = -(v * scale_l);
    __builtin_amdgcn_wave_barrier();  // (the next pass's sums overwrite the slot only after every lane has read it: in-order LDS)
    return -(mean + uniform(f));
  }
};

}  // namespace mc
}  // namespace moe
