// cornell_moe_amd/csrc/kg_mc.hpp -- the shared core of the q-KG / d-KG Monte-Carlo inner-optimisation kernels (gfx950): the
// parameter block, the LDS layout constants, the launcher declarations, the wave reductions, the tile-loop evaluators and the pieces
// of a sample every family uses.  One header per kernel family sits on top of it -- kg_mc_wave.hpp (wave-per-sample), kg_mc_lane.hpp
// (its lane-parked form), kg_mc_stream.hpp (streamed weights), kg_mc_block.hpp (workgroup-per-sample), and kg_mc_lds.hpp (the
// LDS-state line search three of them share) -- instantiated by the per-dimension translation units kg_mc_dp*.hip (compiled in
// parallel).  kg.hip, kg_prep.hip and kg_tail.hip include this header only.
//
// What the reference does per MC sample i (gpp_knowledge_gradient_optimization.cpp:170-196): draw z_i, set the fantasy
// observations y_i = mu(Xu) + L z_i, RE-SOLVE K_after^-1 (y - mean) with two O((N+m)^2) triangular sweeps
// (gpp_math.cpp:531-551), then maximise -mu_after,i(x) from the best discretised start with a back-tracking
// line-search gradient descent (.cpp:420-472, gpp_optimization.hpp:708-828).
//
// What this kernel does instead -- same mathematics, no N^2 work per sample:
//   K_after^-1 (y_i - mean) = [ K^-1(y - mean) - W beta_i ; beta_i ],   W = K^-1 K*(X,Xu),  beta_i = L^-T z_i,
// (block elimination of the (N+m) system; the reference's own gradient tail relies on the same identity, .cpp:199-209),
// so  mu_after,i(x) = mean + sum over the n + u points p of  [ w_p0 base(x,p) + first(x,p) sum_a w_pa (p - x)_{d_a} ]
// with a per-sample weight block w (1 + g values per point: the function-value weight and one weight per observed
// partial derivative) that costs N*m flops to form.
//
// Mapping (wave-per-sample kernels): ONE WAVEFRONT owns one MC sample at a time and pulls the next sample of its evaluation from an atomic
// counter when it finishes (persistent waves: no workgroup-level tail while a slow line search finishes).  Lanes stride
// over the n + u points; point coordinates are staged once per workgroup in LDS, tile-major [tile][dim][64 lanes] so that
// every ds_read_b64 is conflict free and its address is base + immediate; the wave's weights live in its own LDS slab with
// the same tiling; each posterior-mean (or mean + gradient) evaluation ends in a 64-lane butterfly reduction.  Control
// flow of the line search is wave-uniform: there is no intra-wave divergence.
#pragma once
#include <hip/hip_runtime.h>

#include "fastmath.hpp"
#include "kernels.hpp"

namespace moe {

// Phase timing of the workgroup-per-sample kernel (s_memtime cycles summed over samples by wave 0 into counters[...]):
// build with -DMOE_BLOCK_PROF=1 (tools only; off in the product build).
#ifndef MOE_BLOCK_PROF
#define MOE_BLOCK_PROF 0
#endif
#if MOE_BLOCK_PROF
#define MOE_PROF_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define MOE_PROF_ADD(dst, a, b) dst += (b) - (a)
#else
#define MOE_PROF_T(var)
#define MOE_PROF_ADD(dst, a, b)
#endif
constexpr int kTicketStride = 32;  // unsigned ints between the sample-ticket counters of consecutive evaluations (128 B)
constexpr int kMaxM = 64;   // m = (q + p)(1 + g) limit of the wave-per-sample kernel and of every "one lane per component" routine
constexpr int kMaxMB = 128;  // limit of the workgroup-per-sample kernel (r2: q = 8 with all 12 derivatives of C5 observed is
                             // m = 104): beta of the current sample lives at zb[kMaxMB ...), filled from the sample pre-pass
constexpr int kExpTabLen = 64;  // 2^(j/64) table at the start of the MC kernel's LDS (fastmath.hpp exp_nonpos_tab)

struct KgRec {  // offsets (doubles) of one evaluation's small operands inside the blob; identical for every evaluation
  int L;        // [m x m] col-major lower Cholesky factor of Var(Xu) + noise
  int mu_disc;  // [A]      mu_n at the discretised points
  int C_disc;   // [A][m]   L^-1 cov_n(Xu, x_j)
  int disc;     // [A][size] discretised points (unscaled, fidelity dims dropped)
  int XuP;      // [u][dp]  union points, padded (unscaled)
  int Mk;       // unused by the MC kernel
  int stride;   // record length
};

struct KgMcParams {
  int cov_type, dim;
  double alpha;
  double center[kMaxDimPadded];  // training-set mean of table row r's coordinate: the tables and the queries are centred on it
                                 // BEFORE scaling ((x - c) / l is exact to rounding wherever the domain sits)
  double inv_lp[kMaxDimPadded];  // frame scale of table row r (row r holds original dimension perm[r]): 1 / length for the squared
                                 // exponential, sqrt(5) / length for Matern-5/2 (radial3 then needs no sqrt(5)); 0 in pad rows
  int perm[kMaxDimPadded];       // the GP's observed-derivative dimensions come first: perm[a] = derivatives[a], a < g
  int inv_perm[kMaxDimPadded];   // table row of original dimension j (the simplex update walks the coordinates in the reference's order)
  int simplex;                   // inner domain: 0 = tensor product, 1 = its intersection with the unit simplex (line_search_lds only:
                                 // kg_launch keeps such evaluations off the LDS-slab wave-per-sample kernel)
  double inv_sqrt_size;          // 1 / sqrt(dim - f): the components of the diagonal face's unit normal
  int n, g, N, u, m, f, A, ntiles, E;
  int multi_trial;  // 0: one Armijo trial per pass only (point sets spanning > 100 length scales: the projected distances of the
                    // multi-trial passes lose absolute accuracy with the square of the trial's offset)
  double mean;
  const double* XsTab;  // [E][ntiles][DP][64] scaled coordinates of X then Xu_e, zero padded
                        // (pair_rows: rows in pairs, [E][ntiles][DP / 2][64][2] -- WideEval: the streamed wave-per-sample kernel and d > 16)
  int wide_lds_tiles;   // streamed wave-per-sample kernel: leading tiles of the table copied to LDS per workgroup
  long tab_stride;
  const double* KinvY;  // [N], entry (j, a) at j (1 + g) + a
  const double* W;      // K^-1 K*: evaluation e at W + e * w_stride, [N x m], ld N
  long w_stride;
  const double* blob;
  KgRec rec;
  const double* bounds;   // [2 kMaxDimPadded] domain bounds in TABLE-ROW order (row r = original dimension perm[r])
  unsigned int free_mask; // bit r set: table row r is an optimised coordinate (a real, non-fidelity dimension)
  const double* normals;  // [ceil(M/2)][m]
  int first_sample, num_local;
  int max_num_steps, max_num_restarts;
  double gamma, pre_mult, max_relative_change, tolerance;
  double* best_point;  // [E][num_local][DP] (unscaled, fidelity coords = 1, pads = 0)
  double* best_value;  // [E][num_local]
  double* beta;        // [E][num_local][m]
  unsigned long long* counters;  // [E][2]: value passes, value + gradient passes
  unsigned int* next_sample;     // [E] work counters (zeroed before launch)
  unsigned long long* prof;      // 16 spare words behind the counters (MOE_BLOCK_PROF builds)
  const double* V;               // [E][num_local][v_stride] per-sample weights alpha-scaled (kg_sample_weights_kernel, kg_prep.hip), or NULL
  long v_stride;                 // N (workgroup-per-sample kernel) or ntiles * 64 * v_slots1: the fantasy points' weights and the zero
                                 // padding included (streamed-weights kernel, kg_mc_stream_kernel)
  int v_slots1;                  // weights per point in the table: 1 + g, or 1 + G of the streamed-weights instantiation when it has
                                 // more derivative slots than the GP observes (g = 5 .. 7 -> 8, 9 .. 11 -> 12: the extra slots hold 0)
  const int* best_j;             // [E][num_local] start point of every sample's line search, precomputed with beta by
                                 // kg_sample_prep_kernel (kg_prep.hip); NULL = each sample computes them itself
  const double* start_tab;       // [E][A][1 + m][DP + 1] the start table (kg_start_table_kernel, kg_prep.hip; mc::start_from_table), or NULL:
  long start_stride;             // f and grad f at the discretised points as (1 + m)-term dot products with [1 ; beta]
  int steal_min;                 // a workgroup out of tickets moves to the evaluation with the most tickets left while that has at
                                 // least this many (mc::next_evaluation); 0: it exits, the static assignment (MOE_KG_STEAL=0)
  int steal_skew;                // test switch (MOE_KG_STEAL_SKEW=1): every workgroup starts on evaluation 0
};
constexpr int kMovesWord = 15;  // word of KgMcParams::prof that counts the moves of a call (product builds: the words are otherwise unused)

#if defined(__HIPCC__)
namespace mc {

// Launchers, one per kernel family and padded dimension: defined in the family's header and explicitly instantiated in the unit
// kg_mc_dp*.hip that owns the dimension.  `waves` = wavefronts per workgroup, `shm` = dynamic LDS bytes.
// Padded dimensions 24 and 32 (d = 17 .. 32) are built for a reduced set: derivative slots {0, 4} (wave-per-sample kernel,
// coordinates streamed from L2 only), {0, 4, 8, 12} with all tiles in LDS (workgroup-per-sample kernel) and {0, 4, 8, 12}
// (streamed-weights kernel).
// Wave-per-sample kernel (kg_mc_wave.hpp: kg_mc_kernel).
template <int DP> void launch_dp(const KgMcParams& P, int G, bool xlds, int blocks, int waves, size_t shm, hipStream_t s);
// Lane-parked wave-per-sample kernel (r5, kg_mc_lane.hpp): the LDS-table kernel above with the line search's vectors one row per lane and
// the evaluation's record head ([L | mu_disc | C_disc | disc]: `rec_head` doubles) in LDS; 8 wavefronts, padded dimension <= 16.
template <int DP> void launch_lane_dp(const KgMcParams& P, int G, int rec_head, int blocks, int waves, size_t shm, hipStream_t s);
// Streamed-weights wave-per-sample kernel (kg_mc_stream.hpp: kg_mc_stream_kernel): weights from the table P.V, P.wide_lds_tiles tiles
// of coordinates in LDS.
template <int DP> void launch_stream_dp(const KgMcParams& P, int G, int blocks, int waves, size_t shm, hipStream_t s);
// Workgroup-per-sample variant (kg_mc_block.hpp: kg_mc_block_kernel): the first `num_lds_tiles` tiles of 64 points in LDS, `tr` (0, 2
// or 4) register tiles per wavefront for the rest; bytes of dynamic LDS = kg_mc_block_lds_bytes(...).
template <int DP> void launch_block_dp(const KgMcParams& P, int G, int tr, int num_lds_tiles, int blocks, int waves, hipStream_t s);

// One DPP data movement of a double (two 32-bit v_mov_b32 dpp).  FULL = every lane has a valid source (the in-row
// permutations): the destination's previous contents are irrelevant, so the source itself is passed as `old` and no
// zero-fill is emitted.  Otherwise lanes masked off by ROW_MASK read 0.
template <int CTRL, int ROW_MASK, bool FULL>
__device__ __forceinline__ double dpp_move(double v) {
  const int slo = __double2loint(v), shi = __double2hiint(v);
  int lo, hi;
  if (FULL) {  // every destination lane is written: no `old` operand, hence no copy to set it up
    lo = __builtin_amdgcn_mov_dpp(slo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_mov_dpp(shi, CTRL, ROW_MASK, 0xf, false);
  } else {
    lo = __builtin_amdgcn_update_dpp(0, slo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, shi, CTRL, ROW_MASK, 0xf, false);
  }
  return __hiloint2double(hi, lo);
}

// Sum over the 64 lanes, returned wave-uniform (in SGPRs).  All-VALU: four in-row DPP steps (quad xor 1, quad xor 2,
// half-row mirror, row mirror), row_bcast15 into rows 1 and 3, row_bcast31 into rows 2 and 3, then v_readlane of lane 63.
// ~20 instructions with ALU latencies, instead of six dependent ds_bpermute round trips (~100 cycles each) per sum.
// The summation tree is fixed, so results are deterministic.  Requires all 64 lanes active.
__device__ __forceinline__ double wave_sum_uniform(double v) {
  v += dpp_move<0xB1, 0xf, true>(v);    // quad_perm [1,0,3,2]
  v += dpp_move<0x4E, 0xf, true>(v);    // quad_perm [2,3,0,1]
  v += dpp_move<0x141, 0xf, true>(v);   // row_half_mirror
  v += dpp_move<0x140, 0xf, true>(v);   // row_mirror
  v += dpp_move<0x142, 0xa, false>(v);  // row_bcast15 -> rows 1, 3
  v += dpp_move<0x143, 0xc, false>(v);  // row_bcast31 -> rows 2, 3
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

// ---- packed wave reductions (gradient passes) ----
// v_permlane32_swap / v_permlane16_swap (gfx950) exchange half-waves / 16-lane rows between TWO registers in one VALU
// instruction, so two per-lane partial sums can be folded into one register with 3 instructions (2 word swaps + 1 add): the
// lower / even part keeps summing value a, the upper / odd part value b.  Eight sums then cost 12 + 6 folding instructions and
// TWO in-row DPP reductions instead of eight full ones (58 instead of 176 VALU instructions with the read-outs).
__device__ __forceinline__ double fold32(double a, double b) {  // lanes 0-31: a.lo + a.hi, lanes 32-63: b.lo + b.hi
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ double fold16(double a, double b) {  // rows: a.r0 + a.r1 | b.r0 + b.r1 | a.r2 + a.r3 | b.r2 + b.r3
  const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);
  return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ double row_sum(double v) {  // every lane: the sum over its 16-lane row (fixed tree)
  v += dpp_move<0xB1, 0xf, true>(v);    // quad_perm [1,0,3,2]
  v += dpp_move<0x4E, 0xf, true>(v);    // quad_perm [2,3,0,1]
  v += dpp_move<0x141, 0xf, true>(v);   // row_half_mirror
  v += dpp_move<0x140, 0xf, true>(v);   // row_mirror
  return v;
}
__device__ __forceinline__ double lane_value(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
// out[i] = sum over the 64 lanes of v[i], wave-uniform, for four / eight values at a time
__device__ __forceinline__ void wave_sum4_uniform(double v0, double v1, double v2, double v3, double (&out)[4]) {
  const double q = row_sum(fold16(fold32(v0, v1), fold32(v2, v3)));  // rows hold v0 | v2 | v1 | v3
  out[0] = lane_value(q, 0);
  out[2] = lane_value(q, 16);
  out[1] = lane_value(q, 32);
  out[3] = lane_value(q, 48);
}
__device__ __forceinline__ void wave_sum2_uniform(double a, double b, double& sa, double& sb) {
  const double p = fold32(a, b);
  const double q = row_sum(fold16(p, p));
  sa = lane_value(q, 0);
  sb = lane_value(q, 32);
}
// The same with the results handed back through per-wave LDS scratch (N doubles at `scr`) as broadcast reads, i.e. wave-uniform
// values in VGPRs: read out with v_readlane they land in SGPRs, and in the MC kernel -- whose scalar register file is full --
// every one of them was spilled to a VGPR lane (v_writelane) and fetched back (v_readlane), two VALU slots each way.
template <int N>
__device__ __forceinline__ void wave_sum_packed_lds(const double (&v)[N], double* __restrict__ scr, int lane, double (&out)[N]) {
  static_assert(N % 4 == 0, "packed reductions work on multiples of four values");
  volatile __attribute__((address_space(3))) double* S = (volatile __attribute__((address_space(3))) double*)scr;
  const int row = lane >> 4;
  const int slot = ((row & 1) << 1) | (row >> 1);  // rows hold v0 | v2 | v1 | v3
#pragma unroll
  for (int i = 0; i < N; i += 4) {
    const double q = row_sum(fold16(fold32(v[i], v[i + 1]), fold32(v[i + 2], v[i + 3])));
    if ((lane & 15) == 0) S[i + slot] = q;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) out[i] = S[i];  // (LDS operations of one wave complete in order)
}

template <int N>
__device__ __forceinline__ void wave_sum_packed(const double (&v)[N], double (&out)[N]) {
  static_assert(N % 4 == 0, "packed reductions work on multiples of four values");
#pragma unroll
  for (int i = 0; i < N; i += 4) {
    double o[4];
    wave_sum4_uniform(v[i], v[i + 1], v[i + 2], v[i + 3], o);
    out[i] = o[0];
    out[i + 1] = o[1];
    out[i + 2] = o[2];
    out[i + 3] = o[3];
  }
}

// dst[i] = sum over the 64 lanes of v[i], i < N (N padded to a multiple of four with zeros): the packed folds above, the four row
// sums of a group written straight to memory by the first lane of each row -- for callers that only need the sums in LDS (the
// workgroup-per-sample kernel's per-wave partial slots: 16 sums cost 4 folds + 4 in-row reductions instead of 16 full ones).
template <int N>
__device__ __forceinline__ void wave_sum_packed_store(const double (&v)[N], double* __restrict__ dst, int lane) {
  constexpr int NP = (N + 3) / 4 * 4;
  const int row = lane >> 4;
  const int slot = ((row & 1) << 1) | (row >> 1);  // rows hold v0 | v2 | v1 | v3
#pragma unroll
  for (int i = 0; i < NP; i += 4) {
    const double a = v[i], b = (i + 1 < N) ? v[i + 1 < N ? i + 1 : 0] : 0.0, c = (i + 2 < N) ? v[i + 2 < N ? i + 2 : 0] : 0.0,
                 d = (i + 3 < N) ? v[i + 3 < N ? i + 3 : 0] : 0.0;
    const double q = row_sum(fold16(fold32(a, b), fold32(c, d)));
    if ((lane & 15) == 0 && i + slot < N) dst[i + slot] = q;
  }
}

__device__ __forceinline__ double uniform(double v) {
  // all lanes hold the same bits after a butterfly; tell the compiler so (value moves to SGPRs, branches become scalar)
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// The first gradient of a sample's line search from the evaluation's START TABLE (kg_start_table_kernel, kg_prep.hip).  A line search
// starts at a discretised point x_c, and mu_after,i(x) = mu_n(x) + cov_n(Xu, x)^T beta_i is linear in the sample's beta: f = -mu_after
// and its frame gradient at x_c are (1 + m)-term dot products whose coefficients depend on the evaluation alone.  `row` = the table
// row of x_c, [1 + m][DP + 1] doubles: column 0 the mu_n part, column 1 + l the coefficient of beta_l; entry k < DP the frame gradient's
// row k, entry DP the value -- signs and alpha folded so that the sums ARE what a value + gradient pass at x_c returns.  `beta` = the
// wave's copy of beta (0 beyond m).  Lane k <= DP returns entry k (lanes beyond DP repeat entry DP): ascending l, one fma each --
// the one operation order of every kernel that takes the table (lane-parked and frame line search: same bits).
template <int DP>
__device__ __forceinline__ double start_from_table(const double* __restrict__ row,
                                                   const volatile __attribute__((address_space(3))) double* beta, int m, int lane) {
  constexpr int RS = DP + 1;
  const double* p = row + min(lane, DP);
  double v = p[0];
  for (int c0 = 0; c0 < m; c0 += 4) {  // four columns requested together (column index clamped to m - 1; beta is 0 beyond m)
    const double t0 = p[(1 + c0) * RS];
    const double t1 = p[(1 + min(c0 + 1, m - 1)) * RS];
    const double t2 = p[(1 + min(c0 + 2, m - 1)) * RS];
    const double t3 = p[(1 + min(c0 + 3, m - 1)) * RS];
    v = fma(t0, beta[c0], v);
    v = fma(t1, beta[min(c0 + 1, kMaxM - 1)], v);
    v = fma(t2, beta[min(c0 + 2, kMaxM - 1)], v);
    v = fma(t3, beta[min(c0 + 3, kMaxM - 1)], v);
  }
  return v;
}

// A coordinate in the frame of the tables: centred, then scaled.
__device__ __forceinline__ double to_frame(const KgMcParams& P, double v, int r) { return (v - P.center[r]) * P.inv_lp[r]; }

// Armijo trial points are not limited to the domain and, with small length scales (step ~ gradient ~ 1 / length), land
// millions of length scales away, where sqrt(5 r2) * 64 / ln2 leaves the 32-bit exponent arithmetic of exp_nonpos_tab.
// Every tabulated point lies within kTableExtent = 1e5 length scales of the centre per coordinate (validated on the host),
// so a query beyond kFarRadius from the centre has covariance exactly 0 with all of them: the wave-per-sample kernel skips
// such a pass (eval_loop), the workgroup-per-sample kernel pulls the query back to kQueryClamp per coordinate (same zeros).
// One wave-uniform test per pass either way.
constexpr double kTableExtent = 1.0e5;
constexpr double kFarRadius = 5.657e5 + 400.0;  // sqrt(kMaxDimPadded = 32) * kTableExtent + 400
constexpr double kQueryClamp = 1.0e6;
template <int DP>
__device__ __forceinline__ void clamp_query(double (&xq)[DP]) {
  double qq = 0.0;
#pragma unroll
  for (int k = 0; k < DP; ++k) qq = fma(xq[k], xq[k], qq);
  if (!(uniform(qq) <= kQueryClamp * kQueryClamp)) {
#pragma unroll
    for (int k = 0; k < DP; ++k) xq[k] = fmin(fmax(xq[k], -kQueryClamp), kQueryClamp);
  }
}

// Radial scalars divided by alpha (alpha is folded into the weights): base = cov[0,0], first = first-derivative
// coefficient, second = Hessian-product coefficient (device_cov.hpp), all in the FRAME of the tables.  For the Matern kernel
// the frame's scale is sqrt(5) / length (KgMcParams::inv_lp carries the sqrt(5)), so r2 here is 5 r^2 and a = sqrt(r2) needs
// no multiplication; with differences that are sqrt(5) times larger the derivative coefficients shrink by 5 and 25:
//   d base / d q'_k = (1/3) e^-a (1 + a) (x'_k - q'_k),   d first / d (x' - q')_k = -(1/3) e^-a (x' - q')_k.
// In two halves (fastmath.hpp: exp_nonpos_tab_head / _finish).  Head: the distance -> exp argument chain and the table read, through
// `etab` as the caller types it -- a volatile LDS pointer (lds_tile_ptr) in the lookup-first tile loops, whose reads then keep their
// program order among the tile reads.  Finish: the polynomial, the scaling and the covariance factors.  radial3 is the composition.
struct RadialHead {
  double T, a, r;  // the table entry | sqrt(r2) (Matern) | the reduced exp argument
  int k;
};
template <int COV, class TabPtr>
__device__ __forceinline__ RadialHead radial3_head(double r2, TabPtr etab) {
  // r2 >= 1e-300 by construction (the distance accumulation starts from 1e-300, see eval_loop)
  RadialHead h;
  if (COV == MOE_COV_SQUARE_EXPONENTIAL) {
    h.a = 0.0;
    h.T = etab[exp_nonpos_tab_head(fmax(-0.5 * r2, -1000.0), h.r, h.k)];  // (r2 can reach 1e13 here: keep the table exp in range)
  } else {
    h.a = sqrt_pos_fast(r2);  // (seed + one Heron step: <= 36 ulp, two instructions less per covariance entry)
    h.T = etab[exp_nonpos_tab_head(-h.a, h.r, h.k)];
  }
  return h;
}
template <int COV, bool NEED_FIRST, bool NEED_SECOND>
__device__ __forceinline__ void radial3_finish(const RadialHead& h, double& base, double& first, double& second) {
  const double e = exp_nonpos_tab_finish(h.T, h.r, h.k);
  if (COV == MOE_COV_SQUARE_EXPONENTIAL) {
    base = e;
    first = base;
    second = base;
  } else {
    const double a = h.a;
    base = e * fma(a, fma(a, 1.0 / 3.0, 1.0), 1.0);  // e^-a (1 + a + a^2/3)
    first = NEED_FIRST ? (1.0 / 3.0) * (e * (a + 1.0)) : 0.0;
    second = NEED_SECOND ? (1.0 / 3.0) * e : 0.0;
  }
}
template <int COV, bool NEED_FIRST, bool NEED_SECOND>
__device__ __forceinline__ void radial3(double r2, const double* __restrict__ etab, double& base, double& first,
                                        double& second) {
  radial3_finish<COV, NEED_FIRST, NEED_SECOND>(radial3_head<COV>(r2, etab), base, first, second);
}

// One pass over the n + u points for the wave's sample: returns f = -mu_after(x) and (if WG) grad f in table-row order.
// xq = scaled query coordinates in table-row order (wave-uniform).  xs = coordinate table [tile][DP][64] (LDS, or global
// when it does not fit), aw = this wave's weights [tile][1+G][64] in LDS (zero beyond the real points, so padded lanes
// contribute exactly 0).
// Tile loads from LDS are volatile loads through an explicit LDS pointer: they must stay single ds_read_b64.  Merged into
// ds_read2st64_b64 (what the load/store optimiser makes of two loads 512 B apart) they run at half the LDS rate on gfx950
// -- 126 vs 218 B/clk/CU measured (tools/ldsbench.hip) -- and the tile loop moves 4.6 KB per tile and wavefront.
typedef const volatile __attribute__((address_space(3))) double* lds_tile_ptr;
template <bool LDS>
struct tile_ptr {
  typedef const double* type;
};
template <>
struct tile_ptr<true> {
  typedef lds_tile_ptr type;
};

//
// With the table in LDS (XL) every tile carries one more row, |x_j - c|^2 of the centred scaled coordinates, and the value
// passes -- nine in ten of all passes -- get the squared distance as |x_j|^2 + |q|^2 - 2 x_j . q: DP FMAs, one add and one
// max per point instead of DP subtractions + DP FMAs (6 of 43 VALU instructions per point at DP = 8).  The coordinates
// and the queries are centred on the training-set mean before they are scaled (KgMcParams::center) so that the three terms
// are of the size of the distance itself wherever the domain sits: the rounding error of r2 stays within a small multiple of the direct form's
// (absolute ~1e-15 at unit-box scales; the kernel is smooth at r = 0, so close pairs lose nothing).  Gradient passes keep
// the direct differences (they need them anyway).
// A value pass (!WG) takes q2 = -2 x in `xq_in` (what the dot-product distances multiply the table rows with), so a trial point
// costs DP fmas to set up instead of DP frame conversions + DP scalings.  A gradient pass (WG) takes the frame point x itself and
// returns the gradient with respect to the FRAME coordinates (not multiplied by the frame scale).
template <int DP, int G, bool WG, int COV, bool SMALL, bool XL, bool LF = false>
__device__ __forceinline__ double eval_loop(const double* __restrict__ xs, const double* __restrict__ aw,
                                            const double* __restrict__ etab, int ntiles, double mean,
                                            const double (&xq_in)[DP], double (&grad)[DP], int lane,
                                            double* __restrict__ scr = nullptr) {
  // (gradient passes keep the direct differences: in dot-product form, grad = sum_j coef_j x_j - q sum_j coef_j, the gradient carries
  //  the cancellation of the two terms, and where the inner optimiser runs to convergence -- 100 steps x 10 restarts, the reference's
  //  own ping-test settings -- the end points drift to 1.4e-6 from the reference's instead of 1e-7)
  constexpr bool DOT = XL && !WG;  // squared distance from the |x|^2 row
  constexpr bool LFX = LF && XL;  // lookup-first order of the tile loop (LDS table only; the caller asks for it: kg_mc_lane.hpp)
  constexpr int XR = DP + (XL ? 1 : 0);  // rows per coordinate tile
  double q2[DP], xq[DP];
  double qq;
  if (!WG) {
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      q2[k] = xq_in[k];
      ss = fma(q2[k], q2[k], ss);
      if (!DOT || G > 0) xq[k] = -0.5 * q2[k];
    }
    qq = fma(ss, 0.25, 1.0e-300);
  } else {
    // (a gradient pass reads neither qq nor q2; they stay because taking them out moves two instructions of kg_mc_kernel<DP, 0, true, true>)
    qq = 1.0e-300;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      xq[k] = xq_in[k];
      qq = fma(xq[k], xq[k], qq);
      q2[k] = -2.0 * xq[k];
    }
  }
  // A trial point more than kFarRadius length scales from the centre is > 400 length scales from every tabulated point
  // (all inside the ball of radius sqrt(32) * kTableExtent): every covariance underflows to exactly 0 and the posterior mean
  // IS the prior mean -- the pass is skipped.  Closer than that, sqrt(r2) * 64 / ln2 < 2^31: exp_nonpos_tab is in range.
  if (!WG && !(uniform(qq) <= kFarRadius * kFarRadius)) return -mean;  // (uniform: a scalar branch, and the callers' Armijo decisions stay scalar)
  double accf = 0.0;
  double accg[DP];
  double accd[G > 0 ? G : 1];
#pragma unroll
  for (int k = 0; k < DP; ++k) accg[k] = 0.0;
#pragma unroll
  for (int a = 0; a < (G > 0 ? G : 1); ++a) accd[a] = 0.0;
  // Software-pipelined tile loop: the next tile's coordinates / weights are requested from LDS before the current
  // tile's ~55 FP64 instructions run, so the ds_read latency hides behind them instead of stalling every tile.
  typename tile_ptr<XL>::type xt = (typename tile_ptr<XL>::type)(xs + lane);
  lds_tile_ptr wt = (lds_tile_ptr)(aw + lane);
  constexpr int NX = DP + (DOT ? 1 : 0);  // rows this pass reads: the |x|^2 row only where it is used
  double cx[NX], cw[1 + G];
#pragma unroll
  for (int k = 0; k < NX; ++k) cx[k] = xt[k * 64];
#pragma unroll
  for (int a = 0; a < 1 + G; ++a) cw[a] = wt[a * 64];
#pragma unroll(SMALL ? 1 : (WG ? 2 : 4))
  for (int t = 0; t < ntiles; ++t) {
    double nx[NX], nw[1 + G];
    // unconditional advance (constant stride: the unrolled tiles share one address register and use immediate offsets);
    // the last iteration prefetches one tile past the end -- the host pads both arrays by one tile, the values are unused
    xt += XR * 64;
    wt += (1 + G) * 64;
    if (!LFX) {
#pragma unroll
      for (int k = 0; k < NX; ++k) nx[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) nw[a] = wt[a * 64];
    }
    double diff[DP];
    double r2;
    if (DOT) {
      r2 = cx[DP] + qq;
#pragma unroll
      for (int k = 0; k < DP; ++k) r2 = fma(cx[k], q2[k], r2);
      r2 = fmax(r2, 1.0e-300);  // rounding can leave a point that coincides with the query a hair below zero
      if (G > 0) {
#pragma unroll
        for (int a = 0; a < G; ++a) diff[a] = cx[a] - xq[a];
      }
    } else {
      r2 = 1.0e-300;  // keeps r2 > 0 for the rsq-based sqrt at no cost (invisible next to any r2 >= 1e-284)
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        diff[k] = cx[k] - xq[k];
        r2 = fma(diff[k], diff[k], r2);
      }
    }
    const double w0 = cw[0];  // alpha * (function-value weight)
    double base, first, second;
    if (LFX) {
      // the exp-table read goes out BEFORE the next tile's reads (volatile LDS reads keep their order, and LDS returns in
      // order), so the wait in front of the finish leaves the prefetch in flight instead of draining it every tile
      const RadialHead h = radial3_head<COV>(r2, (lds_tile_ptr)etab);
#pragma unroll
      for (int k = 0; k < NX; ++k) nx[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < 1 + G; ++a) nw[a] = wt[a * 64];
      radial3_finish<COV, (WG || G > 0), (WG && G > 0)>(h, base, first, second);
    } else {
      radial3<COV, (WG || G > 0), (WG && G > 0)>(r2, etab, base, first, second);
    }
    double sd = 0.0;  // sum_a w_a diff[a]  (derivative-observation weights; table rows a < G are the observed dims)
    if (G > 0) {
#pragma unroll
      for (int a = 0; a < G; ++a) sd = fma(cw[1 + a], diff[a], sd);
    }
    accf = fma(w0, base, accf);
    if (G > 0) accf = fma(first, sd, accf);
    if (WG) {
      double coef = w0 * first;
      if (G > 0) {
        coef = fma(second, sd, coef);
#pragma unroll
        for (int a = 0; a < G; ++a) accd[a] = fma(first, cw[1 + a], accd[a]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) accg[k] = fma(coef, diff[k], accg[k]);
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) cx[k] = nx[k];
#pragma unroll
    for (int a = 0; a < 1 + G; ++a) cw[a] = nw[a];
  }
  const double mu = mean + wave_sum_uniform(accf);
  if (WG) {
    double sg[DP];
    if (scr != nullptr)
      wave_sum_packed_lds<DP>(accg, scr, lane, sg);  // DP sums folded into DP / 4 in-row reductions
    else
      wave_sum_packed<DP>(accg, sg);
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      // d mu / d x'_k = sum coef (Xs_k - xq_k)  -  [k < G] sum first w_k   (frame coordinates);   f = -mu
      double v = sg[k];
      if (G > 0 && k < G) v -= wave_sum_uniform(accd[k < G ? k : 0]);
      grad[k] = -v;
    }
  }
  return -mu;
}

// The covariance type is wave-uniform: branch ONCE per pass (a branch inside the tile loop would split it into basic blocks
// and stop the scheduler from interleaving the independent per-tile dependency chains).
template <int DP, int G, bool WG, bool SMALL, bool XL, bool LF = false>
__device__ __forceinline__ double eval_pass(const double* __restrict__ xs, const double* __restrict__ aw,
                                            const double* __restrict__ etab, int ntiles, int cov_type, double mean,
                                            const double (&xq)[DP], double (&grad)[DP], int lane, double* __restrict__ scr = nullptr) {
  if (cov_type == MOE_COV_SQUARE_EXPONENTIAL)
    return eval_loop<DP, G, WG, MOE_COV_SQUARE_EXPONENTIAL, SMALL, XL, LF>(xs, aw, etab, ntiles, mean, xq, grad, lane, scr);
  return eval_loop<DP, G, WG, MOE_COV_MATERN_NU_2P5, SMALL, XL, LF>(xs, aw, etab, ntiles, mean, xq, grad, lane, scr);
}

// T Armijo trial points x' + alpha_t g s^2, alpha_t = alpha0 / 2^t, in ONE sweep over the tiles (no derivative observations, LDS
// table).  With x2 = -2 x' and d2 = -2 g s^2 (line_search_frame) the trial's q2 is x2 + alpha_t d2, so
//   r2_t = |x_j|^2 + |q_t|^2 + x_j . q2_t = (|x_j|^2 + x_j . x2) + alpha_t (x_j . d2) + |q_t|^2:
// the two projections p0, p1 are formed once per point (2 DP fmas) and every trial costs an add, an fma and a max on top of
// its square root / exp / polynomial -- (2 DP + 1) / T + 3 instructions per point for r2 instead of DP + 2, and one set of
// coordinate / weight loads, one reduction round and one decision round per T trials.  |q_t|^2 = (|x2|^2 + 2 alpha_t x2.d2 +
// alpha_t^2 |d2|^2) / 4 (wave-uniform).  Returns false without evaluating when a trial lies beyond kFarRadius (see eval_loop;
// |q(alpha)|^2 is convex in alpha, so the two ends of the bracket bound all trials).
// XL = false (coordinates streamed from L2: no |x|^2 row): the same with direct differences about x0' = -x2 / 2, as the
// workgroup-per-sample kernel does (point_terms_multi): r2_t = |x_j - x0'|^2 - 2 alpha_t (x_j - x0') . dv + alpha_t^2 |dv|^2, dv = -d2 / 2
// -- there one coordinate sweep through L2 serves T trials instead of one, which is most of what that kernel paid per trial.
// G > 0 (derivative observations; table rows a < G are the observed dimensions): a point also carries the derivative-weight sum
// sum_a w_a (x_j - q_t)_a = sdA - alpha_t sdB,  sdA = sum_a w_a (x_j - x0')_a,  sdB = sum_a w_a dv_a  (2 G fmas once per point, one
// fma per trial), multiplied by the first-derivative coefficient of the trial's distance.
// (eval_multi_loop_s: the three sums |x2|^2, x2.d2, |d2|^2 -- fixed along a trial line -- handed in by a caller that forms them once
//  per bracket, kg_mc_lane.hpp; eval_multi_loop forms them itself, in the same order)
template <int DP, int COV, int T, bool SMALL, bool XL = true, int G = 0, bool LF = false>
__device__ __forceinline__ bool eval_multi_loop_s(const double* __restrict__ xs, const double* __restrict__ aw,
                                                  const double* __restrict__ etab, int ntiles, double mean, const double (&x2)[DP],
                                                  const double (&d2)[DP], double sxx, double sxd, double sdd, double alpha0, int lane,
                                                  double (&f)[T]) {
  constexpr int WR = 1 + G;  // weight rows per tile
  double al[T], qq[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    al[t] = (t == 0) ? alpha0 : 0.5 * al[t > 0 ? t - 1 : 0];
    qq[t] = fma(0.25, fma(al[t], fma(al[t], sdd, 2.0 * sxd), sxx), 1.0e-300);
  }
  if (!(uniform(fmax(qq[0], 0.25 * sxx)) <= kFarRadius * kFarRadius)) return false;
  double acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.0;
  constexpr int NX = DP + (XL ? 1 : 0);  // rows per coordinate tile
  typename tile_ptr<XL>::type xt = (typename tile_ptr<XL>::type)(xs + lane);
  lds_tile_ptr wt = (lds_tile_ptr)(aw + lane);
  double cx[NX], cwa[WR];
#pragma unroll
  for (int k = 0; k < NX; ++k) cx[k] = xt[k * 64];
#pragma unroll
  for (int a = 0; a < WR; ++a) cwa[a] = wt[a * 64];
  double x0[DP], dv[DP], tt[T];  // (direct-difference form, and the derivative-weight sums)
  if (!XL || G > 0) {
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      x0[k] = -0.5 * x2[k];
      dv[k] = -0.5 * d2[k];
    }
#pragma unroll
    for (int t = 0; t < T; ++t) tt[t] = (al[t] * al[t]) * (0.25 * sdd);  // alpha_t^2 |dv|^2
  }
  if constexpr (LF && XL) {
    // Lookup-first order (LDS table; the caller asks for it: kg_mc_lane.hpp kLaneLookupFirst).  Per tile: the heads of all T trials and
    // their T exp-table reads, back to back; THEN the next tile's reads; then the finishes, whose polynomials need no table entry and
    // cover the one round trip a tile now waits for (the reads are volatile LDS reads: they keep this order, LDS returns in order, and
    // the wait before the first finish leaves the prefetch in flight).
    // one_tile ADVANCES xt / wt to the next tile, adds the current tile's terms to acc[] and leaves the next tile's rows in cx[] / cwa[].
    auto one_tile = [&]() __attribute__((always_inline)) {
      double nx[NX], nwa[WR];
      xt += NX * 64;  // (one tile of padding behind both arrays: see eval_loop)
      wt += WR * 64;
      const double cw = cwa[0];
      double sdA = 0.0, sdB = 0.0;  // derivative-weight sum of trial t: sdA - alpha_t sdB (see the loop below)
      if (G > 0) {
#pragma unroll
        for (int a = 0; a < G; ++a) {
          sdA = fma(cwa[1 + a], cx[a] - x0[a], sdA);
          sdB = fma(cwa[1 + a], dv[a], sdB);
        }
      }
      double p0 = cx[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) p0 = fma(cx[k], x2[k], p0);
      double p1 = cx[0] * d2[0];
#pragma unroll
      for (int k = 1; k < DP; ++k) p1 = fma(cx[k], d2[k], p1);
      RadialHead h[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const double r2 = fmax(fma(al[t], p1, p0 + qq[t]), 1.0e-300);
        h[t] = radial3_head<COV>(r2, (lds_tile_ptr)etab);
      }
#pragma unroll
      for (int k = 0; k < NX; ++k) nx[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < WR; ++a) nwa[a] = wt[a * 64];
      // (left to itself the scheduler runs some tiles' trials as a chain of head / read / wait / finish again)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < T; ++t) {
        double base, first, second;
        radial3_finish<COV, (G > 0), false>(h[t], base, first, second);
        acc[t] = fma(cw, base, acc[t]);
        if (G > 0) acc[t] = fma(first, fma(-al[t], sdB, sdA), acc[t]);
      }
#pragma unroll
      for (int k = 0; k < NX; ++k) cx[k] = nx[k];
#pragma unroll
      for (int a = 0; a < WR; ++a) cwa[a] = nwa[a];
    };
    // two tiles per iteration by hand: sched_barrier is a convergent operation, and the unroller leaves a loop with one and a
    // run-time trip count alone
    int tile = 0;
    for (; tile + 1 < ntiles; tile += 2) {
      one_tile();
      one_tile();
    }
    if (tile < ntiles) one_tile();
  } else {
#pragma unroll(SMALL ? 1 : 2)  // (four tiles for few trials: +-0.3 %, r5)
    for (int tile = 0; tile < ntiles; ++tile) {
      double nx[NX], nwa[WR];
      xt += NX * 64;  // (one tile of padding behind both arrays: see eval_loop)
      wt += WR * 64;
#pragma unroll
      for (int k = 0; k < NX; ++k) nx[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < WR; ++a) nwa[a] = wt[a * 64];
      const double cw = cwa[0];
      // derivative-weight sum of trial t: sum_a w_a (x_ja - x0_a - alpha_t dv_a) = sdA - alpha_t sdB
      double sdA = 0.0, sdB = 0.0;
      if (G > 0) {
#pragma unroll
        for (int a = 0; a < G; ++a) {
          sdA = fma(cwa[1 + a], cx[a] - x0[a], sdA);
          sdB = fma(cwa[1 + a], dv[a], sdB);
        }
      }
      if (XL) {
        double p0 = cx[XL ? DP : 0];
#pragma unroll
        for (int k = 0; k < DP; ++k) p0 = fma(cx[k], x2[k], p0);
        double p1 = cx[0] * d2[0];
#pragma unroll
        for (int k = 1; k < DP; ++k) p1 = fma(cx[k], d2[k], p1);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const double r2 = fmax(fma(al[t], p1, p0 + qq[t]), 1.0e-300);
          double base, first, second;
          radial3<COV, (G > 0), false>(r2, etab, base, first, second);
          acc[t] = fma(cw, base, acc[t]);
          if (G > 0) acc[t] = fma(first, fma(-al[t], sdB, sdA), acc[t]);
        }
      } else {
        double A = 1.0e-300, B = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double d0 = cx[k] - x0[k];
          A = fma(d0, d0, A);
          B = fma(d0, dv[k], B);
        }
        const double mB2 = -2.0 * B;
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const double r2 = fmax(fma(al[t], mB2, A + tt[t]), 1.0e-300);
          double base, first, second;
          radial3<COV, (G > 0), false>(r2, etab, base, first, second);
          acc[t] = fma(cw, base, acc[t]);
          if (G > 0) acc[t] = fma(first, fma(-al[t], sdB, sdA), acc[t]);
        }
      }
#pragma unroll
      for (int k = 0; k < NX; ++k) cx[k] = nx[k];
#pragma unroll
      for (int a = 0; a < WR; ++a) cwa[a] = nwa[a];
    }
  }
  // T wave sums, folded four / two at a time (packed reductions above)
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
  return true;
}

// T Armijo trials in one sweep with EVERY trial computed exactly as a single-trial value pass computes it (r6): q2_t = x2 + alpha_t d2
// and |q_t|^2 formed per trial as a value pass of eval_loop forms them, r2 = (|x_j|^2 + |q_t|^2) then the DP fmas in row order, the tile
// sums in tile order, one wave_sum_uniform per trial -- the bits of T separate passes (T DP fmas per point instead of the 2 DP + 2 T of
// the line decomposition above: no dearer up to DP = 4 and T = 5), with one set of coordinate / weight loads and one decision round.
// For the small shapes whose end points the reference's 100-step x 10-restart fixtures pin: there the line decomposition's rounding moved
// them by 1.01e-6 (kg.hip), so until r6 those shapes ran one trial per pass.  LDS table only.  Returns false without evaluating when a
// trial lies beyond kFarRadius (the single-trial pass returns the prior mean there: the caller falls back to it).
template <int DP, int COV, int T, int G, bool LF = false>
__device__ __forceinline__ bool eval_multi_exact(const double* __restrict__ xs, const double* __restrict__ aw,
                                                 const double* __restrict__ etab, int ntiles, double mean, const double (&x2)[DP],
                                                 const double (&d2)[DP], double alpha0, int lane, double (&f)[T]) {
  constexpr int WR = 1 + G;
  constexpr int NX = DP + 1;
  double al[T], qq[T], q2[T][DP], xq[T][G > 0 ? G : 1];
  bool near_all = true;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    al[t] = (t == 0) ? alpha0 : 0.5 * al[t > 0 ? t - 1 : 0];
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      q2[t][k] = fma(al[t], d2[k], x2[k]);
      ss = fma(q2[t][k], q2[t][k], ss);
    }
#pragma unroll
    for (int a = 0; a < G; ++a) xq[t][a] = -0.5 * q2[t][a];
    qq[t] = fma(ss, 0.25, 1.0e-300);
    near_all = near_all && (uniform(qq[t]) <= kFarRadius * kFarRadius);
  }
  if (!near_all) return false;
  double acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.0;
  lds_tile_ptr xt = (lds_tile_ptr)(xs + lane);
  lds_tile_ptr wt = (lds_tile_ptr)(aw + lane);
  double cx[NX], cw[WR];
#pragma unroll
  for (int k = 0; k < NX; ++k) cx[k] = xt[k * 64];
#pragma unroll
  for (int a = 0; a < WR; ++a) cw[a] = wt[a * 64];
#pragma unroll 1
  for (int tile = 0; tile < ntiles; ++tile) {
    double nx[NX], nw[WR];
    xt += NX * 64;  // (one tile of padding behind both arrays: see eval_loop)
    wt += WR * 64;
    const double w0 = cw[0];
    if (!LF) {
#pragma unroll
      for (int k = 0; k < NX; ++k) nx[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < WR; ++a) nw[a] = wt[a * 64];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        double r2 = cx[DP] + qq[t];
#pragma unroll
        for (int k = 0; k < DP; ++k) r2 = fma(cx[k], q2[t][k], r2);
        r2 = fmax(r2, 1.0e-300);
        double base, first, second;
        radial3<COV, (G > 0), false>(r2, etab, base, first, second);
        acc[t] = fma(w0, base, acc[t]);
        if (G > 0) {
          double sd = 0.0;
#pragma unroll
          for (int a = 0; a < G; ++a) sd = fma(cw[1 + a], cx[a] - xq[t][a], sd);
          acc[t] = fma(first, sd, acc[t]);
        }
      }
    } else {
      RadialHead h[T];  // (lookup-first, as in eval_multi_loop_s: T heads and table reads, the next tile's reads, T finishes)
#pragma unroll
      for (int t = 0; t < T; ++t) {
        double r2 = cx[DP] + qq[t];
#pragma unroll
        for (int k = 0; k < DP; ++k) r2 = fma(cx[k], q2[t][k], r2);
        r2 = fmax(r2, 1.0e-300);
        h[t] = radial3_head<COV>(r2, (lds_tile_ptr)etab);
      }
#pragma unroll
      for (int k = 0; k < NX; ++k) nx[k] = xt[k * 64];
#pragma unroll
      for (int a = 0; a < WR; ++a) nw[a] = wt[a * 64];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        double base, first, second;
        radial3_finish<COV, (G > 0), false>(h[t], base, first, second);
        acc[t] = fma(w0, base, acc[t]);
        if (G > 0) {
          double sd = 0.0;
#pragma unroll
          for (int a = 0; a < G; ++a) sd = fma(cw[1 + a], cx[a] - xq[t][a], sd);
          acc[t] = fma(first, sd, acc[t]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) cx[k] = nx[k];
#pragma unroll
    for (int a = 0; a < WR; ++a) cw[a] = nw[a];
  }
#pragma unroll
  for (int t = 0; t < T; ++t) f[t] = -(mean + wave_sum_uniform(acc[t]));
  return true;
}

template <int DP, int COV, int T, bool SMALL, bool XL = true, int G = 0>
__device__ __forceinline__ bool eval_multi_loop(const double* __restrict__ xs, const double* __restrict__ aw,
                                                const double* __restrict__ etab, int ntiles, double mean, const double (&x2)[DP],
                                                const double (&d2)[DP], double alpha0, int lane, double (&f)[T]) {
  double sxx = 0.0, sxd = 0.0, sdd = 0.0;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    sxx = fma(x2[k], x2[k], sxx);
    sxd = fma(x2[k], d2[k], sxd);
    sdd = fma(d2[k], d2[k], sdd);
  }
  return eval_multi_loop_s<DP, COV, T, SMALL, XL, G>(xs, aw, etab, ntiles, mean, x2, d2, sxx, sxd, sdd, alpha0, lane, f);
}

// TensorProductDomain::LimitUpdate (gpp_domain.cpp:64-105) on one coordinate.
__device__ __forceinline__ double limit_update_1d(double lo, double hi, double max_relative_change, double x, double desired) {
  double dist = fmin(x - lo, hi - x);
  if (fabs(desired) > max_relative_change * dist) desired = copysign(max_relative_change * dist, desired);
  const double next = x + desired;
  if (next < lo || next > hi) {
    if (next < lo) {
      dist = lo - x;
      desired = (x + desired * 0.5 < lo) ? dist * 0.5 : desired * 0.5;
    } else {
      dist = hi - x;
      desired = (x + desired * 0.5 > hi) ? dist * 0.5 : desired * 0.5;
    }
  }
  return desired;
}

// out[r] = v[perm[r]] for wave-uniform v (select chains on uniform data; identity when the GP has no derivatives)
template <int DP, int G>
__device__ __forceinline__ void to_table_order(const double (&v)[DP], const int* perm, double (&out)[DP]) {
  if (G == 0) {
#pragma unroll
    for (int r = 0; r < DP; ++r) out[r] = v[r];
  } else {
#pragma unroll
    for (int r = 0; r < DP; ++r) {
      double o = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) o = (perm[r] == k) ? v[k] : o;
      out[r] = o;
    }
  }
}

template <int DP, int G>
__device__ __forceinline__ void from_table_order(const double (&v)[DP], const int* perm, double (&out)[DP]) {
  if (G == 0) {
#pragma unroll
    for (int k = 0; k < DP; ++k) out[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double o = 0.0;
#pragma unroll
      for (int r = 0; r < DP; ++r) o = (perm[r] == k) ? v[r] : o;
      out[k] = o;
    }
  }
}

// ---- LDS layout constants of the kernel families (the kernels and the host's geometry, kg.hip, read the same ones) ----
constexpr int kCstRows = 6;  // arrays of DP doubles in the LDS constant block of the frame line search (kg_mc_wave.hpp)
constexpr int kPartLen = 48;  // doubles per partial slot of a packed reduction: f | DP gradient sums | sum of coefficients | G derivative sums (<= 1 + 32 + 1 + 12)
constexpr int kLsRows = 6;    // line-search vectors per wave in LDS (line_search_lds): x | masked gradient | step | x at restart start | x0 and dv of the trial line (frame)
// per-wave LDS scratch of the wide-dimension evaluator (WideEval, d > 16) behind the z / beta scratch of a weight slab
constexpr int kWideScratch = kLsRows * kMaxDimPadded + kPartLen;
// Which wave-per-sample instantiations use it: the streamed ones from 16 coordinate rows on.  (r3, streamed tables at 8 / 12 rows:
// the evaluator of kg_mc_wave.hpp with its fused value + gradient passes stays ahead -- n = 1500 .. 3000, d = 8: 1.15 / 1.39 / 2.15 ms per
// evaluation against 1.24 / 1.62 / 2.52; at 16 rows WideEval wins, n = 1000: 0.27 against 0.345 ms.)
constexpr bool wide_eval(int dp, bool xlds) { return !xlds && dp >= 16; }
constexpr int kMaxBlockWaves = 8;  // wavefronts per workgroup of the workgroup-per-sample kernel
// Fixed LDS words of the workgroup-per-sample kernel (doubles), before the tile data.
constexpr int kBlockFixed = kExpTabLen + 2 * kMaxMB + 2 * kMaxBlockWaves * kPartLen + 2 + kMaxBlockWaves * kLsRows * kMaxDimPadded;
constexpr int kLaneCstRows = 8;  // lane-parked kernel: s | 1 / s | centre | pinned value | lower bound | upper bound (original units) | perm | free (1 / 0)

// SimplexIntersectTensorProductDomain::LimitUpdate's second half (gpp_domain.cpp:255-289) on the wave's LDS rows: xs / ss = the
// current point and the step AFTER the tensor-product limit (table-row order; pinned rows hold a zero step), walked in the reference's
// coordinate order j = 0 .. size - 1 through inv_perm.  If the proposed point leaves the unit simplex the step becomes
// relaxed * (step / norm) -- half the distance to the diagonal face along its own direction; returns whether it does.  Every lane
// computes the same scalars (uniform LDS reads).
__device__ __forceinline__ bool simplex_limit(const KgMcParams& P, const double* __restrict__ xs, const double* __restrict__ ss,
                                              double& relaxed, double& norm) {
  const int size = P.dim - P.f;
  // VectorNorm (gpp_linear_algebra.cpp:53-72): the scaled recurrence
  if (size == 1) {
    norm = fabs(ss[P.inv_perm[0]]);
  } else {
    double sc = 0.0, scaled = 1.0;
    for (int j = 0; j < size; ++j) {
      const double v = ss[P.inv_perm[j]];
      if (v != 0.0) {
        const double a = fabs(v);
        if (sc < a) {
          const double t = sc / a;
          scaled = 1.0 + scaled * (t * t);
          sc = a;
        } else {
          const double t = a / sc;
          scaled += t * t;
        }
      }
    }
    norm = sc * sqrt(scaled);
  }
  if (norm == 0.0) norm = 2.2250738585072014e-308;
  // CheckPointInUnitSimplex (gpp_geometry.hpp:313-325) on x + step
  bool inside = true;
  double sum = 0.0;
  for (int j = 0; j < size; ++j) {
    const int r = P.inv_perm[j];
    const double nx = xs[r] + ss[r];
    if (nx < 0.0) inside = false;
    sum += nx;
  }
  inside = inside && (sum - 4.0 * 2.220446049250313e-16) <= 1.0;
  relaxed = 0.0;
  if (inside) return false;
  // Plane::DistanceToPlaneAlongVector (gpp_geometry.hpp:252-272) for the plane sum x_i / sqrt(size) - 1 / sqrt(size) = 0
  double xn = 0.0, vn = 0.0;
  for (int j = 0; j < size; ++j) {
    const int r = P.inv_perm[j];
    xn += xs[r] * P.inv_sqrt_size;
    vn += (ss[r] / norm) * P.inv_sqrt_size;
  }
  const double numerator = P.inv_sqrt_size - xn;
  double dist = (vn == 0.0) ? (numerator == 0.0 ? 0.0 : INFINITY) : numerator / vn;
  if (dist < 0.0) dist = 0.0;
  relaxed = 0.5 * dist;  // kInvalidStepScaleFactor
  return true;
}

// z_i (antithetic pairs, .cpp:171-180) and beta = L^-T z for global sample index s: lane c owns component c; copies go to
// the LDS scratch zb ([0, kMaxM) = z, [kMaxM, 2 kMaxM) = beta) for the uniform reads of the weight loop and the scan.
__device__ __forceinline__ void draw_z_beta(const KgMcParams& P, const double* __restrict__ Lsm, int s, int lane,
                                            double* __restrict__ zb, double& zc, double& bc) {
  const int m = P.m;
  const double sign = (s & 1) ? -1.0 : 1.0;
  zc = 0.0;
  if (lane < m) zc = sign * P.normals[(long)(s >> 1) * m + lane];
  // Back substitution L^T beta = z, column-oriented: once beta_r is final it is broadcast and every lane l < r folds
  // L[r][l] beta_r into its running sum -- no wave reduction per step, and row r of L does not depend on the recurrence, so
  // eight rows are requested at a time (one round trip to L2 per eight steps instead of one per step).
  bc = 0.0;
  double acc = 0.0;
  for (int r0 = m - 1; r0 >= 0; r0 -= 8) {
    double Lrow[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // unconditional loads from clamped addresses (a predicated load becomes a branch, and the eight loads would be
      // waited for one by one); entries of lanes above the diagonal are never used
      Lrow[i] = Lsm[max(r0 - i, 0) + min(lane, m - 1) * m];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = r0 - i;
      if (r >= 0) {
        if (lane == r) bc = (zc - acc) / Lrow[i];
        const int blo = __builtin_amdgcn_readlane(__double2loint(bc), r);
        const int bhi = __builtin_amdgcn_readlane(__double2hiint(bc), r);
        const double br = __hiloint2double(bhi, blo);
        if (lane < r) acc = fma(Lrow[i], br, acc);
      }
    }
  }
  zb[lane] = zc;  // kMaxM == 64 == wavefront size
  zb[kMaxM + lane] = bc;
  __builtin_amdgcn_wave_barrier();  // keep later cross-lane LDS reads after these writes
}

// Discretised-set scan (.cpp:436-449): f_j = -(mu_n(x_j) + c_j . z); returns the index of the FIRST best point.
__device__ __forceinline__ int discrete_scan(const KgMcParams& P, const double* __restrict__ rec, const double* __restrict__ zb,
                                             int lane) {
  const int m = P.m;
  const double* mu_disc = rec + P.rec.mu_disc;
  const double* C_disc = rec + P.rec.C_disc;
  double best_f = -INFINITY;
  int best_j = 0;
  for (int j0 = 0; j0 < P.A; j0 += 64) {
    const int j = j0 + lane;
    double fj = -INFINITY;
    if (j < P.A) {
      double v = mu_disc[j];
      const double* Cj = C_disc + (long)j * m;
      for (int c0 = 0; c0 < m; c0 += 8) {  // eight loads in flight, folded in the same order as one at a time
        double cv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) cv[i] = Cj[min(c0 + i, m - 1)];
#pragma unroll
        for (int i = 0; i < 8; ++i) v = fma(cv[i], (c0 + i < m) ? zb[min(c0 + i, kMaxM - 1)] : 0.0, v);
      }
      fj = -v;
    }
    double wmax = fj;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, off, 64));
    const unsigned long long ballot = __ballot(fj == wmax);
    const int first_lane = __ffsll((long long)ballot) - 1;
    if (wmax > best_f) {  // strict: an earlier chunk wins ties (priority-queue semantics of .cpp:440-447)
      best_f = wmax;
      best_j = j0 + first_lane;
    }
  }
  return __builtin_amdgcn_readfirstlane(best_j);
}

// ---- which evaluation a workgroup serves: the same rule in all four kernel families ----
// Static share first: workgroups b, b + E, b + 2E, ... serve evaluation b mod E (b mod 8 is also the XCD, so with E = 8 each
// evaluation's W / table stay in one XCD's L2); with fewer workgroups than evaluations a workgroup walks b, b + gridDim.x, ...
// Evaluations differ in cost (the line searches' pass counts), so a workgroup whose share has no tickets left does not exit while
// others still run: it MOVES to the evaluation with the most tickets left and draws from that one's counter.  Which wavefront takes
// which sample never mattered to the result -- every per-sample output has its own slot, the pass counters are integer atomics -- so
// the bits are those of the static assignment.
//   first_evaluation: where a workgroup starts.
//   next_evaluation:  called by every thread of the workgroup where a ticket loop has ended (workgroup-uniform control flow); returns the
//     evaluation to stage and draw from next, or -1: exit.  `moved` is the workgroup's own flag (false at first), `slot` one LDS word
//     that no wavefront uses between two samples.  The move: a barrier, then wave 0 reads the ticket counters of all E evaluations
//     (device-scope relaxed atomic loads: a plain load may be served stale), takes the largest num_local - min(counter, num_local), ties
//     to the first in cyclic order behind `e` so that thieves spread out, and exits below P.steal_min; the choice goes to the other
//     wavefronts through `slot`.  An evaluation that was left has nothing remaining ever again (the counters only grow), so a workgroup
//     moves at most E times.
__device__ __forceinline__ int first_evaluation(const KgMcParams& P, const VIdx& blockIdx) {
  return P.steal_skew != 0 ? 0 : (int)(blockIdx.x % (unsigned)P.E);
}
// (the move itself, on scalars.  Inlined: as an out-of-line call it put the headline kernel kg_mc_lane_kernel<8,0> at 256 VGPRs with 16
//  bytes of scratch per lane and added ~100 bytes to the frame kernels; inlined the headline stays at 255 VGPRs without scratch, and the
//  instantiations that already spilt gain 4 .. 20 bytes -- DESIGN 5.3 item 3)
__device__ __forceinline__ int move_to_fullest(const unsigned int* next_sample, unsigned long long* moves, int E, int num_local,
                                            int steal_min, int e, int* slot) {
  __syncthreads();  // every wavefront is out of its ticket loop: `slot` is free
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    unsigned long long key = 0;  // remaining tickets << 32 | ~(cyclic distance behind e)
    for (int c = lane; c < E; c += 64) {
      const unsigned int drawn = __hip_atomic_load(next_sample + (long)c * kTicketStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned int nl = (unsigned int)num_local;
      const unsigned int remaining = nl - min(drawn, nl);
      int dist = c - e - 1;
      if (dist < 0) dist += E;
      const unsigned long long k2 = ((unsigned long long)remaining << 32) | (0xffffffffu - (unsigned int)dist);
      key = k2 > key ? k2 : key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off, 64);
      key = o > key ? o : key;
    }
    if (lane == 0) {
      const unsigned int remaining = (unsigned int)(key >> 32);
      const int dist = (int)(0xffffffffu - (unsigned int)key);
      const int to = (remaining >= (unsigned int)steal_min) ? (e + 1 + dist) % E : -1;
      *(volatile int*)slot = to;
#if !MOE_BLOCK_PROF
      if (to >= 0) atomicAdd(moves, 1ull);
#endif
    }
  }
  __syncthreads();
  const int to = __builtin_amdgcn_readfirstlane(*(volatile int*)slot);
  __syncthreads();  // `slot` goes back to its wavefront
  return to;
}
__device__ __forceinline__ int next_evaluation(const KgMcParams& P, const VIdx& gridDim, int e, bool& moved, int* slot) {
  if (!moved && P.steal_skew == 0 && gridDim.x < (unsigned)P.E && e + (int)gridDim.x < P.E) return e + (int)gridDim.x;
  if (P.steal_min <= 0 || P.E == 1) return -1;
  moved = true;
  return move_to_fullest(P.next_sample, P.prof + kMovesWord, P.E, P.num_local, P.steal_min, e, slot);
}

}  // namespace mc

// bytes of dynamic LDS of the workgroup-per-sample kernel
inline size_t kg_mc_block_lds_bytes(int dp, int G, int num_lds_tiles) {
  return sizeof(double) * (mc::kBlockFixed + (size_t)num_lds_tiles * (dp + 1 + G) * 64);
}
// lane-parked kernel: bytes of LDS in front of the coordinate table
inline size_t kg_mc_lane_fixed_bytes(int dp, int rec_head) {
  return sizeof(double) * ((size_t)kExpTabLen + (size_t)mc::kLaneCstRows * dp + (size_t)((rec_head + 1) & ~1));
}

#endif  // __HIPCC__

}  // namespace moe
