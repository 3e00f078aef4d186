// cornell_moe_amd/csrc/kg.hip -- q-KG / d-KG Monte-Carlo evaluation (value + gradient) on gfx950: host orchestration of
// one BATCH of independent evaluations (the multistart axis).  This unit is the driver alone -- argument checks, the plan of the MC
// step, the records, the phases of one kg_launch and the batching around it; every kernel it launches lives in a unit of its own.
//
// Pipeline for a batch of E evaluations (every stage is one launch, or one launch per kind, for the whole batch):
//   1. state set-up (gp.hip enqueue_kg_state_batch): K*(X, Xu_e), dK*/dXq_e, K(X, discretised set_e) -> L^-1 / K^-1 applies
//      (tile GEMMs against the explicit inverse factor) -> Gram matrices, then the m x m algebra of PointsToSampleState /
//      KnowledgeGradientState (gpp_math.cpp:600-653, gpp_knowledge_gradient_optimization.cpp:292-317) on the device (kg_state.hip);
//   2. the coordinate tables, the start table, the sample pre-pass and the weight table where the plan has them (kg_prep.hip), and the
//      MC kernel (kg_mc.hpp, its family headers kg_mc_{wave,lane,stream,block}.hpp and the kg_mc_dp*.hip units): persistent wavefronts,
//      one MC sample at a time per wave, all E evaluations in one launch;
//   3. gradient tail (kg_tail.hip: T-free for q-KG, else through the materialised N x M covariance matrix), or the sum of the samples'
//      values, and the finish kernels of kg_state.hip.
// All reductions use fixed orders, so results are bitwise reproducible for a given shard layout.
#include "kg.hpp"

#include <algorithm>
#include <array>
#include <memory>
#include <optional>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "kg_mc.hpp"
#include "kg_prep.hpp"
#include "kg_state.hpp"
#include "kg_tail.hpp"

namespace moe {

// how many ensemble members share the launches being recorded on this thread (mcmc.hip; kg_launch sizes its MC grid for its share)
static thread_local int t_ens_members_hint = 1;
int ensemble_members_hint() { return t_ens_members_hint; }
void set_ensemble_members_hint(int members) { t_ens_members_hint = members > 1 ? members : 1; }


namespace {

// tickets per wavefront that the fullest evaluation must have left for an idle workgroup to move to it (plan_mc; DESIGN 7: the A/B of
// 1, 2 and 4 -- 29.11 / 29.05 / 29.12 ms per headline step, the three runs of 2 within 0.005 ms; MOE_KG_STEAL_MIN_PER_WAVE overrides)
constexpr int kStealWaves = 2;

struct EventTimer {
  hipEvent_t a = nullptr, b = nullptr;  // (created on first use: a recorded evaluation -- launch.hpp -- times nothing)
  bool on = false;
  EventTimer() = default;
  EventTimer(const EventTimer&) = delete;
  EventTimer& operator=(const EventTimer&) = delete;
  ~EventTimer() {
    if (a != nullptr) (void)hipEventDestroy(a);
    if (b != nullptr) (void)hipEventDestroy(b);
  }
  void start(hipStream_t s) {
    on = Recorder::current() == nullptr;
    if (!on) return;
    if (a == nullptr) {
      MOE_HIP_CHECK(hipEventCreate(&a));
      MOE_HIP_CHECK(hipEventCreate(&b));
    }
    MOE_HIP_CHECK(hipEventRecord(a, s));
  }
  void stop(hipStream_t s) {
    if (on) MOE_HIP_CHECK(hipEventRecord(b, s));
  }
  double ms() {
    if (!on) return 0.0;
    MOE_HIP_CHECK(hipEventSynchronize(b));
    float t = 0.f;
    MOE_HIP_CHECK(hipEventElapsedTime(&t, a, b));
    return t;
  }
};

std::optional<int> env_opt(const char* name) {  // unset and empty: no value
  const char* v = std::getenv(name);
  if (v && *v) return std::atoi(v);
  return std::nullopt;
}

// the MC kernel families (kg_mc.hpp: instantiated per padded dimension in the kg_mc_dp*.hip units)
void launch_mc(const KgMcParams& P, int dp, int G, bool xlds, int blocks, int waves, size_t shm, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) { mc::launch_dp<decltype(DP)::value>(P, G, xlds, blocks, waves, shm, s); });
}

void launch_mc_lane(const KgMcParams& P, int dp, int G, int rec_head, int blocks, int waves, size_t shm, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) {
    if constexpr (decltype(DP)::value <= 16)  // (kg_mc_lane.hpp kMaxLaneDP)
      mc::launch_lane_dp<decltype(DP)::value>(P, G, rec_head, blocks, waves, shm, s);
    else
      throw Error(MOE_ERR_RUNTIME, "unsupported padded dimension in the lane-parked MC kernel");
  });
}

void launch_mc_stream(const KgMcParams& P, int dp, int G, int blocks, int waves, size_t shm, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) { mc::launch_stream_dp<decltype(DP)::value>(P, G, blocks, waves, shm, s); });
}

void launch_mc_block(const KgMcParams& P, int dp, int G, int tr, int num_lds_tiles, int blocks, int waves, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) { mc::launch_block_dp<decltype(DP)::value>(P, G, tr, num_lds_tiles, blocks, waves, s); });
}

// The shape of one kg_launch: the union of u = q + p points with 1 + g rows each (m rows), A = u + P points in the discretised set,
// `size` = d - num_fidelity coordinates the inner optimisations move, E evaluations of num_local samples each.
struct KgDims {
  int d, dp, f, size, n, g, g1, N;
  int q, p, u, m, A, E, ngrad, qd;
  int num_mc, first_sample, num_local;
  bool want_grad, simplex;
};

KgDims check_kg_args(const GpDev& gp, int f, const moe_gd_params_t& gd, int P, int E, int q, int p, int num_mc, int first_sample,
                     int num_local, bool want_grad) {
  KgDims k;
  k.d = gp.d, k.dp = gp.dp, k.f = f, k.n = gp.n, k.g = gp.g, k.g1 = 1 + gp.g, k.N = gp.N;
  k.q = q, k.p = p, k.u = q + p, k.m = k.u * k.g1, k.A = k.u + P, k.E = E;
  k.ngrad = want_grad ? q * k.g1 * k.d : 0;
  k.qd = q * k.d;
  k.num_mc = num_mc, k.first_sample = first_sample, k.num_local = num_local;
  k.want_grad = want_grad;
  if (q <= 0) throw Error(MOE_ERR_BOUNDS, "num_to_sample must be positive", q, 1, 1e9);
  if (p < 0) throw Error(MOE_ERR_BOUNDS, "num_being_sampled must be non-negative", p, 0, 1e9);
  if (E <= 0) throw Error(MOE_ERR_BOUNDS, "num_evals must be positive", E, 1, 1e9);
  if (k.m > kMaxMB)
    throw Error(MOE_ERR_BOUNDS, "(q + p)(1 + num_derivatives) > 128 is not supported by the device kernels", k.m, 1, kMaxMB);
  if (k.g > 12) throw Error(MOE_ERR_BOUNDS, "d-KG with more than 12 observed derivatives is not supported by the device kernels", k.g, 0, 12);
  if (f < 0 || f >= k.d) throw Error(MOE_ERR_BOUNDS, "num_fidelity out of range", f, 0, k.d - 1);
  if (num_mc <= 0) throw Error(MOE_ERR_BOUNDS, "num_mc must be positive", num_mc, 1, 1e12);
  if (first_sample < 0 || (first_sample & 1) || num_local <= 0 || first_sample + num_local > num_mc)
    throw Error(MOE_ERR_INVALID_VALUE, "MC shard must be an even-aligned slice of [0, num_mc)", first_sample, 0, 0);
  if (gd.max_num_steps <= 0) throw Error(MOE_ERR_BOUNDS, "max_num_steps must be positive", gd.max_num_steps, 1, 1e9);
  k.size = k.d - f;
  if (gd.domain_type != MOE_DOMAIN_TENSOR_PRODUCT && gd.domain_type != MOE_DOMAIN_SIMPLEX)
    throw Error(MOE_ERR_INVALID_VALUE, "unknown domain_type (0 = tensor product, 1 = simplex)", gd.domain_type, 0, 1);
  k.simplex = gd.domain_type == MOE_DOMAIN_SIMPLEX;  // the inner optimisations' domain (r4)
  return k;
}

// How the MC step of one kg_launch runs: which kernel, its launch geometry, the passes around it, and the form of the gradient tail.
struct McPlan {
  int G = 0;                  // derivative-weight slots of the MC kernel instantiation
  int ntiles = 0;             // 64-point tiles of the n + u points
  int variant = 0;            // 0: wave-per-sample (LDS slabs), 1: workgroup-per-sample, 2: streamed weights
  bool xlds = true;           // variant 0: the coordinate table in LDS
  bool far_frame = false;     // the frame is wider than MOE_KG_DOT_MAX_RADIUS2: direct-difference kernels, single-trial passes
  bool wide_frame = false;    // ... or d > 16: no coordinate table in LDS either way
  bool small_lane = false;    // a small shape with few samples: the lane-parked kernel's single-trial passes
  bool lane_kernel = false;   // variant 0 in its lane-parked form (kg_mc_lane.hpp)
  int waves = 0, blocks = 0;  // wavefronts per workgroup, workgroups
  size_t shm = 0;             // dynamic LDS bytes (variants 0, 2)
  int tr = -1, num_lds_tiles = 0;  // variant 1: register tiles per wave, tiles in LDS
  int wide_lds_tiles = 0;     // leading tiles of the coordinate table kept in LDS (WideEval)
  int pair_rows = 0;          // the coordinate table in row pairs
  int rec_head = 0;           // doubles of the record head [L | mu_disc | C_disc | disc] (the lane-parked kernel's LDS copy)
  int multi_trial = 0;        // KgMcParams::multi_trial
  bool prep = false;          // the sample pre-pass runs (beta, best_j)
  bool start_table = false;   // the line searches take their first gradient from the start table (kg_start_table_kernel)
  bool weight_table = false;  // the per-sample weight table is built
  long v_stride = 0;          // its doubles per sample, and its slots per point
  int v_slots1 = 0;
  int steal_min = 0;          // KgMcParams::steal_min (0: static assignment) and ::steal_skew
  int steal_skew = 0;
  bool fused_tail = false;    // the T-free q-KG tail
  int chunk_len = 0;          // samples per TB partial of the tail
};

// Every decision about how the MC step runs, from the evaluation's shape, the GP, the points of the call and the switches read at the
// top (tests set them per call to reach shipped paths at small sizes, or to compare two shipped forms).  Allocates and launches nothing.
McPlan plan_mc(const GpDev& gp, const KgDims& k, const double* bounds, const double* Xq_all, const double* Xp, double weight_table_gb) {
  const double max_radius2 = (double)env_int("MOE_KG_DOT_MAX_RADIUS2", 10000);
  const bool lane_on = env_int("MOE_KG_LANE", 1) != 0;
  const long small_lane_max_samples = env_int("MOE_KG_SMALL_LANE_MAX_SAMPLES", 1024);
  const bool small_multi = env_int("MOE_KG_SMALL_MULTI", 1) != 0;
  const std::optional<int> forced_tr = env_opt("MOE_KG_TR");
  const std::optional<int> forced_variant = env_opt("MOE_KG_VARIANT");
  const int prep_mode = env_int("MOE_KG_PREP", -1);  // 1: the sample pre-pass for every kernel, 0: only where it is mandatory
  const bool stream_weights = env_int("MOE_KG_STREAM_WEIGHTS", 1) != 0;
  const bool steal = env_int("MOE_KG_STEAL", 1) != 0;           // 0: a workgroup keeps to its static share of the evaluations
  const bool steal_skew = env_int("MOE_KG_STEAL_SKEW", 0) != 0;  // test switch: every workgroup starts on evaluation 0
  // the weight table's cap: the caller's share of the workspace budget (kg_evaluate_batch, kg_mcmc_sums), 4 GB for a bare kg_launch
  const double v_cap = std::getenv("MOE_KG_V_MAX_GB") ? (double)env_int("MOE_KG_V_MAX_GB", 4)
                                                      : (weight_table_gb >= 0.0 ? weight_table_gb : 4.0);
  McPlan pl;
  pl.fused_tail = fused_tail_taken(k.want_grad, k.g, k.m);

  const int d = k.d, dp = k.dp, n = k.n, g = k.g, m = k.m, u = k.u, A = k.A, E = k.E, num_local = k.num_local;
  // derivative-weight slots of the MC kernel instantiation: one per observed derivative up to 4, then 8 or 12 (unused slots
  // carry zero weights); more than 4 always take the workgroup-per-sample kernel
  // (d > 16: slot counts {0, 4, 8, 12} only -- the DP > 16 sets of launch_dp / launch_block_dp / launch_stream_dp)
  const bool wide_dp = dp > 16;
  const int G = wide_dp ? (g == 0 ? 0 : (g <= 4 ? 4 : (g <= 8 ? 8 : 12))) : (g <= 4 ? g : (g <= 8 ? 8 : 12));
  const int ntiles = (n + u + 63) / 64;

  // ---- MC launch geometry: workgroup = `waves` wavefronts sharing one LDS coordinate table ----
  const size_t tab_bytes = sizeof(double) * (size_t)ntiles * (dp + 1) * 64;  // LDS copy: + the |x|^2 row (kg_mc.hpp eval_loop)
  const size_t slab_bytes = sizeof(double) * ((size_t)ntiles * (1 + G) * 64 + 2 * kMaxM);
  // (streamed coordinates: + the wave's line-search vectors and packed-sum slot -- kg_mc_lds.hpp WideEval)
  const size_t slab_stream_bytes = slab_bytes + (mc::wide_eval(dp, false) ? sizeof(double) * mc::kWideScratch : 0);
  // the exp table sits in front of everything; one weight tile of padding at the very end (eval_loop prefetches one tile
  // past the last wave's slab)
  const size_t pad_bytes = sizeof(double) * (size_t)(1 + G) * 64;
  const size_t fixed_bytes = sizeof(double) * (kExpTabLen + (size_t)mc::kCstRows * dp);  // exp table + frame constants
  const size_t lds_max = 160 * 1024 - fixed_bytes - pad_bytes;
  bool xlds = true;
  // The value passes of the LDS-table kernel take r^2 as |x_j|^2 + |q|^2 - 2 x_j.q (kg_mc.hpp eval_loop), whose absolute error is
  // ~eps (|x|^2 + |q|^2) in the centred, scaled frame of the tables: harmless while the point set spans tens of length
  // scales, but 1e-9 .. 1e-5 of r^2 at 1e3 .. 1e5 length scales (short length scales of a hyper-parameter MCMC ensemble) --
  // enough to break the 1e-8 parity with the reference.  Beyond a frame radius of 100 length scales the direct-difference
  // kernels are used instead (coordinates streamed from L2, or the workgroup-per-sample kernel): slower, exact.
  bool wide_frame = false, far_frame = false;
  {
    // The extent is taken from what does NOT depend on the batch -- the training points (cached in the GP), the points being
    // sampled, and the DOMAIN box the restarts live in -- so that a restart takes the same kernel whether it is evaluated alone,
    // in a batch, or in another rank's shard (r3, ADVICE: moe_kg_batch_multi / dist.py promise bit-identical restarts).  Only a
    // point_to_sample outside the box (or a fidelity coordinate, which has no inner bound) adds its own distance.
    double rad2 = 0.0;
    for (int kk = 0; kk < d; ++kk) {
      const double c = gp.x_mean[kk];
      double ext = gp.x_ext[kk];
      if (kk < k.size) ext = std::max(ext, std::max(std::fabs(bounds[2 * kk] - c), std::fabs(bounds[2 * kk + 1] - c)));
      for (size_t i = 0; i < (size_t)E * k.q; ++i) {
        const double v = Xq_all[i * d + kk];
        if (kk >= k.size || v < bounds[2 * kk] || v > bounds[2 * kk + 1]) ext = std::max(ext, std::fabs(v - c));
      }
      for (int i = 0; i < k.p; ++i) ext = std::max(ext, std::fabs(Xp[(size_t)i * d + kk] - c));
      rad2 += (ext * gp.cp.inv_l[kk]) * (ext * gp.cp.inv_l[kk]);
    }
    wide_frame = !(rad2 <= max_radius2);
    far_frame = wide_frame;
    // d > 16: the coordinate table of the wave-per-sample kernel would take (dp + 1) 512 bytes per tile; that kernel is built
    // without it there, so these shapes take the same route as a wide frame
    if (wide_dp) wide_frame = true;
    if (wide_frame) xlds = false;
  }
  // one or two tiles per pass: a pass is a short dependent chain, so 16 wavefronts per workgroup (the <= 128-VGPR instantiation,
  // single-trial passes).  From three tiles on the 8-wavefront instantiation with its multi-trial passes is faster (r2: n = 150,
  // d = 6, q = 4: 19 600 vs 12 900 evals/s; n = 200: 17 700 vs 12 100; two tiles, n = 100: 47 000 vs 49 000)
  // ... and only up to four dimensions: with eight or more coordinate rows the 128-VGPR instantiation spills heavily (0.5 - 1 KB of
  // scratch per lane) -- n = 60, d = 8: 27 300 vs 44 500 evals/s on the 8-wavefront instantiation, d = 12: 9 500 vs 35 800,
  // d = 16: 6 200 vs 25 200 (r2)
  // r5: a call with FEW samples on such a shape -- one evaluation of a KG-MCMC suggestion: n = 30, 20 restarts x 128 samples; the
  // drop-in boundary's one-at-a-time calls -- takes the lane-parked kernel instead, eight wavefronts, with the same single-trial passes:
  // the same bits as the 16-wavefront instantiation (tests/test_gpu_sweep.py: test_small_shape_kernels_agree), so which of the two runs
  // may depend on the size of the call.  MC kernel of one evaluation at n = 30, M = 128: 0.087 -> 0.056 ms (M = 2000: 0.165 -> 0.132);
  // a suggestion 0.212 -> 0.18-0.19 s.  In throughput the 16-wavefront instantiation keeps its lead (batch of 64, M = 2000: 0.0200 vs
  // 0.0249 ms per evaluation), hence the sample bound.  (The lane-parked kernel's MULTI-trial passes would be faster still -- 0.17 s --
  // but their dot-form distances move the end points of the reference's 100-step x 10-restart fixtures by up to 1.01e-6, beyond the
  // 1e-6 those fixtures are held to: not taken.)  `profiles/r05_z_*`.
  const bool small_shape = ntiles <= 2 && dp <= 4;
  // r6: decided from the evaluation's OWN sample count, not from the call's -- which kernel an evaluation takes never
  // depends on the batch or the rank it is evaluated in (the two kernels agree bit for bit on the tested shapes; the promise of
  // batch-independent bits no longer rests on that)
  // (a simplex inner domain: the lane-parked kernel at every sample count -- the 16-wavefront instantiation has no simplex update)
  const bool small_lane = small_shape && lane_on && (k.simplex || (long)num_local <= small_lane_max_samples);
  const int max_waves = (small_shape && !small_lane) ? 16 : 8;
  int waves = 0;
  if (tab_bytes + slab_bytes <= lds_max) waves = (int)std::min<size_t>(max_waves, (lds_max - tab_bytes) / slab_bytes);
  // (3 wavefronts per CU on the LDS table still beat the workgroup-per-sample kernel without derivative observations --
  //  n = 1500, d = 8: 2.1 vs 3.1 ms per evaluation; with 2 they lose -- n = 1700: 3.6 vs 3.4)
  const int min_xlds_waves = 4;  // (r2: 4 -- with 3 the streaming kernel and its 8 wavefronts win, n = 1500: 1.15 vs 1.44 ms)
  if (waves < min_xlds_waves || wide_frame) {  // coordinates stay in L2: more wavefronts per workgroup fit
    const int w2 = (int)std::min<size_t>(8, lds_max / slab_stream_bytes);
    if (w2 > waves || wide_frame) {  // (the instantiation without the LDS table is built for <= 8 wavefronts)
      waves = w2;
      xlds = false;
    }
  }
  // Variant selection: the wave-per-sample kernel needs the coordinate table AND >= 3 weight slabs in LDS; bigger point
  // sets (up to 32 tiles = 2048 points) go to the workgroup-per-sample kernel (coordinates in registers, 4 waves);
  // beyond that the wave-per-sample kernel streams coordinates from L2 (slow, but correct).
  // workgroup-per-sample geometry: 8 wavefronts; TR register tiles per wave, the remaining tiles in LDS
  const int bwaves = 8;
  int tr = -1, num_lds_tiles = 0;
  for (int cand : {0, 2, 4}) {
    if (wide_dp && cand != 0) break;  // (d > 16: all tiles in LDS or the streaming wave-per-sample kernel)
    const int tl = std::max(0, ntiles - bwaves * cand);
    if (kg_mc_block_lds_bytes(dp, G, tl) <= (size_t)160 * 1024) {
      tr = cand;
      num_lds_tiles = tl;
      break;
    }
  }
  if (!wide_dp && forced_tr) tr = *forced_tr;
  if (tr >= 0) num_lds_tiles = std::max(0, ntiles - bwaves * tr);
  int variant = (xlds && waves >= min_xlds_waves) ? 0 : (tr >= 0 ? 1 : 0);
  // Without derivative observations the wave-per-sample kernel streaming its coordinates from L2 now beats the workgroup-per-sample
  // kernel at every size both can run (r2: its multi-trial passes sweep the coordinates once per five Armijo trials -- n = 1600:
  // 1.23 vs 2.68 ms per evaluation, 2000: 1.39 vs 2.67, 3000: 2.15 vs 3.21, d = 8, q = 4, M = 1e4); far frames (single-trial
  // passes) keep the old choice
  if (G == 0 && !far_frame && waves >= 1) variant = 0;
  // with derivative observations (a point's 1 + G weights make the slabs bigger) the streamed kernel wins while five of them fit:
  // d = 12, g = 3, q = 8, M = 4000: n = 800 0.86 vs 1.10 ms; with four (n = 1200) 1.28 vs 1.21
  if (G > 0 && G <= 4 && !far_frame && !xlds && waves >= 5) variant = 0;
  if (G > 4 || m > kMaxM) variant = 1;  // (the wave-per-sample kernel: up to four derivative slots, one lane per component)
  // Variant 2, the streamed-weights wave-per-sample kernel (kg_mc_stream.hpp kg_mc_stream_kernel), takes what would go to the
  // workgroup-per-sample kernel whenever the per-sample weight table (fantasy points and tile padding included) fits its cap and
  // every derivative slot is an observed derivative (a point's table rows ARE its weights)
  const long v_stride_tiles = (long)ntiles * 64 * (1 + G);  // (the table of the streamed-weights kernel: 1 + G slots per point)
  // (the size test is per EVALUATION: which kernel an evaluation takes must not depend on the batch it shares a call with -- the
  //  callers size their batches with kg_max_batch, which budgets every evaluation's table)
  // (r4: 8 and 12 observed derivatives and m > 64 too -- the kernel itself needs neither m nor beta once the sample pre-pass and the
  //  weight table are there)
  // (r4: and any number of observed derivatives up to the slot count -- the table pads a point's weights to 1 + G)
  const bool stream_ok = prep_mode != 0 &&
                         8.0 * (double)v_stride_tiles * (double)num_local / 1e9 <= v_cap;
  if (stream_ok && stream_weights) {
    // (r3, ms of MC per evaluation, `profiles/r03_variant2_sweep.txt`: C5 7.9 -> 5.0; d = 12, g = 3, q = 8, M = 4000: n = 1200 1.24 -> 0.68 against the
    //  workgroup-per-sample kernel, n = 800 0.80 -> 0.48 against the wave-per-sample kernel streaming its coordinates with five weight
    //  slabs in LDS; without derivative observations it pays once fewer than five slabs fit: n = 6000, d = 8 5.79 -> 4.96, but n = 3000
    //  -- six slabs -- 2.18 -> 2.34)
    if (variant == 1) variant = 2;
    else if (variant == 0 && !xlds && (G > 0 || waves <= 4)) variant = 2;
    // with derivative observations also against the LDS-table kernel, from 12 table rows on or once it runs fewer than eight waves
    // (`profiles/r03_variant2_small.txt`: n = 300 / 500, d = 12, g = 3: 0.29 -> 0.21 / 0.45 -> 0.30 ms; n = 600, d = 8, g = 4, four
    //  slabs: 0.49 -> 0.33; but n = 400, d = 8, g = 2 on eight waves: 0.18 against 0.20 -- stays)
    else if (variant == 0 && xlds && G > 0 && (dp >= 12 || waves < 8)) variant = 2;
  }
  if (forced_variant) {
    if (*forced_variant == 2 && !stream_ok)
      throw Error(MOE_ERR_RUNTIME, "the streamed-weights MC kernel needs the weight table within its cap");
    // (shapes the LDS-slab wave-per-sample kernel is not built for keep to the other two)
    if (!(*forced_variant == 0 && (G > 4 || m > kMaxM))) variant = *forced_variant;
  }
  if (variant == 0 && waves < 1)
    throw Error(MOE_ERR_RUNTIME, "training set too large for the MC kernel (one sample's weights exceed LDS)");
  size_t shm = 0;
  int wg_per_cu = 1, wide_lds_tiles = 0;
  // r5: the lane-parked form of the LDS-table kernel (kg_mc_lane.hpp) wherever it holds as many wavefronts: its LDS also carries the
  // evaluation's record head [L | mu_disc | C_disc | disc] (the same for every evaluation of a call and every batch: the choice
  // depends on the evaluation's shape alone).  Same results bit for bit (MOE_KG_LANE=0: the frame line search of rounds 2-4).
  auto even = [](int v) { return (v + 1) & ~1; };
  const int rec_head = even(m * m) + even(A) + even(A * m) + even(A * k.size);
  bool lane_kernel = false;
  if (variant == 0 && xlds && waves <= 8 && dp <= 16 && lane_on)
    lane_kernel = kg_mc_lane_fixed_bytes(dp, rec_head) + tab_bytes + (size_t)waves * slab_bytes + pad_bytes <= (size_t)160 * 1024;
  // the simplex update (simplex_limit) lives in the lane-parked line search (r6) and in line_search_lds -- the streamed-weights and the
  // workgroup-per-sample kernel; the frame line search of the other wave-per-sample instantiations has none
  if (k.simplex && variant == 0 && !lane_kernel) variant = stream_ok ? 2 : 1;
  if (variant == 1 && (tr < 0 || kg_mc_block_lds_bytes(dp, G, num_lds_tiles) > (size_t)160 * 1024))
    throw Error(MOE_ERR_RUNTIME, "point set too large for the workgroup-per-sample MC kernel");
  if (variant == 0) {
    shm = (lane_kernel ? kg_mc_lane_fixed_bytes(dp, rec_head) : fixed_bytes) +
          (xlds ? tab_bytes + (size_t)waves * slab_bytes : (size_t)waves * slab_stream_bytes) + pad_bytes;
    wg_per_cu = std::max(1, std::min((int)((size_t)160 * 1024 / shm), (waves > 8 ? 16 : 8) / waves));
    if (mc::wide_eval(dp, xlds)) {  // what the slabs leave of a workgroup's share of LDS holds the leading tiles of the table (kg_mc_lds.hpp WideEval)
      const size_t share = (size_t)160 * 1024 / wg_per_cu;
      wide_lds_tiles = (int)std::min<size_t>((size_t)ntiles, (share - shm) / (sizeof(double) * dp * 64));
      shm += sizeof(double) * (size_t)wide_lds_tiles * dp * 64;
    }
  } else if (variant == 2) {
    waves = 8;
    shm = sizeof(double) * (kExpTabLen + (size_t)waves * mc::kWideScratch);
    wide_lds_tiles = (int)std::min<size_t>((size_t)ntiles, ((size_t)160 * 1024 - shm) / (sizeof(double) * dp * 64));
    shm += sizeof(double) * (size_t)wide_lds_tiles * dp * 64;
  } else {
    waves = bwaves;
  }
  int blocks = gp.num_cu * wg_per_cu;
  if (blocks >= E) blocks = (blocks / E) * E;  // the same number of workgroups for every evaluation
  // r5, wave-per-sample kernels: no more workgroups per evaluation than its samples need for the same number of rounds -- 128 samples
  // on 12 workgroups of 8 wavefronts are two rounds, and so they are on 8; the CUs left alone go to whatever else is running (the other
  // members of an MCMC ensemble: a suggestion at the headline GP size 0.574 -> 0.540 s; alone on the chip 0.0136 vs 0.0140 ms per
  // evaluation, `profiles/r05_blk_*`).  Which wavefront takes which sample never mattered to the result.
  if (variant != 1 && blocks >= E && waves > 0) {
    const long wpe = blocks / E, per_round = wpe * waves;
    const long rounds = (num_local + per_round - 1) / per_round;
    const long need = (num_local + rounds * waves - 1) / (rounds * waves);
    // (only where it frees a fifth of the workgroups or more: 250 instead of 256 for one evaluation of 10 000 samples trades the
    //  ticket counter's slack for nothing -- 0.617 vs 0.598 ms)
    if (need >= 1 && need * 5 <= wpe * 4) blocks = (int)(need * E);
  }
  // r6: an evaluation that shares its launch with the other members of an ensemble (mcmc.hip sets the hint while it records) shares the
  // chip with them, too: 16 members x 20 evaluations x 8 workgroups were ten rounds of workgroups whose wavefronts drew two samples
  // each -- every workgroup ends on its slowest wavefront, a quarter of the kernel's time.  Four draws per wavefront there.
  if (ensemble_members_hint() > 1 && variant != 1 && blocks >= E && waves > 0) {
    const long tickets = 4;
    const long kb = std::max<long>(1, (num_local + tickets * waves - 1) / (tickets * waves));
    blocks = (int)std::min<long>(blocks, kb * E);
  }

  pl.G = G;
  pl.ntiles = ntiles;
  pl.variant = variant;
  pl.xlds = xlds;
  pl.far_frame = far_frame;
  pl.wide_frame = wide_frame;
  pl.small_lane = small_lane;
  pl.lane_kernel = lane_kernel;
  pl.waves = waves;
  pl.blocks = blocks;
  pl.shm = shm;
  pl.tr = tr;
  pl.num_lds_tiles = num_lds_tiles;
  pl.wide_lds_tiles = wide_lds_tiles;
  pl.pair_rows = (wide_dp || variant == 2 || (variant == 0 && mc::wide_eval(dp, xlds))) ? 1 : 0;
  pl.rec_head = rec_head;
  // A workgroup out of tickets moves on while the fullest evaluation has at least kStealWaves tickets per wavefront of the workgroup
  // left (mc::next_evaluation; the workgroup-per-sample kernel draws one ticket per workgroup).  Under the test switch the
  // evaluations other than the first have no workgroup of their own: every ticket left counts.
  if (steal_skew && !steal) throw Error(MOE_ERR_INVALID_VALUE, "MOE_KG_STEAL_SKEW=1 needs MOE_KG_STEAL=1", 0, 0, 0);
  pl.steal_min = !steal ? 0 : (steal_skew ? 1 : std::max(1, env_int("MOE_KG_STEAL_MIN_PER_WAVE", kStealWaves) * (variant == 1 ? 1 : waves)));
  pl.steal_skew = steal_skew ? 1 : 0;
  pl.multi_trial = (far_frame || small_lane) ? 0 : 1;
  // r6: the small shapes on the lane-parked kernel take their Armijo trials several per sweep, too -- each trial computed exactly as
  // a single-trial pass computes it (kg_mc.hpp eval_multi_exact: same bits as one trial per pass; MOE_KG_SMALL_MULTI=0: one per pass)
  if (small_lane && !far_frame && variant == 0 && lane_kernel && dp == 4 && small_multi) pl.multi_trial = 2;
  // the sample pre-pass (beta and the discretised-set winner of every sample, computed with the whole chip): for the
  // workgroup-per-sample kernel, where seven wavefronts would wait for one; the wave-per-sample kernel hides those loads
  // behind the other wavefront of its SIMD (measured: no difference at C3), so it only takes the pre-pass on request
  // (MOE_KG_PREP=1; MOE_KG_PREP=0: never); more components than lanes need it (thread-per-sample pre-pass)
  pl.prep = m > kMaxM || (prep_mode != 0 && (variant >= 1 || prep_mode == 1));
  pl.v_stride = (variant == 2) ? v_stride_tiles : k.N;
  pl.v_slots1 = (variant == 2) ? 1 + G : k.g1;
  // the weight table: N doubles per sample (1.28 GB per evaluation at C5); beyond its cap the samples compute their weights in the
  // kernel (workgroup-per-sample kernel only: the streamed-weights one is not chosen beyond the cap)
  pl.weight_table = variant >= 1 && pl.prep && 8.0 * (double)pl.v_stride * (double)num_local / 1e9 <= v_cap;  // (per evaluation, as above)
  if (variant == 2 && !(pl.weight_table && pl.prep))
    throw Error(MOE_ERR_RUNTIME, "streamed-weights MC kernel selected without its weight table");
  pl.chunk_len = tail_chunk_len(pl.fused_tail, m);
  // the start table: the LDS-table wave-per-sample kernels (lane-parked and frame line search) without derivative observations -- decided
  // by the evaluation's shape alone, like the kernel itself
  pl.start_table = variant == 0 && xlds && g == 0 && G == 0;
  return pl;
}

// table-row order of the dimensions: the GP's observed-derivative dimensions first (so derivative weight a multiplies row a), then
// the remaining dimensions in ascending order; padded rows map to themselves (their lengths are 0).  Frame of the coordinate tables.
TabParams table_rows(const GpDev& gp, const KgDims& k, int G, const double* Xq_all, const double* Xp, const double* disc_head) {
  const int d = k.d;
  TabParams tp;
  std::vector<int> order;
  std::vector<bool> used(kMaxDimPadded, false);
  for (int a = 0; a < k.g; ++a) {
    if (used[gp.derivs.idx[a]]) throw Error(MOE_ERR_INVALID_VALUE, "duplicate derivative index", gp.derivs.idx[a], 0, 0);
    order.push_back(gp.derivs.idx[a]);
    used[gp.derivs.idx[a]] = true;
  }
  for (int r = 0; r < kMaxDimPadded; ++r)  // derivative dims are < d <= dp, so rows [0, dp) are a permutation of [0, dp)
    if (!used[r]) order.push_back(r);
  if (k.dp < G) throw Error(MOE_ERR_RUNTIME, "padded dimension smaller than the derivative-slot count");
  for (int r = 0; r < kMaxDimPadded; ++r) {
    tp.perm[r] = order[r];
    // frame scale: the Matern kernel's sqrt(5) is folded into it (kg_mc.hpp radial3)
    tp.inv_lp[r] = gp.cp.inv_l[order[r]] * (gp.cp.type == MOE_COV_MATERN_NU_2P5 ? 2.236067977499789696409173668731276235 : 1.0);
    const double c = (order[r] < d) ? gp.x_mean[order[r]] : 0.0;  // training-set mean of the row's coordinate (0 for pad rows)
    tp.center[r] = c;
    // the MC kernels' exponent arithmetic covers |x - c| / l up to kTableExtent for every tabulated point
    if (order[r] < d) {
      const int kk = order[r];
      double ext = gp.x_ext[kk];
      for (int e = 0; e < k.E; ++e) {
        for (int i = 0; i < k.q; ++i) ext = std::max(ext, std::fabs(Xq_all[((size_t)e * k.q + i) * d + kk] - c));
      }
      for (int i = 0; i < k.p; ++i) ext = std::max(ext, std::fabs(Xp[(size_t)i * d + kk] - c));
      if (disc_head != nullptr)
        for (int i = 0; i < k.q; ++i) ext = std::max(ext, std::fabs(disc_head[(size_t)i * d + kk] - c));
      if (!(ext * tp.inv_lp[r] <= mc::kTableExtent))
        throw Error(MOE_ERR_BOUNDS, "length scale too small for the extent of the points (|x - mean| / length > 1e5)",
                    ext * tp.inv_lp[r], 0.0, mc::kTableExtent);
    }
  }
  return tp;
}

// The per-evaluation records in the host-side assembly area gp.hKgIn (it travels inside the state set-up's staging buffer): the host
// fills what it knows (discretised set, padded union points); mu, the factor of Var + noise, the discretised set's mu_n / c_j and the
// best posterior mean are written by kg_state_kernel.  Behind the records: [2 kMaxDimPadded] bounds | [kMaxDimPadded] frame centre |
// [kMaxDimPadded] frame scale, table-row order (the MC kernels read them one row per lane).
struct KgRecords {
  KgRec rec;
  int rec_bp = 0;              // offset of the best posterior mean
  size_t blob_size = 0, o_bounds = 0;
  unsigned int free_mask = 0;  // table-row order: the rows the inner optimisations move
};
KgRecords fill_records(GpDev& gp, const KgDims& k, const McPlan& pl, const TabParams& tp, const double* bounds,
                       const std::vector<double>& U_all, const std::vector<double>& disc_all) {
  const int m = k.m, A = k.A, size = k.size, d = k.d, dp = k.dp;
  KgRecords R;
  KgRec& rec = R.rec;
  int off = 0;
  auto take = [&](int cnt) {
    const int o = off;
    off += (cnt + 1) & ~1;
    return o;
  };
  rec.L = take(m * m);
  rec.mu_disc = take(A);
  rec.C_disc = take(A * m);
  rec.disc = take(A * size);
  if (off != pl.rec_head) throw Error(MOE_ERR_RUNTIME, "record head layout mismatch (lane-parked MC kernel)");
  rec.XuP = take(k.u * dp);
  R.rec_bp = take(1);
  rec.Mk = 0;
  rec.stride = off;
  R.blob_size = (size_t)rec.stride * k.E + 4 * kMaxDimPadded;
  R.o_bounds = (size_t)rec.stride * k.E;
  gp.hKgIn.reserve(R.blob_size);
  double* blob = gp.hKgIn.p;
  std::memset(blob, 0, sizeof(double) * R.blob_size);
  // (simplex inner domain, SimplexIntersectTensorProductDomain's constructor, gpp_domain.cpp:107-141: the box clipped to the unit
  //  hypercube; an empty intersection is the reference's BoundsException)
  std::vector<double> box(bounds, bounds + 2 * (size_t)size);
  if (k.simplex) {
    double corner_sum = 0.0;
    bool empty = false;
    for (int kk = 0; kk < size; ++kk) {
      box[2 * kk] = std::fmax(bounds[2 * kk], 0.0);
      box[2 * kk + 1] = std::fmin(bounds[2 * kk + 1], 1.0);
      empty = empty || box[2 * kk] > box[2 * kk + 1];
      corner_sum += box[2 * kk];
    }
    if (corner_sum >= 1.0 || empty)
      throw Error(MOE_ERR_BOUNDS,
                  "Simplex/Tensor product intersection is EMPTY; 'lower left' corner coordinate sum out of bounds or bounding "
                  "boxes do not intersect.",
                  corner_sum, 0.0, 1.0);
  }
  for (int r = 0; r < kMaxDimPadded; ++r) {  // bounds of row r = bounds of original dimension perm[r]
    const int kk = tp.perm[r];
    if (kk < size) {
      blob[R.o_bounds + 2 * r] = box[2 * kk];
      blob[R.o_bounds + 2 * r + 1] = box[2 * kk + 1];
      R.free_mask |= 1u << r;
    }
    blob[R.o_bounds + 2 * kMaxDimPadded + r] = tp.center[r];
    blob[R.o_bounds + 3 * kMaxDimPadded + r] = tp.inv_lp[r];
  }
  for (int e = 0; e < k.E; ++e) {
    const double* U = &U_all[(size_t)e * k.u * d];
    double* r = &blob[(size_t)rec.stride * e];
    std::copy(&disc_all[(size_t)e * A * size], &disc_all[(size_t)(e + 1) * A * size], r + rec.disc);
    for (int i = 0; i < k.u; ++i)
      for (int kk = 0; kk < d; ++kk) r[rec.XuP + (size_t)i * dp + kk] = U[(size_t)i * d + kk];
  }
  return R;
}

// the m x m algebra of the state, on the device (kg_state.hip): launched behind the state set-up, completing the records in place
KgStateParams launch_state_algebra(GpDev& gp, const KgDims& k, const KgStateEnqueued& se, const KgRecords& R, double* dBlobP,
                                   double best_so_far, hipStream_t s) {
  const int m = k.m, tri = m * (m + 1) / 2;
  gp.kStateI.reserve((size_t)2 * k.E);
  gp.kStateD.reserve((size_t)k.E * k.qd * (1 + (k.want_grad ? tri : 0)) + (size_t)k.E * (1 + k.qd + 3) + (size_t)k.E * tri);
  KgStateParams sp;
  sp.cp = gp.cp;
  sp.derivs = gp.derivs;
  for (int b = 0; b <= kMaxDerivs; ++b) sp.noise[b] = (b < k.g1) ? gp.noise[b] : 0.0;
  sp.mean = gp.mean;
  sp.best_so_far = best_so_far;
  sp.E = k.E;
  sp.u = k.u;
  sp.q = k.q;
  sp.m = m;
  sp.g = k.g;
  sp.d = k.d;
  sp.dp = k.dp;
  sp.A = k.A;
  sp.ng = k.ngrad;
  sp.gkk = se.gkk;
  sp.gx = se.gx;
  sp.gkk_slices = se.gkk_slices;
  sp.gx_slices = se.gx_slices;
  sp.ek = se.ek;
  sp.U = se.U;
  sp.extra = se.extra;
  sp.blob = dBlobP;
  sp.rec_stride = R.rec.stride;
  sp.rec_L = R.rec.L;
  sp.rec_mu_disc = R.rec.mu_disc;
  sp.rec_C_disc = R.rec.C_disc;
  sp.rec_bp = R.rec_bp;
  sp.flags = gp.kStateI.p;
  sp.winner = gp.kStateI.p + k.E;
  sp.gmu = gp.kStateD.p;
  sp.dL = gp.kStateD.p + (size_t)k.E * k.qd;
  launch_kg_state(sp, s);
  if (k.want_grad) launch_kg_dchol(sp, s);
  return sp;
}

// The MC step: its parameters, the sample pre-pass and the weight table where the plan has them, the MC kernel.
KgMcParams launch_mc_step(GpDev& gp, const KgDims& k, const McPlan& pl, const moe_gd_params_t& gd, const TabParams& tp,
                          const KgRecords& R, double* dBlobP, const double* dNormalsP, const BatchLayout& bl, long tab_stride,
                          size_t n_ctr, EventTimer& t_state, EventTimer& t_mc, hipStream_t s) {
  const int E = k.E, N = k.N, m = k.m, dp = k.dp, num_local = k.num_local;
  KgMcParams mp;
  mp.cov_type = gp.cp.type;
  mp.dim = k.d;
  mp.alpha = gp.cp.alpha;
  for (int r = 0; r < kMaxDimPadded; ++r) {
    mp.inv_lp[r] = tp.inv_lp[r];
    mp.perm[r] = tp.perm[r];
    mp.center[r] = tp.center[r];
  }
  mp.n = k.n;
  mp.g = k.g;
  mp.N = N;
  mp.u = k.u;
  mp.m = m;
  mp.f = k.f;
  mp.A = k.A;
  mp.ntiles = pl.ntiles;
  mp.E = E;
  mp.mean = gp.mean;
  mp.multi_trial = pl.multi_trial;
  mp.XsTab = gp.kTab.p;
  mp.tab_stride = tab_stride;
  mp.wide_lds_tiles = pl.wide_lds_tiles;
  mp.KinvY = gp.dKinvY.p;
  mp.W = gp.dWE.p + bl.col_kstar0(0) * N;
  mp.w_stride = (long)m * N;
  mp.blob = dBlobP;
  mp.rec = R.rec;
  mp.bounds = dBlobP + R.o_bounds;
  mp.free_mask = R.free_mask;
  mp.normals = dNormalsP;
  mp.first_sample = k.first_sample;
  mp.num_local = num_local;
  mp.max_num_steps = gd.max_num_steps;
  mp.max_num_restarts = gd.max_num_restarts;
  mp.gamma = gd.gamma;
  mp.pre_mult = gd.pre_mult;
  mp.max_relative_change = gd.max_relative_change;
  // (gpp_domain.cpp:245-247: the simplex update never lands precisely on a wall -- kRelativeChangeEpsilonTweak)
  if (k.simplex && mp.max_relative_change == 1.0) mp.max_relative_change -= 4.0 * 2.220446049250313e-16;
  mp.simplex = k.simplex ? 1 : 0;
  mp.inv_sqrt_size = 1.0 / std::sqrt((double)k.size);
  for (int r = 0; r < kMaxDimPadded; ++r) mp.inv_perm[r] = 0;
  for (int r = 0; r < kMaxDimPadded; ++r)
    if (tp.perm[r] >= 0 && tp.perm[r] < kMaxDimPadded) mp.inv_perm[tp.perm[r]] = r;
  mp.tolerance = gd.tolerance;
  mp.best_point = gp.kBestPoint.p;
  mp.best_value = gp.kBestValue.p;
  mp.beta = gp.kBeta.p;
  mp.counters = gp.kCounters.p;
  mp.next_sample = reinterpret_cast<unsigned int*>(gp.kCounters.p + (((size_t)2 * E + 15) / 16) * 16);  // 128-byte aligned
  mp.prof = gp.kCounters.p + n_ctr - 16;
  mp.best_j = nullptr;
  mp.V = nullptr;
  mp.v_stride = pl.v_stride;
  mp.v_slots1 = pl.v_slots1;
  mp.start_tab = nullptr;
  mp.start_stride = 0;
  mp.steal_min = pl.steal_min;
  mp.steal_skew = pl.steal_skew;
  if (pl.start_table) {  // the last kernel of the state phase: it reads the coordinate tables, K^-1 y, W and the records' discretised set
    mp.start_stride = (long)k.A * (1 + m) * (dp + 1);
    gp.kStartTab.reserve((size_t)mp.start_stride * E);
    double* start_tab_p = gp.kStartTab.p;
    launch_start_table(mp, dp, start_tab_p, s);
    mp.start_tab = start_tab_p;
  }
  t_state.stop(s);
  t_mc.start(s);
  const long total = (long)E * num_local;
  if (pl.prep) {
    gp.kBestJ.reserve((size_t)total);
    mp.best_j = gp.kBestJ.p;
    launch_sample_prep(mp, gp.kBestJ.p, gp.num_cu, s);
  }
  if (pl.weight_table) {  // (m > 64: the table kernel takes the columns of W 64 at a time, r4)
    gp.kV.reserve((size_t)mp.v_stride * (size_t)total + (size_t)64 * mp.v_slots1);  // (+ one tile: the sweeps prefetch one tile ahead)
    memset_async(gp.kBeta.p + (size_t)total * m, 0, sizeof(double) * 64, s);
    mp.V = gp.kV.p;
    launch_sample_weights(mp, gp.kV.p, s, pl.variant == 2);
  }
  if (pl.variant == 0 && pl.lane_kernel)
    launch_mc_lane(mp, dp, pl.G, pl.rec_head, pl.blocks, pl.waves, pl.shm, s);
  else if (pl.variant == 0)
    launch_mc(mp, dp, pl.G, pl.xlds, pl.blocks, pl.waves, pl.shm, s);
  else if (pl.variant == 2)
    launch_mc_stream(mp, dp, pl.G, pl.blocks, pl.waves, pl.shm, s);
  else
    launch_mc_block(mp, dp, pl.G, pl.tr, pl.num_lds_tiles, pl.blocks, pl.waves, s);
  t_mc.stop(s);
  return mp;
}

// The gradient tail (T-free for q-KG, else through the materialised N x M covariance matrix T), or the sum of the samples' values.
KgTailParams launch_tail_step(GpDev& gp, const KgDims& k, const McPlan& pl, const KgMcParams& mp, const KgRecords& R,
                              double* dBlobP, const double* dNormalsP, const BatchLayout& bl, double* dFin, int out_stride,
                              EventTimer& t_cov, EventTimer& t_tail, hipStream_t s) {
  const int E = k.E, N = k.N, n = k.n, m = k.m, num_local = k.num_local;
  KgTailParams tl;
  tl.cp = gp.cp;
  tl.derivs = gp.derivs;
  tl.u = k.u;
  tl.q = k.q;
  tl.m = m;
  tl.g = k.g;
  tl.N = N;
  tl.E = E;
  tl.num_local = num_local;
  tl.first_sample = k.first_sample;
  tl.ngrad = k.ngrad;
  tl.chunks = (num_local + pl.chunk_len - 1) / pl.chunk_len;
  tl.chunk_len = pl.chunk_len;
  tl.sw_chunk = ((long)E * num_local / kSwChunk >= 1024) ? kSwChunk : 16;
  tl.T = gp.kT.p;
  tl.SW = nullptr;
  tl.W = mp.W;
  tl.w_stride = mp.w_stride;
  tl.Gm = gp.dE.p + bl.col_grad0(0) * N;  // dK*/dXq itself: K^-1 goes onto the m columns of TB instead (launch_gtb)
  tl.g_stride = (long)k.ngrad * N;
  tl.Linv = gp.dLinv.p;
  tl.ldL = gp.ldL;
  tl.tri_work = gp.dEK.p;  // (reserved by enqueue_kg_state_batch; the state's own use of it is behind us in stream order)
  tl.work = gp.dVE.p;  // [2][N x E m]: enqueue_kg_state_batch reserves it; V = L^-1 K* is not needed any more
  tl.blob = dBlobP;
  tl.rec = R.rec;
  tl.rec_bp = R.rec_bp;
  tl.best_point = gp.kBestPoint.p;
  tl.best_value = gp.kBestValue.p;
  tl.beta = gp.kBeta.p;
  tl.normals = dNormalsP;
  tl.C = gp.kC.p;
  tl.TBpart = gp.kTB.p;
  tl.out = gp.kOut.p;
  tl.out_stride = out_stride;
  if (pl.fused_tail) {
    t_cov.start(s);
    t_cov.stop(s);  // no covariance matrix is built on this path
    t_tail.start(s);
    if (fused_tail_sw_free()) {  // no per-sample workspace: ZC comes from the chunk sums (kg_zc_direct_kernel)
      launch_fused_tail(tl, gp.dX.p, n, nullptr, 0, s);
    } else {
      const int slices = fused_tail_slices(E, num_local, n, gp.num_cu);
      gp.kSW.reserve((size_t)E * num_local * slices * 8);  // [E][num_local][slices][MU <= 8]
      launch_fused_tail(tl, gp.dX.p, n, gp.kSW.p, slices, s);
      gp.kZcPart.reserve((size_t)E * ((num_local + zc_chunk_len(m) - 1) / zc_chunk_len(m)) * m * m);
      launch_zc(tl, gp.kZcPart.p, s, !zc_sum_in_finish(m, num_local));
    }
  } else if (k.want_grad) {
    DerivList none;
    none.g = 0;
    for (int i = 0; i < kMaxDerivs; ++i) none.idx[i] = 0;
    t_cov.start(s);
    launch_cov_build(gp.cp, gp.dX.p, n, gp.derivs, gp.kBestPoint.p, E * num_local, none, nullptr, gp.kT.p, N, 0, s, true);
    t_cov.stop(s);
    t_tail.start(s);
    if (m > 8 || (size_t)N * m * sizeof(double) > 96 * 1024) {
      // S_W = W_e^T T_e per evaluation as a tile GEMM (the one-wave-per-sample loop re-reads W from L2 for every sample,
      // N m 8 bytes each -- fine for q-KG's m = q + p, prohibitive for d-KG's m = (q + p)(1 + g))
      gp.kSW.reserve((size_t)m * E * num_local);
      // A skinny output (m x samples) over a long K (N): every evaluation of the call in ONE launch, K cut into slices so that the chip
      // holds several workgroups per CU (r4: one launch per evaluation, unsplit below N = 2048, was 62 % of the d-KG tail at n = 500 --
      // 63 workgroups walking 125 dependent stages, eight times per call).  The slice count is a function of (m, N) alone.
      const int sw_slices = N >= 1024 ? 8 : (N >= 256 ? 4 : 1);  // (m > 64 too: the stretch point's 104 x 20 000 over N = 26 000 walked 1625 stages unsplit)
      if (sw_slices > 1) gp.kSWpart.reserve((size_t)sw_slices * m * num_local * E);
      if (m > 64 && sw_slices > 1) {  // (the kernel takes W / T / strides from `tl`)
        launch_sw128(tl, gp.kSWpart.p, sw_slices, gp.kSW.p, s);
      } else {
        launch_gemm_tn_splitk(m, num_local, N, tl.W, N, gp.kT.p, N, gp.kSW.p, gp.kSWpart.p, sw_slices, s, E, tl.w_stride, (long)num_local * N);
      }
      tl.SW = gp.kSW.p;
    }
    launch_tail(tl, s);
    // (r4: m > 64 too -- one workgroup per entry of ZC walking every sample with a stride of m doubles took 1.8 ms per evaluation at m = 104)
    gp.kZcPart.reserve((size_t)E * ((num_local + zc_chunk_len(m) - 1) / zc_chunk_len(m)) * m * m);
    launch_zc(tl, gp.kZcPart.p, s, !zc_sum_in_finish(m, num_local));
  } else {
    launch_kg_sum(tl, dFin, gp.kCounters.p, gp.kStateI.p, s);
  }
  MOE_HIP_CHECK(hipGetLastError());
  return tl;
}

// grad KG from the sample sums, on the device (kg_state.hip)
void launch_grad_finish(GpDev& gp, const KgDims& k, const KgStateParams& sp, const KgTailParams& tl, const KgRecords& R, double* dBlobP,
                        double* dFin, int out_stride, bool zc_direct, hipStream_t s) {
  const int m = k.m, num_local = k.num_local;
  KgFinishParams fp;
  fp.E = k.E;
  fp.q = k.q;
  fp.m = m;
  fp.g = k.g;
  fp.d = k.d;
  fp.ng = k.ngrad;
  fp.num_mc = k.num_mc;
  fp.first_sample = k.first_sample;
  fp.blob = dBlobP;
  fp.rec_stride = R.rec.stride;
  fp.rec_L = R.rec.L;
  fp.out = gp.kOut.p;
  fp.out_stride = out_stride;
  fp.winner = sp.winner;
  fp.gmu = sp.gmu;
  fp.dL = sp.dL;
  fp.fin = dFin;
  fp.counters = gp.kCounters.p;
  fp.flags = gp.kStateI.p;
  fp.dir_part = dir_partials(tl);
  fp.dir_slices = dir_slices(num_local);
  fp.zc_part = (!zc_direct && zc_sum_in_finish(m, num_local)) ? gp.kZcPart.p : nullptr;
  fp.zc_direct = zc_direct ? gp.kOut.p + 1 : nullptr;  // (kg_zc_direct_kernel left ZC itself there; kg_sum is still the finish kernel's)
  fp.zc_chunks = (num_local + zc_chunk_len(m) - 1) / zc_chunk_len(m);
  fp.zc_gs = zc_sum_lanes(m);
  fp.best_value = gp.kBestValue.p;
  fp.num_local = num_local;
  fp.rec_bp = R.rec_bp;
  launch_kg_finish(fp, dFin + (size_t)k.E * (1 + k.qd + 3), s);
}

// The results of one kg_launch through pinned memory, and the collect() that waits for them.
KgPending enqueue_results(GpDev& gp, const KgDims& k, const double* dFin, size_t n_ctr, bool want_best_points,
                          std::shared_ptr<std::array<EventTimer, 4>> timers, std::chrono::steady_clock::time_point wall0, hipStream_t s) {
  const int E = k.E, m = k.m, d = k.d, dp = k.dp, num_local = k.num_local, qd = k.qd;
  const bool want_grad = k.want_grad;
  // results through pinned memory in ONE copy: per evaluation kg_sum | grad_sum (q d) | value passes | gradient passes | flag
  const int fin_stride = (want_grad ? 1 + qd : 1) + 3;
  const size_t n_out = (size_t)fin_stride * E;
  gp.hKgOut.reserve(n_out);
  double* out = gp.hKgOut.p;
  copy_async(out, dFin, sizeof(double) * n_out, hipMemcpyDeviceToHost, s, true);  // (hKgOut: pinned)
#if MOE_BLOCK_PROF
  auto prof_p = std::make_shared<std::vector<unsigned long long>>(16);
  copy_async(prof_p->data(), gp.kCounters.p + n_ctr - 16, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost, s);
#endif
  const bool fetch_bp = want_best_points && E == 1;
  auto bp_p = std::make_shared<std::vector<double>>();
  if (fetch_bp) {
    bp_p->resize((size_t)num_local * dp);
    gp.kBestPoint.download(bp_p->data(), bp_p->size(), s);
  }
  GpDev* gpp = &gp;
  KgPending pending;
  pending.collect = [=](double* kg_sum, double* grad_sum, double* best_points, moe_kg_stats_t* stats) {
    GpDev& gp = *gpp;
    gp.use_device();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    MOE_HIP_CHECK(hipStreamSynchronize(s));
#if MOE_BLOCK_PROF
    {
      const unsigned long long* w = prof_p->data();
      const double tot = (double)(w[0] + w[1] + w[2] + w[3]);
      if (tot > 0 && w[8] > 0)
        std::fprintf(stderr,
                     "[moe prof] wave-0 cycles: ticket %.1f%%  z/beta/scan %.1f%%  weights %.1f%%  line search %.1f%%;  inside "
                     "%llu passes: accumulate %.0f  reduce %.0f  barrier %.0f  post %.0f  (cycles per pass; line search total "
                     "%.0f per pass)\n",
                     100.0 * w[0] / tot, 100.0 * w[1] / tot, 100.0 * w[2] / tot, 100.0 * w[3] / tot, w[8],
                     (double)w[4] / w[8], (double)w[5] / w[8], (double)w[6] / w[8], (double)w[7] / w[8], (double)w[3] / w[8]);
      if (w[10] > 0)
        std::fprintf(stderr, "[moe prof] gradient passes: %llu, %.0f cycles each (all phases); cycles per SAMPLE: total %.0f, in passes %.0f\n",
                     w[10], (double)w[9] / w[10], tot / (w[10] / 6.0), (double)(w[4] + w[5] + w[6] + w[7]) / (w[10] / 6.0));
      if (w[10] > 0)
        std::fprintf(stderr, "[moe prof] per sample: z/beta %.0f, scan %.0f cycles\n", (double)w[11] / (w[10] / 6.0), (double)w[12] / (w[10] / 6.0));
      if (w[10] > 0 && w[8] > 0)  // workgroup-per-sample kernel: line_search_lds outside its passes, per pass
        std::fprintf(stderr, "[moe prof] outside the passes, cycles per pass: gradient post + trial-line set-up %.0f, Armijo dispatch / decisions %.0f, "
                     "LimitUpdate + re-evaluation set-up + step end %.0f\n", (double)w[13] / w[8], (double)w[14] / w[8], (double)w[15] / w[8]);
      if (w[13] > 0 && w[10] == 0)  // wave-per-sample kernel (kg_mc_wave.hpp kg_sample): clock ticks of lane 0 of every wave
        std::fprintf(stderr,
                     "[moe prof] wave-per-sample kernel, ticks per sample: z/beta %.0f  weights %.0f  scan %.0f  line search %.0f "
                     "(of which %.1f value passes x %.0f + %.1f gradient passes x %.0f)\n",
                     (double)w[0] / w[13], (double)w[1] / w[13], (double)w[2] / w[13], (double)w[3] / w[13], (double)w[6] / w[13],
                     (double)w[4] / std::max<unsigned long long>(w[6], 1), (double)w[7] / w[13],
                     (double)w[5] / std::max<unsigned long long>(w[7], 1));
    }
#endif
    for (int e = 0; e < E; ++e)
      if (out[(size_t)fin_stride * (e + 1) - 1] != 0.0)
        throw Error(MOE_ERR_SINGULAR,
                    "GP-Variance matrix singular. Check for duplicate points_to_sample/being_sampled or "
                    "points_to_sample/being_sampled duplicating points_sampled with 0 noise.",
                    m, out[(size_t)fin_stride * (e + 1) - 1]);
    if (best_points && fetch_bp)
      for (int i = 0; i < num_local; ++i)
        for (int k = 0; k < d; ++k) best_points[(size_t)i * d + k] = (*bp_p)[(size_t)i * dp + k];

    for (int e = 0; e < E; ++e) {
      const double* o = &out[(size_t)fin_stride * e];
      kg_sum[e] = o[0];
      if (want_grad) std::copy(o + 1, o + 1 + qd, grad_sum + (size_t)e * qd);
      if (stats) {
        stats->posterior_mean_evals += (long long)o[fin_stride - 3];
        stats->posterior_grad_evals += (long long)o[fin_stride - 2];
      }
    }
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    const double ms_mc = (*timers)[0].ms(), ms_cov = want_grad ? (*timers)[1].ms() : 0.0,
                 ms_tail = want_grad ? (*timers)[2].ms() : 0.0;
    gp.last_ms[0] = ms_mc / E;
    gp.last_ms[1] = ms_cov / E;
    gp.last_ms[2] = ms_tail / E;
    const double ms_state = (*timers)[3].ms();
    gp.last_ms[3] = ms_state / E;
    gp.last_ms[4] = wall / E;
    if (stats) {
      stats->ms_state = ms_state;
      stats->ms_mc = ms_mc;
      stats->ms_tail = ms_cov + ms_tail;
    }
  };
  return pending;
}

}  // namespace

// Everything up to and including the asynchronous launches on gp.stream; the returned object's collect() waits for the
// stream and assembles the results.  Launching on several GPs (MCMC ensemble members, each with its own stream and
// workspaces) before collecting any of them overlaps one member's host algebra with the others' kernels.
KgPending kg_launch(GpDev& gp, int num_fidelity, const moe_gd_params_t& gd, const double* bounds, const double* discrete, int P,
                    const double* Xq_all, int num_evals, const double* Xp, int q, int p, int num_mc, double best_so_far,
                    const double* normals, int first_sample, int num_local, bool want_grad, bool want_best_points,
                    double weight_table_gb, const double* disc_head) {
  gp.use_device();
  hipStream_t s = gp.stream;
  const KgDims k = check_kg_args(gp, num_fidelity, gd, P, num_evals, q, p, num_mc, first_sample, num_local, want_grad);
  const int d = k.d, dp = k.dp, u = k.u, m = k.m, A = k.A, E = k.E, size = k.size, N = k.N, qd = k.qd;
  const McPlan pl = plan_mc(gp, k, bounds, Xq_all, Xp, weight_table_gb);

  const auto wall0 = std::chrono::steady_clock::now();

  // ---- 1. state set-up for the whole batch ----
  std::vector<double> U_all((size_t)E * u * d), extra_all((size_t)E * A * d), disc_all((size_t)E * A * size);
  for (int e = 0; e < E; ++e) {
    double* U = &U_all[(size_t)e * u * d];
    const double* Xq = Xq_all + (size_t)e * q * d;
    // union of points, discretised set = [Xu without fidelity dims ; discrete points]  (.cpp:246-261)
    std::copy(Xq, Xq + (size_t)q * d, U);
    if (p > 0) std::copy(Xp, Xp + (size_t)p * d, U + (size_t)q * d);
    double* ds = &disc_all[(size_t)e * A * size];
    // (disc_head: the state this evaluation runs on was BUILT at other points_to_sample and moved here with SetCurrentPoint,
    //  which leaves the discretised set behind -- .cpp:232-243 vs 259-261; the reference's multistart drivers do that)
    for (int i = 0; i < u; ++i) {
      const double* src = (disc_head != nullptr && i < q) ? disc_head + (size_t)i * d : U + (size_t)i * d;
      std::copy(src, src + size, ds + (size_t)i * size);
    }
    std::copy(discrete, discrete + (size_t)P * size, ds + (size_t)u * size);
    double* ex = &extra_all[(size_t)e * A * d];
    for (int j = 0; j < A; ++j) {
      for (int kk = 0; kk < size; ++kk) ex[(size_t)j * d + kk] = ds[(size_t)j * size + kk];
      for (int kk = size; kk < d; ++kk) ex[(size_t)j * d + kk] = 1.0;
    }
  }
  const TabParams tp = table_rows(gp, k, pl.G, Xq_all, Xp, disc_head);
  const KgRecords R = fill_records(gp, k, pl, tp, bounds, U_all, disc_all);
  const double* blob = gp.hKgIn.p;
  const size_t blob_size = R.blob_size;
  const long num_norm = (long)((num_mc + 1) / 2) * m;

  auto timers = std::make_shared<std::array<EventTimer, 4>>();
  EventTimer &t_mc = (*timers)[0], &t_cov = (*timers)[1], &t_tail = (*timers)[2], &t_state = (*timers)[3];
  t_state.start(s);
  // everything N-sized of the state, left on the device (gp.hip): no wait, no download -- the m x m algebra follows as kernels.
  // The records and the normal draws ride down in the same host->device copy as the points (r4: one copy per call instead of three).
  StateAppendix apx;
  apx.doubles = blob_size + (size_t)num_norm;
  apx.fill = [&](double* dst) {
    std::memcpy(dst, blob, sizeof(double) * blob_size);
    std::memcpy(dst + blob_size, normals, sizeof(double) * num_norm);
  };
  const KgStateEnqueued se = enqueue_kg_state_batch(gp, U_all.data(), u, want_grad ? q : 0, extra_all.data(), A, E, &apx);
  double* dBlobP = const_cast<double*>(gp.dAppendix);  // (kg_state_kernel completes the records in place)
  const double* dNormalsP = gp.dAppendix + blob_size;
  const KgStateParams sp = launch_state_algebra(gp, k, se, R, dBlobP, best_so_far, s);
  double* dFin = gp.kStateD.p + (size_t)E * qd * (1 + (want_grad ? m * (m + 1) / 2 : 0));

  // ---- device buffers ----
  const long tab_stride = (long)pl.ntiles * dp * 64;
  gp.kTab.reserve((size_t)tab_stride * E + (size_t)dp * 64);  // + one tile: eval_loop's last prefetch reads past the end
  gp.kBestPoint.reserve((size_t)E * num_local * dp);
  gp.kBestValue.reserve((size_t)E * num_local);
  gp.kBeta.reserve((size_t)E * num_local * m + 64);  // + a zeroed pad: kg_sample_weights_kernel reads whole 16/32/64-blocks
  // [2 E] pass counters | [E] sample-ticket counters, one 128-byte line each (kTicketStride unsigned ints)
  const size_t n_ctr = (size_t)2 * E + (size_t)E * (kTicketStride / 2) + 32;  // (+16 alignment slack, +16 profiling words)
  gp.kCounters.reserve(n_ctr);
  const int out_stride = 1 + m * m + 2 * k.ngrad;
  gp.kOut.reserve((size_t)out_stride * E);
  const bool sw_free = pl.fused_tail && fused_tail_sw_free();  // the T-free tail without its per-sample W^T T sums
  if (want_grad) {
    const int chunks = (num_local + pl.chunk_len - 1) / pl.chunk_len;
    if (!pl.fused_tail) gp.kT.reserve((size_t)N * E * num_local);
    if (!sw_free) gp.kC.reserve((size_t)E * num_local * m);
    // chunk partials + their sum + DIR partials + (S_W-free tail) KB chunk partials
    gp.kTB.reserve((size_t)E * (chunks + 1) * m * N + (size_t)E * k.ngrad * kDirSlices + (sw_free ? (size_t)E * chunks * m * m : 0));
  }

  // ---- coordinate tables ----
  launch_xs_tab(gp.dX.p, k.n, gp.dUnion, u, dp, pl.ntiles, tp, gp.kTab.p, tab_stride, pl.pair_rows, gp.kCounters.p, (long)n_ctr, E, s);

  // ---- 2. MC kernel (the start table in front of it closes the state phase) ----
  const KgMcParams mp = launch_mc_step(gp, k, pl, gd, tp, R, dBlobP, dNormalsP, se.bl, tab_stride, n_ctr, t_state, t_mc, s);
  {
    // (bits 1 / 2 of the second word, r4: the frame-extent decisions -- a domain box or point set wider than 100 length scales
    //  silently costs the LDS-table kernel and the multi-trial passes; this is where a caller can see it)
    const int info[8] = {pl.variant,
                         ((pl.variant == 0 && pl.xlds) ? 1 : 0) | (pl.far_frame ? 2 : 0) | (pl.wide_frame ? 4 : 0) | (pl.lane_kernel ? 8 : 0) |
                             (pl.start_table ? 16 : 0),
                         pl.waves, pl.variant == 1 ? pl.tr : pl.wide_lds_tiles, pl.weight_table ? 1 : 0, pl.fused_tail ? 1 : 0, pl.blocks,
                         pl.prep ? 1 : 0};
    std::copy(info, info + 8, gp.last_info);
    gp.last_moves = mp.prof + kMovesWord;
    gp.last_best_shape[0] = E;
    gp.last_best_shape[1] = k.num_local;
  }

  // ---- 3. gradient tail ----
  const KgTailParams tl = launch_tail_step(gp, k, pl, mp, R, dBlobP, dNormalsP, se.bl, dFin, out_stride, t_cov, t_tail, s);
  if (want_grad) {
    launch_grad_finish(gp, k, sp, tl, R, dBlobP, dFin, out_stride, sw_free, s);
    t_tail.stop(s);
  }
  return enqueue_results(gp, k, dFin, n_ctr, want_best_points, timers, wall0, s);
}

// How many evaluations one kg_launch may carry on this GP within `budget_gb` of device workspace (>= 1): the state
// matrices E / VE / WE, the materialised tail matrix T (d-KG and m > 8) with its TB partials, the per-sample outputs.
// A d-KG evaluation at C5 is 1.4 GB (N x M doubles of T alone), so a 200-start multistart cannot go down in one piece.
int kg_max_batch(const GpDev& gp, int P, int q, int p, int num_local, bool want_grad, double budget_gb) {
  const double N = gp.N, g1 = 1 + gp.g, u = q + p, m = u * g1, A = u + P;
  const double ngrad = want_grad ? q * g1 * gp.d : 0.0;
  const bool fused = fused_tail_taken(want_grad, gp.g, (int)m);
  const double chunks = std::ceil((double)num_local / tail_chunk_len(fused, (int)m));
  // state matrix E (all columns), V = L^-1 K* with the tail's K^-1 TB workspace behind it, W = K^-1 K*; the packed d chol / d Xq
  double doubles = N * (m + ngrad + A) + 3.0 * N * m + (double)num_local * (gp.dp + 1 + 2 * m) +
                   (want_grad ? (double)q * gp.d * m * (m + 1) / 2 : 0.0);
  if (want_grad) doubles += (fused ? 0.0 : N * (double)num_local) + (chunks + 1.0) * m * N;
  if (want_grad && !fused) doubles += 9.0 * m * (double)num_local;  // S_W = W^T T and its (up to eight) K slices
  // the per-sample weight table of the workgroup-per-sample / streamed-weights kernels (the latter: whole tiles, fantasy points included)
  // (always: whether an evaluation takes one of those kernels is decided per evaluation in kg_launch -- far frames send small
  //  q-KG shapes there too -- and the batch must fit whatever it decides)
  const double slots1 = gp.g <= 4 ? g1 : (gp.g <= 8 ? 9.0 : 13.0);  // (the streamed-weights table pads a point's weights to 1 + G)
  doubles += (gp.n + u + 64.0) * slots1 * (double)num_local;
  //  the split-K workspace of the state's triangular / Gram products (gp.dEK: ~8 N m per evaluation) and the evaluation's
  // share of the staging appendix (its record: L, mu_disc, C_disc, the discretised set, the padded union points)
  doubles += 8.0 * N * m + (m * m + A * (1.0 + m + gp.d) + u * gp.dp + 8.0);
  const double per_eval_gb = 8.0 * doubles / 1e9;
  return (int)std::max(1.0, std::floor(budget_gb / std::max(per_eval_gb, 1e-9)));
}

void kg_evaluate_batch(GpDev& gp, int num_fidelity, const moe_gd_params_t& gd, const double* bounds, const double* discrete,
                       int P, const double* Xq_all, int num_evals, const double* Xp, int q, int p, int num_mc,
                       double best_so_far, const double* normals, int first_sample, int num_local, bool want_grad,
                       double* kg_sum, double* grad_sum, double* best_points, moe_kg_stats_t* stats, const double* disc_head) {
  // batches beyond the workspace budget (MOE_KG_BATCH_GB, default 48) go down in pieces
  const double budget = (double)env_int("MOE_KG_BATCH_GB", 48);
  const int max_e = kg_max_batch(gp, P, q, p, num_local, want_grad, budget);
  if (num_evals <= max_e) {
    KgPending pending = kg_launch(gp, num_fidelity, gd, bounds, discrete, P, Xq_all, num_evals, Xp, q, p, num_mc, best_so_far,
                                  normals, first_sample, num_local, want_grad, best_points != nullptr, budget, disc_head);
    pending.collect(kg_sum, grad_sum, best_points, stats);
    return;
  }
  const size_t qd = (size_t)q * gp.d;
  moe_kg_stats_t total{}, part{};
  for (int e0 = 0; e0 < num_evals; e0 += max_e) {
    const int ne = std::min(max_e, num_evals - e0);
    KgPending pending = kg_launch(gp, num_fidelity, gd, bounds, discrete, P, Xq_all + (size_t)e0 * qd, ne, Xp, q, p, num_mc,
                                  best_so_far, normals, first_sample, num_local, want_grad, false, budget, disc_head);
    pending.collect(kg_sum + e0, grad_sum ? grad_sum + (size_t)e0 * qd : nullptr, nullptr, stats ? &part : nullptr);
    total.posterior_mean_evals += part.posterior_mean_evals;
    total.posterior_grad_evals += part.posterior_grad_evals;
    total.ms_state += part.ms_state;
    total.ms_mc += part.ms_mc;
    total.ms_tail += part.ms_tail;
  }
  if (stats) *stats = total;
}

}  // namespace moe
