// cornell_moe_amd/csrc/kg1_opt.hip -- the exact discretised one-point knowledge gradient (kg1.hip) averaged over a hyper-parameter
// ensemble, and its multistart gradient ascent, on the device (moe_kg_discrete_mcmc, moe_kg_discrete_mcmc_multistart): "the next point
// under the ensemble" as examples/main.py asks gen_sample_from_qkg_mcmc for it, at q = 1 deterministic and in one call.
//
// For E members (each with its own sampled points, discrete set of A_e points and best value), one upload, ONE stream (the first
// member's), and these phases:
//   set, once    per member K(X, A_e), V_A = L^-1 K(X, A_e), a_A               kg1_prepare_set            never repeated in the call
//   evaluate     every member's chain of kg1.hip at points that are already    kg1_eval_points, recorded  one launch per kernel for
//                in device memory, results left in the member's buffers         once and replayed          all members (launch.hpp)
//   mean         sum over the members in member order, divided by E            kg1_mean_kernel
//   step         x += limit(alpha grad) for every kept start, in place         kg1_step_kernel            no wait between steps
//   round        |x_begin - x| > tolerance -> alive, count of alive starts     kg1_round_kernel           one 4-byte-per-word wait
// The ascent is multistart() / gradient_ascent() of multistart.hip operation for operation: value at every start, top_k_order on the
// host (the one wait of the screening), T steps per restart round with a stopped start evaluated and MASKED (a candidate's bits do not
// depend on who shares its pass), value at every end point, strict compare.
// With pending points (kg1_pending.hip; moe_kg_discrete_mcmc_pending, moe_kg_discrete_mcmc_multistart_pending) stage() also builds every
// member's extension before its set phase; moe_kg_discrete_mcmc_suggest stages once and runs the ascent (ascend()) once per point of
// the batch, appending the picked point to every member's extension in between.
// The kernels of the mean, step and round phases, the recorded evaluation and ascend() itself know nothing of the objective and live
// in kg1_ascent.hpp, which ei1.hip (the ensemble analytic expected improvement) includes too; this file keeps the staging, the set
// phase and the entry points.
//
// Bits.  A member's evaluation is kg1.hip's own kernels in kg1.hip's own pass structure, launched by itself or as the member's share of
// an ensemble twin: the same instructions on the same operands.  The mean adds the members in member order and divides once.  The
// step is the host's arithmetic one operation at a time with floating-point contraction switched off: alpha (std::pow on the host) *
// grad, the limiter's compares, x + step, the step's norm as a sequential sum.
#include "kg1_ascent.hpp"

namespace moe {

namespace {

void check_members(const std::vector<GpDev*>& gps, int nf) {
  const GpDev* g0 = gps[0];
  if (nf >= g0->d) throw Error(MOE_ERR_BOUNDS, "num_fidelity out of range", nf, 0, g0->d - 1);
  for (size_t e = 0; e < gps.size(); ++e) {
    const GpDev* g = gps[e];
    if (g->d != g0->d) throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share dim", g->d, g0->d, (double)e);
    if (g->device != g0->device)
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must live on one device", g->device, g0->device, (double)e);
  }
  for (size_t e = 0; e < gps.size(); ++e) {
    check_kg_discrete_member(*gps[e], nf);
    for (size_t f = 0; f < e; ++f)
      if (gps[f] == gps[e])
        throw Error(MOE_ERR_INVALID_VALUE, "an MCMC ensemble member is listed twice (every member keeps its own workspaces)", (double)e,
                    (double)f, 0);
  }
}

// The members' layouts and the one upload:
//   [kg pointers E | grad pointers E | bounds 2 d | set of member 0 .. E - 1, padded | points C dp | the same, fidelity 1 (fid)]
// extra_ints: integers of the caller behind the E failure words in the first member's kg1oI.
void stage(Kg1Ensemble& T, const std::vector<GpDev*>& gps, int nf, const double* discrete_all, const int* num_discrete,
           const double* best_so_far, const double* bounds, const double* pts, int C, bool with_grad, size_t extra_ints,
           const double* pending = nullptr, int p = 0, int pcap = 0) {
  GpDev& g0 = *gps[0];
  T.gps = gps;
  T.E = (int)gps.size();
  T.d = g0.d;
  T.dp = g0.dp;
  T.nf = nf;
  T.fid = nf > 0;
  g0.use_device();
  T.z = g0.stream;
  T.ens = ensemble_launches() && T.E > 1;
  const int E = T.E, d = T.d, dp = T.dp, size = d - nf;
  T.p = 0;
  T.pcap = pcap;
  T.W = pcap > 0 ? 2 * E : E;
  g0.kg1oI.reserve((size_t)T.W + extra_ints);
  T.iFail = g0.kg1oI.p;
  size_t nSets = 0;
  for (int e = 0; e < E; ++e) nSets += (size_t)num_discrete[e];
  const size_t nC = (size_t)C, oBounds = 2 * (size_t)E, oSets = oBounds + 2 * (size_t)d, oPts = oSets + nSets * dp;
  const size_t oPend = oPts + nC * dp * (T.fid ? 2 : 1);
  const size_t nIn = oPend + (size_t)pcap * dp;
  g0.hStateIn.reserve(nIn);
  g0.dStateIn.reserve(nIn);
  T.mem.clear();
  for (int e = 0; e < E; ++e) T.mem.push_back(kg1_member(*gps[e], nf, num_discrete[e], C, best_so_far[e], with_grad, T.iFail + e, pcap,
                                                         pcap > 0 ? T.iFail + E + e : nullptr));
  double* h = g0.hStateIn.p;
  static_assert(sizeof(const double*) == sizeof(double), "the pointer tables travel inside a buffer of doubles");
  for (int e = 0; e < E; ++e) {
    const double* pk = T.mem[e].dKg;
    const double* pg = T.mem[e].dGrad;
    std::memcpy(h + e, &pk, sizeof(pk));
    std::memcpy(h + E + e, &pg, sizeof(pg));
  }
  for (int k = 0; k < 2 * d; ++k) h[oBounds + k] = bounds != nullptr ? bounds[k] : 0.0;
  const double* dIn = g0.dStateIn.p;
  size_t row = 0;
  for (int e = 0; e < E; ++e) {
    T.mem[e].dPA = dIn + oSets + row * dp;
    for (size_t i = 0; i < (size_t)num_discrete[e]; ++i, ++row)
      for (int k = 0; k < dp; ++k) h[oSets + row * dp + k] = (k < size) ? discrete_all[row * size + k] : (k < d ? 1.0 : 0.0);
  }
  for (size_t i = 0; i < nC; ++i)
    for (int k = 0; k < dp; ++k) {
      const double v = (k < d) ? pts[i * d + k] : 0.0;
      h[oPts + i * dp + k] = v;
      if (T.fid) h[oPts + (nC + i) * dp + k] = (k >= size && k < d) ? 1.0 : v;
    }
  for (size_t i = 0; i < (size_t)pcap; ++i)  // (the pending points as given, fidelity coordinates included; the rest joins on the device)
    for (int k = 0; k < dp; ++k) h[oPend + i * dp + k] = (i < (size_t)p && k < d) ? pending[i * d + k] : 0.0;
  g0.dStateIn.upload(h, nIn, T.z, true);
  T.dPending = g0.dStateIn.p + oPend;
  T.dKgTab = reinterpret_cast<const double* const*>(dIn);
  T.dGradTab = reinterpret_cast<const double* const*>(dIn + E);
  T.dBounds = dIn + oBounds;
  T.dPts = dIn + oPts;
  T.dPtsH = T.fid ? T.dPts + nC * dp : T.dPts;
  kg1_clear_fail(T.iFail, E, T.z);
  if (pcap > 0) kg1_clear_fail(T.iFail + E, E, T.z);
  for (Kg1Member& m : T.mem) {
    if (pcap > 0) {
      m.dPP = T.dPending;
      kg1_pending_begin(m, T.z);
      if (p > 0) kg1_pending_append(m, p, false, T.z);
    }
    kg1_prepare_set(m, T.z);
  }
  T.p = p;
}


}  // namespace

void check_kg_discrete_ensemble_shapes(int num_mcmc, int num_fidelity, const int* num_discrete, int num_points) {
  if (num_mcmc < 1 || num_mcmc > 1024) throw Error(MOE_ERR_BOUNDS, "num_mcmc must be between 1 and 1024", num_mcmc, 1, 1024);
  if (num_discrete == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL argument");
  for (int e = 0; e < num_mcmc; ++e) check_kg_discrete_shapes(0, num_discrete[e], 1);
  check_kg_discrete_shapes(num_fidelity, 1, num_points);  // (the number of points, then num_fidelity >= 0)
}

void kg_discrete_mcmc_on_device(const std::vector<GpDev*>& gps, int nf, const double* discrete_all, const int* num_discrete,
                                const double* best_so_far, const double* pts, int C, bool want_grad, double* kg_out, double* grad_out,
                                const double* pending, int num_pending) {
  check_members(gps, nf);
  GpDev& g0 = *gps[0];
  Kg1Ensemble T;
  const int d = g0.d;
  const int E = num_pending > 0 ? 2 * (int)gps.size() : (int)gps.size();  // (the failure words in front of the results: Kg1Ensemble::W)
  // the call's doubles, all of them the copy back: [failure words | kg C | grad C d]
  const size_t nOut = (size_t)E + (size_t)C * (want_grad ? 1 + d : 1);
  g0.use_device();
  g0.kg1oD.reserve(nOut);
  g0.hStateOut.reserve(nOut);
  stage(T, gps, nf, discrete_all, num_discrete, best_so_far, nullptr, pts, C, want_grad, 0, pending, num_pending, num_pending);
  Kg1Recording rec;
  evaluate(T, rec, T.dPts, T.dPtsH, C, want_grad);
  double* dOut = g0.kg1oD.p;
  launch_mean_of_members(T, T.dKgTab, C, dOut + E);
  if (want_grad) launch_mean_of_members(T, T.dGradTab, (long)C * d, dOut + E + C);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, T.z, (const int*)T.iFail, E, dOut);
  MOE_HIP_CHECK(hipGetLastError());
  g0.kg1oD.download(g0.hStateOut.p, nOut, T.z);
  MOE_HIP_CHECK(hipStreamSynchronize(T.z));
  const double* o = g0.hStateOut.p;
  throw_if_singular(T, o);
  std::memcpy(kg_out, o + E, sizeof(double) * (size_t)C);
  if (want_grad) std::memcpy(grad_out, o + E + C, sizeof(double) * (size_t)C * d);
}

namespace {

// the buffers of ascend() and the one upload; pcap: room for pending points, the first p of them the caller's
void stage_ascent(Kg1Ensemble& T, const std::vector<GpDev*>& gps, int nf, const moe_gd_params_t& outer, const double* domain_bounds,
                  const double* discrete_all, const int* num_discrete, const double* best_so_far, const double* starts, int S,
                  bool ascent, bool want_path, const double* pending, int p, int pcap) {
  check_members(gps, nf);
  GpDev& g0 = *gps[0];
  const int E = (int)gps.size(), W = pcap > 0 ? 2 * E : E, d = g0.d, dp = g0.dp;
  const int R = std::max(outer.max_num_restarts, 0), Tn = outer.max_num_steps;
  const int Kmax = ascent ? std::min(S, kMaxKept) : 0;
  const size_t nBack = (size_t)W + Kmax + S + (size_t)Kmax * dp + (want_path ? (size_t)Kmax * (R * Tn + 1) * d : 0);
  g0.use_device();
  g0.kg1oD.reserve(nBack + 2 * (size_t)Kmax * dp);
  g0.hStateOut.reserve(nBack);
  // integers behind the failure words: [alive count | steps Kmax | order, running, alive Kmax each]
  stage(T, gps, nf, discrete_all, num_discrete, best_so_far, domain_bounds, starts, S, ascent && R > 0, 1 + 4 * (size_t)Kmax, pending, p,
        pcap);
}

}  // namespace

void kg_discrete_mcmc_multistart(const std::vector<GpDev*>& gps, int nf, const moe_gd_params_t& outer, const double* domain_bounds,
                                 const double* discrete_all, const int* num_discrete, const double* best_so_far,
                                 const double* starts, int num_starts, int do_gradient_ascent, double* best_point,
                                 double* best_value, int* found, double* start_values, int* kept_index, double* end_points,
                                 double* end_values, double* path, int* steps_taken, const double* pending, int num_pending) {
  Kg1Ensemble T;
  const bool ascent = do_gradient_ascent != 0;
  stage_ascent(T, gps, nf, outer, domain_bounds, discrete_all, num_discrete, best_so_far, starts, num_starts, ascent,
               ascent && path != nullptr, pending, num_pending, num_pending);
  ascend(T, outer, starts, num_starts, do_gradient_ascent, best_point, best_value, found, start_values, kept_index, end_points,
         end_values, path, steps_taken);
}

// q points greedily: round t is the ascent above with the caller's pending points and the t points already picked; the set phase
// runs once, a round appends one column to every member's extension and one row under its set.
void kg_discrete_mcmc_suggest(const std::vector<GpDev*>& gps, int nf, const moe_gd_params_t& outer, const double* domain_bounds,
                              const double* discrete_all, const int* num_discrete, const double* best_so_far, const double* starts,
                              int num_starts, int do_gradient_ascent, const double* pending, int num_pending, int num_to_sample,
                              double* best_points, double* best_values, int* found) {
  Kg1Ensemble T;
  stage_ascent(T, gps, nf, outer, domain_bounds, discrete_all, num_discrete, best_so_far, starts, num_starts, do_gradient_ascent != 0,
               false, pending, num_pending, num_pending + num_to_sample - 1);
  const int d = T.d;
  for (int t = 0; t < num_to_sample; ++t) {
    const double* dBest = ascend(T, outer, starts, num_starts, do_gradient_ascent, best_points + (size_t)t * d, best_values + t,
                                 found + t, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (t + 1 == num_to_sample) break;
    copy_async(T.dPending + (size_t)T.p * T.dp, dBest, sizeof(double) * (size_t)T.dp, hipMemcpyDeviceToDevice, T.z);
    for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, true, T.z);
    T.p += 1;
  }
}

}  // namespace moe
