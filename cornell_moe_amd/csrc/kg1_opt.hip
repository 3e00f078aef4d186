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
// With pending points (kg1_pending.hip; moe_kg_discrete_mcmc_pending, moe_kg_discrete_mcmc_multistart_pending) the staging also builds
// every member's extension before its set phase; moe_kg_discrete_mcmc_suggest stages once and runs the ascent once per point of the
// batch, appending the picked point to every member's extension in between.
// The staging, the kernels of the mean, step and round phases, the recorded evaluation, the ascent and the drivers of the three entry
// points know nothing of the objective and are compiled once in kg1_ascent.hip (declared in kg1_ascent.hpp), which ei1.hip (the
// ensemble analytic expected improvement) and its relatives go through too; this file keeps what is the knowledge gradient's own:
// the description of the call (kg1_call: its sets, how a member is built, the set phase behind a member's extension, the members'
// check) and the check of the shapes that needs no handle.
//
// Bits.  A member's evaluation is kg1.hip's own kernels in kg1.hip's own pass structure, launched by itself or as the member's share of
// an ensemble twin: the same instructions on the same operands.  The mean adds the members in member order and divides once.  The
// step is the host's arithmetic one operation at a time with floating-point contraction switched off: alpha (std::pow on the host) *
// grad, the limiter's compares, x + step, the step's norm as a sequential sum.
#include "kg1_ascent.hpp"

namespace moe {

namespace {

void check_member(const GpDev& g, const GpDev&, size_t, int nf) { check_kg_discrete_member(g, nf); }

// (the row limit is the pending check's: a point is one row here)
void check_members(const Kg1Objective& o, const std::vector<GpDev*>& gps, int) { kg1_check_members(gps, o.nf, check_member); }

Kg1Member member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) {
  return kg1_member(gp, o.nf, o.num_discrete[e], C, o.best_so_far[e], with_grad, fail, pcap, fail_pending);
}

// a pick joins every member's extension and the rows under its set
void pick_appended(Kg1Ensemble& T) {
  for (Kg1Member& m : T.mem) kg1_pending_append(m, 1, true, T.z);
}

}  // namespace

// (begin -> append -> the set phase, member after member; nothing left once every extension stands)
Kg1Call kg1_call(int nf, const double* discrete_all, const int* num_discrete, const double* best_so_far) {
  Kg1Call call;
  call.o.nf = nf;
  call.o.discrete_all = discrete_all;
  call.o.num_discrete = num_discrete;
  call.o.best_so_far = best_so_far;
  call.o.member = member;
  call.o.eval_points = kg1_eval_points;
  call.o.member_extended = kg1_prepare_set;
  call.o.pick_appended = pick_appended;
  call.check_members = check_members;
  return call;
}

void check_kg_discrete_ensemble_shapes(int num_mcmc, int num_fidelity, const int* num_discrete, int num_points) {
  if (num_mcmc < 1 || num_mcmc > 1024) throw Error(MOE_ERR_BOUNDS, "num_mcmc must be between 1 and 1024", num_mcmc, 1, 1024);
  if (num_discrete == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL argument");
  for (int e = 0; e < num_mcmc; ++e) check_kg_discrete_shapes(0, num_discrete[e], 1);
  check_kg_discrete_shapes(num_fidelity, 1, num_points);  // (the number of points, then num_fidelity >= 0)
}

}  // namespace moe
