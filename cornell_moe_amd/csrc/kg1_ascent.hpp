// cornell_moe_amd/csrc/kg1_ascent.hpp -- what the ensemble forms of the one-point acquisition functions share, declared here and
// compiled once in kg1_ascent.hip: the members' common checks, the staging of a call, the ensemble mean, the multistart ascent and
// the drivers behind the three shapes of entry point (evaluate at points, multistart, greedy batch).  None of it knows the
// objective; each client describes a call of its own in a Kg1Call (its Kg1Objective, what that points into, its members' check),
// and the entry points (api.hip) hand that to a driver.  The clients: kg1_opt.hip (the discretised knowledge gradient), ei1.hip
// (the analytic expected improvement), gibbon1.hip (the min-value entropy acquisition), cei1.hip (the constrained expected
// improvement, whose members are groups of 1 + K GPs combined by its own rule in the place of the ensemble mean), ehvi1.hip
// (the two-objective expected hypervolume improvement: groups of two GPs and a Pareto front per group), logcei1.hip (the log of
// the constrained expected improvement: cei1.hip's groups under a log-sum-exp, taken with groups of one GP too) and ehvi3.hip (the
// three-objective expected hypervolume improvement: groups of three GPs, a front and its box table per group) and cehvi1.hip (the
// constrained expected hypervolume improvement for two and for three objectives, the eighth and ninth client: groups of M + K GPs,
// ehvi1.hip's or ehvi3.hip's front and kernels over the objective GPs, times cei1.hip's probabilities of feasibility) and logehvi1.hip
// (the log of the two-objective constrained expected hypervolume improvement, the tenth: cehvi1.hip's groups and fronts under a
// log-sum-exp over the strips and over the members, taken with K = 0 too) and logehvi3.hip (the log of the three-objective one, the
// eleventh) and chebei1.hip (the Chebyshev-scalarised expected improvement for 2 to 8 objectives, the twelfth: groups of M GPs on
// ehvi1.hip's chain, a fixed quadrature per member, and a scalarisation and incumbents of its own for every point of a batch) and
// logchebei1.hip (the log of that with constraints, the thirteenth: groups of M + K GPs, a log-sum-exp over the quadrature's nodes
// and over the members) and logeipc1.hip (the log of the constrained expected improvement per unit cost, the fourteenth: logcei1.hip's
// groups with one more GP, of the log of the evaluation cost, whose role adds -alpha (mu + var / 2) to the member's log).
#pragma once
#include <memory>
#include <vector>

#include "gp.hpp"
#include "kg.hpp"

namespace moe {

constexpr int kMaxKept = 64;  // (one workgroup of 64 threads moves the kept starts; top_k_order keeps 20)

// where the parts of ascend()'s buffers lie (kg1_ascent.hip: stage_ascent() works them out, ascend() reads them)
struct Kg1AscentSizes {
  int Kmax, rows;
  bool want_path;
  size_t oVals, oX, oPath, nBack;
};

struct Kg1Objective;

// What the members of one call share: their layouts, the stream, and whether their chains are recorded and zipped.
struct Kg1Ensemble {
  // pending_room: the pending points the call will hold at most (the caller's and a greedy batch's picks)
  Kg1Ensemble(const std::vector<GpDev*>& members, const Kg1Objective& o, int pending_room);
  std::vector<GpDev*> gps;
  std::vector<Kg1Member> mem;
  hipStream_t z = nullptr;
  bool ens = false;
  int E = 0, d = 0, dp = 0, nf = 0;
  // a member's chain at C points in device memory, results left in its dKg / dGrad (recordable: launch.hpp)
  void (*eval_points)(const Kg1Member& m, const double* Px, const double* Ph, int C, bool with_grad, hipStream_t s) = nullptr;
  bool fid = false;
  // device addresses inside the first member's dStateIn (the one upload)
  const double* const* dKgTab = nullptr;
  const double* const* dGradTab = nullptr;
  const double* dBounds = nullptr;
  const double* dPts = nullptr;
  const double* dPtsH = nullptr;
  int* iFail = nullptr;  // [E] in the first member's kg1oI
  // pending points (kg1_pending.hip): p of pcap in use; with room for them the members' pending failure words [E] follow iFail, and
  // W = 2 E words travel where E do without
  int p = 0, pcap = 0, W = 0;
  double* dPending = nullptr;  // [pcap][dp] inside the one upload
  // an objective that combines the members itself (Kg1Objective::combine; NULL: the ensemble mean): its hook, the members per
  // group, the ascent's combined gradient [Kmax][d] behind the ascent's doubles and the one-entry table that names it
  void (*combine)(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) = nullptr;
  int group = 1;
  double* dComb = nullptr;
  const double* const* dCombTab = nullptr;
  // Kg1Objective::client, and with Kg1Objective::group_values the groups' own values [E / group][C] (C: the staged candidates) that
  // combine leaves whenever it forms the value: the objective's all_extended hook says where they lie
  const void* client = nullptr;
  bool group_values = false;
  int group_value_rows = 1;  // Kg1Objective::group_value_rows
  const double* dGroupVals = nullptr;
  Kg1AscentSizes sz = {};
};

// An objective as the staging and the drivers see it: a client names the fields it sets (the hooks but `member`, `eval_points` and
// `pick_appended` may stay NULL).
struct Kg1Objective {
  int nf = 0;                            // fidelity coordinates (0: one view of the points)
  const double* discrete_all = nullptr;  // the members' discrete sets back to back [sum A_e][d - nf]; NULL: the objective has none
  const int* num_discrete = nullptr;     // [E]: A_e
  const double* best_so_far = nullptr;   // [E]
  // member e's layout for at most C candidates and pcap pending points (fail, fail_pending: its failure words)
  Kg1Member (*member)(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending) = nullptr;
  // the member's chain (Kg1Ensemble::eval_points)
  void (*eval_points)(const Kg1Member& m, const double* Px, const double* Ph, int C, bool with_grad, hipStream_t s) = nullptr;
  // staging, once a member's extension by the caller's pending points stands ...
  void (*member_extended)(const Kg1Member& m, hipStream_t s) = nullptr;
  // ... and once every member's does: the first p of T.dPending are in use
  void (*all_extended)(Kg1Ensemble& T, int p) = nullptr;
  // a greedy batch has written its pick to row T.p of T.dPending: every member's extension takes it (T.p is raised afterwards)
  void (*pick_appended)(Kg1Ensemble& T) = nullptr;
  // num_member_extra doubles per member that travel in the call's one upload, behind the pending points: [E][num_member_extra];
  // member e's reach it as Kg1Member::dExtra / nExtra.  NULL: the objective has none and the upload is laid out without the block.
  const double* member_extra = nullptr;
  int num_member_extra = 0;
  // group > 1 and combine set: the E members are E / group groups of `group` consecutive members, and combine forms the ensemble's
  // value [C] and / or gradient [C][d] (either may be NULL) from the members' dKg / dGrad (T.dKgTab, T.dGradTab) on T.z, in the
  // place of the mean of the members.  With combine NULL or group <= 1 the drivers issue the launches they always did.
  int group = 0;
  void (*combine)(const Kg1Ensemble& T, int C, double* value_out, double* grad_out) = nullptr;
  // combine is taken with groups of ONE member too (group <= 1 reads as 1): an objective whose ensemble rule is no mean of the
  // members even where every member is one GP (logcei1.hip: a log-sum-exp).  false: the gate above stands, as every other client
  // relies on (cei1.hip with K = 0 is ei1.hip's launches).
  bool combine_single_groups = false;
  // what the objective's hooks need of the call beside the members (Kg1Ensemble::client); nothing here reads it
  const void* client = nullptr;
  // with combine: kg1_ensemble_evaluate's members_out is the groups' own values [E / group][C], taken from Kg1Ensemble::dGroupVals,
  // in the place of the members' [E][C]; with group_value_rows = R > 1 every group leaves R rows, [E / group][R][C] (cehvi1.hip:
  // the member's hypervolume term and its K feasibility factors)
  bool group_values = false;
  int group_value_rows = 1;
};

// One dim, one device, no member listed twice (MOE_ERR_INVALID_VALUE), behind num_fidelity < dim (MOE_ERR_BOUNDS); check_member:
// the objective's own check of member e, made before that member's duplicate check.
void kg1_check_members(const std::vector<GpDev*>& gps, int nf, void (*check_member)(const GpDev& g, const GpDev& g0, size_t e, int nf));

// A client's description of one call: the objective, the storage the objective points into (cei1.hip: the sub-members' limits,
// ehvi1.hip: its zeros and what its hooks need of the call) and the members' check -- one dim, one device, no member listed twice
// and the client's own conditions, with room for pending_room pending points (the caller's and a greedy batch's picks).
struct Kg1Call {
  Kg1Call() = default;
  Kg1Call(Kg1Call&&) = default;  // (moved, never copied: o points into the storage, which a move leaves where it is)
  Kg1Call& operator=(Kg1Call&&) = default;
  Kg1Objective o;
  std::vector<double> doubles;
  std::shared_ptr<const void> client;
  void (*check_members)(const Kg1Objective& o, const std::vector<GpDev*>& gps, int pending_room) = nullptr;
};
// The fourteen clients' descriptions, one function each (the caller has made the checks that need no handle; the arrays are the
// caller's and outlive the call).  gp.hpp says what the arguments are.
Kg1Call kg1_call(int num_fidelity, const double* discrete_all, const int* num_discrete, const double* best_so_far);  // kg1_opt.hip
Kg1Call ei1_call(const double* best_so_far);                                                                       // ei1.hip
Kg1Call gibbon1_call(const double* min_values, int num_min_values);                                                // gibbon1.hip
Kg1Call cei1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* best_so_far);         // cei1.hip
Kg1Call ehvi1_call(int num_mcmc, const double* reference_point, const double* front, int num_front);               // ehvi1.hip
Kg1Call logcei1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* best_so_far);      // logcei1.hip
Kg1Call ehvi3_call(int num_mcmc, const double* reference_point, const double* front, int num_front);              // ehvi3.hip
// (with num_constraints = 0 the two below return ehvi1_call / ehvi3_call themselves)
Kg1Call cehvi1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                    int num_front);  // cehvi1.hip
Kg1Call cehvi3_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                    int num_front);  // cehvi1.hip
// (K = 0 is taken by the log form itself)
Kg1Call logehvi1_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                      int num_front);  // logehvi1.hip
Kg1Call logehvi3_call(int num_mcmc, int num_constraints, const double* thresholds, const double* reference_point, const double* front,
                      int num_front);  // logehvi3.hip
// (scalarisations [num_rounds][2 M], best_so_far [num_rounds][E]; round 0 until a greedy batch's pick moves on to the next)
Kg1Call chebei1_call(int num_mcmc, int num_objectives, int num_rounds, const double* scalarisations,
                     const double* best_so_far);  // chebei1.hip
Kg1Call logchebei1_call(int num_mcmc, int num_objectives, int num_constraints, const double* thresholds, int num_rounds,
                        const double* scalarisations, const double* best_so_far);  // logchebei1.hip
// (members of 2 + K GPs: the objective, the K constraints, the GP of the log cost)
Kg1Call logeipc1_call(int num_mcmc, int num_constraints, const double* thresholds, double cost_exponent,
                      const double* best_so_far);  // logeipc1.hip

// what a multistart hands back (all but the first three may be NULL) ...
struct Kg1MultistartOut {
  double* best_point = nullptr;  // [d]
  double* best_value = nullptr;
  int* found = nullptr;
  double* start_values = nullptr;  // [S]
  int* kept_index = nullptr;       // [K]
  double* end_points = nullptr;    // [K][d]
  double* end_values = nullptr;    // [K]
  double* path = nullptr;          // [K][rows][d]
  int* steps_taken = nullptr;      // [K]
};
// ... and a greedy batch of q points
struct Kg1BatchOut {
  double* best_points = nullptr;  // [q][d]
  double* best_values = nullptr;  // [q]
  int* found = nullptr;           // [q]
};

// The drivers behind the three shapes of entry point (the members are checked: Kg1Call::check_members with num_pending, a batch
// with num_pending + num_to_sample - 1).  members_out (may be NULL): every member's own value [E][C], in the same copy back.
void kg1_ensemble_evaluate(const Kg1Objective& o, const std::vector<GpDev*>& gps, const double* pts, int C, bool want_grad,
                           double* value_out, double* grad_out, const double* pending, int num_pending, double* members_out);
void kg1_ensemble_multistart(const Kg1Objective& o, const std::vector<GpDev*>& gps, const moe_gd_params_t& outer,
                             const double* domain_bounds, const double* starts, int num_starts, int do_gradient_ascent,
                             const double* pending, int num_pending, const Kg1MultistartOut& out);
void kg1_ensemble_suggest(const Kg1Objective& o, const std::vector<GpDev*>& gps, const moe_gd_params_t& outer,
                          const double* domain_bounds, const double* starts, int num_starts, int do_gradient_ascent,
                          const double* pending, int num_pending, int num_to_sample, const Kg1BatchOut& out);

}  // namespace moe
