// cornell_moe_amd/csrc/gp.hpp -- device-resident Gaussian process (the object behind moe_gp_t) and the per-call
// "points state" set-up shared by the posterior queries, q-EI and q-KG.
#pragma once
#include <cstdlib>
#include <functional>
#include <memory>
#include <vector>

#include "common.hpp"
#include "host_math.hpp"
#include "kernels.hpp"

namespace moe {

// Validated covariance parameters from [alpha, lengths[d]] (throws MOE_ERR_BOUNDS on non-positive entries).
void fill_cov_params(CovParams& cp, int cov_type, int d, const double* hyper);

// HBM-resident state of one GP (replaces GaussianProcess' K_chol_/K_inv_y_ members, gpp_math.hpp:840-868):
//   dX     [n][DP]   padded training points
//   dL     [N][N]    Cholesky factor of K + noise (lower; strict upper zero), column-major with leading dimension ldL
//   dLinv  [N][N]    its explicit inverse (lower), same layout
//   dKinvY [N]       K^-1 (y - mean)
struct GpDev {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side_stream = nullptr;  // early-inverse schedule of the build (kernels.hpp: launch_cholesky_and_inverse); taken on first need
  void release_side_streams();
  int d = 0, dp = 0, n = 0, g = 0, N = 0;
  long ldL = 0;  // leading dimension of dL / dLinv: N at the last rebuild + head-room for appended rows
  const double* zeroed_L = nullptr;  // the buffer / leading dimension dL's strict upper triangle was last cleared for (rebuild)
  long zeroed_ld = 0;
  CovParams cp;
  DerivList derivs;
  std::vector<double> X, y, noise;  // host copies (reference keeps them too, gpp_math.hpp:846-856)
  double mean = 0.0;
  DevBuf<double> dX, dL, dLinv, dKinvY, dNoise, dTmp;
  DevBuf<double> dVarWork;  // variance_on_device (dTmp keeps y - mean for the log likelihood)
  DevBuf<int> dInfo;
  // reusable workspaces for states
  DevBuf<double> dPts, dPtsGrad, dExtra, dE, dVE, dWE, dGram, dEK, dStateIn;
  // inside dStateIn after a state set-up: the padded union points of the batch [E][u][dp], and the caller's appendix (StateAppendix)
  const double* dUnion = nullptr;
  const double* dAppendix = nullptr;
  PinnedBuf<double> hStateIn, hStateOut, hKgIn, hKgOut;  // pinned staging for the per-call operands / results
  // the argument tables of ensemble-wide launches (mcmc.hip: replay_ensemble; held by the ensemble's first member)
  PinnedBuf<unsigned char> hEns;
  DevBuf<unsigned char> dEns;
  PinnedBuf<double> hYc;  // y - mean on its way to the device, and the factorisation's status word on its way back
  // reusable workspaces of the KG evaluator (kg.hip)
  DevBuf<double> kBlob, kNormals, kTab, kBestPoint, kBestValue, kBeta, kT, kC, kTB, kOut, kSW, kSWpart, kZcPart, kV;
  DevBuf<double> kStartTab;  // the start table of the line searches, [E][A][1 + m][dp + 1] (kg_prep.hip: kg_start_table_kernel)
  DevBuf<unsigned long long> kCounters;
  DevBuf<unsigned int> kEiTicket;  // arrival counters of ei_mc_kernel's fused final sum (ei.hip)
  bool ei_ticket_dirty = false;  // a launch of ei_mc_kernel was enqueued and its completion not yet seen: an aborted launch leaves
                                  // the arrival counters non-zero, so the next call clears them first
  DevBuf<int> kBestJ, kStateI;   // kStateI: singular flags | winners of a KG batch (kg_state.hip)
  DevBuf<double> kStateD;        // grad mu | d chol / d Xq (packed) | final [kg_sum | grad] per evaluation
  // joint posterior sampling (sample.hip): the candidate sets' covariances, then factors [E][C][C]; the draws [E][D][C] followed by
  // their argmin [E][D]; the factorisations' status words [E] and the resumed factorisations' [E]
  DevBuf<double> sMat, sOut;
  DevBuf<int> sInfo;
  // marginal mean / std and LCB selection (lcb.hip): the call's doubles (results first: one copy back) and integers
  DevBuf<double> lcbD;
  DevBuf<int> lcbI;
  // leave-one-out predictions and gradient (loo.hip): K^-1, the scaled columns B, M and the per-row vectors
  DevBuf<double> looD;
  // the discretised one-point knowledge gradient (kg1.hip): the call's doubles (results first: one copy back) and integers
  DevBuf<double> kg1D;
  DevBuf<int> kg1I;
  int kg1LastC = 0;  // the candidates kg1D was last laid out for (kg_discrete_last_active)
  // its ensemble forms (kg1_opt.hip; held by the ensemble's first member): the call's doubles (results first: one copy back) and
  // integers (the members' failure words first)
  DevBuf<double> kg1oD;
  DevBuf<int> kg1oI;
  // the expected hypervolume improvement (ehvi1.hip, ehvi3.hip; held by the ensemble's first member): the caller's front, the members' fronts
  // and their counts, the members' values and gradient coefficients
  DevBuf<double> ehviD;
  // the ensemble-averaged posterior mean and the recommendation (recommend.hip; held by the ensemble's first member): the call's
  // doubles (results first: one copy back) and the start indices
  DevBuf<double> recD;
  DevBuf<int> recI;
  // every member's posterior-mean minimiser (pm_members.hip; held by the ensemble's first member): the call's doubles (results
  // first: one copy back) and the start indices
  DevBuf<double> pmmD;
  DevBuf<int> pmmI;
  // posterior function paths (paths.hip; held by the ensemble's first member): the call's doubles (results first: one copy back,
  // the paths' v and its scratch last) and the start indices
  DevBuf<double> pathD;
  DevBuf<int> pathI;
  int num_cu = 256;
  // per-dimension mean and max |x - mean| of the training points (refreshed by rebuild() and by the append path of add_points):
  // the frame centre of the KG coordinate tables and the extent the kernel selection needs, so that an evaluation does not
  // re-walk the n x d coordinates on the host (r3, ADVICE)
  double x_mean[kMaxDimPadded] = {0}, x_ext[kMaxDimPadded] = {0};
  void refresh_extent();
  // timing of the last KG call (ms): mc, cov-build, tail contraction, state, total
  double last_ms[5] = {0, 0, 0, 0, 0};
  // which MC kernel the last KG launch took (moe_last_kernel_info): variant (0 wave-per-sample, 1 workgroup-per-sample) |
  // coordinate table in LDS | wavefronts per workgroup | register tiles per wavefront (variant 1) | streamed per-sample weight
  // table | T-free gradient tail | workgroups | sample pre-pass; bits 1 .. 4 of the second word: far frame | wide frame | lane-parked
  // kernel | the line searches took their first gradient from the start table
  int last_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // device word in which the last KG launch's MC kernel counted its workgroups' moves between evaluations (moe_last_kg_moves;
  // kg_mc.hpp next_evaluation), or NULL before the first launch
  const unsigned long long* last_moves = nullptr;
  // evaluations and samples per evaluation of the last KG launch: the shape of kBestPoint (moe_last_kg_best_points)
  int last_best_shape[2] = {0, 0};

  GpDev(const double* hyper, int cov_type, const double* X_in, const double* y_in, const double* noise_in,
        const int* derivs_in, int g_in, int d_in, int n_in, int device_in);
  ~GpDev();
  GpDev(const GpDev&) = delete;
  GpDev& operator=(const GpDev&) = delete;

  void use_device() const;
  void set_covariance(const double* hyper);  // alpha, lengths -> cp (validated)
  void rebuild();  // K assembly + Cholesky + inverse + K^-1 (y - mean)  (RecomputeDerivedVariables, gpp_math.cpp:481-511)
  // Appends k observations: a rank-k(1+g) block-row append to L and L^-1 while the head-room lasts (launch_cholesky_append),
  // the full rebuild otherwise.  (AddPointsToGP, gpp_math.cpp:1699-1737, always refactorises.)
  void add_points(const double* pts, const double* vals, int k);
  void add_points_unchecked(const double* pts, const double* vals, int k);
  void finish_factorisation();
  // New covariance hyper-parameters [alpha, lengths...] and noise [1 + g] on the same data: rebuild in place (buffers and
  // stream are kept) -- the inner step of hyper-parameter sampling (LogMarginalLikelihoodState::SetHyperparameters,
  // gpp_model_selection.cpp:798-811).
  void set_hyperparameters(const double* hyper, const double* noise_in);
  // log p(y | X, theta) of the current factorisation = -1/2 yc^T K^-1 yc - sum log L_ii - N/2 log 2 pi
  // (LogMarginalLikelihoodEvaluator::ComputeLogLikelihood, gpp_model_selection.cpp:593-612).
  double log_marginal_likelihood();
  // d log p / d [alpha, lengths[d], noise variances[1 + g]] of the current factorisation
  // (LogMarginalLikelihoodEvaluator::ComputeGradLogLikelihood, gpp_model_selection.cpp:629-677; with the reference's
  // Matern-5/2 convention that only the function-value block depends on the covariance hyper-parameters,
  // gpp_covariance.cpp:461-487).
  void grad_log_marginal_likelihood(double* grad);
  std::vector<double> padded(const double* pts, int k) const;  // [k][d] -> [k][DP]
  // Posterior mean of the function value at k points (one kernel, one copy each way): mu[k]; grad (may be NULL) [k][d].
  void mean_of_points(const double* pts, int k, double* mu, double* grad);
};

// Device-side product of a state set-up.  Columns of E (ld = N): see StateLayout.
struct StateDev {
  StateLayout lay;
  bool have_W = false;  // dWE = K^-1 E was computed (needed by the KG kernels)
};

// Builds E = [K*(X,U) | dK*/dU (first nd points) | K(X, extra)], VE = L^-1 E, optionally WE = L^-T VE, then
// gram = VE^T VE and ek = E^T K^-1(y-mean); downloads gram/ek into `host` (synchronises the GP's stream).
void compute_state(GpDev& gp, const double* U, int u, const DerivList& dt, int nd, const double* extra, int A, bool need_W,
                   StateDev* dev, StateHost* host);

// The same for `num_evals` independent point sets in one pass (the multistart axis): U_all[e][u][d], extra_all[e][A][d].
// Columns of E / VE / WE (ld = N) are grouped by kind so that every group is one launch:
//   [ K* of eval 0 | K* of eval 1 | ... | dK* of eval 0 | ... | extra of eval 0 | ... ]
// i.e. W_e = WE + col_kstar0(e) * N (m columns) and K^-1 dK*_e = WE + col_grad0(e) * N (ngrad columns).
struct BatchLayout {
  int E = 1, m = 0, ngrad = 0, A = 0;
  long col_kstar0(int e) const { return (long)e * m; }
  long col_grad0(int e) const { return (long)E * m + (long)e * ngrad; }
  long col_extra0(int e) const { return (long)E * (m + ngrad) + (long)e * A; }
  long total() const { return (long)E * (m + ngrad + A); }
};
// The device half of compute_state_batch -- uploads and kernels on gp.stream, NO sync: Gram matrices [E][c][c] followed by ek [ctot]
// are left in gp.dGram, the padded union points at gp.dUnion.  For callers that keep going on the device (ei.hip).
// Host operands of the CALLER that ride along in the state set-up's single host->device copy (r4: a q-EI evaluation made five
// copies of ~3 us each, a q-KG one seven): `doubles` doubles written by fill() into the pinned staging buffer behind the points;
// their device address afterwards is GpDev::dAppendix.
struct StateAppendix {
  size_t doubles = 0;
  std::function<void(double*)> fill;
};
struct StateEnqueued {
  BatchLayout bl;
  StateLayout lay;
  size_t nG = 0;   // doubles of Gram matrices in front of ek
  long ctot = 0;
  bool fused = false;  // small state, caller asked for it: neither the Gram matrices nor ek were formed -- V = L^-1 E (gp.dVE) and E
                       // (gp.dE) are left for a consumer that forms them itself (ei.hip: ei_state_kernel)
};
// whether a state of c columns over N rows is "small": its V and E columns fit the LDS of the workgroup that consumes them
inline bool state_fits_lds(int N, int c) { return c <= 48 && sizeof(double) * ((size_t)c * c + c + N + 2 * (size_t)c * N) <= 144 * 1024; }
StateEnqueued enqueue_state_batch(GpDev& gp, const double* U_all, int u, const DerivList& dt, int nd, const double* extra_all,
                                  int A, bool need_W, int num_evals, const StateAppendix* apx = nullptr,
                                  bool consumer_forms_gram = false);
// The KG evaluator's state set-up (r4), everything left on the device for kg_state.hip: see gp.hip.
struct KgStateEnqueued {
  BatchLayout bl;
  const double* gkk = nullptr;    // [E][m x m]              -- or, gkk_slices > 1: [E][gkk_slices][m x m] partial sums over K slices that
  const double* gx = nullptr;     // [E][(ngrad + A) x m]    --     the consumer adds up in slice order (r5, m <= 8: two launches less)
  int gkk_slices = 1, gx_slices = 1;
  const double* ek = nullptr;     // [E m | E ngrad | E A]
  const double* U = nullptr;      // [E][u][dp]
  const double* extra = nullptr;  // [E][A][dp]
};
KgStateEnqueued enqueue_kg_state_batch(GpDev& gp, const double* U_all, int u, int nd, const double* extra_all, int A, int num_evals,
                                       const StateAppendix* apx = nullptr);
void compute_state_batch(GpDev& gp, const double* U_all, int u, const DerivList& dt, int nd, const double* extra_all, int A,
                         bool need_W, int num_evals, BatchLayout* blay, std::vector<StateHost>* hosts);
// Variance (or its Cholesky factor) of k query points with the m x m algebra on the device: gp.hip.  For large query sets; small ones
// keep the host algebra.  Two thresholds in rows of the m x m variance: from kDeviceVarianceMinMPlain the variance itself is assembled
// on the device (both endpoints), from kDeviceVarianceMinM its factor too (below that the host's column sweep factors the downloaded
// variance).
constexpr int kDeviceVarianceMinM = 224;      // the factorisation on the device (r6: was 33; the blocked kernels cost 70 us before they do anything --
                                              // host sweep 287 us at 192 rows against 357, 536 at 256 against 277: profiles/r06_an_cholesky_variance_threshold.txt)
constexpr int kDeviceVarianceMinMPlain = 16;  // the variance on the device (r6: measured break-even, profiles/r06_am_variance_threshold.txt: at 32 rows 64 against 96 us)
// (MOE_GP_VARIANCE_DEVICE_MIN / MOE_GP_CHOL_VARIANCE_DEVICE_MIN: A/B runs of the thresholds, read per call; 1 = the device at every size)
inline int device_variance_min_m(bool cholesky) {
  const char* v = std::getenv(cholesky ? "MOE_GP_CHOL_VARIANCE_DEVICE_MIN" : "MOE_GP_VARIANCE_DEVICE_MIN");
  return (v && *v) ? std::atoi(v) : (cholesky ? kDeviceVarianceMinM : kDeviceVarianceMinMPlain);
}
void variance_on_device(GpDev& gp, const double* pts, int k, bool cholesky, double* out);
// Joint posterior sampling (SamplePointsFromGP, gpp_math.cpp:1800-1848) of E candidate sets of C points each, function values only.
// The value-only state of every set in one pass -- V = L^-1 K* through the per-problem triangular kernels, so that a set's bits do
// not depend on the batch it shares: gram = V^T V [E][C][C] followed by ek = K*^T K^-1 (y - mean) [E C] in gp.dGram; the padded
// points at gp.dUnion, the appendix at gp.dAppendix.  No sync.
void enqueue_sample_state_batch(GpDev& gp, const double* U_all, int C, int E, const StateAppendix* apx);
// sample.hip: values[E][D][C] = mu + L z for the D normal vectors normals[E][D][C] of each set, L the factor of the set's C x C
// posterior covariance; argmin[E][D] by the reference's rule (-1 when candidate 0 is the minimum); failed[E] = 0 or the failing
// pivot + 1.  stop_at_failure: ComputeCholeskyFactorL's early stop (gpp_linear_algebra.cpp:117-143) -- the partial factor with the
// trailing Schur complement in place is L; otherwise a failing pivot's column is zeroed and the factorisation goes on (the
// semidefinite continuation that comment names).
void sample_points_on_device(GpDev& gp, const double* pts, int C, int E, const double* normals, int D, bool stop_at_failure,
                             double* values, int* argmin, int* failed);
// lcb.hip: marginal posterior mean and standard deviation of the function value at C points, C x C never formed; a candidate whose
// variance fails the pivot rule (var > 1e-16) raises MOE_ERR_SINGULAR with payload (1, index of the first such candidate).
// Candidates go through in passes of lcb_pass_size(N, C), a function of (N, C) alone.
int lcb_pass_size(int N, int C);
void mean_std_on_device(GpDev& gp, const double* pts, int C, double* mean_out, double* std_out);
// lower_confidence_bound_optimization (cpp_wrappers/lower_confidence_bound.py) on the device; the GP is not modified.  index_out[q];
// points_out[q][d], mean_out[C], std_out[C], num_kept_out may be NULL.
void lcb_select_on_device(GpDev& gp, const double* pts, int C, int q, int* index_out, double* points_out, double* mean_out,
                          double* std_out, int* num_kept_out);
// kg1.hip: the exact discretised one-point knowledge gradient (moe_gp_kg_discrete) of C candidates [C][d] over A discrete points
// [A][d - num_fidelity]; grad_out [C][d] (want_grad) and nact_out [C] may be NULL.  check_kg_discrete_shapes: the limits that need no
// GP (MOE_ERR_BOUNDS).  Candidates go through in passes of kg1_pass_size(N, A).
int kg1_pass_size(int N, int A);
void check_kg_discrete_shapes(int num_fidelity, int A, int C);
void kg_discrete_on_device(GpDev& gp, int num_fidelity, const double* discrete, int A, const double* pts, int C, double best,
                           bool want_grad, double* kg_out, double* grad_out, int* nact_out);
// the number of lines on the envelope of each of the C candidates the GP last evaluated (alone or as a member of an ensemble call)
void kg_discrete_last_active(GpDev& gp, int C, int* nact_out);
// The same in the parts the ensemble forms (kg1_opt.hip) share with it.  Kg1Member: where one GP's set, per-pass scratch and
// results live for a call of at most C candidates -- everything inside the GP's own kg1D / kg1I (results first: [fail | kg C |
// active C | grad C d]), dE and dEK, so that the members of an ensemble never share a buffer.
struct Kg1Member {
  GpDev* gp = nullptr;
  int nf = 0, A = 0, n2 = 0, C = 0, per_pass = 0, widest = 0;
  bool with_grad = false, fid = false;
  double best = 0.0;
  const double* dPA = nullptr;  // the set [A][dp], fidelity coordinates 1 (the caller's upload)
  double *dOut = nullptr, *dKg = nullptr, *dAct = nullptr, *dGrad = nullptr;
  double *dVA = nullptr, *dAA = nullptr;  // V_A = L^-1 K(X, A) [N][A], a_A = mu_n(A)
  double *dVx = nullptr, *dVh = nullptr, *dT = nullptr, *dU = nullptr, *dMuh = nullptr, *dS2 = nullptr, *dB0 = nullptr, *dS = nullptr,
         *dHw = nullptr, *dScal = nullptr;
  int *iFail = nullptr, *iHid = nullptr;
  // pending points (kg1_pending.hip): the conditioned GP's pcap rows of room beside the member's own factor, p of them in use.  ld = N +
  // pcap is the leading dimension of V_A, V_x, V_x^, T and U: a column is [L^-1 k(X, z) ; r_z], the pending rows under the member's.
  // A member with g observed derivatives (ei1.hip only) counts ROWS here: a pending point is g1 = 1 + g rows, p and pcap multiples of g1.
  int p = 0, pcap = 0, ld = 0, g1 = 1;
  const double* dPP = nullptr;  // the pending points [pcap / g1][dp] (the caller's upload; rows past p filled as they are picked)
  double* dXe = nullptr;        // X u P, points [n + pcap / g1][dp]
  double* dKe = nullptr;        // [K^-1 (y - mean) ; 0]
  double* dVP = nullptr;        // column j [ld]: L^-1 k(X, P_j), then row j of L_P with its diagonal
  int* iFailP = nullptr;        // the first pending point whose Schur pivot fails the pivot rule
  double* dBp = nullptr;        // ei1.hip: the member's believed best b' = min(best, min_j mu(P_j)), in device memory
  const double* dExtra = nullptr;  // the objective's per-member block of the upload (gibbon1.hip: the member's min-values), [nExtra]
  int nExtra = 0;
  int role = 0;  // cei1.hip: 0 the objective GP of its member (best: the incumbent), k > 0 constraint k (best: its threshold)
  size_t out_doubles() const { return 1 + 2 * (size_t)C + (with_grad ? (size_t)C * gp->d : 0); }
};
// the handle's checks of moe_gp_kg_discrete (num_fidelity < dim, no derivative observations), the buffers and their layout; nothing
// is launched.  fail (may be NULL: the member's own word) is where a candidate failing the pivot rule leaves its index.
void check_kg_discrete_member(const GpDev& gp, int num_fidelity);
// pending_room > 0: room for that many pending points (fail_pending: where the first failing one leaves its index).
Kg1Member kg1_member(GpDev& gp, int num_fidelity, int A, int C, double best, bool with_grad, int* fail = nullptr,
                     int pending_room = 0, int* fail_pending = nullptr);
// op(L^-1) B for c columns, the kernel family fixed by the GP's N alone: a column's bits do not depend on c or the leading dimensions
void tri_cols(GpDev& gp, char op, int c, const double* B, long ldb, double* Cout, long ldc, hipStream_t s);
// kg1_pending.hip -- the posterior covariance conditioned on pending points, as an extension of at most kKg1MaxPending rows beside
// the member's factor (the handle is never modified, no (N + p)^2 matrix is formed):
//   kg1_pending_begin   X u P and [K^-1 (y - mean) ; 0] for the gradient's pass over the rows; m.dPP must be set, m.p becomes 0
//   kg1_pending_append  `count` more points of m.dPP join: L^-1 k(X, P_j), row j of L_P (pivot rule: m.iFailP), their rows of X u P;
//                       set_ready: the set's V_A gains their rows (otherwise kg1_prepare_set forms all of them)
//   kg1_pending_rows    rows i0 .. i1 - 1 of r_z = L_P^-1 (k(P, z) - V_P^T v_z) under the ncols columns V of the points Z [ncols][dp]
//   kg1_pending_back    u_P = L_P^-T t_P into m.dU and t -= V_P u_P on the member's rows of m.dT, for ncols columns
// With m.g1 = 1 + g > 1 (derivative observations; ei1.hip) a pending point is g1 extension rows and i0, i1 count rows: the limit is
// kKg1MaxPending ROWS.
constexpr int kKg1MaxPending = 64;
void kg1_pending_begin(Kg1Member& m, hipStream_t s);
void kg1_pending_append(Kg1Member& m, int count, bool set_ready, hipStream_t s);
void kg1_pending_rows(const Kg1Member& m, const double* Z, double* V, int ncols, int i0, int i1, hipStream_t s);
void kg1_pending_back(const Kg1Member& m, int ncols, hipStream_t s);
// "set, once": K(X, A), V_A, a_A on stream s (m.dPA must be set)
void kg1_prepare_set(const Kg1Member& m, hipStream_t s);
// nc <= m.widest candidates Px [nc][dp] (Ph: the same with fidelity coordinates 1; Px itself without fidelity) already on the
// device -> m.dKg / m.dAct / m.dGrad [c0 ..), on stream s.  No host memory is touched and nothing waits: every launch can be
// recorded (launch.hpp).  with_grad = false leaves the gradient out (the value's bits are the same).
void kg1_eval_pass(const Kg1Member& m, const double* Px, const double* Ph, int nc, int c0, bool with_grad, hipStream_t s);
// ... the same for C <= m.C candidates, pass after pass of m.per_pass
void kg1_eval_points(const Kg1Member& m, const double* Px, const double* Ph, int C, bool with_grad, hipStream_t s);
void kg1_clear_fail(int* fail, int count, hipStream_t s);  // INT_MAX: no candidate has failed
// The ensemble forms of the one-point acquisitions: evaluate at points, multistart ascent and greedy batches of each, with pending
// points [num_pending][dim] by the Kriging-believer fantasy of kg1_pending.hip.  Every client describes its call in one function
// (kg1_ascent.hpp: kg1_call, ei1_call, gibbon1_call, cei1_call, ehvi1_call, logcei1_call, ehvi3_call, cehvi1_call, cehvi3_call,
// logehvi1_call, logehvi3_call, chebei1_call, logchebei1_call, logeipc1_call) and the three drivers of kg1_ascent.hip run it; here are the checks that need no handle, which the entry points
// make first, and the limits.
// kg1_opt.hip: the discretised knowledge gradient (moe_kg_discrete_mcmc*).  discrete_all: the members' sets back to back.
void check_kg_discrete_ensemble_shapes(int num_mcmc, int num_fidelity, const int* num_discrete, int num_points);
// pending points (0: the launches of before) and num_to_sample points greedily, each round the ascent with the points picked so
// far appended to the pending ones
void check_kg_discrete_pending(const double* pending, int num_pending, int num_to_sample);
// ei1.hip: the analytic one-point expected improvement (moe_ei_analytic_mcmc*).  Candidates go through in passes of
// ei1_pass_size(N).  Members may carry derivative observations (one observed-derivative list for all of them): a pending point
// then believes its value and those derivatives, 1 + g rows, and (num_pending + num_to_sample - 1) (1 + g) <= kKg1MaxPending
// (MOE_ERR_BOUNDS after the handle checks).
int ei1_pass_size(int N);
void check_ei_analytic_mcmc_shapes(int num_mcmc, int num_points);
// gibbon1.hip: the min-value entropy acquisition GIBBON (moe_gibbon_mcmc*): ei1.hip's three with the members' samples of the
// minimum value min_values [E][num_min_values] in the place of best_so_far; the same pending points, passes, derivative-observing
// members and row limit.  check_gibbon_min_values: the count, then every value finite.
constexpr int kGibbonMaxMinValues = 1024;
void check_gibbon_min_values(const double* min_values, int num_mcmc, int num_min_values);
// cei1.hip: the constrained expected improvement (moe_ei_constrained_mcmc*): ei1.hip's three over members of 1 + K GPs each.  The
// GPs of a call [E (1 + K)] are the sub-members ordered [e][role], role 0 the objective GP, role k constraint k (satisfied where
// c_k <= thresholds[k - 1]); best_so_far [E] may hold +infinity.  check_ei_constrained_shapes: K, the product limit, the arrays
// K > 0 needs, finite thresholds, best_so_far neither NaN nor -infinity.  The members' own values of an evaluation are the
// sub-members' factor values [E (1 + K)][C].  logcei1.hip: the log of the same quantity (moe_log_ei_constrained_mcmc*), the same
// arguments, checks and limits; the members' own values are the sub-members' logs.
constexpr int kCeiMaxConstraints = 8;
void check_ei_constrained_shapes(int num_mcmc, int num_constraints, const void* constraint_gps, const double* thresholds,
                                 const double* best_so_far);
// ehvi1.hip: the two-objective expected hypervolume improvement (moe_ehvi_mcmc*): ei1.hip's three over members of two GPs each,
// the GPs of a call [2 E] ordered [e][objective], without derivative observations.  reference_point [2]; front [num_front][2]
// sorted by the first objective ascending, mutually non-dominated, strictly inside the reference point.  The members' own values
// of an evaluation are [E][C], every member's A_e.
constexpr int kEhviMaxFront = 960;
constexpr int kEhviMaxMembers = 512;
void check_ehvi_num_mcmc(int num_mcmc);
void check_ehvi_front(const double* reference_point, const double* front, int num_front);
// ehvi3.hip: the three-objective expected hypervolume improvement (moe_ehvi3_mcmc*): the same over members of three GPs each, the
// GPs of a call [3 E] ordered [e][objective].  reference_point [3]; front [num_front][3] in the canonical order (the third
// objective ascending, ties by the first, then by the second), mutually non-dominated, strictly inside the reference point.
constexpr int kEhvi3MaxFront = 192;
constexpr int kEhvi3MaxMembers = 341;
void check_ehvi3_num_mcmc(int num_mcmc);
void check_ehvi3_front(const double* reference_point, const double* front, int num_front);
// cehvi1.hip: the constrained expected hypervolume improvement (moe_ehvi_constrained_mcmc*, moe_ehvi3_constrained_mcmc*): the two
// above over members of M + K GPs each, the GPs of a call [E (M + K)] ordered [e][role], roles 0 .. M - 1 the objectives, role
// M - 1 + k constraint k (satisfied where c_k <= thresholds[k - 1]).  check_ehvi_constrained_shapes: K, the product limit, the
// arrays K > 0 needs, finite thresholds.  The groups' own values of an evaluation are [E][1 + K][C]: H_e, F_{e,1} .. F_{e,K}.
// logehvi1.hip: the log of the two-objective form (moe_log_ehvi_constrained_mcmc*), K = 0 included: the same arguments, checks and
// limits; the groups' own values are the logs L_e, log F_{e,1} .. log F_{e,K}.  logehvi3.hip: the log of the three-objective form
// (moe_log_ehvi3_constrained_mcmc*), likewise.
void check_ehvi_constrained_shapes(int num_objectives, int num_mcmc, int num_constraints, const void* constraint_gps,
                                   const double* thresholds);
// chebei1.hip: the Chebyshev-scalarised expected improvement (moe_ei_chebyshev_mcmc*): ei1.hip's three over members of M GPs each,
// 2 <= M <= 8, the GPs of a call [E M] ordered [e][objective], without derivative observations.  scalarisations [R][2 M] (a > 0,
// then b) and best_so_far [R][E], R = 1 but for a greedy batch, which takes one row per point.  check_chebei_objectives: M, then
// the product limit; check_chebei_values: every a, b and incumbent.  The members' own values of an evaluation are [E][C].
constexpr int kChebMinObjectives = 2;
constexpr int kChebMaxObjectives = 8;
void check_chebei_objectives(int num_objectives, int num_mcmc);
void check_chebei_values(int num_objectives, int num_mcmc, int num_rounds, const double* scalarisations, const double* best_so_far);
// logchebei1.hip: the log of the same with 0 <= K <= 8 constraints (moe_log_ei_chebyshev_constrained_mcmc*): members of M + K GPs
// each, the GPs of a call [E (M + K)] ordered [e][role], the objectives first.  check_logchebei_shapes: M, K, then the product
// limit; check_logchebei_values: every a, b, threshold and incumbent (all finite).  The groups' own values of an evaluation are
// [E][1 + K][C]: LA_e, log F_{e,1} .. log F_{e,K}.
void check_logchebei_shapes(int num_objectives, int num_constraints, int num_mcmc);
void check_logchebei_values(int num_objectives, int num_constraints, int num_mcmc, int num_rounds, const double* scalarisations,
                            const double* thresholds, const double* best_so_far);
// logeipc1.hip: the log of the constrained expected improvement per unit cost (moe_log_ei_per_cost_mcmc*): logcei1.hip's three over
// members of 2 + K GPs each, the GPs of a call [E (2 + K)] ordered [e][role], the last role a GP of the log of the evaluation cost;
// cost_exponent >= 0 (alpha).  check_log_ei_per_cost_shapes: K, the product limit E (2 + K) <= 1024, check_ei_constrained_shapes'
// remaining checks, then the exponent finite and not negative.  The members' own values of an evaluation are the sub-members'
// logs [E (2 + K)][C], the cost row last.
void check_log_ei_per_cost_shapes(int num_mcmc, int num_constraints, const void* constraint_gps, const double* thresholds,
                                  double cost_exponent, const double* best_so_far);
// loo.hip: leave-one-out cross-validation on the GP's current factorisation, every one of the N = n (1 + g) scalar observations left
// out by itself.  mean_out / var_out [n][1 + g]: the LOO predictive mean (function values in the caller's units) and variance.
void loo_predict_on_device(GpDev& gp, double* mean_out, double* var_out);
// d L_LOO / d [alpha, lengths[d], noise variances[1 + g]], the conventions of GpDev::grad_log_marginal_likelihood.
void grad_loo_log_likelihood(GpDev& gp, double* grad);
// what a member of an ensemble contributes to recommend.hip's and pm_members.hip's kernels: its covariance, K^-1 (y - mean)
// [n (1 + g)] and the constant mean; the members' records travel as a table in front of the call's other operands
struct PmMember {
  CovParams cp;
  const double* kinvy;
  double mean;
};
static_assert(sizeof(PmMember) % sizeof(double) == 0, "the member table travels inside a buffer of doubles");
// recommend.hip, for the ensemble calls below: the members `gps` must be non-NULL GPs of one dim, observed-derivative list, set of
// sampled points and device, and 0 <= num_fidelity < dim (MOE_ERR_BOUNDS / MOE_ERR_RUNTIME / MOE_ERR_INVALID_VALUE otherwise) ...
void check_pm_members(const std::vector<GpDev*>& gps, int num_fidelity);
// ... and the call's operands in the first member's pinned staging buffer hStateIn, one copy down: [member table (PmMember) | `rows` points [rows][d - num_fidelity] padded to dp, fidelity coordinates 1, padding 0 | room for `extra` doubles];
// returns the offset (in doubles) of the extras.
size_t stage_pm_inputs(const std::vector<GpDev*>& gps, int num_fidelity, const double* pts, size_t rows, size_t extra);
// recommend.hip: f(p) = -(1/E) sum_e mu_e(p, fidelity coordinates 1) and its gradient over the free coordinates at P points
// [P][d - num_fidelity], for the E members `gps` (same data, same device); value_out [P] / grad_out [P][d - num_fidelity] may be NULL.
void posterior_mean_mcmc_batch(const std::vector<GpDev*>& gps, int num_fidelity, const double* pts, int P, double* value_out,
                               double* grad_out);
// recommend.hip: screen C candidates, descend from the S best, pick, keep or fall back (moe_posterior_mean_mcmc_recommend); the
// caller has validated gd, C and S.
void posterior_mean_mcmc_recommend(const std::vector<GpDev*>& gps, int num_fidelity, const moe_gd_params_t& gd,
                                   const double* domain_bounds, const double* candidates, int C, int S, double* point_out,
                                   double* value_out, int* screened_index_out, int* refined_out, double* candidate_values_out,
                                   double* end_points_out, double* path_out);
// pm_members.hip: for every member by itself, screen its C candidates (candidates [C][size], or per_member [E][C][size]), run
// posterior_mean_optimize's line search from the best on the device, keep or fall back (moe_posterior_mean_members_minimize); the
// caller has validated gd and C.  means_out [E][C] and trace_out [E][restarts steps][size + 6] may be NULL.
void posterior_mean_members_minimize(const std::vector<GpDev*>& gps, int num_fidelity, const moe_gd_params_t& gd,
                                     const double* domain_bounds, const double* candidates, int C, bool per_member,
                                     double* best_points, double* best_values, int* start_index, int* fell_back, double* means_out,
                                     double* trace_out);
// pm_members.hip's selection for any table of rows: index[r] = numpy.argmin(values[r][0 .. C)), one workgroup per row
void launch_pmm_argmin(int rows, int C, const double* values, int* index, hipStream_t s);
// paths.hip: posterior function paths by pathwise conditioning and their minimisers (moe_gp_paths_evaluate, moe_gp_paths_minimize).
// frequencies [M][dim], phases [M], weights [E][S][M], noise_normals [E][S][n]; the members without derivative observations, of one
// dim, device, set of sampled points and cov_type (MOE_ERR_INVALID_VALUE otherwise).  check_paths_shapes: what needs no handle.
constexpr int kPathsMaxFeatures = 4096;
constexpr int kPathsMaxPaths = 1024;
void check_paths_shapes(int num_features, int num_paths, int num_mcmc);
// values [E][S][C]; grad [E][S][C][dim] (want_grad)
void paths_evaluate(const std::vector<GpDev*>& gps, const double* frequencies, const double* phases, int M, const double* weights,
                    const double* noise_normals, int S, const double* pts, int C, bool want_grad, double* values, double* grad);
// best_points [E][S][dim]; best_values / start_index / fell_back [E][S], screened_out [E][S][C] and trace_out
// [E S][restarts steps][dim + 6] may be NULL; the caller has validated gd and C.
void paths_minimize(const std::vector<GpDev*>& gps, const double* frequencies, const double* phases, int M, const double* weights,
                    const double* noise_normals, int S, const moe_gd_params_t& gd, const double* domain_bounds, const double* candidates,
                    int C, double* best_points, double* best_values, int* start_index, int* fell_back, double* screened_out,
                    double* trace_out);
// r6 (query_grad.hip): ComputeGradVarianceOfPoints / ComputeGradCholeskyVarianceOfPoints (gpp_math.cpp:1267-1474) for the first
// `num_derivs` of the `num_pts` points, the m x m x d algebra on the device: out[num_derivs][d m m] in the reference's layout.
void grad_variance_on_device(GpDev& gp, const double* pts, int num_pts, int num_derivs, bool cholesky, double* out);

}  // namespace moe
