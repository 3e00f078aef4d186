/* include/moe_hip.h -- public C ABI of libmoe_hip.so (MI355X / gfx950).
 *
 * A drop-in for the one hot path of wujian16/Cornell-MOE: GP posterior + Monte-Carlo acquisition (q-EI, q-KG, d-KG).
 * Each entry point states the reference interface it replaces (file:line under moe/optimal_learning/cpp/ of the
 * reference).  The reference crosses this boundary through a boost::python module (`moe.build.GPP`,
 * gpp_python.cpp:453-600); INTEGRATION.md shows the ctypes/pybind stub a maintainer would add to bind these symbols
 * instead.
 *
 * Conventions (identical to the reference's Python boundary, gpp_python_common.cpp:52-129):
 *   - all floating point is FP64; points are row-major [point][dim]; sizes are explicit ints;
 *   - all pointers are HOST pointers owned by the caller unless the name ends in `_dev`;
 *   - every function returns a status code (0 = ok) and, on failure, fills *err (may be NULL);
 *     codes map one-to-one onto the reference's exception classes (gpp_exception.hpp:144-509).
 *   - matrices returned to the caller are column-major exactly as the reference C++ fills them
 *     (the Python shim applies the same symmetrisation / transposition as gpp_python_gaussian_process.cpp:136-185).
 * There is NO CPU fallback: every compute entry point requires a visible gfx950 device and fails with
 * MOE_ERR_RUNTIME otherwise.
 *
 * SIZE LIMITS of the device kernels (the reference has none: gpp_knowledge_gradient_optimization.hpp:310-480 allocates by
 * size).  Beyond them the KG entry points return MOE_ERR_BOUNDS (payload: value, min, max) and compute nothing:
 *   - dim <= 32                       (coordinate tables are built for padded dimensions 4, 8, 12, 16, 24, 32);
 *   - num_derivatives <= 12           (derivative-weight slots of the d-KG Monte-Carlo kernels: 0..4, 8, 12);
 *   - (num_to_sample + num_being_sampled) * (1 + num_derivatives) <= 128   (m, the fantasy-observation count of one evaluation);
 *   - |x - mean(X)| / length <= 1e5 per coordinate for every tabulated point (32-bit exponent arithmetic of the table exp).
 * q,p-EI (moe_ei*): num_to_sample + num_being_sampled <= 64; up to 16 the whole evaluation stays on the device, beyond that its
 *   u x u algebra (variance, factor, Smith's derivative) runs on the host between two waits (r6; it was refused).
 * Every configuration BASELINE.json names is inside them (C5 with all 12 derivatives observed: m = 104).  The GP itself
 * (moe_gp_*, moe_ll_*) is limited by device memory only (N = 26 000 builds in 0.3 s; two N x N matrices stay resident).
 */
#ifndef MOE_HIP_H_
#define MOE_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

#define MOE_OK 0
#define MOE_ERR_RUNTIME 1        /* OptimalLearningException (gpp_exception.hpp:144) - also HIP runtime failures */
#define MOE_ERR_BOUNDS 2         /* BoundsException<T>(value, min, max)        (gpp_exception.hpp:260) */
#define MOE_ERR_INVALID_VALUE 3  /* InvalidValueException<T>(value, truth, tol) (gpp_exception.hpp:350) */
#define MOE_ERR_SINGULAR 4       /* SingularMatrixException(num_rows, leading_minor_index) (gpp_exception.hpp:440) */

#define MOE_COV_SQUARE_EXPONENTIAL 0 /* gpp_covariance.hpp:195 */
#define MOE_COV_MATERN_NU_2P5 1      /* gpp_covariance.hpp:313 (what the Python boundary always builds, gpp_python_gaussian_process.cpp:53) */

typedef struct moe_error {
  int code;
  char message[480];
  double payload[3]; /* Bounds: value,min,max; InvalidValue: value,truth,tolerance; Singular: num_rows,leading_minor_index,0 */
} moe_error_t;

/* GradientDescentParameters (gpp_optimizer_parameters.hpp:81-133) */
typedef struct moe_gd_params {
  int num_multistarts;
  int max_num_steps;
  int max_num_restarts;
  int num_steps_averaged;
  double gamma;
  double pre_mult;
  double max_relative_change;
  double tolerance;
  int domain_type; /* (r4) 0 = tensor-product domain, 1 = its intersection with the unit simplex {x_i >= 0, sum x_i <= 1}
                      (SimplexIntersectTensorProductDomain, gpp_domain.hpp:215-349; gpp_domain.cpp:234-290).  In the OUTER parameters
                      of a multistart driver: applied to each of the q points (RepeatedDomain).  In the INNER parameters of a KG
                      evaluation / driver and in moe_posterior_mean_optimize: the domain of every sample's posterior-mean
                      optimisation over the dim - num_fidelity free coordinates (the reference builds both of one type:
                      gpp_python_knowledge_gradient.cpp:279-296, 327-341; its single-evaluation entry points always pass a
                      tensor product: :97-144). */
} moe_gd_params_t;
#define MOE_DOMAIN_TENSOR_PRODUCT 0
#define MOE_DOMAIN_SIMPLEX 1

/* Counters the device fills during one KG evaluation (S and G must be counted on device). */
typedef struct moe_kg_stats {
  long long posterior_mean_evals; /* value-only passes over the N+m points made by the line search (all samples) */
  long long posterior_grad_evals; /* value+gradient passes */
  double ms_state;                /* wall ms: state set-up (K*, solves, Var, chol, grad chol) */
  double ms_mc;                   /* wall ms: MC inner-optimisation kernel */
  double ms_tail;                 /* wall ms: gradient tail (N x M covariance build + contraction) */
} moe_kg_stats_t;

typedef struct moe_gp moe_gp_t; /* opaque; replaces the heap GaussianProcess owned by the Python object
                                   (gpp_python_gaussian_process.cpp:55-61).  `const moe_gp_t*` means the GP it represents is
                                   not changed; every call works in the handle's own device workspaces, so calls on ONE handle
                                   are serialised by a per-handle mutex (calls on different handles run concurrently).
                                   NULL handles / NULL mandatory arguments return MOE_ERR_RUNTIME, never crash. */

/* ---- runtime ---- */
int moe_device_count(int* count);
/* "gfx950" etc. of device `device`; name_len >= 64. */
int moe_device_arch(int device, char* name, int name_len);
const char* moe_version(void);

/* ---- Gaussian process: GaussianProcess ctor (gpp_math.cpp:553-573, RecomputeDerivedVariables :481-511) ----
 * hyperparameters = [alpha, length_0 .. length_{d-1}] (gpp_python_common.cpp:100-105). K assembly, Cholesky,
 * triangular inverse and K^-1 (y - mean) run on device `device` and stay resident there.
 * Fails with MOE_ERR_SINGULAR (payload: N, leading minor index) when a pivot <= 1e-16 (gpp_linear_algebra.cpp:118). */
int moe_gp_create(const double* hyperparameters, int cov_type, const double* points_sampled,
                  const double* points_sampled_value, const double* noise_variance, const int* derivatives,
                  int num_derivatives, int dim, int num_sampled, int device, moe_gp_t** gp_out, moe_error_t* err);
int moe_gp_destroy(moe_gp_t* gp);
int moe_gp_dim(const moe_gp_t* gp);
int moe_gp_num_sampled(const moe_gp_t* gp);
int moe_gp_num_derivatives(const moe_gp_t* gp);
/* AddPointsToGP (gpp_math.cpp:1699-1718): appends points and re-derives everything (mean included). */
int moe_gp_add_points(moe_gp_t* gp, const double* new_points, const double* new_values, int num_new, moe_error_t* err);
/* Debug/parity accessors: K_chol [N*N col-major, lower triangle valid], K_inv_y [N], mean (any may be NULL). */
int moe_gp_get_factor(const moe_gp_t* gp, double* K_chol, double* K_inv_y, double* mean, moe_error_t* err);

/* ---- posterior queries; semantics of the Python-visible methods (gpp_python_gaussian_process.cpp:64-236) ----
 * m = num_pts * (1 + num_derivatives of the GP). */
/* compute_mean_of_points -> ComputeMeanOfPoints (gpp_math.cpp:662-678); out[num_pts] (function values only) */
int moe_gp_mean(const moe_gp_t* gp, const double* pts, int num_pts, double* out, moe_error_t* err);
/* compute_mean_of_additional_points -> ComputeMeanOfAdditionalPoints (gpp_math.cpp:688-710); out[num_pts] */
int moe_gp_additional_mean(const moe_gp_t* gp, const double* pts, int num_pts, double* out, moe_error_t* err);
/* compute_grad_mean_of_points -> ComputeGradMeanOfPoints (gpp_math.cpp:721-726); out[dim * m] */
int moe_gp_grad_mean(const moe_gp_t* gp, const double* pts, int num_pts, double* out, moe_error_t* err);
/* compute_variance_of_points -> ComputeVarianceOfPoints (gpp_math.cpp:924-970); out[m*m] col-major */
int moe_gp_variance(const moe_gp_t* gp, const double* pts, int num_pts, double* out, moe_error_t* err);
/* compute_cholesky_variance_of_points: chol of the above (lower; strict upper holds the variance leftovers exactly like
 * ComputeCholeskyFactorL leaves them); MOE_ERR_SINGULAR on failure */
int moe_gp_cholesky_variance(const moe_gp_t* gp, const double* pts, int num_pts, double* out, moe_error_t* err);
/* Joint posterior sampling -> GaussianProcess::SamplePointsFromGP (gpp_math.cpp:1800-1848), num_draws draws sharing one candidate
 * set and one factor.  Function values only, whatever derivatives the GP observes (the reference passes no derivative rows):
 *   values[num_draws][num_pts] = mu + L normals[d], L the Cholesky factor of the num_pts x num_pts posterior covariance;
 *   argmin[num_draws]: best = y[0], index -1, replaced on a strictly smaller value (so -1 when candidate 0 is the minimum);
 *   failed_pivot: 0, or the failing pivot + 1.  A failed factorisation is no error (the reference never raises here):
 *     reference quirks on (the default, moe_set_reference_quirks) -> ComputeCholeskyFactorL's early stop
 *     (gpp_linear_algebra.cpp:117-143): the columns before the pivot factored, the lower triangle of the trailing Schur
 *     complement in place, and that matrix is L;  quirks off -> the semidefinite continuation: the failing column is zeroed and
 *     the factorisation goes on.
 * MOE_ERR_BOUNDS only for num_pts <= 0 or num_draws <= 0.  No size limit beyond device memory: about
 * 8 (3 C^2 + 2 N C + 2 D C) bytes for C = num_pts candidates, D = num_draws and N = num_sampled (1 + num_derivatives)
 * (covariance / factor, Gram matrix, K* and L^-1 K*, normals and draws). */
int moe_gp_sample_points(const moe_gp_t* gp, const double* pts, int num_pts, const double* normals, int num_draws, double* values,
                         int* argmin, int* failed_pivot, moe_error_t* err);
/* GaussianProcess::SampleGlobalOptimaFromGP (gpp_math.cpp:1853-1870) on caller-drawn candidates: candidates[num_optima][inner_number][dim]
 * and normals[num_optima][inner_number], one draw per candidate set; all sets in one batch (one upload, one stream, one wait) and a
 * set's result does not depend on the others.  points_optima[num_optima][dim] = the set's candidate at its argmin; index[num_optima]
 * and failed_pivot[num_optima] as moe_gp_sample_points' argmin and failed_pivot.  DEVIATION: for an index of -1 the reference reads
 * before its candidate array (undefined behaviour); here the optimum is candidate 0 and index reports -1.  Bytes per set: as above
 * with D = 1. */
int moe_gp_sample_global_optima(const moe_gp_t* gp, const double* candidates, int inner_number, int num_optima, const double* normals,
                                double* points_optima, int* index, int* failed_pivot, moe_error_t* err);
/* Marginal posterior mean and standard deviation of the FUNCTION VALUE at each of num_candidates points, without the
 * num_candidates^2 covariance: mean_out[i] is what moe_gp_mean returns, std_out[i] = sqrt(var_i) with
 * var_i = k(c_i, c_i) - |L^-1 k*(c_i)|^2 over all N = num_sampled (1 + num_derivatives) training rows -- entry [0,0] of
 * moe_gp_cholesky_variance of that single point.  A candidate whose var fails the pivot rule (var > 1e-16,
 * gpp_linear_algebra.cpp:117-143) makes the call fail with MOE_ERR_SINGULAR, payload (1, index of the first such candidate):
 * what a loop of compute_cholesky_variance_of_points over the candidates raises there.
 * DEVIATION: with derivative observations the reference also factors the candidate's own derivative rows and can fail on one of
 * their pivots; those rows are not formed here.
 * No limit on num_candidates beyond memory: candidates go through in passes of moe_lcb_pass_size(N, num_candidates), a function
 * of those two numbers alone, and every kernel is chosen from them alone, so a candidate's bits do not depend on its neighbours.
 * MOE_ERR_BOUNDS for num_candidates < 1. */
int moe_gp_mean_std(const moe_gp_t* gp, const double* candidates, int num_candidates, double* mean_out, double* std_out,
                    moe_error_t* err);
int moe_lcb_pass_size(int num_rows, int num_candidates);
/* lower_confidence_bound_optimization (cpp_wrappers/lower_confidence_bound.py) on the device: one copy down, one wait, one copy
 * back, and the handle is NEVER modified (the reference appends its picks to the caller's GP; cornell_moe_amd's Python function of
 * the same name does that under reference quirks).
 *   1. mean, std as moe_gp_mean_std; target = mean - std, ucb = mean + std;
 *   2. index_out[0] = first index of min(target) (numpy argmin);
 *   3. kept set = {i : target_i <= min(ucb)} in candidate order, its size in *num_kept_out;
 *   4. for t = 1 .. num_to_sample - 1: the 1 + num_derivatives observation rows of candidate index_out[t-1] join the data with
 *      the GP's own noise variances (values play no part); index_out[t] = first index of the largest conditional std over the
 *      kept set.  A kept set smaller than num_to_sample re-picks points, as the reference does.
 * points_out[num_to_sample][dim] = the picked candidates; mean_out / std_out [num_candidates] (step 1's) -- each of the four
 * optional outputs may be NULL.
 * MOE_ERR_SINGULAR: a candidate failing step 1's pivot rule (payload as moe_gp_mean_std), or a conditioning block whose Schur
 * pivot is <= 1e-16 -- the reference's add_sampled_points raising on a noiseless duplicate (payload: rows of the extended matrix,
 * failing leading minor).
 * DEVIATIONS: the one of moe_gp_mean_std; the reference's SamplePoint carries a noise of 0.25 that its own add_sampled_points
 * ignores (gaussian_process.py:334-339 passes no noise on), so the GP's own noise applies here too; in the rounds a kept
 * candidate whose conditional variance has dropped to the pivot threshold or below (the noiseless pick itself) counts with
 * std = sqrt(max(var, 0)) where the reference's per-candidate factorisation would raise.
 * Limits: 1 <= num_to_sample <= 64 at every num_derivatives and dim <= 32, num_candidates >= 1 (MOE_ERR_BOUNDS otherwise).
 * Memory: 8 num_candidates (N + (num_to_sample - 1)(1 + num_derivatives) + 5) bytes besides a pass's K*. */
int moe_gp_lcb_select(const moe_gp_t* gp, const double* candidates, int num_candidates, int num_to_sample, int* index_out,
                      double* points_out, double* mean_out, double* std_out, int* num_kept_out, moe_error_t* err);
/* The exact discretised one-point knowledge gradient (Frazier, Powell & Dayanik 2009) of num_points candidates [dim] over ONE
 * discrete set of num_discrete points [dim - num_fidelity], for a GP WITHOUT derivative observations; no counterpart in the
 * reference's boundary (its knowledge gradient is Monte Carlo at every q).  With x^ = the candidate with its last num_fidelity
 * coordinates set to 1, the discrete points padded the same way, Z = {x^} u discrete, mu_n / Sigma_n the posterior mean (what
 * moe_gp_mean returns) and covariance and sigma^2 = noise_variance[0]:
 *   s^2(x) = Sigma_n(x, x) + sigma^2,  a_z = mu_n(z),  b_z(x) = Sigma_n(z, x) / s(x)
 *   kg[i] = min(best_so_far, mu_n(x^_i)) - E[min_{z in Z} (a_z + b_z(x_i) Z)],  Z ~ N(0, 1)
 * -- the fantasy of gpp_knowledge_gradient_optimization.cpp:83-107 / :298-316 conditioned on with noise sigma^2, evaluated
 * exactly: the lines are sorted by slope, the lower envelope is scanned, and the segments' normal probabilities are summed.  It is
 * a LOWER BOUND of the continuous knowledge gradient the Monte-Carlo evaluators estimate (their inner minimum runs over the
 * whole domain, not over Z).  grad[i][dim] (want_grad != 0) is the gradient in ALL dim coordinates of the candidate, exact by the
 * envelope theorem away from ties; num_active[i] (may be NULL) the number of lines on the envelope.  Among lines of equal slope
 * the smallest intercept survives and among exact duplicates the lowest index (x^ before the discrete points), so duplicates in
 * the set, x^ in the set and a permutation of the set leave every bit of kg unchanged; a candidate's bits do not depend on how
 * many candidates share the call (passes of moe_kg1_pass_size(N, num_discrete) candidates).
 * One copy down, one wait, one copy back; the handle is never modified.
 * Limits (MOE_ERR_BOUNDS, checked in this order before the device is touched): num_points >= 1; 1 <= num_discrete <= 4095 (the
 * num_discrete + 1 lines of a candidate are sorted in the LDS of one workgroup, 20 bytes each); num_fidelity >= 0; then, with the
 * handle: num_fidelity < dim; num_derivatives == 0 -- with derivative observations the fantasy has 1 + num_derivatives dimensions
 * and the quantity is not a minimum of lines (payload (num_derivatives, 0, 0)).
 * MOE_ERR_SINGULAR, payload (1, i): the first candidate i with s^2 <= 1e-16 (the pivot rule), reported after the wait.
 * Memory: 8 N num_discrete bytes for the set, and per pass 8 P (6 N + 2.5 num_discrete) bytes, P = the pass size. */
int moe_gp_kg_discrete(const moe_gp_t* gp, int num_fidelity, const double* discrete, int num_discrete, const double* points,
                       int num_points, double best_so_far, int want_grad, double* kg, double* grad, int* num_active,
                       moe_error_t* err);
int moe_kg1_pass_size(int num_rows, int num_discrete);
/* num_active[num_points]: the number of lines on the envelope of each candidate of the LAST discretised knowledge-gradient
 * evaluation this GP took part in (moe_gp_kg_discrete, or as a member of moe_kg_discrete_mcmc / moe_kg_discrete_mcmc_pending, which
 * have no such output), read back from the GP's workspace.  num_points must be that call's (MOE_ERR_BOUNDS, payload (num_points,
 * that call's, that call's)); a NULL handle or array -> MOE_ERR_RUNTIME. */
int moe_gp_kg_discrete_last_active(const moe_gp_t* gp, int num_points, int* num_active, moe_error_t* err);
/* moe_gp_kg_discrete averaged over an ensemble of num_mcmc GPs (one per hyper-parameter sample), every member e with its own
 * discrete set of num_discrete[e] points -- discrete_all holds the sets back to back, member e's [num_discrete[e]][dim -
 * num_fidelity] -- and its own best_so_far[e]:
 *   kg[i] = (KG_0(x_i) + KG_1(x_i) + ... + KG_{E-1}(x_i)) / E,  grad[i][dim] the same sum of the members' gradients
 * The members are added in member order and the sum is divided once; a member's term carries the bits moe_gp_kg_discrete returns
 * for it (the same kernels in the same passes), so the result is, bit for bit, the members' results added up on the host.
 * One copy down, one stream (the first member's), one wait, one copy back.  Every member's chain of kernels is recorded and each
 * kernel is launched once for all members where their launches line up (same N, same padded line count; moe_set_ensemble_launches,
 * counted in moe_ensemble_launch_stats), member after member otherwise: the same bits either way.
 * The members need NOT share their sampled points or their number; they share dim and the device, and none has derivative
 * observations.  No counterpart in the reference's boundary.
 * Errors, in this order, everything that needs no handle before a handle is touched: num_mcmc outside 1 .. 1024 -> MOE_ERR_BOUNDS;
 * a NULL array (gps, discrete_all, num_discrete, best_so_far, points, kg, grad with want_grad) -> MOE_ERR_RUNTIME; the first
 * num_discrete[e] outside 1 .. 4095 -> MOE_ERR_BOUNDS, payload (num_discrete[e], 1, 4095); num_points < 1 -> MOE_ERR_BOUNDS;
 * num_fidelity < 0 -> MOE_ERR_BOUNDS; a NULL handle -> MOE_ERR_RUNTIME; num_fidelity >= dim -> MOE_ERR_BOUNDS; a member of another
 * dim, then of another device -> MOE_ERR_INVALID_VALUE, payload (its value, the first member's, the member); a member with
 * derivative observations -> MOE_ERR_BOUNDS, payload (num_derivatives, 0, 0); a handle listed twice -> MOE_ERR_INVALID_VALUE (every
 * member keeps its own workspaces).
 * MOE_ERR_SINGULAR, payload (e, i): the first member e in which a candidate has s^2 <= 1e-16, and the first such candidate i of
 * that member; reported after the wait. */
int moe_kg_discrete_mcmc(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const double* discrete_all,
                         const int* num_discrete, const double* best_so_far, const double* points, int num_points, int want_grad,
                         double* kg, double* grad, moe_error_t* err);
/* One suggestion by the ensemble-averaged discretised knowledge gradient: the multistart gradient ascent of the drivers above
 * (MultistartOptimizer over GradientDescentOptimizer, gpp_optimization.hpp:619-705, 1472-1546) with moe_kg_discrete_mcmc's plain
 * ensemble mean as the objective, q = 1, and the whole loop on the device.  It has NO counterpart in the reference: no fidelity-cost
 * division, none of the KG-MCMC state behaviour moe_set_reference_quirks governs, and the objective is exact, not Monte Carlo.
 *   1. screening: the value at every start [num_starts][dim] (start_values, may be NULL); with do_gradient_ascent == 0 the best
 *      start by a strict compare in list order is returned (best_point seeded with the first start) and the outputs of 2. - 3. are
 *      left untouched.
 *   2. the K = min(20, num_starts) best starts are kept in the reference's order and tie rule (lowest kept value first, equal
 *      values by descending index; kept_index[K]); best_point is seeded with the first of them.
 *   3. ascent of all kept starts at once, R = max_num_restarts rounds of T = max_num_steps steps: with alpha_i = pre_mult
 *      (i + 1)^-gamma, step = alpha_i grad, limited per coordinate by TensorProductDomain::LimitUpdate (max_relative_change of the
 *      distance to the nearer bound; halved, or half-way to the bound, where it would leave the domain), x += step; a start stops
 *      for the round when |step| < tolerance / T and for good when a round moved it by no more than tolerance; the ascent ends
 *      when no start is left.  A stopped start is still evaluated and its update masked.
 *   4. the value at every end point (end_points[K][dim], end_values[K]); the first of the largest is returned (strict compare,
 *      against -infinity: found = 0 only if every value is NaN).
 * path (may be NULL): [K][R T + 1][dim], row 0 the start, row 1 + r T + i the point after step i of round r (a stopped start
 * repeats its point).  steps_taken[K]: the steps a start took while running.  All of these may be NULL.
 * The update is the host drivers' arithmetic operation for operation (no fused multiply-add), so the path is, bit for bit, the one
 * a host loop over moe_kg_discrete_mcmc walks.  The set phase (K(X, A_e), L^-1 K(X, A_e), mu_n(A_e)) runs once per member for the
 * whole call.  One copy down; the host waits once after the screening (it picks the kept starts), once per restart round (the count
 * of starts still alive) and once at the end.  Ensemble-wide launches as in moe_kg_discrete_mcmc, a step's recording made once and
 * issued every step.
 * Errors, in this order: those of moe_kg_discrete_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value
 * and found among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles.
 * MOE_ERR_SINGULAR, payload (e, i): member e, and the index i of the start (screening: into starts; later: into the kept starts)
 * whose s^2 <= 1e-16 at any step; reported at the next wait. */
int moe_kg_discrete_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* outer,
                                    const double* domain_bounds, const double* discrete_all, const int* num_discrete,
                                    const double* best_so_far, const double* starts, int num_starts, int do_gradient_ascent,
                                    double* best_point, double* best_value, int* found, double* start_values, int* kept_index,
                                    double* end_points, double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* moe_kg_discrete_mcmc with pending points: points_being_sampled [num_being_sampled][dim], FULL points with their fidelity
 * coordinates as given, whose experiments are running.  The posterior COVARIANCE of every member is conditioned on them (with the
 * member's noise sigma^2) and the posterior MEAN is left alone -- the Kriging-believer fantasy of Ginsbourger et al. 2008 (the
 * believed values are mu_n(P), so K'^-1 (y' - mean) = [K^-1 (y - mean) ; 0] exactly; the reference's docstrings still describe it,
 * gpp_python_expected_improvement.cpp:452-469).  With V_P = L^-1 k(X, P), L_P L_P^T = k(P, P) + sigma^2 I - V_P^T V_P and
 * r_z = L_P^-1 (k(P, z) - V_P^T v_z):
 *   Sigma(z, x | P) = k(z, x) - v_z . v_x - r_z . r_x
 * and kg / grad are moe_kg_discrete_mcmc's, word for word, with Sigma_n replaced by Sigma(. | P): s^2, the slopes, the tie rules,
 * best_so_far, x^'s line, the envelope-theorem gradient over the N + num_being_sampled rows (P does not move with x), the members
 * added in member order and divided once.  An ensemble of one is the single-GP form.
 * The pending rows are an extension of at most 64 rows beside each member's own factor: no handle is modified and no matrix of
 * N + num_being_sampled rows is formed.  A slope is one fused multiply-add chain over the member's rows in row order and then the
 * pending rows in order, the same chain for x^'s line and the set's, so the duplicate and tie rules of moe_gp_kg_discrete hold bit
 * for bit; a candidate's bits do not depend on how many share the call.  With num_being_sampled == 0 the call issues exactly the
 * kernels of moe_kg_discrete_mcmc and returns its bits.  One copy down, one wait, one copy back.
 * Errors, in this order: those of moe_kg_discrete_mcmc up to and including num_fidelity < 0; num_being_sampled outside 0 .. 64 ->
 * MOE_ERR_BOUNDS, payload (num_being_sampled, 0, 64); points_being_sampled NULL with num_being_sampled > 0 -> MOE_ERR_RUNTIME; all
 * of these before a handle is touched; then those of moe_kg_discrete_mcmc that need the handles.
 * MOE_ERR_SINGULAR after the wait: payload (e, j) with a message that names the pending point -- the first member e whose
 * extension has a Schur pivot <= 1e-16, and the first such pending point j (a noise-free member and a pending point repeating a
 * pending or sampled point); reported before, and otherwise as, moe_kg_discrete_mcmc's candidate case (payload (e, i), its text).
 * Memory: per member 8 (N + 64) (num_being_sampled + dim + 1) bytes besides moe_gp_kg_discrete's with N + num_being_sampled rows. */
int moe_kg_discrete_mcmc_pending(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const double* discrete_all,
                                 const int* num_discrete, const double* best_so_far, const double* points_being_sampled,
                                 int num_being_sampled, const double* points, int num_points, int want_grad, double* kg, double* grad,
                                 moe_error_t* err);
/* moe_kg_discrete_mcmc_multistart with moe_kg_discrete_mcmc_pending's objective: the same screening, top-20 rule, on-device step,
 * rounds, end values and optional outputs.  The extension is built once, before the set phase.  With num_being_sampled == 0 the
 * kernels and bits of moe_kg_discrete_mcmc_multistart.
 * Errors, in this order: those of moe_kg_discrete_mcmc_multistart up to and including num_fidelity < 0; num_being_sampled, then
 * points_being_sampled as above; max_num_steps; domain_type; then those that need the handles.  MOE_ERR_SINGULAR as above, at the
 * next wait; a candidate's payload as in moe_kg_discrete_mcmc_multistart. */
int moe_kg_discrete_mcmc_multistart_pending(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* outer,
                                            const double* domain_bounds, const double* discrete_all, const int* num_discrete,
                                            const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                            const double* starts, int num_starts, int do_gradient_ascent, double* best_point,
                                            double* best_value, int* found, double* start_values, int* kept_index,
                                            double* end_points, double* end_values, double* path, int* steps_taken,
                                            moe_error_t* err);
/* num_to_sample points greedily by the ensemble-averaged discretised knowledge gradient: round t = 0 .. num_to_sample - 1 is
 * moe_kg_discrete_mcmc_multistart_pending from the same starts [num_starts][dim] with pending points = points_being_sampled
 * followed by the points x_0 .. x_{t-1} of the rounds before, and writes best_points[t][dim], best_values[t], found[t]: bit for bit
 * what num_to_sample calls of that function return when each is fed its predecessors' points.
 * The set phase runs once per member for the whole call.  Round t >= 1 appends ONE row to each member's extension -- one triangular
 * product with one column, one row of L_P, one new row of r under the set's columns: O(N^2 + N num_discrete[e]), nothing is rebuilt
 * -- and the picked point reaches the extension inside device memory.  One copy down; the host waits as often as
 * moe_kg_discrete_mcmc_multistart does per round, and no more.
 * Errors, in this order: those of moe_kg_discrete_mcmc_multistart_pending, with, directly after num_being_sampled: num_to_sample
 * < 1 or num_being_sampled + num_to_sample - 1 > 64 -> MOE_ERR_BOUNDS, payload (num_to_sample, 1, 65 - num_being_sampled); and
 * best_points, best_values, found among the arrays that must not be NULL.  MOE_ERR_SINGULAR as above: the pending index counts the
 * caller's points first, then the rounds' picks. */
int moe_kg_discrete_mcmc_suggest(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* outer,
                                 const double* domain_bounds, const double* discrete_all, const int* num_discrete,
                                 const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                 const double* starts, int num_starts, int do_gradient_ascent, int num_to_sample, double* best_points,
                                 double* best_values, int* found, moe_error_t* err);
/* The analytic one-point expected improvement (OnePotentialSampleExpectedImprovementEvaluator, gpp_math.cpp:2195-2259) averaged over
 * an ensemble of num_mcmc GPs, with pending points, evaluated on the device: ei[i] and grad[i][dim] (want_grad != 0) at points
 * [num_points][dim].  Member e has posterior mean mu_e, noise sigma^2_e = noise_variance[0] and best value best_so_far[e]; its
 * posterior covariance of the latent function (no noise added to the variance) is conditioned on points_being_sampled
 * [num_being_sampled][dim] with sigma^2_e on their diagonal and its mean is left alone -- moe_kg_discrete_mcmc_pending's fantasy,
 * word for word: var_e(x) = k(x, x) - v_x . v_x - r_x . r_x.  The believed values join the incumbent,
 *   b'_e = min(best_so_far[e], min_j mu_e(P_j))        (b'_e = best_so_far[e] without pending points)
 * -- without this a greedy batch re-picks its own point, where var -> 0 and EI -> max(0, best - mu).  With t = b'_e - mu_e(x):
 *   EI_e = max(0, t Phi(c) + sigma phi(c)),  sigma = sqrt(max(DBL_MIN, var_e)),  c = t / sigma
 *   grad EI_e = -Phi(c_g) grad mu_e + phi(c_g) grad var_e / (2 sigma_g),  sigma_g = sqrt(max(150 eps^2, var_e)),  c_g = t / sigma_g
 * (the reference's two floors and its unclamped gradient; P and b' do not move with x), and
 *   ei[i] = (EI_0 + ... + EI_{E-1}) / E,  grad likewise: the members added in member order and divided once.
 * There is no fidelity handling (the reference's EI has none).  The gradient costs one transposed triangular product with ONE
 * column per candidate and one pass over the rows: 2 N^2 + O(N (num_being_sampled + dim)), not N^2 dim.
 * A candidate's bits do not depend on how many share the call (passes of moe_ei1_pass_size(N) candidates), nor on want_grad, nor on
 * ensemble-wide launches (moe_set_ensemble_launches); the ensemble's result is, bit for bit, the members' own results added up on
 * the host in member order.  With num_being_sampled == 0 (points_being_sampled may be NULL) no pending kernel is issued.  One copy
 * down, one stream (the first member's), one wait, one copy back; no handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_mcmc outside 1 .. 1024 ->
 * MOE_ERR_BOUNDS; a NULL array (gps, best_so_far, points, ei, grad with want_grad) -> MOE_ERR_RUNTIME; num_points < 1 ->
 * MOE_ERR_BOUNDS; num_being_sampled outside 0 .. 64 -> MOE_ERR_BOUNDS, payload (num_being_sampled, 0, 64); points_being_sampled NULL
 * with num_being_sampled > 0 -> MOE_ERR_RUNTIME; a NULL handle -> MOE_ERR_RUNTIME; a member of another dim, then of another device ->
 * MOE_ERR_INVALID_VALUE, payload (its value, the first member's, the member); a member whose observed-derivative list is not the
 * first member's -> MOE_ERR_INVALID_VALUE, payload (its num_derivatives, the first member's, the member); a handle listed twice ->
 * MOE_ERR_INVALID_VALUE; num_being_sampled (1 + g) > 64 -> MOE_ERR_BOUNDS, payload (num_being_sampled, 0, 64 / (1 + g) rounded down).
 * Derivative observations.  The members may observe g = num_derivatives partial derivatives at every sampled point (one list for
 * all members).  A pending experiment then returns its value AND those derivatives: P_j contributes 1 + g rows to the conditioned
 * covariance, row a with noise_variance[a] on its diagonal, all believed at the member's posterior means (so the mean is still left
 * alone); only the believed function value mu_e(P_j) joins b'_e.  The candidate is a function value.  The extension holds 64 ROWS:
 * num_being_sampled (1 + g) <= 64.  A member without derivative observations issues the launches it always did.
 * MOE_ERR_SINGULAR only for a pending point: payload (e, j), the first member e whose extension has a Schur pivot <= 1e-16 and the
 * first such pending point j; reported after the wait.  A candidate never raises: the two variance floors are the reference's. */
int moe_ei_analytic_mcmc(const moe_gp_t* const* gps, int num_mcmc, const double* best_so_far, const double* points_being_sampled,
                         int num_being_sampled, const double* points, int num_points, int want_grad, double* ei, double* grad,
                         moe_error_t* err);
/* The number of candidates per pass of the calls above and below: a function of the member's number of rows alone. */
int moe_ei1_pass_size(int num_rows);
/* One suggestion by moe_ei_analytic_mcmc's objective, q = 1, the whole loop on the device: moe_kg_discrete_mcmc_multistart_pending's
 * ascent (its kernels are shared), in the same words:
 *   1. screening: the value at every start [num_starts][dim] (start_values, may be NULL); with do_gradient_ascent == 0 the best
 *      start by a strict compare in list order is returned (best_point seeded with the first start) and the outputs of 2. - 3. are
 *      left untouched.
 *   2. the K = min(20, num_starts) best starts are kept in the reference's order and tie rule (lowest kept value first, equal
 *      values by descending index; kept_index[K]); best_point is seeded with the first of them.
 *   3. ascent of all kept starts at once, R = max_num_restarts rounds of T = max_num_steps steps: with alpha_i = pre_mult
 *      (i + 1)^-gamma, step = alpha_i grad, limited per coordinate by TensorProductDomain::LimitUpdate (max_relative_change of the
 *      distance to the nearer bound; halved, or half-way to the bound, where it would leave the domain), x += step; a start stops
 *      for the round when |step| < tolerance / T and for good when a round moved it by no more than tolerance; the ascent ends
 *      when no start is left.  A stopped start is still evaluated and its update masked.
 *   4. the value at every end point (end_points[K][dim], end_values[K]); the first of the largest is returned (strict compare,
 *      against -infinity: found = 0 only if every value is NaN).
 * path (may be NULL): [K][R T + 1][dim], row 0 the start, row 1 + r T + i the point after step i of round r (a stopped start
 * repeats its point).  steps_taken[K]: the steps a start took while running.  All of these may be NULL.
 * The update is the host drivers' arithmetic operation for operation (no fused multiply-add), so the path is, bit for bit, the one
 * a host loop over moe_ei_analytic_mcmc walks.  The extensions and the believed bests are built once.  One copy down; the host
 * waits once after the screening (it picks the kept starts), once per restart round (the count of starts still alive) and once at
 * the end.  Ensemble-wide launches as in moe_ei_analytic_mcmc, a step's recording made once and issued every step.
 * Errors, in this order: those of moe_ei_analytic_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value and
 * found among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles, the
 * row limit num_being_sampled (1 + g) <= 64 of members with g observed derivatives last.  MOE_ERR_SINGULAR as above, at the next
 * wait. */
int moe_ei_analytic_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, const moe_gd_params_t* outer, const double* domain_bounds,
                                    const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                    const double* starts, int num_starts, int do_gradient_ascent, double* best_point,
                                    double* best_value, int* found, double* start_values, int* kept_index, double* end_points,
                                    double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* num_to_sample points greedily: round t = 0 .. num_to_sample - 1 is moe_ei_analytic_mcmc_multistart from the same starts with
 * pending points = points_being_sampled followed by the picks x_0 .. x_{t-1} of the rounds before, and writes best_points[t][dim],
 * best_values[t], found[t]: bit for bit what num_to_sample calls of that function return when each is fed its predecessors' points.
 * Staged once; after round t ONE row (1 + g rows of a member with g observed derivatives) joins each member's extension and one value mu_e(x_t) its believed best, the pick reaching both
 * inside device memory.  The host waits as often as moe_kg_discrete_mcmc_suggest does, and no more.
 * Errors, in this order: those of moe_ei_analytic_mcmc_multistart, with, directly after num_being_sampled: num_to_sample < 1 or
 * num_being_sampled + num_to_sample - 1 > 64 -> MOE_ERR_BOUNDS, payload (num_to_sample, 1, 65 - num_being_sampled); and best_points,
 * best_values, found among the arrays that must not be NULL.  With g observed derivatives a round appends 1 + g rows, and after
 * the handle checks (num_being_sampled + num_to_sample - 1) (1 + g) > 64 -> MOE_ERR_BOUNDS, payload (num_being_sampled +
 * num_to_sample - 1, 0, 64 / (1 + g) rounded down).  MOE_ERR_SINGULAR as above: the pending index counts the caller's points first,
 * then the rounds' picks; it names the first point any of whose rows fails the pivot rule. */
int moe_ei_analytic_mcmc_suggest(const moe_gp_t* const* gps, int num_mcmc, const moe_gd_params_t* outer, const double* domain_bounds,
                                 const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                 const double* starts, int num_starts, int do_gradient_ascent, int num_to_sample, double* best_points,
                                 double* best_values, int* found, moe_error_t* err);
/* The min-value entropy acquisition GIBBON (Moss, Leslie, Gonzalez & Rayson, JMLR 2021: max-value entropy search, Wang & Jegelka
 * 2017, made right under observation noise and for batches) for minimisation, averaged over an ensemble of num_mcmc GPs, with
 * pending points, evaluated on the device: value[i] and grad[i][dim] (want_grad != 0) at points [num_points][dim].  Member e has
 * posterior mean mu_e, noise sigma^2 = noise_variance[0] and the caller's samples of the global minimum VALUE m_k = min_values[e][k],
 * k < num_min_values (for instance the minima of joint posterior draws at a candidate set, moe_gp_sample_points: an upper bound of the
 * domain minimum that tightens with the set).  Its covariance is conditioned on points_being_sampled as in moe_ei_analytic_mcmc, word
 * for word (the member's noise on their diagonal, the mean left alone, 1 + g rows per point under derivative observations).  With
 * var0 = k(x, x) - v_x . v_x the unconditioned and varc = var0 - r_x . r_x the conditioned variance of the latent function:
 *   s0 = max(DBL_MIN, var0),  sc = max(DBL_MIN, varc),  sigma0 = sqrt(s0),  rho^2 = s0 / (s0 + sigma^2),  gamma_k = (mu_e(x) - m_k) / sigma0
 *   r(gamma) = phi(gamma) / Phi(gamma) = sqrt(2 / pi) / erfcx(-gamma / sqrt 2),   q_k = clamp(r_k (gamma_k + r_k), 0, 1)
 *   G_k = -1/2 log1p(-min(rho^2 q_k, 1 - DBL_EPSILON))
 *   alpha_e = [num_being_sampled > 0] 1/2 (log(sc + sigma^2) - log(s0 + sigma^2)) + (1 / num_min_values) sum_k G_k
 *   value[i] = (alpha_0 + ... + alpha_{E-1}) / E,  grad likewise: the members added in member order and divided once.
 * 1 - rho^2 q is Var(y | f >= m) / Var(y) of the noisy observation; the bracket is the exact greedy increment of GIBBON's batch term
 * 1/2 log |R_B| (R: the correlation matrix of the batch's noisy predictive outputs), (varc + sigma^2) / (var0 + sigma^2) being the
 * Schur complement of x over its marginal.  It tends to -infinity at a noise-free pending point: unlike plain max-value entropy
 * search, whose value depends on gamma alone, a greedy batch does not re-pick its own point.  gamma and rho^2 take the unconditioned
 * moments and the min-values stay fixed over the batch.
 * The gradient is unclamped, P and m do not move with x, and max(150 eps^2, .) replaces both floors in its denominators and in the
 * gamma and rho^2 of its factors (moe_ei_analytic_mcmc's second floor); it costs one transposed triangular product with ONE column per
 * candidate, the kernels being moe_ei_analytic_mcmc's.
 * Bits as in moe_ei_analytic_mcmc: a candidate's do not depend on how many share the call (passes of moe_ei1_pass_size(N)), on
 * want_grad or on ensemble-wide launches; the ensemble's result is the members' own added on the host in member order; the terms
 * are added in a fixed shape (lane l of 64 takes k = l, l + 64, ..., then a butterfly).  The min-values travel in the call's one
 * upload.  One copy down, one stream, one wait, one copy back; no handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_mcmc outside 1 .. 1024 ->
 * MOE_ERR_BOUNDS; a NULL array (gps, min_values, points, value, grad with want_grad) -> MOE_ERR_RUNTIME; num_min_values outside
 * 1 .. 1024 -> MOE_ERR_BOUNDS, payload (num_min_values, 1, 1024); a min-value that is not finite -> MOE_ERR_INVALID_VALUE, payload
 * (the value, member, index); then moe_ei_analytic_mcmc's from num_points < 1 on, in its order and with its payloads, the row limit
 * num_being_sampled (1 + g) <= 64 last.  MOE_ERR_SINGULAR only for a pending point, payload (e, j), after the wait; a candidate
 * never raises. */
int moe_gibbon_mcmc(const moe_gp_t* const* gps, int num_mcmc, const double* min_values, int num_min_values,
                    const double* points_being_sampled, int num_being_sampled, const double* points, int num_points, int want_grad,
                    double* value, double* grad, moe_error_t* err);
/* One suggestion by moe_gibbon_mcmc's objective, the whole loop on the device: moe_ei_analytic_mcmc_multistart's screening, top-20
 * rule, restarted ascent and end-point selection, its outputs and their meaning (the kernels of the ascent are shared), so that the
 * path is, bit for bit, the one a host loop over moe_gibbon_mcmc walks.
 * Errors, in this order: those of moe_gibbon_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value and found
 * among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles.
 * MOE_ERR_SINGULAR as above, at the next wait. */
int moe_gibbon_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, const moe_gd_params_t* outer, const double* domain_bounds,
                               const double* min_values, int num_min_values, const double* points_being_sampled,
                               int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                               double* best_point, double* best_value, int* found, double* start_values, int* kept_index,
                               double* end_points, double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* num_to_sample points greedily: round t is moe_gibbon_mcmc_multistart from the same starts with pending points =
 * points_being_sampled followed by the picks of the rounds before -- bit for bit what num_to_sample calls of that function return
 * when each is fed its predecessors' points; the sum of the rounds' brackets is GIBBON's batch term.  Staged once; a round appends
 * ONE point (1 + g rows) to each member's extension inside device memory.
 * Errors: those of moe_gibbon_mcmc_multistart with moe_ei_analytic_mcmc_suggest's additions (num_to_sample, the row limit). */
int moe_gibbon_mcmc_suggest(const moe_gp_t* const* gps, int num_mcmc, const moe_gd_params_t* outer, const double* domain_bounds,
                            const double* min_values, int num_min_values, const double* points_being_sampled, int num_being_sampled,
                            const double* starts, int num_starts, int do_gradient_ascent, int num_to_sample, double* best_points,
                            double* best_values, int* found, moe_error_t* err);
/* The constrained expected improvement -- expected improvement times the probability of feasibility (Schonlau, Welch & Jones 1998;
 * Gardner et al. 2014; Gelbart, Snoek & Adams 2014) -- for minimisation under K = num_constraints unknown constraints, averaged over
 * an ensemble of E = num_mcmc joint hyper-samples, with pending points, evaluated on the device: value[i] and grad[i][dim] (want_grad
 * != 0) at points [num_points][dim].  0 <= K <= 8.  Member e is a tuple of 1 + K GP handles: the objective GP gps[e] and the
 * constraint GPs constraint_gps[k * num_mcmc + e] (one flat array [K][E]); constraint k is satisfied where c_k(x) <= thresholds[k].
 * All GPs of a call share dim, the device and the observed-derivative list; they may differ in num_sampled, covariance type,
 * hyper-parameters and noise.  No handle may appear twice anywhere in the call (every GP keeps its own workspaces).
 * Pending points condition the covariance of EVERY GP of the call as in moe_ei_analytic_mcmc, word for word: the GP's own noise on
 * their diagonal, its mean left alone, 1 + g rows per point under derivative observations, num_being_sampled (1 + g) <= 64.
 * Per member e at x, with mu and var the posterior mean and the conditioned latent variance of the GP in question:
 *   feasibility factor   F_{e,k} = Phi(z),  z = (tau_k - mu) / sigma,  sigma = sqrt(max(DBL_MIN, var)); Phi through erfc on the side
 *                        of z's sign
 *   its gradient         sigma_g = sqrt(max(150 eps^2, var)),  z_g = (tau_k - mu) / sigma_g,
 *                        grad F = -(phi(z_g) / sigma_g) grad mu - (phi(z_g) z_g / (2 sigma_g^2)) grad var
 *                        (moe_ei_analytic_mcmc's gradient form with (phi(z_g) / sigma_g, -phi(z_g) z_g / sigma_g^2) where it has
 *                        (Phi(c_g), phi(c_g) / sigma_g): the same kernels serve)
 *   improvement factor   EI_e exactly as in moe_ei_analytic_mcmc with the incumbent
 *                        b'_e = min(best_so_far[e], min over the believed-feasible pending points j of mu_{e,0}(P_j)),
 *                        P_j believed feasible under member e when mu_{e,k}(P_j) <= tau_k for every k
 *                        (without the rule a greedy batch re-picks its own point, or lets a believed-infeasible pick lower the
 *                        incumbent)
 *   no feasible incumbent  best_so_far[e] may be +infinity ("no feasible observation yet"): while b'_e is +infinity the improvement
 *                        factor is exactly 1 with a zero gradient, and the member's acquisition is its probability of feasibility;
 *                        a believed-feasible pending point makes b'_e finite in the ordinary way
 *   member value         A_e = EI_e F_{e,1} ... F_{e,K}, multiplied left to right; grad A_e by the product rule, each excluded
 *                        product formed by the same left-to-right multiplication with its factor skipped, the terms added in the
 *                        order objective, k = 1 .. K
 *   ensemble             value[i] = (A_0 + ... + A_{E-1}) / E, grad likewise: members added in member order and divided once, no
 *                        fused multiply-add anywhere in the product rule or the mean
 * factors (may be NULL): [E][1 + K][num_points], the factor values EI_e, F_{e,1}, ..., F_{e,K} at every point; value[i] is, bit for
 * bit, what the rule above makes of them on the host.  With K = 0 the call is moe_ei_analytic_mcmc bit for bit while every
 * best_so_far[e] is finite.  A candidate's bits do not depend on how many share the call (passes of moe_ei1_pass_size(N) candidates),
 * nor on want_grad, nor on ensemble-wide launches (the E (1 + K) GPs' chains are recorded and zipped where their shapes agree).
 * One copy down, one stream (the first objective GP's), one wait, one copy back; no handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_mcmc outside 1 .. 1024 ->
 * MOE_ERR_BOUNDS; a NULL array (gps, best_so_far, points, value, grad with want_grad) -> MOE_ERR_RUNTIME; num_constraints outside
 * 0 .. 8 -> MOE_ERR_BOUNDS, payload (num_constraints, 0, 8); num_mcmc (1 + num_constraints) > 1024 -> MOE_ERR_BOUNDS, payload
 * (num_mcmc, 1, 1024 / (1 + num_constraints) rounded down); constraint_gps or thresholds NULL with num_constraints > 0 ->
 * MOE_ERR_RUNTIME; a threshold that is not finite -> MOE_ERR_INVALID_VALUE, payload (the value, k, 0); a best_so_far[e] that is NaN
 * or -infinity -> MOE_ERR_INVALID_VALUE, payload (the value, e, 0); then moe_ei_analytic_mcmc's from num_points < 1 on, in its order
 * and with its payloads, "member" counting the GPs flat as e (1 + K) + role (role 0: the objective GP, role k: constraint k): a
 * NULL handle; a GP of another dim, then of another device; another observed-derivative list; a handle listed twice (a constraint
 * handle equal to an objective handle included), payload (the later flat index, the earlier, 0); the row limit last.
 * MOE_ERR_SINGULAR only for a pending point: payload (the flat index e (1 + K) + role of the first failing GP, the pending point),
 * reported at the next wait.  A candidate never raises: the two variance floors are moe_ei_analytic_mcmc's. */
int moe_ei_constrained_mcmc(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps, int num_constraints,
                            const double* thresholds, const double* best_so_far, const double* points_being_sampled,
                            int num_being_sampled, const double* points, int num_points, int want_grad, double* value, double* grad,
                            double* factors, moe_error_t* err);
/* One suggestion by moe_ei_constrained_mcmc's objective, the whole loop on the device: moe_ei_analytic_mcmc_multistart's screening,
 * top-20 rule, restarted ascent and end-point selection, its outputs and their meaning (the kernels of the ascent are shared; the
 * product rule leaves ONE combined gradient per step, which the step kernel takes as a one-member ensemble), so that the path is,
 * bit for bit, the one a host loop over moe_ei_constrained_mcmc walks.  Tensor-product domains only.  The host waits as often as
 * moe_ei_analytic_mcmc_multistart does, and no more.
 * Errors, in this order: those of moe_ei_constrained_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value
 * and found among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles.
 * MOE_ERR_SINGULAR as above, at the next wait. */
int moe_ei_constrained_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps,
                                       int num_constraints, const double* thresholds, const moe_gd_params_t* outer,
                                       const double* domain_bounds, const double* best_so_far, const double* points_being_sampled,
                                       int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                       double* best_point, double* best_value, int* found, double* start_values, int* kept_index,
                                       double* end_points, double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* num_to_sample points greedily: round t is moe_ei_constrained_mcmc_multistart from the same starts with pending points =
 * points_being_sampled followed by the picks of the rounds before -- bit for bit what num_to_sample calls of that function return
 * when each is fed its predecessors' points.  Staged once; a round appends ONE point (1 + g rows) to the extension of each of the
 * E (1 + K) GPs, and where member e believes the pick feasible its believed value mu_{e,0}(x_t) joins b'_e, inside device memory.
 * Errors: those of moe_ei_constrained_mcmc_multistart with moe_ei_analytic_mcmc_suggest's additions (num_to_sample, the row limit). */
int moe_ei_constrained_mcmc_suggest(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps,
                                    int num_constraints, const double* thresholds, const moe_gd_params_t* outer,
                                    const double* domain_bounds, const double* best_so_far, const double* points_being_sampled,
                                    int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                    int num_to_sample, double* best_points, double* best_values, int* found, moe_error_t* err);
/* The LOG of moe_ei_constrained_mcmc's quantity (Ament et al. 2023, "Unexpected improvements to expected improvement"), computed
 * without ever forming a Phi or phi that float64 would underflow: finite, with a useful gradient, for every finite input -- where
 * the plain form and its gradient are exactly 0 (c = (b' - mu) / sigma below about -38, or one constraint far from feasible).
 * The call is moe_ei_constrained_mcmc's, argument for argument: the members, their order, the pending points and the believed-
 * feasible incumbent b'_e are those.  num_constraints = 0 is the log of the ensemble-averaged analytic expected improvement.
 * Per member e at x, with ONE variance floor for value and gradient, sigma = sqrt(max(150 eps^2, var)):
 *   improvement   c = (b'_e - mu) / sigma,  h(c) = c Phi(c) + phi(c):   l_{e,0} = log sigma + log h(c),
 *                 grad l = -(lambda / sigma) grad mu + (kappa / (2 sigma^2)) grad var,  lambda = Phi / h,  kappa = phi / h
 *                 (c >= 0 directly; -6 <= c < 0 through h / phi = 1 + c sqrt(pi / 2) erfcx(-c / sqrt 2); c < -6 through 20 terms
 *                 of Laplace's continued fraction of the Mills ratio);  b'_e = +infinity: l_{e,0} = 0 with a zero gradient
 *   feasibility   z = (tau_k - mu) / sigma:   l_{e,k} = log Phi(z),  grad l = -(r / sigma) grad mu - (r z / (2 sigma^2)) grad var,
 *                 r = phi / Phi  (z < 0 through erfcx, z >= 0 through log1p(-erfc / 2))
 *   member        L_e = l_{e,0} + ... + l_{e,K}, the gradient g_e likewise, added in the order objective, k = 1 .. K
 *   ensemble      m = max_e L_e, w_e = exp(L_e - m), W = w_0 + ... + w_{E-1}:  value[i] = m + log W - log E,
 *                 grad[i] = (w_0 g_0 + ... + w_{E-1} g_{E-1}) / W; members in member order, no fused multiply-add in the rule
 * log_factors (may be NULL): [E][1 + K][num_points], every l_{e,r}.  With E = 1 and K = 0 value[i] is log_factors[0][0][i] bit for
 * bit.  A candidate's bits do not depend on how many share the call, on want_grad or on ensemble-wide launches.
 * Errors: moe_ei_constrained_mcmc's, in its order and with its payloads. */
int moe_log_ei_constrained_mcmc(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps, int num_constraints,
                                const double* thresholds, const double* best_so_far, const double* points_being_sampled,
                                int num_being_sampled, const double* points, int num_points, int want_grad, double* value,
                                double* grad, double* log_factors, moe_error_t* err);
/* moe_ei_constrained_mcmc_multistart with moe_log_ei_constrained_mcmc's objective: the same screening, top-20 rule, restarted
 * ascent and outputs, bit for bit the path a host loop over moe_log_ei_constrained_mcmc walks.  Errors: that function's, the
 * ascent's named "the log constrained expected improvement". */
int moe_log_ei_constrained_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps,
                                           int num_constraints, const double* thresholds, const moe_gd_params_t* outer,
                                           const double* domain_bounds, const double* best_so_far,
                                           const double* points_being_sampled, int num_being_sampled, const double* starts,
                                           int num_starts, int do_gradient_ascent, double* best_point, double* best_value, int* found,
                                           double* start_values, int* kept_index, double* end_points, double* end_values, double* path,
                                           int* steps_taken, moe_error_t* err);
/* moe_ei_constrained_mcmc_suggest with moe_log_ei_constrained_mcmc's objective: num_to_sample points greedily, bit for bit what
 * num_to_sample calls of moe_log_ei_constrained_mcmc_multistart return when each is fed its predecessors' points.  Errors: that
 * function's. */
int moe_log_ei_constrained_mcmc_suggest(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps,
                                        int num_constraints, const double* thresholds, const moe_gd_params_t* outer,
                                        const double* domain_bounds, const double* best_so_far, const double* points_being_sampled,
                                        int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                        int num_to_sample, double* best_points, double* best_values, int* found, moe_error_t* err);
/* The LOG of the constrained expected improvement PER UNIT COST (Snoek, Larochelle & Adams 2012, "EI per second"; the exponent of
 * cost-cooling, Lee et al. 2020) averaged over a hyper-parameter ensemble.  The call is moe_log_ei_constrained_mcmc's with
 * (cost_gps, cost_exponent) behind thresholds: cost_gps [E], cost_gps[e] member e's GP of the LOG of the evaluation cost;
 * cost_exponent = alpha >= 0 (1: improvement per unit cost; lowered towards 0 as a budget runs out; 0: the cost plays no part).
 * Member e is 2 + K GPs, counted flat as e (2 + K) + role: role 0 the objective, roles 1 .. K the constraints, role K + 1 the cost
 * GP.  All 2 + K GPs of a call carry one dim, one device and ONE observed-derivative list (a pending point is 1 + g extension rows
 * of at most 64), and every GP's covariance, the cost GP's too, is conditioned on the pending points with the mean left alone: one
 * staging serves every sub-member, so the cost's variance term is the conditioned one.  The believed-feasible incumbent b'_e is
 * moe_ei_constrained_mcmc's; the cost GP takes no part in it.  Per member e at x, with ONE variance floor for value and gradient,
 * v = max(150 eps^2, var), sigma = sqrt(v):
 *   improvement   l_{e,0} and its gradient exactly moe_log_ei_constrained_mcmc's (b'_e = +infinity: 0 with a zero gradient)
 *   feasibility   l_{e,k} and its gradient exactly moe_log_ei_constrained_mcmc's
 *   cost          l_{e,c} = -(alpha (mu_c + v_c / 2)), the log of E[cost]^-alpha under a log-normal cost,
 *                 grad l = -alpha grad mu_c - (alpha / 2) grad var_c, the second term 0 where var_c lies below the floor
 *   member        L_e = ((l_{e,0} + l_{e,1}) + ... + l_{e,K}) + l_{e,c}, the gradient g_e likewise, in that order
 *   ensemble      m = max_e L_e, w_e = exp(L_e - m), W = w_0 + ... + w_{E-1}:  value[i] = m + log W - log E,
 *                 grad[i] = (w_0 g_0 + ... + w_{E-1} g_{E-1}) / W; members in member order, every operation rounded by itself, no
 *                 fused multiply-add in the rule, no atomics
 * log_factors (may be NULL): [E][2 + K][num_points], every l_{e,r}, the cost row last.  With E = 1 value[i] is the member's log
 * factors added left to right, bit for bit; with cost_exponent = 0 value, grad and rows 0 .. K are moe_log_ei_constrained_mcmc's bit
 * for bit and the cost row is 0.  A candidate's bits do not depend on how many share the call, on want_grad or on ensemble-wide
 * launches.  The value is finite with a useful gradient for every finite input.
 * Errors: moe_log_ei_constrained_mcmc's, in its order and with its payloads, with these changes: cost_gps is among the arrays
 * that must not be NULL (MOE_ERR_RUNTIME); the product limit is num_mcmc (2 + num_constraints) > 1024 -> MOE_ERR_BOUNDS, payload
 * (num_mcmc, 1, 1024 / (2 + num_constraints) rounded down); behind the best_so_far check, a cost_exponent that is not finite or is
 * negative -> MOE_ERR_INVALID_VALUE, payload (the value, 0, 0); the handle checks count the GPs flat as e (2 + K) + role, and so does
 * MOE_ERR_SINGULAR's payload for a pending point. */
int moe_log_ei_per_cost_mcmc(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps, int num_constraints,
                             const double* thresholds, const moe_gp_t* const* cost_gps, double cost_exponent,
                             const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                             const double* points, int num_points, int want_grad, double* value, double* grad, double* log_factors,
                             moe_error_t* err);
/* moe_log_ei_constrained_mcmc_multistart with moe_log_ei_per_cost_mcmc's objective: the same screening, top-20 rule, restarted
 * ascent and outputs, bit for bit the path a host loop over moe_log_ei_per_cost_mcmc walks.  Errors: that function's, the ascent's
 * named "the log expected improvement per unit cost". */
int moe_log_ei_per_cost_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps,
                                        int num_constraints, const double* thresholds, const moe_gp_t* const* cost_gps,
                                        double cost_exponent, const moe_gd_params_t* outer, const double* domain_bounds,
                                        const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                        const double* starts, int num_starts, int do_gradient_ascent, double* best_point,
                                        double* best_value, int* found, double* start_values, int* kept_index, double* end_points,
                                        double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* moe_log_ei_constrained_mcmc_suggest with moe_log_ei_per_cost_mcmc's objective: num_to_sample points greedily, bit for bit what
 * num_to_sample calls of moe_log_ei_per_cost_mcmc_multistart return when each is fed its predecessors' points; a pick joins the
 * extension of each of the E (2 + K) GPs.  Errors: that function's. */
int moe_log_ei_per_cost_mcmc_suggest(const moe_gp_t* const* gps, int num_mcmc, const moe_gp_t* const* constraint_gps,
                                     int num_constraints, const double* thresholds, const moe_gp_t* const* cost_gps,
                                     double cost_exponent, const moe_gd_params_t* outer, const double* domain_bounds,
                                     const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                     const double* starts, int num_starts, int do_gradient_ascent, int num_to_sample,
                                     double* best_points, double* best_values, int* found, moe_error_t* err);
/* The two-objective expected hypervolume improvement (EHVI; Emmerich, Giannakoglou & Naujoks 2006; Emmerich, Deutz & Klinkenberg
 * 2011; Yang et al. 2019) averaged over a hyper-parameter ensemble, at points [num_points][dim], with pending points.  Minimisation.
 * Member e is two GPs, gps[e] for objective 1 and gps2[e] for objective 2: one dim, one device, no derivative observations; their
 * observation lists may differ.  reference_point [2] = (r1, r2); front [num_front][2] = (u_i, v_i), 0 <= num_front <= 960, finite,
 * strictly inside the reference point, sorted u_1 < ... < u_F and mutually non-dominated, hence v_1 > ... > v_F (may be NULL with
 * num_front = 0).  With u_0 = -infinity, u_{F+1} = r1, v_0 = r2, and mu_r, var_r the posterior mean and the conditioned latent
 * variance of objective r's GP at x:
 *   psi_r(t) = (t - mu_r) Phi(z) + sigma_r phi(z),  z = (t - mu_r) / sigma_r,  sigma_r = sqrt(max(DBL_MIN, var_r)),
 *              psi_1(-infinity) = 0
 *   member value   A_e = max(0, sum_{i = 0 .. F} [psi_1(u_{i+1}) - psi_1(u_i)] psi_2(v_i))
 *   its gradient   through d psi / d mu = -Phi(z_g) and d psi / d var = phi(z_g) / (2 sigma_g), sigma_g = sqrt(max(150 eps^2, var))
 *                  (moe_ei_analytic_mcmc's two floors), applied to grad mu_r and grad var_r of both GPs; 0 where A_e is clipped
 *   ensemble       value[i] = (A_0 + ... + A_{E-1}) / E, grad likewise: members added in member order and divided once
 * With num_front = 0 a member's value is the product of two analytic expected improvements with the incumbents r1 and r2.
 * Pending points: both GPs' variances are conditioned on them as in moe_ei_analytic_mcmc (the means are left alone), and the believed
 * outcome (mu_{e,1}(P_j), mu_{e,2}(P_j)) joins member e's OWN front, in the order of j, when it lies strictly inside the reference
 * point and no front point (u, v) has u <= it and v <= it in both objectives; the front points it dominates leave.
 * member_values_out (may be NULL): [E][num_points], every A_e; value[i] is, bit for bit, their mean formed in member order on the host.
 * A candidate's bits do not depend on how many share the call (passes of moe_ei1_pass_size(N) candidates), nor on want_grad, nor on
 * ensemble-wide launches; the strip sum's order is fixed by the front's size alone (csrc/ehvi1.hip).  No handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_mcmc outside 1 .. 512 ->
 * MOE_ERR_BOUNDS, payload (num_mcmc, 1, 512); a NULL array (gps, gps2, reference_point, points, value, grad with want_grad, front
 * with num_front > 0) -> MOE_ERR_RUNTIME; num_front outside 0 .. 960 -> MOE_ERR_BOUNDS, payload (num_front, 0, 960); a reference
 * point that is not finite -> MOE_ERR_INVALID_VALUE, payload (the value, its index, 0); a front point that is not finite, not
 * strictly inside the reference point, or not behind its predecessor in the order above -> MOE_ERR_INVALID_VALUE, payload (the
 * point's index, 0, 0); num_points < 1 -> MOE_ERR_BOUNDS; num_being_sampled outside 0 .. 64 -> MOE_ERR_BOUNDS; points_being_sampled
 * NULL with num_being_sampled > 0 -> MOE_ERR_RUNTIME; then, "member" counting the GPs flat as 2 e + objective - 1: a NULL handle ->
 * MOE_ERR_RUNTIME; a GP of another dim, then of another device -> MOE_ERR_INVALID_VALUE; a GP with derivative observations ->
 * MOE_ERR_INVALID_VALUE, payload (its num_derivatives, 0, the flat index); a handle listed twice (gps2[e] equal to some gps[f]
 * included) -> MOE_ERR_INVALID_VALUE, payload (the later flat index, the earlier, 0).
 * MOE_ERR_SINGULAR only for a pending point: payload (the flat index of the first failing GP, the pending point), reported at the
 * next wait.  A candidate never raises. */
int moe_ehvi_mcmc(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, int num_mcmc, const double* reference_point,
                  const double* front, int num_front, const double* points_being_sampled, int num_being_sampled, const double* points,
                  int num_points, int want_grad, double* value, double* grad, double* member_values_out, moe_error_t* err);
/* One suggestion by moe_ehvi_mcmc's objective, the whole loop on the device: moe_ei_analytic_mcmc_multistart's screening, top-20
 * rule, restarted ascent and end-point selection, its outputs and their meaning (the kernels of the ascent are shared; the strip
 * rule leaves ONE combined gradient per step), so that the path is, bit for bit, the one a host loop over moe_ehvi_mcmc walks.
 * Tensor-product domains only.
 * Errors, in this order: those of moe_ehvi_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value and found
 * among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles. */
int moe_ehvi_mcmc_multistart(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, int num_mcmc, const double* reference_point,
                             const double* front, int num_front, const moe_gd_params_t* outer, const double* domain_bounds,
                             const double* points_being_sampled, int num_being_sampled, const double* starts, int num_starts,
                             int do_gradient_ascent, double* best_point, double* best_value, int* found, double* start_values,
                             int* kept_index, double* end_points, double* end_values, double* path, int* steps_taken,
                             moe_error_t* err);
/* num_to_sample points greedily: round t is moe_ehvi_mcmc_multistart from the same starts with pending points = points_being_sampled
 * followed by the picks of the rounds before -- bit for bit what num_to_sample calls of that function return when each is fed its
 * predecessors' points.  Staged once; a round appends ONE row to the extension of each of the 2 E GPs and the pick's believed
 * outcome to every member's front, inside device memory.
 * Errors: those of moe_ehvi_mcmc_multistart, with num_to_sample < 1 or num_being_sampled + num_to_sample - 1 > 64 -> MOE_ERR_BOUNDS
 * behind num_being_sampled. */
int moe_ehvi_mcmc_suggest(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, int num_mcmc, const double* reference_point,
                          const double* front, int num_front, const moe_gd_params_t* outer, const double* domain_bounds,
                          const double* points_being_sampled, int num_being_sampled, const double* starts, int num_starts,
                          int do_gradient_ascent, int num_to_sample, double* best_points, double* best_values, int* found,
                          moe_error_t* err);
/* The three-objective expected hypervolume improvement averaged over a hyper-parameter ensemble, at points [num_points][dim], with
 * pending points.  Minimisation.  Member e is three GPs, gps[e], gps2[e] and gps3[e] for objectives 1, 2 and 3: one dim, one
 * device, no derivative observations; their observation lists may differ.  reference_point [3] = (r1, r2, r3); front
 * [num_front][3] = (u_i, v_i, w_i), 0 <= num_front <= 192, finite, strictly inside the reference point, mutually non-dominated
 * (no point <= another in all three objectives; equal points count as dominated) and in the CANONICAL ORDER: w ascending, ties by
 * u, then by v (may be NULL with num_front = 0).  psi_k, sigma_k and the gradient's floor are moe_ehvi_mcmc's.  With w_0 =
 * -infinity and w_{F+1} = r3, the slab between w_k and w_{k+1} has the two-dimensional non-dominated region of the first k points'
 * (u, v) projections as its cross-section:
 *   S2_k           = sum over the strips of the staircase of points 1 .. k in (u, v) of [psi_1(right) - psi_1(left)] psi_2(height)
 *   member value   A_e = max(0, sum_{k = 0 .. F} S2_k [psi_3(w_{k+1}) - psi_3(w_k)])
 *   its gradient   through the six coefficients dA/dmu_k and dA/dvar_k applied to grad mu_k and grad var_k; 0 where A_e is clipped
 *   ensemble       value[i] = (A_0 + ... + A_{E-1}) / E, grad likewise: members added in member order and divided once
 * With num_front = 0 a member's value is (EI_1 EI_2) EI_3, the analytic expected improvements with the incumbents r1, r2 and r3,
 * each product rounded once.  Pending points: all three GPs' variances are conditioned on them (the means are left alone), and the
 * believed outcome (mu_{e,1}, mu_{e,2}, mu_{e,3})(P_j) joins member e's OWN front, in the order of j, when it is finite, strictly
 * inside the reference point and no front point is <= it in all three objectives; the front points >= it in all three leave, and
 * the canonical order is kept.
 * member_values_out (may be NULL): [E][num_points], every A_e; value[i] is, bit for bit, their mean formed in member order on the host.
 * A candidate's bits do not depend on how many share the call (passes of moe_ei1_pass_size(N) candidates), nor on want_grad, nor on
 * ensemble-wide launches; the box sum's order is fixed by the member's front alone (csrc/ehvi3.hip).  No handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_mcmc outside 1 .. 341 ->
 * MOE_ERR_BOUNDS, payload (num_mcmc, 1, 341); a NULL array (gps, gps2, gps3, reference_point, points, value, grad with want_grad,
 * front with num_front > 0) -> MOE_ERR_RUNTIME; num_front outside 0 .. 192 -> MOE_ERR_BOUNDS, payload (num_front, 0, 192); a
 * reference point that is not finite -> MOE_ERR_INVALID_VALUE, payload (the value, its index, 0); a front point that is not
 * finite, not strictly inside the reference point, not behind its predecessor in the canonical order, or >= an earlier point
 * in all three objectives -> MOE_ERR_INVALID_VALUE, payload (the point's index, 0, 0); num_points < 1 -> MOE_ERR_BOUNDS;
 * num_being_sampled outside 0 .. 64 -> MOE_ERR_BOUNDS; points_being_sampled NULL with num_being_sampled > 0 -> MOE_ERR_RUNTIME;
 * then, "member" counting the GPs flat as 3 e + objective - 1: a NULL handle -> MOE_ERR_RUNTIME; a GP of another dim, then of
 * another device -> MOE_ERR_INVALID_VALUE; a GP with derivative observations -> MOE_ERR_INVALID_VALUE, payload (its
 * num_derivatives, 0, the flat index); a handle listed twice -> MOE_ERR_INVALID_VALUE, payload (the later flat index, the earlier, 0).
 * MOE_ERR_SINGULAR only for a pending point: payload (the flat index of the first failing GP, the pending point), reported at the
 * next wait.  A candidate never raises. */
int moe_ehvi3_mcmc(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3, int num_mcmc,
                   const double* reference_point, const double* front, int num_front, const double* points_being_sampled,
                   int num_being_sampled, const double* points, int num_points, int want_grad, double* value, double* grad,
                   double* member_values_out, moe_error_t* err);
/* One suggestion by moe_ehvi3_mcmc's objective, the whole loop on the device, as moe_ehvi_mcmc_multistart is for moe_ehvi_mcmc: the
 * path is, bit for bit, the one a host loop over moe_ehvi3_mcmc walks.  Tensor-product domains only.
 * Errors, in this order: those of moe_ehvi3_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value and found
 * among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles. */
int moe_ehvi3_mcmc_multistart(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3, int num_mcmc,
                              const double* reference_point, const double* front, int num_front, const moe_gd_params_t* outer,
                              const double* domain_bounds, const double* points_being_sampled, int num_being_sampled,
                              const double* starts, int num_starts, int do_gradient_ascent, double* best_point, double* best_value,
                              int* found, double* start_values, int* kept_index, double* end_points, double* end_values, double* path,
                              int* steps_taken, moe_error_t* err);
/* num_to_sample points greedily: round t is moe_ehvi3_mcmc_multistart from the same starts with pending points =
 * points_being_sampled followed by the picks of the rounds before -- bit for bit what num_to_sample calls of that function return
 * when each is fed its predecessors' points.  Staged once; a round appends ONE row to the extension of each of the 3 E GPs and the
 * pick's believed outcome to every member's front, whose box table is rebuilt, inside device memory.
 * Errors: those of moe_ehvi3_mcmc_multistart, with num_to_sample < 1 or num_being_sampled + num_to_sample - 1 > 64 ->
 * MOE_ERR_BOUNDS behind num_being_sampled. */
int moe_ehvi3_mcmc_suggest(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3, int num_mcmc,
                           const double* reference_point, const double* front, int num_front, const moe_gd_params_t* outer,
                           const double* domain_bounds, const double* points_being_sampled, int num_being_sampled,
                           const double* starts, int num_starts, int do_gradient_ascent, int num_to_sample, double* best_points,
                           double* best_values, int* found, moe_error_t* err);
/* The constrained expected hypervolume improvement for two objectives: moe_ehvi_mcmc's quantity times the probability of
 * feasibility (Schonlau, Welch & Jones 1998; Gardner et al. 2014), averaged over a hyper-parameter ensemble, at points
 * [num_points][dim], with pending points.  Minimisation.  Member e is 2 + K GPs: gps[e] and gps2[e] for the objectives and the
 * constraint GPs constraint_gps[e * num_constraints + k] (one flat array [E][K]), 0 <= K = num_constraints <= 8; constraint k is
 * satisfied where c_k(x) <= thresholds[k].  One dim, one device, no derivative observations; the observation lists may differ.
 * reference_point and front are moe_ehvi_mcmc's, the front being that of the FEASIBLE observations.  Per member e at x, with mu and
 * var the posterior mean and the conditioned latent variance of the GP in question:
 *   hypervolume term     H_e: moe_ehvi_mcmc's A_e, the same strip sum in the same order, the same clip at 0, and its four
 *                        coefficients dH/dmu_r, dH/dvar_r
 *   feasibility factor   F_{e,k} = Phi(z),  z = (tau_k - mu) / sigma,  sigma = sqrt(max(DBL_MIN, var))
 *   its gradient         sigma_g = sqrt(max(150 eps^2, var)),  z_g = (tau_k - mu) / sigma_g,
 *                        grad F = -(phi(z_g) / sigma_g) grad mu - (phi(z_g) z_g / (2 sigma_g^2)) grad var
 *   member value         A_e = H_e F_{e,1} ... F_{e,K}, multiplied left to right; grad A_e by the product rule, each excluded
 *                        product formed by the same left-to-right multiplication with its factor skipped, the terms added in the
 *                        order H, k = 1 .. K; grad H_e from its coefficients in moe_ehvi_mcmc's order
 *   ensemble             value[i] = (A_0 + ... + A_{E-1}) / E, grad likewise: members added in member order and divided once, no
 *                        fused multiply-add anywhere in the product rule or the mean
 * Pending points: every GP's variance is conditioned on them as in moe_ei_analytic_mcmc (the means are left alone), whichever way
 * the belief falls.  P_j is BELIEVED FEASIBLE under member e when mu_{e,k}(P_j) <= tau_k for every k; its believed outcome
 * (mu_{e,1}(P_j), mu_{e,2}(P_j)) is offered to member e's own front, in the order of j and under moe_ehvi_mcmc's join rule, only
 * where member e believes it feasible: a believed-infeasible point does not shrink the non-dominated region.
 * factors_out (may be NULL): [E][1 + K][num_points], the values H_e, F_{e,1}, ..., F_{e,K} at every point; value[i] is, bit for bit,
 * what the rule above makes of them on the host.  With K = 0 the call is moe_ehvi_mcmc bit for bit (factors_out is then its
 * member_values_out).  A candidate's bits do not depend on how many share the call (passes of moe_ei1_pass_size(N) candidates),
 * nor on want_grad, nor on ensemble-wide launches (csrc/cehvi1.hip).  No handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_mcmc outside 1 .. 512 ->
 * MOE_ERR_BOUNDS, payload (num_mcmc, 1, 512); a NULL array (gps, gps2, reference_point, points, value, grad with want_grad, front
 * with num_front > 0) -> MOE_ERR_RUNTIME; num_constraints outside 0 .. 8 -> MOE_ERR_BOUNDS, payload (num_constraints, 0, 8);
 * num_mcmc (2 + num_constraints) > 1024 -> MOE_ERR_BOUNDS, payload (num_mcmc, 1, 1024 / (2 + num_constraints) rounded down);
 * constraint_gps or thresholds NULL with num_constraints > 0 -> MOE_ERR_RUNTIME; a threshold that is not finite ->
 * MOE_ERR_INVALID_VALUE, payload (the value, k, 0); then moe_ehvi_mcmc's from num_front on, in its order and with its payloads,
 * "member" counting the GPs flat as e (2 + K) + role (roles 0 and 1: the objectives, role 1 + k: constraint k = 1 .. K): a NULL
 * handle; a GP of another dim, then of another device; a GP with derivative observations, objective or constraint, payload (its
 * num_derivatives, 0, the flat index); a handle listed twice, across roles too, payload (the later flat index, the earlier, 0).
 * MOE_ERR_SINGULAR only for a pending point: payload (the flat index e (2 + K) + role of the first failing GP, the pending point),
 * reported at the next wait.  A candidate never raises. */
int moe_ehvi_constrained_mcmc(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* constraint_gps,
                              int num_constraints, const double* thresholds, int num_mcmc, const double* reference_point,
                              const double* front, int num_front, const double* points_being_sampled, int num_being_sampled,
                              const double* points, int num_points, int want_grad, double* value, double* grad, double* factors_out,
                              moe_error_t* err);
/* One suggestion by moe_ehvi_constrained_mcmc's objective, the whole loop on the device, as moe_ehvi_mcmc_multistart is for
 * moe_ehvi_mcmc: the path is, bit for bit, the one a host loop over moe_ehvi_constrained_mcmc walks.  Tensor-product domains only.
 * With K = 0 the call is moe_ehvi_mcmc_multistart bit for bit.
 * Errors, in this order: those of moe_ehvi_constrained_mcmc that need no handle (outer, domain_bounds, starts, best_point,
 * best_value and found among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with
 * do_gradient_ascent != 0 -> MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those
 * that need the handles. */
int moe_ehvi_constrained_mcmc_multistart(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* constraint_gps,
                                         int num_constraints, const double* thresholds, int num_mcmc, const double* reference_point,
                                         const double* front, int num_front, const moe_gd_params_t* outer, const double* domain_bounds,
                                         const double* points_being_sampled, int num_being_sampled, const double* starts,
                                         int num_starts, int do_gradient_ascent, double* best_point, double* best_value, int* found,
                                         double* start_values, int* kept_index, double* end_points, double* end_values, double* path,
                                         int* steps_taken, moe_error_t* err);
/* num_to_sample points greedily: round t is moe_ehvi_constrained_mcmc_multistart from the same starts with pending points =
 * points_being_sampled followed by the picks of the rounds before -- bit for bit what num_to_sample calls of that function return
 * when each is fed its predecessors' points.  Staged once; a round appends ONE row to the extension of each of the E (2 + K) GPs
 * and offers the pick's believed outcome to the fronts of the members that believe it feasible, inside device memory.
 * Errors: those of moe_ehvi_constrained_mcmc_multistart, with num_to_sample < 1 or num_being_sampled + num_to_sample - 1 > 64 ->
 * MOE_ERR_BOUNDS behind num_being_sampled. */
int moe_ehvi_constrained_mcmc_suggest(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* constraint_gps,
                                      int num_constraints, const double* thresholds, int num_mcmc, const double* reference_point,
                                      const double* front, int num_front, const moe_gd_params_t* outer, const double* domain_bounds,
                                      const double* points_being_sampled, int num_being_sampled, const double* starts, int num_starts,
                                      int do_gradient_ascent, int num_to_sample, double* best_points, double* best_values, int* found,
                                      moe_error_t* err);
/* The constrained expected hypervolume improvement for three objectives: moe_ehvi_constrained_mcmc with moe_ehvi3_mcmc's hypervolume
 * term in the place of moe_ehvi_mcmc's.  Member e is 3 + K GPs, gps[e], gps2[e], gps3[e] and constraint_gps[e * num_constraints +
 * k]; reference_point [3], front [num_front][3] and the join rule are moe_ehvi3_mcmc's, H_e is its A_e with its six coefficients
 * (the same box sum in the same order, the member's box table rebuilt whenever its front changes), and the feasibility factors,
 * the product rule, the ensemble mean, the believed-feasible rule for pending points and factors_out [E][1 + K][num_points] are
 * moe_ehvi_constrained_mcmc's.  With K = 0 the call is moe_ehvi3_mcmc bit for bit.
 * Errors: moe_ehvi_constrained_mcmc's, in its order, with moe_ehvi3_mcmc's limits and checks where that has moe_ehvi_mcmc's:
 * num_mcmc outside 1 .. 341, payload (num_mcmc, 1, 341); gps3 among the arrays that must not be NULL; num_mcmc (3 +
 * num_constraints) > 1024 -> MOE_ERR_BOUNDS, payload (num_mcmc, 1, 1024 / (3 + num_constraints) rounded down); num_front outside
 * 0 .. 192; the canonical order; "member" counting the GPs flat as e (3 + K) + role (roles 0 .. 2: the objectives, role 2 + k:
 * constraint k = 1 .. K). */
int moe_ehvi3_constrained_mcmc(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3,
                               const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds, int num_mcmc,
                               const double* reference_point, const double* front, int num_front, const double* points_being_sampled,
                               int num_being_sampled, const double* points, int num_points, int want_grad, double* value, double* grad,
                               double* factors_out, moe_error_t* err);
/* moe_ehvi_constrained_mcmc_multistart with moe_ehvi3_constrained_mcmc's objective; with K = 0 moe_ehvi3_mcmc_multistart bit for bit.
 * Errors: moe_ehvi3_constrained_mcmc's that need no handle, the ascent's parameters, then those that need the handles. */
int moe_ehvi3_constrained_mcmc_multistart(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3,
                                          const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                          int num_mcmc, const double* reference_point, const double* front, int num_front,
                                          const moe_gd_params_t* outer, const double* domain_bounds, const double* points_being_sampled,
                                          int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                          double* best_point, double* best_value, int* found, double* start_values, int* kept_index,
                                          double* end_points, double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* moe_ehvi_constrained_mcmc_suggest with moe_ehvi3_constrained_mcmc's objective: num_to_sample points greedily, bit for bit what
 * num_to_sample calls of moe_ehvi3_constrained_mcmc_multistart return when each is fed its predecessors' points; with K = 0
 * moe_ehvi3_mcmc_suggest bit for bit.  Errors: those of moe_ehvi3_constrained_mcmc_multistart with moe_ehvi3_mcmc_suggest's additions. */
int moe_ehvi3_constrained_mcmc_suggest(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3,
                                       const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                       int num_mcmc, const double* reference_point, const double* front, int num_front,
                                       const moe_gd_params_t* outer, const double* domain_bounds, const double* points_being_sampled,
                                       int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                       int num_to_sample, double* best_points, double* best_values, int* found, moe_error_t* err);
/* The LOG of moe_ehvi_constrained_mcmc's quantity (two objectives, 0 <= K = num_constraints <= 8; K = 0 is the log of
 * moe_ehvi_mcmc's), computed so that it stays finite with a useful gradient where that value and its gradient are exactly 0 in
 * float64: psi underflows where a candidate's mean lies a few dozen deviations above the reference point in either objective, Phi
 * from 38 deviations down.  Arguments, members, fronts, the join rule, the believed-feasible rule for pending points and the limits
 * are moe_ehvi_constrained_mcmc's.  A member's front is F' points u_1 < ... < u_F' < r1, r2 > v_1 > ... > v_F'; u_0 = -infinity,
 * u_{F'+1} = r1, v_0 = r2.  ONE variance floor for value and gradient, sigma = sqrt(max(150 eps^2, var)).  For objective r and an
 * edge t:  z = (t - mu_r) / sigma_r, h(z) = z Phi(z) + phi(z), lam = Phi / h, kap = phi / h,
 *   lambda_r(t) = log sigma_r + log h(z) = log psi_r(t);  lambda_1(-infinity) = -infinity with lam = kap = 0
 * (log h, lam and kap as in moe_log_ei_constrained_mcmc: none is the log of a float64 Phi or phi that could have underflowed).
 *   strip i = 0 .. F'    a = u_i, b = u_{i+1}:  rho_i = exp(lambda_1(a) - lambda_1(b)) in [0, 1],
 *                        log Delta_i = lambda_1(b) + log(1 - rho_i)  (log1p(-rho) for rho <= 1/2, log(-expm1(lambda_1(a) -
 *                        lambda_1(b))) above),  l_i = log Delta_i + lambda_2(v_i)
 *   its derivatives      dl_i/dmu_1 = -(lam_b - rho_i lam_a) / (sigma_1 (1 - rho_i)),  dl_i/dvar_1 = (kap_b - rho_i kap_a) / (2 sigma_1^2
 *                        (1 - rho_i)),  dl_i/dmu_2 = -lam(v_i) / sigma_2,  dl_i/dvar_2 = kap(v_i) / (2 sigma_2^2); 1 - rho from the same
 *                        expm1 where rho > 1/2.  A strip whose two edges do not give lambda_1(a) < lambda_1(b) in float64 (rho = 1)
 *                        carries weight 0 and its terms are skipped, not evaluated.
 *   hypervolume term     L_e = log sum_i exp l_i as a log-sum-exp whose order depends on F' alone (csrc/logehvi1.hip), its four
 *                        coefficients (sum_i w_i dl_i/d.) / W_e.  Never clipped: the sum is positive for every finite input.
 *   feasibility          log F_{e,k} = log Phi(z), z = (tau_k - mu) / sigma, r = phi(z) / Phi(z),
 *                        grad log F = -(r / sigma) grad mu - (r z / (2 sigma^2)) grad var   (moe_log_ei_constrained_mcmc's role k)
 *   member               LL_e = L_e + log F_{e,1} + ... + log F_{e,K}, added in that order;  g_e = ((c_mu1 grad mu_1 + c_var1 grad
 *                        var_1) + c_mu2 grad mu_2) + c_var2 grad var_2, then + grad log F_{e,k} for k = 1 .. K
 *   ensemble             m = max_e LL_e, w_e = exp(LL_e - m), W = w_0 + ... + w_{E-1} in member order;
 *                        value[i] = m + log W - log E,  grad = (w_0 g_0 + ... + w_{E-1} g_{E-1}) / W, every operation rounded by
 *                        itself, no atomics
 * factors_out (may be NULL): [E][1 + K][num_points], L_e, log F_{e,1}, ..., log F_{e,K} at every point; value[i] is what the rule
 * above makes of them (with E = 1 their sum, bit for bit).  A candidate's bits do not depend on how many share the call, nor on
 * want_grad, nor on ensemble-wide launches.  No handle is modified.
 * Errors: moe_ehvi_constrained_mcmc's, in its order and with its payloads. */
int moe_log_ehvi_constrained_mcmc(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* constraint_gps,
                                  int num_constraints, const double* thresholds, int num_mcmc, const double* reference_point,
                                  const double* front, int num_front, const double* points_being_sampled, int num_being_sampled,
                                  const double* points, int num_points, int want_grad, double* value, double* grad, double* factors_out,
                                  moe_error_t* err);
/* moe_ehvi_constrained_mcmc_multistart with moe_log_ehvi_constrained_mcmc's objective: the same screening, top-20 rule, restarted
 * ascent and outputs, bit for bit the path a host loop over moe_log_ehvi_constrained_mcmc walks.  Tensor-product domains only.
 * Errors: that function's, in its order. */
int moe_log_ehvi_constrained_mcmc_multistart(const moe_gp_t* const* gps, const moe_gp_t* const* gps2,
                                             const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                             int num_mcmc, const double* reference_point, const double* front, int num_front,
                                             const moe_gd_params_t* outer, const double* domain_bounds,
                                             const double* points_being_sampled, int num_being_sampled, const double* starts,
                                             int num_starts, int do_gradient_ascent, double* best_point, double* best_value, int* found,
                                             double* start_values, int* kept_index, double* end_points, double* end_values,
                                             double* path, int* steps_taken, moe_error_t* err);
/* moe_ehvi_constrained_mcmc_suggest with moe_log_ehvi_constrained_mcmc's objective: num_to_sample points greedily, bit for bit what
 * num_to_sample calls of moe_log_ehvi_constrained_mcmc_multistart return when each is fed its predecessors' points.  Errors: that
 * function's, in its order. */
int moe_log_ehvi_constrained_mcmc_suggest(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* constraint_gps,
                                          int num_constraints, const double* thresholds, int num_mcmc, const double* reference_point,
                                          const double* front, int num_front, const moe_gd_params_t* outer,
                                          const double* domain_bounds, const double* points_being_sampled, int num_being_sampled,
                                          const double* starts, int num_starts, int do_gradient_ascent, int num_to_sample,
                                          double* best_points, double* best_values, int* found, moe_error_t* err);
/* The LOG of moe_ehvi3_constrained_mcmc's quantity (three objectives, 0 <= K = num_constraints <= 8; K = 0 is the log of
 * moe_ehvi3_mcmc's), computed so that it stays finite with a useful gradient where that value and its gradient are exactly 0 in
 * float64 -- with three psi factors sooner than with two.  Arguments, members, fronts, box tables, the join rule, the
 * believed-feasible rule for pending points and the limits are moe_ehvi3_constrained_mcmc's; sigma, lambda_r(t), lam, kap, the
 * feasibility terms, the member's sum and the ensemble's log-sum-exp are moe_log_ehvi_constrained_mcmc's.  For an objective r and
 * edges a < b the DIFFERENCE RULE is that function's strip rule:
 *   rho = exp(lambda_r(a) - lambda_r(b)),  log[psi_r(b) - psi_r(a)] = lambda_r(b) + log(1 - rho)  (log1p(-rho) for rho <= 1/2,
 *   log(-expm1(.)) above),  d/dmu_r = -(lam_b - rho lam_a) / (sigma_r (1 - rho)),  d/dvar_r = (kap_b - rho kap_a) / (2 sigma_r^2
 *   (1 - rho));  edges that do not give lambda_r(a) < lambda_r(b) in float64 carry weight 0.
 *   box b of the member's table (left, right, height, slab k):  l_b = ((log P) + lambda_2(height)) + log W_k, log P by the rule
 *                        from objective 1 at (left, right), log W_k from objective 3 at (w_k, w_{k+1}); every term of the plain
 *                        sum is P Q W >= 0, so no signed terms arise.  dl_b/d(mu_2, var_2) = (-lam / sigma_2, kap / (2 sigma_2^2))
 *                        at the height.  A box whose P or W has weight 0 is skipped, not evaluated; the box of slab 0 always counts.
 *   hypervolume term     L_e = log sum_b exp l_b as a log-sum-exp whose order depends on the member's table alone
 *                        (csrc/logehvi3.hip), its six coefficients (sum_b w_b dl_b/d.) / W_e.  Never clipped.
 *   member               LL_e = L_e + log F_{e,1} + ... + log F_{e,K};  g_e = ((((c_mu1 grad mu_1 + c_var1 grad var_1) + c_mu2 grad
 *                        mu_2) + c_var2 grad var_2) + c_mu3 grad mu_3) + c_var3 grad var_3, then + grad log F_{e,k} for k = 1 .. K
 * factors_out (may be NULL): [E][1 + K][num_points], L_e, log F_{e,1}, ..., log F_{e,K}; value[i] is what the ensemble rule makes
 * of them (with E = 1 their sum, bit for bit).  A candidate's bits do not depend on how many share the call, nor on want_grad, nor
 * on ensemble-wide launches.  No handle is modified.
 * Errors: moe_ehvi3_constrained_mcmc's, in its order and with its payloads. */
int moe_log_ehvi3_constrained_mcmc(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3,
                                   const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds, int num_mcmc,
                                   const double* reference_point, const double* front, int num_front, const double* points_being_sampled,
                                   int num_being_sampled, const double* points, int num_points, int want_grad, double* value, double* grad,
                                   double* factors_out, moe_error_t* err);
/* moe_ehvi3_constrained_mcmc_multistart with moe_log_ehvi3_constrained_mcmc's objective: the same screening, top-20 rule, restarted
 * ascent and outputs, bit for bit the path a host loop over moe_log_ehvi3_constrained_mcmc walks.  Tensor-product domains only.
 * Errors: that function's, in its order. */
int moe_log_ehvi3_constrained_mcmc_multistart(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3,
                                              const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                              int num_mcmc, const double* reference_point, const double* front, int num_front,
                                              const moe_gd_params_t* outer, const double* domain_bounds, const double* points_being_sampled,
                                              int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                              double* best_point, double* best_value, int* found, double* start_values, int* kept_index,
                                              double* end_points, double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* moe_ehvi3_constrained_mcmc_suggest with moe_log_ehvi3_constrained_mcmc's objective: num_to_sample points greedily, bit for bit
 * what num_to_sample calls of moe_log_ehvi3_constrained_mcmc_multistart return when each is fed its predecessors' points.  Errors:
 * that function's, in its order. */
int moe_log_ehvi3_constrained_mcmc_suggest(const moe_gp_t* const* gps, const moe_gp_t* const* gps2, const moe_gp_t* const* gps3,
                                           const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                           int num_mcmc, const double* reference_point, const double* front, int num_front,
                                           const moe_gd_params_t* outer, const double* domain_bounds, const double* points_being_sampled,
                                           int num_being_sampled, const double* starts, int num_starts, int do_gradient_ascent,
                                           int num_to_sample, double* best_points, double* best_values, int* found, moe_error_t* err);
/* The Chebyshev-scalarised expected improvement for 2 <= M = num_objectives <= 8 objectives (ParEGO, Knowles 2006; the analytic
 * one-point form of qParEGO, Daulton et al. 2020), averaged over a hyper-parameter ensemble, at points [num_points][dim], with
 * pending points.  Minimisation.  Member e is M GPs, objective_gps[e * M + j] (one flat array [E][M]), without derivative
 * observations; E M <= 1024.  scalarisations [R][2 M]: a_0 .. a_{M-1} > 0, then b_0 .. b_{M-1}, all finite (from weights w, an
 * ideal and a nadir point: a_j = w_j / (nadir_j - ideal_j), b_j = -a_j ideal_j); best_so_far [R][E]: the members' incumbents, the
 * smallest scalarised value observed, finite.  R = 1 here and in the multistart call.  With mu_j, var_j the posterior mean and the
 * conditioned latent variance of GP j at x, sigma_j = sqrt(max(150 eps^2, var_j)) for the value and the gradient alike,
 * s_j = a_j mu_j + b_j (product and sum each rounded), tau_j = a_j sigma_j, L = max_j (s_j - 38 tau_j):
 *   member value   A_e = E[(g*_e - max_j (a_j Y_j + b_j))^+] = integral over L <= t <= g*_e of prod_j Phi((t - s_j) / tau_j);
 *                  exactly 0, with zero coefficients, where g*_e <= L (L is a constant in the gradient)
 *   coefficients   dA/dmu_j = -a_j integral phi(z_j) / tau_j prod_{k != j} Phi(z_k),  dA/dvar_j = -(a_j / (2 sigma_j)) integral
 *                  z_j phi(z_j) / tau_j prod_{k != j} Phi(z_k),  z_j = (t - s_j) / tau_j; the products without j are formed from
 *                  prefix and suffix products, never by a division
 *   quadrature     FIXED: the 14 M + 2 breakpoints s_j + c tau_j, c in {-38, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8}, each
 *                  clamped to [L, g*_e], with L and g*_e, sorted ascending (list position 14 j + the place of c, then L, then
 *                  g*_e, breaks ties); on each of the 14 M + 1 panels the 8-point Gauss-Legendre rule; a panel of zero width
 *                  contributes an exact 0.  The sum's order depends on M alone (csrc/chebei1.hip).
 *   ensemble       value[i] = (A_0 + ... + A_{E-1}) / E; grad: per member sum_j (c_mu_j grad mu_j + c_var_j grad var_j) in the order
 *                  of j, mu before var; members added in member order and divided once
 * Pending points: the variances of all M GPs are conditioned on them (the means are left alone); member e keeps the believed
 * outcomes mu_{e,j}(P_i) and its incumbent is g*_e = min(best_so_far[e], min_i max_j (a_j mu_{e,j}(P_i) + b_j)) over the pending
 * points whose scalarised outcome is finite.
 * member_values_out (may be NULL): [E][num_points], every A_e; value[i] is, bit for bit, their mean formed in member order on the
 * host.  A candidate's bits do not depend on how many share the call, nor on want_grad, nor on ensemble-wide launches.  No handle
 * is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_objectives outside 2 .. 8
 * -> MOE_ERR_BOUNDS, payload (num_objectives, 2, 8); num_mcmc < 1 or num_mcmc num_objectives > 1024 -> MOE_ERR_BOUNDS, payload
 * (num_mcmc, 1, 1024 / num_objectives rounded down); a NULL array (objective_gps, scalarisations, best_so_far, points, value, grad
 * with want_grad) -> MOE_ERR_RUNTIME; an a_j that is not positive, or an a_j or b_j that is not finite -> MOE_ERR_INVALID_VALUE,
 * payload (the value, its flat index in scalarisations, 0); an incumbent that is not finite -> MOE_ERR_INVALID_VALUE, payload (the
 * value, its flat index in best_so_far, 1); num_points < 1 -> MOE_ERR_BOUNDS; num_being_sampled outside 0 .. 64 -> MOE_ERR_BOUNDS;
 * points_being_sampled NULL with num_being_sampled > 0 -> MOE_ERR_RUNTIME; then, "member" counting the GPs flat as e M + j: a NULL
 * handle -> MOE_ERR_RUNTIME; a GP of another dim, then of another device -> MOE_ERR_INVALID_VALUE; a GP with derivative
 * observations -> MOE_ERR_INVALID_VALUE, payload (its num_derivatives, 0, the flat index); a handle listed twice ->
 * MOE_ERR_INVALID_VALUE.  MOE_ERR_SINGULAR only for a pending point: payload (the flat index of the first failing GP, the pending
 * point).  A candidate never raises. */
int moe_ei_chebyshev_mcmc(const moe_gp_t* const* objective_gps, int num_objectives, int num_mcmc, const double* scalarisations,
                          const double* best_so_far, const double* points_being_sampled, int num_being_sampled, const double* points,
                          int num_points, int want_grad, double* value, double* grad, double* member_values_out, moe_error_t* err);
/* One suggestion by moe_ei_chebyshev_mcmc's objective, the whole loop on the device, as moe_ehvi3_mcmc_multistart is for
 * moe_ehvi3_mcmc: the path is, bit for bit, the one a host loop over moe_ei_chebyshev_mcmc walks.  Tensor-product domains only.
 * Errors, in this order: those of moe_ei_chebyshev_mcmc that need no handle (outer, domain_bounds, starts, best_point, best_value
 * and found among the arrays that must not be NULL; num_starts for num_points); max_num_steps < 1 with do_gradient_ascent != 0 ->
 * MOE_ERR_BOUNDS; domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_INVALID_VALUE; then those that need the handles. */
int moe_ei_chebyshev_mcmc_multistart(const moe_gp_t* const* objective_gps, int num_objectives, int num_mcmc,
                                     const double* scalarisations, const double* best_so_far, const moe_gd_params_t* outer,
                                     const double* domain_bounds, const double* points_being_sampled, int num_being_sampled,
                                     const double* starts, int num_starts, int do_gradient_ascent, double* best_point,
                                     double* best_value, int* found, double* start_values, int* kept_index, double* end_points,
                                     double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* num_to_sample points greedily with a scalarisation of its own per point: scalarisations [num_to_sample][2 M] and best_so_far
 * [num_to_sample][E].  Round t is moe_ei_chebyshev_mcmc_multistart from the same starts with scalarisation t, row t of best_so_far
 * and pending points = points_being_sampled followed by the picks of the rounds before -- bit for bit what num_to_sample calls of
 * that function return when each is fed its predecessors' points.  Staged once; a round appends ONE row to the extension of each
 * of the E M GPs and the pick's believed outcomes to every member's list, from which the round's incumbents are formed, inside
 * device memory.
 * Errors: those of moe_ei_chebyshev_mcmc_multistart, every row of scalarisations and best_so_far checked (num_to_sample < 1 reads
 * as one row there), with num_to_sample < 1 or num_being_sampled + num_to_sample - 1 > 64 -> MOE_ERR_BOUNDS behind
 * num_being_sampled. */
int moe_ei_chebyshev_mcmc_suggest(const moe_gp_t* const* objective_gps, int num_objectives, int num_mcmc, const double* scalarisations,
                                  const double* best_so_far, const moe_gd_params_t* outer, const double* domain_bounds,
                                  const double* points_being_sampled, int num_being_sampled, const double* starts, int num_starts,
                                  int do_gradient_ascent, int num_to_sample, double* best_points, double* best_values, int* found,
                                  moe_error_t* err);
/* The LOG of moe_ei_chebyshev_mcmc's quantity with 0 <= K = num_constraints <= 8 constraints, computed so that it stays finite with
 * a useful gradient where that value and its gradient are exactly 0 in float64 (the incumbent at or below L, or a product of M
 * normal CDFs too small to tell the starts of an ascent apart).  Minimisation.  Member e is M + K GPs without derivative
 * observations: its objectives objective_gps[e * M + j] ([E][M]), then its constraint GPs constraint_gps[k * E + e] ([K][E]; may
 * be NULL with K = 0), constraint k satisfied where c_k(x) <= thresholds[k]; E (M + K) <= 1024.  scalarisations and best_so_far
 * as in moe_ei_chebyshev_mcmc, best_so_far being the incumbents of the FEASIBLE observations.  Every incumbent must be finite:
 * the integral's upper limit is the incumbent, so a caller without a feasible observation passes a finite cap of its own (the
 * Python wrapper takes the largest scalarised observation).  With that function's s_j, tau_j, sigma_j, L and the incumbent g:
 *   integrand      z_j(t) = (t - s_j) / tau_j, log f(t) = sum_j log Phi(z_j(t)) added in the order of j, r_j = phi(z_j) / Phi(z_j)
 *   decay length   ell = min(1 / sum_j (r_j(g) / tau_j), max_j tau_j): f is log-concave, so f(t) <= f(g) exp((t - g) sum_j r_j(g) /
 *                  tau_j) below g; the cap binds only where f does not decay at g
 *   member         LA_e = log integral over Lambda <= t <= g of f, Lambda = min(L, g - 40 ell): finite for every finite input,
 *                  there is no `g <= L` branch.  dLA/dmu_j = -a_j <r_j / tau_j>, dLA/dvar_j = -(a_j / (2 sigma_j)) <z_j r_j /
 *                  tau_j>, <.> the f-weighted mean over [Lambda, g], accumulated as signed sums of scaled terms.  Lambda and
 *                  the breakpoints are constants in the gradient (Lambda's boundary term is below e^-40 relative).
 *   quadrature     FIXED, and formed in OFFSETS u = g - t below the incumbent from d_j = g - s_j (rounded once), z_j = (d_j - u) /
 *                  tau_j, so that no node is lost where ell lies below an ulp of g (a floored sigma_j under an s_j above the
 *                  incumbent): moe_ei_chebyshev_mcmc's 14 M breakpoints, d_j - c tau_j, and the ladder kappa ell, kappa in {1/2, 1,
 *                  2, 3, 4.5, 6, 8, 10.5, 13, 16, 20, 24, 29, 34}, each clamped to [0, U], U = g - Lambda = max(min_j (d_j + 38
 *                  tau_j), 40 ell), with U and 0: 14 M + 16 points sorted ascending in the offset (list position breaks ties:
 *                  objectives, ladder, U, 0); the 8-point Gauss-Legendre rule per
 *                  panel; the nodes' terms log(weight) + log f enter a log-sum-exp whose order depends on M alone
 *                  (csrc/logchebei1.hip)
 *   feasibility    log F_{e,k} and its derivatives: moe_log_ehvi_constrained_mcmc's
 *   ensemble       LL_e = LA_e + log F_{e,1} + ... + log F_{e,K};  m = max_e LL_e, value = m + log(sum_e exp(LL_e - m)) - log E;
 *                  grad = sum_e w_e g_e / sum_e w_e with g_e = sum_j (c_mu_j grad mu_j + c_var_j grad var_j) in the order of j,
 *                  mu before var, then + grad log F_{e,k} for k = 1 .. K.  With E = 1 the value is LL_0 bit for bit.
 * Pending points condition every GP's variance; member e keeps the believed outcomes mu_{e,j}(P_i), and P_i's scalarised outcome
 * lowers its incumbent only where the member believes the point feasible, mu_{e,c_k}(P_i) <= thresholds[k] for every k (K = 0:
 * moe_ei_chebyshev_mcmc's rule bit for bit).
 * factors_out (may be NULL): [E][1 + K][num_points], LA_e, log F_{e,1}, ..., log F_{e,K}; value[i] is what the ensemble rule makes
 * of them: with E = 1 their sum, bit for bit; with more members the rule takes exp and log, which a host's library and the
 * device's round alike only within a unit in the last place, so a host's value agrees within a few units in the last place of
 * max(1, |value|), not in every bit.  A candidate's bits do not depend on how many share the call, nor on want_grad, nor on
 * ensemble-wide launches.  No handle is modified.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: num_objectives outside 2 .. 8
 * -> MOE_ERR_BOUNDS, payload (num_objectives, 2, 8); num_constraints outside 0 .. 8 -> MOE_ERR_BOUNDS, payload (num_constraints,
 * 0, 8); num_mcmc < 1 or num_mcmc (M + K) > 1024 -> MOE_ERR_BOUNDS, payload (num_mcmc, 1, 1024 / (M + K) rounded down); a NULL
 * array (moe_ei_chebyshev_mcmc's, and constraint_gps and thresholds with K > 0) -> MOE_ERR_RUNTIME; an a_j that is not positive,
 * or an a_j or b_j that is not finite -> MOE_ERR_INVALID_VALUE, payload (the value, its flat index in scalarisations, 0); a
 * threshold that is not finite -> MOE_ERR_INVALID_VALUE, payload (the value, k, 2); an incumbent that is not finite, +infinity
 * included -> MOE_ERR_INVALID_VALUE, payload (the value, its flat index in best_so_far, 1); then moe_ei_chebyshev_mcmc's from
 * num_points on, "member" counting the GPs flat as e (M + K) + role. */
int moe_log_ei_chebyshev_constrained_mcmc(const moe_gp_t* const* objective_gps, int num_objectives, const moe_gp_t* const* constraint_gps,
                                          int num_constraints, const double* thresholds, int num_mcmc, const double* scalarisations,
                                          const double* best_so_far, const double* points_being_sampled, int num_being_sampled,
                                          const double* points, int num_points, int want_grad, double* value, double* grad,
                                          double* factors_out, moe_error_t* err);
/* moe_ei_chebyshev_mcmc_multistart with moe_log_ei_chebyshev_constrained_mcmc's objective: the same screening, top-20 rule,
 * restarted ascent and outputs, bit for bit the path a host loop over moe_log_ei_chebyshev_constrained_mcmc walks.  Tensor-product
 * domains only.  Errors: those two functions', in their order. */
int moe_log_ei_chebyshev_constrained_mcmc_multistart(const moe_gp_t* const* objective_gps, int num_objectives,
                                                     const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                                     int num_mcmc, const double* scalarisations, const double* best_so_far,
                                                     const moe_gd_params_t* outer, const double* domain_bounds,
                                                     const double* points_being_sampled, int num_being_sampled, const double* starts,
                                                     int num_starts, int do_gradient_ascent, double* best_point, double* best_value,
                                                     int* found, double* start_values, int* kept_index, double* end_points,
                                                     double* end_values, double* path, int* steps_taken, moe_error_t* err);
/* moe_ei_chebyshev_mcmc_suggest with moe_log_ei_chebyshev_constrained_mcmc's objective: num_to_sample points greedily with a
 * scalarisation and incumbents per point, bit for bit what num_to_sample calls of moe_log_ei_chebyshev_constrained_mcmc_multistart
 * return when each is fed its predecessors' points; a pick lowers a member's incumbent only where the member believes it
 * feasible.  Errors: those functions', in their order. */
int moe_log_ei_chebyshev_constrained_mcmc_suggest(const moe_gp_t* const* objective_gps, int num_objectives,
                                                  const moe_gp_t* const* constraint_gps, int num_constraints, const double* thresholds,
                                                  int num_mcmc, const double* scalarisations, const double* best_so_far,
                                                  const moe_gd_params_t* outer, const double* domain_bounds,
                                                  const double* points_being_sampled, int num_being_sampled, const double* starts,
                                                  int num_starts, int do_gradient_ascent, int num_to_sample, double* best_points,
                                                  double* best_values, int* found, moe_error_t* err);
/* compute_grad_variance_of_points -> ComputeGradVarianceOfPoints (gpp_math.cpp:1359-1373); out[num_derivs][m][m][dim] */
int moe_gp_grad_variance(const moe_gp_t* gp, const double* pts, int num_pts, int num_derivs, double* out, moe_error_t* err);
/* compute_grad_cholesky_variance_of_points -> ComputeGradCholeskyVarianceOfPoints (gpp_math.cpp:1454-1474) */
int moe_gp_grad_cholesky_variance(const moe_gp_t* gp, const double* pts, int num_pts, int num_derivs, double* out,
                                  moe_error_t* err);

/* compute_posterior_mean / compute_grad_posterior_mean (gpp_python_knowledge_gradient.cpp:44-72 ->
 * PosteriorMeanEvaluator, gpp_knowledge_gradient_optimization.cpp:322-351). point[dim - num_fidelity];
 * value = -mu(point, fidelity coords = 1); grad[dim - num_fidelity] = -grad mu. Either output may be NULL. */
int moe_posterior_mean(const moe_gp_t* gp, int num_fidelity, const double* point, double* value, double* grad,
                       moe_error_t* err);

/* ---- normal draws ----
 * Fills out[count] with N(0,1) draws: the host-side stand-in for NormalRNG(seed) (gpp_random.hpp:204-303 = boost::mt19937 +
 * boost::normal_distribution).  The engine is bit-identical to std::mt19937; boost::normal_distribution's algorithm is
 * Boost-version dependent and the reference pins no draws, so parity with an arbitrary Boost is NOT claimed.
 * The stream IS, draw for draw, that of the reference as it builds in this repository (oracle/_ref, Boost shimmed onto the
 * C++ standard library: Marsaglia's polar method over generate_canonical<double, 53>) -- pinned by tests/test_oracle.py and
 * the committed fixture tests/golden/ref_kg_multistart.npz (keys stream_seeds / stream_draws) -- so a seeded RandomnessSourceContainer run reproduces that
 * build's results; cross-implementation parity runs still pass explicit tables. */
int moe_normal_draws(unsigned int seed, long long count, double* out);

/* ---- q,p-EI by Monte Carlo: compute_expected_improvement / compute_grad_expected_improvement
 * (gpp_python_expected_improvement.cpp:44-109 -> ExpectedImprovementEvaluator, gpp_math.cpp:1991-2126).
 * normals[num_mc][q+p] is the explicit N(0,1) table (row i feeds sample i, the role NormalRNGSimulator plays in the
 * reference's tests, gpp_random.hpp:314-340).  ei and/or grad_ei[q*dim] may be NULL. */
int moe_ei(const moe_gp_t* gp, const double* points_to_sample, const double* points_being_sampled, int num_to_sample,
           int num_being_sampled, int num_mc, double best_so_far, const double* normals, double* ei, double* grad_ei,
           moe_error_t* err);

/* Batched form: `num_evals` independent points_to_sample sets (points_to_sample_all[e][q][dim]) against the same
 * points_being_sampled and normal table -- evaluate_EI_at_point_list (gpp_python_expected_improvement.cpp:401-440 ->
 * EvaluateEIAtPointList, gpp_math.hpp:1900-1950).  ei[num_evals] and/or grad_ei[num_evals][q*dim] may be NULL. */
int moe_ei_batch(const moe_gp_t* gp, const double* points_to_sample_all, int num_evals, const double* points_being_sampled,
                 int num_to_sample, int num_being_sampled, int num_mc, double best_so_far, const double* normals,
                 double* ei, double* grad_ei, moe_error_t* err);

/* Analytic 1,0-EI and its gradient at `num_evals` single points (points[num_evals][dim]) --
 * OnePotentialSampleExpectedImprovementEvaluator::Compute[Grad]ExpectedImprovement (gpp_math.cpp:2195-2259), the evaluator
 * the reference's multistart / point-list drivers take when num_to_sample == 1 and num_being_sampled == 0
 * (gpp_math.hpp:1703, gpp_math.cpp:2317).  ei[num_evals] and/or grad_ei[num_evals][dim] may be NULL. */
int moe_ei_analytic_batch(const moe_gp_t* gp, const double* points, int num_evals, double best_so_far, double* ei,
                          double* grad_ei, moe_error_t* err);

/* q,p-EI optimisation from caller-supplied starts (start_points[num_starts][q][dim]) --
 * ComputeOptimalPointsToSampleViaMultistartGradientDescent (gpp_math.hpp:1683-1800: EI at every start, best 20 kept,
 * restarted gradient ascent on each, best end point returned) when do_gradient_ascent != 0, EvaluateEIAtPointList
 * (gpp_math.cpp:2305-2356: best start by value) otherwise; behind multistart_expected_improvement_optimization
 * (gpp_python_expected_improvement.cpp:221-276).  q == 1 && p == 0 uses the analytic evaluator (normals may be NULL);
 * otherwise normals[num_mc][q+p] is replayed by every evaluation.  Tensor-product domain: domain_bounds[2*dim] applies to
 * each of the q points.  *found = 1 when some end point beats -1.0, the reference's starting best (gpp_math.hpp:1728). */
int moe_ei_multistart(const moe_gp_t* gp, const moe_gd_params_t* outer_params, const double* domain_bounds,
                      const double* start_points, int num_starts, const double* points_being_sampled, int num_to_sample,
                      int num_being_sampled, int num_mc, double best_so_far, const double* normals, int do_gradient_ascent,
                      double* best_points, double* best_ei, int* found, moe_error_t* err);

/* ---- q-KG / d-KG by Monte Carlo: compute_knowledge_gradient / compute_grad_knowledge_gradient
 * (gpp_python_knowledge_gradient.cpp:74-154 -> KnowledgeGradientEvaluator<TensorProductDomain>,
 * gpp_knowledge_gradient_optimization.cpp:69-227, state :246-317, inner optimisation :420-472,
 * gpp_optimization.hpp:708-828/1242-1283, gpp_domain.cpp:64-105).
 *   domain_bounds[2*(dim-num_fidelity)] = [min0,max0,...]; discrete_pts[num_pts][dim-num_fidelity];
 *   normals[ceil(num_mc/2)][m], m = (q+p)(1+g): even sample 2j uses row j, odd sample 2j+1 uses -row j
 *   (antithetic pairs, .cpp:171-180);
 *   first_sample/num_local select the contiguous, even-aligned slice [first_sample, first_sample+num_local) of the MC
 *   samples this call evaluates (multi-GPU sharding); pass 0,num_mc for the whole evaluation.
 * Outputs: kg_sum = SUM over the local samples of (best_posterior + best_function_value) (divide by num_mc after the
 * cross-rank sum); grad_sum[q*dim] likewise un-normalised, the winner term M*grad_mu (.cpp:157-161) being added only
 * by the call with first_sample == 0; best_points[num_local][dim] (may be NULL); stats (may be NULL).
 * want_grad = 0 reproduces ComputeKnowledgeGradient (value only). */
int moe_kg(const moe_gp_t* gp, int num_fidelity, const moe_gd_params_t* inner_params, const double* domain_bounds,
           const double* discrete_pts, int num_pts, const double* points_to_sample, const double* points_being_sampled,
           int num_to_sample, int num_being_sampled, int num_mc, double best_so_far, const double* normals,
           int first_sample, int num_local, int want_grad, double* kg_sum, double* grad_sum, double* best_points,
           moe_kg_stats_t* stats, moe_error_t* err);

/* Batched form: `num_evals` independent evaluations (different points_to_sample[e][q][dim], same GP / discrete set /
 * normals) in one pass -- the multistart axis of ComputeKGOptimalPointsToSampleViaMultistartGradientDescent
 * (gpp_knowledge_gradient_optimization.hpp:860-935) and EvaluateKGAtPointList (:1090-1141).
 * kg_sum[num_evals], grad_sum[num_evals][q*dim]. */
int moe_kg_batch(const moe_gp_t* gp, int num_fidelity, const moe_gd_params_t* inner_params, const double* domain_bounds,
                 const double* discrete_pts, int num_pts, const double* points_to_sample_all, int num_evals,
                 const double* points_being_sampled, int num_to_sample, int num_being_sampled, int num_mc,
                 double best_so_far, const double* normals, int first_sample, int num_local, int want_grad,
                 double* kg_sum, double* grad_sum, moe_kg_stats_t* stats, moe_error_t* err);

/* ---- one node, several devices, from a plain C/C++ host (SURVEY 8b "multistart drivers taking num_devices"; the axis the
 * reference runs as OpenMP iterations, gpp_optimization.hpp:1472-1546).  gps[num_devices] are handles of the SAME GP built on
 * different devices (moe_gp_create with device = 0 .. num_devices-1; distinct handles on one device are accepted too); one
 * host thread per handle drives its device.
 *   shard_mode 0 (restarts): evaluation e runs whole on handle e % num_devices; results equal moe_kg_batch's bit for bit
 *     (which kernel an evaluation takes is decided from the training set, points_being_sampled and the domain box alone --
 *     never from the other evaluations of its batch -- as long as its points_to_sample lie inside domain_bounds).
 *   shard_mode 1 (MC samples): every handle evaluates every point set on its contiguous EVEN-ALIGNED slice of the samples and
 *     the per-handle sums are added on the host in handle order (a fixed-order reduction of num_evals x (1 + q d) doubles).
 * Outputs as moe_kg_batch (un-normalised sums over all num_mc samples); stats: pass counts summed, times = the slowest
 * handle's.  The multi-PROCESS equivalent (one rank per GPU, RCCL) is cornell_moe_amd/dist.py. */
int moe_kg_batch_multi(const moe_gp_t* const* gps, int num_devices, int shard_mode, int num_fidelity,
                       const moe_gd_params_t* inner_params, const double* domain_bounds, const double* discrete_pts, int num_pts,
                       const double* points_to_sample_all, int num_evals, const double* points_being_sampled,
                       int num_to_sample, int num_being_sampled, int num_mc, double best_so_far, const double* normals,
                       int want_grad, double* kg_sum, double* grad_sum, moe_kg_stats_t* stats, moe_error_t* err);

/* ---- callers of the hot path: the outer optimisation over points_to_sample ----
 * multistart_knowledge_gradient_optimization (gpp_python_knowledge_gradient.cpp:243-313) ->
 * ComputeKGOptimalPointsToSampleViaMultistartGradientDescent (gpp_knowledge_gradient_optimization.hpp:860-935) when
 * do_gradient_ascent != 0: KG at every start, best 20 kept, restarted gradient ascent with `outer_params`
 * (gpp_optimization.hpp:619-705, 1144-1185), best end point returned; with do_gradient_ascent == 0 the value search of
 * ...ViaLatinHypercubeSearch / EvaluateKGAtPointList (:1090-1141).  start_points[num_starts][q][dim] are supplied by
 * the caller (moe_latin_hypercube reproduces the reference's generator, gpp_random.cpp:173-194); domain_bounds[2*dim].
 * Every step evaluates all live restarts in ONE batched device pass.  *found = 1 iff a point with KG > -inf was found.
 * Reproduced from the reference, because they decide which point is returned (pinned to the reference's own end points,
 * tests/golden/ref_kg_multistart.npz): (1) the drivers build their KnowledgeGradientState at the FIRST start and move it with
 * SetCurrentPoint, which does not refresh the state's discretised set (gpp_knowledge_gradient_optimization.cpp:232-243,
 * 259-261): every evaluation of a run scores / starts its inner optimisation from start_points[0]'s q points (+ the
 * points being sampled + discrete_pts), not from the points being evaluated -- moe_kg / moe_kg_batch, like the
 * single-evaluation Python entry points, evaluate on a fresh state; (2) the best 20 starts are kept and walked in the order
 * the reference's std::priority_queue pops them (lowest kept value first, equal values by descending index), and the first
 * of equal end values wins. */
int moe_kg_multistart(const moe_gp_t* gp, int num_fidelity, const moe_gd_params_t* outer_params,
                      const moe_gd_params_t* inner_params, const double* domain_bounds, const double* discrete_pts, int num_pts,
                      const double* start_points, int num_starts, const double* points_being_sampled, int num_to_sample,
                      int num_being_sampled, int num_mc, double best_so_far, const double* normals, int do_gradient_ascent,
                      double* best_points, double* best_kg, int* found, moe_error_t* err);
/* The outer-optimisation drivers (moe_kg_multistart, moe_kg_mcmc_multistart) reproduce the reference's EXECUTION by default --
 * the frozen discretised set, and for KG-MCMC the partially-updated state and the accumulating gradient described at
 * moe_kg_mcmc_multistart -- because the bar of this library is "the reference's results on the reference's inputs".  Those
 * behaviours are defects of the reference's drivers, and for q > 1 the KG-MCMC one optimises only the first point.  Switch:
 *   moe_set_reference_quirks(0)  (or MOE_REFERENCE_QUIRKS=0 in the environment)  -> the drivers as the reference intends them:
 *     every evaluation on a fresh state, all q points move and are returned, the plain gradient at every step;
 *   moe_set_reference_quirks(1)  -> bug-compatible (the default);  moe_set_reference_quirks(-1) -> back to the environment.
 * Process-wide; the single-evaluation entry points (moe_kg, moe_kg_batch, moe_kg_mcmc_batch) are unaffected: they always build
 * a fresh state per call, as the reference's Python boundary does. */
int moe_set_reference_quirks(int on);
int moe_get_reference_quirks(void);
/* Ensemble-wide launches (r6): the MCMC-averaged KG entry points (moe_kg_mcmc_batch, moe_kg_mcmc_multistart and their _comm
 * forms: KnowledgeGradientMCMCEvaluator, gpp_knowledge_gradient_mcmc_optimization.cpp:129-180, evaluates the ensemble members one
 * after another; and moe_ei_mcmc_batch / moe_ei_mcmc_multistart for Monte-Carlo EI) record every member's chain of kernels and issue each kernel ONCE for all members of the ensemble; same bits as
 * member-by-member launches.  moe_set_ensemble_launches(0) -> member by member (MOE_ENS_LAUNCH=0 in the environment does the same),
 * (1) -> on (the default), (-1) -> back to the environment.  moe_ensemble_launch_stats: out[0] = evaluations of an ensemble that
 * went down merged, out[1] = that fell back to member-by-member launches, out[2] = kernel launches issued by merged evaluations,
 * out[3] = member launches they stand for.  Process-wide. */
int moe_set_ensemble_launches(int on);
int moe_ensemble_launch_stats(long long* out4);
/* posterior_mean_optimization (gpp_python_knowledge_gradient.cpp:315-342) -> ComputeOptimalPosteriorMean from ONE initial
 * guess: line-search ascent on -mu with fidelity coordinates pinned to 1.  best_point[dim - num_fidelity]. */
int moe_posterior_mean_optimize(const moe_gp_t* gp, int num_fidelity, const moe_gd_params_t* params, const double* domain_bounds,
                                const double* initial_guess, double* best_point, double* best_value, moe_error_t* err);
/* ComputeLatinHypercubePointsInDomain (gpp_random.cpp:173-194) with mt19937(seed): out[num_points][dim]. */
int moe_latin_hypercube(unsigned int seed, const double* domain_bounds, int dim, int num_points, double* out);

/* ---- MCMC-averaged evaluators: the acquisition averaged over `num_mcmc` GPs built on the same data, one
 * per hyper-parameter sample -- GaussianProcessMCMC (gpp_knowledge_gradient_mcmc_optimization.cpp:24-49; Python ctor
 * gpp_python_knowledge_gradient_mcmc.cpp:45-75).  `gps` is an array of num_mcmc handles from moe_gp_create (the caller owns
 * them; they must share dim and the observed-derivative list).  best_so_far[num_mcmc] is per GP; every GP replays the same
 * normal table. ----
 * compute_knowledge_gradient_mcmc / compute_grad_knowledge_gradient_mcmc / evaluate_KG_mcmc_at_point_list
 * (gpp_python_knowledge_gradient_mcmc.cpp:77-190, 400-470 -> KnowledgeGradientMCMCEvaluator, .cpp:51-180) for `num_evals`
 * point sets points_to_sample_all[num_evals][q][dim]; discrete_pts_all[num_mcmc][num_pts][dim - num_fidelity].
 * finalize != 0: kg[e] = mean_i KG_i / cost, grad likewise with the cost-gradient term (cost = largest product of the
 * fidelity coordinates over the q points, 1 when num_fidelity == 0; .cpp:84-127), normalised by total_num_mcmc.
 * finalize == 0: plain sums over the GPs given -- the GP-index shard of a multi-GPU evaluation, to be all-reduced and then
 * passed through moe_kg_mcmc_finalize.  grad_kg may be NULL (value only). */
int moe_kg_mcmc_batch(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* inner_params,
                      const double* domain_bounds, const double* discrete_pts_all, int num_pts,
                      const double* points_to_sample_all, int num_evals, const double* points_being_sampled, int num_to_sample,
                      int num_being_sampled, int num_mc, const double* best_so_far, const double* normals, int finalize,
                      int total_num_mcmc, double* kg, double* grad_kg, moe_error_t* err);
int moe_kg_mcmc_finalize(double* kg, double* grad_kg, const double* points_to_sample_all, int num_evals, int num_to_sample,
                         int dim, int num_fidelity, int total_num_mcmc);
/* ---- the ensemble-averaged posterior mean and the recommendation step (examples/main.py:142-157, 243-260) ----
 * PosteriorMeanMCMC.compute_posterior_mean_mcmc / compute_grad_posterior_mean_mcmc (cpp_wrappers/knowledge_gradient_mcmc.py:109-155)
 * at num_points points[num_points][dim - num_fidelity] in one launch, one copy down, one wait and one copy back:
 *   value_out[p] = -(1 / num_mcmc) sum_e mu_e(point_p, fidelity coordinates = 1), grad_out[p][dim - num_fidelity] its gradient over
 * the free coordinates -- the sign and fidelity conventions of moe_posterior_mean.  The members are summed in ascending order and
 * the sum is then divided by num_mcmc, as the reference does.  Either output may be NULL.
 * The members must share dim, the sampled points and the observed-derivative list, and live on one device (MOE_ERR_INVALID_VALUE
 * otherwise, as moe_kg_mcmc_batch).  Every reduction has a fixed order: the bits of a point's result depend neither on its
 * neighbours nor on num_points.  Points go through in launches of 16 384, whatever (N, num_mcmc, num_points).  No limit on
 * num_points or num_mcmc beyond memory; dim <= 32 and num_derivatives <= 12 as everywhere.  No handle is modified.
 * Errors: gps or points NULL, a NULL handle -> MOE_ERR_RUNTIME; num_mcmc < 1, num_points < 1, num_fidelity outside [0, dim) ->
 * MOE_ERR_BOUNDS. */
int moe_posterior_mean_mcmc_batch(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const double* points, int num_points,
                                  double* value_out, double* grad_out, moe_error_t* err);
/* The whole recommendation on the device: one copy down, one stream of kernels, one wait, one copy back; no handle is modified.
 * size = dim - num_fidelity, f = the objective of moe_posterior_mean_mcmc_batch, candidates[num_candidates][size].
 *   1. screen: f at every candidate (candidate_values_out); i0 = *screened_index_out = the first index of the largest f
 *      (numpy.argmin of the averaged mean, main.py:252);
 *   2. starts: the num_starts candidates with the largest f, equal values by index (the reference: num_starts = 1, candidate i0).
 *      NaN values are never picked: neither i0 nor a start is a candidate whose f is NaN while a candidate with a number is left
 *      (with nothing left to pick a round answers candidate 0);
 *   3. descent from each start, python_version/optimization.py GradientDescentOptimizer.optimize (:444-527) literally: x_0 = the
 *      start; for i = 1 .. T = max_num_steps: a_i = pre_mult i^-gamma (computed on the host with pow), step = a_i grad f(x_{i-1}),
 *      each coordinate limited as python_version/domain.py:187-200 (dist = fmin(x - lo, hi - x); |step| > max_relative_change dist
 *      -> step = copysign(max_relative_change dist, step)), x_i = x_{i-1} + step.  The end point is the mean of the last k steps,
 *      _get_averaging_range's k (:416-442): num_steps_averaged < 0 or > T -> T, 0 -> 1; x_0 is never included.
 *      max_num_restarts, tolerance and num_multistarts are IGNORED, as the reference's Python optimiser ignores them: no restarts,
 *      no tolerance stop;
 *   4. pick: f at every end point; the winner is the first of the largest (MultistartOptimizer.optimize's strict compare, :595-603);
 *   5. keep or fall back (main.py:259-260): -f(winner) > -f(candidate i0) -> point_out = candidate i0, *refined_out = 0; otherwise
 *      point_out = the winner, *refined_out = 1.  *value_out = f(point_out).
 * point_out[size]; end_points_out[num_starts][size] and path_out[num_starts][max_num_steps + 1][size] (x_0 .. x_T of every start)
 * may be NULL, as may value_out, screened_index_out, refined_out and candidate_values_out.
 * The descent of a start belongs to one workgroup: its bits do not depend on the other starts in the call.
 * Errors, in this order: gps NULL -> MOE_ERR_RUNTIME; num_mcmc < 1 -> MOE_ERR_BOUNDS; gd, domain_bounds, candidates or point_out
 * NULL -> MOE_ERR_RUNTIME; num_candidates < 1, num_starts outside [1, num_candidates], max_num_steps < 1, domain_type other than
 * MOE_DOMAIN_TENSOR_PRODUCT (only tensor-product domains are supported), num_fidelity outside [0, dim) -> MOE_ERR_BOUNDS; a NULL
 * handle -> MOE_ERR_RUNTIME; mismatched members as above. */
int moe_posterior_mean_mcmc_recommend(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* gd,
                                      const double* domain_bounds, const double* candidates, int num_candidates, int num_starts,
                                      double* point_out, double* value_out, int* screened_index_out, int* refined_out,
                                      double* candidate_values_out, double* end_points_out, double* path_out, moe_error_t* err);
/* ---- every member's own posterior-mean minimiser: the per-member discretisation of a KG-MCMC iteration (examples/main.py:172-197) ----
 * For each of the num_mcmc members BY ITSELF (nothing is averaged), in one device call -- one copy down, one stream of kernels, one
 * wait, one copy back; no handle is modified.  size = dim - num_fidelity; mu_e = member e's posterior mean of the function value with
 * the num_fidelity trailing coordinates pinned to 1 (the POSITIVE mean: no sign flip on the outputs).
 *   1. screen: mu_e at each of num_candidates candidates -- candidates[num_candidates][size] shared by the members (per_member == 0)
 *      or candidates[num_mcmc][num_candidates][size], member e's own set (per_member != 0).  start_index[e] = the first index of the
 *      smallest mu_e (numpy.argmin's rule: a NaN counts as smaller than every number).  means_out[num_mcmc][num_candidates] (may be
 *      NULL) are the screened means.  Candidates go through in launches of 16 384 per member.
 *   2. descend: ComputeOptimalPosteriorMean from that candidate, with the decisions of moe_posterior_mean_optimize in its order:
 *      for r < max_num_restarts, for i < max_num_steps: f0, g = value and gradient of f = -mu_e at x; alpha = pre_mult (i + 1)^-gamma
 *      (a table computed on the host with pow); at most 30 trials x + alpha g, accepted when f_trial - f0 > alpha |g|^2 / 2, alpha
 *      halved otherwise; the step alpha g limited per coordinate by TensorProductDomain::LimitUpdate (max_relative_change; halved
 *      when it would leave the domain); no move and the end of the restart when all 30 trials failed or the limited step is zero;
 *      f re-evaluated at x + step when the limiter changed the step; the end of the restart when that value <= f0; otherwise x +=
 *      step, and the end of the restart when |step| < tolerance / max_num_steps.  After a restart: stop unless it moved x by more
 *      than tolerance.
 *   3. keep or fall back (main.py:191-193): mu_e(end) > mu_e(start candidate) -> best_points[e] = that candidate, fell_back[e] = 1;
 *      otherwise best_points[e] = the end point, fell_back[e] = 0.  best_values[e] = mu_e(best_points[e]).
 *      A step of 2. is taken only after f rose (the trial test, and value > f0 where the limiter changed the step), so mu_e(end) <=
 *      mu_e(start) by construction: fell_back[e] = 1 is unreachable short of a rounding error as large as the whole improvement.
 *      The rule is kept because the reference keeps it.
 * best_points[num_mcmc][size]; best_values[num_mcmc], start_index[num_mcmc], fell_back[num_mcmc] may be NULL.
 * trace_out (may be NULL): [num_mcmc][max_num_restarts][max_num_steps][size + 6], one row per step of the line search:
 *   x after the step (size) | f0 | halvings taken (30: every trial failed) | 1 if the limiter changed the step | 1 if rejected by
 *   value <= f0 | 1 if stopped by the step norm | state: 0 the step was not reached, 1 accepted, 2 ended without a move (30 failed
 *   trials or a zero step), 3 rejected.
 * An evaluation's sums have a fixed order that depends on the number of sampled points alone: a member's outputs carry the same bits
 * whatever num_mcmc, the other members and -- for the screened means -- num_candidates and the other candidates.
 * The members must share dim, the sampled points and the observed-derivative list, and live on one device.  Tensor-product domains
 * only: domain_type = MOE_DOMAIN_SIMPLEX is refused.  num_steps_averaged and num_multistarts are ignored, as in
 * moe_posterior_mean_optimize.  dim <= 32, num_mcmc <= 65 535.
 * Errors, in this order, everything that needs no handle before a handle is touched: gps NULL -> MOE_ERR_RUNTIME; num_mcmc < 1 ->
 * MOE_ERR_BOUNDS; gd, domain_bounds, candidates or best_points NULL -> MOE_ERR_RUNTIME; num_candidates < 1, num_fidelity < 0,
 * max_num_steps < 1, max_num_restarts < 1, domain_type other than MOE_DOMAIN_TENSOR_PRODUCT -> MOE_ERR_BOUNDS; a NULL handle ->
 * MOE_ERR_RUNTIME; num_fidelity >= dim -> MOE_ERR_BOUNDS; mismatched members -> MOE_ERR_INVALID_VALUE. */
int moe_posterior_mean_members_minimize(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* gd,
                                        const double* domain_bounds, const double* candidates, int num_candidates, int per_member,
                                        double* best_points, double* best_values, int* start_index, int* fell_back,
                                        double* means_out, double* trace_out, moe_error_t* err);
/* Posterior function paths by pathwise conditioning (Wilson et al. 2020) on the factor each member holds, and their minimisers: the
 * purpose of the reference's moe/optimal_learning/python/random_features.py (sample_gp_with_random_features,
 * global_optimization_of_GP_approximation, sample_from_global_optima), NOT its weight-space posterior: no M x M or n x n system of
 * the features is formed, and E[f_s(x)] = mu(x) exactly for every number of features.
 * Member e (no derivative observations; signal variance alpha, lengths l, noise s^2 = noise_variance[0], constant mean m, sampled
 * points X [n][dim], K = K(X, X) + s^2 I) and its path s:
 *   om_i = frequencies_i / l (coordinate by coordinate),   g_s(x) = sqrt(2 alpha / M) sum_i w_si cos(om_i . x + phases_i)
 *   v_s = K^-1 (y - m - g_s(X) - s z_s),                   f_s(x) = m + g_s(x) + sum_j v_sj k(x, X_j)
 * with M = num_features, S = num_paths, w = weights [num_mcmc][S][M] and z = noise_normals [num_mcmc][S][n] standard normals.
 * frequencies [M][dim] and phases [M] (uniform on [0, 2 pi)) are shared by every member and path of the call; the caller draws the
 * frequencies for the members' covariance: standard normals for the squared exponential, standard normals divided by sqrt(u / 5),
 * u ~ chi^2_5 (one u per feature), for Matern-5/2.  f_s(X_j) = y_j - s z_sj - s^2 v_sj identically.
 * moe_gp_paths_evaluate: values [num_mcmc][S][num_points] and, with want_grad != 0, grad [num_mcmc][S][num_points][dim] at points
 * [num_points][dim].
 * moe_gp_paths_minimize: moe_posterior_mean_members_minimize with the path f_s in the place of the member's mean, for every one of
 * the num_mcmc S paths: every path screened at the shared candidates [num_candidates][dim] (screened_out [num_mcmc][S][C]),
 * start_index by numpy.argmin's rule, that call's line search on -f_s decision for decision, its keep-or-fall-back rule.
 * best_points [num_mcmc][S][dim]; best_values, start_index, fell_back [num_mcmc][S], screened_out and trace_out
 * ([num_mcmc S][max_num_restarts][max_num_steps][dim + 6], that call's columns) may be NULL.
 * An evaluation's sums have a fixed order that depends on (M, n) alone: a (path, point) value carries the same bits whatever
 * num_points, S, num_mcmc and want_grad share the call, and the descent starts from the screened bits.
 * One copy down, one stream, one wait, one copy back; no handle is modified; scratch is pooled in the first member.
 * Errors, in this order, everything that needs no handle before a handle or the device is touched: gps NULL -> MOE_ERR_RUNTIME;
 * num_features outside 1 .. 4096, num_paths outside 1 .. 1024, num_mcmc outside 1 .. 1024, num_mcmc num_paths > 65 535 ->
 * MOE_ERR_BOUNDS (payload: the value, the limits); a NULL table, points or output -> MOE_ERR_RUNTIME; num_points / num_candidates <
 * 1, and for the minimiser max_num_steps < 1, max_num_restarts < 1, domain_type other than MOE_DOMAIN_TENSOR_PRODUCT ->
 * MOE_ERR_BOUNDS; a NULL handle -> MOE_ERR_RUNTIME; members of different dim, device, sampled points or cov_type, then a member with
 * derivative observations -> MOE_ERR_INVALID_VALUE (payload as in moe_ei_analytic_mcmc: the two values, the member).  There are no
 * fidelity coordinates: every coordinate is free. */
int moe_gp_paths_evaluate(const moe_gp_t* const* gps, int num_mcmc, const double* frequencies, const double* phases, int num_features,
                          const double* weights, const double* noise_normals, int num_paths, const double* points, int num_points,
                          int want_grad, double* values, double* grad, moe_error_t* err);
int moe_gp_paths_minimize(const moe_gp_t* const* gps, int num_mcmc, const double* frequencies, const double* phases, int num_features,
                          const double* weights, const double* noise_normals, int num_paths, const moe_gd_params_t* gd,
                          const double* domain_bounds, const double* candidates, int num_candidates, double* best_points,
                          double* best_values, int* start_index, int* fell_back, double* screened_out, double* trace_out,
                          moe_error_t* err);
/* compute_expected_improvement_mcmc / compute_grad_expected_improvement_mcmc / evaluate_EI_mcmc_at_point_list
 * (gpp_python_expected_improvement_mcmc.cpp:42-108 -> ExpectedImprovementMCMCEvaluator,
 * gpp_expected_improvement_mcmc_optimization.cpp:48-88); analytic != 0 takes the 1,0-EI evaluator (:136-176; needs
 * num_to_sample == 1, num_being_sampled == 0; normals may be NULL).  ei and/or grad_ei may be NULL. */
int moe_ei_mcmc_batch(const moe_gp_t* const* gps, int num_mcmc, const double* points_to_sample_all, int num_evals,
                      const double* points_being_sampled, int num_to_sample, int num_being_sampled, int num_mc,
                      const double* best_so_far, const double* normals, int analytic, double* ei, double* grad_ei,
                      moe_error_t* err);
/* multistart_knowledge_gradient_mcmc_optimization / multistart_expected_improvement_mcmc_optimization from caller-supplied
 * starts (gpp_knowledge_gradient_mcmc_optimization.hpp:665-862, gpp_expected_improvement_mcmc_optimization.hpp:840-990):
 * same driver as moe_kg_multistart / moe_ei_multistart on the MCMC-averaged objective.  The EI driver reports found = 0
 * unless some end point has EI > 0 (the reference seeds it with 0.0, not -1.0).
 * moe_kg_mcmc_multistart follows the reference's EXECUTION, not its intent (end points pinned to the reference's,
 * tests/golden/ref_kg_multistart.npz): KnowledgeGradientMCMCState::SetCurrentPoint copies only the first of the q points into
 * the array GetCurrentPoint and the fidelity cost read (gpp_knowledge_gradient_mcmc_optimization.cpp:186-195, .hpp:439-441), so
 * the optimiser steps from and returns [moved first point ; points 2..q of start_points[0]] while the objective is evaluated at
 * the points really reached; ComputeGradKnowledgeGradient accumulates into its output (.cpp:163-166), which the optimiser
 * allocates once per restart: step i sees ((G_{i-1} + sum of the per-GP gradients) / num_mcmc * cost - KG * gradcost) / cost^2;
 * the per-GP states keep start_points[0]'s discretised set (see moe_kg_multistart).  With q = 1 and no fidelity dimension
 * only the last two are visible. */
int moe_kg_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, int num_fidelity, const moe_gd_params_t* outer_params,
                           const moe_gd_params_t* inner_params, const double* domain_bounds, const double* discrete_pts_all,
                           int num_pts, const double* start_points, int num_starts, const double* points_being_sampled,
                           int num_to_sample, int num_being_sampled, int num_mc, const double* best_so_far,
                           const double* normals, int do_gradient_ascent, double* best_points, double* best_kg, int* found,
                           moe_error_t* err);
/* ---- r5: a whole suggestion on several GPUs (SURVEY 8e + 8f rank 1 / 2).  The reference parallelises its outer optimisers over
 * the restarts -- omp-parallel GradientDescentOptimizer runs merged under `omp critical`
 * (gpp_optimization.hpp:1472-1546, gpp_knowledge_gradient_optimization.hpp:860-935) -- and its MCMC-averaged objective is a sum
 * over independent GPs (gpp_knowledge_gradient_mcmc_optimization.hpp:666-1023).  Here every batched evaluation of the optimiser is
 * dealt to the ranks and followed by ONE all-gather; every rank then takes the same decisions on the same bits and returns the
 * same point:
 *   - moe_kg_multistart_comm: the restarts are dealt (evaluation i of a batch on rank i % world): the result is moe_kg_multistart's
 *     BIT FOR BIT, for any world size (an evaluation's bits do not depend on the batch it shares a call with);
 *   - moe_kg_mcmc_multistart_comm: the ensemble members are dealt -- member g is built and evaluated on rank g % world, which passes
 *     its members (ascending g) with their rows of discrete_pts / best_so_far; the per-member values are exchanged and every rank
 *     adds them up in global member order: moe_kg_mcmc_multistart's result bit for bit.
 * The exchange is the caller's: one process per GPU hands in its collective (cornell_moe_amd/dist.py: torch.distributed all_gather,
 * backend nccl = RCCL over xGMI, or gloo); a rank whose evaluation fails still takes part in the exchange and then EVERY rank
 * returns that error -- no rank is left waiting in a collective.  Payloads are small (a GD step of 20 restarts at q d = 32:
 * 5 KB per rank). */
typedef int (*moe_allgather_fn)(void* ctx, const double* send, double* recv, int count); /* recv[world][count], rank order; 0 = ok */
typedef struct moe_comm {
  int rank;  /* this process */
  int world; /* number of processes; 1 = no exchange (allgather may be NULL) */
  moe_allgather_fn allgather;
  void* ctx; /* passed back to allgather */
} moe_comm_t;
/* Timeline of the LAST outer optimisation this process ran (moe_kg_multistart*, moe_kg_mcmc_multistart*; rank 0 / worker 0): one row
 * per batched evaluation the optimiser issued, out[3 i ..] = kind (0 values, 1 gradients), items in the batch, wall milliseconds
 * (device work + exchange).  Returns the number of rows (out may be NULL / cap 0 to ask). */
int moe_multistart_trace(double* out, int cap);

/* Device-memory pool (r5).  The library keeps the device buffers, pinned staging buffers and streams its objects release (a GP of
 * N = 8000 holds 1 GB; a fresh hipMalloc / hipStreamCreate per hyper-parameter sample costs a 14 ms build 3 ms) and hands them to the
 * next object they fit.  Environment: MOE_POOL=0 switches it off; MOE_POOL_MAX_GB (default 48) bounds the device bytes held.
 * moe_pool_held_bytes: device bytes the pool holds right now (not those in use by live objects).  moe_pool_trim: returns all of them
 * (and the pinned buffers) to the runtime -- call it before handing the device to another library that needs the memory.  No
 * counterpart in the reference (its GaussianProcess lives in host memory). */
long long moe_pool_held_bytes(void);
int moe_pool_trim(void);
/* (diagnostic) the deal-and-exchange step alone, on synthetic items -- out[n][width], item i = seed + i + j / 1000; fail_item >= 0
 * makes its owner fail with MOE_ERR_SINGULAR, which every rank must then report.  No device work: the CPU tests run it over gloo. */
int moe_debug_sharded_items(const moe_comm_t* comm, int n, int width, double seed, int fail_item, double* out, moe_error_t* err);
int moe_kg_multistart_comm(const moe_gp_t* gp, const moe_comm_t* comm, int num_fidelity, const moe_gd_params_t* outer_params,
                           const moe_gd_params_t* inner_params, const double* domain_bounds, const double* discrete_pts,
                           int num_pts, const double* start_points, int num_starts, const double* points_being_sampled,
                           int num_to_sample, int num_being_sampled, int num_mc, double best_so_far, const double* normals,
                           int do_gradient_ascent, double* best_points, double* best_kg, int* found, moe_error_t* err);
int moe_kg_mcmc_multistart_comm(const moe_gp_t* const* local_gps, int num_local, int total_num_mcmc, const moe_comm_t* comm,
                                int num_fidelity, const moe_gd_params_t* outer_params, const moe_gd_params_t* inner_params,
                                const double* domain_bounds, const double* discrete_pts_local, int num_pts,
                                const double* start_points, int num_starts, const double* points_being_sampled,
                                int num_to_sample, int num_being_sampled, int num_mc, const double* best_so_far_local,
                                const double* normals, int do_gradient_ascent, double* best_points, double* best_kg, int* found,
                                moe_error_t* err);
/* Native exchange (r6): moe_comm_t carried by RCCL itself -- ncclAllGather on a stream and staging buffers the library owns, one pinned
 * copy in, one out, one stream wait per exchange; the optimiser loop never re-enters the host language.  This is the merge the reference
 * does under `omp critical` (cpp/gpp_optimization.hpp:1537-1545) once its restarts are dealt to processes, one per GPU.  librccl is
 * resolved at run time (dlopen; MOE_RCCL_LIB overrides the search): without it these entry points return MOE_ERR_RUNTIME.
 *   moe_rccl_unique_id: on rank 0; the 128 bytes travel to the other ranks by whatever the host has (dist.py: the gloo control group).
 *   moe_rccl_create: collective over the `world` ranks (ncclCommInitRank), one rank per device.
 *   moe_rccl_comm: fills a moe_comm_t (valid while the handle lives) for moe_kg_multistart_comm / moe_kg_mcmc_multistart_comm.
 *   moe_rccl_allreduce_sum: the MC-sharded evaluation's one collective (1 + q d doubles), host buffer in and out.
 *   moe_rccl_stats: exchanges so far, bytes received, seconds spent in them. */
#define MOE_RCCL_ID_BYTES 128
typedef struct moe_rccl moe_rccl_t;
int moe_rccl_unique_id(char* id, moe_error_t* err);
int moe_rccl_create(const char* id, int rank, int world, int device, moe_rccl_t** out, moe_error_t* err);
int moe_rccl_comm(moe_rccl_t* r, moe_comm_t* out);
int moe_rccl_allreduce_sum(moe_rccl_t* r, double* inout, int count, moe_error_t* err);
int moe_rccl_stats(const moe_rccl_t* r, long long* calls, long long* bytes, double* seconds);
void moe_rccl_destroy(moe_rccl_t* r);
/* The same for ONE process that drives several devices (a C / C++ host without torch; the twins of moe_kg_batch_multi): one host
 * thread per worker, the exchange in shared memory.  moe_kg_multistart_multi: gps[num_devices] hold the SAME GP on different
 * devices.  moe_kg_mcmc_multistart_multi: gps[num_mcmc] is the whole ensemble (the caller builds member g on device
 * g % num_workers); worker k takes members k, k + num_workers, ...  Results as above: bit for bit the single-device ones. */
int moe_kg_multistart_multi(const moe_gp_t* const* gps, int num_devices, int num_fidelity, const moe_gd_params_t* outer_params,
                            const moe_gd_params_t* inner_params, const double* domain_bounds, const double* discrete_pts,
                            int num_pts, const double* start_points, int num_starts, const double* points_being_sampled,
                            int num_to_sample, int num_being_sampled, int num_mc, double best_so_far, const double* normals,
                            int do_gradient_ascent, double* best_points, double* best_kg, int* found, moe_error_t* err);
int moe_kg_mcmc_multistart_multi(const moe_gp_t* const* gps, int num_mcmc, int num_workers, int num_fidelity,
                                 const moe_gd_params_t* outer_params, const moe_gd_params_t* inner_params,
                                 const double* domain_bounds, const double* discrete_pts_all, int num_pts,
                                 const double* start_points, int num_starts, const double* points_being_sampled,
                                 int num_to_sample, int num_being_sampled, int num_mc, const double* best_so_far,
                                 const double* normals, int do_gradient_ascent, double* best_points, double* best_kg, int* found,
                                 moe_error_t* err);
int moe_ei_mcmc_multistart(const moe_gp_t* const* gps, int num_mcmc, const moe_gd_params_t* outer_params,
                           const double* domain_bounds, const double* start_points, int num_starts,
                           const double* points_being_sampled, int num_to_sample, int num_being_sampled, int num_mc,
                           const double* best_so_far, const double* normals, int do_gradient_ascent, double* best_points,
                           double* best_ei, int* found, moe_error_t* err);

/* ---- log marginal likelihood of the data under the GP prior: compute_log_likelihood /
 * evaluate_log_likelihood_at_hyperparameter_list (gpp_python_model_selection.cpp:43-69, 270-340 ->
 * LogMarginalLikelihoodEvaluator, gpp_model_selection.cpp:540-612).  A handle keeps the data and the device buffers so
 * that a hyper-parameter sampler's thousands of evaluations on the same data re-use them.
 * hyperparameters_all[num_sets][1 + dim + 1 + num_derivatives] = (alpha, lengths[dim], noise_variance[1 + g]) per set, the
 * layout of the reference's hyperparameter lists (gpp_python_model_selection.cpp:301-303).  Like the reference, 1e-6 is
 * added to the diagonal of K + noise before it is factored (gpp_model_selection.cpp:546-549).  Where the reference
 * ignores a failed factorisation (:551-553, "TODO(GH-211)") and returns a meaningless number, values[i] is -infinity.
 * The sets of one call are factorised together (up to 64 per device pass): a sampler that proposes for all its walkers at
 * once should pass them in one call. */
typedef struct moe_ll moe_ll_t;
int moe_ll_create(int cov_type, const double* points_sampled, const double* points_sampled_value, const int* derivatives,
                  int num_derivatives, int dim, int num_sampled, int device, moe_ll_t** ll_out, moe_error_t* err);
int moe_ll_destroy(moe_ll_t* ll);
int moe_ll_evaluate(moe_ll_t* ll, const double* hyperparameters_all, int num_sets, double* values, moe_error_t* err);
/* compute_hyperparameter_grad_log_likelihood (gpp_python_model_selection.cpp:88-135 ->
 * LogMarginalLikelihoodEvaluator::ComputeGradLogLikelihood, gpp_model_selection.cpp:629-677):
 * grad[1 + dim + 1 + g] = d log p(y | X, theta) / d (alpha, lengths[dim], noise_variance[1 + g]) at ONE hyper-parameter set
 * (layout as above) = 1/2 a^T (dK/dtheta) a - 1/2 tr(K^-1 dK/dtheta), a = K^-1 (y - mean).  The Matern-5/2 kernel follows
 * the reference's convention that only the function-value block of K depends on (alpha, lengths)
 * (MaternNu2p5::HyperparameterGradCovariance, gpp_covariance.cpp:461-487, fills that block alone); the squared
 * exponential is provided without derivative observations.  A singular K + noise is MOE_ERR_SINGULAR. */
int moe_ll_grad(moe_ll_t* ll, const double* hyperparameters, double* grad, moe_error_t* err);
/* r5 -- multistart_hyperparameter_optimization / restarted_hyperparameter_optimization (gpp_python_model_selection.cpp:428-474 ->
 * MultistartGradientDescentHyperparameterOptimization / RestartedGradientDescentHyperparameterOptimizationTensor,
 * gpp_model_selection.hpp:967-1103) from caller-supplied initial guesses: the maximum-likelihood hyper-parameters by restarted gradient
 * ascent (GradientDescentOptimizer, gpp_optimization.hpp:619-705, 1144-1185) on log p(y | X, theta) over
 * theta = (alpha, lengths[dim], noise_variance[1 + g]) in LINEAR space, inside the tensor-product domain domain_log10[n_hyper][2] given
 * in LOG-10 space (as the reference's boundary takes it).  initial_guesses[num_starts][n_hyper] are linear-space points (the reference
 * draws a Latin hypercube in log space and exponentiates, :841-858; moe_latin_hypercube reproduces the generator).  As in the reference
 * the best initial guess seeds the result (InitializeBestKnownPoint, :911-930) and *found reports whether an optimised end point beat
 * it.  num_starts = 1 is the restarted (single-start) optimiser.  Every ascent step evaluates the gradients of all running starts. */
int moe_ll_multistart(moe_ll_t* ll, const moe_gd_params_t* gd_params, const double* domain_log10, const double* initial_guesses,
                      int num_starts, double* best_hyperparameters, double* best_value, int* found, moe_error_t* err);
/* restarted_hyperparameter_optimization (RestartedGradientDescentHyperparameterOptimizationTensor, gpp_model_selection.hpp:989-1012):
 * the point the restarted ascent from x0[n_hyper] (linear space) ENDS at -- the reference returns the state's current point, whether
 * or not it improved on the start. */
int moe_ll_ascend(moe_ll_t* ll, const moe_gd_params_t* gd_params, const double* domain_log10, const double* x0, double* end_point,
                  moe_error_t* err);
/* ---- the leave-one-out objective: LogLikelihoodTypes.leave_one_out_log_likelihood (GaussianProcessLeaveOneOutLogLikelihood,
 * python/cpp_wrappers/log_likelihood.py:447; Rasmussen & Williams 5.4.2).  With K = K(X, X) + diag(noise + 1e-6), yc the values
 * centred as for the marginal likelihood (the mean is NOT re-estimated per fold), alpha = K^-1 yc and kappa_i = (K^-1)_ii, each of the
 * N = num_sampled (1 + g) scalar observations -- a function value or one observed partial derivative -- is left out by itself:
 *   mu_i = yc_i - alpha_i / kappa_i,   var_i = 1 / kappa_i,
 *   L_LOO(theta) = sum_i [ 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi ].
 * A handle has an objective, MOE_LL_LOG_MARGINAL (0, what it starts with) or MOE_LL_LEAVE_ONE_OUT (1) -- the values of the
 * reference's LogLikelihoodTypes -- which selects what moe_ll_evaluate, moe_ll_grad, moe_ll_ascend, moe_ll_multistart and moe_ll_mcmc
 * compute; everything else about those calls (layouts, the 1e-6, -infinity on a failed pivot, MOE_ERR_SINGULAR from the gradient) is
 * as documented with them.  moe_ll_set_objective: MOE_ERR_BOUNDS for any other value.
 * Gradient under MOE_LL_LEAVE_ONE_OUT: with c_i = alpha_i / kappa_i, e_i = 1/2 (1 + alpha_i^2 / kappa_i) / kappa_i, u = K^-1 c and
 * M = K^-1 diag(e) K^-1,  d L_LOO / d theta = sum_ab (u_a alpha_b - M_ab) (dK / d theta)_ab, with moe_ll_grad's convention for
 * dK / d (alpha, lengths) (only the function-value block depends on them) and its restriction (derivative observations: Matern-5/2
 * only, MOE_ERR_INVALID_VALUE otherwise).  The value and the predictions are provided for both kernels at every g. */
#define MOE_LL_LOG_MARGINAL 0
#define MOE_LL_LEAVE_ONE_OUT 1
int moe_ll_set_objective(moe_ll_t* ll, int objective, moe_error_t* err);
int moe_ll_get_objective(const moe_ll_t* ll);
/* mean_out / var_out [num_sampled][1 + g]: the LOO predictive mean and variance of every observation at ONE hyper-parameter set,
 * whatever the handle's objective (which the call does not change).  The means of function values are in the caller's units (the
 * centring mean added back); those of derivative observations need none.  A singular K + noise is MOE_ERR_SINGULAR. */
int moe_ll_loo_predict(moe_ll_t* ll, const double* hyperparameters, double* mean_out, double* var_out, moe_error_t* err);

/* ---- hyper-parameter sampling: GaussianProcessLogLikelihoodMCMC.train() (python/cpp_wrappers/log_likelihood_mcmc.py:170-239),
 * which hands its log posterior to emcee.EnsembleSampler.  moe_ll_mcmc is that sampler -- the affine-invariant ensemble sampler with
 * the stretch move (Goodman & Weare 2010) -- with the whole chain resident on the device: one upload, one stream of kernels for all
 * num_steps steps, one wait, one download.
 *
 * State: num_walkers = W walkers of nh = 1 + dim + 1 + g log-space coordinates theta = log(alpha, lengths[dim], noise[1 + g]).
 * W must be even and >= 2 nh (MOE_ERR_BOUNDS; the wrapper's default is max(n_hypers, 2 nh), log_likelihood_mcmc.py:122).
 *
 * Log posterior of a walker: -inf if any |theta_k| > 20 (log_likelihood_mcmc.py:286) or the log prior is -inf; otherwise
 * log prior(theta) + the log marginal likelihood at exp(theta) exactly as moe_ll_evaluate defines it (1e-6 on the diagonal, values
 * centred, -inf on a failed pivot).
 *
 * The prior is a table of nh entries (kind, a, b), one per coordinate, in log space; the per-coordinate terms are added
 * (default_priors.py:27-36), -inf wins over +inf.  With moe_set_reference_quirks(1), the default, NORMAL and HORSESHOE are what the
 * reference computes; with quirks off they are what it intends:
 *   MOE_PRIOR_NONE                  0
 *   MOE_PRIOR_TOPHAT    (min, max)  0 inside [min, max], -inf outside                                    (base_prior.py:120-123)
 *   MOE_PRIOR_NORMAL    (mean, sd)  quirks: the normal DENSITY, not its log (base_prior.py:354, sic); off: the log density
 *   MOE_PRIOR_HORSESHOE (scale)     quirks: ln ln(1 + 3 (scale / theta)^2) of the LOG-SPACE coordinate, +inf at theta = 0
 *                                   (base_prior.py:199-201, sic); off: the same formula of exp(theta)
 *   MOE_PRIOR_LOGNORMAL (sd, mean)  scipy.stats.lognorm.logpdf(theta, sd, loc=mean)                      (base_prior.py:281)
 *   MOE_PRIOR_FIXED     (value)     the coordinate is set to `value` in every proposal before it is evaluated, and stored so; it adds
 *                                   nothing.  This is the wrapper's noisy=False (noise pinned at log 1e-8, log_likelihood_mcmc.py:288-289)
 * DefaultPrior (default_priors.py:19-35) is NORMAL(0, 1) on alpha, TOPHAT(-2, 3) on the lengths, HORSESHOE(0.1) on the noises.
 *
 * One step is two half-steps: walkers [0, W/2) move against [W/2, W), then the second half against the updated first.  For walker s
 * of the moving half, at index i of half-step (t, h) of the tables below:
 *   c = walker partner[t][h][i] of the other half;   z = ((a - 1) u_stretch[t][h][i] + 1)^2 / a   (a = stretch_a > 1; emcee's is 2);
 *   proposal = c - z (c - s);   ln r = (nh_free - 1) ln z + lnp(proposal) - lnp(s),   nh_free = the coordinates that are not FIXED;
 *   accepted iff ln r > ln u_accept[t][h][i], and always when lnp(proposal) = +inf.
 * Randomness crosses the ABI as tables, as everywhere in this library: u_stretch, u_accept [num_steps][2][W/2] uniforms in [0, 1),
 * partner [num_steps][2][W/2] integers in [0, W/2) (MOE_ERR_BOUNDS otherwise).
 *
 * p0[W][nh]: the initial walkers.  Each must have a finite log posterior: otherwise MOE_ERR_INVALID_VALUE (payload: the first such
 * walker's index, its log posterior) and the outputs are undefined.
 * chain[num_steps][W][nh] and lnprob[num_steps][W]: positions and log posteriors AFTER step t.  lnprob0[W]: of p0.
 * proposal_lnprob[num_steps][W] (or NULL): the log posterior of the proposal made for walker w in step t, accepted or not;
 * accepted[num_steps][W] (or NULL): 1 / 0.  num_steps = 0 evaluates lnprob0 only. */
#define MOE_PRIOR_NONE 0
#define MOE_PRIOR_TOPHAT 1
#define MOE_PRIOR_NORMAL 2
#define MOE_PRIOR_HORSESHOE 3
#define MOE_PRIOR_LOGNORMAL 4
#define MOE_PRIOR_FIXED 5
typedef struct moe_prior {
  int kind; /* MOE_PRIOR_* */
  double a, b;
} moe_prior_t;
int moe_ll_mcmc(moe_ll_t* ll, const moe_prior_t* priors, int num_walkers, int num_steps, double stretch_a, const double* p0,
                const double* u_stretch, const int* partner, const double* u_accept, double* chain, double* lnprob, double* lnprob0,
                double* proposal_lnprob, int* accepted, moe_error_t* err);

/* ---- covariance assembly (exposed for parity tests and the HBM-roofline measurement) ----
 * BuildMixCovarianceMatrix (gpp_math.cpp:309-335, 469-479): out[N x num_pts*(1+g2)] col-major = K(X, pts) with
 * derivative blocks; derivs2[g2] are the derivative observations carried by `pts`. */
int moe_gp_mix_covariance(const moe_gp_t* gp, const double* pts, int num_pts, const int* derivs2, int g2, double* out,
                          moe_error_t* err);
/* Timing probe: builds K(X, pts) [N x num_pts] on device `repeat` times without copying it back; returns the average
 * kernel milliseconds (HIP events) and the algorithmic bytes per launch. */
int moe_cov_build_probe(const moe_gp_t* gp, const double* pts, int num_pts, int repeat, double* avg_ms,
                        double* bytes_per_launch, moe_error_t* err);

/* Timing probe of the GP's own covariance assembly: K(X, X) + noise on the diagonal, N x N with the derivative-observation
 * blocks (BuildCovarianceMatrixWithNoiseVariance, gpp_math.cpp:391-455) -- the launch GaussianProcess construction makes --
 * `repeat` times into a scratch matrix; average kernel ms (HIP events) and the algorithmic bytes 8 [2 n d + N^2]. */
int moe_kxx_build_probe(const moe_gp_t* gp, int repeat, double* avg_ms, double* bytes_per_launch, moe_error_t* err);
/* What the chip sustains on nothing but dependent FP64 FMA chains (8 per lane, 16 wavefronts per CU), TFLOP/s: the rate the
 * FP64-bound kernels can be held against next to the 78.6 TFLOP/s of the data sheet (the clock does not hold 2.4 GHz under
 * FP64 load). */
int moe_debug_fp64_rate(int device, double* tflops, moe_error_t* err);

/* Parity probe of the device factorisation used by moe_gp_create: factors the SPD matrix a[n*n] (column-major, lower
 * triangle read) with the blocked device Cholesky that replaces ComputeCholeskyFactorL (gpp_linear_algebra.cpp:109-148);
 * writes the factor to chol[n*n] (strict upper = 0) and its explicit inverse to chol_inv[n*n]; *info = 0 or the failing
 * leading-minor index (pivot <= 1e-16), in which case MOE_ERR_SINGULAR is returned. */
int moe_debug_cholesky(int n, const double* a, int device, double* chol, double* chol_inv, int* info, moe_error_t* err);

/* Accuracy probe of the device exp / sqrt used inside the covariance loops (csrc/fastmath.hpp):
 * exp_neg[i] = exp(-x[i]), sqrt_out[i] = sqrt(x[i]) for x[i] >= 0. */
int moe_debug_math(int n, const double* x, int device, double* exp_neg, double* sqrt_out, moe_error_t* err);

/* Timing of the last moe_kg / moe_kg_batch call's dominant kernels, measured with HIP events on the library's stream:
 * out[0] = MC inner-optimisation kernel ms, out[1] = N x M covariance-build ms, out[2] = tail contraction ms,
 * out[3] = state set-up ms, out[4] = total device ms. */
int moe_last_kernel_ms(const moe_gp_t* gp, double* out5);
/* Which Monte-Carlo kernel the last moe_kg* call on this handle launched (diagnostics; the tests use it to assert that a
 * fixture really exercised the path it was built for): out[0] = variant (0 wave-per-sample, 1 workgroup-per-sample, 2 streamed-weights wave-per-sample),
 * out[1] = bit 0: coordinate table in LDS; bit 1: FAR FRAME -- the training set, the points being sampled or the inner domain box
 *          span more than 100 length scales from the training-set mean, so the evaluation took the direct-difference kernels with
 *          single-trial passes (exact, slower: typical triggers are the short length scales of a hyper-parameter MCMC ensemble or a
 *          search box far wider than the data); bit 2: coordinates streamed from L2 (far frame, or d > 16); bit 3 (r5): the lane-parked
 *          form of the LDS-table kernel (kg_mc_lane.hpp; MOE_KG_LANE=0 selects the round-4 form -- same results bit for bit);
 *          bit 4: the line searches took their first gradient from the evaluation's start table (no derivative observations,
 *          LDS-table kernels) instead of a pass over the points,
 * out[2] = wavefronts per workgroup, out[3] = register tiles per wavefront (variant 1) or
 * leading tiles of the paired-row table kept in LDS (variant 0, d > 16),
 * out[4] = streamed per-sample weight table, out[5] = T-free gradient tail, out[6] = workgroups, out[7] = sample pre-pass. */
int moe_last_kernel_info(const moe_gp_t* gp, int* out8);
/* How many times a workgroup of the last moe_kg* call's Monte-Carlo kernel moved from an evaluation whose samples were all drawn to
 * one that still had some (diagnostics; 0 with MOE_KG_STEAL=0, with one evaluation per call, and before the first call).  Reads one
 * word back from the device: call it after the evaluation has returned. */
int moe_last_kg_moves(const moe_gp_t* gp, long long* moves);
/* The end points of the inner optimisations of the last moe_kg* call on this handle, all evaluations of the call (moe_kg returns them
 * for its one evaluation only): *num_evals and *num_local are set to the call's shape; `out`, if not NULL, receives
 * [num_evals][num_local][dim] doubles (capacity: doubles available in out).  Diagnostics: reads the points back from the device. */
int moe_last_kg_best_points(const moe_gp_t* gp, int* num_evals, int* num_local, double* out, long long capacity);

#ifdef __cplusplus
}
#endif
#endif /* MOE_HIP_H_ */
