// cornell_moe_amd/csrc/hyper_mcmc.hip -- the device side of moe_ll_mcmc: the affine-invariant ensemble sampler with the stretch
// move (Goodman & Weare 2010; what emcee.EnsembleSampler runs for GaussianProcessLogLikelihoodMCMC.train(),
// python/cpp_wrappers/log_likelihood_mcmc.py:170-239) over log-space hyper-parameters, for gfx950.
//
// A half-step of the chain is a fixed sequence of launches on one stream, with no host involvement (api.hip: ll_mcmc_locked):
//   hmc_propose_kernel     W/2 proposals from the walkers and the random tables in device memory; box, prior, (nh_free - 1) ln z; the
//                          linear-space covariance parameters and noise + 1e-6 of every proposal
//   hmc_cov_batch_kernel   K(X, X; theta_b) + noise of the whole half-ensemble in ONE launch (grid.z = set), parameters read from the
//                          device array the propose kernel wrote -- launch_cov_build takes them by value from the host, one launch per set
//   launch_ll_border / launch_cholesky_batch / launch_ll_terms_batch (kernels_linalg.hip), as moe_ll_evaluate uses them
//   hmc_accept_kernel      (sum log L_ii, |L^-1 yc|^2, info) -> log posterior; the decision; walkers, chain and diagnostics updated
// The arithmetic that defines a proposal (z and c - z (c - s)) is compiled without contraction, so that it is the sequence of
// correctly rounded operations its description names; everything else follows the build's defaults.
#include <algorithm>
#include <cmath>

#include "device_cov.hpp"

namespace moe {

namespace {

constexpr double kHmcBox = 20.0;                     // log_likelihood_mcmc.py:286
constexpr double kSqrt2Pi = 2.50662827463100050242;  // sqrt(2 pi)
constexpr double kLog2Pi = 1.8378770664093454835607;

// z = ((a - 1) u + 1)^2 / a and c - z (c - s): each operation rounded on its own
__device__ __forceinline__ double stretch_z(double a, double u) {
#pragma clang fp contract(off)
  const double t = (a - 1.0) * u + 1.0;
  return (t * t) / a;
}
__device__ __forceinline__ double stretch_coord(double c, double s, double z) {
#pragma clang fp contract(off)
  const double diff = c - s;
  const double step = z * diff;
  return c - step;
}

// log prior of ONE log-space coordinate (include/moe_hip.h: moe_prior_t); -inf / +inf are results, not errors
__device__ __forceinline__ double hmc_log_prior(int kind, double a, double b, double theta, int quirks) {
  switch (kind) {
    case MOE_PRIOR_TOPHAT:
      return (theta < a || theta > b) ? -INFINITY : 0.0;
    case MOE_PRIOR_NORMAL: {  // (mean a, sigma b)
      const double t = (theta - a) / b;
      if (quirks) return exp(-0.5 * t * t) / (b * kSqrt2Pi);  // base_prior.py:354 returns the density (sic)
      return -0.5 * t * t - log(b) - 0.5 * kLog2Pi;
    }
    case MOE_PRIOR_HORSESHOE: {  // (scale a)
      if (quirks && theta == 0.0) return INFINITY;  // base_prior.py:199-200
      const double q = a / (quirks ? theta : exp(theta));  // base_prior.py:201 takes the log-space coordinate (sic)
      return log(log1p(3.0 * (q * q)));
    }
    case MOE_PRIOR_LOGNORMAL: {  // (sigma a, mean b): scipy.stats.lognorm.logpdf(theta, a, loc=b)
      const double y = theta - b;
      if (!(y > 0.0)) return -INFINITY;
      const double ly = log(y);
      return -(ly * ly) / (2.0 * a * a) - log(a * y * kSqrt2Pi);
    }
    default:  // MOE_PRIOR_NONE, MOE_PRIOR_FIXED
      return 0.0;
  }
}

// One thread per moving walker.  step < 0: the initial evaluation -- the "proposal" of walker s is the walker itself.
__global__ __launch_bounds__(64) void hmc_propose_kernel(HmcState st, int step, int half) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= st.H) return;
  const int nh = st.nh, d = st.d, g1 = st.g1;
  const int s = half * st.H + b;
  const double* ws = st.walkers + (long)s * nh;
  double* prop = st.prop + (long)b * nh;
  double zterm = 0.0;
  if (step >= 0) {
    const long idx = ((long)step * 2 + half) * st.H + b;
    const int c = (1 - half) * st.H + st.partner[idx];
    const double* wc = st.walkers + (long)c * nh;
    const double z = stretch_z(st.stretch_a, st.u_stretch[idx]);
    for (int k = 0; k < nh; ++k) prop[k] = stretch_coord(wc[k], ws[k], z);
    zterm = (double)(st.nh_free - 1) * log(z);
  } else {
    for (int k = 0; k < nh; ++k) prop[k] = ws[k];
  }
  bool dead = false, pinf = false;
  double lp = 0.0;
  for (int k = 0; k < nh; ++k) {
    const moe_prior_t pr = st.priors[k];
    if (pr.kind == MOE_PRIOR_FIXED) prop[k] = pr.a;
    const double th = prop[k];
    if (!(fabs(th) <= kHmcBox)) dead = true;  // (a NaN coordinate too)
    const double v = hmc_log_prior(pr.kind, pr.a, pr.b, th, st.quirks);
    if (v == -INFINITY || v != v) dead = true;
    else if (v == INFINITY) pinf = true;
    else lp += v;
  }
  st.prior[b] = dead ? -INFINITY : (pinf ? INFINITY : lp);
  st.zterm[b] = zterm;
  // what a covariance build needs (gp.hip fill_cov_params; gpp_model_selection.cpp:546-549 for the 1e-6).  A proposal the box or
  // the prior has already rejected is factored at theta = 0, a well-conditioned matrix whose result the accept ignores.
  CovParams* cp = st.cps + b;
  cp->type = st.cov_type;
  cp->dim = d;
  cp->dp = st.dp;
  cp->alpha = dead ? 1.0 : exp(prop[0]);
  for (int k = 0; k < kMaxDimPadded; ++k) {
    double il = 0.0, il2 = 0.0;
    if (k < d) {
      const double l = dead ? 1.0 : exp(prop[1 + k]);
      il2 = 1.0 / (l * l);
      il = 1.0 / l;
    }
    cp->inv_l2[k] = il2;
    cp->inv_l[k] = il;
    cp->center[k] = 0.0;
  }
  for (int a = 0; a < g1; ++a) st.noise[(long)b * g1 + a] = (dead ? 1.0 : exp(prop[1 + d + a])) + 1.0e-6;
}

// K(X, X; theta_set) + noise for every set of a pass: one thread per output row, so a wavefront's 64 stores of one column are 512
// contiguous bytes; the column tile's points are staged in LDS and read as broadcasts; the set's parameters are read from device memory
// at an address that is uniform over the workgroup.  An entry is radial_scalars + cov_entry of device_cov.hpp on the differences the other covariance builds form
// (kernels_cov.hip).  lower_only: entries above the diagonal are neither computed nor stored (the one-level batched factorisation
// reads the lower triangle only).
// Tile shape: a workgroup has as many wavefronts as the rows need, at most four (N of tens: one or two wavefronts, none idle), and
// covers kHmcCols = 4 column points.  At these sizes the launch does not fill the chip -- n / 4 workgroups per set -- so a narrow
// column tile is what spreads a set over the CUs; the price is that a row's point is re-read (from L2) once per tile, 8 DP bytes
// against the 32 (1 + g) bytes the thread stores for it.  Measured share of a chain: DESIGN 5.8.
constexpr int kHmcRows = 256;  // most rows per workgroup
constexpr int kHmcCols = 4;

template <int DP, bool DERIVS>
__global__ __launch_bounds__(kHmcRows) void hmc_cov_batch_kernel(const CovParams* __restrict__ cps, const double* __restrict__ noise,
                                                                const double* __restrict__ X, int n, DerivList dl,
                                                                double* __restrict__ out, long ld, long set_stride, int lower_only) {
  __shared__ double Bs[kHmcCols][DP];
  const int g1 = DERIVS ? 1 + dl.g : 1;
  const int rows = n * g1;
  const int j0 = blockIdx.x * kHmcCols;
  const int nj = min(kHmcCols, n - j0);
  const int brows = blockDim.x;  // rows of this launch's workgroups (a multiple of 64, <= kHmcRows)
  if (lower_only && (long)blockIdx.y * brows + brows - 1 < (long)j0 * g1) return;  // a tile above the diagonal
  const CovParams& cp = cps[blockIdx.z];  // (written by an earlier kernel, read-only here; the index is uniform over the workgroup)
  const double* nz = noise + (long)blockIdx.z * g1;
  double* o = out + (long)blockIdx.z * set_stride;
  for (int t = threadIdx.x; t < nj * DP; t += brows) Bs[t / DP][t % DP] = X[(long)(j0 + t / DP) * DP + (t % DP)];
  __syncthreads();
  const int r = blockIdx.y * brows + threadIdx.x;
  if (r >= rows) return;
  const int i = DERIVS ? r / g1 : r;
  const int a = DERIVS ? r % g1 : 0;
  double xi[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xi[k] = X[(long)i * DP + k];
  for (int jj = 0; jj < nj; ++jj) {
    double diff[DP];
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      diff[k] = xi[k] - Bs[jj][k];
      r2 = fma(diff[k] * diff[k], cp.inv_l2[k], r2);
    }
    const Radial rd = radial_scalars(cp.type, cp.alpha, r2);
    for (int b = 0; b < g1; ++b) {
      const long colrel = (long)(j0 + jj) * g1 + b;
      if (lower_only && (long)r < colrel) continue;
      double v = DERIVS ? cov_entry<DP>(cp, rd, diff, a, b, dl, dl) : rd.base;
      if ((long)r == colrel) v += nz[a];
      o[(long)r + colrel * ld] = v;
    }
  }
}

template <int DP>
void hmc_cov_batch_dp(const CovParams* cps, const double* noise, const double* X, int n, const DerivList& dl, double* out, long ld,
                      long set_stride, int sets, bool lower_only, hipStream_t s) {
  const int rows = n * (1 + dl.g);
  const int brows = std::min(kHmcRows, (rows + 63) / 64 * 64);
  const dim3 grid((n + kHmcCols - 1) / kHmcCols, (rows + brows - 1) / brows, sets);
  if (dl.g > 0)
    MOE_LAUNCH_NOW((hmc_cov_batch_kernel<DP, true>), grid, dim3(brows), 0, s, cps, noise, X, n, dl, out, ld, set_stride,
                   lower_only ? 1 : 0);
  else
    MOE_LAUNCH_NOW((hmc_cov_batch_kernel<DP, false>), grid, dim3(brows), 0, s, cps, noise, X, n, dl, out, ld, set_stride,
                   lower_only ? 1 : 0);
}

// One thread per moving walker: the log posterior of its proposal, the decision, the bookkeeping.
__global__ __launch_bounds__(64) void hmc_accept_kernel(HmcState st, const double* __restrict__ terms, const int* __restrict__ info,
                                                       int N, int step, int half) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= st.H) return;
  const int nh = st.nh;
  const int s = half * st.H + b;
  double lp = st.prior[b];
  if (lp != -INFINITY) {
    if (info[b] != 0)
      lp = -INFINITY;  // a failed pivot (moe_ll_evaluate)
    else
      lp += -0.5 * terms[2 * b + 1] - terms[2 * b] - 0.5 * (double)N * kLog2Pi;
  }
  double* ws = st.walkers + (long)s * nh;
  const double* prop = st.prop + (long)b * nh;
  if (step < 0) {
    for (int k = 0; k < nh; ++k) ws[k] = prop[k];  // (FIXED coordinates are stored at their value)
    st.lnp[s] = lp;
    st.lnprob0[s] = lp;
    return;
  }
  const long idx = ((long)step * 2 + half) * st.H + b;
  const double lnr = st.zterm[b] + lp - st.lnp[s];
  const bool acc = (lp == INFINITY) || (lnr > log(st.u_accept[idx]));  // (a NaN ratio rejects)
  if (acc) {
    for (int k = 0; k < nh; ++k) ws[k] = prop[k];
    st.lnp[s] = lp;
  }
  const long row = (long)step * st.W + s;
  for (int k = 0; k < nh; ++k) st.chain[row * nh + k] = ws[k];
  st.lnprob[row] = st.lnp[s];
  if (st.proposal_lnprob != nullptr) st.proposal_lnprob[row] = lp;
  if (st.accepted != nullptr) st.accepted[row] = acc ? 1 : 0;
}

}  // namespace

void launch_hmc_propose(const HmcState& st, int step, int half, hipStream_t s) {
  MOE_LAUNCH_NOW(hmc_propose_kernel, dim3((st.H + 63) / 64), dim3(64), 0, s, st, step, half);
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_hmc_cov_batch(int dp, const CovParams* cps, const double* noise, const double* X, int n, const DerivList& dl, double* out,
                          long ld, long set_stride, int sets, bool lower_only, hipStream_t s) {
  if (sets <= 0 || n <= 0) return;
  dispatch_dp(dp, [&](auto DP) { hmc_cov_batch_dp<DP>(cps, noise, X, n, dl, out, ld, set_stride, sets, lower_only, s); });
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_hmc_accept(const HmcState& st, const double* terms, const int* info, int N, int step, int half, hipStream_t s) {
  MOE_LAUNCH_NOW(hmc_accept_kernel, dim3((st.H + 63) / 64), dim3(64), 0, s, st, terms, info, N, step, half);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace moe
