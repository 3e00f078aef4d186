// cornell_moe_amd/csrc/pm_members.hip -- every ensemble member's own posterior-mean minimiser in one device call: the per-member
// discretisation of a KG-MCMC iteration (the reference's examples/main.py:172-197 over ComputeOptimalPosteriorMean from one start,
// gpp_knowledge_gradient_optimization.cpp:420-472, gpp_optimization.hpp:708-828 / 1242-1283 -- what posterior_mean_optimize
// (multistart.hip) restates on the host, one launch and one wait per evaluation).
//
// For E members over the same n training points and C candidates (one shared set or one set per member), one upload, one stream, one
// wait, one copy back:
//   screen    mu_e(c, fidelity = 1) of every (member, candidate) pair              pmm_screen_kernel (one workgroup per pair)
//   select    start_index[e] = the first index of the smallest mu_e                pmm_argmin_kernel (one workgroup per member)
//   descend   the back-tracking line-search ascent on -mu_e from that candidate,   pmm_descent_kernel (one workgroup per member,
//             then keep or fall back                                               resident for the whole optimisation)
//
// One evaluation of one member at one point (pmm_eval) belongs to ONE workgroup of 256 threads, whichever kernel asks: thread t takes
// the training points t, t + 256, ...; a wavefront's lanes are added by a butterfly and the four wavefronts as (0 + 1) + (2 + 3) by
// the thread that owns the component.  The order of every sum is a function of n alone, so a pair's or a member's bits depend
// neither on C, nor on E, nor on what else is in the call.  Every thread of the descent reads the sums from LDS and takes the same
// scalar decisions: control flow is workgroup-uniform, and nothing crosses workgroups.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_cov.hpp"
#include "gp.hpp"
#include "pm_descent.hpp"

namespace moe {

namespace {

constexpr int kPmmPass = 16384;    // candidates per launch of pmm_screen_kernel (moe_hip.h: moe_posterior_mean_members_minimize)

static_assert(sizeof(CovParams) % sizeof(unsigned int) == 0, "the descent copies a member's covariance into LDS by words");

struct PmmData {
  const PmMember* members;  // [E]
  const double* X;          // [n][DP]: the members share the data
  DerivList dX;
  int n, size;  // size = dim - num_fidelity: the free coordinates
};

// mu (and with GRAD d mu / d x_k) of the member (cp, w_m = K^-1 y, mean) at the point pt (LDS, [DP], fidelity coordinates 1, padding 0):
//   tot[0] = mu, tot[1 + k] = d mu / d x_k.  Valid for every thread on return.  red: LDS [4][1 + DP].
// Begins with a barrier (pt is visible, the previous tot has been read) and ends with one.
template <int DP, bool GRAD>
__device__ __forceinline__ void pmm_eval(const CovParams& cp, const double* __restrict__ w_m, double mean,
                                         const double* __restrict__ X, int n, const DerivList& dX, const double* pt, double* red,
                                         double* tot) {
  constexpr int W1 = 1 + DP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  DerivList none;
  none.g = 0;
  __syncthreads();
  const int g1 = 1 + dX.g;
  double xp[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xp[k] = pt[k];
  double acc = 0.0, accg[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) accg[k] = 0.0;
  for (int j = tid; j < n; j += kPmmThreads) {
    double diff[DP];
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      diff[k] = xp[k] - X[(long)j * DP + k];
      r2 = fma(diff[k] * diff[k], cp.inv_l2[k], r2);
    }
    const Radial rd = radial_scalars(cp.type, cp.alpha, r2);
    for (int b = 0; b < g1; ++b) {
      const double w = w_m[(long)j * g1 + b];
      acc = fma(cov_entry<DP>(cp, rd, diff, 0, b, none, dX), w, acc);
      if (GRAD) {
#pragma unroll
        for (int dd = 0; dd < DP; ++dd)
          if (dd < cp.dim) accg[dd] = fma(grad_cov_entry<DP>(cp, rd, diff, 0, b, dd, none, dX), w, accg[dd]);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) red[wave * W1] = acc;
  if (GRAD) {
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double u = accg[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) u += __shfl_xor(u, off, 64);
      if (lane == 0) red[wave * W1 + 1 + k] = u;
    }
  }
  __syncthreads();
  if (tid < (GRAD ? W1 : 1)) {
    const double s = (red[tid] + red[W1 + tid]) + (red[2 * W1 + tid] + red[3 * W1 + tid]);
    tot[tid] = (tid == 0) ? mean + s : s;
  }
  __syncthreads();
}

// workgroup (b, e): mu_e at candidate c0 + b -> means[e][c0 + b].  cand [.][DP]; member e's set begins at row e * member_stride
// (0: one shared set).
template <int DP>
__global__ __launch_bounds__(kPmmThreads) void pmm_screen_kernel(PmmData T, const double* __restrict__ cand, long member_stride,
                                                                 int c0, int C, double* __restrict__ means) {
  __shared__ double red[4 * (1 + DP)], tot[1 + DP], pt[DP];
  const int e = blockIdx.y, tid = threadIdx.x;
  const long c = (long)c0 + blockIdx.x;
  if (c >= C) return;
  if (tid < DP) pt[tid] = cand[((long)e * member_stride + c) * DP + tid];
  const PmMember& m = T.members[e];
  pmm_eval<DP, false>(m.cp, m.kinvy, m.mean, T.X, T.n, T.dX, pt, red, tot);
  if (tid == 0) means[(long)e * C + c] = tot[0];
}

// numpy.argmin's order on (value, index): the smaller value, a NaN below every number, equal values by index
__device__ __forceinline__ bool pmm_before(double v, int i, double best, int bi) {
  const bool vn = v != v, bn = best != best;
  if (vn != bn) return vn;
  if (!vn && v != best) return v < best;
  return i < bi;
}

// workgroup e: index[e] = numpy.argmin(means[e][0 .. C))
__global__ __launch_bounds__(256) void pmm_argmin_kernel(int C, const double* __restrict__ means, int* __restrict__ index) {
  __shared__ double s_val[4];
  __shared__ int s_idx[4];
  const int tid = threadIdx.x, e = blockIdx.x;
  const double* f = means + (long)e * C;
  double best = 0.0;
  int bi = INT_MAX;  // nothing seen
  for (int i = tid; i < C; i += 256) {
    const double v = f[i];
    if (bi == INT_MAX || pmm_before(v, i, best, bi)) {
      best = v;
      bi = i;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(best, off);
    const int oi = __shfl_down(bi, off);
    if (oi != INT_MAX && (bi == INT_MAX || pmm_before(ov, oi, best, bi))) {
      best = ov;
      bi = oi;
    }
  }
  if ((tid & 63) == 0) {
    s_val[tid >> 6] = best;
    s_idx[tid >> 6] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (s_idx[w] != INT_MAX && (bi == INT_MAX || pmm_before(s_val[w], s_idx[w], best, bi))) {
        best = s_val[w];
        bi = s_idx[w];
      }
    index[e] = (bi == INT_MAX) ? 0 : bi;
  }
}

// pmm_descend's evaluator (pm_descent.hpp): member e's posterior mean through pmm_eval
template <int DP>
struct PmmMeanEval {
  const CovParams& cp;
  const double* kinvy;
  double mean;
  const double* X;
  int n;
  const DerivList& dX;
  template <bool GRAD>
  __device__ __forceinline__ void eval(const double* p, double* red, double* tot) const {
    pmm_eval<DP, GRAD>(cp, kinvy, mean, X, n, dX, p, red, tot);
  }
};

// workgroup e: member e's whole optimisation (pm_descent.hpp: pmm_descend) on f = -mu_e
template <int DP>
__global__ __launch_bounds__(kPmmThreads) void pmm_descent_kernel(PmmData T, PmmDescent D) {
  __shared__ double red[4 * (1 + DP)], tot[1 + DP], xs[DP], pt[DP], gs[DP], xb[DP];
  // the member's covariance and the observed-derivative list: read per training point by every evaluation, kept out of the scalar
  // registers (held there they spilled, and the spills brought scratch with them)
  __shared__ CovParams cp;
  __shared__ DerivList dX;
  const int tid = threadIdx.x, e = blockIdx.x;
  {
    const unsigned int* src = reinterpret_cast<const unsigned int*>(&T.members[e].cp);
    unsigned int* dst = reinterpret_cast<unsigned int*>(&cp);
    for (int i = tid; i < (int)(sizeof(CovParams) / sizeof(unsigned int)); i += kPmmThreads) dst[i] = src[i];
  }
  if (tid == 0) dX = T.dX;
  const PmmMeanEval<DP> ev{cp, T.members[e].kinvy, T.members[e].mean, T.X, T.n, dX};
  pmm_descend<DP>(ev, D, e, (long)e * D.member_stride, T.size, red, tot, xs, pt, gs, xb);
}

template <int DP>
void launch_dp(const PmmData& T, PmmDescent D, int E, double* dMeans, int* dIndex, hipStream_t s) {
  for (int c0 = 0; c0 < D.C; c0 += kPmmPass) {
    const int np = std::min(kPmmPass, D.C - c0);
    MOE_LAUNCH_NOW((pmm_screen_kernel<DP>), dim3((unsigned)np, (unsigned)E), dim3(kPmmThreads), 0, s, T, D.cand, D.member_stride, c0,
                   D.C, dMeans);
  }
  MOE_LAUNCH_NOW(pmm_argmin_kernel, dim3((unsigned)E), dim3(256), 0, s, D.C, (const double*)dMeans, dIndex);
  MOE_LAUNCH_NOW((pmm_descent_kernel<DP>), dim3((unsigned)E), dim3(kPmmThreads), 0, s, T, D);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_pmm_argmin(int rows, int C, const double* values, int* index, hipStream_t s) {
  MOE_LAUNCH_NOW(pmm_argmin_kernel, dim3((unsigned)rows), dim3(256), 0, s, C, values, index);
  MOE_HIP_CHECK(hipGetLastError());
}

void posterior_mean_members_minimize(const std::vector<GpDev*>& gps, int num_fidelity, const moe_gd_params_t& gd,
                                     const double* domain_bounds, const double* candidates, int C, bool per_member,
                                     double* best_points, double* best_values, int* start_index, int* fell_back, double* means_out,
                                     double* trace_out) {
  check_pm_members(gps, num_fidelity);
  GpDev& gp = *gps[0];
  if ((long)gps.size() > 65535) throw Error(MOE_ERR_BOUNDS, "num_mcmc out of range", (double)gps.size(), 1, 65535);
  gp.use_device();
  hipStream_t s = gp.stream;
  const int E = (int)gps.size(), dp = gp.dp, size = gp.d - num_fidelity, T_steps = gd.max_num_steps, R = gd.max_num_restarts;
  // one copy down: [member table | candidates (padded, fidelity coordinates 1) | alpha_0 (T) | bounds (2 size)]
  const size_t rows = (size_t)C * (per_member ? E : 1);
  const size_t nExtra = (size_t)T_steps + 2 * (size_t)size;
  const size_t off = stage_pm_inputs(gps, num_fidelity, candidates, rows, nExtra);
  double* hx = gp.hStateIn.p + off;
  for (int i = 0; i < T_steps; ++i) hx[i] = gd.pre_mult * std::pow((double)(i + 1), -gd.gamma);  // (the host's pow, as the host loop)
  std::copy(domain_bounds, domain_bounds + 2 * (size_t)size, hx + T_steps);
  gp.dStateIn.upload(gp.hStateIn.p, off + nExtra, s, true);
  // the call's doubles, results first (one copy back): [out E (3 + dp) | means E C | trace E R T (size + 6)]
  const size_t tw = (size_t)size + kPmmTraceExtra;
  const size_t nOut = (size_t)E * (kPmmHead + dp), nMeans = (size_t)E * C;
  const size_t nTrace = trace_out ? (size_t)E * R * T_steps * tw : 0;
  gp.pmmD.reserve(nOut + nMeans + nTrace);
  gp.pmmI.reserve((size_t)E);
  if (nTrace) MOE_HIP_CHECK(hipMemsetAsync(gp.pmmD.p + nOut + nMeans, 0, sizeof(double) * nTrace, s));
  PmmData T;
  T.members = reinterpret_cast<const PmMember*>(gp.dStateIn.p);
  T.X = gp.dX.p;
  T.dX = gp.derivs;
  T.n = gp.n;
  T.size = size;
  PmmDescent D;
  D.start_index = gp.pmmI.p;
  D.cand = gp.dStateIn.p + (off - rows * dp);
  D.member_stride = per_member ? C : 0;
  D.alpha0 = gp.dStateIn.p + off;
  D.bounds = D.alpha0 + T_steps;
  D.means = gp.pmmD.p + nOut;
  D.C = C;
  D.T = T_steps;
  D.R = R;
  D.max_relative_change = gd.max_relative_change;
  D.tolerance = gd.tolerance;
  D.step_tol = gd.tolerance / (double)std::max(T_steps, 1);
  D.out = gp.pmmD.p;
  D.trace = nTrace ? gp.pmmD.p + nOut + nMeans : nullptr;
  double* dMeans = gp.pmmD.p + nOut;
  dispatch_dp(dp, [&](auto DP) { launch_dp<DP>(T, D, E, dMeans, gp.pmmI.p, s); });
  const size_t nBack = nOut + ((means_out || trace_out) ? nMeans : 0) + nTrace;
  gp.hStateOut.reserve(nBack);
  gp.pmmD.download(gp.hStateOut.p, nBack, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  const double* h = gp.hStateOut.p;
  for (int e = 0; e < E; ++e) {
    const double* o = h + (size_t)e * (kPmmHead + dp);
    if (start_index) start_index[e] = (int)o[0];
    if (fell_back) fell_back[e] = (int)o[1];
    if (best_values) best_values[e] = o[2];
    if (best_points) std::copy(o + kPmmHead, o + kPmmHead + size, best_points + (size_t)e * size);
  }
  if (means_out) std::memcpy(means_out, h + nOut, sizeof(double) * nMeans);
  if (trace_out) std::memcpy(trace_out, h + nOut + nMeans, sizeof(double) * nTrace);
}

}  // namespace moe
