// cornell_moe_amd/csrc/recommend.hip -- the posterior mean averaged over a hyper-parameter ensemble, at many points, and the
// recommendation step of a Bayesian-optimisation iteration on the device (the reference's examples/main.py:142-157 and :243-260
// over cpp_wrappers/knowledge_gradient_mcmc.py: PosteriorMeanMCMC and python_version/optimization.py: GradientDescentOptimizer).
//
// For E ensemble members over the same n training points, C candidates and S starts, everything in one upload, on one stream, with
// one wait:
//   screen     f(c) = -(1/E) sum_e mu_e(c, fidelity = 1) at every candidate            pm_batch_kernel (one workgroup per point)
//   starts     the S largest f, ties by index                                          pm_select_kernel (one workgroup)
//   descent    T steps of x += clamp(a_i grad f(x)) from each start, Polyak window     pm_descent_kernel (one workgroup per start,
//                                                                                      resident for the whole descent)
//   pick       f at the S end points, the first of the largest, keep or fall back      pm_batch_kernel + pm_pick_kernel
//
// One evaluation of the ensemble at one point (ensemble_sums) belongs to ONE workgroup of W wavefronts.  The members go through in
// groups of MG = min(E, W); inside a group wavefront w takes member w / S and the slice w % S of its training points, S = W / MG,
// lanes striding the slice's points by 64 S.  A wavefront's lanes are added by a butterfly, the slices of a member in slice order and
// the members in ascending order by the thread that owns the component: the order of every sum is a function of (n, E) and the
// kernel's W alone, so a point's bits do not depend on what else is in the call.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_cov.hpp"
#include "gp.hpp"

namespace moe {

namespace {

constexpr int kPmPass = 16384;  // points per launch of pm_batch_kernel (moe_hip.h: moe_posterior_mean_mcmc_batch)

struct PmEnsemble {
  const PmMember* members;  // [E]
  const double* X;          // [n][DP]: the members share the data
  DerivList dX;
  int E, n, size;  // size = dim - num_fidelity: the free coordinates
};

// Sums over the ensemble at the point xs (LDS, [DP], fidelity coordinates 1, padding 0):
//   tot[0] = sum_e mu_e(x), tot[1 + k] = sum_e d mu_e / d x_k (GRAD), members ascending.  Valid for every thread on return.
// red: LDS [WAVES][1 + DP].
template <int DP, int WAVES, bool GRAD>
__device__ __forceinline__ void ensemble_sums(const PmEnsemble& T, const double* __restrict__ X, const double* xs, double* red,
                                              double* tot) {
  constexpr int W1 = 1 + DP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int MG = min(T.E, WAVES), S = WAVES / MG;
  const int lm = wave / S, slice = wave % S;
  const int g1 = 1 + T.dX.g;
  DerivList none;
  none.g = 0;
  double xp[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xp[k] = xs[k];
  double run = 0.0;  // thread c < 1 + DP: component c over the members so far
  for (int e0 = 0; e0 < T.E; e0 += MG) {
    const int e = e0 + lm;
    double acc = 0.0, accg[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) accg[k] = 0.0;
    if (lm < MG && e < T.E) {
      const PmMember& m = T.members[e];
      const double* __restrict__ w_e = m.kinvy;
      for (int j = slice * 64 + lane; j < T.n; j += S * 64) {
        double diff[DP];
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          diff[k] = xp[k] - X[(long)j * DP + k];
          r2 = fma(diff[k] * diff[k], m.cp.inv_l2[k], r2);
        }
        const Radial rd = radial_scalars(m.cp.type, m.cp.alpha, r2);
        for (int b = 0; b < g1; ++b) {
          const double w = w_e[(long)j * g1 + b];
          acc = fma(cov_entry<DP>(m.cp, rd, diff, 0, b, none, T.dX), w, acc);
          if (GRAD) {
#pragma unroll
            for (int dd = 0; dd < DP; ++dd)
              if (dd < m.cp.dim) accg[dd] = fma(grad_cov_entry<DP>(m.cp, rd, diff, 0, b, dd, none, T.dX), w, accg[dd]);
          }
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
      for (int l = 0; l < MG && e0 + l < T.E; ++l) {
        double ge = red[(l * S) * W1 + tid];
        for (int s = 1; s < S; ++s) ge += red[(l * S + s) * W1 + tid];
        if (tid == 0) ge = T.members[e0 + l].mean + ge;
        run += ge;
      }
    }
    __syncthreads();  // (red is written again by the next group)
  }
  if (tid < (GRAD ? W1 : 1)) tot[tid] = run;
  __syncthreads();
}

// workgroup b: point p0 + b of P [.][DP]; value[p] = -(sum mu) / E, grad[p][size] = -(sum grad mu) / E
template <int DP, int WAVES, bool GRAD>
__global__ __launch_bounds__(WAVES * 64) void pm_batch_kernel(PmEnsemble T, const double* __restrict__ P, int p0,
                                                              double* __restrict__ value, double* __restrict__ grad) {
  __shared__ double red[WAVES * (1 + DP)], tot[1 + DP], xs[DP];
  const long p = (long)p0 + blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < DP) xs[tid] = P[p * DP + tid];
  __syncthreads();
  ensemble_sums<DP, WAVES, GRAD>(T, T.X, xs, red, tot);
  const double E = (double)T.E;
  if (tid == 0 && value != nullptr) value[p] = -(tot[0] / E);
  if (GRAD && tid < T.size) grad[p * T.size + tid] = -(tot[1 + tid] / E);
}

// the better of two (value, index) pairs for an argmax: larger value, then smaller index -- the winner of a sequential scan
__device__ __forceinline__ bool pm_better(double v, int i, double best, int bi) {
  if (i == INT_MAX) return false;
  return bi == INT_MAX || v > best || (v == best && i < bi);
}

// One workgroup: index[t], t < S = the candidates with the S largest f, equal values by index (index[0]: numpy.argmin of -f).
// Round t scans the candidates that come after round t - 1's pick in that order.  NaN values are never picked; with nothing left to
// pick a round answers 0.
__global__ __launch_bounds__(256) void pm_select_kernel(int C, int S, const double* __restrict__ f, int* __restrict__ index) {
  __shared__ double s_val[4];
  __shared__ int s_idx[4];
  __shared__ double s_pv;
  __shared__ int s_pi;
  const int tid = threadIdx.x;
  double pv = 0.0;
  int pi = -1;
  for (int t = 0; t < S; ++t) {
    double best = 0.0;
    int bi = INT_MAX;
    for (int i = tid; i < C; i += 256) {  // i ascends: the first index of this thread's maximum
      const double v = f[i];
      const bool open = v == v && (t == 0 || v < pv || (v == pv && i > pi));
      if (open && (bi == INT_MAX || v > best)) {
        best = v;
        bi = i;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_down(best, off);
      const int oi = __shfl_down(bi, off);
      if (pm_better(ov, oi, best, bi)) {
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
        if (pm_better(s_val[w], s_idx[w], best, bi)) {
          best = s_val[w];
          bi = s_idx[w];
        }
      if (bi == INT_MAX) bi = 0;
      index[t] = bi;
      s_pv = best;
      s_pi = bi;
    }
    __syncthreads();
    pv = s_pv;
    pi = s_pi;
  }
}

struct PmDescent {
  const int* start_index;  // [S] into cand
  const double* cand;      // [C][DP]
  const double* step;      // [T]: a_i = pre_mult i^-gamma, i = 1 .. T
  const double* bounds;    // [size][2]
  int T, window;           // window: the last `window` steps are averaged
  double max_relative_change;
  double* ends;  // [S][DP]
  double* path;  // [S][T + 1][size] or NULL
};

// workgroup b: the whole descent of start b (python_version/optimization.py:498-527, domain.py:187-200)
template <int DP, int WAVES, bool XLDS>
__global__ __launch_bounds__(WAVES * 64) void pm_descent_kernel(PmEnsemble T, PmDescent D) {
  extern __shared__ double x_lds[];  // XLDS: the training points [n][DP]
  __shared__ double red[WAVES * (1 + DP)], tot[1 + DP], xs[DP];
  const int tid = threadIdx.x, b = blockIdx.x, size = T.size;
  const double* X = T.X;
  if (XLDS) {
    for (long i = tid; i < (long)T.n * DP; i += WAVES * 64) x_lds[i] = T.X[i];
    X = x_lds;
  }
  double x = 0.0, lo = 0.0, hi = 0.0, wsum = 0.0;
  double* path = D.path ? D.path + (size_t)b * (D.T + 1) * size : nullptr;
  if (tid < DP) {
    x = D.cand[(size_t)D.start_index[b] * DP + tid];
    xs[tid] = x;
    if (tid < size) {
      lo = D.bounds[2 * tid];
      hi = D.bounds[2 * tid + 1];
      if (path) path[tid] = x;
    }
  }
  __syncthreads();
  const double E = (double)T.E;
  for (int i = 1; i <= D.T; ++i) {
    ensemble_sums<DP, WAVES, true>(T, X, xs, red, tot);  // (ends in a barrier: every thread has read xs)
    if (tid < size) {
      double step = D.step[i - 1] * -(tot[1 + tid] / E);
      const double limit = D.max_relative_change * fmin(x - lo, hi - x);
      if (fabs(step) > limit) step = copysign(limit, step);
      x = x + step;
      xs[tid] = x;
      if (i > D.T - D.window) wsum += x;
      if (path) path[(size_t)i * size + tid] = x;
    }
    __syncthreads();
  }
  if (tid < DP) D.ends[(size_t)b * DP + tid] = (tid < size) ? wsum / (double)D.window : x;
}

// One thread: the winner among the S end points (the first of the largest f: MultistartOptimizer.optimize's strict compare), then
// main.py:259-260: the screened candidate unless the winner is at least as good.
//   head = [screened index | refined | value | winner | point (DP)]
__global__ void pm_pick_kernel(int S, int DP, const int* __restrict__ index, const double* __restrict__ cand_f,
                               const double* __restrict__ end_f, const double* __restrict__ cand, const double* __restrict__ ends,
                               double* __restrict__ head) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int w = 0;
  double best = -INFINITY;
  for (int s = 0; s < S; ++s)
    if (end_f[s] > best) {
      best = end_f[s];
      w = s;
    }
  const int i0 = index[0];
  const double fw = end_f[w], f0 = cand_f[i0];
  const bool fall_back = -fw > -f0;
  const double* src = fall_back ? cand + (size_t)i0 * DP : ends + (size_t)w * DP;
  head[0] = (double)i0;
  head[1] = fall_back ? 0.0 : 1.0;
  head[2] = fall_back ? f0 : fw;
  head[3] = (double)w;
  for (int k = 0; k < DP; ++k) head[4 + k] = src[k];
}

PmEnsemble ensemble_of(const std::vector<GpDev*>& gps, int num_fidelity, const double* d_in) {
  const GpDev& gp = *gps[0];
  PmEnsemble T;
  T.members = reinterpret_cast<const PmMember*>(d_in);
  T.X = gp.dX.p;
  T.dX = gp.derivs;
  T.E = (int)gps.size();
  T.n = gp.n;
  T.size = gp.d - num_fidelity;
  return T;
}

// wavefronts per workgroup, from the padded dimension: a lane holds the point, the differences and the gradient accumulators
// (3 DP doubles), and a workgroup of 16 / 8 / 4 wavefronts leaves a lane 128 / 256 / 512 registers
constexpr int waves_of(int dp) { return dp <= 4 ? 16 : (dp <= 16 ? 8 : 4); }

template <int DP>
void batch_dp(const PmEnsemble& T, const double* dP, int P, bool want_grad, double* dValue, double* dGrad, hipStream_t s) {
  constexpr int W = waves_of(DP);
  for (int p0 = 0; p0 < P; p0 += kPmPass) {
    const int np = std::min(kPmPass, P - p0);
    if (want_grad)
      MOE_LAUNCH_NOW((pm_batch_kernel<DP, W, true>), dim3((unsigned)np), dim3(W * 64), 0, s, T, dP, p0, dValue, dGrad);
    else
      MOE_LAUNCH_NOW((pm_batch_kernel<DP, W, false>), dim3((unsigned)np), dim3(W * 64), 0, s, T, dP, p0, dValue, dGrad);
  }
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_batch(int dp, const PmEnsemble& T, const double* dP, int P, bool want_grad, double* dValue, double* dGrad, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) { batch_dp<DP>(T, dP, P, want_grad, dValue, dGrad, s); });
}

// MOE_RECOMMEND_XLDS=1: the descent stages the training points in LDS where they fit (A/B runs; same bits either way)
bool descent_x_in_lds(int n, int dp) {
  const char* v = std::getenv("MOE_RECOMMEND_XLDS");
  return v != nullptr && *v == '1' && sizeof(double) * (size_t)n * dp <= 96 * 1024;
}

template <int DP>
void descent_dp(const PmEnsemble& T, const PmDescent& D, int S, hipStream_t s) {
  constexpr int W = waves_of(DP);
  if (descent_x_in_lds(T.n, DP)) {
    const size_t shm = sizeof(double) * (size_t)T.n * DP;
    auto kernel = pm_descent_kernel<DP, W, true>;
    if (shm > 48 * 1024)
      MOE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    MOE_LAUNCH_NOW(kernel, dim3((unsigned)S), dim3(W * 64), shm, s, T, D);
  } else {
    MOE_LAUNCH_NOW((pm_descent_kernel<DP, W, false>), dim3((unsigned)S), dim3(W * 64), 0, s, T, D);
  }
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_descent(int dp, const PmEnsemble& T, const PmDescent& D, int S, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) { descent_dp<DP>(T, D, S, s); });
}

}  // namespace

void check_pm_members(const std::vector<GpDev*>& gps, int num_fidelity) {
  if (gps.empty()) throw Error(MOE_ERR_BOUNDS, "num_mcmc must be positive", 0, 1, 1e9);
  const GpDev* g0 = gps[0];
  for (const GpDev* g : gps) {
    if (g == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL GP handle in the MCMC ensemble");
    if (g->d != g0->d || g->g != g0->g || !std::equal(g->derivs.idx, g->derivs.idx + g->g, g0->derivs.idx))
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share dim and the observed-derivative list", g->d, g0->d, 0);
    if (g->n != g0->n || g->X != g0->X)
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share the sampled points", g->n, g0->n, 0);
    if (g->device != g0->device) throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must live on one device", g->device, g0->device, 0);
  }
  if (num_fidelity < 0 || num_fidelity >= g0->d) throw Error(MOE_ERR_BOUNDS, "num_fidelity out of range", num_fidelity, 0, g0->d - 1);
}

size_t stage_pm_inputs(const std::vector<GpDev*>& gps, int num_fidelity, const double* pts, size_t rows, size_t extra) {
  GpDev& gp = *gps[0];
  const int E = (int)gps.size(), dp = gp.dp, size = gp.d - num_fidelity;
  const size_t nTab = (size_t)E * sizeof(PmMember) / sizeof(double), nP = rows * dp;
  gp.hStateIn.reserve(nTab + nP + extra);
  for (int e = 0; e < E; ++e) {
    PmMember m;
    std::memset(&m, 0, sizeof(m));
    m.cp = gps[e]->cp;
    m.kinvy = gps[e]->dKinvY.p;
    m.mean = gps[e]->mean;
    std::memcpy(reinterpret_cast<unsigned char*>(gp.hStateIn.p) + (size_t)e * sizeof(PmMember), &m, sizeof(m));
  }
  double* hp = gp.hStateIn.p + nTab;
  for (size_t i = 0; i < rows; ++i)
    for (int k = 0; k < dp; ++k) hp[i * dp + k] = (k < size) ? pts[i * size + k] : (k < gp.d ? 1.0 : 0.0);
  return nTab + nP;
}

void posterior_mean_mcmc_batch(const std::vector<GpDev*>& gps, int num_fidelity, const double* pts, int P, double* value_out,
                               double* grad_out) {
  check_pm_members(gps, num_fidelity);
  if (P < 1) throw Error(MOE_ERR_BOUNDS, "the number of points must be positive", P, 1, 1e9);
  if (pts == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL argument");
  if (value_out == nullptr && grad_out == nullptr) return;
  GpDev& gp = *gps[0];
  gp.use_device();
  hipStream_t s = gp.stream;
  const int size = gp.d - num_fidelity;
  const size_t nIn = stage_pm_inputs(gps, num_fidelity, pts, P, 0);
  gp.dStateIn.upload(gp.hStateIn.p, nIn, s, true);
  const PmEnsemble T = ensemble_of(gps, num_fidelity, gp.dStateIn.p);
  const double* dP = gp.dStateIn.p + (nIn - (size_t)P * gp.dp);
  const bool want_grad = grad_out != nullptr;
  const size_t nOut = (size_t)P * (want_grad ? 1 + size : 1);
  gp.recD.reserve(nOut);
  launch_batch(gp.dp, T, dP, P, want_grad, gp.recD.p, gp.recD.p + P, s);
  gp.hStateOut.reserve(nOut);
  gp.recD.download(gp.hStateOut.p, nOut, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  if (value_out) std::memcpy(value_out, gp.hStateOut.p, sizeof(double) * (size_t)P);
  if (want_grad) std::memcpy(grad_out, gp.hStateOut.p + P, sizeof(double) * (size_t)P * size);
}

void posterior_mean_mcmc_recommend(const std::vector<GpDev*>& gps, int num_fidelity, const moe_gd_params_t& gd,
                                   const double* domain_bounds, const double* candidates, int C, int S, double* point_out,
                                   double* value_out, int* screened_index_out, int* refined_out, double* candidate_values_out,
                                   double* end_points_out, double* path_out) {
  check_pm_members(gps, num_fidelity);
  GpDev& gp = *gps[0];
  gp.use_device();
  hipStream_t s = gp.stream;
  const int dp = gp.dp, size = gp.d - num_fidelity, T_steps = gd.max_num_steps;
  const int nsa = gd.num_steps_averaged;
  const int window = (nsa < 0 || nsa > T_steps) ? T_steps : (nsa == 0 ? 1 : nsa);  // _get_averaging_range (:435-442)
  // one copy down: [member table | candidates | a_i (T) | bounds (2 size)]
  const size_t nExtra = (size_t)T_steps + 2 * (size_t)size;
  const size_t off = stage_pm_inputs(gps, num_fidelity, candidates, C, nExtra);
  double* hx = gp.hStateIn.p + off;
  for (int i = 1; i <= T_steps; ++i) hx[i - 1] = gd.pre_mult * std::pow((double)i, -gd.gamma);
  std::copy(domain_bounds, domain_bounds + 2 * (size_t)size, hx + T_steps);
  gp.dStateIn.upload(gp.hStateIn.p, off + nExtra, s, true);
  const PmEnsemble Tens = ensemble_of(gps, num_fidelity, gp.dStateIn.p);
  const double* dCand = gp.dStateIn.p + (off - (size_t)C * dp);
  const double* dExtra = gp.dStateIn.p + off;
  // the call's doubles, results first (one copy back): [head (4 + dp) | end points S dp | f(end points) S | f(candidates) C | path]
  const size_t nHead = 4 + (size_t)dp, nEnds = (size_t)S * dp, nPath = path_out ? (size_t)S * (T_steps + 1) * size : 0;
  gp.recD.reserve(nHead + nEnds + S + C + nPath);
  gp.recI.reserve((size_t)S);
  double* dHead = gp.recD.p;
  double* dEnds = dHead + nHead;
  double* dEndF = dEnds + nEnds;
  double* dCandF = dEndF + S;
  double* dPath = dCandF + C;
  launch_batch(dp, Tens, dCand, C, false, dCandF, nullptr, s);
  MOE_LAUNCH_NOW(pm_select_kernel, dim3(1), dim3(256), 0, s, C, S, (const double*)dCandF, gp.recI.p);
  PmDescent D;
  D.start_index = gp.recI.p;
  D.cand = dCand;
  D.step = dExtra;
  D.bounds = dExtra + T_steps;
  D.T = T_steps;
  D.window = window;
  D.max_relative_change = gd.max_relative_change;
  D.ends = dEnds;
  D.path = path_out ? dPath : nullptr;
  launch_descent(dp, Tens, D, S, s);
  launch_batch(dp, Tens, dEnds, S, false, dEndF, nullptr, s);
  MOE_LAUNCH_NOW(pm_pick_kernel, dim3(1), dim3(64), 0, s, S, dp, (const int*)gp.recI.p, (const double*)dCandF, (const double*)dEndF,
                 dCand, (const double*)dEnds, dHead);
  MOE_HIP_CHECK(hipGetLastError());
  const size_t nBack = nHead + nEnds + S + ((candidate_values_out || path_out) ? (size_t)C : 0) + nPath;
  gp.hStateOut.reserve(nBack);
  gp.recD.download(gp.hStateOut.p, nBack, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  const double* h = gp.hStateOut.p;
  if (screened_index_out) *screened_index_out = (int)h[0];
  if (refined_out) *refined_out = (int)h[1];
  if (value_out) *value_out = h[2];
  if (point_out) std::copy(h + 4, h + 4 + size, point_out);
  if (end_points_out)
    for (int b = 0; b < S; ++b) std::copy(h + nHead + (size_t)b * dp, h + nHead + (size_t)b * dp + size, end_points_out + (size_t)b * size);
  if (candidate_values_out) std::memcpy(candidate_values_out, h + nHead + nEnds + S, sizeof(double) * (size_t)C);
  if (path_out) std::memcpy(path_out, h + nHead + nEnds + S + C, sizeof(double) * nPath);
}

}  // namespace moe
