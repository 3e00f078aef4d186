// cornell_moe_amd/csrc/paths.hip -- posterior function paths by pathwise conditioning (Wilson et al. 2020) on the factor the GP holds,
// and their minimisers: moe_gp_paths_evaluate and moe_gp_paths_minimize (the reference's moe/optimal_learning/python/
// random_features.py in purpose; not its weight-space posterior).
//
// Member e: a GP without derivative observations, signal variance alpha, lengths l, noise s^2, constant mean m, K + s^2 I = L L^T.
// Tables: frequencies Om [M][dim] (unit scale) and phases b [M] for the whole call; weights w [E][S][M] and noise normals z [E][S][n]
// per path s of member e.
//   om_i = Om_i / l,   g_s(x) = sqrt(2 alpha / M) sum_i w_si cos(om_i . x + b_i)
//   v_s  = K^-1 (y - m - g_s(X) - s z_s)
//   f_s(x) = m + g_s(x) + sum_j v_sj k(x, X_j)
//
//   set      g_s(X_j) and the residual columns [n][S] of every member         paths_design_kernel (one workgroup per (member, row))
//            v = L^-T (L^-1 r): the chain that forms K^-1 (y - m), S columns   launch_tri_gemm_cols against the member's L^-1
//   screen   f_s at every (member, point), all the member's paths at once      paths_points_kernel (one workgroup per (member, point))
//   gradient f_s and grad f_s of one (path, point)                             paths_grad_kernel (one workgroup per evaluation)
//   select   start_index = numpy.argmin of a path's screened values            pm_members.hip's pmm_argmin_kernel, E S rows
//   descend  pm_members.hip's line search on -f_s, then keep or fall back      paths_descent_kernel (one workgroup per path)
//
// One evaluation (path_eval) belongs to ONE workgroup of 256 threads: thread t takes the features t, t + 256, ... and then the rows
// t, t + 256, ..., each sum in an accumulator of its own; the thread's term is fma(scale, features, rows); a wavefront's lanes are
// added by a butterfly and the four wavefronts as (0 + 1) + (2 + 3).  The order is a function of (M, n) alone.  paths_points_kernel
// computes a point's cosines and covariance entries once, by the thread that owns them in that order (kept in LDS: all M features and
// the first kPathRowCache rows; rows past that are recomputed per chunk), and contracts them with the weights of 8 paths at a time:
// every (path, point) sum has path_eval's order and its bits, whatever C, S, E and want_grad share the call.
// The descent is pm_descent.hpp's pmm_descend, the body pm_members.hip's pmm_descent_kernel runs, with path_eval as its evaluator.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_cov.hpp"
#include "gp.hpp"
#include "pm_descent.hpp"

namespace moe {

namespace {

constexpr int kPathPass = 16384;      // points per launch
constexpr int kPathThreads = kPmmThreads;  // the feature and row stride of an evaluation
constexpr int kPathChunk = 8;         // paths contracted per pass over a point's features and rows
constexpr int kPathRowCache = 3584;   // rows of a point's covariance column kept in LDS beside the M <= 4096 cosines (60 KB)

static_assert(sizeof(CovParams) % sizeof(unsigned int) == 0, "the descent copies a member's covariance into LDS by words");

struct PathData {
  const PmMember* members;  // [E]; kinvy is not read
  const double* X;          // [n][DP]: the members share the data
  const double* Om;         // [M][DP], padding 0
  const double* ph;         // [M]
  const double* W;          // [E][S][M]
  const double* V;          // [E][S][n]: v_s
  const double* scale;      // [E]: sqrt(2 alpha / M)
  int n, M, S, dim;
};

// om_i . x + b_i
template <int DP>
__device__ __forceinline__ double path_arg(const CovParams& cp, const double* __restrict__ om, double b, const double (&xp)[DP]) {
  double a = b;
#pragma unroll
  for (int k = 0; k < DP; ++k) a = fma(om[k] * cp.inv_l[k], xp[k], a);
  return a;
}

// k(x, X_j) and x - X_j
template <int DP>
__device__ __forceinline__ Radial path_row(const CovParams& cp, const double* __restrict__ xj, const double (&xp)[DP], double (&diff)[DP]) {
  double r2 = 0.0;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    diff[k] = xp[k] - xj[k];
    r2 = fma(diff[k] * diff[k], cp.inv_l2[k], r2);
  }
  return radial_scalars(cp.type, cp.alpha, r2);
}

// f_s (and with GRAD d f_s / d x_k) of the path (w [M], v [n]) of the member (cp, scale, mean) at the point pt (LDS, [DP], padding 0):
//   tot[0] = f_s, tot[1 + k] = d f_s / d x_k.  Valid for every thread on return.  red: LDS [4][1 + DP].
// Begins with a barrier (pt is visible, the previous tot has been read) and ends with one.
template <int DP, bool GRAD>
__device__ __forceinline__ void path_eval(const CovParams& cp, double scale, double mean, const PathData& T, const double* __restrict__ w,
                                          const double* __restrict__ v, const double* pt, double* red, double* tot) {
  constexpr int W1 = 1 + DP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();
  double xp[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xp[k] = pt[k];
  double accf = 0.0, acck = 0.0, accgf[DP], accgk[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) accgf[k] = accgk[k] = 0.0;
  for (int i = tid; i < T.M; i += kPathThreads) {
    const double* om = T.Om + (long)i * DP;
    const double a = path_arg<DP>(cp, om, T.ph[i], xp), wi = w[i];
    accf = fma(wi, cos(a), accf);
    if (GRAD) {
      const double ws = -(wi * sin(a));
#pragma unroll
      for (int k = 0; k < DP; ++k) accgf[k] = fma(ws, om[k] * cp.inv_l[k], accgf[k]);
    }
  }
  for (int j = tid; j < T.n; j += kPathThreads) {
    double diff[DP];
    const Radial rd = path_row<DP>(cp, T.X + (long)j * DP, xp, diff);
    const double vj = v[j];
    acck = fma(rd.base, vj, acck);
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < DP; ++k) accgk[k] = fma((-diff[k] * cp.inv_l2[k]) * rd.first, vj, accgk[k]);
    }
  }
  double u = fma(scale, accf, acck);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) u += __shfl_xor(u, off, 64);
  if (lane == 0) red[wave * W1] = u;
  if (GRAD) {
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      double g = fma(scale, accgf[k], accgk[k]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) g += __shfl_xor(g, off, 64);
      if (lane == 0) red[wave * W1 + 1 + k] = g;
    }
  }
  __syncthreads();
  if (tid < (GRAD ? W1 : 1)) {
    const double s = (red[tid] + red[W1 + tid]) + (red[2 * W1 + tid] + red[3 * W1 + tid]);
    tot[tid] = (tid == 0) ? mean + s : s;
  }
  __syncthreads();
}

// The sums of every path of member e at one point xp, path_eval's order: emit(s, (0 + 1) + (2 + 3)) by thread s % 8 for s < S.
// ROWS = false leaves the covariance rows out (the set phase: g_s alone, scale applied).  cache: LDS [M + min(n, kPathRowCache)].
template <int DP, bool ROWS, class Emit>
__device__ __forceinline__ void paths_point_sums(const CovParams& cp, double scale, const PathData& T, int e, const double (&xp)[DP],
                                                 double* cache, double* red, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = T.M, n = T.n, S = T.S;
  const double* We = T.W + (long)e * S * M;
  const double* Ve = ROWS ? T.V + (long)e * S * n : nullptr;
  for (int s0 = 0; s0 < S; s0 += kPathChunk) {
    double accf[kPathChunk], acck[kPathChunk];
#pragma unroll
    for (int p = 0; p < kPathChunk; ++p) accf[p] = acck[p] = 0.0;
    for (int i = tid; i < M; i += kPathThreads) {
      double c;
      if (s0 == 0) {
        c = cos(path_arg<DP>(cp, T.Om + (long)i * DP, T.ph[i], xp));
        cache[i] = c;
      } else {
        c = cache[i];
      }
#pragma unroll
      for (int p = 0; p < kPathChunk; ++p)
        if (s0 + p < S) accf[p] = fma(We[(long)(s0 + p) * M + i], c, accf[p]);
    }
    if (ROWS) {
      for (int j = tid; j < n; j += kPathThreads) {
        double kj;
        if (s0 == 0 || j >= kPathRowCache) {
          double diff[DP];
          kj = path_row<DP>(cp, T.X + (long)j * DP, xp, diff).base;
          if (j < kPathRowCache) cache[M + j] = kj;
        } else {
          kj = cache[M + j];
        }
#pragma unroll
        for (int p = 0; p < kPathChunk; ++p)
          if (s0 + p < S) acck[p] = fma(kj, Ve[(long)(s0 + p) * n + j], acck[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < kPathChunk; ++p) {
      double u = fma(scale, accf[p], acck[p]);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) u += __shfl_xor(u, off, 64);
      if (lane == 0) red[wave * kPathChunk + p] = u;
    }
    __syncthreads();
    if (tid < kPathChunk && s0 + tid < S)
      emit(s0 + tid, (red[tid] + red[kPathChunk + tid]) + (red[2 * kPathChunk + tid] + red[3 * kPathChunk + tid]));
    __syncthreads();
  }
}

// workgroup (j, e): column entries j of member e's residuals, R[e][s][j] = (y_j - m) - g_s(X_j) - sigma z_sj
template <int DP>
__global__ __launch_bounds__(kPathThreads) void paths_design_kernel(PathData T, const double* __restrict__ yc, const double* __restrict__ sigma,
                                                                    const double* __restrict__ Z, double* __restrict__ R) {
  extern __shared__ double path_cache[];
  __shared__ double red[4 * kPathChunk];
  const int e = blockIdx.y, j = blockIdx.x, n = T.n, S = T.S;
  double xp[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xp[k] = T.X[(long)j * DP + k];
  const double ycj = yc[(long)e * n + j], sg = sigma[e];
  const double* Ze = Z + (long)e * S * n;
  double* Re = R + (long)e * S * n;
  paths_point_sums<DP, false>(T.members[e].cp, T.scale[e], T, e, xp, path_cache, red, [&](int s, double g) {
#pragma clang fp contract(off)
    Re[(long)s * n + j] = (ycj - g) - sg * Ze[(long)s * n + j];
  });
}

// workgroup (b, e): f_s at point c0 + b for every path s of member e -> values[e][s][c0 + b].  pts [C][DP]
template <int DP>
__global__ __launch_bounds__(kPathThreads) void paths_points_kernel(PathData T, const double* __restrict__ pts, int c0, int C,
                                                                    double* __restrict__ values) {
  extern __shared__ double path_cache[];
  __shared__ double red[4 * kPathChunk];
  const int e = blockIdx.y, S = T.S;
  const long c = (long)c0 + blockIdx.x;
  if (c >= C) return;
  double xp[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xp[k] = pts[c * DP + k];
  const double mean = T.members[e].mean;
  double* out = values + (long)e * S * C + c;
  paths_point_sums<DP, true>(T.members[e].cp, T.scale[e], T, e, xp, path_cache, red, [&](int s, double sum) { out[(long)s * C] = mean + sum; });
}

// workgroup (b, e S + s): f_s and its gradient at point c0 + b -> values[e][s][c], grad[e][s][c][dim]
template <int DP>
__global__ __launch_bounds__(kPathThreads) void paths_grad_kernel(PathData T, const double* __restrict__ pts, int c0, int C,
                                                                  double* __restrict__ values, double* __restrict__ grad) {
  __shared__ double red[4 * (1 + DP)], tot[1 + DP], pt[DP];
  __shared__ CovParams cp;
  const int r = blockIdx.y, e = r / T.S, tid = threadIdx.x;
  const long c = (long)c0 + blockIdx.x;
  if (c >= C) return;
  {
    const unsigned int* src = reinterpret_cast<const unsigned int*>(&T.members[e].cp);
    unsigned int* dst = reinterpret_cast<unsigned int*>(&cp);
    for (int i = tid; i < (int)(sizeof(CovParams) / sizeof(unsigned int)); i += kPathThreads) dst[i] = src[i];
  }
  if (tid < DP) pt[tid] = pts[c * DP + tid];
  path_eval<DP, true>(cp, T.scale[e], T.members[e].mean, T, T.W + (long)r * T.M, T.V + (long)r * T.n, pt, red, tot);
  if (tid == 0) values[(long)r * C + c] = tot[0];
  if (tid < T.dim) grad[((long)r * C + c) * T.dim + tid] = tot[1 + tid];
}

// pmm_descend's evaluator (pm_descent.hpp): one path through path_eval
template <int DP>
struct PathEval {
  const CovParams& cp;
  double scale, mean;
  const PathData& T;
  const double* w;
  const double* v;
  template <bool GRAD>
  __device__ __forceinline__ void eval(const double* p, double* red, double* tot) const {
    path_eval<DP, GRAD>(cp, scale, mean, T, w, v, p, red, tot);
  }
};

// workgroup r = e S + s: the whole optimisation of path s of member e (pm_descent.hpp: pmm_descend, pmm_descent_kernel's body) on
// f = -f_s, from the path's best candidate of the shared set
template <int DP>
__global__ __launch_bounds__(kPmmThreads) void paths_descent_kernel(PathData T, PmmDescent D) {
  __shared__ double red[4 * (1 + DP)], tot[1 + DP], xs[DP], pt[DP], gs[DP], xb[DP];
  __shared__ CovParams cp;  // read per feature and per row by every evaluation: kept out of the scalar registers (pm_members.hip)
  const int tid = threadIdx.x, r = blockIdx.x, e = r / T.S;
  {
    const unsigned int* src = reinterpret_cast<const unsigned int*>(&T.members[e].cp);
    unsigned int* dst = reinterpret_cast<unsigned int*>(&cp);
    for (int i = tid; i < (int)(sizeof(CovParams) / sizeof(unsigned int)); i += kPmmThreads) dst[i] = src[i];
  }
  const PathEval<DP> ev{cp, T.scale[e], T.members[e].mean, T, T.W + (long)r * T.M, T.V + (long)r * T.n};
  pmm_descend<DP>(ev, D, r, 0, T.dim, red, tot, xs, pt, gs, xb);
}

size_t cache_bytes(int M, int n) { return sizeof(double) * ((size_t)M + (size_t)std::min(n, kPathRowCache)); }

template <int DP>
void launch_design(const PathData& T, int E, const double* yc, const double* sigma, const double* Z, double* R, hipStream_t s) {
  MOE_LAUNCH_NOW((paths_design_kernel<DP>), dim3((unsigned)T.n, (unsigned)E), dim3(kPathThreads), cache_bytes(T.M, 0), s, T, yc, sigma, Z, R);
  MOE_HIP_CHECK(hipGetLastError());
}

template <int DP>
void launch_points(const PathData& T, int E, const double* pts, int C, double* values, double* grad, hipStream_t s) {
  for (int c0 = 0; c0 < C; c0 += kPathPass) {
    const int np = std::min(kPathPass, C - c0);
    if (grad != nullptr)
      MOE_LAUNCH_NOW((paths_grad_kernel<DP>), dim3((unsigned)np, (unsigned)(E * T.S)), dim3(kPathThreads), 0, s, T, pts, c0, C, values, grad);
    else
      MOE_LAUNCH_NOW((paths_points_kernel<DP>), dim3((unsigned)np, (unsigned)E), dim3(kPathThreads), cache_bytes(T.M, T.n), s, T, pts, c0,
                     C, values);
  }
  MOE_HIP_CHECK(hipGetLastError());
}

template <int DP>
void launch_descent(const PathData& T, const PmmDescent& D, int rows, hipStream_t s) {
  MOE_LAUNCH_NOW((paths_descent_kernel<DP>), dim3((unsigned)rows), dim3(kPathThreads), 0, s, T, D);
  MOE_HIP_CHECK(hipGetLastError());
}

// the members' checks, after the handles are known to be non-NULL
void check_path_members(const std::vector<GpDev*>& gps) {
  const GpDev* g0 = gps[0];
  for (size_t e = 0; e < gps.size(); ++e) {
    const GpDev* g = gps[e];
    if (g->d != g0->d) throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share dim", g->d, g0->d, (double)e);
    if (g->device != g0->device)
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must live on one device", g->device, g0->device, (double)e);
    if (g->n != g0->n || g->X != g0->X)
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share the sampled points", g->n, g0->n, (double)e);
    if (g->cp.type != g0->cp.type)
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share cov_type: the frequencies are drawn for one spectral density",
                  g->cp.type, g0->cp.type, (double)e);
  }
  for (size_t e = 0; e < gps.size(); ++e)
    if (gps[e]->g != 0)
      throw Error(MOE_ERR_INVALID_VALUE, "posterior paths need members without derivative observations (their rows would need sine features)",
                  gps[e]->g, 0, (double)e);
}

// The call's operands behind stage_pm_inputs' [member table | points]: [Om M dp | ph M | W E S M | Z E S n | yc E n | sigma E |
// scale E | tail], one copy down; then the set phase into V (and its scratch behind it).  Returns the offset of the tail.
struct PathStage {
  PathData T;
  const double* dPts;
  size_t tail;
};
PathStage stage_and_set(const std::vector<GpDev*>& gps, const double* frequencies, const double* phases, int M, const double* weights,
                        const double* noise_normals, int S, const double* pts, int C, size_t nTail,
                        const std::function<void(double*)>& fill_tail, double* dV) {
  GpDev& gp = *gps[0];
  hipStream_t s = gp.stream;
  const int E = (int)gps.size(), dp = gp.dp, d = gp.d, n = gp.n;
  const size_t nOm = (size_t)M * dp, nW = (size_t)E * S * M, nZ = (size_t)E * S * n, nY = (size_t)E * n;
  const size_t nExtra = nOm + M + nW + nZ + nY + 2 * (size_t)E + nTail;
  const size_t off = stage_pm_inputs(gps, 0, pts, (size_t)C, nExtra);
  double* h = gp.hStateIn.p + off;
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < dp; ++k) h[(size_t)i * dp + k] = (k < d) ? frequencies[(size_t)i * d + k] : 0.0;
  double* hph = h + nOm;
  std::copy(phases, phases + M, hph);
  double* hW = hph + M;
  std::copy(weights, weights + nW, hW);
  double* hZ = hW + nW;
  std::copy(noise_normals, noise_normals + nZ, hZ);
  double* hY = hZ + nZ;
  double* hSig = hY + nY;
  double* hScale = hSig + E;
  for (int e = 0; e < E; ++e) {
    const GpDev& g = *gps[e];
    for (int j = 0; j < n; ++j) hY[(size_t)e * n + j] = g.y[j] - g.mean;
    hSig[e] = std::sqrt(g.noise[0]);
    hScale[e] = std::sqrt(2.0 * g.cp.alpha / (double)M);
  }
  if (nTail) fill_tail(hScale + E);
  gp.dStateIn.upload(gp.hStateIn.p, off + nExtra, s, true);
  const double* dIn = gp.dStateIn.p + off;
  PathStage P;
  P.T.members = reinterpret_cast<const PmMember*>(gp.dStateIn.p);
  P.T.X = gp.dX.p;
  P.T.Om = dIn;
  P.T.ph = dIn + nOm;
  P.T.W = P.T.ph + M;
  const double* dZ = P.T.W + nW;
  const double* dY = dZ + nZ;
  const double* dSig = dY + nY;
  P.T.scale = dSig + E;
  P.T.V = dV;
  P.T.n = n;
  P.T.M = M;
  P.T.S = S;
  P.T.dim = d;
  P.dPts = gp.dStateIn.p + (off - (size_t)C * dp);
  P.tail = off + nExtra - nTail;
  // set: residual columns into V, L^-1 of them into the scratch behind V, L^-T of those back into V
  double* dTmp = dV + nZ;
  dispatch_dp(dp, [&](auto DP) { launch_design<DP>(P.T, E, dY, dSig, dZ, dV, s); });
  if (n >= 128) gp.dEK.reserve(tri_cols_work_doubles(n, S));
  for (int e = 0; e < E; ++e) {
    const GpDev& g = *gps[e];
    double* ve = dV + (size_t)e * S * n;
    double* te = dTmp + (size_t)e * S * n;
    launch_tri_gemm_cols('N', n, S, 17, g.dLinv.p, g.ldL, ve, n, te, n, gp.dEK.p, s);
    launch_tri_gemm_cols('T', n, S, 17, g.dLinv.p, g.ldL, te, n, ve, n, gp.dEK.p, s);
  }
  return P;
}

}  // namespace

void check_paths_shapes(int num_features, int num_paths, int num_mcmc) {
  if (num_features < 1 || num_features > kPathsMaxFeatures)
    throw Error(MOE_ERR_BOUNDS, "num_features must be between 1 and 4096", num_features, 1, kPathsMaxFeatures);
  if (num_paths < 1 || num_paths > kPathsMaxPaths)
    throw Error(MOE_ERR_BOUNDS, "num_paths must be between 1 and 1024", num_paths, 1, kPathsMaxPaths);
  if (num_mcmc < 1 || num_mcmc > 1024) throw Error(MOE_ERR_BOUNDS, "num_mcmc must be between 1 and 1024", num_mcmc, 1, 1024);
  if ((long)num_mcmc * num_paths > 65535)
    throw Error(MOE_ERR_BOUNDS, "num_mcmc x num_paths out of range", (double)num_mcmc * num_paths, 1, 65535);
}

void paths_evaluate(const std::vector<GpDev*>& gps, const double* frequencies, const double* phases, int M, const double* weights,
                    const double* noise_normals, int S, const double* pts, int C, bool want_grad, double* values, double* grad) {
  check_path_members(gps);
  GpDev& gp = *gps[0];
  gp.use_device();
  hipStream_t s = gp.stream;
  const int E = (int)gps.size(), d = gp.d, n = gp.n;
  // the call's doubles, results first (one copy back): [values E S C | grad E S C d | V E S n | scratch E S n]
  const size_t nVal = (size_t)E * S * C, nGrad = want_grad ? nVal * d : 0, nV = (size_t)E * S * n;
  gp.pathD.reserve(nVal + nGrad + 2 * nV);
  double* dV = gp.pathD.p + nVal + nGrad;
  const PathStage P = stage_and_set(gps, frequencies, phases, M, weights, noise_normals, S, pts, C, 0, nullptr, dV);
  dispatch_dp(gp.dp, [&](auto DP) { launch_points<DP>(P.T, E, P.dPts, C, gp.pathD.p, want_grad ? gp.pathD.p + nVal : nullptr, s); });
  gp.hStateOut.reserve(nVal + nGrad);
  gp.pathD.download(gp.hStateOut.p, nVal + nGrad, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  std::memcpy(values, gp.hStateOut.p, sizeof(double) * nVal);
  if (want_grad) std::memcpy(grad, gp.hStateOut.p + nVal, sizeof(double) * nGrad);
}

void paths_minimize(const std::vector<GpDev*>& gps, const double* frequencies, const double* phases, int M, const double* weights,
                    const double* noise_normals, int S, const moe_gd_params_t& gd, const double* domain_bounds, const double* candidates,
                    int C, double* best_points, double* best_values, int* start_index, int* fell_back, double* screened_out,
                    double* trace_out) {
  check_path_members(gps);
  GpDev& gp = *gps[0];
  gp.use_device();
  hipStream_t s = gp.stream;
  const int E = (int)gps.size(), dp = gp.dp, d = gp.d, n = gp.n, rows = E * S, T_steps = gd.max_num_steps, R = gd.max_num_restarts;
  // the call's doubles, results first (one copy back): [out E S (3 + dp) | screened E S C | trace E S R T (d + 6) | V | scratch]
  const size_t tw = (size_t)d + kPmmTraceExtra;
  const size_t nOut = (size_t)rows * (kPmmHead + dp), nScr = (size_t)rows * C, nV = (size_t)rows * n;
  const size_t nTrace = trace_out ? (size_t)rows * R * T_steps * tw : 0;
  gp.pathD.reserve(nOut + nScr + nTrace + 2 * nV);
  gp.pathI.reserve((size_t)rows);
  double* dScr = gp.pathD.p + nOut;
  double* dV = dScr + nScr + nTrace;
  if (nTrace) MOE_HIP_CHECK(hipMemsetAsync(dScr + nScr, 0, sizeof(double) * nTrace, s));
  const size_t nTail = (size_t)T_steps + 2 * (size_t)d;
  const PathStage P = stage_and_set(gps, frequencies, phases, M, weights, noise_normals, S, candidates, C, nTail,
                                    [&](double* h) {
                                      for (int i = 0; i < T_steps; ++i) h[i] = gd.pre_mult * std::pow((double)(i + 1), -gd.gamma);
                                      std::copy(domain_bounds, domain_bounds + 2 * (size_t)d, h + T_steps);
                                    },
                                    dV);
  PmmDescent D;
  D.member_stride = 0;
  D.start_index = gp.pathI.p;
  D.cand = P.dPts;
  D.alpha0 = gp.dStateIn.p + P.tail;
  D.bounds = D.alpha0 + T_steps;
  D.means = dScr;
  D.C = C;
  D.T = T_steps;
  D.R = R;
  D.max_relative_change = gd.max_relative_change;
  D.tolerance = gd.tolerance;
  D.step_tol = gd.tolerance / (double)std::max(T_steps, 1);
  D.out = gp.pathD.p;
  D.trace = nTrace ? dScr + nScr : nullptr;
  dispatch_dp(dp, [&](auto DP) { launch_points<DP>(P.T, E, P.dPts, C, dScr, nullptr, s); });
  launch_pmm_argmin(rows, C, dScr, gp.pathI.p, s);
  dispatch_dp(dp, [&](auto DP) { launch_descent<DP>(P.T, D, rows, s); });
  const size_t nBack = nOut + ((screened_out || trace_out) ? nScr : 0) + nTrace;
  gp.hStateOut.reserve(nBack);
  gp.pathD.download(gp.hStateOut.p, nBack, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  const double* h = gp.hStateOut.p;
  for (int r = 0; r < rows; ++r) {
    const double* o = h + (size_t)r * (kPmmHead + dp);
    if (start_index) start_index[r] = (int)o[0];
    if (fell_back) fell_back[r] = (int)o[1];
    if (best_values) best_values[r] = o[2];
    std::copy(o + kPmmHead, o + kPmmHead + d, best_points + (size_t)r * d);
  }
  if (screened_out) std::memcpy(screened_out, h + nOut, sizeof(double) * nScr);
  if (trace_out) std::memcpy(trace_out, h + nOut + nScr, sizeof(double) * nTrace);
}

}  // namespace moe
