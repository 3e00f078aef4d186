// cornell_moe_amd/csrc/lcb.hip -- marginal posterior mean / standard deviation at many points, and batch lower-confidence-bound
// selection on the device (cpp_wrappers/lower_confidence_bound.py: lower_confidence_bound_optimization, GP-BUCB style).
//
// For C candidates, N training rows and a batch of q points, everything in one upload, on one stream, with one wait:
//   state      E = K(X, c), V = L^-1 E per pass of lcb_pass_size(N, C) candidates   launch_cov_build + launch_tri_gemm_cols   N^2 C flop
//   finish     var = k(c, c) - |V_c|^2, mean = mean0 + E_c . K^-1 (y - mean0)       lcb_finish_kernel (one pass over V and E)
//   pick 0     argmin (mean - std), min (mean + std), first index                   target_partial_kernel + target_final_kernel
//   kept set   {i : mean_i - std_i <= min ucb}, in candidate order                  keep_count / keep_scan / keep_scatter
//   round t    the picked point's 1 + g observation rows join the data:             launch_cov_build, launch_tri_gemm_cols (skinny),
//              its block row of the picks' factor, the Schur block's factor,        launch_gemm_tn, pick_block_kernel,
//              every kept candidate's new coordinates and variance downdate,        cand_round_kernel,
//              argmax of the conditional std, first index                           argmax_partial_kernel + argmax_final_kernel
// The C x C posterior covariance is never formed.  The GP itself is not touched: the picks extend a factor of their own.
//
// Conditioning keeps, for every kept candidate, its coordinates against the picks' rows in the extended factor
// (w_t = L22_t^-1 [k(c, S_t) - V_c^T V_{S_t} - sum_{u<t} w_u(c)^T w_u(S_t)]): kept x (q - 1)(1 + g) doubles.  A round is then one
// pass over V (the data part of the cross-covariance) and one short dot product per candidate; recomputing the cross terms from the
// points against K^-1 k(X, s) would cost a second triangular product per round and still need the earlier picks' corrections.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_cov.hpp"
#include "gp.hpp"

namespace moe {

namespace {

constexpr int kLcbMaxQ = 64;                  // points per batch
constexpr int kLcbChunk = 1024;               // candidates per workgroup of the reductions and the compaction (4 per lane)
constexpr int kLcbMaxBlock = 1 + kMaxDerivs;  // observation rows of one point
constexpr int kLcbTinyCols = 1024;            // N < 128: columns per triangular product, so that tile_gemm's kernel choice
                                              // (64 x 64 blocks >= 48) never depends on the candidate count
constexpr double kPivotMin = 1.0e-16;         // gpp_linear_algebra.cpp:118

// one wavefront per candidate column: |V_c|^2 and E_c . K^-1 (y - mean0), lanes stride over the N rows (fixed order from N alone)
__global__ __launch_bounds__(256) void lcb_finish_kernel(int N, int ncols, int col0, int cov_type, double alpha,
                                                         const double* __restrict__ V, const double* __restrict__ E,
                                                         const double* __restrict__ kinvy, double mean0, double* __restrict__ mean_out,
                                                         double* __restrict__ var_out, double* __restrict__ std_out,
                                                         int* __restrict__ fail) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= ncols) return;
  const double* v = V + (size_t)c * N;
  const double* e = E + (size_t)c * N;
  double ss = 0.0, mu = 0.0;
  for (int r = lane; r < N; r += 64) {
    const double x = v[r];
    ss = fma(x, x, ss);
    mu = fma(e[r], kinvy[r], mu);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ss += __shfl_xor(ss, off, 64);
    mu += __shfl_xor(mu, off, 64);
  }
  if (lane == 0) {
    const double kcc = radial_scalars(cov_type, alpha, 0.0).base;
    const double var = kcc - ss;
    const int i = col0 + c;
    mean_out[i] = mean0 + mu;
    var_out[i] = var;
    std_out[i] = sqrt(fmax(var, 0.0));
    if (!(var > kPivotMin)) atomicMin(fail, i);  // the first failing candidate of the call
  }
}

// the better of two (value, index) pairs: smaller (MAX: larger) value, then smaller index -- the winner of a sequential scan
template <bool MAX>
__device__ __forceinline__ bool better(double v, int i, double best, int bi) {
  return (MAX ? v > best : v < best) || (v == best && i < bi);
}

// workgroup-wide winner; valid in thread 0
template <bool MAX>
__device__ __forceinline__ void block_best(double& best, int& bi) {
  __shared__ double s_val[4];
  __shared__ int s_idx[4];
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(best, off);
    const int oi = __shfl_down(bi, off);
    if (better<MAX>(ov, oi, best, bi)) {
      best = ov;
      bi = oi;
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_val[wave] = best;
    s_idx[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w)
      if (better<MAX>(s_val[w], s_idx[w], best, bi)) {
        best = s_val[w];
        bi = s_idx[w];
      }
  __syncthreads();
}

__device__ __forceinline__ double block_min(double v) {
  __shared__ double s_min[4];
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off));
  if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) v = fmin(fmin(v, s_min[1]), fmin(s_min[2], s_min[3]));
  __syncthreads();
  return v;
}

// workgroup b: candidates [b kLcbChunk, (b + 1) kLcbChunk): argmin of mean - std (first index) and min of mean + std
__global__ __launch_bounds__(256) void target_partial_kernel(int C, const double* __restrict__ mean, const double* __restrict__ sd,
                                                             double* __restrict__ pval, int* __restrict__ pidx,
                                                             double* __restrict__ pucb) {
  const int base = blockIdx.x * kLcbChunk, end = min(C, base + kLcbChunk);
  double best = INFINITY, ucb = INFINITY;
  int bi = INT_MAX;
  for (int i = base + threadIdx.x; i < end; i += 256) {  // i ascends: the first index of this lane's minimum
    const double t = mean[i] - sd[i];
    if (t < best) {
      best = t;
      bi = i;
    }
    ucb = fmin(ucb, mean[i] + sd[i]);
  }
  block_best<false>(best, bi);
  ucb = block_min(ucb);
  if (threadIdx.x == 0) {
    pval[blockIdx.x] = best;
    pidx[blockIdx.x] = bi;
    pucb[blockIdx.x] = ucb;
  }
}

// one workgroup: the winners of the G partial results; index[0], min ucb, and the picked point for the first round
__global__ __launch_bounds__(256) void target_final_kernel(int G, int dp, const double* __restrict__ pval, const int* __restrict__ pidx,
                                                           const double* __restrict__ pucb, const double* __restrict__ P,
                                                           int* __restrict__ index, double* __restrict__ min_ucb,
                                                           double* __restrict__ pick) {
  __shared__ int s_pick;
  double best = INFINITY, ucb = INFINITY;
  int bi = INT_MAX;
  for (int b = threadIdx.x; b < G; b += 256) {
    if (better<false>(pval[b], pidx[b], best, bi)) {
      best = pval[b];
      bi = pidx[b];
    }
    ucb = fmin(ucb, pucb[b]);
  }
  block_best<false>(best, bi);
  ucb = block_min(ucb);
  if (threadIdx.x == 0) {
    if (bi == INT_MAX) bi = 0;  // (no comparable target -- NaN coordinates: the call fails on the candidates' pivot check)
    index[0] = bi;
    *min_ucb = ucb;
    s_pick = bi;
  }
  __syncthreads();
  if ((int)threadIdx.x < dp) pick[threadIdx.x] = P[(size_t)s_pick * dp + threadIdx.x];
}

__device__ __forceinline__ bool is_kept(int i, int C, const double* mean, const double* sd, double min_ucb) {
  return i < C && mean[i] - sd[i] <= min_ucb;
}

__global__ __launch_bounds__(256) void keep_count_kernel(int C, const double* __restrict__ mean, const double* __restrict__ sd,
                                                         const double* __restrict__ min_ucb, int* __restrict__ counts) {
  __shared__ int s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  const double bound = *min_ucb;
  const int base = blockIdx.x * kLcbChunk;
  int mine = 0;
  for (int k = 0; k < kLcbChunk / 256; ++k) mine += is_kept(base + k * 256 + (int)threadIdx.x, C, mean, sd, bound) ? 1 : 0;
  atomicAdd(&s_count, mine);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_count;
}

// exclusive scan of the G workgroup counts (one thread: G = C / 1024), the kept set's size
__global__ void keep_scan_kernel(int G, const int* __restrict__ counts, int* __restrict__ offsets, int* __restrict__ num_kept) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int run = 0;
  for (int b = 0; b < G; ++b) {
    offsets[b] = run;
    run += counts[b];
  }
  *num_kept = run;
}

// order-preserving scatter: kept[pos] = i, and the candidate's variance as the start of its conditional variance
__global__ __launch_bounds__(256) void keep_scatter_kernel(int C, const double* __restrict__ mean, const double* __restrict__ sd,
                                                           const double* __restrict__ var, const double* __restrict__ min_ucb,
                                                           const int* __restrict__ offsets, int* __restrict__ kept,
                                                           double* __restrict__ cvar) {
  __shared__ int s_wave[4];
  const double bound = *min_ucb;
  const int base = blockIdx.x * kLcbChunk, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int run = offsets[blockIdx.x];
  for (int k = 0; k < kLcbChunk / 256; ++k) {
    const int i = base + k * 256 + (int)threadIdx.x;
    const bool keep = is_kept(i, C, mean, sd, bound);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += s_wave[w];
      total += s_wave[w];
    }
    if (keep) {
      const int pos = run + before + __popcll(mask & ((1ull << lane) - 1ull));
      kept[pos] = i;
      cvar[pos] = var[i];
    }
    run += total;
    __syncthreads();
  }
}

// One workgroup: the picked point's block row of the picks' factor Pf (Q x Q lower, ld Q) and the factor of its Schur block.
//   M (ld Q): K(picks 0..r, pick r), (r + 1) b rows x b columns;  Gm: the same entries of VS^T VS (the data's share)
//   rows < tb = r b:   Y = Pf[0:tb, 0:tb]^-1 (M - Gm)            -> Pf[tb + a][i] = Y[i][a]
//   rows >= tb:        S = (M + noise) - Gm - Y^T Y, factored by the reference's outer-product algorithm (pivot rule 1e-16)
// status[0] = r + 1 and status[1] = the failing pivot on failure; every later kernel of the call then returns at once.
__global__ __launch_bounds__(256) void pick_block_kernel(int r, int b, int Q, double* __restrict__ M, const double* __restrict__ Gm,
                                                         const double* __restrict__ noise, double* __restrict__ Pf,
                                                         int* __restrict__ status) {
  if (status[0] != 0) return;
  const int tb = r * b, rows = tb + b, tid = threadIdx.x;
  for (int idx = tid; idx < rows * b; idx += 256) {
    const int row = idx % rows, a = idx / rows;
    double v = M[row + (size_t)a * Q];
    if (row == tb + a) v += noise[a];
    M[row + (size_t)a * Q] = v - Gm[row + (size_t)a * Q];
  }
  __syncthreads();
  for (int i = 0; i < tb; ++i) {
    if (tid < b) M[i + (size_t)tid * Q] = M[i + (size_t)tid * Q] / Pf[i + (size_t)i * Q];
    __syncthreads();
    const int below = rows - i - 1;
    for (int idx = tid; idx < below * b; idx += 256) {
      const int row = i + 1 + idx % below, a = idx / below;
      const double l = (row < tb) ? Pf[row + (size_t)i * Q] : M[i + (size_t)(row - tb) * Q];
      M[row + (size_t)a * Q] = M[row + (size_t)a * Q] - l * M[i + (size_t)a * Q];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < tb * b; idx += 256) {
    const int i = idx % tb, a = idx / tb;
    Pf[(tb + a) + (size_t)i * Q] = M[i + (size_t)a * Q];
  }
  if (tid == 0) {
    double* S = M + tb;  // S[i + j Q], lower triangle
    for (int k = 0; k < b; ++k) {
      const double piv = S[k + (size_t)k * Q];
      if (!(piv > kPivotMin)) {
        status[0] = r + 1;
        status[1] = k;
        return;
      }
      const double lkk = sqrt(piv);
      S[k + (size_t)k * Q] = lkk;
      for (int i = k + 1; i < b; ++i) S[i + (size_t)k * Q] = S[i + (size_t)k * Q] / lkk;
      for (int j = k + 1; j < b; ++j)
        for (int i = j; i < b; ++i) S[i + (size_t)j * Q] = S[i + (size_t)j * Q] - S[i + (size_t)k * Q] * S[j + (size_t)k * Q];
    }
    for (int k = 0; k < b; ++k)
      for (int i = k; i < b; ++i) Pf[(tb + i) + (size_t)(tb + k) * Q] = S[i + (size_t)k * Q];
  }
}

// One wavefront per kept candidate: its cross-covariance with the picked block given the data and the earlier picks, its new
// coordinates w = L22^-1 cross, the variance downdate and the conditional standard deviation.
__global__ __launch_bounds__(256) void cand_round_kernel(int N, int r, int b, int Q, const CovParams cp, const DerivList dl,
                                                         const double* __restrict__ P, const double* __restrict__ pick,
                                                         const double* __restrict__ V, const double* __restrict__ VS,
                                                         const double* __restrict__ Pf, const int* __restrict__ kept,
                                                         const int* __restrict__ num_kept, double* __restrict__ W,
                                                         double* __restrict__ cvar, double* __restrict__ cstd,
                                                         const int* __restrict__ status) {
  if (status[0] != 0) return;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= *num_kept) return;
  const int col = kept[j], tb = r * b;
  const double* v = V + (size_t)col * N;
  double* w = W + (size_t)j * Q;
  double acc[kLcbMaxBlock];
#pragma unroll
  for (int a = 0; a < kLcbMaxBlock; ++a) acc[a] = 0.0;
  for (int row = lane; row < N; row += 64) {
    const double x = v[row];
#pragma unroll
    for (int a = 0; a < kLcbMaxBlock; ++a)
      if (a < b) acc[a] = fma(x, VS[row + (size_t)a * N], acc[a]);
  }
  for (int i = lane; i < tb; i += 64) {
    const double x = w[i];
#pragma unroll
    for (int a = 0; a < kLcbMaxBlock; ++a)
      if (a < b) acc[a] = fma(x, Pf[(tb + a) + (size_t)i * Q], acc[a]);
  }
#pragma unroll
  for (int a = 0; a < kLcbMaxBlock; ++a)
    if (a < b)
      for (int off = 32; off > 0; off >>= 1) acc[a] += __shfl_xor(acc[a], off, 64);
  if (lane != 0) return;
  DerivList none;
  none.g = 0;
  const PointDiff df{P + (size_t)col * cp.dp, pick};
  const Radial rd = pair_radial(cp, df, cp.dp);
  double var = cvar[j];
  double wn[kLcbMaxBlock];
#pragma unroll
  for (int a = 0; a < kLcbMaxBlock; ++a) {
    if (a < b) {
      double x = cov_entry_g(cp, rd, df, 0, a, none, dl) - acc[a];
#pragma unroll
      for (int a2 = 0; a2 < kLcbMaxBlock; ++a2)
        if (a2 < a) x -= Pf[(tb + a) + (size_t)(tb + a2) * Q] * wn[a2];
      x = x / Pf[(tb + a) + (size_t)(tb + a) * Q];
      wn[a] = x;
      w[tb + a] = x;
      var -= x * x;
    }
  }
  cvar[j] = var;
  cstd[j] = sqrt(fmax(var, 0.0));
}

// workgroup b: kept positions [b kLcbChunk, (b + 1) kLcbChunk): argmax of the conditional std, first position
__global__ __launch_bounds__(256) void argmax_partial_kernel(const int* __restrict__ num_kept, const double* __restrict__ cstd,
                                                             double* __restrict__ pval, int* __restrict__ pidx,
                                                             const int* __restrict__ status) {
  if (status[0] != 0) return;
  const int n = *num_kept;
  const int base = blockIdx.x * kLcbChunk, end = min(n, base + kLcbChunk);
  double best = -INFINITY;
  int bi = INT_MAX;
  for (int j = base + threadIdx.x; j < end; j += 256)
    if (cstd[j] > best) {
      best = cstd[j];
      bi = j;
    }
  block_best<true>(best, bi);
  if (threadIdx.x == 0) {
    pval[blockIdx.x] = best;
    pidx[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(256) void argmax_final_kernel(int G, int dp, int t, const double* __restrict__ pval,
                                                           const int* __restrict__ pidx, const int* __restrict__ kept,
                                                           const double* __restrict__ P, int* __restrict__ index,
                                                           double* __restrict__ pick, const int* __restrict__ status) {
  __shared__ int s_pick;
  if (status[0] != 0) return;
  double best = -INFINITY;
  int bi = INT_MAX;
  for (int b = threadIdx.x; b < G; b += 256)
    if (better<true>(pval[b], pidx[b], best, bi)) {
      best = pval[b];
      bi = pidx[b];
    }
  block_best<true>(best, bi);
  if (threadIdx.x == 0) {
    s_pick = (bi == INT_MAX) ? index[0] : kept[bi];  // (an empty kept set -- NaN targets -- re-picks index[0]; the call fails anyway)
    index[t] = s_pick;
  }
  __syncthreads();
  if ((int)threadIdx.x < dp) pick[(size_t)t * dp + threadIdx.x] = P[(size_t)s_pick * dp + threadIdx.x];
}

__global__ void lcb_init_kernel(int* __restrict__ ints, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) ints[i] = (i == 0) ? INT_MAX : 0;  // [first failing candidate | status (2) | kept | index ...]
}

// the call's integers behind one another as doubles, in front of mean and std: one copy back
__global__ void lcb_pack_kernel(const int* __restrict__ ints, int n, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (double)ints[i];
}

// the padded candidates, one copy down; returns their device address
const double* upload_candidates(GpDev& gp, const double* pts, int C) {
  const size_t nP = (size_t)C * gp.dp;
  gp.hStateIn.reserve(nP);
  for (size_t i = 0; i < (size_t)C; ++i)
    for (int k = 0; k < gp.dp; ++k) gp.hStateIn.p[i * gp.dp + k] = (k < gp.d) ? pts[i * gp.d + k] : 0.0;
  gp.dStateIn.upload(gp.hStateIn.p, nP, gp.stream, true);
  return gp.dStateIn.p;
}

// Phase one for all C candidates, pass by pass: mean, var, std [C] and the first failing candidate.  keep_v: V = L^-1 K* of every
// candidate stays in gp.dVE (N x C); otherwise a pass's columns only.
void enqueue_mean_std(GpDev& gp, const double* dP, int C, bool keep_v, double* dMean, double* dVar, double* dStd, int* dFail) {
  hipStream_t s = gp.stream;
  const int N = gp.N, per_pass = lcb_pass_size(N, C), widest = std::min(per_pass, C);
  const DerivList none = no_derivs();
  const bool split = N >= 128 && C > 16;
  gp.dE.reserve((size_t)N * widest);
  gp.dVE.reserve((size_t)N * (keep_v ? C : widest));
  if (split) gp.dEK.reserve(tri_cols_work_doubles(N, widest));
  for (int c0 = 0; c0 < C; c0 += per_pass) {
    const int nc = std::min(per_pass, C - c0);
    double* Vp = gp.dVE.p + (keep_v ? (size_t)c0 * N : 0);
    launch_cov_build(gp.cp, gp.dX.p, gp.n, gp.derivs, dP + (size_t)c0 * gp.dp, nc, none, nullptr, gp.dE.p, N, 0, s);
    if (N < 128) {
      for (int k0 = 0; k0 < nc; k0 += kLcbTinyCols) {
        const int nk = std::min(kLcbTinyCols, nc - k0);
        launch_tri_gemm_cols('N', N, nk, nk, gp.dLinv.p, gp.ldL, gp.dE.p + (size_t)k0 * N, N, Vp + (size_t)k0 * N, N, nullptr, s);
      }
    } else {
      // (the kernel family from C, not from the pass's own width: a short last pass takes the kernels of the others)
      launch_tri_gemm_cols('N', N, nc, split ? 17 : C, gp.dLinv.p, gp.ldL, gp.dE.p, N, Vp, N, gp.dEK.p, s);
    }
    MOE_LAUNCH_NOW(lcb_finish_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, N, nc, c0, gp.cp.type, gp.cp.alpha,
                   (const double*)Vp, (const double*)gp.dE.p, (const double*)gp.dKinvY.p, gp.mean, dMean, dVar, dStd, dFail);
    MOE_HIP_CHECK(hipGetLastError());
  }
}

[[noreturn]] void throw_candidate_singular(int fail) {
  throw Error(MOE_ERR_SINGULAR,
              "GP-Variance matrix singular. Check for duplicate points_to_sample or points_to_sample "
              "duplicating points_sampled with 0 noise.",
              1, fail);
}

}  // namespace

// Candidates per pass, from N alone (C is part of the signature because the kernel family depends on it, not the width): the pass's
// K* and V columns stay within 2^26 doubles each, and within the 65 535 grid rows of the split-K sum.
int lcb_pass_size(int N, int /*C*/) {
  const long cap = ((long)1 << 26) / std::max(N, 1);
  return (int)std::max<long>(kLcbTinyCols, std::min<long>(16384, cap / kLcbTinyCols * kLcbTinyCols));
}

void mean_std_on_device(GpDev& gp, const double* pts, int C, double* mean_out, double* std_out) {
  if (C <= 0) throw Error(MOE_ERR_BOUNDS, "the number of candidates must be positive", C, 1, 1e9);
  if (pts == nullptr || mean_out == nullptr || std_out == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL argument");
  gp.use_device();
  hipStream_t s = gp.stream;
  const double* dP = upload_candidates(gp, pts, C);
  const size_t nC = (size_t)C;
  gp.lcbD.reserve(1 + 3 * nC);  // [fail | mean | std | var]
  gp.lcbI.reserve(1);
  double* dOut = gp.lcbD.p;
  MOE_LAUNCH_NOW(lcb_init_kernel, dim3(1), dim3(256), 0, s, gp.lcbI.p, 1);
  enqueue_mean_std(gp, dP, C, false, dOut + 1, dOut + 1 + 2 * nC, dOut + 1 + nC, gp.lcbI.p);
  MOE_LAUNCH_NOW(lcb_pack_kernel, dim3(1), dim3(256), 0, s, (const int*)gp.lcbI.p, 1, dOut);
  MOE_HIP_CHECK(hipGetLastError());
  gp.hStateOut.reserve(1 + 2 * nC);
  gp.lcbD.download(gp.hStateOut.p, 1 + 2 * nC, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  const double fail = gp.hStateOut.p[0];
  if (fail < (double)C) throw_candidate_singular((int)fail);
  std::memcpy(mean_out, gp.hStateOut.p + 1, sizeof(double) * nC);
  std::memcpy(std_out, gp.hStateOut.p + 1 + nC, sizeof(double) * nC);
}

void lcb_select_on_device(GpDev& gp, const double* pts, int C, int q, int* index_out, double* points_out, double* mean_out,
                          double* std_out, int* num_kept_out) {
  if (C < 1) throw Error(MOE_ERR_BOUNDS, "the number of candidates must be positive", C, 1, 1e9);
  if (q < 1 || q > kLcbMaxQ) throw Error(MOE_ERR_BOUNDS, "num_to_sample out of range", q, 1, kLcbMaxQ);
  if (pts == nullptr || index_out == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL argument");
  gp.use_device();
  hipStream_t s = gp.stream;
  const int N = gp.N, dp = gp.dp, b = 1 + gp.g, Q = std::max(1, (q - 1) * b);
  const int G = (C + kLcbChunk - 1) / kLcbChunk;
  const size_t nC = (size_t)C;
  const bool want_surface = mean_out != nullptr || std_out != nullptr;
  const double* dP = upload_candidates(gp, pts, C);

  // integers: [fail | status (2) | kept | index (q)] (packed for the copy back) | pidx G | counts G | offsets G | kept set C
  const int nHead = 4 + q;
  gp.lcbI.reserve((size_t)nHead + 3 * (size_t)G + nC);
  int* iFail = gp.lcbI.p;
  int* iStatus = iFail + 1;
  int* iKept = iFail + 3;
  int* iIndex = iFail + 4;
  int* iPidx = iFail + nHead;
  int* iCounts = iPidx + G;
  int* iOffsets = iCounts + G;
  int* iKeptSet = iOffsets + G;
  // doubles: [head | mean C | std C] (the copy back) | var C | cvar C | cstd C | pval G | pucb G | min ucb | picks q dp | M, Gm Q b |
  //          Pf Q Q | K(X, pick) N b | VS N Q | W C Q
  const size_t nW = (q > 1) ? nC * Q : 0, nVS = (q > 1) ? (size_t)N * Q : 0, nES = (q > 1) ? (size_t)N * b : 0;
  gp.lcbD.reserve((size_t)nHead + 5 * nC + 2 * (size_t)G + 1 + (size_t)q * dp + 2 * (size_t)Q * b + (size_t)Q * Q + nES + nVS + nW);
  double* dHead = gp.lcbD.p;
  double* dMean = dHead + nHead;
  double* dStd = dMean + nC;
  double* dVar = dStd + nC;
  double* dCvar = dVar + nC;
  double* dCstd = dCvar + nC;
  double* dPval = dCstd + nC;
  double* dPucb = dPval + G;
  double* dMinUcb = dPucb + G;
  double* dPick = dMinUcb + 1;
  double* dM = dPick + (size_t)q * dp;
  double* dGm = dM + (size_t)Q * b;
  double* dPf = dGm + (size_t)Q * b;
  double* dES = dPf + (size_t)Q * Q;
  double* dVS = dES + nES;
  double* dW = dVS + nVS;

  if (q > 1) gp.dEK.reserve(tri_cols_work_doubles(N, b));  // (the picked blocks' triangular products; phase one may ask for more)
  MOE_LAUNCH_NOW(lcb_init_kernel, dim3((unsigned)((nHead + 255) / 256)), dim3(256), 0, s, iFail, nHead);
  enqueue_mean_std(gp, dP, C, q > 1, dMean, dVar, dStd, iFail);
  MOE_LAUNCH_NOW(target_partial_kernel, dim3((unsigned)G), dim3(256), 0, s, C, (const double*)dMean, (const double*)dStd, dPval,
                 iPidx, dPucb);
  MOE_LAUNCH_NOW(target_final_kernel, dim3(1), dim3(256), 0, s, G, dp, (const double*)dPval, (const int*)iPidx,
                 (const double*)dPucb, dP, iIndex, dMinUcb, dPick);
  MOE_LAUNCH_NOW(keep_count_kernel, dim3((unsigned)G), dim3(256), 0, s, C, (const double*)dMean, (const double*)dStd,
                 (const double*)dMinUcb, iCounts);
  MOE_LAUNCH_NOW(keep_scan_kernel, dim3(1), dim3(64), 0, s, G, (const int*)iCounts, iOffsets, iKept);
  MOE_LAUNCH_NOW(keep_scatter_kernel, dim3((unsigned)G), dim3(256), 0, s, C, (const double*)dMean, (const double*)dStd,
                 (const double*)dVar, (const double*)dMinUcb, (const int*)iOffsets, iKeptSet, dCvar);
  MOE_HIP_CHECK(hipGetLastError());
  for (int t = 1; t < q; ++t) {
    const int r = t - 1;
    const double* pick = dPick + (size_t)r * dp;
    double* VSr = dVS + (size_t)r * b * N;
    launch_cov_build(gp.cp, gp.dX.p, gp.n, gp.derivs, pick, 1, gp.derivs, nullptr, dES, N, 0, s);
    launch_tri_gemm_cols('N', N, b, b, gp.dLinv.p, gp.ldL, dES, N, VSr, N, gp.dEK.p, s);
    launch_cov_build(gp.cp, dPick, r + 1, gp.derivs, pick, 1, gp.derivs, nullptr, dM, Q, 0, s);
    launch_gemm_tn((r + 1) * b, b, N, dVS, N, VSr, N, dGm, Q, s);
    MOE_LAUNCH_NOW(pick_block_kernel, dim3(1), dim3(256), 0, s, r, b, Q, dM, (const double*)dGm, (const double*)gp.dNoise.p, dPf,
                   iStatus);
    MOE_LAUNCH_NOW(cand_round_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, N, r, b, Q, gp.cp, gp.derivs, dP, pick,
                   (const double*)gp.dVE.p, (const double*)VSr, (const double*)dPf, (const int*)iKeptSet, (const int*)iKept, dW,
                   dCvar, dCstd, (const int*)iStatus);
    MOE_LAUNCH_NOW(argmax_partial_kernel, dim3((unsigned)G), dim3(256), 0, s, (const int*)iKept, (const double*)dCstd, dPval, iPidx,
                   (const int*)iStatus);
    MOE_LAUNCH_NOW(argmax_final_kernel, dim3(1), dim3(256), 0, s, G, dp, t, (const double*)dPval, (const int*)iPidx,
                   (const int*)iKeptSet, dP, iIndex, dPick, (const int*)iStatus);
    MOE_HIP_CHECK(hipGetLastError());
  }
  MOE_LAUNCH_NOW(lcb_pack_kernel, dim3((unsigned)((nHead + 255) / 256)), dim3(256), 0, s, (const int*)iFail, nHead, dHead);
  MOE_HIP_CHECK(hipGetLastError());
  const size_t nBack = (size_t)nHead + (want_surface ? 2 * nC : 0);
  gp.hStateOut.reserve(nBack);
  gp.lcbD.download(gp.hStateOut.p, nBack, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  const double* h = gp.hStateOut.p;
  if (h[0] < (double)C) throw_candidate_singular((int)h[0]);
  if (h[1] != 0.0) {
    const int t = (int)h[1], k = (int)h[2];
    throw Error(MOE_ERR_SINGULAR,
                "Covariance matrix singular. Check for duplicate points / points too close together or overly large/small "
                "hyperparameter values.",
                N + t * b, N + (t - 1) * b + k + 1);
  }
  if (num_kept_out) *num_kept_out = (int)h[3];
  for (int t = 0; t < q; ++t) {
    index_out[t] = (int)h[4 + t];
    if (points_out) std::copy(pts + (size_t)index_out[t] * gp.d, pts + (size_t)(index_out[t] + 1) * gp.d, points_out + (size_t)t * gp.d);
  }
  if (mean_out) std::memcpy(mean_out, h + nHead, sizeof(double) * nC);
  if (std_out) std::memcpy(std_out, h + nHead + nC, sizeof(double) * nC);
}

}  // namespace moe
