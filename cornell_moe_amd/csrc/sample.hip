// cornell_moe_amd/csrc/sample.hip -- joint posterior sampling on the device: SamplePointsFromGP / SampleGlobalOptimaFromGP
// (gpp_math.cpp:1800-1870) for a batch of candidate sets.
//
// For E sets of C candidates and D normal vectors per set, everything in one upload, on one stream, with one wait:
//   state       V = L^-1 K*, gram = V^T V, ek = K*^T K^-1 (y - mean)   enqueue_sample_state_batch (gp.hip)   N C^2 + N^2 C flop per set
//   covariance  Var = K(U, U) - gram                                   launch_cov_build + sub_kernel
//   factor      one-level blocked Cholesky of every set                launch_cholesky_batch (grid.z = set)   C^3 / 3
//   draws       Y = L Z                                                TRMM on the matrix pipe (D >= kTrmmMinDraws) or
//                                                                      trmv_draws_kernel                      C^2 D
//   finish      y = mu + L z, argmin by the reference's rule           draw_finish_kernel
// Every kernel is chosen from (N, C, D) alone and works on one set at a time, so a set's results do not depend on the batch.
//
// A set whose factorisation fails (pivot <= 1e-16, gpp_linear_algebra.cpp:118) is resumed after the wait from the first column of
// its failing block by the reference's unblocked outer-product algorithm, one column per launch pair: stop_at_failure keeps
// ComputeCholeskyFactorL's early stop (the columns before the failing pivot factored, the trailing Schur complement left in the
// lower triangle -- the reference then uses that matrix as L), otherwise a failing column is zeroed and the factorisation goes on.
// Its draws are then made again.  Those columns cost a launch pair each: this path is for the rare singular set.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gp.hpp"

namespace moe {

namespace {

constexpr int kTrmmMinDraws = 8;       // from this many draws per set the draws are a TRMM on the FP64 matrix pipe (tile_gemm)
constexpr int kMaxSetsPerPass = 2048;  // grid.z of the batched kernels (sets x K slices of the Gram kernel) stays below 65 536
constexpr int kMaxGridY = 65535;

// Sets per pass, from (N, C) alone -- never from E, so that a set's results do not depend on its batch.  Where V = L^-1 K* takes the
// split-K kernels (launch_tri_gemm_cols: N >= 128, more than 16 columns per problem) the sum over the K slices runs one grid row
// per candidate of the whole pass: grid.y = sets x C must stay within the 65 536 the device advertises.
int sets_per_pass(int N, int C) {
  if (N >= 128 && C > 16) return std::max(1, std::min(kMaxSetsPerPass, kMaxGridY / C));
  return kMaxSetsPerPass;
}

__global__ __launch_bounds__(256) void sub_kernel(double* __restrict__ var, const double* __restrict__ gram, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) var[i] = var[i] - gram[i];
}

// Y[e][d][i] = sum_{j <= i} L_e[i][j] Z[e][d][j] for D < kTrmmMinDraws: lanes walk rows (coalesced column reads of L), j ascends.
__global__ __launch_bounds__(256) void trmv_draws_kernel(int C, int D, const double* __restrict__ L, const double* __restrict__ Z,
                                                         double* __restrict__ Y) {
  const int e = blockIdx.y;
  const int i0 = blockIdx.x * 256, i = i0 + threadIdx.x;
  const double* Le = L + (size_t)e * C * C;
  const double* Ze = Z + (size_t)e * D * C;
  double acc[kTrmmMinDraws];
#pragma unroll
  for (int d = 0; d < kTrmmMinDraws; ++d) acc[d] = 0.0;
  const int jend = min(C, i0 + 256);
  for (int j = 0; j < jend; ++j) {
    const double l = (i < C && j <= i) ? Le[(size_t)i + (size_t)j * C] : 0.0;
#pragma unroll
    for (int d = 0; d < kTrmmMinDraws; ++d)
      if (d < D) acc[d] = fma(l, Ze[(size_t)d * C + j], acc[d]);
  }
  if (i < C) {
#pragma unroll
    for (int d = 0; d < kTrmmMinDraws; ++d)
      if (d < D) Y[((size_t)e * D + d) * C + i] = acc[d];
  }
}

// y = mu + (L z) in place for draw d of set e (one workgroup each), then the index of its minimum by SamplePointsFromGP's rule
// (gpp_math.cpp:1839-1847): best = y[0], index -1, replaced only on a strictly smaller value -- i.e. the first index of the
// minimum, or -1 when y[0] is a minimum.  argmin is written as a double behind the draws (one download).
__global__ __launch_bounds__(256) void draw_finish_kernel(int C, int D, double mean, const double* __restrict__ ek,
                                                          double* __restrict__ Y, double* __restrict__ argmin) {
  __shared__ double s_val[4];
  __shared__ int s_idx[4];
  const int d = blockIdx.x, e = blockIdx.y;
  double* y = Y + ((size_t)e * D + d) * C;
  const double* mu = ek + (size_t)e * C;
  double best = INFINITY;
  int bi = C;  // (no candidate yet)
  double y0 = 0.0;
  for (int i = threadIdx.x; i < C; i += 256) {
    const double v = (mean + mu[i]) + y[i];
    y[i] = v;
    if (i == 0) y0 = v;
    if (v < best) {  // i ascends: the first index of this lane's minimum
      best = v;
      bi = i;
    }
  }
  // smallest value, then smallest index: the winner of the sequential scan
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(best, off);
    const int oi = __shfl_down(bi, off);
    if (ov < best || (ov == best && oi < bi)) {
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
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (s_val[w] < best || (s_val[w] == best && s_idx[w] < bi)) {
        best = s_val[w];
        bi = s_idx[w];
      }
    argmin[(size_t)e * D + d] = (best < y0) ? (double)bi : -1.0;  // (lane 0 owns candidate 0)
  }
}

// Column k of ComputeCholeskyFactorL's outer-product algorithm on the lower triangle of A (C x C, ld C), trailing update:
// A_ij -= L_ik L_jk for k < j <= i, with L_ik = A_ik / sqrt(A_kk) formed here exactly as the stored value will be.  Nothing to do
// for a failing pivot (pivot_column_kernel leaves or zeroes its column) or after an early stop.
__global__ __launch_bounds__(256) void trailing_update_kernel(double* __restrict__ A, int C, int k, const int* __restrict__ status,
                                                              int stop_at_failure) {
  if (stop_at_failure && *status != 0) return;
  const double piv = A[(size_t)k * C + k];
  if (!(piv > 1.0e-16)) return;
  const double lkk = sqrt(piv);
  for (int j = k + 1 + blockIdx.y; j < C; j += gridDim.y) {
    const int i = j + blockIdx.x * 256 + threadIdx.x;
    if (i >= C) continue;
    const double lik = A[(size_t)k * C + i] / lkk, ljk = A[(size_t)k * C + j] / lkk;
    A[(size_t)j * C + i] = A[(size_t)j * C + i] - lik * ljk;
  }
}

// Column k itself (one workgroup, after the trailing update has read it): L_kk = sqrt(A_kk), L_ik = A_ik / L_kk.  A failing pivot
// records status = k + 1 (the first one) and either stops everything after it or zeroes the column.
__global__ __launch_bounds__(256) void pivot_column_kernel(double* __restrict__ A, int C, int k, int* __restrict__ status,
                                                           int stop_at_failure) {
  __shared__ int s_status;
  if (threadIdx.x == 0) s_status = *status;
  const double piv = A[(size_t)k * C + k];
  __syncthreads();  // (every lane has read the pivot before lane 0 overwrites it)
  if (stop_at_failure && s_status != 0) return;
  double* col = A + (size_t)k * C;
  if (piv > 1.0e-16) {
    const double lkk = sqrt(piv);
    for (int i = k + threadIdx.x; i < C; i += 256) col[i] = (i == k) ? lkk : col[i] / lkk;
  } else {
    if (threadIdx.x == 0 && s_status == 0) *status = k + 1;
    if (!stop_at_failure)
      for (int i = k + threadIdx.x; i < C; i += 256) col[i] = 0.0;
  }
}

// draws and their finish for the sets [e0, e0 + ne)
void enqueue_draws(double mean, int C, int D, int e0, int ne, const double* dL, const double* dZ, const double* dEk, double* dY,
                   double* dArg, hipStream_t s) {
  const size_t CC = (size_t)C * C, DC = (size_t)D * C;
  if (D >= kTrmmMinDraws) {
    for (int e = e0; e < e0 + ne; ++e) launch_tri_gemm('N', C, D, dL + e * CC, C, dZ + e * DC, C, dY + e * DC, C, s);
  } else {
    MOE_LAUNCH(trmv_draws_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)ne), dim3(256), 0, s, C, D, dL + e0 * CC,
               dZ + e0 * DC, dY + e0 * DC);
  }
  MOE_LAUNCH(draw_finish_kernel, dim3((unsigned)D, (unsigned)ne), dim3(256), 0, s, C, D, mean, dEk + (size_t)e0 * C,
             dY + e0 * DC, dArg + (size_t)e0 * D);
  MOE_HIP_CHECK(hipGetLastError());
}

// one pass over E <= sets_per_pass(N, C) sets
void sample_pass(GpDev& gp, const double* pts, int C, int E, const double* normals, int D, bool stop_at_failure, double* values,
                 int* argmin, int* failed) {
  hipStream_t s = gp.stream;
  const size_t CC = (size_t)C * C, DC = (size_t)D * C, nY = (size_t)E * DC, nA = (size_t)E * D;
  StateAppendix apx;  // the normals ride along in the state set-up's single host -> device copy
  apx.doubles = nY;
  apx.fill = [&](double* dst) { std::memcpy(dst, normals, sizeof(double) * nY); };
  enqueue_sample_state_batch(gp, pts, C, E, &apx);
  const double* dZ = gp.dAppendix;
  const double* dEk = gp.dGram.p + (size_t)E * CC;
  gp.sMat.reserve((size_t)E * CC);
  gp.sOut.reserve(nY + nA);
  gp.sInfo.reserve((size_t)2 * E);
  double* dV = gp.sMat.p;
  double* dY = gp.sOut.p;
  double* dArg = dY + nY;
  int* dInfo = gp.sInfo.p;
  int* dStatus = dInfo + E;
  DerivList none;
  none.g = 0;
  for (int i = 0; i < kMaxDerivs; ++i) none.idx[i] = 0;
  for (int e = 0; e < E; ++e) {
    const double* Ue = gp.dUnion + (size_t)e * C * gp.dp;
    launch_cov_build(gp.cp, Ue, C, none, Ue, C, none, nullptr, dV + e * CC, C, 0, s);
  }
  const double* dGram = gp.dGram.p;
  MOE_LAUNCH(sub_kernel, dim3((unsigned)((E * CC + 255) / 256)), dim3(256), 0, s, dV, dGram, (long)(E * CC));
  MOE_HIP_CHECK(hipGetLastError());
  // (the Grams are spent: their room takes the inverses of the diagonal blocks, which the factorisation writes in C x C layout)
  launch_cholesky_batch(C, dV, C, (long)CC, gp.dGram.p, C, (long)CC, dInfo, E, s, nullptr, /*one_level=*/true);
  enqueue_draws(gp.mean, C, D, 0, E, dV, dZ, dEk, dY, dArg, s);
  gp.hStateOut.reserve(nY + nA);
  std::vector<int> info(E, 0);
  gp.sOut.download(gp.hStateOut.p, nY + nA, s);
  MOE_HIP_CHECK(hipMemcpyAsync(info.data(), dInfo, sizeof(int) * E, hipMemcpyDeviceToHost, s));
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  bool any_failed = false;
  for (int e = 0; e < E; ++e) any_failed = any_failed || info[e] != 0;
  if (any_failed) {
    MOE_HIP_CHECK(hipMemsetAsync(dStatus, 0, sizeof(int) * E, s));
    for (int e = 0; e < E; ++e) {
      if (info[e] == 0) continue;
      double* Ae = dV + e * CC;
      const int k0 = (info[e] - 1) / kCholBatchBlock * kCholBatchBlock;  // the failing block's first column
      for (int k = k0; k < C; ++k) {
        if (k + 1 < C) {
          const unsigned rows = (unsigned)((C - k - 1 + 255) / 256), cols = (unsigned)std::min(C - k - 1, 65535);
          MOE_LAUNCH(trailing_update_kernel, dim3(rows, cols), dim3(256), 0, s, Ae, C, k, (const int*)(dStatus + e),
                     (int)stop_at_failure);
        }
        MOE_LAUNCH(pivot_column_kernel, dim3(1), dim3(256), 0, s, Ae, C, k, dStatus + e, (int)stop_at_failure);
      }
      MOE_HIP_CHECK(hipGetLastError());
      enqueue_draws(gp.mean, C, D, e, 1, dV, dZ, dEk, dY, dArg, s);
    }
    gp.sOut.download(gp.hStateOut.p, nY + nA, s);
    MOE_HIP_CHECK(hipMemcpyAsync(info.data(), dStatus, sizeof(int) * E, hipMemcpyDeviceToHost, s));  // (0 for the others)
    MOE_HIP_CHECK(hipStreamSynchronize(s));
  }
  std::memcpy(values, gp.hStateOut.p, sizeof(double) * nY);
  for (size_t a = 0; a < nA; ++a) argmin[a] = (int)gp.hStateOut.p[nY + a];
  for (int e = 0; e < E; ++e) failed[e] = info[e];
}

}  // namespace

void sample_points_on_device(GpDev& gp, const double* pts, int C, int E, const double* normals, int D, bool stop_at_failure,
                             double* values, int* argmin, int* failed) {
  if (C <= 0) throw Error(MOE_ERR_BOUNDS, "num_pts must be positive", C, 1, 1e9);
  if (E <= 0) throw Error(MOE_ERR_BOUNDS, "the number of candidate sets must be positive", E, 1, 1e9);
  if (D <= 0) throw Error(MOE_ERR_BOUNDS, "num_draws must be positive", D, 1, 1e9);
  if (pts == nullptr || normals == nullptr || values == nullptr || argmin == nullptr || failed == nullptr)
    throw Error(MOE_ERR_RUNTIME, "NULL argument");
  gp.use_device();
  const int per_pass = sets_per_pass(gp.N, C);
  for (int e0 = 0; e0 < E; e0 += per_pass) {
    const int ne = std::min(per_pass, E - e0);
    const size_t DC = (size_t)D * C;
    sample_pass(gp, pts + (size_t)e0 * C * gp.d, C, ne, normals + e0 * DC, D, stop_at_failure, values + e0 * DC,
                argmin + (size_t)e0 * D, failed + e0);
  }
}

}  // namespace moe
