// cornell_moe_amd/csrc/loo.hip -- the leave-one-out (LOO) cross-validation objective: its value for batches of hyper-parameter
// sets, its hyper-parameter gradient, and the per-row LOO predictive mean and variance (Rasmussen & Williams 5.4.2).
//
// With K = K(X, X) + diag(noise), alpha = K^-1 yc and kappa_i = (K^-1)_ii, leaving out row i alone predicts
//   mu_i = yc_i - alpha_i / kappa_i,   var_i = 1 / kappa_i,
//   L_LOO = sum_i [ 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi ].
// Gradient, ONE N^3 product for all hyper-parameters: with c_i = alpha_i / kappa_i, e_i = 1/2 (1 + alpha_i^2 / kappa_i) / kappa_i,
// u = K^-1 c and M = K^-1 diag(e) K^-1,
//   d L_LOO / d theta = sum_ab (u_a alpha_b - M_ab) (dK / d theta)_ab
// -- the contraction of the marginal likelihood's gradient (gp.hip: ll_grad_kernel) with another weight.
//
//   value      X = L^-1 from the batched factor (loo_trinv_kernel), kappa = column norms of X, alpha = X^T (L^-1 yc)
//              (loo_terms_kernel), the two sums per set (loo_terms_sum_kernel)                                  N^3 / 3 flop per set
//   predict    kappa from the GP's explicit inverse factor (loo_terms_kernel), loo_point_kernel                 N^2 / 2
//   gradient   K^-1 = X^T X (launch_tri_gram_strided, stride 1), u = K^-1 c (launch_gemm_tn), B = diag(sqrt e) K^-1 on the
//              function-value columns + diag M (loo_scale_kernel), M = B^T B (launch_gemm_tn: n x n over K = N),
//              loo_grad_kernel<DP> + loo_grad_finish_kernel                                        N^3 / 3 + 2 n^2 N + O(n^2 d)
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_cov.hpp"
#include "gp.hpp"

namespace moe {

namespace {

constexpr int kLooBlock = 64;  // block rows / columns of the batched triangular inversion
constexpr int kLooTK = 16;     // its K step

// X = L^-1 for `batch` lower-triangular factors (the leading N x N block of matrix b at L + b a_stride; its strict upper triangle is
// never read).  One workgroup per (64-column block J, matrix): block row by block row, I = J, J + 1, ...
//     X_JJ = L_JJ^-1,   X_IJ = -L_II^-1 sum_{J <= K < I} L_IK X_KJ.
// Lane = row of the block, wavefront w owns columns 16 w .. 16 w + 15 of block J: the 64 x 64 accumulator lives in registers (16 per
// lane), and the substitution with L_II is a register recurrence whose row k travels by a lane broadcast -- no pass over LDS.
// The blocks X_KJ of earlier rows are read back from global memory by the workgroup that wrote them.  A matrix whose factorisation
// failed (info[b] != 0) is skipped: its value is -infinity whatever is in X.
__global__ __launch_bounds__(256) void loo_trinv_kernel(const double* __restrict__ L, long lda, long a_stride, int N, double* X,
                                                        long ldx, long x_stride, const int* __restrict__ info) {
  __shared__ double As[kLooTK][kLooBlock];
  __shared__ double Bs[kLooTK][kLooBlock + 1];
  __shared__ double Ld[kLooBlock][kLooBlock];  // L_II, column-major: Ld[k][r] = L(I0 + r, I0 + k)
  const int b = blockIdx.y;
  if (info != nullptr && info[b] != 0) return;
  const double* Lb = L + (long)b * a_stride;
  double* Xb = X + (long)b * x_stride;
  const int nB = (N + kLooBlock - 1) / kLooBlock;
  const int J = blockIdx.x, j0 = J * kLooBlock;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int I = J; I < nB; ++I) {
    const int i0 = I * kLooBlock, gr = i0 + lane;
    double acc[16];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) acc[cc] = 0.0;
    for (int k0 = j0; k0 < i0; k0 += kLooTK) {  // (i0 - j0 is a multiple of 64: whole K steps, all of them below N)
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int t = threadIdx.x + 256 * it;
        {  // L(i0 + r, k0 + kk): rows contiguous
          const int r = t % kLooBlock, kk = t / kLooBlock;
          As[kk][r] = (i0 + r < N) ? Lb[(long)(i0 + r) + (long)(k0 + kk) * lda] : 0.0;
        }
        {  // X(k0 + kk, j0 + c): K contiguous; the strict upper triangle of X_JJ is zero without being stored
          const int kk = t % kLooTK, c = t / kLooTK;
          Bs[kk][c] = (j0 + c < N && k0 + kk >= j0 + c) ? Xb[(long)(k0 + kk) + (long)(j0 + c) * ldx] : 0.0;
        }
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kLooTK; ++kk) {
        const double a = As[kk][lane];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) acc[cc] = fma(a, Bs[kk][16 * wave + cc], acc[cc]);
      }
      __syncthreads();
    }
    // L_II (rows past N: the identity) and the reciprocal of this lane's pivot
    for (int t = threadIdx.x; t < kLooBlock * kLooBlock; t += 256) {
      const int r = t % kLooBlock, k = t / kLooBlock;
      Ld[k][r] = (i0 + r < N && i0 + k < N && k <= r) ? Lb[(long)(i0 + r) + (long)(i0 + k) * lda] : (r == k ? 1.0 : 0.0);
    }
    __syncthreads();
    const double rinv = 1.0 / Ld[lane][lane];
    double tv[16];
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) tv[cc] = (I == J) ? ((lane == 16 * wave + cc) ? 1.0 : 0.0) : -acc[cc];
    for (int k = 0; k < kLooBlock; ++k) {
      const double lk = Ld[k][lane];
      const double rk = __shfl(rinv, k, 64);
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        const double xk = __shfl(tv[cc], k, 64) * rk;
        if (lane == k)
          tv[cc] = xk;
        else if (lane > k)
          tv[cc] = fma(-lk, xk, tv[cc]);
      }
    }
    if (gr < N) {
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        const int gc = j0 + 16 * wave + cc;
        if (gc < N) Xb[(long)gr + (long)gc * ldx] = tv[cc];
      }
    }
    __threadfence_block();  // the next block row reads X_IJ back
    __syncthreads();
  }
}

// v[b][j] = row N of the bordered factor b = (L^-1 yc)_j, gathered into a contiguous vector (the row is strided by lda in memory).
__global__ __launch_bounds__(256) void loo_border_row_kernel(const double* __restrict__ A, long lda, long a_stride, int N,
                                                             double* __restrict__ v, long v_stride) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < N) v[(long)blockIdx.y * v_stride + j] = A[(long)blockIdx.y * a_stride + (long)N + (long)j * lda];
}

// The LOO terms of column i of X = L^-1: kappa_i = sum_{r >= i} X_ri^2 = (K^-1)_ii and, with v = L^-1 yc given, alpha_i =
// sum_{r >= i} X_ri v_r = (K^-1 yc)_i (v == NULL: alpha is the caller's and only kappa is written).  One wavefront per column, lanes
// stride over the rows: a fixed summation order from N alone.  grid.y = matrix.
__global__ __launch_bounds__(256) void loo_terms_kernel(int N, const double* __restrict__ X, long ldx, long x_stride,
                                                        const double* __restrict__ v, double* __restrict__ kappa,
                                                        double* __restrict__ alpha, long out_stride) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const long b = blockIdx.y;
  const double* col = X + b * x_stride + (long)i * ldx;
  const double* vb = (v != nullptr) ? v + b * out_stride : nullptr;
  double kq = 0.0, al = 0.0;
  for (int r = i + lane; r < N; r += 64) {
    const double x = col[r];
    kq = fma(x, x, kq);
    if (vb != nullptr) al = fma(x, vb[r], al);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    kq += __shfl_xor(kq, off, 64);
    al += __shfl_xor(al, off, 64);
  }
  if (lane == 0) {
    kappa[b * out_stride + i] = kq;
    if (vb != nullptr) alpha[b * out_stride + i] = al;
  }
}

// out[b] = (t0, t1) = (-sum_i 1/2 log kappa_i, sum_i alpha_i^2 / kappa_i): -1/2 t1 - t0 - 1/2 N log 2 pi is L_LOO, the same
// combination the log marginal likelihood's (sum log L_ii, |L^-1 yc|^2) goes through.  One workgroup per matrix, fixed-order reduction.
__global__ __launch_bounds__(256) void loo_terms_sum_kernel(int N, const double* __restrict__ kappa, const double* __restrict__ alpha,
                                                            long stride, double* __restrict__ out) {
  __shared__ double red[2][256];
  const double* kp = kappa + (long)blockIdx.x * stride;
  const double* ap = alpha + (long)blockIdx.x * stride;
  double a = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) {
    a -= 0.5 * log(kp[i]);
    q += ap[i] * ap[i] / kp[i];
  }
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = red[0][0];
    out[2 * blockIdx.x + 1] = red[1][0];
  }
}

// Per row i: the LOO prediction (mu_i in the caller's units: `mean` added back on the function-value rows, var_i) and the gradient's
// weights c_i = alpha_i / kappa_i, e_i = 1/2 (1 + alpha_i^2 / kappa_i) / kappa_i, sqrt(e_i).  Any output may be NULL.
__global__ __launch_bounds__(256) void loo_point_kernel(int N, int g1, const double* __restrict__ kappa,
                                                        const double* __restrict__ alpha, const double* __restrict__ yc, double mean,
                                                        double* __restrict__ mu, double* __restrict__ var, double* __restrict__ c,
                                                        double* __restrict__ e, double* __restrict__ se) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double k = kappa[i], a = alpha[i];
  const double ci = a / k;
  if (mu != nullptr) mu[i] = (yc[i] - ci) + ((i % g1 == 0) ? mean : 0.0);
  if (var != nullptr) var[i] = 1.0 / k;
  if (c != nullptr) c[i] = ci;
  const double ei = 0.5 * (1.0 + a * ci) / k;
  if (e != nullptr) e[i] = ei;
  if (se != nullptr) se[i] = sqrt(ei);
}

// One pass over K^-1 (N x N, symmetric, ld ldk), one wavefront per column i:
//   mdiag[i] = sum_k e_k K^-1_ki^2 = M_ii, and, where i is a function-value row (i = j g1),
//   B[k + j ldb] = sqrt(e_k) K^-1_ki: column j of B = diag(sqrt e) K^-1 restricted to the columns M's consumers read.
__global__ __launch_bounds__(256) void loo_scale_kernel(int N, int g1, const double* __restrict__ Kinv, long ldk,
                                                        const double* __restrict__ e, const double* __restrict__ se,
                                                        double* __restrict__ B, long ldb, double* __restrict__ mdiag) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  const double* col = Kinv + (long)i * ldk;
  const bool value_row = (i % g1) == 0;
  double* bcol = B + (long)(i / g1) * ldb;
  double m = 0.0;
  for (int k = lane; k < N; k += 64) {
    const double x = col[k];
    m = fma(e[k] * x, x, m);
    if (value_row) bcol[k] = se[k] * x;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off, 64);
  if (lane == 0) mdiag[i] = m;
}

// The weight of entry (i, j) of the function-value block in the gradient's contraction: u_i alpha_j - M_ij.
struct LooWeight {
  const double* u;      // [N]
  const double* alpha;  // [N]
  const double* M;      // n x n, ld ldm: M on the function-value rows / columns
  long ldm;
  int g1;
  __device__ __forceinline__ double row(int i) const { return u[(long)i * g1]; }
  __device__ __forceinline__ double col(int j) const { return alpha[(long)j * g1]; }
  __device__ __forceinline__ double weight(double ri, double cj, int i, int j) const { return fma(ri, cj, -M[(long)i + (long)j * ldm]); }
};

// sum_ij w_ij dK_ij / d(alpha, lengths) over the n x n function-value block, the blocking of the log marginal likelihood's
// ll_grad_kernel (gp.hip: 256 rows x 64 columns per workgroup, row per thread, the 64 x_j broadcast from LDS) with the weight read
// through a functor:
//   part[block][0]     = sum w_ij  dK_ij / d alpha
//   part[block][1 + k] = sum w_ij  first_ij (x_ik - x_jk)^2      (dK_ij / d l_k = first diff_k^2 / l_k^3; the host scales)
template <int DP, class Weight>
__global__ __launch_bounds__(256) void loo_grad_kernel(CovParams cp, const double* __restrict__ X, int n, Weight wt,
                                                       double* __restrict__ part) {
  __shared__ double Xj[64][DP];
  __shared__ double cj[64];
  __shared__ double red[4][1 + DP];
  const int j0 = blockIdx.y * 64, nj = min(64, n - j0);
  for (int t = threadIdx.x; t < nj * DP; t += 256) Xj[t / DP][t % DP] = X[(long)(j0 + t / DP) * DP + t % DP];
  if ((int)threadIdx.x < nj) cj[threadIdx.x] = wt.col(j0 + threadIdx.x);
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  double acc[1 + DP];
#pragma unroll
  for (int k = 0; k <= DP; ++k) acc[k] = 0.0;
  if (i < n) {
    double xi[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xi[k] = X[(long)i * DP + k];
    const double ri = wt.row(i);
    for (int jj = 0; jj < nj; ++jj) {
      double diff2[DP];
      double r2 = 0.0;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const double dlt = xi[k] - Xj[jj][k];
        diff2[k] = dlt * dlt;
        r2 = fma(diff2[k], cp.inv_l2[k], r2);
      }
      const Radial rd = radial_scalars(cp.type, 1.0, r2);  // alpha = 1: base IS dK/d alpha
      const double w = wt.weight(ri, cj[jj], i, j0 + jj);
      acc[0] = fma(w, rd.base, acc[0]);
      const double wf = w * rd.first;
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[1 + k] = fma(wf, diff2[k], acc[1 + k]);
    }
  }
#pragma unroll
  for (int k = 0; k <= DP; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x <= DP) {
    const int k = threadIdx.x;
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * (1 + DP) + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// out[k] = sum over blocks of part[block][k] (k < width), then the noise-variance gradients out[width + a] =
// sum_i u_{i,a} alpha_{i,a} - M_{(i,a),(i,a)} (dK / d sigma_a is the indicator of the rows of observation kind a).  One workgroup.
__global__ __launch_bounds__(256) void loo_grad_finish_kernel(const double* __restrict__ part, int nblocks, int width, int n, int g1,
                                                              const double* __restrict__ u, const double* __restrict__ alpha,
                                                              const double* __restrict__ mdiag, double* __restrict__ out) {
  __shared__ double red[256];
  for (int k = 0; k < width + g1; ++k) {
    double v = 0.0;
    if (k < width) {
      for (int b = threadIdx.x; b < nblocks; b += 256) v += part[(long)b * width + k];
    } else {
      const int a = k - width;
      for (int i = threadIdx.x; i < n; i += 256) {
        const long r = (long)i * g1 + a;
        v += fma(u[r], alpha[r], -mdiag[r]);
      }
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = red[0];
    __syncthreads();
  }
}

template <int DP>
void launch_loo_grad(const CovParams& cp, const double* X, int n, int g1, const LooWeight& wt, const double* mdiag, double* part,
                     double* out, hipStream_t s) {
  dim3 grid((n + 255) / 256, (n + 63) / 64);
  MOE_LAUNCH((loo_grad_kernel<DP, LooWeight>), grid, dim3(256), 0, s, cp, X, n, wt, part);
  MOE_LAUNCH(loo_grad_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (int)(grid.x * grid.y), 1 + DP, n, g1, wt.u,
             wt.alpha, mdiag, out);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

size_t loo_terms_work_doubles(int N) { return (size_t)3 * (size_t)N; }

void launch_loo_terms_batch(const double* A, long lda, long a_stride, int N, double* X, long ldx, long x_stride, double* work,
                            const int* info, double* out, int batch, hipStream_t s) {
  if (batch <= 0 || N <= 0) return;
  const long ws = (long)N;  // per matrix: v | kappa | alpha, each a block of batch * N doubles
  double* v = work;
  double* kappa = work + (size_t)batch * N;
  double* alpha = work + (size_t)2 * batch * N;
  MOE_LAUNCH(loo_trinv_kernel, dim3((N + kLooBlock - 1) / kLooBlock, batch), dim3(256), 0, s, A, lda, a_stride, N, X, ldx, x_stride,
             info);
  MOE_LAUNCH(loo_border_row_kernel, dim3((N + 255) / 256, batch), dim3(256), 0, s, A, lda, a_stride, N, v, ws);
  MOE_LAUNCH(loo_terms_kernel, dim3((N + 3) / 4, batch), dim3(256), 0, s, N, (const double*)X, ldx, x_stride, (const double*)v, kappa,
             alpha, ws);
  MOE_LAUNCH(loo_terms_sum_kernel, dim3(batch), dim3(256), 0, s, N, (const double*)kappa, (const double*)alpha, ws, out);
  MOE_HIP_CHECK(hipGetLastError());
}

void loo_predict_on_device(GpDev& gp, double* mean_out, double* var_out) {
  gp.use_device();
  const int N = gp.N, g1 = 1 + gp.g;
  hipStream_t s = gp.stream;
  gp.looD.reserve((size_t)3 * N);
  const double *Linv = gp.dLinv.p, *alpha = gp.dKinvY.p, *yc = gp.dTmp.p;  // dTmp[0, N): yc = y - mean on the value rows (rebuild)
  const long ldL = gp.ldL;
  const double mean = gp.mean;
  double* kappa = gp.looD.p;
  double* mu = kappa + N;
  double* var = mu + N;
  MOE_LAUNCH(loo_terms_kernel, dim3((N + 3) / 4, 1), dim3(256), 0, s, N, Linv, ldL, 0L, (const double*)nullptr, kappa,
             (double*)nullptr, 0L);
  MOE_LAUNCH(loo_point_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, g1, (const double*)kappa, alpha, yc, mean, mu, var,
             (double*)nullptr, (double*)nullptr, (double*)nullptr);
  MOE_HIP_CHECK(hipGetLastError());
  std::vector<double> h((size_t)2 * N);
  MOE_HIP_CHECK(hipMemcpyAsync(h.data(), mu, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  std::copy(h.begin(), h.begin() + N, mean_out);
  std::copy(h.begin() + N, h.end(), var_out);
}

void grad_loo_log_likelihood(GpDev& gp, double* grad) {
  gp.use_device();
  if (gp.cp.type == MOE_COV_SQUARE_EXPONENTIAL && gp.g > 0)
    throw Error(MOE_ERR_INVALID_VALUE,
                "hyper-parameter gradient with derivative observations is provided for the Matern-5/2 kernel only "
                "(the kernel the reference's Python boundary builds)");
  const int N = gp.N, n = gp.n, g1 = 1 + gp.g, d = gp.d, dp = gp.dp;
  hipStream_t s = gp.stream;
  const size_t nblocks = (size_t)((n + 255) / 256) * ((n + 63) / 64);
  const size_t o_kinv = 0, o_b = o_kinv + (size_t)N * N, o_m = o_b + (size_t)N * n, o_vec = o_m + (size_t)n * n,
               o_part = o_vec + (size_t)6 * N, o_out = o_part + nblocks * (1 + dp), total = o_out + (size_t)(1 + dp + g1);
  gp.looD.reserve(total);
  double* Kinv = gp.looD.p + o_kinv;
  double* B = gp.looD.p + o_b;
  double* M = gp.looD.p + o_m;
  double* kappa = gp.looD.p + o_vec;
  double *c = kappa + N, *e = c + N, *se = e + N, *u = se + N, *mdiag = u + N;
  double* part = gp.looD.p + o_part;
  double* out = gp.looD.p + o_out;
  const double *Linv = gp.dLinv.p, *alpha = gp.dKinvY.p, *yc = gp.dTmp.p, *Xp = gp.dX.p;
  const long ldL = gp.ldL;
  const double mean = gp.mean;
  const CovParams cp = gp.cp;
  // K^-1 = L^-T L^-1, all of it: u and diag M read every column
  launch_tri_gram_strided(N, N, 1, Linv, ldL, Kinv, N, nullptr, s);
  MOE_LAUNCH(loo_terms_kernel, dim3((N + 3) / 4, 1), dim3(256), 0, s, N, Linv, ldL, 0L, (const double*)nullptr, kappa,
             (double*)nullptr, 0L);
  MOE_LAUNCH(loo_point_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, g1, (const double*)kappa, alpha, yc, mean,
             (double*)nullptr, (double*)nullptr, c, e, se);
  launch_gemm_tn(N, 1, N, Kinv, N, c, N, u, N, s);  // u = K^-1 c (K^-1 is symmetric)
  MOE_LAUNCH(loo_scale_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, g1, (const double*)Kinv, (long)N, (const double*)e,
             (const double*)se, B, (long)N, mdiag);
  launch_gemm_tn(n, n, N, B, N, B, N, M, n, s);  // M on the function-value rows / columns: 2 n^2 N flop on the matrix pipe
  LooWeight wt;
  wt.u = u;
  wt.alpha = alpha;
  wt.M = M;
  wt.ldm = n;
  wt.g1 = g1;
  dispatch_dp(dp, [&](auto DP) { launch_loo_grad<DP>(cp, Xp, n, g1, wt, mdiag, part, out, s); });
  std::vector<double> h((size_t)(1 + dp + g1));
  MOE_HIP_CHECK(hipMemcpyAsync(h.data(), out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  grad[0] = h[0];
  for (int k = 0; k < d; ++k) grad[1 + k] = cp.alpha * h[1 + k] * cp.inv_l2[k] * cp.inv_l[k];
  for (int a = 0; a < g1; ++a) grad[1 + d + a] = h[1 + dp + a];
}

}  // namespace moe
