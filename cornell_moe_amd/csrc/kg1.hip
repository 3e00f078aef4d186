// cornell_moe_amd/csrc/kg1.hip -- the exact discretised one-point knowledge gradient and its gradient on the device
// (moe_gp_kg_discrete; Frazier, Powell & Dayanik 2009: the expectation of the minimum of |A| + 1 lines in one standard normal).
//
// For a GP without derivative observations (N = n rows), C candidates x and a discrete set of A points z, with x^ = x with its
// fidelity coordinates set to 1 and Z = {x^} u A:
//   a_z = mu_n(z),  s^2(x) = Sigma_n(x, x) + noise,  b_z(x) = Sigma_n(z, x) / s,  KG_A(x) = min(best, mu_n(x^)) - E[min_z a_z + b_z Z]
// Everything in one upload, on one stream, with one wait and one copy back:
//   once       E_A = K(X, A), V_A = L^-1 E_A, a_A = mu_n(A)                         launch_cov_build, launch_tri_gemm_cols, launch_mean  N^2 A flop
//   per pass of kg1_pass_size(N, A) candidates
//     state    v_x = L^-1 k(X, x) (and v_x^ with fidelity coordinates), mu_n(x^)    launch_cov_build, launch_tri_gemm_cols, launch_mean  N^2 C
//     finish   s^2 = k(x, x) + noise - |v_x|^2 (pivot rule), Sigma_n(x^, x)         kg1_cand_kernel
//     slopes   V_A^T v_x, every entry one fused multiply-add chain over the rows     kg1_slope_kernel                                     2 N A C
//     envelope lines in LDS, bitonic sort, stack scan, segment sums                 kg1_envelope_kernel                                  A log^2 A per candidate
//     gradient t = sum_j w_j V_{z_j} over the envelope's lines, two columns per     kg1_t_kernel, launch_tri_gemm_cols ('T'),
//              candidate through L^-T, then one pass over X per candidate           kg1_grad_kernel                                      2 N^2 C
//
// The host side comes in parts that kg1_opt.hip (the ensemble average and its multistart ascent) shares: kg1_member (checks, buffers,
// layout), kg1_prepare_set ("once"), kg1_eval_pass / kg1_eval_points (a pass of candidates already in device memory, results left
// there, every launch recordable: the five kernels of this file have the body + wrapper form of launch.hpp), then the copy back.
// With pending points (kg1_pending.hip) a member's columns carry p more rows under the N of its own factor: the kernels take the
// number of rows and the columns' leading dimension apart, and the pass calls kg1_pending_rows / kg1_pending_back where m.p > 0.
//
// Bits.  The triangular products take the split-K family at every column count (N < 128: the tiled kernel in chunks that never reach
// its other branch), the slopes are serial fused multiply-add chains over the rows in row order, the slope of x^'s own line is the
// same chain, and the envelope's sums run in the sorted order of the lines.  So a candidate's result does not depend on how many
// candidates share the call, a line that duplicates another (x^ in A included) is bit for bit that line and drops out by the tie
// rule, and a permutation of A changes nothing.  (launch_gemm_tn picks its kernel from the output's shape, and its matrix-pipe
// kernel sums in another order than any chain x^'s own line could repeat: hence the slope kernel of this file.)
//
// The gradient (envelope theorem: the breakpoints' terms cancel), with u1 = L^-T [t / s - (sum_j w_j b_j / s^2) v_x],
// u2 = L^-T [(w_0 / s) v_x], P_0 and w_0 the weights of x^'s line (0 when it is not on the envelope):
//   grad KG = sum_r u1_r grad_x k(X_r, x) - (1 / s) sum_j w_j grad_x k(z_j, x)
//           + [sum_r (([mu_n(x^) < best] - P_0) (K^-1 (y - mean))_r + u2_r) grad k(X_r, x^)] on the free coordinates
// -- d k(x^, x) / d x^ vanishes on the free coordinates, where the two points agree.  One triangular product with two columns per
// candidate replaces grad_kstar and a product with dim columns: N^2 instead of N^2 dim per candidate.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "acq1_device.hpp"
#include "device_cov.hpp"
#include "gp.hpp"

namespace moe {

namespace {

constexpr int kKg1MaxLines = 4096;     // A + 1: 20 B per line in LDS, 80 KiB of the CU's 160
constexpr int kKg1TinyCols = 1024;     // N < 128: columns per triangular product (lcb.hip: kLcbTinyCols)
constexpr double kPivotMin = 1.0e-16;  // gpp_linear_algebra.cpp:118
constexpr int kScal = 4;               // per candidate: P_0, w_0, sum_j w_j b_j, [mu_n(x^) < best]

// one wavefront per candidate: s^2 = k(x, x) + noise - |v_x|^2 with the lanes striding over the rows, and by lane 0 the slope
// numerator of x^'s own line, Sigma_n(x^, x) = k(x^, x) - v_x^ . v_x, as the chain kg1_slope_kernel runs for the lines of A
struct kg1_cand_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int ld, int ncols, int col0, int dp, const CovParams& cp, double noise, const double* __restrict__ Px, const double* __restrict__ Ph, const double* __restrict__ Vx, const double* __restrict__ Vh, double* __restrict__ s2_out, double* __restrict__ b0_out, int* __restrict__ fail) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const double* vx = Vx + (size_t)c * ld;
    double ss = 0.0;
    for (int r = lane; r < N; r += 64) ss = fma(vx[r], vx[r], ss);
  #pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (lane != 0) return;
    const double* vh = Vh + (size_t)c * ld;
    double dot = 0.0;
    for (int r = 0; r < N; ++r) dot = fma(vh[r], vx[r], dot);
    const PointDiff df{Ph + (size_t)c * dp, Px + (size_t)c * dp};
    const double var = (radial_scalars(cp.type, cp.alpha, 0.0).base - ss) + noise;
    s2_out[c] = var;
    b0_out[c] = pair_radial(cp, df, dp).base - dot;
    if (!(var > kPivotMin)) atomicMin(fail, col0 + c);  // the first failing candidate of the call
  }
};
__global__ __launch_bounds__(256) void kg1_cand_kernel(int N, int ld, int ncols, int col0, int dp, const CovParams cp, double noise, const double* __restrict__ Px, const double* __restrict__ Ph, const double* __restrict__ Vx, const double* __restrict__ Vh, double* __restrict__ s2_out, double* __restrict__ b0_out, int* __restrict__ fail) {
  kg1_cand_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, ld, ncols, col0, dp, cp, noise, Px, Ph, Vx, Vh, s2_out, b0_out, fail);
}

// S[z + c A] = V_A[:, z] . V_x[:, c]: 64 x 64 outputs per workgroup, 4 x 4 per thread, the rows staged 32 at a time.  Every output is
// ONE accumulator that takes its products in row order (rows past N add exact zeros).
struct kg1_slope_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int ld, int A, int nc, const double* __restrict__ VA, const double* __restrict__ Vx, double* __restrict__ S) {
    __shared__ double As[32][65];
    __shared__ double Bs[32][65];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, rr = tid & 31, q = tid >> 5;
    const int z0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    double acc[4][4];
  #pragma unroll
    for (int a = 0; a < 4; ++a)
  #pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int r0 = 0; r0 < N; r0 += 32) {
      const int r = r0 + rr;
  #pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int col = q + 8 * i;
        As[rr][col] = (r < N && z0 + col < A) ? VA[r + (size_t)(z0 + col) * ld] : 0.0;
        Bs[rr][col] = (r < N && c0 + col < nc) ? Vx[r + (size_t)(c0 + col) * ld] : 0.0;
      }
      __syncthreads();
  #pragma unroll 8
      for (int kk = 0; kk < 32; ++kk) {
        double fa[4], fb[4];
  #pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = As[kk][tx + 16 * a];
  #pragma unroll
        for (int b = 0; b < 4; ++b) fb[b] = Bs[kk][ty + 16 * b];
  #pragma unroll
        for (int a = 0; a < 4; ++a)
  #pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = fma(fa[a], fb[b], acc[a][b]);
      }
      __syncthreads();
    }
  #pragma unroll
    for (int a = 0; a < 4; ++a)
  #pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int z = z0 + tx + 16 * a, c = c0 + ty + 16 * b;
        if (z < A && c < nc) S[z + (size_t)c * A] = acc[a][b];
      }
  }
};
__global__ __launch_bounds__(256) void kg1_slope_kernel(int N, int ld, int A, int nc, const double* __restrict__ VA, const double* __restrict__ Vx, double* __restrict__ S) {
  kg1_slope_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, ld, A, nc, VA, Vx, S);
}

// the order of the lines: larger slope first, then smaller intercept, then lower index
__device__ __forceinline__ bool line_before(double b1, double a1, int i1, double b2, double a2, int i2) {
  return b1 > b2 || (b1 == b2 && (a1 < a2 || (a1 == a2 && i1 < i2)));
}

// Phi(hi) - Phi(lo) for lo < hi, erfc on the side of the common sign: no cancellation in the tails
__device__ __forceinline__ double normal_cdf_diff(double lo, double hi) {
  const double r = 0.7071067811865475244008443621048490392848;
  if (hi <= 0.0) return 0.5 * (erfc(-hi * r) - erfc(-lo * r));
  if (lo >= 0.0) return 0.5 * (erfc(lo * r) - erfc(hi * r));
  return (1.0 - 0.5 * erfc(-lo * r)) - 0.5 * erfc(hi * r);
}

// sum over the workgroup's 256 threads in a fixed order; valid in every thread
__device__ __forceinline__ double kg1_block_sum(double v, double* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// One workgroup per candidate.  The A + 1 lines (b, a, index; index 0 = x^, 1 + j = point j of A) go to LDS padded to n2, a power of
// two, with lines that sort last; bitonic sort; thread 0 scans them onto the lower envelope in place (equal slopes: the first of the
// sorted run survives, so the smallest intercept and among exact duplicates the lowest index); then every thread takes segments:
//   P_j = Phi(c_j) - Phi(c_j-1),  w_j = phi(c_j-1) - phi(c_j),  E[min] = sum_j a_j P_j + b_j w_j
// hull_w / hull_id [nc][A + 1]: the envelope's w_j and line indices in slope order; scal [nc][kScal].
struct kg1_envelope_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int A, int n2, int dp, int col0, const CovParams& cp, double best, const double* __restrict__ PA, const double* __restrict__ Px, const double* __restrict__ aA, const double* __restrict__ muh, const double* __restrict__ s2, const double* __restrict__ b0, const double* __restrict__ S, double* __restrict__ kg_out, double* __restrict__ nact_out, double* __restrict__ hull_w, int* __restrict__ hull_id, double* __restrict__ scal) {
    extern __shared__ double kg1_smem[];
    __shared__ double s_red[4];
    __shared__ double s_line0[2];
    __shared__ int s_count;
    double* sb = kg1_smem;
    double* sa = kg1_smem + n2;
    int* si = reinterpret_cast<int*>(kg1_smem + 2 * (size_t)n2);
    const int c = blockIdx.x, tid = threadIdx.x;
    const double var = s2[c];
    if (!(var > kPivotMin)) {  // (the call fails on this candidate; the gradient kernels see no lines)
      if (tid == 0) {
        kg_out[col0 + c] = NAN;
        nact_out[col0 + c] = 0.0;
        for (int k = 0; k < kScal; ++k) scal[(size_t)c * kScal + k] = 0.0;
      }
      return;
    }
    const double s = sqrt(var);
    const double* x = Px + (size_t)c * dp;
    for (int i = tid; i < n2; i += 256) {
      double b = -INFINITY, a = INFINITY;
      int id = INT_MAX;
      if (i == 0) {
        b = b0[c] / s;
        a = muh[c];
        id = 0;
      } else if (i <= A) {
        const PointDiff df{PA + (size_t)(i - 1) * dp, x};
        b = (pair_radial(cp, df, dp).base - S[(i - 1) + (size_t)c * A]) / s;
        a = aA[i - 1];
        id = i;
      }
      sb[i] = b;
      sa[i] = a;
      si[i] = id;
    }
    if (tid == 0) {
      s_line0[0] = 0.0;
      s_line0[1] = 0.0;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (n2 >> 1); t += 256) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
          const double b1 = sb[lo], a1 = sa[lo], b2 = sb[hi], a2 = sa[hi];
          const int i1 = si[lo], i2 = si[hi];
          const bool up = (lo & k) == 0;
          if (up ? line_before(b2, a2, i2, b1, a1, i1) : line_before(b1, a1, i1, b2, a2, i2)) {
            sb[lo] = b2;
            sa[lo] = a2;
            si[lo] = i2;
            sb[hi] = b1;
            sa[hi] = a1;
            si[hi] = i1;
          }
        }
        __syncthreads();
      }
    if (tid == 0) {
      // lines p before q (b_p > b_q) cross at (a_q - a_p) / (b_p - b_q), q is the lower one to the right of it.  The top of the stack
      // goes when the new line overtakes the line below the top no later than the top did (compared cross-multiplied: both
      // denominators are positive).
      int sp = 0;
      double prev_b = NAN, bt = 0.0, at = 0.0, bu = 0.0, au = 0.0;  // top of the stack and the line below it
      for (int i = 0; i <= A; ++i) {
        const double bi = sb[i], ai = sa[i];
        const int idi = si[i];
        if (i > 0 && bi == prev_b) continue;
        prev_b = bi;
        while (sp >= 2 && (ai - au) * (bu - bt) <= (at - au) * (bu - bi)) {
          --sp;
          bt = bu;
          at = au;
          if (sp >= 2) {
            bu = sb[sp - 2];
            au = sa[sp - 2];
          }
        }
        sb[sp] = bi;
        sa[sp] = ai;
        si[sp] = idi;
        ++sp;
        bu = bt;
        au = at;
        bt = bi;
        at = ai;
      }
      s_count = sp;
    }
    __syncthreads();
    const int k = s_count;
    double val = 0.0, wb = 0.0;
    for (int j = tid; j < k; j += 256) {
      const double bj = sb[j], aj = sa[j];
      const double lo = (j == 0) ? -INFINITY : (aj - sa[j - 1]) / (sb[j - 1] - bj);
      const double hi = (j == k - 1) ? INFINITY : (sa[j + 1] - aj) / (bj - sb[j + 1]);
      const double P = normal_cdf_diff(lo, hi), w = normal_pdf(lo) - normal_pdf(hi);
      val += fma(bj, w, aj * P);
      wb = fma(w, bj, wb);
      hull_w[(size_t)c * (A + 1) + j] = w;
      hull_id[(size_t)c * (A + 1) + j] = si[j];
      if (si[j] == 0) {
        s_line0[0] = P;
        s_line0[1] = w;
      }
    }
    val = kg1_block_sum(val, s_red);
    wb = kg1_block_sum(wb, s_red);
    if (tid == 0) {
      const double a0 = muh[c];
      kg_out[col0 + c] = fmin(best, a0) - val;
      nact_out[col0 + c] = (double)k;
      scal[(size_t)c * kScal + 0] = s_line0[0];
      scal[(size_t)c * kScal + 1] = s_line0[1];
      scal[(size_t)c * kScal + 2] = wb;
      scal[(size_t)c * kScal + 3] = (a0 < best) ? 1.0 : 0.0;
    }
  }
};
__global__ __launch_bounds__(256) void kg1_envelope_kernel(int A, int n2, int dp, int col0, const CovParams cp, double best, const double* __restrict__ PA, const double* __restrict__ Px, const double* __restrict__ aA, const double* __restrict__ muh, const double* __restrict__ s2, const double* __restrict__ b0, const double* __restrict__ S, double* __restrict__ kg_out, double* __restrict__ nact_out, double* __restrict__ hull_w, int* __restrict__ hull_id, double* __restrict__ scal) {
  kg1_envelope_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, A, n2, dp, col0, cp, best, PA, Px, aA, muh, s2, b0, S, kg_out, nact_out, hull_w, hull_id, scal);
}

// One workgroup per candidate: t = sum_j w_j V_{z_j} over the envelope's lines (x^'s line brings v_x^), then the two right-hand sides
// of the gradient's triangular product, T[:, 2 c] = t / s - (sum_j w_j b_j / s^2) v_x and T[:, 2 c + 1] = (w_0 / s) v_x.
struct kg1_t_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int ld, int A, const double* __restrict__ VA, const double* __restrict__ Vx, const double* __restrict__ Vh, const double* __restrict__ s2, const double* __restrict__ nact, int col0, const double* __restrict__ hull_w, const int* __restrict__ hull_id, const double* __restrict__ scal, double* __restrict__ T) {
    __shared__ double s_w[256];
    __shared__ int s_id[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int k = (int)nact[col0 + c];
    double* t1 = T + (size_t)(2 * c) * ld;
    double* t2 = t1 + ld;
    if (k == 0) {
      for (int r = tid; r < N; r += 256) {
        t1[r] = 0.0;
        t2[r] = 0.0;
      }
      return;
    }
    const double var = s2[c], s = sqrt(var);
    const double w0 = scal[(size_t)c * kScal + 1], swb = scal[(size_t)c * kScal + 2];
    const double* vx = Vx + (size_t)c * ld;
    const double* vh = Vh + (size_t)c * ld;
    const int sweeps = (N + 255) / 256;
    for (int sw = 0; sw < sweeps; ++sw) {
      const int r = sw * 256 + tid;
      double t = 0.0;
      for (int j0 = 0; j0 < k; j0 += 256) {
        __syncthreads();
        if (j0 + tid < k) {
          s_w[tid] = hull_w[(size_t)c * (A + 1) + j0 + tid];
          s_id[tid] = hull_id[(size_t)c * (A + 1) + j0 + tid];
        }
        __syncthreads();
        const int nj = min(256, k - j0);
        if (r < N)
          for (int j = 0; j < nj; ++j) {
            const int id = s_id[j];
            t = fma(s_w[j], (id == 0) ? vh[r] : VA[r + (size_t)(id - 1) * ld], t);
          }
      }
      if (r < N) {
        t1[r] = t / s - (swb / var) * vx[r];
        t2[r] = (w0 / s) * vx[r];
      }
    }
  }
};
__global__ __launch_bounds__(256) void kg1_t_kernel(int N, int ld, int A, const double* __restrict__ VA, const double* __restrict__ Vx, const double* __restrict__ Vh, const double* __restrict__ s2, const double* __restrict__ nact, int col0, const double* __restrict__ hull_w, const int* __restrict__ hull_id, const double* __restrict__ scal, double* __restrict__ T) {
  kg1_t_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, ld, A, VA, Vx, Vh, s2, nact, col0, hull_w, hull_id, scal, T);
}

// One workgroup per candidate: the gradient from the two solved columns U = L^-T T, K^-1 (y - mean) and the envelope's lines.
// FID: fidelity coordinates present -- x^ differs from x, its sums run separately and stay off the fidelity coordinates.
template <int DP, bool FID>
struct kg1_grad_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int n, int ld, int A, int d, int nf, int col0, const CovParams& cp, const double* __restrict__ X, const double* __restrict__ kinvy, const double* __restrict__ PA, const double* __restrict__ Px, const double* __restrict__ Ph, const double* __restrict__ U, const double* __restrict__ s2, const double* __restrict__ nact, const double* __restrict__ hull_w, const int* __restrict__ hull_id, const double* __restrict__ scal, double* __restrict__ grad) {
    __shared__ double s_part[4][DP];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int k = (int)nact[col0 + c];
    double* out = grad + (size_t)(col0 + c) * d;
    if (k == 0) {
      if (tid < d) out[tid] = NAN;
      return;
    }
    const double s = sqrt(s2[c]);
    const double cb = scal[(size_t)c * kScal + 3] - scal[(size_t)c * kScal + 0];  // [mu_n(x^) < best] - P_0
    const double* u1 = U + (size_t)(2 * c) * ld;
    const double* u2 = u1 + ld;
    double x[DP], xh[DP], g[DP];
  #pragma unroll
    for (int i = 0; i < DP; ++i) {
      x[i] = Px[(size_t)c * DP + i];
      xh[i] = FID ? Ph[(size_t)c * DP + i] : x[i];
      g[i] = 0.0;
    }
    for (int r = tid; r < n; r += 256) {
      const double* xr = X + (size_t)r * DP;
      double diff[DP], r2 = 0.0;
  #pragma unroll
      for (int i = 0; i < DP; ++i) {
        diff[i] = xr[i] - x[i];
        r2 = fma(diff[i] * diff[i], cp.inv_l2[i], r2);
      }
      const double ch = fma(cb, kinvy[r], u2[r]);
      const double f = radial_scalars(cp.type, cp.alpha, r2).first * (FID ? u1[r] : u1[r] + ch);
  #pragma unroll
      for (int i = 0; i < DP; ++i) g[i] = fma(f, diff[i] * cp.inv_l2[i], g[i]);
      if (FID) {
        double r2h = 0.0;
  #pragma unroll
        for (int i = 0; i < DP; ++i) {
          diff[i] = xr[i] - xh[i];
          r2h = fma(diff[i] * diff[i], cp.inv_l2[i], r2h);
        }
        const double fh = radial_scalars(cp.type, cp.alpha, r2h).first * ch;
  #pragma unroll
        for (int i = 0; i < DP; ++i)
          if (i < d - nf) g[i] = fma(fh, diff[i] * cp.inv_l2[i], g[i]);
      }
    }
    for (int j = tid; j < k; j += 256) {
      const int id = hull_id[(size_t)c * (A + 1) + j];
      const double* z = (id == 0) ? Ph + (size_t)c * DP : PA + (size_t)(id - 1) * DP;
      double diff[DP], r2 = 0.0;
  #pragma unroll
      for (int i = 0; i < DP; ++i) {
        diff[i] = z[i] - x[i];
        r2 = fma(diff[i] * diff[i], cp.inv_l2[i], r2);
      }
      const double f = -radial_scalars(cp.type, cp.alpha, r2).first * hull_w[(size_t)c * (A + 1) + j] / s;
  #pragma unroll
      for (int i = 0; i < DP; ++i) g[i] = fma(f, diff[i] * cp.inv_l2[i], g[i]);
    }
  #pragma unroll
    for (int i = 0; i < DP; ++i) {
  #pragma unroll
      for (int off = 32; off > 0; off >>= 1) g[i] += __shfl_xor(g[i], off, 64);
    }
    if ((tid & 63) == 0) {
  #pragma unroll
      for (int i = 0; i < DP; ++i) s_part[tid >> 6][i] = g[i];
    }
    __syncthreads();
    if (tid < d) out[tid] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
  }
};
template <int DP, bool FID>
__global__ __launch_bounds__(256) void kg1_grad_kernel(int n, int ld, int A, int d, int nf, int col0, const CovParams cp, const double* __restrict__ X, const double* __restrict__ kinvy, const double* __restrict__ PA, const double* __restrict__ Px, const double* __restrict__ Ph, const double* __restrict__ U, const double* __restrict__ s2, const double* __restrict__ nact, const double* __restrict__ hull_w, const int* __restrict__ hull_id, const double* __restrict__ scal, double* __restrict__ grad) {
  kg1_grad_kernel_body<DP, FID>::run(MOE_VBLOCK, MOE_VGRID, nullptr, n, ld, A, d, nf, col0, cp, X, kinvy, PA, Px, Ph, U, s2, nact, hull_w, hull_id, scal, grad);
}

__global__ void kg1_init_kernel(int* __restrict__ fail, int count) {
  if (blockIdx.x == 0 && (int)threadIdx.x < count) fail[threadIdx.x] = INT_MAX;
}

// the first failing candidate as a double in front of the results: one copy back
__global__ void kg1_pack_kernel(const int* __restrict__ fail, double* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (double)*fail;
}

}  // namespace

// op(L^-1) B for c independent columns, the kernel family fixed by N alone (never by c): below 128 rows the tiled kernel in chunks
// that stay under its switch to the matrix-pipe kernel, from 128 rows the split-K kernels at every column count
void tri_cols(GpDev& gp, char op, int c, const double* B, long ldb, double* Cout, long ldc, hipStream_t s) {
  const int N = gp.N;
  if (N < 128) {
    for (int k0 = 0; k0 < c; k0 += kKg1TinyCols) {
      const int nk = std::min(kKg1TinyCols, c - k0);
      launch_tri_gemm_cols(op, N, nk, nk, gp.dLinv.p, gp.ldL, B + (size_t)k0 * ldb, ldb, Cout + (size_t)k0 * ldc, ldc, nullptr, s);
    }
  } else {
    launch_tri_gemm_cols(op, N, c, 17, gp.dLinv.p, gp.ldL, B, ldb, Cout, ldc, gp.dEK.p, s);
  }
}

// Candidates per pass, from N and A alone: a pass's columns of V stay within 2^24 doubles and its A x pass slope matrix within 2^22,
// a multiple of 64 between 64 and 4096.
int kg1_pass_size(int N, int A) {
  const long cap_v = ((long)1 << 24) / std::max(N, 1), cap_s = ((long)1 << 22) / ((long)std::max(A, 1) + 1);
  return (int)std::max<long>(64, std::min<long>(4096, std::min(cap_v, cap_s) / 64 * 64));
}

void check_kg_discrete_shapes(int num_fidelity, int A, int C) {
  if (C < 1) throw Error(MOE_ERR_BOUNDS, "the number of candidates must be positive", C, 1, 1e9);
  if (A < 1 || A + 1 > kKg1MaxLines)
    throw Error(MOE_ERR_BOUNDS, "the discrete set and the candidate make between 2 and 4096 lines", A, 1, kKg1MaxLines - 1);
  if (num_fidelity < 0) throw Error(MOE_ERR_BOUNDS, "num_fidelity out of range", num_fidelity, 0, 1e9);
}

void check_kg_discrete_member(const GpDev& gp, int nf) {
  if (nf >= gp.d) throw Error(MOE_ERR_BOUNDS, "num_fidelity out of range", nf, 0, gp.d - 1);
  if (gp.g > 0)
    throw Error(MOE_ERR_BOUNDS,
                "the discretised one-point knowledge gradient needs a GP without derivative observations: with them the fantasy "
                "has 1 + num_derivatives dimensions and the quantity is not a minimum of lines",
                gp.g, 0, 0);
}

Kg1Member kg1_member(GpDev& gp, int nf, int A, int C, double best, bool with_grad, int* fail, int pcap, int* fail_pending) {
  check_kg_discrete_shapes(nf, A, C);
  check_kg_discrete_member(gp, nf);
  gp.use_device();
  Kg1Member m;
  m.gp = &gp;
  m.nf = nf;
  m.A = A;
  m.C = C;
  m.best = best;
  m.with_grad = with_grad;
  m.fid = nf > 0;
  m.per_pass = kg1_pass_size(gp.N, A);
  m.widest = std::min(m.per_pass, C);
  m.n2 = 2;
  while (m.n2 < A + 1) m.n2 <<= 1;
  const int N = gp.N;
  m.pcap = pcap;
  m.ld = N + pcap;  // (the columns of V, T and U keep room for the pending rows under the member's own)
  const size_t nA = (size_t)A, nC = (size_t)C, nW = (size_t)m.widest, nL = (size_t)m.ld;
  // doubles: [fail | kg C | active C | grad C d] (the copy back) | V_A N A | a_A A | per pass: V_x, V_x^ N W each | T, U N 2W each |
  //          mu_n(x^), s^2, slope numerator of x^ W each | slopes A W | envelope weights (A + 1) W | scalars kScal W |
  //          with pending points (kg1_pending.hip): X u P (N + pcap) dp | [K^-1 (y - mean) ; 0] N + pcap | the extension (N + pcap) pcap
  const size_t nOut = m.out_doubles();
  const size_t nV = nL * nW;
  gp.kg1D.reserve(nOut + nL * nA + nA + (m.fid ? 2 : 1) * nV + (with_grad ? 4 * nV : 0) + 3 * nW + nA * nW + (nA + 1) * nW +
                  kScal * nW + (pcap > 0 ? nL * ((size_t)gp.dp + 1 + (size_t)pcap) : 0));
  gp.kg1I.reserve(2 + (nA + 1) * nW);
  gp.kg1LastC = C;
  m.dOut = gp.kg1D.p;
  m.dKg = m.dOut + 1;
  m.dAct = m.dKg + nC;
  m.dGrad = m.dAct + nC;
  m.dVA = m.dOut + nOut;
  m.dAA = m.dVA + nL * nA;
  m.dVx = m.dAA + nA;
  m.dVh = m.fid ? m.dVx + nV : m.dVx;
  m.dT = m.dVh + nV;
  m.dU = m.dT + (with_grad ? 2 * nV : 0);
  m.dMuh = m.dU + (with_grad ? 2 * nV : 0);
  m.dS2 = m.dMuh + nW;
  m.dB0 = m.dS2 + nW;
  m.dS = m.dB0 + nW;
  m.dHw = m.dS + nA * nW;
  m.dScal = m.dHw + (nA + 1) * nW;
  if (pcap > 0) {
    m.dXe = m.dScal + kScal * nW;
    m.dKe = m.dXe + nL * (size_t)gp.dp;
    m.dVP = m.dKe + nL;
  }
  m.iFail = fail != nullptr ? fail : gp.kg1I.p;
  m.iFailP = fail_pending != nullptr ? fail_pending : gp.kg1I.p + 1;
  m.iHid = gp.kg1I.p + 2;
  gp.dE.reserve((size_t)N * std::max(std::max(nA, nW), (size_t)pcap));
  if (N >= 128) gp.dEK.reserve(tri_cols_work_doubles(N, (int)std::max(std::max(nA, 2 * nW), (size_t)pcap)));
  MOE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kg1_envelope_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kKg1MaxLines * (2 * sizeof(double) + sizeof(int)))));
  return m;
}

void kg_discrete_last_active(GpDev& gp, int C, int* nact_out) {
  if (C < 1 || C != gp.kg1LastC)
    throw Error(MOE_ERR_BOUNDS, "num_points must be the number of candidates of the GP's last discretised knowledge-gradient call", C,
                gp.kg1LastC, gp.kg1LastC);
  if (nact_out == nullptr) throw Error(MOE_ERR_RUNTIME, "NULL argument");
  gp.use_device();
  gp.hStateOut.reserve((size_t)C);
  MOE_HIP_CHECK(hipMemcpyAsync(gp.hStateOut.p, gp.kg1D.p + 1 + (size_t)C, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, gp.stream));
  MOE_HIP_CHECK(hipStreamSynchronize(gp.stream));
  for (int i = 0; i < C; ++i) nact_out[i] = (int)gp.hStateOut.p[i];
}

void kg1_clear_fail(int* fail, int count, hipStream_t s) {
  if (count < 1 || count > 1024) throw Error(MOE_ERR_RUNTIME, "kg1_clear_fail: between 1 and 1024 words");
  MOE_LAUNCH(kg1_init_kernel, dim3(1), dim3(1024), 0, s, fail, count);
  MOE_HIP_CHECK(hipGetLastError());
}

void kg1_prepare_set(const Kg1Member& m, hipStream_t s) {
  GpDev& gp = *m.gp;
  const DerivList none = no_derivs();
  launch_cov_build(gp.cp, gp.dX.p, gp.n, none, m.dPA, m.A, none, nullptr, gp.dE.p, gp.N, 0, s);
  tri_cols(gp, 'N', m.A, gp.dE.p, gp.N, m.dVA, m.ld, s);
  launch_mean(gp.cp, gp.dX.p, gp.n, none, gp.dKinvY.p, m.dPA, m.A, gp.mean, false, m.dAA, s);
  if (m.p > 0) kg1_pending_rows(m, m.dPA, m.dVA, m.A, 0, m.p, s);
}

void kg1_eval_pass(const Kg1Member& m, const double* Px, const double* Ph, int nc, int c0, bool with_grad, hipStream_t s) {
  GpDev& gp = *m.gp;
  if (nc < 1 || nc > m.widest || c0 < 0 || c0 + nc > m.C || (with_grad && !m.with_grad))
    throw Error(MOE_ERR_RUNTIME, "kg1_eval_pass: the pass does not fit the member's buffers");
  // R rows of X u P under the columns' leading dimension; without pending points the member's own N rows, the kernels of before
  const int N = gp.N, n = gp.n, d = gp.d, dp = gp.dp, A = m.A, nf = m.nf, R = N + m.p, ld = m.ld;
  const double* Xr = m.p > 0 ? m.dXe : gp.dX.p;
  const double* Kr = m.p > 0 ? m.dKe : gp.dKinvY.p;
  const DerivList none = no_derivs();
  const size_t shm = (size_t)m.n2 * (2 * sizeof(double) + sizeof(int));
  const dim3 b256(256);
  launch_cov_build(gp.cp, gp.dX.p, n, none, Px, nc, none, nullptr, gp.dE.p, N, 0, s);
  tri_cols(gp, 'N', nc, gp.dE.p, N, m.dVx, ld, s);
  if (m.p > 0) kg1_pending_rows(m, Px, m.dVx, nc, 0, m.p, s);
  if (m.fid) {
    launch_cov_build(gp.cp, gp.dX.p, n, none, Ph, nc, none, nullptr, gp.dE.p, N, 0, s);
    tri_cols(gp, 'N', nc, gp.dE.p, N, m.dVh, ld, s);
    if (m.p > 0) kg1_pending_rows(m, Ph, m.dVh, nc, 0, m.p, s);
  }
  launch_mean(gp.cp, gp.dX.p, n, none, gp.dKinvY.p, Ph, nc, gp.mean, false, m.dMuh, s);
  launch_kernel_ens<kg1_cand_kernel_body, 256>(kg1_cand_kernel, dim3((unsigned)((nc + 3) / 4)), b256, 0, s, R, ld, nc, c0, dp, gp.cp,
                                               gp.noise[0], Px, Ph, (const double*)m.dVx, (const double*)m.dVh, m.dS2, m.dB0, m.iFail);
  launch_kernel_ens<kg1_slope_kernel_body, 256>(kg1_slope_kernel, dim3((unsigned)((A + 63) / 64), (unsigned)((nc + 63) / 64)), b256, 0, s,
                                                R, ld, A, nc, (const double*)m.dVA, (const double*)m.dVx, m.dS);
  launch_kernel_ens<kg1_envelope_kernel_body, 256>(kg1_envelope_kernel, dim3((unsigned)nc), b256, shm, s, A, m.n2, dp, c0, gp.cp, m.best,
                                                   m.dPA, Px, (const double*)m.dAA, (const double*)m.dMuh, (const double*)m.dS2,
                                                   (const double*)m.dB0, (const double*)m.dS, m.dKg, m.dAct, m.dHw, m.iHid, m.dScal);
  MOE_HIP_CHECK(hipGetLastError());
  if (!with_grad) return;
  launch_kernel_ens<kg1_t_kernel_body, 256>(kg1_t_kernel, dim3((unsigned)nc), b256, 0, s, R, ld, A, (const double*)m.dVA, (const double*)m.dVx,
                                            (const double*)m.dVh, (const double*)m.dS2, (const double*)m.dAct, c0, (const double*)m.dHw,
                                            (const int*)m.iHid, (const double*)m.dScal, m.dT);
  if (m.p > 0) kg1_pending_back(m, 2 * nc, s);  // (L'^-T: the pending block first, then the member's own on the corrected rows)
  tri_cols(gp, 'T', 2 * nc, m.dT, ld, m.dU, ld, s);
  dispatch_dp(dp, [&](auto DP) {
    if (m.fid)
      launch_kernel_ens<kg1_grad_kernel_body<DP, true>, 256>(kg1_grad_kernel<DP, true>, dim3((unsigned)nc), b256, 0, s, R, ld, A, d, nf, c0, gp.cp,
                                                             Xr, Kr, m.dPA, Px, Ph,
                                                             (const double*)m.dU, (const double*)m.dS2, (const double*)m.dAct,
                                                             (const double*)m.dHw, (const int*)m.iHid, (const double*)m.dScal, m.dGrad);
    else
      launch_kernel_ens<kg1_grad_kernel_body<DP, false>, 256>(kg1_grad_kernel<DP, false>, dim3((unsigned)nc), b256, 0, s, R, ld, A, d, nf, c0, gp.cp,
                                                              Xr, Kr, m.dPA, Px, Ph,
                                                              (const double*)m.dU, (const double*)m.dS2, (const double*)m.dAct,
                                                              (const double*)m.dHw, (const int*)m.iHid, (const double*)m.dScal, m.dGrad);
  });
  MOE_HIP_CHECK(hipGetLastError());
}

void kg1_eval_points(const Kg1Member& m, const double* Px, const double* Ph, int C, bool with_grad, hipStream_t s) {
  const int dp = m.gp->dp;
  for (int c0 = 0; c0 < C; c0 += m.per_pass)
    kg1_eval_pass(m, Px + (size_t)c0 * dp, Ph + (size_t)c0 * dp, std::min(m.per_pass, C - c0), c0, with_grad, s);
}

// prepare the set, evaluate pass after pass, copy back: one upload, one stream, one wait
void kg_discrete_on_device(GpDev& gp, int nf, const double* discrete, int A, const double* pts, int C, double best, bool want_grad,
                           double* kg_out, double* grad_out, int* nact_out) {
  check_kg_discrete_shapes(nf, A, C);
  check_kg_discrete_member(gp, nf);
  if (discrete == nullptr || pts == nullptr || kg_out == nullptr || (want_grad && grad_out == nullptr))
    throw Error(MOE_ERR_RUNTIME, "NULL argument");
  Kg1Member m = kg1_member(gp, nf, A, C, best, want_grad);
  hipStream_t s = gp.stream;
  const int d = gp.d, dp = gp.dp, size = d - nf;
  const bool fid = m.fid;
  const size_t nA = (size_t)A, nC = (size_t)C;

  // one copy down: [A discrete points, fidelity coordinates 1 | C candidates | C candidates with fidelity coordinates 1], padded
  const size_t nIn = (nA + nC * (fid ? 2 : 1)) * dp;
  gp.hStateIn.reserve(nIn);
  double* h = gp.hStateIn.p;
  for (size_t i = 0; i < nA; ++i)
    for (int k = 0; k < dp; ++k) h[i * dp + k] = (k < size) ? discrete[i * size + k] : (k < d ? 1.0 : 0.0);
  for (size_t i = 0; i < nC; ++i)
    for (int k = 0; k < dp; ++k) {
      const double v = (k < d) ? pts[i * d + k] : 0.0;
      h[(nA + i) * dp + k] = v;
      if (fid) h[(nA + nC + i) * dp + k] = (k >= size && k < d) ? 1.0 : v;
    }
  gp.dStateIn.upload(h, nIn, s, true);
  m.dPA = gp.dStateIn.p;
  const double* dPx = m.dPA + nA * dp;
  const double* dPh = fid ? dPx + nC * dp : dPx;

  kg1_clear_fail(m.iFail, 1, s);
  kg1_prepare_set(m, s);
  kg1_eval_points(m, dPx, dPh, C, want_grad, s);
  MOE_LAUNCH_NOW(kg1_pack_kernel, dim3(1), dim3(64), 0, s, (const int*)m.iFail, m.dOut);
  MOE_HIP_CHECK(hipGetLastError());
  const size_t nOut = m.out_doubles();
  gp.hStateOut.reserve(nOut);
  gp.kg1D.download(gp.hStateOut.p, nOut, s);
  MOE_HIP_CHECK(hipStreamSynchronize(s));
  const double* o = gp.hStateOut.p;
  if (o[0] < (double)C)
    throw Error(MOE_ERR_SINGULAR,
                "GP-Variance matrix singular. Check for duplicate points_to_sample or points_to_sample "
                "duplicating points_sampled with 0 noise.",
                1, (int)o[0]);
  std::memcpy(kg_out, o + 1, sizeof(double) * nC);
  if (nact_out)
    for (size_t i = 0; i < nC; ++i) nact_out[i] = (int)o[1 + nC + i];
  if (want_grad) std::memcpy(grad_out, o + 1 + 2 * nC, sizeof(double) * nC * d);
}

}  // namespace moe
