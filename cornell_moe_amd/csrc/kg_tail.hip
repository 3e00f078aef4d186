// cornell_moe_amd/csrc/kg_tail.hip -- the gradient tail of a q-KG / d-KG Monte-Carlo evaluation on gfx950: its kernels and their
// launchers (kg_tail.hpp; the driver is kg.hip).
//
// The tail (gpp_knowledge_gradient_optimization.cpp:199-225 restated so that nothing of size M x (q d) is ever formed):
//        T   = K(X, x*_i) for every sample                      (covariance build, N x M per evaluation, HBM write-bound)
//        c_i = L^-1 ( K(Xu, x*_i) - W^T T_i )                   (kg_sw_kernel: one wave per sample)
//        TB  = sum_i T_i beta_i^T                               (kg_tb_kernel + fixed-order chunk reduction)
//      and three small reductions  ZC = sum_i z_i c_i^T (m x m),  DIR = sum_i beta_i,(k,b) dK(Xu_k, x*_i)[b,0]/dXu_k,
//      GTB = (K^-1 dK*/dXq)^T TB,  from which kg_state.hip's finish kernels assemble
//        grad KG[k,dd] = ( [winner = k] M grad mu_k  -  sum_b (DIR - GTB)[(k,b),dd]  +  < L^-1 dL/dXq_k,dd , ZC > ) / M.
//      This is  sum_i z_i^T d(c_i)/dXq_k  of the reference (gpp_math.cpp:1601-1651) with the sum over samples pulled inside.
//      (q-KG, m <= 8: T is never written and, by default, c_i never formed -- ZC = L^T (KB - TB^T W) L^-T, see launch_fused_tail.)
// All reductions use fixed orders, so results are bitwise reproducible for a given shard layout.
#include "kg_tail.hpp"

#include <type_traits>

#include "device_cov.hpp"
#include "fastmath.hpp"
#include "gemm128.hpp"

namespace moe {

namespace {

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sum over a 256-thread workgroup in a fixed order; result valid in thread 0.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const double w = wave_sum64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// c_i = L^-1 ( K(Xu, x*_i)[:, 0] - W^T T_i ) for every sample; one wavefront per sample at a time, lane r owns component r.
// S_W = W^T T_i comes either precomputed (P.SW: tile GEMM, large m) or is formed here by lanes striding the N rows with
// W_e staged ONCE per workgroup in LDS ([c][row], conflict-free) and reused for the kSwChunk samples of the workgroup --
// re-reading W from L2 for every sample (N m 8 bytes each) made this the slowest kernel of the tail.
// SLOTS = 2: components lane and lane + 64 (m up to 128; S_W always precomputed there).
template <int DP, int MU, int SLOTS = 1>
struct kg_sw_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P) {
    extern __shared__ __attribute__((aligned(16))) double Ws[];  // [m][N] when P.SW == nullptr
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.y;
    const int m = P.m, g1 = 1 + P.g, N = P.N;
    const double* rec = P.blob + (long)e * P.rec.stride;
    const double* Lsm = rec + P.rec.L;
    if (P.SW == nullptr) {
      const double* We = P.W + (long)e * P.w_stride;
      for (int t = threadIdx.x; t < N * m; t += 256) Ws[t] = We[t];  // W_e is [N x m] col-major == [c][row]
      __syncthreads();
    }
    const int i1 = min(P.num_local, (int)(blockIdx.x + 1) * P.sw_chunk);
    for (int i = blockIdx.x * P.sw_chunk + wave; i < i1; i += 4) {
      const long w = (long)e * P.num_local + i;
      double mine[SLOTS];
  #pragma unroll
      for (int sl = 0; sl < SLOTS; ++sl) mine[sl] = 0.0;
      if (P.SW != nullptr) {
  #pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
          if (lane + 64 * sl < m) mine[sl] = P.SW[w * m + lane + 64 * sl];
      } else {
        const double* Tc = P.T + w * N;
        double acc[MU];
  #pragma unroll
        for (int c = 0; c < MU; ++c) acc[c] = 0.0;
  #pragma unroll 4
        for (int row = lane; row < N; row += 64) {
          const double t = Tc[row];
  #pragma unroll
          for (int c = 0; c < MU; ++c)
            if (c < m) acc[c] = fma(Ws[c * N + row], t, acc[c]);
        }
  #pragma unroll
        for (int c = 0; c < MU; ++c) {
          const double v = wave_sum64(acc[c]);
          if (lane == c) mine[0] = v;
        }
      }
      double R[SLOTS], cv[SLOTS];
  #pragma unroll
      for (int sl = 0; sl < SLOTS; ++sl) {
        R[sl] = 0.0;
        cv[sl] = 0.0;
        const int comp = lane + 64 * sl;
        if (comp < m) {
          const int r = comp / g1, b = comp - r * g1;
          const double* Xu = rec + P.rec.XuP + (long)r * DP;
          const double* xs = P.best_point + w * DP;
          double diff[DP];
          double r2 = 0.0;
  #pragma unroll
          for (int k = 0; k < DP; ++k) {
            diff[k] = Xu[k] - xs[k];
            r2 = fma(diff[k] * diff[k], P.cp.inv_l2[k], r2);
          }
          const Radial rd = radial_scalars(P.cp.type, P.cp.alpha, r2);
          DerivList none;
          none.g = 0;
          R[sl] = cov_entry<DP>(P.cp, rd, diff, b, 0, P.derivs, none) - mine[sl];
        }
      }
      for (int r = 0; r < m; ++r) {
        double part = 0.0;
  #pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
          if (lane + 64 * sl < r) part = fma(Lsm[r + (long)(lane + 64 * sl) * m], cv[sl], part);
        const double tot = wave_sum64(part);
  #pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
          if (lane + 64 * sl == r) cv[sl] = (R[sl] - tot) / Lsm[r + (long)r * m];
      }
  #pragma unroll
      for (int sl = 0; sl < SLOTS; ++sl)
        if (lane + 64 * sl < m) P.C[w * m + lane + 64 * sl] = cv[sl];
    }
  }
};
template <int DP, int MU, int SLOTS = 1>
__global__ __launch_bounds__(256) void kg_sw_kernel(KgTailParams P) {
  kg_sw_kernel_body<DP, MU, SLOTS>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P);
}

// TBpart[e][chunk][c][row] = sum over the chunk's samples of T[row, i] beta_i[c]   (thread = row; T read coalesced, the
// beta row is wave-uniform).
template <int MU>
struct kg_tb_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, int c_lo) {    // columns [c_lo, c_lo + MU) of beta / TB
    const int row = blockIdx.x * 256 + threadIdx.x;
    const int chunk = blockIdx.y, e = blockIdx.z;
    const int m = P.m;
    const int i0 = chunk * P.chunk_len, i1 = min(P.num_local, i0 + P.chunk_len);
    double acc[MU];
  #pragma unroll
    for (int c = 0; c < MU; ++c) acc[c] = 0.0;
    const bool ok = row < P.N;
    const double* __restrict__ Tcol = P.T + (ok ? row : 0);
    const double* __restrict__ beta = P.beta;
  #pragma unroll 4
    for (int i = i0; i < i1; ++i) {
      const long w = (long)e * P.num_local + i;
      const double t = Tcol[w * P.N];
      const double* __restrict__ b = beta + w * m + c_lo;
      // all MU entries unconditionally (uniform, contiguous: wide scalar loads, no branch per entry); the entries beyond m
      // belong to the next sample / the pad behind the buffer and only feed accumulators that are never stored
  #pragma unroll
      for (int c = 0; c < MU; ++c) acc[c] = fma(t, b[c], acc[c]);
    }
    if (ok) {
      double* dst = P.TBpart + ((long)e * P.chunks + chunk) * m * P.N;
  #pragma unroll
      for (int c = 0; c < MU; ++c)
        if (c_lo + c < m) dst[(long)(c_lo + c) * P.N + row] = acc[c];
    }
  }
};
template <int MU>
__global__ __launch_bounds__(256) void kg_tb_kernel(KgTailParams P, int c_lo = 0) {
  kg_tb_kernel_body<MU>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, c_lo);
}

// The same partial sums for m > 64 (r4; the stretch point's m = 104) as a product on the matrix pipe: TBpart[e][chunk] (N x m) =
// T_e[:, chunk] (N x len) beta_e[chunk, :] (len x m) through gemm128.hpp's tile core -- one pass over T instead of one per 64 columns
// of beta, chunks of kTbChunkWide samples (ten partials instead of 79 at M = 20 000).  Grid (row tiles of 128, chunks, E).
struct kg_tb128_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int chunk = blockIdx.y, e = blockIdx.z, m = P.m;
    const int i0 = chunk * P.chunk_len, len = min(P.num_local - i0, P.chunk_len);
    const long w0 = (long)e * P.num_local + i0;
    g128::Operand A{P.T + w0 * P.N, (long)P.N, P.N, len, 1};     // T[row + sample N]: rows contiguous
    g128::Operand B{P.beta + w0 * m, (long)m, m, len, 1};        // beta[sample m + c]: the output column contiguous
    g128::f64x4 acc[4][4];
    const int r0 = blockIdx.x * g128::TM;
    g128::tile_product<false, false>(A, B, r0, 0, 0, len, smem, acc);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wi = (wave & 1) * 64, wj = (wave >> 1) * 64;
    const int lk = lane >> 4, lx = lane & 15;
    double* dst = P.TBpart + ((long)e * P.chunks + chunk) * m * P.N;
  #pragma unroll
    for (int a = 0; a < 4; ++a)
  #pragma unroll
      for (int b = 0; b < 4; ++b)
  #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + wi + 16 * a + lx, c = wj + 16 * b + lk + 4 * r;
          if (row < P.N && c < m) dst[(long)c * P.N + row] = acc[a][b][r];
        }
  }
};
__global__ __launch_bounds__(256, 2) void kg_tb128_kernel(KgTailParams P) {
  kg_tb128_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P);
}

// S_W = W_e^T T_e (m x samples) for 64 < m <= 128 on the same tile core: one 128-row tile holds all m rows, so T is read ONCE (the
// 64-tile kernel reads it once per row tile: twice at m = 104).  K = N is cut into `slices`; slice sl of evaluation e goes to
// SWpart[sl][e] (dense m x num_local), summed in slice order by sum_slices_kernel.  Grid (column tiles of 128 samples, slices, E).
struct kg_sw128_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, double* __restrict__ SWpart, int slices) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int sl = blockIdx.y, e = blockIdx.z, m = P.m;
    const int ks = ((P.N + slices - 1) / slices + g128::TK - 1) / g128::TK * g128::TK;
    const int k_lo = sl * ks, k_hi = min(P.N, k_lo + ks);
    g128::Operand A{P.W + (long)e * P.w_stride, (long)P.N, m, P.N, 1};                        // W[row + c N]: K (= row) contiguous
    g128::Operand B{P.T + (long)e * P.num_local * P.N, (long)P.N, P.num_local, P.N, 1};      // T[row + sample N]: K contiguous
    g128::f64x4 acc[4][4];
    const int j0 = blockIdx.x * g128::TM;
    g128::tile_product<true, true>(A, B, 0, j0, k_lo, k_hi, smem, acc);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wi = (wave & 1) * 64, wj = (wave >> 1) * 64;
    const int lk = lane >> 4, lx = lane & 15;
    double* dst = SWpart + ((long)sl * P.E + e) * m * P.num_local;
  #pragma unroll
    for (int a = 0; a < 4; ++a)
  #pragma unroll
      for (int b = 0; b < 4; ++b)
  #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = wi + 16 * a + lx, smp = j0 + wj + 16 * b + lk + 4 * r;
          if (c < m && smp < P.num_local) dst[(long)smp * m + c] = acc[a][b][r];
        }
  }
};
__global__ __launch_bounds__(256, 2) void kg_sw128_kernel(KgTailParams P, double* __restrict__ SWpart, int slices) {
  kg_sw128_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, SWpart, slices);
}

// TB[e][c][row] = sum of the chunk partials in chunk order (one pass over TBpart instead of one per gradient column).
struct kg_tbsum_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, double* __restrict__ TBsum) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over m * N
    const int e = blockIdx.y;
    const long mn = (long)P.m * P.N;
    if (idx >= mn) return;
    const double* part = P.TBpart + (long)e * P.chunks * mn + idx;
    double tb = 0.0;
  #pragma unroll 8
    for (int ch = 0; ch < P.chunks; ++ch) tb += part[(long)ch * mn];  // (independent loads, issued eight at a time)
    TBsum[(long)e * mn + idx] = tb;
  }
};
__global__ __launch_bounds__(256) void kg_tbsum_kernel(KgTailParams P, double* __restrict__ TBsum) {
  kg_tbsum_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, TBsum);
}

// GTB[e][gc] = sum_row dK*_e[row, gc] * (K^-1 TB_e)[row, col(gc)];  gc = (k (1+g) + b) d + dd  ->  col = k (1+g) + b.
struct kg_gtb_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, const double* __restrict__ TBsum) {
    __shared__ double red[4];
    const int gc = blockIdx.x, e = blockIdx.y;
    const int col = gc / P.cp.dim;
    const double* Gc = P.Gm + (long)e * P.g_stride + (long)gc * P.N;
    const double* tb = TBsum + ((long)e * P.m + col) * P.N;
    double acc = 0.0;
    for (int row = threadIdx.x; row < P.N; row += 256) acc = fma(Gc[row], tb[row], acc);
    const double tot = block_sum_256(acc, red);
    if (threadIdx.x == 0) P.out[(long)e * P.out_stride + 1 + P.m * P.m + P.ngrad + gc] = tot;
  }
};
__global__ __launch_bounds__(256) void kg_gtb_kernel(KgTailParams P, const double* __restrict__ TBsum) {
  kg_gtb_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, TBsum);
}

// The summed TB lives behind the chunk partials in the same buffer (the host reserves E (chunks + 1) m N doubles).
void launch_gtb(const KgTailParams& P, hipStream_t s) {
  const long mn = (long)P.m * P.N;
  double* TBsum = P.TBpart + (long)P.E * P.chunks * mn;
  launch_kernel_ens<kg_tbsum_kernel_body, 256>(kg_tbsum_kernel, dim3((unsigned)((mn + 255) / 256), P.E), dim3(256), 0, s, P, TBsum);
  // (K^-1 dK*)^T TB = dK*^T (K^-1 TB): the two triangular products run over the m columns of TB, not over the q (1 + g) d columns of
  // dK* (r4: 32 against 384 per evaluation at C5)
  const int cm = P.E * P.m;
  double* half = P.work;
  double* KinvTB = P.work + (long)P.N * cm;
  launch_tri_gemm_cols('N', P.N, cm, P.m, P.Linv, P.ldL, TBsum, P.N, half, P.N, P.tri_work, s);
  launch_tri_gemm_cols('T', P.N, cm, P.m, P.Linv, P.ldL, half, P.N, KinvTB, P.N, P.tri_work, s);
  launch_kernel_ens<kg_gtb_kernel_body, 256>(kg_gtb_kernel, dim3(P.ngrad, P.E), dim3(256), 0, s, P, (const double*)KinvTB);
}

// ZC[e][r + j m] = sum_i z_i[r] c_i[j] and kg_sum = sum_i (best_posterior + best_value_i)   (.cpp:196).
// Without a strided sample walk (round 1: one workgroup per (r, j) reading c_i[j] every m doubles: 254 us for two
// C5 evaluations): a workgroup takes a chunk of kZcChunk samples, stages their z and c rows in LDS with coalesced loads and forms all
// m x m partial products; kg_zc_sum_kernel adds the chunk partials in chunk order and forms kg_sum exactly as kg_sum_kernel does.
struct kg_zc_part_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, double* __restrict__ part, int chunks, int len) {
    extern __shared__ __attribute__((aligned(16))) double zc_sm[];  // z [len][m] | c [len][m]
    const int chunk = blockIdx.x, e = blockIdx.y, m = P.m;
    const int i0 = chunk * len, cnt = min(len, P.num_local - i0);
    double* zs = zc_sm;
    double* cs = zc_sm + len * m;
    for (int t = threadIdx.x; t < cnt * m; t += 256) {
      const int ii = t / m, r = t - ii * m;
      const int s = P.first_sample + i0 + ii;
      zs[t] = ((s & 1) ? -1.0 : 1.0) * P.normals[(long)(s >> 1) * m + r];
      cs[t] = P.C[((long)e * P.num_local + i0 + ii) * m + r];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < m * m; o += 256) {
      const int r = o % m, j = o / m;
      double acc = 0.0;
  #pragma unroll 4
      for (int ii = 0; ii < cnt; ++ii) acc = fma(zs[ii * m + r], cs[ii * m + j], acc);
      part[((long)e * chunks + chunk) * m * m + o] = acc;
    }
  }
};
__global__ __launch_bounds__(256) void kg_zc_part_kernel(KgTailParams P, double* __restrict__ part, int chunks, int len) {
  kg_zc_part_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, part, chunks, len);
}

// (r4: `gs` lanes share an output -- a power of two, m m gs <= 256 -- and stride the chunks, then a fixed butterfly: a lane per output
//  walked all the chunks in batches of eight loads, one memory round trip per batch: 19 us for the 157 chunks of one C3 evaluation)
struct kg_zc_sum_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, const double* __restrict__ part, int chunks, int gs) {
    __shared__ double red[4];
    const int e = blockIdx.y, m = P.m;
    const int per_block = 256 / gs;
    const int o = blockIdx.x * per_block + (int)threadIdx.x / gs, g = (int)threadIdx.x % gs;
    double* out = P.out + (long)e * P.out_stride;
    {
      const bool ok = o < m * m;
      const double* p = part + (long)e * chunks * m * m + (ok ? o : 0);
      double v = 0.0;
  #pragma unroll 8
      for (int ch = g; ch < chunks; ch += gs) v += p[(long)ch * m * m];
      for (int off = gs >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (ok && g == 0) out[1 + o] = v;
    }
    if (blockIdx.x == 0) {  // kg_sum = sum_i (best_posterior + best_value_i): the summation of kg_sum_kernel, bit for bit
      const double bp = P.blob[(long)e * P.rec.stride + P.rec_bp];
      double acc = 0.0;
  #pragma unroll 8
      for (int i = threadIdx.x; i < P.num_local; i += 256) acc += bp + P.best_value[(long)e * P.num_local + i];
      const double tot = block_sum_256(acc, red);
      if (threadIdx.x == 0) out[0] = tot;
    }
  }
};
__global__ __launch_bounds__(256) void kg_zc_sum_kernel(KgTailParams P, const double* __restrict__ part, int chunks, int gs) {
  kg_zc_sum_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, part, chunks, gs);
}

// DIR[e][(k (1+g) + b) d + dd] = sum_i beta_i[(k,b)] * d cov(Xu_k, x*_i)[b, 0] / d Xu_k,dd ; workgroup (k, e).
template <int DP>
struct kg_dir_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, double* __restrict__ part, int slices) {
    __shared__ double red[4];
    const int k = blockIdx.x, e = blockIdx.y, sl = blockIdx.z;
    // the samples are cut into `slices` contiguous ranges (grid.z) so that q x E workgroups become q x E x slices -- at C5
    // eight workgroups walked 20 000 samples each while 248 CUs idled; kg_dir_sum_kernel adds the partials in slice order
    const int per = (P.num_local + slices - 1) / slices;
    const int i_lo = sl * per, i_hi = min(P.num_local, i_lo + per);
    const int m = P.m, g1 = 1 + P.g, d = P.cp.dim;
    const double* Xu = P.blob + (long)e * P.rec.stride + P.rec.XuP + (long)k * DP;
    DerivList none;
    none.g = 0;
    double xk[DP];
  #pragma unroll
    for (int kk = 0; kk < DP; ++kk) xk[kk] = Xu[kk];
    for (int b = 0; b < g1; ++b) {
      double acc[DP];
  #pragma unroll
      for (int dd = 0; dd < DP; ++dd) acc[dd] = 0.0;
      for (int i = i_lo + threadIdx.x; i < i_hi; i += 256) {
        const long w = (long)e * P.num_local + i;
        const double* xs = P.best_point + w * DP;
        double diff[DP];
        double r2 = 0.0;
  #pragma unroll
        for (int kk = 0; kk < DP; ++kk) {
          diff[kk] = xk[kk] - xs[kk];
          r2 = fma(diff[kk] * diff[kk], P.cp.inv_l2[kk], r2);
        }
        const Radial rd = radial_scalars(P.cp.type, P.cp.alpha, r2);
        const double bt = P.beta[w * m + k * g1 + b];
  #pragma unroll
        for (int dd = 0; dd < DP; ++dd)
          if (dd < d) acc[dd] = fma(bt, grad_cov_entry<DP>(P.cp, rd, diff, b, 0, dd, P.derivs, none), acc[dd]);
      }
  #pragma unroll
      for (int dd = 0; dd < DP; ++dd) {
        if (dd < d) {  // d is workgroup-uniform
          const double tot = block_sum_256(acc[dd], red);
          if (threadIdx.x == 0) part[((long)e * P.ngrad + (k * g1 + b) * d + dd) * slices + sl] = tot;
        }
      }
    }
  }
};
template <int DP>
__global__ __launch_bounds__(256) void kg_dir_kernel(KgTailParams P, double* __restrict__ part, int slices) {
  kg_dir_kernel_body<DP>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, part, slices);
}

// (T-free tail, S_W-free form) the KB chunk partials [E][chunks][m][m] behind the DIR partials (the host reserves E chunks m m doubles more)
__host__ __device__ inline double* kb_partials(const KgTailParams& P) {
  return P.TBpart + (long)P.E * (P.chunks + 1) * (long)P.m * P.N + (long)P.E * P.ngrad * kDirSlices;
}

template <int DP>
void launch_dir(const KgTailParams& P, hipStream_t s) {
  const int slices = dir_slices(P.num_local);
  launch_kernel_ens<kg_dir_kernel_body<DP>, 256>(kg_dir_kernel<DP>, dim3(P.q, P.E, slices), dim3(256), 0, s, P, dir_partials(P), slices);
}

template <int DP, int MU>
void launch_sw_inst(const KgTailParams& P, hipStream_t s) {
  dim3 grid((P.num_local + P.sw_chunk - 1) / P.sw_chunk, P.E);
  const size_t shm = (P.SW == nullptr) ? sizeof(double) * (size_t)P.N * P.m : 0;
  launch_kernel_ens<kg_sw_kernel_body<DP, MU>, 256>(kg_sw_kernel<DP, MU>, grid, dim3(256), shm, s, P);
}

// f(std::integral_constant<int, MU>{}) for the smallest MU of 4, 8, 16, 32, 64 that holds m columns; false, f not called, for m > 64
template <class F>
bool dispatch_mu(int m, F&& f) {
  if (m <= 4)
    f(std::integral_constant<int, 4>{});
  else if (m <= 8)
    f(std::integral_constant<int, 8>{});
  else if (m <= 16)
    f(std::integral_constant<int, 16>{});
  else if (m <= 32)
    f(std::integral_constant<int, 32>{});
  else if (m <= 64)
    f(std::integral_constant<int, 64>{});
  else
    return false;
  return true;
}

template <int DP>
void launch_sw_dp(const KgTailParams& P, hipStream_t s) {
  if (!dispatch_mu(P.m, [&](auto MU) { launch_sw_inst<DP, decltype(MU)::value>(P, s); })) {
    // two components per lane; S_W comes precomputed (the host always forms it by GEMM for m > 8)
    if (P.SW == nullptr) throw Error(MOE_ERR_RUNTIME, "m > 64 needs the precomputed W^T T");
    dim3 grid((P.num_local + P.sw_chunk - 1) / P.sw_chunk, P.E);
    launch_kernel_ens<kg_sw_kernel_body<DP, 1, 2>, 256>(kg_sw_kernel<DP, 1, 2>, grid, dim3(256), 0, s, P);
  }
  launch_dir<DP>(P, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused tail for q-KG (no derivative observations, m = q + p <= 8): the N x M matrix T = K(X, x*_i) is never written.
// Its entries are recomputed where they are consumed -- once with a thread per SAMPLE (S_W = W^T T_i, then c_i), once with a
// thread per training POINT (TB partials) -- which costs ~2 x 46 FP64 instructions per entry against 16 B written + 24 B
// re-read per entry through HBM: at C3 the covariance build + S_W + TB kernels took 86 us per evaluation, these two take
// about half.  Operands that are uniform over the workgroup (the point tile in the first kernel, the sample chunk in the
// second) are staged in LDS pre-scaled by 1/length and read as broadcasts.
// By default only the second of the two runs (the S_W-free form further down: ZC from the chunk sums, no per-sample quantity);
// MOE_KG_FUSED_ONE_PASS=0 keeps both, with kg_fused_c_kernel and the ZC chunk partials behind them, as the comparator of the tests.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kFusedTile = 256;  // points (kernel A) / samples (kernel B, at most: KgTailParams::chunk_len) staged per LDS tile

template <int COV>
__device__ __forceinline__ double radial_base(double r2, const double* __restrict__ etab) {
  if (COV == MOE_COV_SQUARE_EXPONENTIAL) return exp_nonpos_tab(fmax(-0.5 * r2, -1000.0), etab);  // (table exp range)
  const double a = 2.236067977499789696409173668731276235 * sqrt_pos(r2);
  return exp_nonpos_tab(-a, etab) * fma(a, fma(a, 1.0 / 3.0, 1.0), 1.0);
}

// thread = sample, blockIdx.z = slice of the training points: SWpart[e][i][slice][c] = sum over the slice of W[j, c] k(X_j, x*_i)
// (the slices only exist to give the chip enough wavefronts: E * M / 64 alone is ~1 per SIMD at the headline shape)
template <int DP, int MU, int COV>
struct kg_fused_sample_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, const double* __restrict__ X, int n, double* __restrict__ SWpart) {
    __shared__ double etab[kExpTabLen];
    __shared__ double Xt[kFusedTile][DP];
    __shared__ double Wt[kFusedTile][MU];
    const int e = blockIdx.y, m = P.m, N = P.N;
    const int slices = gridDim.z, slice = blockIdx.z;
    const int per = ((n + slices - 1) / slices + 63) / 64 * 64;
    const int j_lo = slice * per, j_hi = min(n, j_lo + per);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool ok = i < P.num_local;
    const long w = (long)e * P.num_local + (ok ? i : 0);
    if (threadIdx.x < kExpTabLen) etab[threadIdx.x] = kExp2Tab64[threadIdx.x];
    double xs[DP], acc[MU];
  #pragma unroll
    for (int k = 0; k < DP; ++k) xs[k] = P.best_point[w * DP + k] * P.cp.inv_l[k];
  #pragma unroll
    for (int c = 0; c < MU; ++c) acc[c] = 0.0;
    const double* We = P.W + (long)e * P.w_stride;
    for (int j0 = j_lo; j0 < j_hi; j0 += kFusedTile) {
      __syncthreads();
      for (int t = threadIdx.x; t < kFusedTile * DP; t += 256) {
        const int jj = t / DP, k = t % DP;
        Xt[jj][k] = (j0 + jj < j_hi) ? X[(long)(j0 + jj) * DP + k] * P.cp.inv_l[k] : 0.0;
      }
      for (int t = threadIdx.x; t < kFusedTile * MU; t += 256) {
        const int jj = t % kFusedTile, c = t / kFusedTile;  // W_e is [N x m] col-major: consecutive jj are contiguous
        Wt[jj][c] = (j0 + jj < j_hi && c < m) ? We[(long)c * N + j0 + jj] : 0.0;  // zero weight: padded points drop out
      }
      __syncthreads();
      const int cnt = min(kFusedTile, j_hi - j0);
  #pragma unroll 2
      for (int jj = 0; jj < cnt; ++jj) {
        double r2 = 1.0e-300;
  #pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double dlt = Xt[jj][k] - xs[k];
          r2 = fma(dlt, dlt, r2);
        }
        const double t = radial_base<COV>(r2, etab);
  #pragma unroll
        for (int c = 0; c < MU; ++c) acc[c] = fma(Wt[jj][c], t, acc[c]);
      }
    }
    if (!ok) return;
  #pragma unroll
    for (int c = 0; c < MU; ++c) SWpart[(w * slices + slice) * MU + c] = acc[c];
  }
};
template <int DP, int MU, int COV>
__global__ __launch_bounds__(256) void kg_fused_sample_kernel(KgTailParams P, const double* __restrict__ X, int n,
                                                             double* __restrict__ SWpart) {
  kg_fused_sample_kernel_body<DP, MU, COV>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, X, n, SWpart);
}

// thread = sample: S_W = sum of the slices (fixed order); R_r = alpha (k(Xu_r, x*_i) - S_W[r]); c_i = L^-1 R by forward
// substitution (L is m x m, column-major, workgroup-uniform)
template <int DP, int MU, int COV>
struct kg_fused_c_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, const double* __restrict__ SWpart, int slices) {
    __shared__ double etab[kExpTabLen];
    const int e = blockIdx.y, m = P.m;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < kExpTabLen) etab[threadIdx.x] = kExp2Tab64[threadIdx.x];
    __syncthreads();
    if (i >= P.num_local) return;
    const long w = (long)e * P.num_local + i;
    double xs[DP], sw[MU], cv[MU];
  #pragma unroll
    for (int k = 0; k < DP; ++k) xs[k] = P.best_point[w * DP + k] * P.cp.inv_l[k];
  #pragma unroll
    for (int c = 0; c < MU; ++c) {
      sw[c] = 0.0;
      for (int sl = 0; sl < slices; ++sl) sw[c] += SWpart[(w * slices + sl) * MU + c];
    }
    const double* rec = P.blob + (long)e * P.rec.stride;
    const double* Lsm = rec + P.rec.L;
  #pragma unroll
    for (int r = 0; r < MU; ++r) {
      cv[r] = 0.0;
      if (r < m) {
        const double* Xu = rec + P.rec.XuP + (long)r * DP;
        double r2 = 1.0e-300;
  #pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double dlt = Xu[k] * P.cp.inv_l[k] - xs[k];
          r2 = fma(dlt, dlt, r2);
        }
        double R = P.cp.alpha * (radial_base<COV>(r2, etab) - sw[r]);
  #pragma unroll
        for (int c = 0; c < MU; ++c)
          if (c < r) R -= Lsm[r + c * m] * cv[c];
        cv[r] = R / Lsm[r + r * m];
        P.C[w * m + r] = cv[r];
      }
    }
  }
};
template <int DP, int MU, int COV>
__global__ __launch_bounds__(256) void kg_fused_c_kernel(KgTailParams P, const double* __restrict__ SWpart, int slices) {
  kg_fused_c_kernel_body<DP, MU, COV>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, SWpart, slices);
}

// thread = training point: TBpart[e][chunk][c][row] = sum over the chunk's samples of K(X_row, x*_i) beta_i[c]
// kb_rows > 0 (the S_W-free form below; kb_rows = m): the evaluation's union points follow the training points as rows n .. n + m - 1
// of the same launch -- the same contraction at Xu_r, KBpart[e][chunk][c][r] = alpha sum_i beta_i[c] k(Xu_r, x*_i), through the same
// radial_base on the same scaled differences as kg_fused_c_kernel's k(Xu_r, x*_i).  A training point's sums do not depend on kb_rows.
template <int DP, int MU, int COV>
struct kg_fused_point_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, const double* __restrict__ X, int n, int kb_rows) {
    __shared__ double etab[kExpTabLen];
    __shared__ double St[kFusedTile][DP];
    __shared__ double Bt[kFusedTile][MU];
    const int row = blockIdx.x * 256 + threadIdx.x;
    const int chunk = blockIdx.y, e = blockIdx.z;
    const int m = P.m;
    const int i0 = chunk * P.chunk_len, cnt = min(P.num_local - i0, P.chunk_len);  // (chunk_len <= kFusedTile)
    if (threadIdx.x < kExpTabLen) etab[threadIdx.x] = kExp2Tab64[threadIdx.x];
    for (int t = threadIdx.x; t < kFusedTile * DP; t += 256) {
      const int ii = t / DP, k = t % DP;
      St[ii][k] = (ii < cnt) ? P.best_point[((long)e * P.num_local + i0 + ii) * DP + k] * P.cp.inv_l[k] : 0.0;
    }
    for (int t = threadIdx.x; t < kFusedTile * MU; t += 256) {
      const int ii = t / MU, c = t % MU;
      Bt[ii][c] = (ii < cnt && c < m) ? P.beta[((long)e * P.num_local + i0 + ii) * m + c] : 0.0;
    }
    __syncthreads();
    if (row >= n + kb_rows) return;  // (no barrier below)
    const bool ok = row < n;
    const double* __restrict__ xp = ok ? X + (long)row * DP : P.blob + (long)e * P.rec.stride + P.rec.XuP + (long)(row - n) * DP;
    double xr[DP], acc[MU];
  #pragma unroll
    for (int k = 0; k < DP; ++k) xr[k] = xp[k] * P.cp.inv_l[k];
  #pragma unroll
    for (int c = 0; c < MU; ++c) acc[c] = 0.0;
  #pragma unroll 2
    for (int ii = 0; ii < cnt; ++ii) {
      double r2 = 1.0e-300;
  #pragma unroll
      for (int k = 0; k < DP; ++k) {
        const double dlt = xr[k] - St[ii][k];
        r2 = fma(dlt, dlt, r2);
      }
      const double t = radial_base<COV>(r2, etab);
  #pragma unroll
      for (int c = 0; c < MU; ++c) acc[c] = fma(t, Bt[ii][c], acc[c]);
    }
    if (ok) {
      double* dst = P.TBpart + ((long)e * P.chunks + chunk) * m * P.N;
  #pragma unroll
      for (int c = 0; c < MU; ++c)
        if (c < m) dst[(long)c * P.N + row] = P.cp.alpha * acc[c];
    } else {
      double* dst = kb_partials(P) + ((long)e * P.chunks + chunk) * m * m;
  #pragma unroll
      for (int c = 0; c < MU; ++c)
        if (c < m) dst[c * m + (row - n)] = P.cp.alpha * acc[c];
    }
  }
};
template <int DP, int MU, int COV>
__global__ __launch_bounds__(256) void kg_fused_point_kernel(KgTailParams P, const double* __restrict__ X, int n, int kb_rows) {
  kg_fused_point_kernel_body<DP, MU, COV>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, X, n, kb_rows);
}

// The S_W-free form of the T-free tail (the default: MOE_KG_FUSED_ONE_PASS=1; every shape of the T-free path).  S_W,i = W^T T_i is
// only ever used in c_i = L^-1 alpha (k(Xu, x*_i) - S_W,i), and c_i only in ZC = sum_i z_i c_i^T.  With z_i = L^T beta_i (the MC
// kernel's own beta_i = L^-T z_i) the sum over the samples moves inside:
//     ZC = L^T ( KB - TB^T W ) L^-T,    KB[c][r] = alpha sum_i beta_i[c] k(Xu_r, x*_i),    TB = the alpha-scaled sum GTB already uses,
// so the second contraction of T (kg_fused_sample_kernel, or the one-pass kg_fused_pair_kernel that held both sets of partial sums
// in registers and was LDS-bound at low occupancy: 1.71 ms per 64 C3 evaluations against kg_fused_point_kernel's 0.89) and every
// per-sample quantity of the tail (S_W, c_i, the ZC chunk partials) drop out: KB is the TB contraction at m more rows of the point
// kernel, TB^T W is m m dot products of length N per evaluation.  The gradient changes by rounding only; where the posterior
// covariance between Xu and x* is far below the prior one the subtraction happens after the sum over the samples instead of inside
// every sample (tests/test_gpu_sw_free_tail.py bounds that case against the CPU oracle).
// One workgroup per evaluation: thread = row (stride 256) with all m x m products in registers, a fixed butterfly per wavefront and
// the four wavefronts added as (0 + 1) + (2 + 3); the KB chunk partials by groups of m m lanes striding the chunks, the groups added
// in order.  Every order is a function of (N, m, num_local) alone.  Then A = L^T B and ZC = A L^-T by substitution along each row.
template <int MU>
struct kg_zc_direct_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, const double* __restrict__ TBsum) {
    __shared__ double red[4][MU * MU], kbs[256], Bs[MU * MU], As[MU * MU];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = P.m, N = P.N, mm = m * m;
    const double* __restrict__ tb = TBsum + (long)e * m * N;
    const double* __restrict__ We = P.W + (long)e * P.w_stride;
    double acc[MU][MU];
  #pragma unroll
    for (int c = 0; c < MU; ++c)
  #pragma unroll
      for (int r = 0; r < MU; ++r) acc[c][r] = 0.0;
  #pragma unroll 2
    for (int row = tid; row < N; row += 256) {
      double t[MU], w[MU];
  #pragma unroll
      for (int c = 0; c < MU; ++c) {  // (m is uniform; columns beyond it feed sums that are never read)
        t[c] = (c < m) ? tb[(long)c * N + row] : 0.0;
        w[c] = (c < m) ? We[(long)c * N + row] : 0.0;
      }
  #pragma unroll
      for (int c = 0; c < MU; ++c)
  #pragma unroll
        for (int r = 0; r < MU; ++r) acc[c][r] = fma(t[c], w[r], acc[c][r]);
    }
  #pragma unroll
    for (int c = 0; c < MU; ++c)
  #pragma unroll
      for (int r = 0; r < MU; ++r) {
        const double v = wave_sum64(acc[c][r]);
        if (lane == 0) red[wave][c * MU + r] = v;
      }
    {
      const int groups = 256 / mm;  // >= 4
      const int o = tid % mm, g = tid / mm;
      const double* __restrict__ kp = kb_partials(P) + (long)e * P.chunks * mm + o;
      double v = 0.0;
      if (g < groups) {
  #pragma unroll 4
        for (int ch = g; ch < P.chunks; ch += groups) v += kp[(long)ch * mm];
      }
      kbs[tid] = v;
    }
    __syncthreads();
    if (tid < mm) {
      const int groups = 256 / mm;
      const int c = tid / m, r = tid - c * m;
      double kb = 0.0;
      for (int g = 0; g < groups; ++g) kb += kbs[g * mm + tid];
      const int o = c * MU + r;
      Bs[tid] = kb - ((red[0][o] + red[1][o]) + (red[2][o] + red[3][o]));
    }
    __syncthreads();
    const double* Lsm = P.blob + (long)e * P.rec.stride + P.rec.L;  // m x m, column-major, lower
    if (tid < mm) {  // A[a][r] = sum_{c >= a} L[c][a] B[c][r]
      const int a = tid / m, r = tid - a * m;
      double v = 0.0;
      for (int c = a; c < m; ++c) v = fma(Lsm[c + a * m], Bs[c * m + r], v);
      As[tid] = v;
    }
    __syncthreads();
    if (tid < m) {  // row tid of ZC L^T = A, ascending columns
      double* out = P.out + (long)e * P.out_stride + 1;
      double zc[MU];
  #pragma unroll
      for (int j = 0; j < MU; ++j) {
        zc[j] = 0.0;
        if (j < m) {
          double v = As[tid * m + j];
  #pragma unroll
          for (int k = 0; k < MU; ++k)
            if (k < j) v = fma(-zc[k], Lsm[j + k * m], v);
          zc[j] = v / Lsm[j + j * m];
          out[tid + j * m] = zc[j];
        }
      }
    }
  }
};
template <int MU>
__global__ __launch_bounds__(256) void kg_zc_direct_kernel(KgTailParams P, const double* __restrict__ TBsum) {
  kg_zc_direct_kernel_body<MU>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, TBsum);
}

template <int DP, int MU, int COV>
void launch_fused_tail_cov(const KgTailParams& P, const double* X, int n, double* SWpart, int slices, hipStream_t s) {
  if (fused_tail_sw_free()) {
    dim3 gb((n + P.m + 255) / 256, P.chunks, P.E);  // (the m union rows behind the training points)
    launch_kernel_ens<kg_fused_point_kernel_body<DP, MU, COV>, 256>(kg_fused_point_kernel<DP, MU, COV>, gb, dim3(256), 0, s, P, X, n, P.m);
    launch_dir<DP>(P, s);
    launch_gtb(P, s);
    const double* TBsum = P.TBpart + (long)P.E * P.chunks * (long)P.m * P.N;  // (launch_gtb)
    launch_kernel_ens<kg_zc_direct_kernel_body<MU>, 256>(kg_zc_direct_kernel<MU>, dim3(P.E), dim3(256), 0, s, P, TBsum);
    MOE_HIP_CHECK(hipGetLastError());
    return;
  }
  dim3 ga((P.num_local + 255) / 256, P.E, slices), gc((P.num_local + 255) / 256, P.E), gb((n + 255) / 256, P.chunks, P.E);
  launch_kernel_ens<kg_fused_sample_kernel_body<DP, MU, COV>, 256>(kg_fused_sample_kernel<DP, MU, COV>, ga, dim3(256), 0, s, P, X, n, SWpart);
  launch_kernel_ens<kg_fused_c_kernel_body<DP, MU, COV>, 256>(kg_fused_c_kernel<DP, MU, COV>, gc, dim3(256), 0, s, P, SWpart, slices);
  launch_dir<DP>(P, s);
  launch_kernel_ens<kg_fused_point_kernel_body<DP, MU, COV>, 256>(kg_fused_point_kernel<DP, MU, COV>, gb, dim3(256), 0, s, P, X, n, 0);
  launch_gtb(P, s);
  MOE_HIP_CHECK(hipGetLastError());
}

template <int DP, int MU>
void launch_fused_tail_inst(const KgTailParams& P, const double* X, int n, double* SWpart, int slices, hipStream_t s) {
  if (P.cp.type == MOE_COV_SQUARE_EXPONENTIAL)
    launch_fused_tail_cov<DP, MU, MOE_COV_SQUARE_EXPONENTIAL>(P, X, n, SWpart, slices, s);
  else
    launch_fused_tail_cov<DP, MU, MOE_COV_MATERN_NU_2P5>(P, X, n, SWpart, slices, s);
}

// value-only finish: kg_sum per evaluation (same summation as block 0 of kg_zc_sum_kernel)
struct kg_sum_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgTailParams& P, double* __restrict__ fin, const unsigned long long* __restrict__ counters, const int* __restrict__ flags) {
    __shared__ double red[4];
    const int e = blockIdx.x;
    const double bp = P.blob[(long)e * P.rec.stride + P.rec_bp];
    double acc = 0.0;
    for (int i = threadIdx.x; i < P.num_local; i += 256) acc += bp + P.best_value[(long)e * P.num_local + i];
    const double tot = block_sum_256(acc, red);
    if (threadIdx.x == 0) {  // the record the host reads back: kg_sum | value passes | gradient passes | singular flag
      fin[4 * e] = tot;
      fin[4 * e + 1] = (double)counters[2 * e];
      fin[4 * e + 2] = (double)counters[2 * e + 1];
      fin[4 * e + 3] = (double)flags[e];
    }
  }
};
__global__ __launch_bounds__(256) void kg_sum_kernel(KgTailParams P, double* __restrict__ fin, const unsigned long long* __restrict__ counters,
                                                     const int* __restrict__ flags) {
  kg_sum_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, fin, counters, flags);
}

}  // namespace

void launch_tail(const KgTailParams& P, hipStream_t s) {
  dispatch_dp(P.cp.dp, [&](auto DP) { launch_sw_dp<decltype(DP)::value>(P, s); });
  dim3 gtb((P.N + 255) / 256, P.chunks, P.E);
  if (!dispatch_mu(P.m, [&](auto MU) {
        constexpr int kMu = decltype(MU)::value;
        launch_kernel_ens<kg_tb_kernel_body<kMu>, 256>(kg_tb_kernel<kMu>, gtb, dim3(256), 0, s, P, 0);
      }))  // (m <= kMaxMB = 128: one column tile)
    launch_kernel_ens<kg_tb128_kernel_body, 256, 2>(kg_tb128_kernel, dim3((P.N + g128::TM - 1) / g128::TM, P.chunks, P.E), dim3(256), g128::kSmemBytes, s, P);
  launch_gtb(P, s);
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_sw128(const KgTailParams& P, double* SWpart, int slices, double* SW, hipStream_t s) {
  launch_kernel_ens<kg_sw128_kernel_body, 256, 2>(kg_sw128_kernel, dim3((P.num_local + g128::TM - 1) / g128::TM, slices, P.E), dim3(256), g128::kSmemBytes, s, P,
                                                  SWpart, slices);
  launch_sum_slices(SWpart, slices, (long)P.m * P.num_local * P.E, SW, s);
}

// number of point slices of kg_fused_sample_kernel: enough wavefronts for ~4 per SIMD when ONE evaluation runs alone.  It does not
// depend on the batch size: the slices are summed in order, so an evaluation's bits would otherwise change with its batch.
int fused_tail_slices(int /*E*/, int num_local, int n, int num_cu) {
  const long waves = (long)((num_local + 255) / 256) * 4;
  const long want = (long)num_cu * 4 * 4;
  int s = (int)std::min<long>(8, std::max<long>(1, (want + waves - 1) / waves));
  return std::max(1, std::min(s, (n + 63) / 64));
}

// (chunk_len <= kFusedTile)
void launch_fused_tail(const KgTailParams& P, const double* X, int n, double* SWpart, int slices, hipStream_t s) {
  static_assert(kFusedChunk <= kFusedTile, "a chunk of samples is staged in one LDS tile");
  dispatch_dp(P.cp.dp, [&](auto DP) {
    if (P.m <= 4)
      launch_fused_tail_inst<decltype(DP)::value, 4>(P, X, n, SWpart, slices, s);
    else
      launch_fused_tail_inst<decltype(DP)::value, 8>(P, X, n, SWpart, slices, s);
  });
}

void launch_zc(const KgTailParams& P, double* part, hipStream_t s, bool sum_here) {
  const int len = zc_chunk_len(P.m);
  const int chunks = (P.num_local + len - 1) / len;
  const size_t shm = sizeof(double) * 2 * len * P.m;
  launch_kernel_ens<kg_zc_part_kernel_body, 256>(kg_zc_part_kernel, dim3(chunks, P.E), dim3(256), shm, s, P, part, chunks, len);
  if (!sum_here) return;
  const int gs = zc_sum_lanes(P.m);
  const int per_block = 256 / gs;
  launch_kernel_ens<kg_zc_sum_kernel_body, 256>(kg_zc_sum_kernel, dim3((P.m * P.m + per_block - 1) / per_block, P.E), dim3(256), 0, s, P, (const double*)part, chunks, gs);
}

void launch_kg_sum(const KgTailParams& P, double* fin, const unsigned long long* counters, const int* flags, hipStream_t s) {
  launch_kernel_ens<kg_sum_kernel_body, 256>(kg_sum_kernel, dim3(P.E), dim3(256), 0, s, P, fin, counters, flags);
}

}  // namespace moe
