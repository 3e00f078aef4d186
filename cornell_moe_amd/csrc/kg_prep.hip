// cornell_moe_amd/csrc/kg_prep.hip -- what runs around the MC kernel of a q-KG / d-KG evaluation on gfx950, per evaluation and per
// sample: the coordinate tables, the start table of the line searches, the sample pre-pass and the per-sample weight table
// (kg_prep.hpp; the driver is kg.hip).  They share the MC kernels' device functions (kg_mc.hpp), hence their bits.
#include "kg_prep.hpp"

#include <algorithm>

#include "fastmath.hpp"
#include "gemm128.hpp"

namespace moe {

namespace {

// XsTab[e][tile][r][lane] = coordinate perm[r] of point (tile*64 + lane) of evaluation e, minus the training-set mean of that
// coordinate, divided by its length scale (centred first: the difference of two nearby numbers is exact, so the scaled
// coordinates carry the precision of the distances however far from the origin the domain sits):
// the n training points, then the u union points of that evaluation, zero beyond.
// (r5: the workgroups of evaluation 0 also clear the call's counter block -- pass counters, sample tickets -- which a memset did before)
struct build_xs_tab_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const double* __restrict__ X, int n, const double* __restrict__ XuAll, int u, int dp, int ntiles, const TabParams& tp, double* __restrict__ tab, long tab_stride, int pair_rows, unsigned long long* __restrict__ ctr, long n_ctr) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = blockIdx.y;
    if (e == 0)
      for (long i = idx; i < n_ctr; i += (long)gridDim.x * blockDim.x) ctr[i] = 0ull;
    if (idx >= ntiles * dp * 64) return;
    const int l = idx & 63, r = (idx >> 6) % dp, t = (idx >> 6) / dp;
    const int j = t * 64 + l;
    const int k = tp.perm[r];
    double v = tp.center[r];  // padded points sit at the centre (zero weight; a far-away pad would only stress the exp)
    if (j < n)
      v = X[(long)j * dp + k];
    else if (j < n + u)
      v = XuAll[((long)e * u + (j - n)) * dp + k];
    // (pair_rows: the rows of a point in pairs, [tile][dp / 2][64][2] -- one 16-byte load per lane and pair, kg_mc_lds.hpp WideEval)
    const long out = pair_rows ? (((long)t * (dp / 2) + (r >> 1)) * 64 + l) * 2 + (r & 1) : idx;
    tab[(long)e * tab_stride + out] = (v - tp.center[r]) * tp.inv_lp[r];
  }
};
__global__ __launch_bounds__(256) void build_xs_tab_kernel(const double* __restrict__ X, int n, const double* __restrict__ XuAll, int u, int dp,
                                    int ntiles, TabParams tp, double* __restrict__ tab, long tab_stride, int pair_rows,
                                    unsigned long long* __restrict__ ctr, long n_ctr) {
  build_xs_tab_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, X, n, XuAll, u, dp, ntiles, tp, tab, tab_stride, pair_rows, ctr, n_ctr);
}

// z, beta = L^-T z and the discretised-set winner of EVERY sample (they depend on the normal draws alone): one wavefront
// per sample, grid-stride, the same device functions the MC kernels use -- so the values are the ones they would compute.
struct kg_sample_prep_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P, int* __restrict__ best_j) {
    __shared__ double zbs[4][2 * kMaxM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* zb = zbs[wave];
    const long total = (long)P.E * P.num_local;
    for (long idx = (long)blockIdx.x * 4 + wave; idx < total; idx += (long)gridDim.x * 4) {
      const int e = (int)(idx / P.num_local), sl = (int)(idx % P.num_local);
      const double* rec = P.blob + (long)e * P.rec.stride;
      double zc, bc;
      mc::draw_z_beta(P, rec + P.rec.L, P.first_sample + sl, lane, zb, zc, bc);
      const int bj = mc::discrete_scan(P, rec, zb, lane);
      if (lane < P.m) P.beta[idx * P.m + lane] = bc;
      if (lane == 0) best_j[idx] = bj;
      __builtin_amdgcn_wave_barrier();
    }
  }
};
__global__ __launch_bounds__(256) void kg_sample_prep_kernel(KgMcParams P, int* __restrict__ best_j) {
  kg_sample_prep_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, best_j);
}

// The same for m > 64 (more components than lanes): one THREAD per sample, serial O(m^2) back substitution and O(A m) scan
// against operands in L2 -- a few hundred microseconds for 2 x 10^4 samples at m = 104; only the workgroup-per-sample kernel
// consumes it.  z_i (antithetic pairs, .cpp:171-180), beta_i = L^-T z_i, first best discretised point (.cpp:436-449).
struct kg_sample_prep_generic_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P, int* __restrict__ best_j) {
    const long idx = (long)blockIdx.x * 64 + threadIdx.x;
    const long total = (long)P.E * P.num_local;
    if (idx >= total) return;
    const int e = (int)(idx / P.num_local), sl = (int)(idx % P.num_local);
    const int m = P.m, s = P.first_sample + sl;
    const double* rec = P.blob + (long)e * P.rec.stride;
    const double* L = rec + P.rec.L;
    const double sign = (s & 1) ? -1.0 : 1.0;
    const double* zrow = P.normals + (long)(s >> 1) * m;
    double beta[kMaxMB];
    for (int r = m - 1; r >= 0; --r) {
      double acc = 0.0;
      for (int l = m - 1; l > r; --l) acc = fma(L[l + (long)r * m], beta[l], acc);
      beta[r] = (sign * zrow[r] - acc) / L[r + (long)r * m];
    }
    for (int c = 0; c < m; ++c) P.beta[idx * m + c] = beta[c];
    const double* mu_disc = rec + P.rec.mu_disc;
    const double* C_disc = rec + P.rec.C_disc;
    double best_f = -INFINITY;
    int bj = 0;
    for (int j = 0; j < P.A; ++j) {
      double v = mu_disc[j];
      for (int c = 0; c < m; ++c) v = fma(C_disc[(long)j * m + c], sign * zrow[c], v);
      if (-v > best_f) {  // strict: the first best point wins
        best_f = -v;
        bj = j;
      }
    }
    best_j[idx] = bj;
  }
};
__global__ __launch_bounds__(64) void kg_sample_prep_generic_kernel(KgMcParams P, int* __restrict__ best_j) {
  kg_sample_prep_generic_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, best_j);
}

// The START TABLE of an evaluation without derivative observations (mc::start_from_table, kg_mc.hpp): for every discretised point x_c
// -- where the line searches start -- the coefficients of [1 ; beta] in f = -mu_after(x_c) and in its frame gradient:
//   column 0:      -(mean + sum_j alpha KinvY_j b_j)              | -sum_j alpha KinvY_j b'_j (x_j - x_c)_k
//   column 1 + l:  -(alpha b_{n+l} - sum_j alpha W_jl b_j)        | the same with b' (x - x_c)_k
// (b, b' = radial3's base and first-derivative coefficient of |x_j - x_c|^2, j over the training points, n + l = fantasy point l): the
// sums of a value + gradient pass (grad_pass_parked) with the sample's weights alpha (KinvY - W beta | beta) taken apart by beta's
// components.  The kernel reads what the pass reads -- the frame table XsTab, KinvY, W -- through radial3, so an entry differs from
// the pass's sum by the order of additions alone.
// One WAVEFRONT per (discretised point, group of kStartCols<DP> columns, evaluation): every lane walks the tiles in order (one fma
// chain per sum), then the fixed butterfly -- the order depends on n + u and DP alone, never on the batch or the ensemble.  A group's
// columns share the radial terms, and at m <= 4 (q-KG up to four points; DP <= 8) one group is all there is.
template <int DP>
constexpr int kStartCols = DP <= 8 ? 5 : (DP <= 12 ? 3 : 2);

template <int DP, int COV>
__device__ __forceinline__ void start_table_sums(const KgMcParams& P, const double* __restrict__ xg, const double* __restrict__ We,
                                                 const double* __restrict__ etab, const double (&xq)[DP], int col0, int lane,
                                                 double* __restrict__ out) {
  constexpr int CG = kStartCols<DP>;
  const int n = P.n, u = P.u, m = P.m, ntiles = P.ntiles;
  double accf[CG], accg[CG][DP];
#pragma unroll
  for (int i = 0; i < CG; ++i) {
    accf[i] = 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) accg[i][k] = 0.0;
  }
  // column col0 + i reads W's column col0 + i - 1 (clamped: a column beyond m, or column 0 here, is masked below)
  long wcol[CG];
#pragma unroll
  for (int i = 0; i < CG; ++i) wcol[i] = (long)min(max(col0 + i - 1, 0), m - 1) * P.N;
  for (int t0 = 0; t0 < ntiles; t0 += 2) {
    // the loads of two tiles in one batch (clamped addresses: always valid)
    double cx[2][DP], wv[2][CG];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = min(t0 + h, ntiles - 1);
      const long row = min(t * 64 + lane, n - 1);
#pragma unroll
      for (int k = 0; k < DP; ++k) cx[h][k] = xg[((long)t * DP + k) * 64 + lane];
#pragma unroll
      for (int i = 0; i < CG; ++i) wv[h][i] = (col0 + i == 0) ? P.KinvY[row] : -We[row + wcol[i]];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = t0 + h;
      if (t < ntiles) {
        const int j = t * 64 + lane;
        double diff[DP];
        double r2 = 1.0e-300;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          diff[k] = cx[h][k] - xq[k];
          r2 = fma(diff[k], diff[k], r2);
        }
        double base, first, second;
        mc::radial3<COV, true, false>(r2, etab, base, first, second);
#pragma unroll
        for (int i = 0; i < CG; ++i) {
          const int col = col0 + i;
          double w = wv[h][i];
          if (j >= n) w = (col >= 1 && j - n == col - 1 && j < n + u) ? 1.0 : 0.0;  // fantasy point l carries beta_l; padding nothing
          if (col > m) w = 0.0;
          w *= P.alpha;
          accf[i] = fma(w, base, accf[i]);
          const double coef = w * first;
#pragma unroll
          for (int k = 0; k < DP; ++k) accg[i][k] = fma(coef, diff[k], accg[i][k]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CG; ++i) {
    const int col = col0 + i;
    const double f = mc::wave_sum_uniform(accf[i]);
    double v = -((col == 0 ? P.mean : 0.0) + f);  // entry DP: the value
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const double gk = mc::wave_sum_uniform(accg[i][k]);
      v = (lane == k) ? -gk : v;
    }
    if (col <= m && lane <= DP) out[(long)col * (DP + 1) + lane] = v;
  }
}

template <int DP>
struct kg_start_table_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P, double* __restrict__ tab) {
    __shared__ double etab[kExpTabLen];
    const int lane = threadIdx.x;
    const int c = blockIdx.x, col0 = blockIdx.y * kStartCols<DP>, e = blockIdx.z;
    const int size = P.dim - P.f;
    etab[lane] = kExp2Tab64[lane];  // (kExpTabLen == 64 == the workgroup)
    __syncthreads();
    const double* rec = P.blob + (long)e * P.rec.stride;
    // the discretised point in the frame, as the line searches enter it: its coordinates on the optimised rows, 1 on fidelity rows,
    // 0 on pads (.cpp:353-357)
    double xq[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const int pk = P.perm[k];
      const double xo = (pk < size) ? rec[P.rec.disc + c * size + min(pk, size - 1)] : ((pk < P.dim) ? 1.0 : 0.0);
      xq[k] = (xo - P.center[k]) * P.inv_lp[k];
    }
    const double* xg = P.XsTab + (long)e * P.tab_stride;
    const double* We = P.W + (long)e * P.w_stride;
    double* out = tab + (long)e * P.start_stride + (long)c * (1 + P.m) * (DP + 1);
    if (P.cov_type == MOE_COV_SQUARE_EXPONENTIAL)
      start_table_sums<DP, MOE_COV_SQUARE_EXPONENTIAL>(P, xg, We, etab, xq, col0, lane, out);
    else
      start_table_sums<DP, MOE_COV_MATERN_NU_2P5>(P, xg, We, etab, xq, col0, lane, out);
  }
};
template <int DP>
__global__ __launch_bounds__(64) void kg_start_table_kernel(KgMcParams P, double* __restrict__ tab) {
  kg_start_table_kernel_body<DP>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, tab);
}


// Per-sample weights of the training rows for every sample, V[(e, sl)][r] = scale_a (KinvY[r] - sum_c W_e[r, c] beta[(e, sl), c])
// (r = (j, a); scale_0 = alpha, scale_a = -alpha / l_{d_a}): what point_weights computes inside the MC kernel, same
// operation order, hence the same bits.  Inside the workgroup-per-sample kernel that computation reads all of W_e
// (N x m) per sample and CU through a few dozen loads in flight -- a sixth of the kernel at m = 16; here one thread keeps
// a row of W in registers, beta arrives through scalar loads, and the chip writes N x M doubles at streaming speed.
// m > 64 (r4): the columns go down in passes of 64 -- pass [c_lo, c_lo + MB) continues the fma chain from the partial sum the previous
// pass left in V (plain store), the last pass scales and streams the result out; one pass (first = last) is the code of m <= 64.
template <int MB>
struct kg_sample_weights_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P, double* __restrict__ V, int samples_per_block, int c_lo, int first, int last) {
    // table entry t = (point j, slot a) <-> row r = j (1 + g) + a of the N training rows / the m fantasy rows; slots beyond the GP's
    // 1 + g (r4: a streamed-weights instantiation with more derivative slots than observed derivatives) hold zeros
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int e = blockIdx.z;
    const int m = P.m, g1 = 1 + P.g;
    const int pj = t / P.v_slots1, pa = t - pj * P.v_slots1;
    const bool slot_ok = pa < g1;
    const int r = slot_ok ? pj * g1 + pa : P.N + m;  // (an unused slot: behind everything, stored as 0)
    const double* __restrict__ We = P.W + (long)e * P.w_stride;
    const double* __restrict__ beta = P.beta;
    double l[MB];
    const int rr = min(r, P.N - 1);
  #pragma unroll
    for (int c = 0; c < MB; ++c) {  // zero beyond m: the unconditional fma below then leaves v untouched
      const double t = We[rr + (long)min(c_lo + c, m - 1) * P.N];
      l[c] = (c_lo + c < m) ? t : 0.0;
    }
    const double kiy = P.KinvY[rr];
    const int a = rr % g1;
    const double scale = (a == 0) ? P.alpha : -P.alpha * P.inv_lp[a > 0 ? a - 1 : 0];
    const int s0 = blockIdx.y * samples_per_block, s1 = min(P.num_local, s0 + samples_per_block);
    // rows behind the training set (v_stride > N: the streamed-weights MC kernel reads whole tiles): the fantasy points' weights are the
    // sample's beta itself, scaled like a training row (kg_mc_wave.hpp kg_sample), then zeros up to the end of the last tile
    const int cf = r - P.N;
    const bool fantasy = cf >= 0 && cf < m;
    const double fscale = ((cf % g1) == 0) ? P.alpha : -P.alpha * P.inv_lp[max(cf % g1, 1) - 1];
    for (int sl = s0; sl < s1; ++sl) {
      const long so = (long)e * P.num_local + sl;
      const double* __restrict__ bs = beta + so * m + c_lo;
      double v = first ? kiy : V[so * P.v_stride + min(t, (int)P.v_stride - 1)];
  #pragma unroll
      for (int c = 0; c < MB; ++c) v = fma(-l[c], bs[c], v);  // uniform, contiguous: wide scalar loads (reads up to MB - m
                                                              // doubles past the row: next rows / the zeroed pad, times l = 0)
      if (t >= P.v_stride) continue;
      if (r < P.N) {
        if (last)
          __builtin_nontemporal_store(v * scale, &V[so * P.v_stride + t]);  // (streaming: 1.28 GB at C5, read once by the MC kernel)
        else
          V[so * P.v_stride + t] = v;
      } else if (last) {
        V[so * P.v_stride + t] = fantasy ? beta[so * m + min(cf, m - 1)] * fscale : 0.0;
      }
    }
  }
};
template <int MB>
__global__ __launch_bounds__(256) void kg_sample_weights_kernel(KgMcParams P, double* __restrict__ V, int samples_per_block,
                                                               int c_lo = 0, int first = 1, int last = 1) {
  kg_sample_weights_kernel_body<MB>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, V, samples_per_block, c_lo, first, last);
}

// The same table for m > 64 (r4; the stretch point's m = 104) with its sums on the matrix pipe: V_e (table rows x samples) = K^-1 y -
// W_e beta_e^T through gemm128.hpp's tile core, scaled and written ONCE (the kernel above needs two passes over a partially written
// table there: 2 x 5.1 ms per evaluation against the MC kernel's own 9.4).  Needs the table's rows to BE the training rows
// (v_slots1 == 1 + g).  The sums are formed in the MFMA's order, not in the c-order of the in-kernel weights: for these shapes a result
// depends at rounding level on whether the table fitted its cap (the m <= 64 paths keep their bit-for-bit equality).
// Grid (row tiles of 128 table entries, column tiles of 128 samples, E).
struct kg_table128_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P, double* __restrict__ V) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int e = blockIdx.z, m = P.m, g1 = 1 + P.g;
    const long s0 = (long)e * P.num_local;
    g128::Operand A{P.W + (long)e * P.w_stride, (long)P.N, P.N, m, 1};   // W[t + c N]: table rows contiguous
    g128::Operand B{P.beta + s0 * m, (long)m, P.num_local, m, 1};        // beta[sample m + c]: K (= c) contiguous
    g128::f64x4 acc[4][4];
    const int t0 = blockIdx.x * g128::TM, j0 = blockIdx.y * g128::TM;
    if (t0 < P.N) g128::tile_product<false, true>(A, B, t0, j0, 0, m, smem, acc);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wi = (wave & 1) * 64, wj = (wave >> 1) * 64;
    const int lk = lane >> 4, lx = lane & 15;
  #pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int t = t0 + wi + 16 * a + lx;
      const int tt = min(t, P.N - 1);
      const double kiy = P.KinvY[tt];
      const int sa = tt % g1;
      const double scale = (sa == 0) ? P.alpha : -P.alpha * P.inv_lp[sa > 0 ? sa - 1 : 0];
      // rows behind the training set: the fantasy points' weights are the sample's beta itself, scaled like a training row, then zeros
      const int cf = t - P.N;
      const bool fantasy = cf >= 0 && cf < m;
      const double fscale = ((cf % g1) == 0) ? P.alpha : -P.alpha * P.inv_lp[max(cf % g1, 1) - 1];
  #pragma unroll
      for (int b = 0; b < 4; ++b)
  #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int smp = j0 + wj + 16 * b + lk + 4 * r;
          if (t < P.v_stride && smp < P.num_local) {
            const long so = s0 + smp;
            double v;
            if (t < P.N)
              v = (kiy - acc[a][b][r]) * scale;
            else
              v = fantasy ? P.beta[so * m + min(cf, m - 1)] * fscale : 0.0;
            __builtin_nontemporal_store(v, &V[so * P.v_stride + t]);
          }
        }
    }
  }
};
__global__ __launch_bounds__(256, 2) void kg_table128_kernel(KgMcParams P, double* __restrict__ V) {
  kg_table128_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, P, V);
}

}  // namespace

void launch_xs_tab(const double* X, int n, const double* XuAll, int u, int dp, int ntiles, const TabParams& tp, double* tab, long tab_stride,
                   int pair_rows, unsigned long long* ctr, long n_ctr, int E, hipStream_t s) {
  dim3 grid((unsigned)((tab_stride + 255) / 256), E);
  launch_kernel_ens<build_xs_tab_kernel_body, 256>(build_xs_tab_kernel, grid, dim3(256), 0, s, X, n, XuAll, u, dp, ntiles, tp, tab, tab_stride, pair_rows,
                                                   ctr, n_ctr);
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_start_table(const KgMcParams& P, int dp, double* tab, hipStream_t s) {
  dispatch_dp(dp, [&](auto DP) {
    constexpr int kDp = decltype(DP)::value;
    if constexpr (kDp <= 16) {
      const dim3 grid((unsigned)P.A, (unsigned)((1 + P.m + kStartCols<kDp> - 1) / kStartCols<kDp>), (unsigned)P.E);
      launch_kernel_ens<kg_start_table_kernel_body<kDp>, 64>(kg_start_table_kernel<kDp>, grid, dim3(64), 0, s, P, tab);
      MOE_HIP_CHECK(hipGetLastError());
    } else {
      throw Error(MOE_ERR_RUNTIME, "the start table is built for padded dimensions up to 16");
    }
  });
}

void launch_sample_prep(const KgMcParams& P, int* best_j, int num_cu, hipStream_t s) {
  const long total = (long)P.E * P.num_local;
  if (P.m > kMaxM) {  // more components than lanes: thread-per-sample pre-pass (mandatory there)
    launch_kernel_ens<kg_sample_prep_generic_kernel_body, 64>(kg_sample_prep_generic_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, P, best_j);
  } else {
    const int pb = (int)std::min<long>((total + 3) / 4, (long)num_cu * 8);
    launch_kernel_ens<kg_sample_prep_kernel_body, 256>(kg_sample_prep_kernel, dim3(pb), dim3(256), 0, s, P, best_j);
  }
  MOE_HIP_CHECK(hipGetLastError());
}

void launch_sample_weights(const KgMcParams& P, double* V, hipStream_t s, bool table_only) {
  // r6: `table_only` -- the consumer (the streamed-weights kernel) has no in-kernel form of the weights whose bits the table would have
  // to reproduce -- takes the matrix-pipe kernel from m = 16 on: per (row, sample) entry the fma version's loop is one dependent chain
  // of m fmas behind a scalar-load round trip and the previous store's acknowledgement (1.17 ms per 2.56 GB at C5 = 2.2 TB/s)
  const bool mfma = P.v_slots1 == 1 + P.g && (P.m > 64 || (table_only && P.m >= 16));
  if (mfma) {
    launch_kernel_ens<kg_table128_kernel_body, 256, 2>(kg_table128_kernel, dim3((unsigned)((P.v_stride + g128::TM - 1) / g128::TM), (P.num_local + g128::TM - 1) / g128::TM, P.E),
                       dim3(256), g128::kSmemBytes, s, P, V);
    MOE_HIP_CHECK(hipGetLastError());
    return;
  }
  const int spb = 64;
  dim3 grid((unsigned)((P.v_stride + 255) / 256), (P.num_local + spb - 1) / spb, P.E);
  if (P.m <= 16)
    launch_kernel_ens<kg_sample_weights_kernel_body<16>, 256>(kg_sample_weights_kernel<16>, grid, dim3(256), 0, s, P, V, spb, 0, 1, 1);
  else if (P.m <= 32)
    launch_kernel_ens<kg_sample_weights_kernel_body<32>, 256>(kg_sample_weights_kernel<32>, grid, dim3(256), 0, s, P, V, spb, 0, 1, 1);
  else  // (m > 64 in passes of 64 columns; ONE pass with a 128-column row of W in registers -- 256 of them, half in the accumulation file --
        //  measured slower: 34 against 21 ms of MC phase per evaluation at the stretch point, m = 104)
    for (int c_lo = 0; c_lo < P.m; c_lo += 64)
      launch_kernel_ens<kg_sample_weights_kernel_body<64>, 256>(kg_sample_weights_kernel<64>, grid, dim3(256), 0, s, P, V, spb, c_lo, c_lo == 0 ? 1 : 0, c_lo + 64 >= P.m ? 1 : 0);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace moe
