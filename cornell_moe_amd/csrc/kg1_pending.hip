// cornell_moe_amd/csrc/kg1_pending.hip -- the discretised one-point knowledge gradient (kg1.hip) with pending points: the posterior
// COVARIANCE conditioned on p <= 64 points P whose experiments are running, the posterior MEAN left alone (the Kriging-believer
// fantasy of Ginsbourger et al. 2008: the believed values are mu_n(P), so K'^-1 (y' - mean) = [K^-1 (y - mean) ; 0]).
//
// The conditioned GP has the rows X' = X u P.  Its factor is never formed; with L the member's own,
//   L'^-1 = [[L^-1, 0], [-L_P^-1 V_P^T L^-1, L_P^-1]],   V_P = L^-1 k(X, P),   L_P L_P^T = k(P, P) + sigma^2 I - V_P^T V_P
// so the column of a point z under L'^-1 is the member's column with p rows under it,
//   v'_z = [v_z ; r_z],   r_z = L_P^-1 (k(P, z) - V_P^T v_z),   Sigma(z, x | P) = k(z, x) - v'_z . v'_x
// and kg1.hip's candidate, slope, envelope, t and gradient kernels run as they are on N + p rows of columns whose leading dimension
// keeps room for the pending rows: every slope stays ONE fused multiply-add chain, the member's rows in row order and then the
// pending rows in order, the same chain for a candidate's x^ and for the set, so the duplicate and tie rules hold bit for bit.
//
// The extension is kept column by column in V'_P [ld][pcap]: column j is v'_{P_j} = [L^-1 k(X, P_j) ; row j of L_P], its last entry
// the diagonal sqrt(k(P_j, P_j) + sigma^2 - |v'_{P_j}|^2) -- row j of L_P IS r_{P_j} over the rows before it, so appending a point
// is the row kernel on its own column plus the pivot (pivot rule: > 1e-16).  A greedy batch appends one column per round: one
// triangular product with one column, one row of L_P, one new row under the set's columns; nothing is rebuilt.
//   kg1_pending_rows_kernel   rows i0 .. i1 - 1 of r_z under the columns of the points z, one wavefront per column; with `append` the
//                             column is the pending point's own and gains its diagonal
//   kg1_pending_back_kernel   the pending block of L'^-T for the gradient's right-hand sides: u_P = L_P^-T t_P, t -= V_P u_P on the
//                             member's rows, which tri_cols('T') then takes through L^-T
//
// Members with g observed derivatives per point (ei1.hip; the knowledge gradient refuses them): a pending point is a block of
// g1 = 1 + g rows, its value and then its partial derivatives in the member's derivative order, extension row i = j g1 + a, with
// noise[a] on row a's diagonal (lcb.hip's rule).  Rows, pivots and the layout are as above row by row -- at most 64 extension ROWS --
// and only the covariance entries differ: kg1_pending_rows_g_kernel, entry i of a point z's column cov(P_j[a], z[0]), of a pending
// block's own column cov(P_j[a], P_j'[a']).  m.p, m.pcap and m.ld count rows; a member with g = 0 takes the kernels above.
#include <algorithm>
#include <climits>

#include "device_cov.hpp"
#include "gp.hpp"

namespace moe {

namespace {

constexpr double kPivotMin = 1.0e-16;  // gpp_linear_algebra.cpp:118

// One wavefront per column c of V (the point Z[c]): r_i = (k(P_i, z) - V'_P[0 .. N + i, i] . v'_z[0 .. N + i]) / L_P[i][i] for
// i = i0 .. i1 - 1 in order, lane m holding r_m; rows below i0 are read back from the column.  The dot product's partial sums go
// through a fixed butterfly, so a column's bits depend on nothing but the column.
struct kg1_pending_rows_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int ld, int i0, int i1, int ncols, int dp, const CovParams& cp, double noise, int append, const double* __restrict__ PP, const double* __restrict__ Z, const double* __restrict__ VP, double* __restrict__ V, int* __restrict__ fail) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    double* v = V + (size_t)c * ld;
    const double* z = Z + (size_t)c * dp;
    double rl = (lane < i0) ? v[N + lane] : 0.0;
    for (int i = i0; i < i1; ++i) {
      const double* vp = VP + (size_t)i * ld;
      double acc = 0.0;
      for (int r = lane; r < N; r += 64) acc = fma(vp[r], v[r], acc);
      if (lane < i) acc = fma(vp[N + lane], rl, acc);
  #pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      const PointDiff df{PP + (size_t)i * dp, z};
      const double ri = (pair_radial(cp, df, dp).base - acc) / vp[N + i];
      if (lane == i) rl = ri;
    }
    if (lane >= i0 && lane < i1) v[N + lane] = rl;
    if (append == 0) return;
    // the column is pending point i1's own (i0 = 0): its Schur pivot k(P, P) + sigma^2 - |v'_P|^2 and the diagonal of L_P
    double ss = 0.0;
    for (int r = lane; r < N; r += 64) ss = fma(v[r], v[r], ss);
    if (lane < i1) ss = fma(rl, rl, ss);
  #pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (lane != 0) return;
    const double pivot = (radial_scalars(cp.type, cp.alpha, 0.0).base - ss) + noise;
    v[N + i1] = sqrt(pivot);
    if (!(pivot > kPivotMin)) atomicMin(fail, i1);  // the first failing pending point of the call
  }
};
__global__ __launch_bounds__(256) void kg1_pending_rows_kernel(int N, int ld, int i0, int i1, int ncols, int dp, const CovParams cp, double noise, int append, const double* __restrict__ PP, const double* __restrict__ Z, const double* __restrict__ VP, double* __restrict__ V, int* __restrict__ fail) {
  kg1_pending_rows_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, ld, i0, i1, ncols, dp, cp, noise, append, PP, Z, VP, V, fail);
}

// The same for a member with g = dl.g observed derivatives per point: extension row i is observation a = i % g1 of pending point
// i / g1 (g1 = 1 + g), the column that of observation za of its point z (0: a function value -- every candidate; with `append` the
// column is row i1's own, za = i1 % g1, and its pivot takes noise[za]).  A point's radial scalars are taken once for its g1 rows.
struct kg1_pending_rows_g_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int ld, int i0, int i1, int ncols, int dp, const CovParams& cp, const DerivList& dl, int za, int append, const double* __restrict__ noise, const double* __restrict__ PP, const double* __restrict__ Z, const double* __restrict__ VP, double* __restrict__ V, int* __restrict__ fail) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    const int g1 = 1 + dl.g;
    double* v = V + (size_t)c * ld;
    const double* z = Z + (size_t)c * dp;
    double rl = (lane < i0) ? v[N + lane] : 0.0;
    Radial rd = {0.0, 0.0, 0.0, 0.0};
    for (int i = i0; i < i1; ++i) {
      const int j = i / g1, a = i - j * g1;
      const double* vp = VP + (size_t)i * ld;
      double acc = 0.0;
      for (int r = lane; r < N; r += 64) acc = fma(vp[r], v[r], acc);
      if (lane < i) acc = fma(vp[N + lane], rl, acc);
  #pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      const PointDiff df{PP + (size_t)j * dp, z};
      if (a == 0 || i == i0) rd = pair_radial(cp, df, dp);
      const double ri = (cov_entry_g(cp, rd, df, a, za, dl, dl) - acc) / vp[N + i];
      if (lane == i) rl = ri;
    }
    if (lane >= i0 && lane < i1) v[N + lane] = rl;
    if (append == 0) return;
    double ss = 0.0;
    for (int r = lane; r < N; r += 64) ss = fma(v[r], v[r], ss);
    if (lane < i1) ss = fma(rl, rl, ss);
  #pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (lane != 0) return;
    const PointDiff own{z, z};
    const double pivot = (cov_entry_g(cp, radial_scalars(cp.type, cp.alpha, 0.0), own, za, za, dl, dl) - ss) + noise[za];
    v[N + i1] = sqrt(pivot);
    if (!(pivot > kPivotMin)) atomicMin(fail, i1 / g1);  // the first pending POINT of the call with a failing row
  }
};
__global__ __launch_bounds__(256) void kg1_pending_rows_g_kernel(int N, int ld, int i0, int i1, int ncols, int dp, const CovParams cp, const DerivList dl, int za, int append, const double* __restrict__ noise, const double* __restrict__ PP, const double* __restrict__ Z, const double* __restrict__ VP, double* __restrict__ V, int* __restrict__ fail) {
  kg1_pending_rows_g_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, ld, i0, i1, ncols, dp, cp, dl, za, append, noise, PP, Z, VP, V, fail);
}

// One wavefront per column c of T: the back substitution u_P = L_P^-T t_P with lane m holding u_m (L_P[m][i] is entry N + i of
// column m of V'_P), stored under the member's rows of U; then t_r -= sum_m V_P[r][m] u_m for the member's rows, pending points in order.
struct kg1_pending_back_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, int N, int ld, int p, int ncols, const double* __restrict__ VP, double* __restrict__ T, double* __restrict__ U) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncols) return;
    double* t = T + (size_t)c * ld;
    double ul = (lane < p) ? t[N + lane] : 0.0;
    for (int i = p - 1; i >= 0; --i) {
      double acc = (lane > i && lane < p) ? VP[(size_t)lane * ld + N + i] * ul : 0.0;
  #pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
      const double ui = (__shfl(ul, i, 64) - acc) / VP[(size_t)i * ld + N + i];
      if (lane == i) ul = ui;
    }
    if (lane < p) U[(size_t)c * ld + N + lane] = ul;
    for (int r0 = 0; r0 < N; r0 += 64) {  // (every lane takes part in every shuffle)
      const int r = min(r0 + lane, N - 1);
      double x = t[r];
      for (int m = 0; m < p; ++m) x = fma(-VP[(size_t)m * ld + r], __shfl(ul, m, 64), x);
      if (r0 + lane < N) t[r] = x;
    }
  }
};
__global__ __launch_bounds__(256) void kg1_pending_back_kernel(int N, int ld, int p, int ncols, const double* __restrict__ VP, double* __restrict__ T, double* __restrict__ U) {
  kg1_pending_back_kernel_body::run(MOE_VBLOCK, MOE_VGRID, nullptr, N, ld, p, ncols, VP, T, U);
}

// za: which observation of its point the column is (append: the pending row's own; otherwise 0)
void launch_rows(const Kg1Member& m, const double* Z, double* V, int ncols, int i0, int i1, int append, int za, hipStream_t s) {
  const GpDev& gp = *m.gp;
  if (i0 < 0 || i0 > i1 || i1 + (append != 0 ? 1 : 0) > m.pcap || ncols < 1 || (append != 0 && (ncols != 1 || i0 != 0)) || za < 0 ||
      za >= m.g1 || m.g1 != 1 + gp.g)
    throw Error(MOE_ERR_RUNTIME, "kg1_pending_rows: the rows do not fit the member's extension");
  if (m.g1 > 1) {
    launch_kernel_ens<kg1_pending_rows_g_kernel_body, 256>(kg1_pending_rows_g_kernel, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, s,
                                                           gp.N, m.ld, i0, i1, ncols, gp.dp, gp.cp, gp.derivs, za, append,
                                                           (const double*)gp.dNoise.p, m.dPP, Z, (const double*)m.dVP, V, m.iFailP);
    MOE_HIP_CHECK(hipGetLastError());
    return;
  }
  launch_kernel_ens<kg1_pending_rows_kernel_body, 256>(kg1_pending_rows_kernel, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, s, gp.N,
                                                       m.ld, i0, i1, ncols, gp.dp, gp.cp, gp.noise[0], append, m.dPP, Z,
                                                       (const double*)m.dVP, V, m.iFailP);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace

void check_kg_discrete_pending(const double* pending, int num_pending, int num_to_sample) {
  if (num_pending < 0 || num_pending > kKg1MaxPending)
    throw Error(MOE_ERR_BOUNDS, "num_being_sampled must be between 0 and 64", num_pending, 0, kKg1MaxPending);
  if (num_to_sample < 1 || num_pending + num_to_sample - 1 > kKg1MaxPending)
    throw Error(MOE_ERR_BOUNDS, "num_to_sample must be positive, and num_being_sampled + num_to_sample - 1 at most 64", num_to_sample, 1,
                kKg1MaxPending + 1 - num_pending);
  if (num_pending > 0 && pending == nullptr) throw Error(MOE_ERR_RUNTIME, "points_being_sampled is NULL");
}

void kg1_pending_begin(Kg1Member& m, hipStream_t s) {
  const GpDev& gp = *m.gp;
  if (m.pcap < 1 || m.pcap > kKg1MaxPending || m.dPP == nullptr || m.dXe == nullptr)
    throw Error(MOE_ERR_RUNTIME, "kg1_pending_begin: the member has no room for pending points");
  const size_t N = (size_t)gp.N;
  copy_async(m.dXe, gp.dX.p, sizeof(double) * (size_t)gp.n * gp.dp, hipMemcpyDeviceToDevice, s);  // (points: n = N without derivatives)
  copy_async(m.dKe, gp.dKinvY.p, sizeof(double) * N, hipMemcpyDeviceToDevice, s);
  memset_async(m.dKe + N, 0, sizeof(double) * (size_t)m.pcap, s);
  m.p = 0;
}

void kg1_pending_append(Kg1Member& m, int count, bool set_ready, hipStream_t s) {
  GpDev& gp = *m.gp;
  const int N = gp.N, dp = gp.dp, g1 = m.g1, i0 = m.p, j0 = i0 / g1, rows = count * g1;  // (g1 = 1: a row is a point)
  if (count < 1 || i0 + rows > m.pcap) throw Error(MOE_ERR_RUNTIME, "kg1_pending_append: more pending points than the member has room for");
  if (set_ready && g1 != 1) throw Error(MOE_ERR_RUNTIME, "kg1_pending_append: the knowledge gradient's set takes no derivative rows");
  const double* Pj = m.dPP + (size_t)j0 * dp;
  copy_async(m.dXe + (size_t)(gp.n + j0) * dp, Pj, sizeof(double) * (size_t)count * dp, hipMemcpyDeviceToDevice, s);
  launch_cov_build(gp.cp, gp.dX.p, gp.n, gp.derivs, Pj, count, gp.derivs, nullptr, gp.dE.p, N, 0, s);
  tri_cols(gp, 'N', rows, gp.dE.p, N, m.dVP + (size_t)i0 * m.ld, m.ld, s);
  for (int i = i0; i < i0 + rows; ++i)  // (row i of L_P needs the rows before it)
    launch_rows(m, m.dPP + (size_t)(i / g1) * dp, m.dVP + (size_t)i * m.ld, 1, 0, i, 1, i % g1, s);
  m.p = i0 + rows;
  if (set_ready) launch_rows(m, m.dPA, m.dVA, m.A, i0, m.p, 0, 0, s);
}

void kg1_pending_rows(const Kg1Member& m, const double* Z, double* V, int ncols, int i0, int i1, hipStream_t s) {
  launch_rows(m, Z, V, ncols, i0, i1, 0, 0, s);
}

void kg1_pending_back(const Kg1Member& m, int ncols, hipStream_t s) {
  launch_kernel_ens<kg1_pending_back_kernel_body, 256>(kg1_pending_back_kernel, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, s, m.gp->N,
                                                       m.ld, m.p, ncols, (const double*)m.dVP, m.dT, m.dU);
  MOE_HIP_CHECK(hipGetLastError());
}

}  // namespace moe
