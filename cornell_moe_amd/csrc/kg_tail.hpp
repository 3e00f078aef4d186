// cornell_moe_amd/csrc/kg_tail.hpp -- the gradient tail of a q-KG / d-KG evaluation (kg_tail.hip): what the driver (kg.hip) fills in,
// sizes its workspaces with and launches.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "gp.hpp"
#include "kg_mc.hpp"

namespace moe {

struct KgTailParams {
  CovParams cp;
  DerivList derivs;  // the GP's derivative observations (carried by the union points too)
  int u, q, m, g, N, E, num_local, first_sample, ngrad, chunks, sw_chunk;
  int chunk_len;  // samples per TB partial (kTbChunk, or kFusedChunk on the T-free q-KG path): chunks = ceil(num_local / chunk_len)
  const double* T;           // [N x E*num_local], ld N
  const double* SW;          // optional precomputed W^T T, [m x E*num_local] col-major (large m: tile GEMM); else null
  const double* W;           // evaluation e at W + e * w_stride, [N x m], ld N
  long w_stride;
  const double* Gm;          // dK*/dXq: evaluation e at Gm + e * g_stride, [N x ngrad], ld N
  long g_stride;
  const double* Linv;        // the GP's explicit inverse factor (ld ldL) and 2 N E m doubles of workspace: K^-1 TB (launch_gtb)
  long ldL;
  double* work;
  double* tri_work;          // tri_cols_work_doubles(N, E m) doubles (split-K partials)
  const double* blob;
  KgRec rec;
  int rec_bp;                // offset of best_posterior inside a record
  const double* best_point;  // [E][num_local][dp]
  const double* best_value;  // [E][num_local]
  const double* beta;        // [E][num_local][m]
  const double* normals;     // [ceil(M/2)][m]
  double* C;                 // [E][num_local][m]   c_i = L^-1 cov_n(Xu, x*_i)
  double* TBpart;            // [E][chunks][m][N]
  double* out;               // [E][out_stride]: kg_sum | ZC (m*m, col-major) | DIR (ngrad) | GTB (ngrad)
  int out_stride;
};

constexpr int kTbChunk = 256;  // samples per workgroup of kg_tb_kernel
constexpr int kTbChunkWide = 2048;  // m > 64: samples per partial of the matrix-pipe TB product (kg_tb128_kernel)
// ... and of kg_fused_point_kernel: 128, so that ONE q-KG evaluation (n = 1000: 4 row blocks x 79 chunks) puts more than one
// workgroup on every CU -- 40.7 -> ~20 us of a batch-1 evaluation's tail.  Fixed per path, not per batch size: an evaluation's
// bits do not depend on what it is batched with.
constexpr int kFusedChunk = 128;
constexpr int kDirSlices = 32;  // sample ranges of kg_dir_kernel
constexpr int kSwChunk = 64;  // samples per workgroup of kg_sw_kernel (16 per wavefront); 16 when the batch is too small to fill the chip
constexpr int kZcChunk = 64;  // samples per chunk of kg_zc_part_kernel (32 for m > 32: the two staged blocks stay within 32 KB)

// an integer switch of the process (unset and empty: dflt)
inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}

inline int zc_chunk_len(int m) { return m > 32 ? kZcChunk / 2 : kZcChunk; }  // (r4: m > 64 too -- 2 x 32 x 128 doubles: 64 KB, opted in)
inline int zc_sum_lanes(int m) {  // lanes that share an entry of ZC in kg_zc_sum_kernel
  int gs = 1;
  while (gs < 64 && m * m * gs * 2 <= 256) gs *= 2;
  return gs;
}
// r5: for small m and few chunks the sum of the partials is taken by kg_finish_kernel itself (one launch less on the latency path)
inline bool zc_sum_in_finish(int m, int num_local) {
  const long chunks = (num_local + zc_chunk_len(m) - 1) / zc_chunk_len(m);
  return m <= 8 && chunks * m * m <= 16384;
}
// (the slices of DIR are added up in order by kg_finish_kernel, where DIR is consumed -- r5; a kernel of its own before)
inline int dir_slices(int num_local) { return std::max(1, std::min(kDirSlices, (num_local + 255) / 256)); }
inline double* dir_partials(const KgTailParams& P) {
  // behind the summed TB in the TB buffer (the host reserves E * ngrad * kDirSlices doubles more)
  return P.TBpart + (long)P.E * (P.chunks + 1) * (long)P.m * P.N;
}

// q-KG fast path: the gradient tail never materialises the N x M covariance matrix (see launch_fused_tail).  A function of the
// evaluation's shape and MOE_KG_FUSED_TAIL -- kg_launch (plan_mc) and kg_max_batch both ask here, so they cannot disagree.
inline bool fused_tail_taken(bool want_grad, int g, int m) { return want_grad && g == 0 && m <= 8 && env_int("MOE_KG_FUSED_TAIL", 1) != 0; }
// which form the T-free tail takes: a switch of the process, never a function of the batch
inline bool fused_tail_sw_free() { return env_int("MOE_KG_FUSED_ONE_PASS", 1) != 0; }
// samples per TB partial of the gradient tail
inline int tail_chunk_len(bool fused_tail, int m) { return fused_tail ? kFusedChunk : (m > 64 ? kTbChunkWide : kTbChunk); }
// number of point slices of kg_fused_sample_kernel (a function of the evaluation's shape, never of the batch)
int fused_tail_slices(int E, int num_local, int n, int num_cu);

// The tail through the materialised T = K(X, x*_i): c_i (kg_sw_kernel; S_W = W^T T from P.SW where set), DIR, the TB partials, GTB.
void launch_tail(const KgTailParams& P, hipStream_t s);
// S_W = W_e^T T_e for 64 < m <= 128 (kg_sw128_kernel): the K slices' partials in SWpart, added up in slice order into SW.
void launch_sw128(const KgTailParams& P, double* SWpart, int slices, double* SW, hipStream_t s);
// T-free tail (requires g == 0, m <= 8); SWpart / slices: the two-kernel form's workspace (fused_tail_sw_free(): unused).
void launch_fused_tail(const KgTailParams& P, const double* X, int n, double* SWpart, int slices, hipStream_t s);
// ZC chunk partials (part = E * chunks * m * m doubles of workspace) and, with sum_here, their sum and kg_sum.
void launch_zc(const KgTailParams& P, double* part, hipStream_t s, bool sum_here = true);
// value-only finish: kg_sum per evaluation and the record the host reads back (kg_sum | value passes | gradient passes | singular flag)
void launch_kg_sum(const KgTailParams& P, double* fin, const unsigned long long* counters, const int* flags, hipStream_t s);

}  // namespace moe
