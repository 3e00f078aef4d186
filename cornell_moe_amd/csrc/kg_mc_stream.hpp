// cornell_moe_amd/csrc/kg_mc_stream.hpp -- the streamed-weights wave-per-sample q-KG / d-KG Monte-Carlo kernel
// kg_mc_stream_kernel (gfx950) and its launchers, over the shared core kg_mc.hpp and the LDS-state line search kg_mc_lds.hpp.
// Instantiated by kg_mc_dp{4,8,12,16}b.hip and kg_mc_dp{24,32}.hip.
#pragma once
#include "kg_mc.hpp"
#include "kg_mc_lds.hpp"

namespace moe {
namespace mc {

// Streamed-weights variant of the wave-per-sample kernel (r3), for point sets whose per-sample weights are too large for eight
// LDS slabs (d-KG at n = 2000 with 3 observed derivatives: 64 KB per sample).  The sample pre-pass (kg_sample_prep_kernel) and the
// weight table V (kg_sample_weights_kernel: every sample's weights, the fantasy points' and the zero padding included) exist
// already for the workgroup-per-sample kernel; here a WAVE owns a sample and reads its row of V inside the sweeps (16-byte loads, two per
// point at g = 3; a sample's 64 KB are re-read once per sweep -- eight waves x 256 CUs keep 131 MB of rows live, which the
// Infinity Cache holds), so the 160 KB of LDS serve the COORDINATES, shared by the workgroup's eight waves (22 of C5's 32
// tiles; the rest streams from L2).  No barrier, no lock-step line search: the passes are WideEval's.
// LDS: [64] exp table | leading tiles of the paired-row table | per wave: kWideScratch doubles.
template <int DP, int G>
struct kg_mc_stream_kernel_body {
  static __device__ __forceinline__ void run(const VIdx blockIdx, const VIdx gridDim, const void*, const KgMcParams& P) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wtab = P.wide_lds_tiles * DP * 64;
    double* coords = smem + kExpTabLen;
    double* st = coords + wtab + wave * kWideScratch;
    if (threadIdx.x < kExpTabLen) smem[threadIdx.x] = kExp2Tab64[threadIdx.x];
    const int size = P.dim - P.f;
    // (which evaluations this workgroup serves, and in what order: kg_mc.hpp next_evaluation; its LDS word is wave 0's scratch)
    bool moved = false;
    for (int e = first_evaluation(P, blockIdx); e >= 0; e = next_evaluation(P, gridDim, e, moved, reinterpret_cast<int*>(coords + wtab))) {
      const double* xs = P.XsTab + (long)e * P.tab_stride;
      const double* rec = P.blob + (long)e * P.rec.stride;
      __syncthreads();  // previous evaluation's readers are done (and the exp table is visible)
      {
        const d2t* src = reinterpret_cast<const d2t*>(xs);
        d2t* dst = reinterpret_cast<d2t*>(coords);
        for (int i = threadIdx.x; i < wtab / 2; i += blockDim.x) dst[i] = src[i];
      }
      __syncthreads();
      unsigned int ticket = 0;  // drawn one ahead (see kg_mc_kernel)
      unsigned int* next = P.next_sample + (long)e * kTicketStride;
      if (lane == 0) ticket = atomicAdd(next, 1u);
      unsigned long long tot_val = 0, tot_grad = 0;
      while (true) {
        const unsigned int sl = (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket);
        if (sl >= (unsigned int)P.num_local) break;
        if (lane == 0) ticket = atomicAdd(next, 1u);
        const long so = (long)e * P.num_local + sl;
        const int best_j = P.best_j[so];
        const double* disc = rec + P.rec.disc;
        double x[DP];
  #pragma unroll
        for (int k = 0; k < DP; ++k) x[k] = (k < size) ? disc[(long)best_j * size + k] : ((k < P.dim) ? 1.0 : 0.0);
        const d2t* xg = reinterpret_cast<const d2t*>(xs) + lane;
        lds_pair_ptr xl = (lds_pair_ptr)coords + lane;
        WideEval<DP, G, true> ev{xg, xl, {P.V + so * P.v_stride + (long)lane * (1 + G)}, smem, st + kLsRows * kMaxDimPadded,
                                 P.ntiles, P.wide_lds_tiles, P.cov_type, lane, P.mean};
        unsigned long long n_val = 0, n_grad = 0;
        const double fcur = line_search_lds<DP, G>(P, ev, st, x, n_val, n_grad);
        if (lane == 0) P.best_value[so] = fcur;
        tot_val += n_val;
        tot_grad += n_grad;
        if (lane < DP) {
          double v = 0.0;
  #pragma unroll
          for (int k = 0; k < DP; ++k)
            if (lane == k) v = x[k];
          P.best_point[so * DP + lane] = v;
        }
      }
      if (lane == 0 && (tot_val | tot_grad) != 0) {
        atomicAdd(&P.counters[2 * e], tot_val);
        atomicAdd(&P.counters[2 * e + 1], tot_grad);
      }
    }
  }
};
template <int DP, int G>
__global__ __launch_bounds__(512) void kg_mc_stream_kernel(KgMcParams P) {
  kg_mc_stream_kernel_body<DP, G>::run(MOE_VBLOCK, MOE_VGRID, nullptr, P);
}

template <int DP, int G>
inline void launch_stream_inst(const KgMcParams& P, int blocks, int waves, size_t shm, hipStream_t s) {
  auto kern = kg_mc_stream_kernel<DP, G>;
  launch_kernel_ens<kg_mc_stream_kernel_body<DP, G>, 512>(kern, dim3(blocks), dim3(waves * 64), shm, s, P);
  MOE_HIP_CHECK(hipGetLastError());
}

// built for 1 .. 4 derivative slots with every slot observed (1 + g == 1 + G: the table rows of a point are its weights); the wide
// padded dimensions (24, 32) for the reduced set {0, 4, 8, 12}
template <int DP>
void launch_stream_dp(const KgMcParams& P, int G, int blocks, int waves, size_t shm, hipStream_t s) {
  switch (G) {
    case 0: return launch_stream_inst<DP, 0>(P, blocks, waves, shm, s);
    case 1: if constexpr (DP <= 16) return launch_stream_inst<DP, 1>(P, blocks, waves, shm, s); break;
    case 2: if constexpr (DP <= 16) return launch_stream_inst<DP, 2>(P, blocks, waves, shm, s); break;
    case 3: if constexpr (DP <= 16) return launch_stream_inst<DP, 3>(P, blocks, waves, shm, s); break;
    case 4: return launch_stream_inst<DP, 4>(P, blocks, waves, shm, s);
    // r4: 8 and 12 observed derivatives (C5's stretch point, g = 12: a sample's weights are 13 doubles per point, 213 KB at n = 2000 --
    // they fit no on-chip store, and the workgroup-per-sample kernel's all-register instantiation spilt them to scratch: 713 GB of
    // traffic per evaluation; here they stream once per sweep)
    case 8: if constexpr (DP >= 8) return launch_stream_inst<DP, 8>(P, blocks, waves, shm, s); break;
    case 12: if constexpr (DP >= 12) return launch_stream_inst<DP, 12>(P, blocks, waves, shm, s); break;
  }
  throw Error(MOE_ERR_RUNTIME, "unsupported derivative-slot count in the streamed-weights MC kernel");
}

}  // namespace mc
}  // namespace moe
