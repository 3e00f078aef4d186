// cornell_moe_amd/csrc/kg_mc_dp16b.hip -- instantiations of the KG Monte-Carlo kernels for padded dimension 16: the
// workgroup-per-sample (kg_mc_block.hpp) and the streamed-weights (kg_mc_stream.hpp) kernels (the LDS-table kernels are in
// kg_mc_dp16.hip).
#include "kg_mc_block.hpp"
#include "kg_mc_stream.hpp"

template void moe::mc::launch_block_dp<16>(const moe::KgMcParams&, int, int, int, int, int, hipStream_t);
template void moe::mc::launch_stream_dp<16>(const moe::KgMcParams&, int, int, int, size_t, hipStream_t);
