// cornell_moe_amd/csrc/kg_mc_dp24.hip -- instantiations of the KG Monte-Carlo kernels for padded dimension 24 (d = 17 .. 24):
// the reduced sets of launch_dp (kg_mc_wave.hpp), launch_block_dp (kg_mc_block.hpp) and launch_stream_dp (kg_mc_stream.hpp), DP > 16.
#include "kg_mc_block.hpp"
#include "kg_mc_stream.hpp"
#include "kg_mc_wave.hpp"

template void moe::mc::launch_dp<24>(const moe::KgMcParams&, int, bool, int, int, size_t, hipStream_t);
template void moe::mc::launch_block_dp<24>(const moe::KgMcParams&, int, int, int, int, int, hipStream_t);
template void moe::mc::launch_stream_dp<24>(const moe::KgMcParams&, int, int, int, size_t, hipStream_t);
