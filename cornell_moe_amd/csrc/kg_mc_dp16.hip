// cornell_moe_amd/csrc/kg_mc_dp16.hip -- instantiations of the KG Monte-Carlo kernels for padded dimension 16: the LDS-table
// wave-per-sample kernels with the frame line search (kg_mc_wave.hpp) and the lane-parked one (kg_mc_lane.hpp); the
// workgroup-per-sample and streamed-weights kernels are in kg_mc_dp16b.hip (r6: two translation units per dimension -- with the
// ensemble twins one unit took six minutes to compile).
#include "kg_mc_lane.hpp"
#include "kg_mc_wave.hpp"

template void moe::mc::launch_dp<16>(const moe::KgMcParams&, int, bool, int, int, size_t, hipStream_t);
template void moe::mc::launch_lane_dp<16>(const moe::KgMcParams&, int, int, int, int, size_t, hipStream_t);
