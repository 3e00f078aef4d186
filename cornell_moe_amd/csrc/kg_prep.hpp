// cornell_moe_amd/csrc/kg_prep.hpp -- the kernels that prepare a q-KG / d-KG evaluation's Monte-Carlo step (kg_prep.hip): the
// coordinate tables, the start table, the sample pre-pass and the per-sample weight table.  The driver is kg.hip.
#pragma once
#include "kg_mc.hpp"

namespace moe {

// the frame of the coordinate tables, in table-row order (kg.hip table_rows)
struct TabParams {
  int perm[kMaxDimPadded];
  double inv_lp[kMaxDimPadded];
  double center[kMaxDimPadded];  // training-set mean per table row (unscaled)
};

// The coordinate tables of E evaluations (n training points X, then u union points each from XuAll; tab_stride doubles per evaluation);
// evaluation 0's workgroups also clear the call's n_ctr counters.
void launch_xs_tab(const double* X, int n, const double* XuAll, int u, int dp, int ntiles, const TabParams& tp, double* tab, long tab_stride,
                   int pair_rows, unsigned long long* ctr, long n_ctr, int E, hipStream_t s);
// The start table of an evaluation without derivative observations (mc::start_from_table): padded dimensions up to 16.
void launch_start_table(const KgMcParams& P, int dp, double* tab, hipStream_t s);
// beta = L^-T z and the discretised-set winner of every sample (P.beta, best_j), with the whole chip
void launch_sample_prep(const KgMcParams& P, int* best_j, int num_cu, hipStream_t s);
// The per-sample weight table V.  table_only: no in-kernel form of the weights has to be reproduced bit for bit.
void launch_sample_weights(const KgMcParams& P, double* V, hipStream_t s, bool table_only = false);

}  // namespace moe
