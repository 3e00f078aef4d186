// cornell_moe_amd/csrc/cehvi1.hpp -- what cehvi1.hip (the constrained expected hypervolume improvement) lends to logehvi1.hip and logehvi3.hip (its log
// forms for two and for three objectives): the call's record, where its device memory lies, and the description of a call whose members, fronts,
// believed-feasibility mask, pending-row extension and greedy hand-over are cehvi1.hip's while the rule that combines the members is
// the borrower's.  The host functions are compiled once in cehvi1.hip.
#pragma once
#include "ehvi1.hpp"
#include "ehvi3.hpp"
#include "kg1_ascent.hpp"

namespace moe {

struct CehviTau {
  double t[kCeiMaxConstraints];
};

// what the hooks need of the call (Kg1Objective::client)
struct CehviCall {
  int M, K;
  CehviTau tau;
  Ehvi1Call c2;  // M = 2
  Ehvi3Call c3;  // M = 3
};

// The call's device memory inside the first GP's ehviD, in doubles: the unconstrained client's block first (l2 or l3), then the
// table of the objective sub-members' dKg [E][M] (pointers), the believed-feasibility words [E][mask_ld] (integers), the
// feasibility kernel's [E][K][C][F, dF/dmu, dF/dvar] and the group values [E][1 + K][C].
struct CehviLayout {
  int E, M, K, C, mask_ld;
  Ehvi1Layout l2;
  Ehvi3Layout l3;
  size_t oObj, oMask, oFeas, oFactors, total;
};
CehviLayout cehvi_layout(const Kg1Ensemble& T);

// M, K and the thresholds of a call (thresholds may be NULL with num_constraints = 0); the caller sets c2 or c3
CehviCall cehvi_constraints_of(int M, int num_constraints, const double* thresholds);

// cehvi1.hip's description of a call over E (M + K) sub-members -- its members, staging hooks and group values [E][1 + K][C] -- with
// `combine` in the place of its product rule, K = 0 included (the mask is then all ones and the feasibility block empty)
Kg1Call cehvi_call_combined_by(int num_mcmc, const CehviCall& c, void (*combine)(const Kg1Ensemble& T, int C, double* value_out, double* grad_out));

}  // namespace moe
