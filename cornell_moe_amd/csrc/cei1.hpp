// cornell_moe_amd/csrc/cei1.hpp -- what cei1.hip (the constrained expected improvement under the ensemble) lends to logcei1.hip,
// the log of the same quantity: the sub-member's layout with its role, and the believed-feasible incumbent with the two staging
// hooks that keep it.  Compiled once in cei1.hip.
#pragma once
#include "gp.hpp"
#include "kg1_ascent.hpp"

namespace moe {

// Kg1Objective::member: ei1_member with the sub-member's limit o.best_so_far[e] (b_e for role 0, tau_k for role k) and its role
// e mod max(o.group, 1).
Kg1Member cei1_member(const Kg1Objective& o, GpDev& gp, int e, int C, bool with_grad, int* fail, int pcap, int* fail_pending);

// mu of every sub-member at the pending points j0 .. j0 + count - 1, then every member's b' = min(b, min over the believed-feasible
// of them of mu_{e,0}(P_j)) into the sub-members' dBp (first: from the incumbent as given, the thresholds written beside it;
// otherwise joined to the b' that stands).  The groups are T.group sub-members wide.
void cei1_join_believed_feasible(Kg1Ensemble& T, int j0, int count, bool first);

// Kg1Objective::all_extended and Kg1Objective::pick_appended over the join above
void cei1_all_extended(Kg1Ensemble& T, int p);
void cei1_pick_appended(Kg1Ensemble& T);

}  // namespace moe
