// cornell_moe_amd/csrc/ehvi3.hpp -- what ehvi3.hip (the three-objective expected hypervolume improvement) lends to cehvi1.hip (the
// constrained form): the call's record, where its device memory lies, and the launches of the front, table and box kernels over a
// table of the OBJECTIVE sub-members' dKg ordered [e][3].  Compiled once in ehvi3.hip.
#pragma once
#include "gp.hpp"
#include "kg1_ascent.hpp"

namespace moe {

// what the hooks need of a three-objective call (Kg1Objective::client)
struct Ehvi3Call {
  const double* front;  // [F][3], the caller's
  int F;
  double r1, r2, r3;
};

// where the call's own device memory lies inside the first GP's ehviD, in doubles (a box fills one double's room): E members, the
// caller's F points, room for pcap pending points, C staged candidates
struct Ehvi3Layout {
  int E, F, cap, C;
  size_t tstride, oCaller, oFront, oCount, oNbox, oTable, oVals, oCoef, total;
};
Ehvi3Layout ehvi3_layout(int E, int F, int pcap, int C);

// ehvi3_front_kernel, then ehvi3_table_kernel: the members' fronts take the believed outcomes of `count` pending points whose means
// lie aa doubles behind the sub-members' dKg, and every member's box table is rebuilt.  mask (NULL: all of them): [E][mask_ld]
// words, member e offers point j only where its word is not 0.
void ehvi3_launch_front(const Ehvi3Call& k, const Ehvi3Layout& l, double* base, const double* const* kg, size_t aa, const int* mask,
                        int mask_ld, bool first, int count, hipStream_t s);
// ehvi3_box_kernel: A_e into base + l.oVals [E][l.C] and, with want_grad, the six coefficients into base + l.oCoef [E][l.C][6]
void ehvi3_launch_box(const Ehvi3Call& k, const Ehvi3Layout& l, double* base, const double* const* kg, int C, bool want_grad,
                      hipStream_t s);

}  // namespace moe
