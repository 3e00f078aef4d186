// cornell_moe_amd/csrc/ehvi1.hpp -- what ehvi1.hip (the two-objective expected hypervolume improvement) lends to ehvi3.hip (the
// three-objective one) and to cehvi1.hip (the constrained form of both): a sub-member's layout with mu and var kept apart, its chain
// (ehvi1_cand_kernel, the two-sum gradient kernel and its tail), the members' check, and psi with its two derivatives at an edge;
// to cehvi1.hip also the call's record, its layout and the launches of the front and strip kernels.  The host functions are
// compiled once in ehvi1.hip; ehvi1_edge is inlined into the kernel that calls it.
#pragma once
#include <vector>

#include "acq1_device.hpp"
#include "gp.hpp"
#include "kg1_ascent.hpp"

namespace moe {

// EI's layout with two result sets: dKg [mu C | var C], dGrad [grad mu C d | grad var C d]; role: the GP's place in its member
Kg1Member ehvi1_member(GpDev& gp, int role, int C, bool with_grad, int* fail, int pcap, int* fail_pending);

// Kg1Ensemble::eval_points of both clients: ei1.hip's pass with ehvi1_cand_kernel and, in the place of ei1_grad_tail, the two-sum
// gradient kernel behind the same L'^-T
void ehvi1_eval_points(const Kg1Member& m, const double* Px, const double* Ph, int C, bool with_grad, hipStream_t s);

// Kg1Call::check_members of both clients: one dim, one device, no derivative observations, no GP listed twice; then pending_room
// <= kKg1MaxPending
void ehvi1_check_members(const Kg1Objective& o, const std::vector<GpDev*>& gps, int pending_room);

// What cehvi1.hip (the constrained form) takes beside: the two-objective call's record, where its device memory lies, and the
// launches of the front and strip kernels over a table of the OBJECTIVE sub-members' dKg ordered [e][2].
struct Ehvi1Call {
  const double* front;  // [F][2], the caller's
  int F;
  double r1, r2;
};
// where the call's own device memory lies inside the first GP's ehviD, in doubles: E members, the caller's F points, room for pcap
// pending points, C staged candidates
struct Ehvi1Layout {
  int E, F, cap, C;
  size_t oCaller, oFront, oCount, oVals, oCoef, total;
};
Ehvi1Layout ehvi1_layout(int E, int F, int pcap, int C);
// ehvi1_front_kernel: the members' fronts take the believed outcomes of `count` pending points whose means lie aa doubles behind
// the sub-members' dKg.  mask (NULL: all of them): [E][mask_ld] words, member e offers point j only where its word is not 0.
void ehvi1_launch_front(const Ehvi1Call& k, const Ehvi1Layout& l, double* base, const double* const* kg, size_t aa, const int* mask,
                        int mask_ld, bool first, int count, hipStream_t s);
// ehvi1_strip_kernel: A_e into base + l.oVals [E][l.C] and, with want_grad, the four coefficients into base + l.oCoef [E][l.C][4]
void ehvi1_launch_strip(const Ehvi1Call& k, const Ehvi1Layout& l, double* base, const double* const* kg, int C, bool want_grad,
                        hipStream_t s);

// psi and, with a gradient, its two derivatives at the edge t of a GP with mean mu and floored deviations sigma / sg
__device__ __forceinline__ void ehvi1_edge(double t, double mu, double sigma, double sg, bool want_grad, double& psi, double& dmu, double& dvar) {
  const double z = (t - mu) / sigma;
  const double cdf = normal_cdf(z), pdf = normal_pdf(z);
  psi = (t - mu) * cdf + sigma * pdf;
  dmu = 0.0;
  dvar = 0.0;
  if (!want_grad) return;
  if (sg == sigma) {  // (the same inputs give the same bits)
    dmu = -cdf;
    dvar = pdf / (2.0 * sg);
  } else {
    const double zg = (t - mu) / sg;
    dmu = -normal_cdf(zg);
    dvar = normal_pdf(zg) / (2.0 * sg);
  }
}

}  // namespace moe
