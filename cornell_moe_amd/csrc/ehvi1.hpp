// cornell_moe_amd/csrc/ehvi1.hpp -- what ehvi1.hip (the two-objective expected hypervolume improvement) lends to ehvi3.hip (the
// three-objective one): a sub-member's layout with mu and var kept apart, its chain (ehvi1_cand_kernel, the two-sum gradient kernel
// and its tail), the members' check, and psi with its two derivatives at an edge.  The host functions are compiled once in
// ehvi1.hip; ehvi1_edge is inlined into the kernel that calls it.
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
