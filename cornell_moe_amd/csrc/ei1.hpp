// cornell_moe_amd/csrc/ei1.hpp -- what ei1.hip (the ensemble analytic expected improvement) lends to the one-point acquisitions
// whose gradient has its shape, grad = sum_r coef_r grad_x k(row_r, x) with coef_r = -s [K^-1 (y - mean) ; 0]_r - (L'^-T t)_r over
// the rows X u P: the member's layout, the members' check and the tail of the gradient, compiled once in ei1.hip (gibbon1.hip is
// the second client).
#pragma once
#include <vector>

#include "gp.hpp"

namespace moe {

// Where one GP's per-pass scratch and results live for a call of at most C candidates (Kg1Member with an empty set: dKg the values
// [C], dGrad [C][d], dAA mu(P), dScal the candidates' scalars s, dMuh mu(x), dVx the columns, dT / dU the gradient's columns);
// pcap: room for that many extension ROWS, a multiple of 1 + g.  outs: that many result sets back to back, dKg [outs][C] and dGrad
// [outs][C][d] (ehvi1.hip keeps mu and var, and their gradients, apart).  Nothing is launched.
Kg1Member ei1_member(GpDev& gp, int C, double best, bool with_grad, int* fail, int pcap, int* fail_pending, int outs = 1);

// One dim, one device, one observed-derivative list, no member listed twice; then pending_room (1 + g) <= kKg1MaxPending rows.
void ei1_check_members(const std::vector<GpDev*>& gps, int pending_room);

// The gradient of nc candidates Px [nc][dp] of a pass whose candidate kernel has left s in m.dScal and the columns t in m.dT:
// kg1_pending_back (p > 0), tri_cols ('T'), then ei1_grad_kernel<DP> or, for a member with derivative observations,
// ei1_grad_g_kernel<DP>, into m.dGrad from candidate c0 on.  Recordable.
void ei1_grad_tail(const Kg1Member& m, const double* Px, int nc, int c0, hipStream_t s);

}  // namespace moe
