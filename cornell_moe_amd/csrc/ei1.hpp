// cornell_moe_amd/csrc/ei1.hpp -- what ei1.hip (the ensemble analytic expected improvement) lends to the one-point acquisitions
// that run its chain over a member's rows X u P: the member's layout, the members' check, the pass over the candidates and the tail
// of a gradient of the shape grad = sum_r coef_r grad_x k(row_r, x) with coef_r = -s [K^-1 (y - mean) ; 0]_r - (L'^-T t)_r.
// Compiled once in ei1.hip; the clients are gibbon1.hip, cei1.hip and ehvi1.hip.
#pragma once
#include <vector>

#include "gp.hpp"
#include "kg1_ascent.hpp"

namespace moe {

// Where one GP's per-pass scratch and results live for a call of at most C candidates (Kg1Member with an empty set: dKg the values
// [C], dGrad [C][d], dAA mu(P), dScal the candidates' scalars s, dMuh mu(x), dVx the columns, dT / dU the gradient's columns);
// pcap: room for that many extension ROWS, a multiple of 1 + g.  outs: that many result sets back to back, dKg [outs][C] and dGrad
// [outs][C][d] (ehvi1.hip keeps mu and var, and their gradients, apart).  Nothing is launched.
Kg1Member ei1_member(GpDev& gp, int C, double best, bool with_grad, int* fail, int pcap, int* fail_pending, int outs = 1);

// Kg1Call::check_members of ei1.hip, gibbon1.hip and cei1.hip: one dim, one device, one observed-derivative list, no member listed
// twice; then pending_room (1 + g) <= kKg1MaxPending rows.
void ei1_check_members(const Kg1Objective& o, const std::vector<GpDev*>& gps, int pending_room);

// A member's chain at C <= m.C candidates Px [C][dp] in device memory, pass after pass of m.per_pass; per pass (recordable):
//   launch_cov_build, tri_cols ('N'), launch_mean, kg1_pending_rows (p > 0), the client's candidate kernel, the gradient's tail
// cand: launches the candidate kernel for the pass's nc candidates, the first of them candidate c0 of the call; it reads m.dVx
// (ld m.ld, R = N + m.p rows) and m.dMuh and leaves the values in m.dKg [c0 ..) and, with a gradient, what the tail reads.
// who: the client's name for the pass, as the error of a pass that does not fit the member's buffers gives it.
using Ei1PassStep = void (*)(const Kg1Member& m, const double* Px, int nc, int c0, hipStream_t s);
using Ei1CandStep = void (*)(const Kg1Member& m, int nc, int c0, bool with_grad, hipStream_t s);
void ei1_eval_passes(const Kg1Member& m, const double* Px, int C, bool with_grad, hipStream_t s, const char* who, Ei1CandStep cand,
                     Ei1PassStep grad_tail);

// The gradient of nc candidates Px [nc][dp] of a pass whose candidate kernel has left s in m.dScal and the columns t in m.dT:
// kg1_pending_back (p > 0), tri_cols ('T'), then ei1_grad_kernel<DP> or, for a member with derivative observations,
// ei1_grad_g_kernel<DP>, into m.dGrad from candidate c0 on.  Recordable.
void ei1_grad_tail(const Kg1Member& m, const double* Px, int nc, int c0, hipStream_t s);

}  // namespace moe
