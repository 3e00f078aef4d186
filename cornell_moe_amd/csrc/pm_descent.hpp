// cornell_moe_amd/csrc/pm_descent.hpp -- the back-tracking line search that stays resident in one workgroup, for the kernels that
// minimise one function per workgroup: every member's posterior mean (pm_members.hip: pmm_descent_kernel) and every posterior
// function path (paths.hip: paths_descent_kernel).  posterior_mean_optimize's loop (multistart.hip) decision for decision, on f = -mu
// for whatever mu the evaluator computes.
#pragma once
#include <hip/hip_runtime.h>

namespace moe {

constexpr int kPmmThreads = 256;   // threads of the workgroup: the stride of an evaluation's sums
constexpr int kPmmTraceExtra = 6;  // trace columns behind the point: f0 | halvings | limiter changed | rejected | stopped by norm | state
constexpr int kPmmHead = 3;        // result columns in front of the point: start index | fell back | value

struct PmmDescent {
  const int* start_index;  // [rows] into the row's candidates
  const double* cand;      // [.][DP]
  long member_stride;      // rows between the members' candidate sets (0: shared)
  const double* alpha0;    // [T]: pre_mult (i + 1)^-gamma
  const double* bounds;    // [size][2]
  const double* means;     // [rows][C]: the screened values
  int C, T, R;             // candidates; max_num_steps; max_num_restarts
  double max_relative_change, tolerance, step_tol;
  double* out;    // [rows][kPmmHead + DP]
  double* trace;  // [rows][R T][size + kPmmTraceExtra] (zeroed) or NULL
};

// TensorProductDomain::LimitUpdate (gpp_domain.cpp:64-105) on one coordinate: multistart.hip's limit_update_1d
__device__ __forceinline__ double pmm_limit_1d(double lo, double hi, double max_relative_change, double x, double desired) {
#pragma clang fp contract(off)
  const double dist = fmin(x - lo, hi - x);
  if (fabs(desired) > max_relative_change * dist) desired = copysign(max_relative_change * dist, desired);
  const double next = x + desired;
  if (next < lo) {
    desired = (x + desired * 0.5 < lo) ? (lo - x) * 0.5 : desired * 0.5;
  } else if (next > hi) {
    desired = (x + desired * 0.5 > hi) ? (hi - x) * 0.5 : desired * 0.5;
  }
  return desired;
}

// The whole optimisation of unit `unit` (a member, a path) by its workgroup of kPmmThreads threads: from candidate start_index[unit]
// of the set that begins at candidate row cand0, the line search, then keep or fall back.  ev.template eval<GRAD>(pt, red, tot) leaves
// mu(pt) in tot[0] and with GRAD d mu / d x_k in tot[1 + k], valid for every thread, and begins and ends with a barrier; pt is LDS
// [DP] (padding and pinned coordinates as the evaluator wants them: the search moves the first `size` only).  red [4 (1 + DP)],
// tot [1 + DP], xs, pt, gs, xb [DP]: LDS.  Every thread takes the same scalar decisions: control flow is workgroup-uniform.  The
// scalar algebra between evaluations is kept free of fused multiply-adds, as the host loop's is.
template <int DP, class Eval>
__device__ __forceinline__ void pmm_descend(const Eval& ev, const PmmDescent& D, int unit, long cand0, int size, double* red,
                                            double* tot, double* xs, double* pt, double* gs, double* xb) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int start = D.start_index[unit];
  const long tw = size + kPmmTraceExtra;
  double* trace = D.trace ? D.trace + (long)unit * D.R * D.T * tw : nullptr;
  if (tid < DP) xs[tid] = D.cand[(cand0 + start) * DP + tid];
  for (int r = 0; r < D.R; ++r) {
    __syncthreads();
    if (tid < DP) xb[tid] = xs[tid];
    for (int i = 0; i < D.T; ++i) {
      ev.template eval<true>(xs, red, tot);
      const double f0 = -tot[0];
      if (tid < DP) gs[tid] = (tid < size) ? -tot[1 + tid] : 0.0;
      __syncthreads();
      double alpha = D.alpha0[i];
      double n2 = 0.0;
      for (int k = 0; k < size; ++k) n2 += gs[k] * gs[k];
      int search = 0;
      double ftrial = f0;
      for (; search < 30; ++search) {
        if (tid < DP) pt[tid] = (tid < size) ? xs[tid] + alpha * gs[tid] : xs[tid];
        ev.template eval<false>(pt, red, tot);
        ftrial = -tot[0];
        if (ftrial - f0 > 0.5 * alpha * n2) break;
        alpha *= 0.5;
      }
      bool changed = false, nonzero = false;
      double mine = 0.0, s2 = 0.0;  // this thread's coordinate of the limited step; its squared norm
      for (int k = 0; k < size; ++k) {
        const double raw = alpha * gs[k];
        const double st = pmm_limit_1d(D.bounds[2 * k], D.bounds[2 * k + 1], D.max_relative_change, xs[k], raw);
        changed = changed || st != raw;
        nonzero = nonzero || st != 0.0;
        s2 += st * st;
        if (k == tid) mine = st;
      }
      double* row = trace ? trace + ((long)r * D.T + i) * tw : nullptr;
      if (row && tid == 0) {
        row[size] = f0;
        row[size + 1] = (double)search;
        row[size + 2] = changed ? 1.0 : 0.0;
      }
      if (search == 30 || !nonzero) {
        if (row && tid < size) row[tid] = xs[tid];
        if (row && tid == 0) row[size + 5] = 2.0;  // ended without a move
        break;
      }
      double obj2 = ftrial;
      if (changed) {
        if (tid < DP) pt[tid] = (tid < size) ? xs[tid] + mine : xs[tid];
        ev.template eval<false>(pt, red, tot);
        obj2 = -tot[0];
      }
      if (obj2 <= f0) {
        if (row && tid < size) row[tid] = xs[tid];
        if (row && tid == 0) {
          row[size + 3] = 1.0;
          row[size + 5] = 3.0;  // rejected
        }
        break;
      }
      __syncthreads();  // (every thread has read xs)
      if (tid < size) {
        xs[tid] += mine;
        if (row) row[tid] = xs[tid];
      }
      const bool stop = sqrt(s2) < D.step_tol;
      if (row && tid == 0) {
        row[size + 4] = stop ? 1.0 : 0.0;
        row[size + 5] = 1.0;  // accepted
      }
      if (stop) break;
    }
    __syncthreads();
    double s2 = 0.0;
    for (int k = 0; k < size; ++k) {
      const double v = xb[k] - xs[k];
      s2 += v * v;
    }
    if (!(sqrt(s2) > D.tolerance)) break;
  }
  // keep or fall back (main.py:191-193), both means through the screening's evaluation
  ev.template eval<false>(xs, red, tot);
  const double mu_end = tot[0], mu_start = D.means[(long)unit * D.C + start];
  const bool fall_back = mu_end > mu_start;
  double* out = D.out + (long)unit * (kPmmHead + DP);
  if (tid == 0) {
    out[0] = (double)start;
    out[1] = fall_back ? 1.0 : 0.0;
    out[2] = fall_back ? mu_start : mu_end;
  }
  if (tid < DP) out[kPmmHead + tid] = fall_back ? D.cand[(cand0 + start) * DP + tid] : xs[tid];
}

}  // namespace moe
