// cornell_moe_amd/csrc/kg1_ascent.hpp -- what the ensemble forms of the one-point acquisition functions share (kg1_opt.hip: the
// discretised knowledge gradient; ei1.hip: the analytic expected improvement): the ensemble mean, the multistart ascent's gather,
// step and round kernels, the recorded and zipped evaluation of the members' chains, and the ascent itself (ascend()).  None of it
// knows the objective: a member's chain is Kg1Ensemble::eval_points, its results the member's dKg / dGrad.  Every includer gets
// its own copy of the kernels (unnamed namespace): the same text, the same bits.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gp.hpp"
#include "kg.hpp"

namespace moe {

namespace {

// out[i] = (src[0][i] + src[1][i] + ... ) / E, members ascending
__global__ __launch_bounds__(256) void kg1_mean_kernel(int E, long n, const double* const* __restrict__ src, double* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double v = src[0][i];
  for (int e = 1; e < E; ++e) v = v + src[e][i];
  out[i] = v / (double)E;
}

// the words of the call as doubles in front of the results: one copy back
__global__ __launch_bounds__(256) void kg1_words_kernel(const int* __restrict__ words, int n, double* __restrict__ out) {
  for (int i = threadIdx.x; i < n; i += 256) out[i] = (double)words[i];
}

struct Kg1Ascent {
  int K, E, d, dp, size;  // size = d - num_fidelity: the coordinates x^ shares with x
  const double* const* grad;  // [E]: the members' gradients [K][d]
  const double* bounds;       // [d][2]
  double* X;       // [K][dp]: the kept starts, moved in place
  double* Xh;      // [K][dp]: the same with fidelity coordinates 1 (= X without fidelity)
  double* Xbegin;  // [K][dp]: the points at the start of the restart round
  int* running;    // [K]: the start still steps in this round
  int* alive;      // [K]: the start takes part in the next round
  int* steps;      // [K]: steps taken
  int* count;      // alive starts after the last round
  double* path;    // [K][rows][d] or NULL
  int rows;
};

// the kept starts out of the uploaded ones, and the ascent's state
__global__ __launch_bounds__(64) void kg1_gather_kernel(Kg1Ascent a, const int* __restrict__ order, const double* __restrict__ starts,
                                                        const double* __restrict__ starts_h) {
  const int k = threadIdx.x;
  if (k >= a.K) return;
  const size_t src = (size_t)order[k] * a.dp, dst = (size_t)k * a.dp;
  for (int j = 0; j < a.dp; ++j) {
    const double v = starts[src + j];
    a.X[dst + j] = v;
    a.Xbegin[dst + j] = v;
    if (a.Xh != a.X) a.Xh[dst + j] = starts_h[src + j];
  }
  if (a.path != nullptr)
    for (int j = 0; j < a.d; ++j) a.path[(size_t)k * a.rows * a.d + j] = starts[src + j];
  a.running[k] = 1;
  a.alive[k] = 1;
  a.steps[k] = 0;
  if (k == 0) *a.count = a.K;
}

// TensorProductDomain::LimitUpdate on one coordinate (multistart.hip: limit_update_1d), every operation rounded by itself
__device__ __forceinline__ double kg1_limit_update_1d(double lo, double hi, double max_relative_change, double x, double desired) {
#pragma clang fp contract(off)
  const double dist = fmin(x - lo, hi - x);
  const double cap = max_relative_change * dist;
  if (fabs(desired) > cap) desired = copysign(cap, desired);
  const double next = x + desired;
  const double half = desired * 0.5;
  if (next < lo) {
    desired = (x + half < lo) ? (lo - x) * 0.5 : half;
  } else if (next > hi) {
    desired = (x + half > hi) ? (hi - x) * 0.5 : half;
  }
  return desired;
}

// One thread per kept start: gradient_ascent's update (multistart.hip) of a running start -- the members' gradients added in member
// order and divided by E, step = alpha grad, the limiter per coordinate, x += step, and the start stops when the step's 2-norm falls
// below step_tol.  A start that is not running keeps its point.  row: the path row this step writes.
__global__ __launch_bounds__(64) void kg1_step_kernel(Kg1Ascent a, double alpha, double max_relative_change, double step_tol, int row) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  if (k >= a.K) return;
  double* x = a.X + (size_t)k * a.dp;
  if (a.running[k]) {
    double sum = 0.0;
    for (int j = 0; j < a.d; ++j) {
      double g = a.grad[0][(size_t)k * a.d + j];
      for (int e = 1; e < a.E; ++e) g = g + a.grad[e][(size_t)k * a.d + j];
      g = g / (double)a.E;
      const double xj = x[j];
      const double step = kg1_limit_update_1d(a.bounds[2 * j], a.bounds[2 * j + 1], max_relative_change, xj, alpha * g);
      const double moved = xj + step;
      x[j] = moved;
      if (a.Xh != a.X && j < a.size) a.Xh[(size_t)k * a.dp + j] = moved;
      const double sq = step * step;
      sum = sum + sq;
    }
    a.steps[k] += 1;
    if (sqrt(sum) < step_tol) a.running[k] = 0;
  }
  if (a.path != nullptr)
    for (int j = 0; j < a.d; ++j) a.path[((size_t)k * a.rows + row) * a.d + j] = x[j];
}

// The end of a restart round: a start that moved by more than the tolerance since the round began goes into the next one.
__global__ __launch_bounds__(64) void kg1_round_kernel(Kg1Ascent a, double tolerance) {
#pragma clang fp contract(off)
  __shared__ int s_alive[64];
  const int k = threadIdx.x;
  int mine = 0;
  if (k < a.K) {
    if (a.alive[k]) {
      double sum = 0.0;
      for (int j = 0; j < a.d; ++j) {
        const double diff = a.Xbegin[(size_t)k * a.dp + j] - a.X[(size_t)k * a.dp + j];
        const double sq = diff * diff;
        sum = sum + sq;
      }
      mine = (sqrt(sum) > tolerance) ? 1 : 0;
    }
    a.alive[k] = mine;
    a.running[k] = mine;
    for (int j = 0; j < a.dp; ++j) a.Xbegin[(size_t)k * a.dp + j] = a.X[(size_t)k * a.dp + j];
  }
  s_alive[k] = mine;
  __syncthreads();
  if (k == 0) {
    int n = 0;
    for (int i = 0; i < 64; ++i) n += s_alive[i];
    *a.count = n;
  }
}

constexpr int kMaxKept = 64;  // (one workgroup of 64 threads moves the kept starts; top_k_order keeps 20)

// What the members of one call share: their layouts, the stream, and whether their chains are recorded and zipped.
struct Kg1Ensemble {
  std::vector<GpDev*> gps;
  std::vector<Kg1Member> mem;
  hipStream_t z = nullptr;
  bool ens = false;
  int E = 0, d = 0, dp = 0, nf = 0;
  // a member's chain at C points in device memory, results left in its dKg / dGrad (recordable: launch.hpp)
  void (*eval_points)(const Kg1Member& m, const double* Px, const double* Ph, int C, bool with_grad, hipStream_t s) = kg1_eval_points;
  bool fid = false;
  // device addresses inside the first member's dStateIn (the one upload)
  const double* const* dKgTab = nullptr;
  const double* const* dGradTab = nullptr;
  const double* dBounds = nullptr;
  const double* dPts = nullptr;
  const double* dPtsH = nullptr;
  int* iFail = nullptr;  // [E] in the first member's kg1oI
  // pending points (kg1_pending.hip): p of pcap in use; with room for them the members' pending failure words [E] follow iFail, and
  // W = 2 E words travel where E do without
  int p = 0, pcap = 0, W = 0;
  double* dPending = nullptr;  // [pcap][dp] inside the one upload
};

// one evaluation of the ensemble, recorded once and issued as often as the caller likes (the buffers it names stay put)
struct Kg1Recording {
  std::vector<Recorder> recs;
  EnsZip zip;
  bool tried = false, zipped = false;
  ~Kg1Recording() {
    for (Recorder& r : recs) {
      for (auto& b : r.retired_dev) DevicePool::get().give(b.first, b.second);
      for (auto& b : r.retired_host) DevicePool::get().give_host(b.first, b.second);
    }
  }
};

void evaluate(Kg1Ensemble& T, Kg1Recording& rec, const double* Px, const double* Ph, int C, bool with_grad) {
  if (!T.ens) {
    for (const Kg1Member& m : T.mem) T.eval_points(m, Px, Ph, C, with_grad, T.z);
    return;
  }
  EnsArena arena{T.gps[0]->hEns, T.gps[0]->dEns};
  if (!rec.tried) {
    rec.recs.resize(T.mem.size());
    for (size_t e = 0; e < T.mem.size(); ++e) {
      Recorder::Scope scope(&rec.recs[e]);
      T.eval_points(T.mem[e], Px, Ph, C, with_grad, T.z);
    }
    rec.zipped = ensemble_zip(rec.recs, T.z, arena, &rec.zip);
    rec.tried = true;
    if (rec.zipped) ensemble_stats_add(2, 1);  // (the tables' copy)
  }
  const long long L = (long long)rec.recs[0].ops.size(), M = (long long)T.mem.size();
  if (rec.zipped) {
    ensemble_issue(rec.recs, rec.zip, T.z, arena);
    ensemble_stats_add(0, 1);
    ensemble_stats_add(2, rec.zip.merged + (L - rec.zip.merged) * M);
    ensemble_stats_add(3, L * M);
  } else {  // member by member, what immediate launches would have done
    for (const Recorder& r : rec.recs)
      for (const LaunchOp& op : r.ops) op.run(T.z);
    MOE_HIP_CHECK(hipGetLastError());
    ensemble_stats_add(1, 1);
  }
}

void launch_mean_of_members(const Kg1Ensemble& T, const double* const* tab, long n, double* out) {
  MOE_LAUNCH_NOW(kg1_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, T.z, T.E, n, tab, out);
  MOE_HIP_CHECK(hipGetLastError());
}

// after a wait: the first member with a candidate that failed the pivot rule
template <class Word>
void throw_if_singular(const Kg1Ensemble& T, const Word* fail_words) {
  for (int e = T.E; e < T.W; ++e)  // (a failed extension spoils every candidate of its member: it is reported first)
    if (fail_words[e] < (Word)INT_MAX)
      throw Error(MOE_ERR_SINGULAR,
                  "the covariance conditioned on points_being_sampled is singular: pending point " +
                      std::to_string((int)fail_words[e]) + " of the combined list repeats a pending or sampled point with 0 noise.",
                  e - T.E, (int)fail_words[e]);
  for (int e = 0; e < T.E; ++e)
    if (fail_words[e] < (Word)INT_MAX)
      throw Error(MOE_ERR_SINGULAR,
                  "GP-Variance matrix singular. Check for duplicate points_to_sample or points_to_sample "
                  "duplicating points_sampled with 0 noise.",
                  e, (int)fail_words[e]);
}

// One multistart ascent of an ensemble that is staged (stage(): the starts are T.dPts, the set phase has run, the pending points in
// use are the members' p): screening, the kept starts, the rounds, the end values.  Returns where the returned point lies in device
// memory, padded [dp] -- a greedy batch appends it to the pending points without a trip through the host.
const double* ascend(Kg1Ensemble& T, const moe_gd_params_t& outer, const double* starts, int num_starts, int do_gradient_ascent,
                     double* best_point, double* best_value, int* found, double* start_values, int* kept_index, double* end_points,
                     double* end_values, double* path, int* steps_taken) {
  GpDev& g0 = *T.gps[0];
  const int E = T.E, W = T.W, d = T.d, dp = T.dp, S = num_starts;
  const int R = std::max(outer.max_num_restarts, 0), Tn = outer.max_num_steps;
  const bool ascent = do_gradient_ascent != 0;
  const int Kmax = ascent ? std::min(S, kMaxKept) : 0;  // (top_k_order keeps at most 20)
  const int rows = R * Tn + 1;
  const bool want_path = ascent && path != nullptr;
  // the call's doubles: [words: failure W, steps Kmax | values S | X Kmax dp | path Kmax rows d] (the copies back) | X^, X_begin Kmax dp
  const size_t nWords = (size_t)W + Kmax, oVals = nWords, oX = oVals + S, oPath = oX + (size_t)Kmax * dp;
  const size_t nBack = oPath + (want_path ? (size_t)Kmax * rows * d : 0);
  hipStream_t z = T.z;
  double* dD = g0.kg1oD.p;
  double* dVals = dD + oVals;
  int* iCount = T.iFail + W;
  int* iSteps = iCount + 1;
  int* iOrder = iSteps + Kmax;
  double* h = g0.hStateOut.p;

  // screening: the value at every start
  Kg1Recording screen;
  evaluate(T, screen, T.dPts, T.dPtsH, S, false);
  launch_mean_of_members(T, T.dKgTab, S, dVals);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, z, (const int*)T.iFail, W, dD);
  MOE_HIP_CHECK(hipGetLastError());
  g0.kg1oD.download(h, oVals + S, z);
  MOE_HIP_CHECK(hipStreamSynchronize(z));
  throw_if_singular(T, h);
  const std::vector<double> vals(h + oVals, h + oVals + S);
  if (start_values) std::copy(vals.begin(), vals.end(), start_values);
  *found = 0;
  *best_value = -INFINITY;
  if (!ascent) {
    int best_s = 0;
    std::copy(starts, starts + d, best_point);  // seeded with the first point of the list, as multistart() does
    for (int s = 0; s < S; ++s)
      if (vals[s] > *best_value) {
        *best_value = vals[s];
        std::copy(starts + (size_t)s * d, starts + (size_t)(s + 1) * d, best_point);
        *found = 1;
        best_s = s;
      }
    return T.dPts + (size_t)best_s * dp;
  }

  // the kept starts in the reference's order, uploaded; their points gathered on the device
  const std::vector<int> order = top_k_order(vals.data(), S);
  const int K = (int)order.size();
  if (K > Kmax) throw Error(MOE_ERR_RUNTIME, "top_k_order kept more starts than the ascent has room for");
  std::copy(starts + (size_t)order[0] * d, starts + (size_t)(order[0] + 1) * d, best_point);
  const double* dBest = T.dPts + (size_t)order[0] * dp;
  int* hOrder = reinterpret_cast<int*>(g0.hStateIn.p);  // (the upload it carried has been waited for)
  std::copy(order.begin(), order.end(), hOrder);
  MOE_HIP_CHECK(hipMemcpyAsync(iOrder, hOrder, sizeof(int) * (size_t)K, hipMemcpyHostToDevice, z));
  Kg1Ascent a;
  a.K = K;
  a.E = E;
  a.d = d;
  a.dp = dp;
  a.size = d - T.nf;
  a.grad = T.dGradTab;
  a.bounds = T.dBounds;
  a.X = dD + oX;
  a.Xh = T.fid ? dD + nBack : a.X;
  a.Xbegin = dD + nBack + (size_t)Kmax * dp;
  a.count = iCount;
  a.steps = iSteps;
  a.running = iOrder + Kmax;
  a.alive = a.running + Kmax;
  a.path = want_path ? dD + oPath : nullptr;
  a.rows = rows;
  MOE_LAUNCH_NOW(kg1_gather_kernel, dim3(1), dim3(64), 0, z, a, (const int*)iOrder, T.dPts, T.dPtsH);
  MOE_HIP_CHECK(hipGetLastError());

  // the ascent: no host arithmetic and no wait between the steps of a round; one wait per round for the count of alive starts
  const double step_tol = outer.tolerance / (double)outer.max_num_steps;
  Kg1Recording step;
  int alive = K, rows_done = 0;
  int* hWords = reinterpret_cast<int*>(h);
  for (int r = 0; r < R && alive > 0; ++r) {
    for (int i = 0; i < Tn; ++i) {
      const double alpha = outer.pre_mult * std::pow((double)(i + 1), -outer.gamma);
      evaluate(T, step, a.X, a.Xh, K, true);
      MOE_LAUNCH_NOW(kg1_step_kernel, dim3(1), dim3(64), 0, z, a, alpha, outer.max_relative_change, step_tol, 1 + r * Tn + i);
    }
    MOE_LAUNCH_NOW(kg1_round_kernel, dim3(1), dim3(64), 0, z, a, outer.tolerance);
    MOE_HIP_CHECK(hipGetLastError());
    MOE_HIP_CHECK(hipMemcpyAsync(hWords, T.iFail, sizeof(int) * ((size_t)W + 1), hipMemcpyDeviceToHost, z));
    MOE_HIP_CHECK(hipStreamSynchronize(z));
    rows_done = (r + 1) * Tn;
    throw_if_singular(T, hWords);
    alive = hWords[W];
  }

  // the value at every end point, and everything back in one copy
  Kg1Recording last;
  evaluate(T, last, a.X, a.Xh, K, false);
  launch_mean_of_members(T, T.dKgTab, K, dVals);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, z, (const int*)T.iFail, W, dD);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, z, (const int*)iSteps, K, dD + W);
  MOE_HIP_CHECK(hipGetLastError());
  g0.kg1oD.download(h, nBack, z);
  MOE_HIP_CHECK(hipStreamSynchronize(z));
  throw_if_singular(T, h);
  for (int k = 0; k < K; ++k) {
    const double* xk = h + oX + (size_t)k * dp;
    if (kept_index) kept_index[k] = order[k];
    if (steps_taken) steps_taken[k] = (int)h[W + k];
    if (end_points) std::copy(xk, xk + d, end_points + (size_t)k * d);
    if (end_values) end_values[k] = h[oVals + k];
    if (want_path) {
      const double* pk = h + oPath + (size_t)k * rows * d;
      double* out = path + (size_t)k * rows * d;
      std::copy(pk, pk + (size_t)(1 + rows_done) * d, out);
      for (int row = 1 + rows_done; row < rows; ++row) std::copy(xk, xk + d, out + (size_t)row * d);  // (rounds that never ran)
    }
    if (h[oVals + k] > *best_value) {  // strict: the first of equal values wins
      *best_value = h[oVals + k];
      std::copy(xk, xk + d, best_point);
      *found = 1;
      dBest = a.X + (size_t)k * dp;
    }
  }
  return dBest;
}

}  // namespace

}  // namespace moe
