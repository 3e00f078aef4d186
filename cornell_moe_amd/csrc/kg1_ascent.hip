// cornell_moe_amd/csrc/kg1_ascent.hip -- what the ensemble forms of the one-point acquisition functions share (kg1_opt.hip: the
// discretised knowledge gradient; ei1.hip: the analytic expected improvement; gibbon1.hip: the min-value entropy acquisition;
// cei1.hip: the constrained expected improvement; ehvi1.hip: the expected hypervolume improvement; logcei1.hip: the log of the
// constrained expected improvement), compiled once: the ensemble mean, the multistart
// ascent's gather, step and round kernels, the recorded and zipped evaluation of the members' chains, the ascent itself (ascend()),
// the staging of a call (stage(), stage_ascent()) and the three drivers behind the entry points (kg1_ascent.hpp).  None of it knows
// the objective: a Kg1Objective says how a member is built, which chain evaluates it and what follows its extension.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "kg1_ascent.hpp"

namespace moe {

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

// out[e][i] = src[e][i]: every member's own values side by side for the copy back (blockIdx.y: the member)
__global__ __launch_bounds__(256) void kg1_members_kernel(long n, const double* const* __restrict__ src, double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[(size_t)blockIdx.y * n + i] = src[blockIdx.y][i];
}

// the words of the call as doubles in front of the results: one copy back
__global__ __launch_bounds__(256) void kg1_words_kernel(const int* __restrict__ words, int n, double* __restrict__ out) {
  for (int i = threadIdx.x; i < n; i += 256) out[i] = (double)words[i];
}

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

// the ensemble's value at C points from the members' results: the objective's own rule, or the mean of the members
void launch_value_of_members(const Kg1Ensemble& T, int C, double* out) {
  if (T.combine != nullptr)
    T.combine(T, C, out, nullptr);
  else
    launch_mean_of_members(T, T.dKgTab, C, out);
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

// The members' layouts and the one upload:
//   [value pointers E | grad pointers E | bounds 2 d | set of member 0 .. E - 1, padded | points C dp | the same, fidelity 1 (fid) |
//    pending points pcap dp | the members' extra doubles E num_member_extra | the address of the combined gradient (T.combine)]
// (an objective without sets, fidelity coordinates, extra doubles or a rule of its own leaves those sections empty); then every member's extension by
// the first p pending points and what the objective runs behind it.  extra_ints: integers of the caller behind the W failure words in the first
// member's kg1oI.
void stage(Kg1Ensemble& T, const Kg1Objective& o, const double* bounds, const double* pts, int C, bool with_grad, size_t extra_ints,
           const double* pending, int p) {
  GpDev& g0 = *T.gps[0];
  const int E = T.E, d = T.d, dp = T.dp, size = d - T.nf, pcap = T.pcap;
  g0.kg1oI.reserve((size_t)T.W + extra_ints);
  T.iFail = g0.kg1oI.p;
  const double* discrete_all = o.discrete_all;
  const int* num_discrete = o.num_discrete;
  size_t nSets = 0;
  for (int e = 0; e < E && num_discrete != nullptr; ++e) nSets += (size_t)num_discrete[e];
  const size_t nC = (size_t)C, oBounds = 2 * (size_t)E, oSets = oBounds + 2 * (size_t)d, oPts = oSets + nSets * dp;
  const size_t oPend = oPts + nC * dp * (T.fid ? 2 : 1);
  const size_t nX = o.member_extra != nullptr ? (size_t)o.num_member_extra : 0, oExtra = oPend + (size_t)pcap * dp;
  const size_t oComb = oExtra + (size_t)E * nX, nIn = oComb + (T.combine != nullptr ? 1 : 0);
  g0.hStateIn.reserve(nIn);
  g0.dStateIn.reserve(nIn);
  T.mem.clear();
  for (int e = 0; e < E; ++e)
    T.mem.push_back(o.member(o, *T.gps[e], e, C, with_grad, T.iFail + e, pcap, pcap > 0 ? T.iFail + E + e : nullptr));
  double* h = g0.hStateIn.p;
  static_assert(sizeof(const double*) == sizeof(double), "the pointer tables travel inside a buffer of doubles");
  for (int e = 0; e < E; ++e) {
    const double* pk = T.mem[e].dKg;
    const double* pg = T.mem[e].dGrad;
    std::memcpy(h + e, &pk, sizeof(pk));
    std::memcpy(h + E + e, &pg, sizeof(pg));
  }
  for (int k = 0; k < 2 * d; ++k) h[oBounds + k] = bounds != nullptr ? bounds[k] : 0.0;
  const double* dIn = g0.dStateIn.p;
  size_t row = 0;
  for (int e = 0; e < E && num_discrete != nullptr; ++e) {
    T.mem[e].dPA = dIn + oSets + row * dp;
    for (size_t i = 0; i < (size_t)num_discrete[e]; ++i, ++row)
      for (int k = 0; k < dp; ++k) h[oSets + row * dp + k] = (k < size) ? discrete_all[row * size + k] : (k < d ? 1.0 : 0.0);
  }
  for (size_t i = 0; i < nC; ++i)
    for (int k = 0; k < dp; ++k) {
      const double v = (k < d) ? pts[i * d + k] : 0.0;
      h[oPts + i * dp + k] = v;
      if (T.fid) h[oPts + (nC + i) * dp + k] = (k >= size && k < d) ? 1.0 : v;
    }
  for (size_t i = 0; i < (size_t)pcap; ++i)  // (the pending points as given, fidelity coordinates included; the rest joins on the device)
    for (int k = 0; k < dp; ++k) h[oPend + i * dp + k] = (i < (size_t)p && k < d) ? pending[i * d + k] : 0.0;
  if (nX > 0) std::memcpy(h + oExtra, o.member_extra, sizeof(double) * (size_t)E * nX);
  for (int e = 0; e < E && nX > 0; ++e) {
    T.mem[e].dExtra = dIn + oExtra + (size_t)e * nX;
    T.mem[e].nExtra = (int)nX;
  }
  if (T.combine != nullptr) {
    const double* pc = T.dComb;
    std::memcpy(h + oComb, &pc, sizeof(pc));
    T.dCombTab = reinterpret_cast<const double* const*>(dIn + oComb);
  }
  g0.dStateIn.upload(h, nIn, T.z, true);
  T.dPending = g0.dStateIn.p + oPend;
  T.dKgTab = reinterpret_cast<const double* const*>(dIn);
  T.dGradTab = reinterpret_cast<const double* const*>(dIn + E);
  T.dBounds = dIn + oBounds;
  T.dPts = dIn + oPts;
  T.dPtsH = T.fid ? T.dPts + nC * dp : T.dPts;
  kg1_clear_fail(T.iFail, E, T.z);
  if (pcap > 0) kg1_clear_fail(T.iFail + E, E, T.z);
  for (Kg1Member& m : T.mem) {
    if (pcap > 0) {
      m.dPP = T.dPending;
      kg1_pending_begin(m, T.z);
      if (p > 0) kg1_pending_append(m, p, false, T.z);
    }
    if (o.member_extended != nullptr) o.member_extended(m, T.z);
  }
  if (o.all_extended != nullptr) o.all_extended(T, p);
  T.p = p;
}

// The buffers of ascend() -- T.sz, the one place their sizes are worked out -- and the one upload.  The call's doubles:
//   [words: failure W, steps Kmax | values S | X Kmax dp | path Kmax rows d] (the copies back) | X^, X_begin Kmax dp |
//   the combined gradient Kmax d (T.combine)
// and its integers behind the failure words: [alive count | steps Kmax | order, running, alive Kmax each].
void stage_ascent(Kg1Ensemble& T, const Kg1Objective& o, const moe_gd_params_t& outer, const double* domain_bounds,
                  const double* starts, int S, bool ascent, bool want_path, const double* pending, int p) {
  GpDev& g0 = *T.gps[0];
  const int R = std::max(outer.max_num_restarts, 0);
  Kg1AscentSizes& sz = T.sz;
  sz.Kmax = ascent ? std::min(S, kMaxKept) : 0;  // (top_k_order keeps at most 20)
  sz.rows = R * outer.max_num_steps + 1;
  sz.want_path = want_path;
  sz.oVals = (size_t)T.W + sz.Kmax;
  sz.oX = sz.oVals + S;
  sz.oPath = sz.oX + (size_t)sz.Kmax * T.dp;
  sz.nBack = sz.oPath + (want_path ? (size_t)sz.Kmax * sz.rows * T.d : 0);
  const size_t oComb = sz.nBack + 2 * (size_t)sz.Kmax * T.dp;
  g0.kg1oD.reserve(oComb + (T.combine != nullptr ? (size_t)sz.Kmax * T.d : 0));
  g0.hStateOut.reserve(sz.nBack);
  if (T.combine != nullptr) T.dComb = g0.kg1oD.p + oComb;
  stage(T, o, domain_bounds, starts, S, ascent && R > 0, 1 + 4 * (size_t)sz.Kmax, pending, p);
}

// One multistart ascent of an ensemble that is staged (stage_ascent(): the starts are T.dPts, the objective's set phase has run, the
// pending points in use are the members' p): screening, the kept starts, the rounds, the end values.  Returns where the returned point
// lies in device memory, padded [dp] -- a greedy batch appends it to the pending points without a trip through the host.
const double* ascend(Kg1Ensemble& T, const moe_gd_params_t& outer, const double* starts, int num_starts, int do_gradient_ascent,
                     const Kg1MultistartOut& out) {
  double* const best_point = out.best_point;
  double* const best_value = out.best_value;
  int* const found = out.found;
  GpDev& g0 = *T.gps[0];
  const int E = T.E, W = T.W, d = T.d, dp = T.dp, S = num_starts;
  const int R = std::max(outer.max_num_restarts, 0), Tn = outer.max_num_steps;
  const bool ascent = do_gradient_ascent != 0;
  const int Kmax = T.sz.Kmax, rows = T.sz.rows;
  const bool want_path = T.sz.want_path;
  const size_t oVals = T.sz.oVals, oX = T.sz.oX, oPath = T.sz.oPath, nBack = T.sz.nBack;
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
  launch_value_of_members(T, S, dVals);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, z, (const int*)T.iFail, W, dD);
  MOE_HIP_CHECK(hipGetLastError());
  g0.kg1oD.download(h, oVals + S, z);
  MOE_HIP_CHECK(hipStreamSynchronize(z));
  throw_if_singular(T, h);
  const std::vector<double> vals(h + oVals, h + oVals + S);
  if (out.start_values) std::copy(vals.begin(), vals.end(), out.start_values);
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
  a.E = T.combine != nullptr ? 1 : E;  // (the objective's own rule leaves ONE gradient, already divided: g / 1 is exact)
  a.d = d;
  a.dp = dp;
  a.size = d - T.nf;
  a.grad = T.combine != nullptr ? T.dCombTab : T.dGradTab;
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
      if (T.combine != nullptr) T.combine(T, K, nullptr, T.dComb);
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
  launch_value_of_members(T, K, dVals);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, z, (const int*)T.iFail, W, dD);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, z, (const int*)iSteps, K, dD + W);
  MOE_HIP_CHECK(hipGetLastError());
  g0.kg1oD.download(h, nBack, z);
  MOE_HIP_CHECK(hipStreamSynchronize(z));
  throw_if_singular(T, h);
  for (int k = 0; k < K; ++k) {
    const double* xk = h + oX + (size_t)k * dp;
    if (out.kept_index) out.kept_index[k] = order[k];
    if (out.steps_taken) out.steps_taken[k] = (int)h[W + k];
    if (out.end_points) std::copy(xk, xk + d, out.end_points + (size_t)k * d);
    if (out.end_values) out.end_values[k] = h[oVals + k];
    if (want_path) {
      const double* pk = h + oPath + (size_t)k * rows * d;
      double* path_k = out.path + (size_t)k * rows * d;
      std::copy(pk, pk + (size_t)(1 + rows_done) * d, path_k);
      for (int row = 1 + rows_done; row < rows; ++row) std::copy(xk, xk + d, path_k + (size_t)row * d);  // (rounds that never ran)
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

Kg1Ensemble::Kg1Ensemble(const std::vector<GpDev*>& members, const Kg1Objective& o, int pending_room)
    : gps(members), z(members[0]->stream), ens(ensemble_launches() && members.size() > 1), E((int)members.size()), d(members[0]->d),
      dp(members[0]->dp), nf(o.nf), eval_points(o.eval_points), fid(o.nf > 0), pcap(pending_room), W(pending_room > 0 ? 2 * E : E) {
  if (o.combine != nullptr && (o.group > 1 || o.combine_single_groups)) {
    if (E % std::max(o.group, 1) != 0) throw Error(MOE_ERR_RUNTIME, "the members do not fill their groups");
    combine = o.combine;
    group = std::max(o.group, 1);
    group_values = o.group_values;
    group_value_rows = std::max(o.group_value_rows, 1);
  }
  client = o.client;
  gps[0]->use_device();
}

void kg1_check_members(const std::vector<GpDev*>& gps, int nf, void (*check_member)(const GpDev& g, const GpDev& g0, size_t e, int nf)) {
  const GpDev* g0 = gps[0];
  if (nf >= g0->d) throw Error(MOE_ERR_BOUNDS, "num_fidelity out of range", nf, 0, g0->d - 1);
  for (size_t e = 0; e < gps.size(); ++e) {
    const GpDev* g = gps[e];
    if (g->d != g0->d) throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must share dim", g->d, g0->d, (double)e);
    if (g->device != g0->device)
      throw Error(MOE_ERR_INVALID_VALUE, "MCMC ensemble members must live on one device", g->device, g0->device, (double)e);
  }
  for (size_t e = 0; e < gps.size(); ++e) {
    check_member(*gps[e], *g0, e, nf);
    for (size_t f = 0; f < e; ++f)
      if (gps[f] == gps[e])
        throw Error(MOE_ERR_INVALID_VALUE, "an MCMC ensemble member is listed twice (every member keeps its own workspaces)", (double)e,
                    (double)f, 0);
  }
}

void kg1_ensemble_evaluate(const Kg1Objective& o, const std::vector<GpDev*>& gps, const double* pts, int C, bool want_grad,
                           double* value_out, double* grad_out, const double* pending, int num_pending, double* members_out) {
  Kg1Ensemble T(gps, o, num_pending);
  GpDev& g0 = *gps[0];
  const int d = T.d, W = T.W;
  // the call's doubles, all of them the copy back: [failure words | value C | grad C d | the members' values E C (members_out)]
  const size_t oMem = (size_t)W + (size_t)C * (want_grad ? 1 + d : 1);
  const size_t nMem = (size_t)(T.group_values ? (T.E / T.group) * T.group_value_rows : T.E) * C;
  const size_t nOut = oMem + (members_out != nullptr ? nMem : 0);
  g0.kg1oD.reserve(nOut);
  g0.hStateOut.reserve(nOut);
  stage(T, o, nullptr, pts, C, want_grad, 0, pending, num_pending);
  Kg1Recording rec;
  evaluate(T, rec, T.dPts, T.dPtsH, C, want_grad);
  double* dOut = g0.kg1oD.p;
  if (T.combine != nullptr) {
    T.combine(T, C, dOut + W, want_grad ? dOut + W + C : nullptr);
  } else {
    launch_mean_of_members(T, T.dKgTab, C, dOut + W);
    if (want_grad) launch_mean_of_members(T, T.dGradTab, (long)C * d, dOut + W + C);
  }
  if (members_out != nullptr && T.group_values)  // (the objective's combine has left its groups' values side by side)
    copy_async(dOut + oMem, T.dGroupVals, sizeof(double) * nMem, hipMemcpyDeviceToDevice, T.z);
  else if (members_out != nullptr)
    MOE_LAUNCH_NOW(kg1_members_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)T.E), dim3(256), 0, T.z, (long)C, T.dKgTab,
                   dOut + oMem);
  MOE_LAUNCH_NOW(kg1_words_kernel, dim3(1), dim3(256), 0, T.z, (const int*)T.iFail, W, dOut);
  MOE_HIP_CHECK(hipGetLastError());
  g0.kg1oD.download(g0.hStateOut.p, nOut, T.z);
  MOE_HIP_CHECK(hipStreamSynchronize(T.z));
  const double* out = g0.hStateOut.p;
  throw_if_singular(T, out);
  std::memcpy(value_out, out + W, sizeof(double) * (size_t)C);
  if (want_grad) std::memcpy(grad_out, out + W + C, sizeof(double) * (size_t)C * d);
  if (members_out != nullptr) std::memcpy(members_out, out + oMem, sizeof(double) * nMem);
}

void kg1_ensemble_multistart(const Kg1Objective& o, const std::vector<GpDev*>& gps, const moe_gd_params_t& outer,
                             const double* domain_bounds, const double* starts, int num_starts, int do_gradient_ascent,
                             const double* pending, int num_pending, const Kg1MultistartOut& out) {
  Kg1Ensemble T(gps, o, num_pending);
  const bool ascent = do_gradient_ascent != 0;
  stage_ascent(T, o, outer, domain_bounds, starts, num_starts, ascent, ascent && out.path != nullptr, pending, num_pending);
  ascend(T, outer, starts, num_starts, do_gradient_ascent, out);
}

// q points greedily: round t is the ascent above with the caller's pending points and the t points already picked; the staging
// runs once, a round appends one column to every member's extension (and what the objective keeps beside it).
void kg1_ensemble_suggest(const Kg1Objective& o, const std::vector<GpDev*>& gps, const moe_gd_params_t& outer,
                          const double* domain_bounds, const double* starts, int num_starts, int do_gradient_ascent,
                          const double* pending, int num_pending, int num_to_sample, const Kg1BatchOut& out) {
  Kg1Ensemble T(gps, o, num_pending + num_to_sample - 1);
  stage_ascent(T, o, outer, domain_bounds, starts, num_starts, do_gradient_ascent != 0, false, pending, num_pending);
  const int d = T.d;
  for (int t = 0; t < num_to_sample; ++t) {
    Kg1MultistartOut round;
    round.best_point = out.best_points + (size_t)t * d;
    round.best_value = out.best_values + t;
    round.found = out.found + t;
    const double* dBest = ascend(T, outer, starts, num_starts, do_gradient_ascent, round);
    if (t + 1 == num_to_sample) break;
    copy_async(T.dPending + (size_t)T.p * T.dp, dBest, sizeof(double) * (size_t)T.dp, hipMemcpyDeviceToDevice, T.z);
    o.pick_appended(T);
    T.p += 1;
  }
}

}  // namespace moe
