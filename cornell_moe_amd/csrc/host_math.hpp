// cornell_moe_amd/csrc/host_math.hpp -- the O(m^3) "small" posterior algebra that stays on the host.
//
// Everything that touches the N training rows runs on the GPU and arrives here already contracted into
//   gram = (L^-1 E)^T (L^-1 E)   (c x c)   and   ek = E^T K^-1(y - mean)   (c),
// where the columns of E are  [ K*(X, U) | d K*/d U | K(X, extra points) ]  (StateLayout below).  From those and a
// handful of direct covariance evaluations between the <= (q+p) query points, this file assembles the posterior mean,
// variance, their spatial gradients, the Cholesky factor of the variance and its Smith-1995 derivative -- the m x m
// objects of PointsToSampleState / KnowledgeGradientState (gpp_math.cpp:662-678, 721-726, 924-970, 1267-1474).
#pragma once
#include <vector>

#include "kernels.hpp"

namespace moe {

struct StateLayout {
  int d = 0;   // dim
  int u = 0;   // points in the state (num_union)
  int gt = 0;  // derivative observations carried by each of those points
  int m = 0;   // u * (1 + gt)
  int nd = 0;  // number of leading points differentiated against (num_derivatives)
  int A = 0;   // extra plain points (no derivative blocks)
  int c() const { return m + nd * (1 + gt) * d + A; }
  int col_kstar(int j, int b) const { return j * (1 + gt) + b; }
  int col_grad(int i, int a, int dd) const { return m + (i * (1 + gt) + a) * d + dd; }
};

struct StateHost {
  StateLayout lay;
  CovParams cp;
  DerivList dt;               // derivative list of the state's points
  std::vector<double> U;      // [u][d]
  std::vector<double> extra;  // [A][d]
  std::vector<double> gram;   // [c][c] col-major (symmetric)
  std::vector<double> ek;     // [c]
  double mean = 0.0;
  double G(int i, int j) const { return gram[(size_t)i + (size_t)j * lay.c()]; }
};

// cov(p1,p2) block [(1+g1) x (1+g2)] col-major and its gradient wrt p1 [d][(1+g1)][(1+g2)] on the host.
void host_cov(const CovParams& cp, const double* p1, const DerivList& d1, const double* p2, const DerivList& d2, double* out);
void host_grad_cov(const CovParams& cp, const double* p1, const DerivList& d1, const double* p2, const DerivList& d2,
                   double* out);

// ComputeMeanOfPoints / ComputeMeanOfAdditionalPoints (gpp_math.cpp:662-710): mu[m]
void host_mean(const StateHost& s, double* mu);
// ComputeGradMeanOfPoints (gpp_math.cpp:721-726): out[nd*(1+gt)][d]
void host_grad_mean(const StateHost& s, double* out);
// ComputeVarianceOfPoints (gpp_math.cpp:924-970): var[m][m] col-major, fully populated
void host_variance(const StateHost& s, double* var);
// ComputeGradVarianceOfPointsPerPoint (gpp_math.cpp:1267-1357): gv[d + row*d + col*d*m]
void host_grad_variance_per_point(const StateHost& s, int p, double* gv);
// ComputeCholeskyFactorL (gpp_linear_algebra.cpp:109-148): returns 0 or failing pivot index + 1
int host_cholesky(int n, double* a);
// ComputeGradCholeskyVarianceOfPointsPerPoint (gpp_math.cpp:1389-1452)
void host_grad_cholesky_per_point(const StateHost& s, int p, const double* chol, double* gc);
// lower-triangular solves on m x m factors: x <- L^-1 x / L^-T x
void host_tri_solve(const double* L, char trans, int n, double* x);

}  // namespace moe
