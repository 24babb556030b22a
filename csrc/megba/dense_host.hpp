// Dense Cholesky and triangular solves on the host: plain blocked C++ with
// OpenMP, no LAPACK.  The CPU engine's dense Schur route (the oracle of the
// GPU kernels in gpu/dense_chol.hip) is built on these.
//
// Matrices are row-major with leading dimension ld; only the lower triangle
// is read and written.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "engine.hpp"

namespace megba {

// The pivot rule of every dense factorization here: d is the pivot L_ii^2
// after elimination, s the entry S_ii before it.
inline bool densePivotFails(double d, double s, double pivotTol) {
  return !std::isfinite(d) || !(d > 0.0) || d < pivotTol * s;
}

// A = L L^T in place (right-looking, NB-wide panels).  Stops at the first
// failing pivot; the rows before it are factored.
inline DenseFactorInfo denseCholeskyHost(double* A, int64_t n, int64_t ld,
                                         double pivotTol, int nThreads) {
  constexpr int64_t NB = 64;
  (void)nThreads;
  DenseFactorInfo info;
  info.minPivotRatio = 1.0;
  std::vector<double> diag0(n);
  for (int64_t i = 0; i < n; ++i) diag0[i] = A[i * ld + i];
  for (int64_t k0 = 0; k0 < n; k0 += NB) {
    const int64_t k1 = std::min(k0 + NB, n);
    // diagonal block; earlier panels are already subtracted
    for (int64_t j = k0; j < k1; ++j) {
      double* rj = A + j * ld;
      double d = rj[j];
      for (int64_t t = k0; t < j; ++t) d -= rj[t] * rj[t];
      const double ratio = d / diag0[j];
      if (densePivotFails(d, diag0[j], pivotTol)) {
        info.failRow = j;
        info.failPivotRatio = ratio;
        return info;
      }
      info.minPivotRatio = std::min(info.minPivotRatio, ratio);
      const double l = std::sqrt(d);
      rj[j] = l;
      for (int64_t i = j + 1; i < k1; ++i) {
        double* ri = A + i * ld;
        double v = ri[j];
        for (int64_t t = k0; t < j; ++t) v -= ri[t] * rj[t];
        ri[j] = v / l;
      }
    }
    // panel below the block, then the trailing update, one row at a time
#pragma omp parallel for num_threads(nThreads) schedule(dynamic, 8)
    for (int64_t i = k1; i < n; ++i) {
      double* ri = A + i * ld;
      for (int64_t j = k0; j < k1; ++j) {
        const double* rj = A + j * ld;
        double v = ri[j];
        for (int64_t t = k0; t < j; ++t) v -= ri[t] * rj[t];
        ri[j] = v / rj[j];
      }
    }
#pragma omp parallel for num_threads(nThreads) schedule(dynamic, 8)
    for (int64_t i = k1; i < n; ++i) {
      double* ri = A + i * ld;
      for (int64_t c = k1; c <= i; ++c) {
        const double* rc = A + c * ld;
        double v = 0.0;
        for (int64_t t = k0; t < k1; ++t) v += ri[t] * rc[t];
        ri[c] -= v;
      }
    }
  }
  info.ok = true;
  return info;
}

// X := (L L^T)^-1 X for the k columns of X (n x k row-major).
inline void denseCholSolveHost(const double* L, int64_t n, int64_t ld,
                               double* X, int k) {
  for (int64_t i = 0; i < n; ++i) {
    const double* li = L + i * ld;
    double* xi = X + i * k;
    for (int64_t t = 0; t < i; ++t) {
      const double l = li[t];
      if (l == 0.0) continue;
      const double* xt = X + t * k;
      for (int c = 0; c < k; ++c) xi[c] -= l * xt[c];
    }
    for (int c = 0; c < k; ++c) xi[c] /= li[i];
  }
  for (int64_t i = n - 1; i >= 0; --i) {
    const double* li = L + i * ld;
    double* xi = X + i * k;
    for (int c = 0; c < k; ++c) xi[c] /= li[i];
    for (int64_t t = 0; t < i; ++t) {
      const double l = li[t];
      if (l == 0.0) continue;
      double* xt = X + t * k;
      for (int c = 0; c < k; ++c) xt[c] -= l * xi[c];
    }
  }
}

}  // namespace megba
