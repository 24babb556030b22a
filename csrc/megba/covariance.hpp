// Marginal covariances of cameras and points (device-agnostic host code over
// Engine<T>, like lm.hpp).
//
// The covariance of a set of vertices is the matching sub-matrix of H^-1,
// H = J^T W J plus the prior terms: the Gauss-Newton Hessian the LM step
// uses, robust-loss IRLS weights and information matrices included.
// solveLinear already solves H dx = g through the Schur complement, so with
// g = e_j and no damping dx is column j of H^-1, and its entries at the
// requested vertices are the wanted covariance and cross-covariance entries.
// One vertex block of dimension D costs D solves; no dense S is formed and
// every tuned product path carries the solves unchanged.  With batch > 1 the
// columns of a block are solved together where the engine has a batched
// product (Engine::solveUnitBatch): they share every pass over J.
//
// The result is the covariance under unit-variance weighted residuals.
// Scaling by a variance factor chi^2 / dof is left to the caller.
//
// H must be positive definite: the gauge has to be fixed by priors or fixed
// vertices.  Without a datum the PCG does not converge, which the
// `converged` flags (or the strict error) report.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "common.hpp"
#include "engine.hpp"

namespace megba {

struct CovarianceResult {
  int n = 0;                   // camDim * #cams + ptDim * #pts
  std::vector<double> joint;   // n x n row-major, cameras first, symmetrised
  std::vector<int> iters;      // PCG iterations per column (0: fixed vertex)
  std::vector<uint8_t> converged;  // per column (1 for a fixed vertex)
  double asymmetry = 0.0;      // max|A - A^T| / max|A| before symmetrising
  // Schur products S p the engine applied during the call (PCG iterations
  // and initial residuals; a batched application counts once)
  int64_t products = 0;
};

struct CovarianceOption {
  double tol = 1e-10;  // relative residual; the PCG stops on rho/rho_0 < tol^2
  int maxIter = 2000;
  bool strict = true;  // raise if a column does not converge
  // Columns solved together, at most: the non-fixed columns of a vertex block
  // go to Engine::solveUnitBatch in groups of min(batch, maxBatch()); a
  // group never spans two vertices.  1 is the column loop.  An engine
  // without a batched product (the CPU engine: maxBatch() == 1) accepts any
  // batch and runs the column loop.
  int batch = 1;
};

// COLLECTIVE when worldSize>1: every rank calls it with the same arguments
// and gets the same result.  Leaves the engine's g and deltaX, and with them
// a running LM session, as they were.
inline CovarianceResult computeCovariance(Engine<double>& eng,
                                          const std::vector<int>& camIds,
                                          const std::vector<int>& ptIds,
                                          const CovarianceOption& opt = {}) {
  const EngineShape sh = eng.shape();
  MEGBA_CHECK(!camIds.empty() || !ptIds.empty(),
              "covariance: no vertices requested");
  MEGBA_CHECK(opt.tol > 0.0 && opt.maxIter > 0,
              "covariance: tol and max_iter must be positive");
  MEGBA_CHECK(opt.batch >= 1, "covariance: batch must be at least 1");
  const auto checkIds = [](const std::vector<int>& ids, int count,
                           const char* what) {
    std::vector<int> sorted(ids);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < sorted.size(); ++i) {
      MEGBA_CHECK(sorted[i] >= 0 && sorted[i] < count,
                  std::string("covariance: ") + what + " id " +
                      std::to_string(sorted[i]) + " out of range");
      MEGBA_CHECK(i == 0 || sorted[i] != sorted[i - 1],
                  std::string("covariance: duplicate ") + what + " id " +
                      std::to_string(sorted[i]));
    }
  };
  checkIds(camIds, sh.ncam, "camera");
  checkIds(ptIds, sh.npt, "point");

  // Global rows of the requested blocks, and which of them belong to a fixed
  // vertex (zero rows and columns, no solve: the engine gives a fixed vertex
  // an identity block, so a unit solve on it would return the unit vector).
  std::vector<int64_t> rows;
  std::vector<uint8_t> fixedRow;
  for (int c : camIds)
    for (int i = 0; i < sh.camDim; ++i) {
      rows.push_back((int64_t)sh.camDim * c + i);
      fixedRow.push_back(eng.isFixed(true, c));
    }
  const int64_t nc = (int64_t)sh.camDim * sh.ncam;
  for (int p : ptIds)
    for (int i = 0; i < sh.ptDim; ++i) {
      rows.push_back(nc + (int64_t)sh.ptDim * p + i);
      fixedRow.push_back(eng.isFixed(false, p));
    }
  const int n = (int)rows.size();

  CovarianceResult res;
  res.n = n;
  res.joint.assign((size_t)n * n, 0.0);
  res.iters.assign(n, 0);
  res.converged.assign(n, 1);

  // Relinearise at the current parameters.  After a rejected LM step they
  // are already rolled back to the accepted point, so this reproduces the
  // accepted system.
  eng.forward();
  eng.acceptForward();
  eng.buildLinearSystem();
  eng.saveLinearState();

  SolverOptionPCG sopt;
  sopt.maxIter = opt.maxIter;
  sopt.tol = 0.0;
  sopt.refuseRatio = 1e30;
  sopt.relTol = opt.tol * opt.tol;
  sopt.refuseJitter = true;
  std::vector<double> col(n);
  const int64_t productsBefore = eng.productCount();
  const int width = std::min(opt.batch, eng.maxBatch());
  try {
    // 1 + 1/region is exactly 1: no damping
    eng.processDiag(std::numeric_limits<double>::infinity());
    if (width <= 1) {
      for (int j = 0; j < n; ++j) {
        if (fixedRow[j]) continue;
        eng.setUnitRhs(rows[j]);
        res.iters[j] = eng.solveLinear(sopt);
        res.converged[j] = eng.relStopHit();
        eng.readDeltaXRows(rows.data(), n, col.data());
        for (int i = 0; i < n; ++i)
          res.joint[(size_t)i * n + j] = fixedRow[i] ? 0.0 : col[i];
      }
    } else {
      // the columns of one vertex block, `width` at a time
      std::vector<double> cols;
      std::vector<uint8_t> conv(width);
      for (int first = 0; first < n;) {
        const int dim = first < sh.camDim * (int)camIds.size() ? sh.camDim
                                                               : sh.ptDim;
        for (int j = first; j < first + dim && !fixedRow[first]; j += width) {
          const int k = std::min(width, first + dim - j);
          cols.assign((size_t)n * k, 0.0);
          eng.solveUnitBatch(rows.data() + j, k, sopt, rows.data(), n,
                             cols.data(), res.iters.data() + j, conv.data());
          for (int c = 0; c < k; ++c) {
            res.converged[j + c] = conv[c];
            for (int i = 0; i < n; ++i)
              res.joint[(size_t)i * n + j + c] =
                  fixedRow[i] ? 0.0 : cols[(size_t)i * k + c];
          }
        }
        first += dim;
      }
    }
  } catch (...) {
    eng.restoreLinearState();
    throw;
  }
  eng.restoreLinearState();
  res.products = eng.productCount() - productsBefore;

  double maxAbs = 0.0, maxAsym = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      const double a = res.joint[(size_t)i * n + j];
      const double b = res.joint[(size_t)j * n + i];
      maxAbs = std::max(maxAbs, std::fabs(a));
      maxAsym = std::max(maxAsym, std::fabs(a - b));
    }
  res.asymmetry = maxAbs > 0.0 ? maxAsym / maxAbs : 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const double m =
          0.5 * (res.joint[(size_t)i * n + j] + res.joint[(size_t)j * n + i]);
      res.joint[(size_t)i * n + j] = res.joint[(size_t)j * n + i] = m;
    }

  if (opt.strict)
    for (int j = 0; j < n; ++j)
      MEGBA_CHECK(res.converged[j],
                  "covariance: column " + std::to_string(j) +
                      " did not converge in " + std::to_string(opt.maxIter) +
                      " iterations (is the gauge fixed by priors or fixed "
                      "vertices?)");
  return res;
}

}  // namespace megba
