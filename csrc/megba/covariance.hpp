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
// CovarianceMethod::Dense takes the direct route instead: the engine forms S
// as a dense matrix, factors it once with a Cholesky
// (Engine::denseSchurFactor) and solves the columns of a block exactly
// (Engine::solveUnitDense).
//
// The result is the covariance under unit-variance weighted residuals.
// Scaling by a variance factor chi^2 / dof is left to the caller.
//
// H must be positive definite: the gauge has to be fixed by priors or fixed
// vertices.  Without a datum the PCG does not converge, which the
// `converged` flags (or the strict error) report; the dense route fails a
// pivot and reports the whole system singular.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "common.hpp"
#include "engine.hpp"

namespace megba {

enum class CovarianceMethod { Pcg, Dense };

struct CovarianceResult {
  int n = 0;                   // camDim * #cams + ptDim * #pts
  // n x n row-major, cameras first, symmetrised; empty with cross = false
  std::vector<double> joint;
  // cross = false: the vertices' own blocks one after the other, cameras
  // first (camDim^2 values each, then ptDim^2 each), symmetrised
  std::vector<double> blocks;
  std::vector<int> iters;      // PCG iterations per column (0: fixed vertex)
  std::vector<uint8_t> converged;  // per column (1 for a fixed vertex)
  double asymmetry = 0.0;      // max|A - A^T| / max|A| before symmetrising
  // Schur products S p the engine applied during the call (PCG iterations
  // and initial residuals; a batched application counts once)
  int64_t products = 0;
  CovarianceMethod method = CovarianceMethod::Pcg;
  // Dense: min over the rows of L_ii^2 / S_ii; NaN for Pcg
  double minPivotRatio = std::numeric_limits<double>::quiet_NaN();
  // Dense: milliseconds of forming S, of factoring it (trailingMs of them in
  // the trailing-update kernel, -1 if not profiled) and of all block solves
  double formMs = 0.0, factorMs = 0.0, trailingMs = -1.0, solveMs = 0.0;
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
  // Pcg: one Schur PCG solve per column (the default).  Dense: form the
  // camera system S as a dense matrix, factor it once with a Cholesky
  // (Engine::denseSchurFactor, 8 (camDim ncam)^2 bytes) and solve every
  // column exactly; tol, maxIter and batch are ignored.  Prefer it with few
  // cameras, a tight tolerance or many requested vertices.
  CovarianceMethod method = CovarianceMethod::Pcg;
  // Dense: a pivot below pivotTol * S_ii fails the factorization.  The
  // relative error of a solve grows like eps / ratio; below sqrt(eps) fewer
  // than half the digits survive.
  double pivotTol = 1.4901161193847656e-08;  // sqrt(DBL_EPSILON)
  // false: every block is solved against its own rows only; `blocks` is
  // filled and `joint` stays empty (no cross-covariances).
  bool cross = true;
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
  const bool dense = opt.method == CovarianceMethod::Dense;

  CovarianceResult res;
  res.n = n;
  res.method = opt.method;
  if (opt.cross) res.joint.assign((size_t)n * n, 0.0);
  res.iters.assign(n, 0);
  res.converged.assign(n, 1);
  // offset of every vertex block in res.blocks
  std::vector<size_t> blockAt;
  if (!opt.cross) {
    size_t at = 0;
    for (int first = 0; first < n;) {
      const int dim = first < sh.camDim * (int)camIds.size() ? sh.camDim
                                                             : sh.ptDim;
      blockAt.push_back(at);
      at += (size_t)dim * dim;
      first += dim;
    }
    res.blocks.assign(at, 0.0);
  }

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
  const int64_t productsBefore = eng.productCount();
  const int width = dense ? 1 : std::min(opt.batch, eng.maxBatch());
  DenseFactorInfo factor;
  factor.ok = true;
  try {
    // 1 + 1/region is exactly 1: no damping
    eng.processDiag(std::numeric_limits<double>::infinity());
    if (dense) {
      factor = eng.denseSchurFactor(opt.pivotTol);
      res.minPivotRatio = factor.minPivotRatio;
      res.formMs = factor.formMs;
      res.factorMs = factor.factorMs;
      res.trailingMs = factor.trailingMs;
    }
    const auto solveStart = std::chrono::steady_clock::now();
    // One vertex block after the other: its non-fixed columns against the
    // rows of the whole request, or with cross = false against its own.
    std::vector<double> cols, col;
    std::vector<uint8_t> conv(std::max(width, 1));
    int block = 0;
    for (int first = 0; first < n && factor.ok; ++block) {
      const int dim = first < sh.camDim * (int)camIds.size() ? sh.camDim
                                                             : sh.ptDim;
      const int64_t* readRows = opt.cross ? rows.data() : rows.data() + first;
      const int nRead = opt.cross ? n : dim;
      // entry (read row i, column j) of this block's solves
      const auto store = [&](int i, int j, double v) {
        if (opt.cross)
          res.joint[(size_t)i * n + j] = fixedRow[i] ? 0.0 : v;
        else
          res.blocks[blockAt[block] + (size_t)i * dim + (j - first)] = v;
      };
      if (fixedRow[first]) {
        first += dim;
        continue;
      }
      if (dense) {
        cols.assign((size_t)nRead * dim, 0.0);
        eng.solveUnitDense(rows.data() + first, dim, readRows, nRead,
                           cols.data());
        for (int c = 0; c < dim; ++c)
          for (int i = 0; i < nRead; ++i)
            store(i, first + c, cols[(size_t)i * dim + c]);
      } else if (width <= 1) {
        col.resize(nRead);
        for (int j = first; j < first + dim; ++j) {
          eng.setUnitRhs(rows[j]);
          res.iters[j] = eng.solveLinear(sopt);
          res.converged[j] = eng.relStopHit();
          eng.readDeltaXRows(readRows, nRead, col.data());
          for (int i = 0; i < nRead; ++i) store(i, j, col[i]);
        }
      } else {
        // the columns of the block, `width` at a time
        for (int j = first; j < first + dim; j += width) {
          const int k = std::min(width, first + dim - j);
          cols.assign((size_t)nRead * k, 0.0);
          eng.solveUnitBatch(rows.data() + j, k, sopt, readRows, nRead,
                             cols.data(), res.iters.data() + j, conv.data());
          for (int c = 0; c < k; ++c) {
            res.converged[j + c] = conv[c];
            for (int i = 0; i < nRead; ++i)
              store(i, j + c, cols[(size_t)i * k + c]);
          }
        }
      }
      first += dim;
    }
    res.solveMs = std::chrono::duration<double, std::milli>(
                      std::chrono::steady_clock::now() - solveStart)
                      .count();
  } catch (...) {
    if (dense) eng.releaseDenseSchur();
    eng.restoreLinearState();
    throw;
  }
  if (dense) eng.releaseDenseSchur();
  eng.restoreLinearState();
  res.products = eng.productCount() - productsBefore;

  if (!factor.ok) {
    // the whole system is singular: no column is usable
    MEGBA_CHECK(!opt.strict,
                "covariance: the Schur complement is not positive definite "
                "(camera " + std::to_string(factor.failRow / sh.camDim) +
                    ", row " + std::to_string(factor.failRow % sh.camDim) +
                    ", pivot ratio " + std::to_string(factor.failPivotRatio) +
                    "); is the gauge fixed by priors or fixed vertices?");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(res.converged.begin(), res.converged.end(), 0);
    if (opt.cross) {
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
          if (!fixedRow[i] && !fixedRow[j]) res.joint[(size_t)i * n + j] = nan;
    } else {
      int block = 0;
      for (int first = 0; first < n; ++block) {
        const int dim = first < sh.camDim * (int)camIds.size() ? sh.camDim
                                                               : sh.ptDim;
        if (!fixedRow[first])
          std::fill(res.blocks.begin() + blockAt[block],
                    res.blocks.begin() + blockAt[block] + (size_t)dim * dim,
                    nan);
        first += dim;
      }
    }
    return res;
  }

  // asymmetry of the raw columns, then the symmetrised result
  double maxAbs = 0.0, maxAsym = 0.0;
  const auto symmetrise = [&](double* A, int m) {
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        const double a = A[(size_t)i * m + j];
        const double b = A[(size_t)j * m + i];
        maxAbs = std::max(maxAbs, std::fabs(a));
        maxAsym = std::max(maxAsym, std::fabs(a - b));
      }
    for (int i = 0; i < m; ++i)
      for (int j = i + 1; j < m; ++j) {
        const double mean =
            0.5 * (A[(size_t)i * m + j] + A[(size_t)j * m + i]);
        A[(size_t)i * m + j] = A[(size_t)j * m + i] = mean;
      }
  };
  if (opt.cross) {
    symmetrise(res.joint.data(), n);
  } else {
    int block = 0;
    for (int first = 0; first < n; ++block) {
      const int dim = first < sh.camDim * (int)camIds.size() ? sh.camDim
                                                             : sh.ptDim;
      symmetrise(res.blocks.data() + blockAt[block], dim);
      first += dim;
    }
  }
  res.asymmetry = maxAbs > 0.0 ? maxAsym / maxAbs : 0.0;

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
