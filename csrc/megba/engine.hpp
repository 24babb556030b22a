// Engine interface: the device-specific half of the solver.
// CPU (oracle, OpenMP) and GPU (HIP/gfx950) implement the same contract; the
// LM trust-region driver (lm.hpp) is shared host code.
#pragma once

#include <cstdint>
#include <vector>

#include "common.hpp"

namespace megba {

// Everything a test might want to inspect, in double precision.
struct DenseDump {
  int64_t e0 = 0, e1 = 0;  // local edge range (sorted order)
  std::vector<double> r, Jc, Jp;       // accepted set is NOT dumped; these are
                                       // the buffers of the last forward()
  std::vector<double> Hpp, Hll, Hpl;   // [cam][9][9], [pt][3][3], [e][9][3]
  std::vector<double> g, deltaX;       // camera block first
};

struct EngineShape {
  int ncam = 0, npt = 0, camDim = 0, ptDim = 0;
};

// Outcome of a dense Cholesky factorization (denseSchurFactor).
struct DenseFactorInfo {
  bool ok = false;
  int64_t failRow = -1;         // first failing row in elimination order
  double minPivotRatio = 1.0;   // min over the factored rows of L_ii^2 / S_ii
  double failPivotRatio = 0.0;  // that ratio at failRow
  // wall-clock milliseconds of forming S and of factoring it; trailingMs is
  // the trailing-update kernel's share where the engine profiles it, else -1
  double formMs = 0.0, factorMs = 0.0, trailingMs = -1.0;
};

template <typename T>
class Engine {
 public:
  virtual ~Engine() = default;

  // Evaluate residuals + Jacobians from the current parameters into the
  // "current" buffer set; returns the global chi^2 (sum over all ranks).
  virtual double forward() = 0;

  // Accept the current forward pass: current r/J become the accepted/backup
  // set used by buildLinearSystem and rhoDenominator (reference:
  // jvBackup = jv).  Must be called after forward(), before
  // buildLinearSystem().
  virtual void acceptForward() = 0;

  // Assemble Hpp/Hll/Hpl/g from the *accepted* buffers, then allreduce
  // Hpp, Hll, g across ranks (reference site A1,
  // /root/reference/src/edge/build_linear_system.cu:403-422).
  virtual void buildLinearSystem() = 0;

  // Parameter state backup / rollback (reference: edges.backup()/rollback()).
  virtual void backupParams() = 0;
  virtual void rollbackParams() = 0;

  // deltaX (and g) backup / rollback (reference: linearSystem.backup()).
  virtual void backupGDx() = 0;
  virtual void rollbackGDx() = 0;

  // Produce damped copies of the Hpp/Hll diagonals: d' = d * (1 + 1/region)
  // (reference processDiag, schur_LM_linear_system.cu:112-185; originals are
  // kept so no recover pass is needed).
  virtual void processDiag(double region) = 0;

  // Distributed Schur-complement PCG; writes deltaX.  Returns #iterations.
  virtual int solveLinear(const SolverOptionPCG& opt) = 0;

  virtual double deltaXL2() = 0;   // ||deltaX||_2 (full vector)
  virtual double xL2() = 0;        // ||x||_2 over current parameters
  virtual double gInf() = 0;       // ||g||_inf

  // params += deltaX (both camera and point blocks; all ranks, replicated).
  virtual void updateParams() = 0;

  // sum over edges of (J*deltaX + r)^2 - chi2Backup, with r/J from the BACKUP
  // set (reference computeRhoDenominator, lm_algo.cu:82-126).
  virtual double rhoDenominator(double chi2Backup) = 0;

  // Introspection (tests / write-back).  COLLECTIVE when worldSize>1: every
  // rank must call it (point shards are merged with an allreduce).
  virtual void getParams(double* cams, double* pts) = 0;
  virtual DenseDump dump() const = 0;

  // ---- solves against other right-hand sides (covariance.hpp) -------------
  // Rows are global indices in the camera-first ordering of g / deltaX:
  // camDim * cam + i, then camDim * ncam + ptDim * pt + i.
  virtual EngineShape shape() const = 0;
  virtual bool isFixed(bool camera, int id) const = 0;

  // g := e_row, deltaX := 0 (solveLinear warm-starts from deltaX).  A camera
  // row is set on every rank (solveLinear divides g_c by the world size
  // before its allreduce), a point row on the rank that owns the point.
  virtual void setUnitRhs(int64_t row) = 0;

  // out[i] = deltaX[rows[i]] in double.  COLLECTIVE when worldSize>1: camera
  // rows are replicated, point rows come from the rank that owns the point.
  virtual void readDeltaXRows(const int64_t* rows, int n, double* out) = 0;

  // Save / restore g and deltaX in buffers of their own: backupGDx /
  // rollbackGDx belong to the LM loop.
  virtual void saveLinearState() = 0;
  virtual void restoreLinearState() = 0;

  // Whether the last solveLinear ended on the relTol rule.
  virtual bool relStopHit() const = 0;

  // ---- several unit columns at once (covariance.hpp, batch > 1) -----------
  // Most columns solveUnitBatch can carry through one batched Schur product;
  // 1: the engine has no batched product and runs the column loop below.
  virtual int maxBatch() const { return 1; }

  // Solve the k unit right-hand sides e_rhsRows[c] from x = 0 and return the
  // rows readRows[0..n) of every solution: out is n x k row-major, iters and
  // converged are per column.  COLLECTIVE when worldSize>1.  Overwrites g and
  // deltaX like setUnitRhs / solveLinear.
  virtual void solveUnitBatch(const int64_t* rhsRows, int k,
                              const SolverOptionPCG& opt,
                              const int64_t* readRows, int n, double* out,
                              int* iters, uint8_t* converged) {
    std::vector<double> col(n);
    for (int c = 0; c < k; ++c) {
      setUnitRhs(rhsRows[c]);
      iters[c] = solveLinear(opt);
      converged[c] = relStopHit();
      readDeltaXRows(readRows, n, col.data());
      for (int i = 0; i < n; ++i) out[(size_t)i * k + c] = col[i];
    }
  }

  // ---- dense Cholesky of the Schur complement (covariance.hpp, Dense) ------
  // After buildLinearSystem() and processDiag(): invert the point blocks
  // (no jitter: a singular block is an error), form S = HppD - E Cinv E^T
  // as a dense n x n fp64 matrix, n = camDim * ncam, and factor it in place
  // as L L^T.  A pivot fails when it is not finite, not positive or below
  // pivotTol * S_ii; the factor is then unusable.  Costs 8 n^2 bytes until
  // releaseDenseSchur().  COLLECTIVE when worldSize>1: every rank forms the
  // partial S of its point shard, the partials are summed and every rank
  // factors its own copy.  fp64 engines only.
  virtual DenseFactorInfo denseSchurFactor(double /*pivotTol*/) {
    MEGBA_CHECK(false, "this engine has no dense Schur factorization");
    return {};
  }

  // solveUnitBatch against the stored factor: the k <= max(camDim, ptDim)
  // unit right-hand sides e_rhsRows[c] solved exactly, rows readRows[0..n) of
  // every solution into out (n x k row-major).  COLLECTIVE when worldSize>1.
  virtual void solveUnitDense(const int64_t* /*rhsRows*/, int /*k*/,
                              const int64_t* /*readRows*/, int /*n*/,
                              double* /*out*/) {
    MEGBA_CHECK(false, "this engine has no dense Schur factorization");
  }

  // Free the n^2 buffer of denseSchurFactor.
  virtual void releaseDenseSchur() {}

  // Test hooks.  denseSchurMatrix: the S denseSchurFactor would factor, as a
  // symmetric n x n row-major matrix (after buildLinearSystem() and
  // processDiag(); COLLECTIVE).  denseCholesky: factor the caller's n x n
  // symmetric matrix with the engine's factorization; A is overwritten with
  // L, upper triangle zero.
  virtual void denseSchurMatrix(double* /*out*/) {
    MEGBA_CHECK(false, "this engine has no dense Schur factorization");
  }
  virtual DenseFactorInfo denseCholesky(double* /*A*/, int /*n*/,
                                        double /*pivotTol*/) {
    MEGBA_CHECK(false, "this engine has no dense Schur factorization");
    return {};
  }

  // How often the engine has applied the Schur product S p so far (PCG
  // iterations and initial residuals; a batched application counts once).
  int64_t productCount() const { return products_; }

  // Test hook: out = S X for the k columns of X (nc x k row-major, nc =
  // camDim * ncam), after buildLinearSystem() and processDiag(); inverts the
  // blocks itself.  batched=false applies the engine's product column by
  // column, batched=true its batched product (k <= maxBatch()).  COLLECTIVE
  // when worldSize>1.
  virtual void schurApplyColumns(const double* /*X*/, int /*k*/,
                                 bool /*batched*/, double* /*out*/) {
    MEGBA_CHECK(false, "schur_apply is a hook of the GPU engine");
  }

 protected:
  int64_t products_ = 0;
};

}  // namespace megba
