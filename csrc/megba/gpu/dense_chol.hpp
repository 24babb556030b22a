// Dense fp64 Cholesky and triangular solves on the GPU (dense_chol.hip): the
// host-callable half.  Independent of the block dimensions; the engine's
// dense Schur route (Engine::denseSchurFactor) is the caller.
//
// The matrix is np x np row-major, np = paddedDim(n) a multiple of the
// kTile-wide tile, rows n..np an identity tail; only the lower triangle is
// read and written.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace megba {
namespace dense {

constexpr int kTile = 64;
constexpr int kMaxRhs = 16;  // most right-hand sides of solve()

inline int64_t paddedDim(int64_t n) {
  return (n + kTile - 1) / kTile * kTile;
}

// Device words of a factorization; the host reads them once, at the end.
struct FactorWords {
  int failRow;       // first failing row in elimination order, -1 if none
  int pad;
  double minRatio;   // min over the factored rows of L_ii^2 / S_ii
  double failRatio;  // that ratio at failRow
};

// Ones on the diagonal of the tail rows n..np of a zeroed matrix.
void identityTail(double* A, int64_t np, int64_t n, hipStream_t s);

// A = L L^T in place.  invDiag ((np / kTile) x kTile x kTile) receives the
// inverses of the diagonal tiles of L, diag0 (np) the diagonal of A before
// the elimination; words is reset here.  With phaseMs the three kernels are
// timed one by one with events, a synchronisation per launch, and their
// milliseconds added to phaseMs[0..3): diagonal, panel, trailing update.
void factor(double* A, int64_t np, double* invDiag, double* diag0,
            double pivotTol, FactorWords* words, hipStream_t s,
            float* phaseMs = nullptr);

// X = (L L^T)^-1 R for k <= kMaxRhs columns (nothing is done for more) in the camera-block layouts of
// kernels_batch.hpp: R is [cam][kb][cd], X is [cam][kb][xStride]; rows of X
// past n and its pad lanes are left alone.  work holds 2 * np * k doubles.
void solve(const double* L, const double* invDiag, int64_t np, int64_t n,
           const double* R, double* X, double* work, int cd, int kb, int k,
           int xStride, hipStream_t s);

}  // namespace dense
}  // namespace megba
