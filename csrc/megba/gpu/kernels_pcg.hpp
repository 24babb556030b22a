// PCG vector kernels (seven-kernel and rotated body), back-substitution and
// the rho denominator.  Their reductions (blockSum, partialsSum,
// blockSumAtomicAdd, safeRatio) are in gpu_common.hpp, the block-row product
// and the wave sum in edge_ops.hpp, the LDS row reduce in kernels_product.hpp.
#pragma once

#include "edge_ops.hpp"
#include "gpu_common.hpp"
#include "kernels_product.hpp"  // ldsRowsColumnSum

namespace megba {
namespace {

// Fused preconditioner apply + rho partial: z = Binv r (thread per row) and
// per-block partials of r.z in one pass (saves two launches per PCG iter).
template <typename T, int CD>
__global__ void kPrecondRho(int nBlk, const T* __restrict__ Binv,
                            const T* __restrict__ r, T* __restrict__ z,
                            double* part) {
  double local = 0.0;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)nBlk * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const T sv = blockRowDot<T, CD>(Binv, b, (int)(idx % CD), r + b * CD);
    z[idx] = sv;
    local += (double)sv * (double)r[idx];
  }
  const double total = blockSum(local);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// B-apply (y = A x - y, the Schur S-apply tail) fused with the per-block
// p^T q dot partials: saves the separate full pass over p and q per PCG
// iteration (the reference used a standalone cublasDot, its :368-385).
template <typename T, int CD>
__global__ void kBApplyDot(int nBlk, const T* __restrict__ A,
                           const T* __restrict__ x, T* __restrict__ y,
                           double* part) {
  double local = 0.0;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)nBlk * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const T q = blockRowDot<T, CD>(A, b, (int)(idx % CD), x + b * CD) - y[idx];
    y[idx] = q;
    local += (double)x[idx] * (double)q;
  }
  const double total = blockSum(local);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// Small vector kernels
// ---------------------------------------------------------------------------
// Device-side pointer slots for the implicit J buffers: the double-buffered
// accepted set flips on every LM accept, but the captured PCG graph freezes
// kernel arguments — so the kernels dereference this slot array instead and
// acceptForward rewrites it (kernel args carry the values; no host-buffer
// lifetime to manage).  Slots: [0]=Jc, [1]=Jp, [2]=r (all accepted/bak).
template <typename T>
__global__ void kSetPtrSlots(const T** slots, const T* a, const T* b,
                             const T* c) {
  slots[0] = a;
  slots[1] = b;
  slots[2] = c;
}

__global__ void kSetScalar(double* out, double v) { *out = v; }
// (The standalone kRedFinalRhoBeta / kRedFinalAlpha reduction finals were
// folded into kXpbySBeta / kUpdateXRAlpha below in r2.)

// Fused beta + p-update: every block redundantly reduces the (tiny)
// rho partial array to beta = rho/rhoPrev, then updates its slice of
// p = z + beta p.  Replaces the standalone kRedFinalRhoBeta launch
// (block 0 still publishes rho for the host refuse/tol readback).
template <typename T>
__global__ void kXpbySBeta(int64_t n, const T* __restrict__ z,
                           const double* __restrict__ part, int nb,
                           const double* __restrict__ rhoPrev,
                           double* __restrict__ rhoOut, T* __restrict__ p) {
  const double rho = partialsSum(part, nb);
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoOut = rho;
  const T beta = (T)safeRatio(rho, *rhoPrev);
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk)
    p[i] = z[i] + beta * p[i];
}

// Fused alpha + x/r update (incl. the two-deep backup rotation): every
// block reduces BOTH partial arrays (rho from partR, p^T q from partQ),
// forms alpha = rho/pq, and updates its slice; block 0 publishes
// rhoPrev = rho for the next iteration's beta.
template <typename T>
__global__ void kUpdateXRAlpha(int64_t n, const double* __restrict__ partR,
                               int nbR, const double* __restrict__ partQ,
                               int nbQ, double* __restrict__ rhoPrevOut,
                               const T* __restrict__ p,
                               const T* __restrict__ q, T* __restrict__ x,
                               T* __restrict__ xBak,
                               T* __restrict__ xBakPrev, T* __restrict__ r) {
  const double rho = partialsSum(partR, nbR);
  const double pq = partialsSum(partQ, nbQ);
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoPrevOut = rho;
  const T a = (T)safeRatio(rho, pq);
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk) {
    xBakPrev[i] = xBak[i];
    const T xv = x[i];
    xBak[i] = xv;
    x[i] = xv + a * p[i];
    r[i] -= a * q[i];
  }
}

// ---------------------------------------------------------------------------
// Rotated PCG body: three small kernels around the product instead of six
// ---------------------------------------------------------------------------
// The loop is rotated by one kernel (z = Binv r and its rho partials move to
// the end of the previous body; the first ones come from a kPrecondRho
// before the loop), so neighbours that work on the same camera blocks merge:
//   kBetaPPad          = kXpbySBeta + kPadX
//   kLdsReduceBApplyDot = kLdsRowsReduce + kBApplyDot
//   kUpdateXRPrecond   = kUpdateXRAlpha + kPrecondRho
// Each merged kernel calls the device functions its two halves call
// (partialsSum and safeRatio, ldsRowsColumnSum, blockRowDot, blockSum), so
// the sums of the two bodies are the same code.

// beta + p-update (as kXpbySBeta) that also writes the XP-padded copy of the
// new p in kPadX's layout and to kPadX's (dst, stride, off), zero pad lanes
// included.  One thread per padded element.
template <typename T, int CD>
__global__ void kBetaPPad(int ncam, const T* __restrict__ z,
                          const double* __restrict__ part, int nb,
                          const double* __restrict__ rhoPrev,
                          double* __restrict__ rhoOut, T* __restrict__ p,
                          T* __restrict__ dst, int stride, int off) {
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int XP = (CD + VEC - 1) / VEC * VEC;
  const double rho = partialsSum(part, nb);
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoOut = rho;
  const T beta = (T)safeRatio(rho, *rhoPrev);
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)ncam * XP; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t c = idx / XP;
    const int k = (int)(idx % XP);
    T pv = T(0);
    if (k < CD) {
      const int64_t i = c * CD + k;
      pv = z[i] + beta * p[i];
      p[i] = pv;
    }
    dst[c * stride + off + k] = pv;
  }
}

// kLdsRowsReduce whose wave 0 goes on to the B-apply and the p.q partial:
// out = HppD p - (fixed-order sum of the G rows), one partial per block.
// p is read-only here, so a camera that straddles a 64-column block edge is
// read by both blocks.  Only valid when nothing (long-run finishers,
// allreduce) sits between the row reduce and the B-apply.
template <typename T, int CD>
__global__ __launch_bounds__(64 * kLdsRedWaves) void kLdsReduceBApplyDot(
    int G, int nc, const T* __restrict__ rows, const T* __restrict__ A,
    const T* __restrict__ p, T* __restrict__ out, double* __restrict__ part) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const T v = ldsRowsColumnSum<T>(G, nc, rows, col);
  if (threadIdx.x >= 64) return;
  double local = 0.0;
  if (col < nc) {
    const int b = col / CD;
    const T qv = blockRowDot<T, CD>(A, b, col % CD, p + (int64_t)b * CD) - v;
    out[col] = qv;
    local = (double)p[col] * (double)qv;
  }
  local = waveSumDown(local);
  if (threadIdx.x == 0) part[blockIdx.x] = local;
}

// alpha + x/r update (as kUpdateXRAlpha, backup rotation included) followed
// by the NEXT iteration's z = Binv r and rho partials (as kPrecondRho).
// Each block owns kBlk / CD whole cameras and hands r_new to the threads of
// the same camera through LDS, so r is never re-read from global memory
// while other threads store to it.  rho is the scalar the beta kernel
// published (every block of that kernel reduces the same partials in the
// same order), which leaves `part` free for the new partials.
template <typename T, int CD>
__global__ __launch_bounds__(kBlk) void kUpdateXRPrecond(
    int ncam, const double* __restrict__ rhoIn,
    const double* __restrict__ partQ, int nbQ,
    double* __restrict__ rhoPrevOut, const T* __restrict__ p,
    const T* __restrict__ q, T* __restrict__ x, T* __restrict__ xBak,
    T* __restrict__ xBakPrev, T* __restrict__ r, const T* __restrict__ Binv,
    T* __restrict__ z, double* __restrict__ part) {
  constexpr int CPB = kBlk / CD;  // cameras per block
  __shared__ T rNew[CPB * CD];
  const double pq = partialsSum(partQ, nbQ);
  const double rho = *rhoIn;
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoPrevOut = rho;
  const T a = (T)safeRatio(rho, pq);
  const int t = (int)threadIdx.x;
  const int cl = t / CD;  // camera within the block
  const int64_t cam = (int64_t)blockIdx.x * CPB + cl;
  const bool live = cl < CPB && cam < ncam;
  const int64_t i = cam * CD + (t - cl * CD);
  T rn = T(0);
  if (live) {
    xBakPrev[i] = xBak[i];
    const T xv = x[i];
    xBak[i] = xv;
    x[i] = xv + a * p[i];
    rn = r[i] - a * q[i];
    r[i] = rn;
    rNew[t] = rn;
  }
  __syncthreads();  // rNew: a camera's rows are other threads' values
  double local = 0.0;
  if (live) {
    const T sv = blockRowDot<T, CD>(Binv, cam, t - cl * CD, rNew + cl * CD);
    z[i] = sv;
    local = (double)sv * (double)rn;
  }
  const double total = blockSum(local);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// r = v - q
template <typename T>
__global__ void kSub(int64_t n, const T* __restrict__ v, const T* __restrict__ q,
                     T* __restrict__ r) {
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk)
    r[i] = v[i] - q[i];
}
// v = gc * s - v   (s = 1/worldSize pre-compensation, reference :478)
template <typename T>
__global__ void kVMake(int64_t n, const T* __restrict__ gc, T s, T* __restrict__ v) {
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk)
    v[i] = gc[i] * s - v[i];
}
template <typename T>
__global__ void kAddAssign(int64_t n, const T* __restrict__ x, T* __restrict__ y) {
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk)
    y[i] += x[i];
}
template <typename T>
__global__ void kZeroRange(T* p, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk)
    p[i] = T(0);
}
// v[i] = val: the one nonzero of a unit right-hand side (the host checks i).
template <typename T>
__global__ void kSetElement(T* v, int64_t i, T val) {
  if (blockIdx.x == 0 && threadIdx.x == 0) v[i] = val;
}
// out[k] = v[rows[k]] in double for the rows this rank supplies, 0 for the
// others, so that a sum over the ranks holds every row once: rows below nc
// (replicated camera rows) where camOwner is set, rows in [ptLo, ptHi) (this
// rank's point shard) always.  The host checks rows against v's length.
template <typename T>
__global__ void kGatherRows(int n, const T* __restrict__ v,
                            const int64_t* __restrict__ rows, int64_t nc,
                            int64_t ptLo, int64_t ptHi, bool camOwner,
                            double* __restrict__ out) {
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < n;
       k += (int64_t)gridDim.x * kBlk) {
    const int64_t row = rows[k];
    const bool mine = row < nc ? camOwner : (row >= ptLo && row < ptHi);
    out[k] = mine ? (double)v[row] : 0.0;
  }
}
// deltaX_p = HllInv * (g_p - temp)  (local point shard)
template <typename T, int PD>
__global__ void kBackSub(int npt, const T* __restrict__ HllInv,
                         const T* __restrict__ gp, const T* __restrict__ temp,
                         T* __restrict__ dxp) {
  for (int64_t p = blockIdx.x * (int64_t)kBlk + threadIdx.x; p < npt;
       p += (int64_t)gridDim.x * kBlk) {
    T rhs[PD];
    for (int i = 0; i < PD; ++i) rhs[i] = gp[PD * p + i] - temp[PD * p + i];
    T* out = dxp + PD * p;
    cinvApply<T, PD>(HllInv + p * PD * PD, rhs, out);
  }
}

// ---------------------------------------------------------------------------
// rho denominator:  sum over edges of (J dx + r)^2   (backup J/r)
// ---------------------------------------------------------------------------
template <typename T, int CD, int PD, int RD>
__global__ void kRhoDenom(int64_t nL, const int* __restrict__ camOf,
                          const int* __restrict__ ptOf, const T* __restrict__ r,
                          const T* __restrict__ Jc, const T* __restrict__ Jp,
                          const T* __restrict__ dxc, const T* __restrict__ dxp,
                          double* acc, int lossKind, T lossD2) {
  double local = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    const T* dc = dxc + (int64_t)camOf[e] * CD;
    const T* dp = dxp + (int64_t)ptOf[e] * PD;
    T ss = T(0);
    for (int row = 0; row < RD; ++row) {
      T s = r[(int64_t)row * nL + e];
      for (int k = 0; k < CD; ++k)
        s += Jc[((int64_t)(k * RD + row)) * nL + e] * dc[k];
      for (int k = 0; k < PD; ++k)
        s += Jp[((int64_t)(k * RD + row)) * nL + e] * dp[k];
      ss += s * s;
    }
    local += (double)lossRho(lossKind, lossD2, ss);
  }
  blockSumAtomicAdd(local, acc);
}

// Packed-J rho denominator (implicit mode): the accepted [Jc, Jp] vector
// groups and the XP-padded deltaX camera vector replace 26 scalar loads
// per edge (same math as kRhoDenom).
template <typename T, int CD, int PD, int RD>
__global__ void kRhoDenomPk(int64_t nL, const int* __restrict__ camOf,
                            const int* __restrict__ ptOf,
                            const T* __restrict__ r,
                            const T* __restrict__ Jpk,
                            const T* __restrict__ dxcPad,
                            const T* __restrict__ dxp, double* acc,
                            int lossKind, T lossD2) {
  double local = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    using PE = PackedEdge<T, CD, PD, RD, true>;
    typename PackVec<T>::type xbuf[PE::NX], buf[PE::NG];
    loadXPadded<T>(dxcPad, camOf[e], xbuf);
    loadGroups<T>(Jpk, nL, e, buf);
    const T* dp = dxp + (int64_t)ptOf[e] * PD;
    T ss = T(0);
#pragma unroll
    for (int row = 0; row < RD; ++row) {
      T sv = r[(int64_t)row * nL + e];
#pragma unroll
      for (int k = 0; k < CD; ++k)
        sv += pkJc<T, RD>(buf, k, row) * pkX<T>(xbuf, k);
#pragma unroll
      for (int k = 0; k < PD; ++k) sv += pkJp<T, CD, RD>(buf, k, row) * dp[k];
      ss += sv * sv;
    }
    local += (double)lossRho(lossKind, lossD2, ss);
  }
  blockSumAtomicAdd(local, acc);
}

}  // namespace
}  // namespace megba
