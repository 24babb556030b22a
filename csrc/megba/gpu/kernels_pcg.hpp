// PCG vector kernels (seven-kernel and rotated body), back-substitution and
// the rho denominator.
#pragma once

#include "edge_ops.hpp"
#include "gpu_common.hpp"
#include "kernels_product.hpp"  // kLdsRedWaves

namespace megba {
namespace {

// Fused preconditioner apply + rho partial: z = Binv r (thread per row) and
// per-block partials of r.z in one pass (saves two launches per PCG iter).
template <typename T, int CD>
__global__ void kPrecondRho(int nBlk, const T* __restrict__ Binv,
                            const T* __restrict__ r, T* __restrict__ z,
                            double* part) {
  __shared__ double sm[kBlk];
  double local = 0.0;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)nBlk * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const int rr = (int)(idx % CD);
    const T* row = Binv + b * CD * CD + (int64_t)rr * CD;
    const T* xb = r + b * CD;
    T sv = T(0);
    for (int j = 0; j < CD; ++j) sv += row[j] * xb[j];
    z[idx] = sv;
    local += (double)sv * (double)r[idx];
  }
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// B-apply (y = A x - y, the Schur S-apply tail) fused with the per-block
// p^T q dot partials: saves the separate full pass over p and q per PCG
// iteration (the reference used a standalone cublasDot, its :368-385).
template <typename T, int CD>
__global__ void kBApplyDot(int nBlk, const T* __restrict__ A,
                           const T* __restrict__ x, T* __restrict__ y,
                           double* part) {
  __shared__ double sm[kBlk];
  double local = 0.0;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)nBlk * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const int rrow = (int)(idx % CD);
    const T* row = A + b * CD * CD + (int64_t)rrow * CD;
    const T* xb = x + b * CD;
    T s = T(0);
    for (int j = 0; j < CD; ++j) s += row[j] * xb[j];
    const T q = s - y[idx];
    y[idx] = q;
    local += (double)x[idx] * (double)q;
  }
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
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
  __shared__ double sm[kBlk];
  double v = 0.0;
  for (int i = threadIdx.x; i < nb; i += kBlk) v += part[i];
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  const double rho = sm[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoOut = rho;
  const double rp = *rhoPrev;
  const T beta = (T)(rp != 0.0 ? rho / rp : 0.0);
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
  __shared__ double smR[kBlk];
  __shared__ double smQ[kBlk];
  double vR = 0.0, vQ = 0.0;
  for (int i = threadIdx.x; i < nbR; i += kBlk) vR += partR[i];
  for (int i = threadIdx.x; i < nbQ; i += kBlk) vQ += partQ[i];
  smR[threadIdx.x] = vR;
  smQ[threadIdx.x] = vQ;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      smR[threadIdx.x] += smR[threadIdx.x + st];
      smQ[threadIdx.x] += smQ[threadIdx.x + st];
    }
    __syncthreads();
  }
  const double rho = smR[0];
  const double pq = smQ[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoPrevOut = rho;
  const T a = (T)(pq != 0.0 ? rho / pq : 0.0);
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
  __shared__ double sm[kBlk];
  double v = 0.0;
  for (int i = threadIdx.x; i < nb; i += kBlk) v += part[i];
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  const double rho = sm[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoOut = rho;
  const double rp = *rhoPrev;
  const T beta = (T)(rp != 0.0 ? rho / rp : 0.0);
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
  __shared__ T sm[kLdsRedWaves][64];
  const int lane = threadIdx.x & 63;
  const int col = blockIdx.x * 64 + lane;
  const int q = (int)threadIdx.x >> 6;
  const int g0 = (int)((int64_t)G * q / kLdsRedWaves);
  const int g1 = (int)((int64_t)G * (q + 1) / kLdsRedWaves);
  T s = T(0);
  if (col < nc) {
#pragma unroll 8
    for (int g = g0; g < g1; ++g) s += rows[(int64_t)g * nc + col];
  }
  sm[q][lane] = s;
  __syncthreads();
  if (q != 0) return;
  double local = 0.0;
  if (col < nc) {
    T v = sm[0][lane];
    for (int k = 1; k < kLdsRedWaves; ++k) v += sm[k][lane];
    const int b = col / CD;
    const int rrow = col % CD;
    const T* row = A + (int64_t)b * CD * CD + rrow * CD;
    const T* xb = p + (int64_t)b * CD;
    T hp = T(0);
    for (int j = 0; j < CD; ++j) hp += row[j] * xb[j];
    const T qv = hp - v;
    out[col] = qv;
    local = (double)p[col] * (double)qv;
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if (lane == 0) part[blockIdx.x] = local;
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
  __shared__ double sm[kBlk];
  __shared__ T rNew[CPB * CD];
  double vQ = 0.0;
  for (int i = threadIdx.x; i < nbQ; i += kBlk) vQ += partQ[i];
  sm[threadIdx.x] = vQ;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  const double pq = sm[0];
  const double rho = *rhoIn;
  __syncthreads();  // sm is reused for the rho partial below
  if (blockIdx.x == 0 && threadIdx.x == 0) *rhoPrevOut = rho;
  const T a = (T)(pq != 0.0 ? rho / pq : 0.0);
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
  __syncthreads();
  double local = 0.0;
  if (live) {
    const T* row = Binv + cam * CD * CD + (int64_t)(t - cl * CD) * CD;
    const T* xb = rNew + cl * CD;
    T sv = T(0);
    for (int j = 0; j < CD; ++j) sv += row[j] * xb[j];
    z[i] = sv;
    local = (double)sv * (double)rn;
  }
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
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
// deltaX_p = HllInv * (g_p - temp)  (local point shard)
template <typename T, int PD>
__global__ void kBackSub(int npt, const T* __restrict__ HllInv,
                         const T* __restrict__ gp, const T* __restrict__ temp,
                         T* __restrict__ dxp) {
  for (int64_t p = blockIdx.x * (int64_t)kBlk + threadIdx.x; p < npt;
       p += (int64_t)gridDim.x * kBlk) {
    const T* inv = HllInv + p * PD * PD;
    T rhs[PD];
    for (int i = 0; i < PD; ++i) rhs[i] = gp[PD * p + i] - temp[PD * p + i];
    for (int i = 0; i < PD; ++i) {
      T v = T(0);
      for (int j = 0; j < PD; ++j) v += inv[i * PD + j] * rhs[j];
      dxp[PD * p + i] = v;
    }
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
  __shared__ double sm[kBlk];
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
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int s = kBlk / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(acc, sm[0]);
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
  __shared__ double sm[kBlk];
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
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int st = kBlk / 2; st > 0; st >>= 1) {
    if (threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(acc, sm[0]);
}

}  // namespace
}  // namespace megba
