// Batched (multi-right-hand-side) Schur PCG kernels: the products E^T X and
// E W and the PCG vector kernels for up to KB columns that share one pass
// over the packed J (implicit mode) or Hpl (explicit mode).  Instantiated for
// fp64 only; covariance.hpp is the caller.
//
// KB is the compiled width, k <= KB the number of active columns.  Column
// loops are fully unrolled and an inactive column is skipped by the uniform
// test c < k, so no register array is ever indexed dynamically.  The vector
// kernels put the column on blockIdx.y instead: a block works on one column
// and the grid has k rows.
//
// Column-interleaved layouts (one vertex's KB slices are contiguous):
//   camera side, padded    [cam][KB][XP]   XP as in PackedEdge, zero pad lanes
//                                          (P and X; E^T gathers them)
//   camera side, plain     [cam][KB][CD]   (R, Z, Q: the allreduced product)
//   point-side temp        [pt][KB][PD]
//   padded w               [pt][KB][4]
#pragma once

#include "edge_ops.hpp"
#include "gpu_common.hpp"
#include "kernels_product.hpp"  // exChunk, loadWPadded

namespace megba {
namespace {

// The edge weight u -> lw * (W u) as an RD x RD matrix, built once per edge
// by applyEdgeWeight on the unit vectors, so every column of a batch reuses
// the information row and the loss weight instead of loading them again.
template <typename T, int RD, bool HASINFO>
__device__ __forceinline__ void edgeWeightMatrix(
    int64_t j, int64_t nL, const T* __restrict__ info,
    const T* __restrict__ rBak, int lossKind, T lossD2, T (&M)[RD][RD]) {
#pragma unroll
  for (int col = 0; col < RD; ++col) {
    T e[RD];
#pragma unroll
    for (int i = 0; i < RD; ++i) e[i] = i == col ? T(1) : T(0);
    applyEdgeWeight<T, RD, HASINFO>(j, nL, info, rBak, lossKind, lossD2, e);
#pragma unroll
    for (int i = 0; i < RD; ++i) M[i][col] = e[i];
  }
}

// Batched packed E^T X (implicit): kSpmvEtxPk's thread-per-edge layout, run
// scan and tail atomics, with the edge's groups and weight loaded once and
// t_c = Jp^T W (Jc x_c) formed for every active column.
template <typename T, int CD, int PD, int RD, bool HASINFO, int KB>
__global__ __launch_bounds__(kBlk) void kSpmvEtxPkB(
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ Jpk, const T* const* __restrict__ jSlots,
    const T* __restrict__ info, int lossKind, T lossD2,
    const T* __restrict__ xPadB, int k, T* __restrict__ out) {
  using PE = PackedEdge<T, CD, PD, RD, true>;
  using TV = typename PackVec<T>::type;
  const T* rBak = jSlots[2];
  const int lane = threadIdx.x & 63;
  const int64_t nWork = ((nL + kBlk - 1) / kBlk) * (int64_t)kBlk;
  for (int64_t j0 = blockIdx.x * (int64_t)kBlk + threadIdx.x; j0 < nWork;
       j0 += (int64_t)gridDim.x * kBlk) {
    const bool active = j0 < nL;
    const int64_t j = active ? j0 : nL - 1;
    const int pt = ptOf[j];
    T o[KB * PD];
#pragma unroll
    for (int i = 0; i < KB * PD; ++i) o[i] = T(0);
    if (active) {
      TV buf[PE::NG];
      loadGroups<T>(Jpk, nL, j, buf);
      T M[RD][RD];
      edgeWeightMatrix<T, RD, HASINFO>(j, nL, info, rBak, lossKind, lossD2, M);
      const int cam = camOf[j];
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        if (c < k) {
          TV xbuf[PE::NX];
          loadXPadded<T>(xPadB, cam * KB + c, xbuf);
          T u[RD], wu[RD], t[PD];
          packedJcX<T, CD, RD>(buf, xbuf, u);
#pragma unroll
          for (int i = 0; i < RD; ++i) {
            T v = T(0);
#pragma unroll
            for (int q = 0; q < RD; ++q) v += M[i][q] * u[q];
            wu[i] = v;
          }
          packedJpTu<T, CD, PD, RD>(buf, wu, t);
#pragma unroll
          for (int q = 0; q < PD; ++q) o[c * PD + q] = t[q];
        }
      }
    }
    waveSegScan(pt, lane, o);
    if (runTailTiled(pt, lane, active, j0 == nL - 1)) {
      T* op = out + (int64_t)pt * (KB * PD);
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        if (c < k) {
#pragma unroll
          for (int q = 0; q < PD; ++q) atomicAdd(&op[c * PD + q], o[c * PD + q]);
        }
      }
    }
  }
}

// Batched packed E W over the cam-sorted [wJc, Jp] groups: kSpmvExPk's wave
// per chunk, the edge loaded once, acc[c][CD] per active column.
template <typename T, int CD, int PD, int RD, int KB>
__global__ __launch_bounds__(64) void kSpmvExPkB(
    int nChunks, const int* __restrict__ chCam, const int* __restrict__ chLo,
    const int* __restrict__ chHi, const int* __restrict__ ptOfCam,
    const T* __restrict__ JCamPk, int64_t nL, const T* __restrict__ wB, int k,
    T* __restrict__ out) {
  using PE = PackedEdge<T, CD, PD, RD, true>;
  using TV = typename PackVec<T>::type;
  int cam, lo, hi;
  if (!exChunk(nChunks, chCam, chLo, chHi, cam, lo, hi)) return;
  T acc[KB * CD];
#pragma unroll
  for (int i = 0; i < KB * CD; ++i) acc[i] = T(0);
  for (int j = lo + (int)threadIdx.x; j < hi; j += 64) {
    TV buf[PE::NG];
    loadGroups<T>(JCamPk, nL, j, buf);
    const int pt = ptOfCam[j];
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (c < k) {
        TV wbuf[kWPadVecs<T>];
        loadWPadded<T>(wB, pt * KB + c, wbuf);
        T u[RD];
#pragma unroll
        for (int rr = 0; rr < RD; ++rr) {
          T v = T(0);
#pragma unroll
          for (int q = 0; q < PD; ++q)
            v += pkJp<T, CD, RD>(buf, q, rr) * pkX<T>(wbuf, q);
          u[rr] = v;
        }
#pragma unroll
        for (int i = 0; i < CD; ++i) {
          T v = T(0);
#pragma unroll
          for (int rr = 0; rr < RD; ++rr) v += pkJc<T, RD>(buf, i, rr) * u[rr];
          acc[c * CD + i] += v;
        }
      }
    }
  }
  waveSumDown(acc);
  if (threadIdx.x == 0) {
    T* oc = out + (int64_t)cam * (KB * CD);
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (c < k) {
#pragma unroll
        for (int i = 0; i < CD; ++i) atomicAdd(&oc[c * CD + i], acc[c * CD + i]);
      }
    }
  }
}

// Explicit-mode twins over the packed Hpl groups (the block carries the
// weights): the batched forms of kSpmvEtx and kSpmvEx.  x comes from the
// padded [cam][KB][XP] layout like in the implicit kernel.
template <typename T, int CD, int PD, int RD, int KB>
__global__ __launch_bounds__(kBlk) void kSpmvEtxB(
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ Hpl, const T* __restrict__ xPadB, int k,
    T* __restrict__ out) {
  using PE = PackedEdge<T, CD, PD, RD, false>;
  using TV = typename PackVec<T>::type;
  const int lane = threadIdx.x & 63;
  const int64_t nWork = ((nL + kBlk - 1) / kBlk) * (int64_t)kBlk;
  for (int64_t j0 = blockIdx.x * (int64_t)kBlk + threadIdx.x; j0 < nWork;
       j0 += (int64_t)gridDim.x * kBlk) {
    const bool active = j0 < nL;
    const int64_t j = active ? j0 : nL - 1;
    const int pt = ptOf[j];
    T o[KB * PD];
#pragma unroll
    for (int i = 0; i < KB * PD; ++i) o[i] = T(0);
    if (active) {
      TV buf[PE::NG];
      loadGroups<T>(Hpl, nL, j, buf);
      const int cam = camOf[j];
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        if (c < k) {
          TV xbuf[PE::NX];
          loadXPadded<T>(xPadB, cam * KB + c, xbuf);
          T t[PD];
#pragma unroll
          for (int q = 0; q < PD; ++q) t[q] = T(0);
          packedHplTx<T, CD, PD>(buf, [&](int i) { return pkX<T>(xbuf, i); },
                                 t);
#pragma unroll
          for (int q = 0; q < PD; ++q) o[c * PD + q] = t[q];
        }
      }
    }
    waveSegScan(pt, lane, o);
    if (runTailTiled(pt, lane, active, j0 == nL - 1)) {
      T* op = out + (int64_t)pt * (KB * PD);
#pragma unroll
      for (int c = 0; c < KB; ++c) {
        if (c < k) {
#pragma unroll
          for (int q = 0; q < PD; ++q) atomicAdd(&op[c * PD + q], o[c * PD + q]);
        }
      }
    }
  }
}

template <typename T, int CD, int PD, int RD, int KB>
__global__ __launch_bounds__(64) void kSpmvExB(
    int nChunks, const int* __restrict__ chCam, const int* __restrict__ chLo,
    const int* __restrict__ chHi, const int* __restrict__ ptOfCam,
    const T* __restrict__ HplCam, int64_t nL, const T* __restrict__ wB, int k,
    T* __restrict__ out) {
  using PE = PackedEdge<T, CD, PD, RD, false>;
  using TV = typename PackVec<T>::type;
  int cam, lo, hi;
  if (!exChunk(nChunks, chCam, chLo, chHi, cam, lo, hi)) return;
  T acc[KB * CD];
#pragma unroll
  for (int i = 0; i < KB * CD; ++i) acc[i] = T(0);
  for (int j = lo + (int)threadIdx.x; j < hi; j += 64) {
    TV buf[PE::NG];
    loadGroups<T>(HplCam, nL, j, buf);
    const int pt = ptOfCam[j];
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (c < k) {
        TV wbuf[kWPadVecs<T>];
        loadWPadded<T>(wB, pt * KB + c, wbuf);
#pragma unroll
        for (int i = 0; i < CD; ++i) {
          T v = T(0);
#pragma unroll
          for (int q = 0; q < PD; ++q)
            v += pkHpl<T, PD>(buf, i, q) * pkX<T>(wbuf, q);
          acc[c * CD + i] += v;
        }
      }
    }
  }
  waveSumDown(acc);
  if (threadIdx.x == 0) {
    T* oc = out + (int64_t)cam * (KB * CD);
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (c < k) {
#pragma unroll
        for (int i = 0; i < CD; ++i) atomicAdd(&oc[c * CD + i], acc[c * CD + i]);
      }
    }
  }
}

// w_c = Cinv temp_c into the padded [pt][KB][4] layout, one thread per
// (point, column) of the local shard (the three pointers are shard bases).
template <typename T, int PD, int KB>
__global__ void kCinvPadB(int nPt, const T* __restrict__ HllInv,
                          const T* __restrict__ tempB, int k,
                          T* __restrict__ wB) {
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)nPt * KB; idx += (int64_t)gridDim.x * kBlk) {
    if ((int)(idx % KB) < k)
      cinvApplyPad<T, PD>(HllInv + (idx / KB) * PD * PD, tempB + idx * PD,
                          wB + idx * 4);
  }
}

// ---------------------------------------------------------------------------
// Vector kernels: grid (blocks, k), column c = blockIdx.y, per-column partials
// at part[c * gridDim.x + blockIdx.x]
// ---------------------------------------------------------------------------
template <typename T, int CD>
constexpr int kXPB = PackedEdge<T, CD, 3, 2, true>::XP;

// Q = HppD P - Q with the p.q partials of column c (kBApplyDot, batched).
template <typename T, int CD, int KB>
__global__ void kBApplyDotB(int ncam, const T* __restrict__ A,
                            const T* __restrict__ PB, T* __restrict__ QB,
                            double* __restrict__ part) {
  constexpr int XP = kXPB<T, CD>;
  const int c = blockIdx.y;
  double local = 0.0;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)ncam * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const int i = (int)(idx % CD);
    const T* pc = PB + (b * KB + c) * XP;
    T* qc = QB + (b * KB + c) * CD;
    const T q = blockRowDot<T, CD>(A, b, i, pc) - qc[i];
    qc[i] = q;
    local += (double)pc[i] * (double)q;
  }
  const double total = blockSum(local);
  if (threadIdx.x == 0) part[c * gridDim.x + blockIdx.x] = total;
}

// Z = Binv R and the rho partials of column c (kPrecondRho, batched).
template <typename T, int CD, int KB>
__global__ void kPrecondRhoB(int ncam, const T* __restrict__ Binv,
                             const T* __restrict__ RB, T* __restrict__ ZB,
                             double* __restrict__ part) {
  const int c = blockIdx.y;
  double local = 0.0;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)ncam * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const int i = (int)(idx % CD);
    const T* rc = RB + (b * KB + c) * CD;
    const T sv = blockRowDot<T, CD>(Binv, b, i, rc);
    ZB[(b * KB + c) * CD + i] = sv;
    local += (double)sv * (double)rc[i];
  }
  const double total = blockSum(local);
  if (threadIdx.x == 0) part[c * gridDim.x + blockIdx.x] = total;
}

// rho_c from its nb partials, published for the host and the alpha kernel;
// beta_c = rho_c / rhoPrev_c and P_c = Z_c + beta_c P_c in the padded layout
// (the pad lanes are zeroed once and never written).  A column whose done
// flag is set keeps its P.
template <typename T, int CD, int KB>
__global__ void kBetaPB(int ncam, const T* __restrict__ ZB,
                        const double* __restrict__ part, int nb,
                        const double* __restrict__ rhoPrev,
                        const int* __restrict__ done,
                        double* __restrict__ rhoOut, T* __restrict__ PB) {
  constexpr int XP = kXPB<T, CD>;
  const int c = blockIdx.y;
  const double rho = partialsSum(part + (int64_t)c * nb, nb);
  if (blockIdx.x == 0 && threadIdx.x == 0) rhoOut[c] = rho;
  if (done[c]) return;
  const T beta = (T)safeRatio(rho, rhoPrev[c]);
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)ncam * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / CD;
    const int i = (int)(idx % CD);
    T* pc = PB + (b * KB + c) * XP + i;
    *pc = ZB[(b * KB + c) * CD + i] + beta * *pc;
  }
}

// alpha_c = rho_c / (p.q)_c, forced to 0 for a done column (x, r and with
// them z and rho stay as they are); X += alpha P, R -= alpha Q, then the next
// Z = Binv R and rho partials.  As kUpdateXRPrecond: a block owns kBlk / CD
// whole cameras of its column and hands r_new over through LDS; the grid is
// (ceil(ncam / (kBlk / CD)), k).
template <typename T, int CD, int KB>
__global__ __launch_bounds__(kBlk) void kUpdateXRPrecondB(
    int ncam, const double* __restrict__ rhoIn,
    const double* __restrict__ partQ, int nbQ, const int* __restrict__ done,
    double* __restrict__ rhoPrevOut, const T* __restrict__ PB,
    const T* __restrict__ QB, T* __restrict__ XB, T* __restrict__ RB,
    const T* __restrict__ Binv, T* __restrict__ ZB,
    double* __restrict__ part) {
  constexpr int XP = kXPB<T, CD>;
  constexpr int CPB = kBlk / CD;  // cameras per block
  __shared__ T rNew[CPB * CD];
  const int c = blockIdx.y;
  const double pq = partialsSum(partQ + (int64_t)c * nbQ, nbQ);
  const double rho = rhoIn[c];
  if (blockIdx.x == 0 && threadIdx.x == 0) rhoPrevOut[c] = rho;
  const T a = done[c] ? T(0) : (T)safeRatio(rho, pq);
  const int t = (int)threadIdx.x;
  const int cl = t / CD;  // camera within the block
  const int i = t - cl * CD;
  const int64_t cam = (int64_t)blockIdx.x * CPB + cl;
  const bool live = cl < CPB && cam < ncam;
  const int64_t sp = (cam * KB + c) * XP + i;  // padded slices: P, X
  const int64_t sc = (cam * KB + c) * CD + i;  // plain slices: Q, R, Z
  T rn = T(0);
  if (live) {
    XB[sp] += a * PB[sp];
    rn = RB[sc] - a * QB[sc];
    RB[sc] = rn;
    rNew[t] = rn;
  }
  __syncthreads();  // rNew: a camera's rows are other threads' values
  double local = 0.0;
  if (live) {
    const T sv = blockRowDot<T, CD>(Binv, cam, i, rNew + cl * CD);
    ZB[sc] = sv;
    local = (double)sv * (double)rn;
  }
  const double total = blockSum(local);
  if (threadIdx.x == 0) part[c * gridDim.x + blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// Right-hand sides and result rows
// ---------------------------------------------------------------------------
// The unit entries of the k right-hand sides: a camera row goes straight into
// R (every rank holds the replicated camera side), a point row into this
// rank's temp where it owns the point (Cinv and E then form -E Cinv g_p).
template <typename T, int CD, int PD, int KB>
__global__ void kSetUnitsB(int k, const int64_t* __restrict__ rhsRows,
                           int64_t nc, int ptLo, int ptHi, T* __restrict__ RB,
                           T* __restrict__ tempB) {
  const int c = (int)threadIdx.x;
  if (blockIdx.x != 0 || c >= k) return;
  const int64_t row = rhsRows[c];
  if (row < nc) {
    RB[((row / CD) * KB + c) * CD + row % CD] = T(1);
  } else {
    const int64_t pt = (row - nc) / PD;
    if (pt >= ptLo && pt < ptHi)
      tempB[(pt * KB + c) * PD + (row - nc) % PD] = T(1);
  }
}

// r -= q
template <typename T>
__global__ void kSubAssign(int64_t n, const T* __restrict__ q,
                           T* __restrict__ r) {
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk)
    r[i] -= q[i];
}

// out[i * k + c] = row rows[i] of column c's solution in double, under the
// rule of kGatherRows (rank 0 supplies the replicated camera rows, the owner
// a point row).  A point row is back-substituted on the spot as kBackSub
// does: Cinv (g_p - E^T x) with g_p the column's unit entry.
template <typename T, int CD, int PD, int KB>
__global__ void kGatherRowsB(int n, int k, const int64_t* __restrict__ rows,
                             const int64_t* __restrict__ rhsRows,
                             const T* __restrict__ XB,
                             const T* __restrict__ tempB,
                             const T* __restrict__ HllInv, int64_t nc,
                             int ptLo, int ptHi, bool camOwner,
                             double* __restrict__ out) {
  constexpr int XP = kXPB<T, CD>;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)n * k; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t row = rows[idx / k];
    const int c = (int)(idx % k);
    double v = 0.0;
    if (row < nc) {
      if (camOwner) v = (double)XB[((row / CD) * KB + c) * XP + row % CD];
    } else {
      const int64_t pt = (row - nc) / PD;
      if (pt >= ptLo && pt < ptHi) {
        const int64_t first = nc + pt * PD;
        T rhs[PD], w[PD];
        for (int q = 0; q < PD; ++q)
          rhs[q] = (rhsRows[c] == first + q ? T(1) : T(0)) -
                   tempB[(pt * KB + c) * PD + q];
        cinvApply<T, PD>(HllInv + pt * PD * PD, rhs, w);
        T r = T(0);
        for (int q = 0; q < PD; ++q)
          if (q == (int)(row - first)) r = w[q];
        v = (double)r;
      }
    }
    out[idx] = v;
  }
}

}  // namespace
}  // namespace megba
