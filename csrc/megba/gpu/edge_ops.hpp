// Per-edge and per-run device primitives shared by the Schur product
// kernels (E^T x, Cinv, E w and their fused window forms) in
// kernels_product.hpp: inline templates over register arrays taken by
// reference.  Their loops fix the floating-point summation order of the
// paths that use them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../jet.hpp"

namespace megba {
namespace {

// 16-byte vector groups used by the packed J / Hpl layouts.
template <typename T>
struct PackVec {
  static constexpr int VEC = 16 / sizeof(T);
  typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

// Packed-upper symmetric index for an RDxRD (or PDxPD) matrix.
template <int D>
__device__ __host__ constexpr int symIdx(int i, int j) {
  return i <= j ? i * D - i * (i - 1) / 2 + (j - i)
                : j * D - j * (j - 1) / 2 + (i - j);
}

// ---------------------------------------------------------------------------
// Point runs inside a wave
// ---------------------------------------------------------------------------
// Wave segmented inclusive scan keyed by pt (lanes hold pt-sorted edges):
// afterwards every lane holds the sum over its run up to and including
// itself.
// Point runs are short (degree ~5): once no lane continues a segment at
// distance `off`, no lane can at any larger distance either — skip the
// remaining dependent shuffle rounds (the scan chain is the E^T x kernels'
// issue-stall bound, 70% SQ_WAIT_INST_ANY).
template <typename T, int N>
__device__ __forceinline__ void waveSegScan(int pt, int lane, T (&t)[N]) {
  for (int off = 1; off < 64; off <<= 1) {
    const int ppt = __shfl_up(pt, off, 64);
    const bool join = lane >= off && ppt == pt;
    if (__ballot(join) == 0ull) break;
    T a[N];
    for (int k = 0; k < N; ++k) a[k] = __shfl_up(t[k], off, 64);
    if (join)
      for (int k = 0; k < N; ++k) t[k] += a[k];
  }
}

// Run tail, block-tiled edges: the wave's last lane and the last edge close
// a run as well (a run crossing the wave edge adds more than one partial).
__device__ __forceinline__ bool runTailTiled(int pt, int lane, bool active,
                                             bool lastEdge) {
  const int nextPt = __shfl_down(pt, 1, 64);
  return active && (lane == 63 || nextPt != pt || lastEdge);
}

// Run tail, run-aligned window [lo, hi) with lane l on edge lo + l.
__device__ __forceinline__ bool runTailWindow(int pt, int lane, bool active,
                                              int64_t lo, int64_t hi) {
  const int nextPt = __shfl_down(pt, 1, 64);
  return active && (lo + lane == hi - 1 || nextPt != pt);
}

// Broadcast w_p from the run tail back to every lane of the run: tail lanes
// form a mask; this lane's tail is the first tail at or after it (points
// are sorted within the window).
template <typename T, int PD>
__device__ __forceinline__ void tailBroadcast(bool tail, int lane,
                                              T (&wv)[PD]) {
  const unsigned long long tails = __ballot(tail);
  const unsigned long long from = tails >> lane;
  const int tl = from ? lane + __ffsll((long long)from) - 1 : lane;
  for (int k = 0; k < PD; ++k) wv[k] = __shfl(wv[k], tl, 64);
}

// Wave sum by the __shfl_down ladder (32, 16, ... 1): lane 0 ends up with the
// sum over the 64 lanes, of every element of a or of one value.
template <typename T, int N>
__device__ __forceinline__ void waveSumDown(T (&a)[N]) {
  for (int off = 32; off > 0; off >>= 1)
    for (int i = 0; i < N; ++i) a[i] += __shfl_down(a[i], off, 64);
}
template <typename T>
__device__ __forceinline__ T waveSumDown(T v) {
  T a[1] = {v};
  waveSumDown(a);
  return a[0];
}

// ---------------------------------------------------------------------------
// Block-diagonal products
// ---------------------------------------------------------------------------
// Row `row` of block b of a block-diagonal matrix (D x D blocks, row-major)
// times that block's vector x (D values, in global memory or LDS): j
// ascending from T(0).
template <typename T, int D>
__device__ __forceinline__ T blockRowDot(const T* __restrict__ A, int64_t b,
                                         int row, const T* x) {
  const T* r = A + b * D * D + (int64_t)row * D;
  T s = T(0);
  for (int j = 0; j < D; ++j) s += r[j] * x[j];
  return s;
}

// Cinv block apply  w = HllInv[pt] * t  (PD x PD, row-major)
template <typename T, int PD, typename In, typename Out>
__device__ __forceinline__ void cinvApply(const T* inv, const In& t, Out& w) {
  for (int i = 0; i < PD; ++i) {
    T v = T(0);
    for (int k = 0; k < PD; ++k) v += inv[i * PD + k] * t[k];
    w[i] = v;
  }
}

// Same, stored as one whole 4-padded w slot (16/32-byte vector stores).
template <typename T, int PD, typename In>
__device__ __forceinline__ void cinvApplyPad(const T* inv, const In& t,
                                             T* slot) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int WL = (4 + VEC - 1) / VEC;
  T out[WL * VEC];
  for (int k = 0; k < WL * VEC; ++k) out[k] = T(0);
  cinvApply<T, PD>(inv, t, out);
  TV* o = (TV*)slot;
  for (int l = 0; l < WL; ++l) {
    TV v;
    for (int q = 0; q < VEC; ++q) v[q] = out[l * VEC + q];
    o[l] = v;
  }
}

// ---------------------------------------------------------------------------
// Edge weight: information matrix and robust-loss scale
// ---------------------------------------------------------------------------
// u = lw * (W u): W the edge's packed symmetric info row (HASINFO), lw the
// loss weight of its accepted residual (lossKind != 0).  The loss scale
// stays inside the lossKind branch so that u is complete before the branch
// and the loads it came from are dead across it.
template <typename T, int RD, bool HASINFO>
__device__ __forceinline__ void applyEdgeWeight(
    int64_t j, int64_t nL, const T* __restrict__ info,
    const T* __restrict__ rBak, int lossKind, T lossD2, T (&u)[RD]) {
  constexpr int RW = RD * (RD + 1) / 2;
  if (HASINFO) {
    T wu[RD];
    for (int i = 0; i < RD; ++i) {
      T v = T(0);
      for (int k = 0; k < RD; ++k)
        v += info[RW * j + symIdx<RD>(i, k)] * u[k];
      wu[i] = v;
    }
    for (int i = 0; i < RD; ++i) u[i] = wu[i];
  }
  if (lossKind) {
    T ss = T(0);
    for (int rr = 0; rr < RD; ++rr) {
      const T rv = rBak[(int64_t)rr * nL + j];
      ss += rv * rv;
    }
    const T w = lossWeight(lossKind, lossD2, ss);
    for (int rr = 0; rr < RD; ++rr) u[rr] *= w;
  }
}

// ---------------------------------------------------------------------------
// Packed edge: 16-byte vector groups ([group][nL][VEC]) of [Jc(CR), Jp(PR)]
// (implicit) or of the Hpl block (explicit), and the XP-padded camera vector
// ---------------------------------------------------------------------------
template <typename T, int CD, int PD, int RD, bool IMP>
struct PackedEdge {
  static constexpr int VEC = PackVec<T>::VEC;
  static constexpr int CR = CD * RD, PR = PD * RD;
  static constexpr int NG = IMP ? (CR + PR + VEC - 1) / VEC
                                : (CD * PD + VEC - 1) / VEC;
  static constexpr int XP = (CD + VEC - 1) / VEC * VEC;
  static constexpr int NX = XP / VEC;
};

template <typename T, int NX>
__device__ __forceinline__ void loadXPadded(
    const T* __restrict__ xPad, int cam,
    typename PackVec<T>::type (&xbuf)[NX]) {
  using TV = typename PackVec<T>::type;
  const TV* xv4 = (const TV*)(xPad + (int64_t)cam * (NX * PackVec<T>::VEC));
#pragma unroll
  for (int l = 0; l < NX; ++l) xbuf[l] = xv4[l];
}

template <typename T, int NG>
__device__ __forceinline__ void loadGroups(
    const T* __restrict__ packed, int64_t nL, int64_t j,
    typename PackVec<T>::type (&buf)[NG]) {
  using TV = typename PackVec<T>::type;
  const TV* src = (const TV*)packed;
#pragma unroll
  for (int g = 0; g < NG; ++g) buf[g] = src[(int64_t)g * nL + j];
}

// Unpack indexing of the packed layouts.
template <typename T, int RD, typename B>
__device__ __forceinline__ T pkJc(const B& buf, int i, int rr) {
  constexpr int VEC = PackVec<T>::VEC;
  const int k = i * RD + rr;
  return buf[k / VEC][k % VEC];
}
template <typename T, int CD, int RD, typename B>
__device__ __forceinline__ T pkJp(const B& buf, int k, int rr) {
  constexpr int VEC = PackVec<T>::VEC;
  const int kk = CD * RD + k * RD + rr;
  return buf[kk / VEC][kk % VEC];
}
template <typename T, int PD, typename B>
__device__ __forceinline__ T pkHpl(const B& buf, int i, int k) {
  constexpr int VEC = PackVec<T>::VEC;
  const int kk = i * PD + k;
  return buf[kk / VEC][kk % VEC];
}
template <typename T, typename B>
__device__ __forceinline__ T pkX(const B& xbuf, int i) {
  constexpr int VEC = PackVec<T>::VEC;
  return xbuf[i / VEC][i % VEC];
}

// u = Jc x
template <typename T, int CD, int RD, typename B, typename X>
__device__ __forceinline__ void packedJcX(const B& buf, const X& xbuf,
                                          T (&u)[RD]) {
#pragma unroll
  for (int rr = 0; rr < RD; ++rr) {
    T v = T(0);
#pragma unroll
    for (int i = 0; i < CD; ++i)
      v += pkJc<T, RD>(buf, i, rr) * pkX<T>(xbuf, i);
    u[rr] = v;
  }
}

// t = Jp^T u
template <typename T, int CD, int PD, int RD, typename B>
__device__ __forceinline__ void packedJpTu(const B& buf, const T (&u)[RD],
                                           T (&t)[PD]) {
#pragma unroll
  for (int k = 0; k < PD; ++k) {
    T v = T(0);
#pragma unroll
    for (int rr = 0; rr < RD; ++rr) v += pkJp<T, CD, RD>(buf, k, rr) * u[rr];
    t[k] = v;
  }
}

// Packed implicit E_e^T x:  t = Jp^T W (Jc x)
template <typename T, int CD, int PD, int RD, bool HASINFO, typename B,
          typename X>
__device__ __forceinline__ void packedEtx(
    const B& buf, const X& xbuf, int64_t j, int64_t nL,
    const T* __restrict__ info, const T* __restrict__ rBak, int lossKind,
    T lossD2, T (&t)[PD]) {
  T u[RD];
  packedJcX<T, CD, RD>(buf, xbuf, u);
  applyEdgeWeight<T, RD, HASINFO>(j, nL, info, rBak, lossKind, lossD2, u);
  packedJpTu<T, CD, PD, RD>(buf, u, t);
}

// Packed explicit E_e^T x:  t += Hpl^T x, x(i) the camera vector's value.
template <typename T, int CD, int PD, typename B, typename XAt>
__device__ __forceinline__ void packedHplTx(const B& buf, XAt x,
                                            T (&t)[PD]) {
#pragma unroll
  for (int i = 0; i < CD; ++i) {
    const T xi = x(i);
#pragma unroll
    for (int k = 0; k < PD; ++k) t[k] += pkHpl<T, PD>(buf, i, k) * xi;
  }
}

// ---------------------------------------------------------------------------
// Grad-major edge of the two-pass window kernels: implicit J through the
// grad-major accepted set ([k][nL], one scalar load per value), explicit Hpl
// through its vector groups; x read value by value from the XP-padded camera
// vector.  The edge stays in jcv/jpv (or hplv) for fusedScatter.
// ---------------------------------------------------------------------------
template <typename T, int CD, int PD, int RD, bool IMP, bool HASINFO>
__device__ inline void fusedLoadEdge(int64_t j, int64_t nL,
                                     const int* __restrict__ camOf,
                                     const T* __restrict__ Hpl,
                                     const T* __restrict__ Jc,
                                     const T* __restrict__ Jp,
                                     const T* __restrict__ info,
                                     const T* __restrict__ rBak, int lossKind,
                                     T lossD2, const T* __restrict__ xPad,
                                     T (&jcv)[RD][CD], T (&jpv)[RD][PD],
                                     T (&hplv)[CD][PD], T (&t)[PD]) {
  constexpr int XPV = PackVec<T>::VEC;
  constexpr int XP = (CD + XPV - 1) / XPV * XPV;
  const T* xc = xPad + (int64_t)camOf[j] * XP;
  if (IMP) {
    for (int i = 0; i < CD; ++i)
      for (int rr = 0; rr < RD; ++rr)
        jcv[rr][i] = Jc[((int64_t)(i * RD + rr)) * nL + j];
    for (int k = 0; k < PD; ++k)
      for (int rr = 0; rr < RD; ++rr)
        jpv[rr][k] = Jp[((int64_t)(k * RD + rr)) * nL + j];
    T u[RD];
    for (int rr = 0; rr < RD; ++rr) {
      T v = T(0);
      for (int i = 0; i < CD; ++i) v += jcv[rr][i] * xc[i];
      u[rr] = v;
    }
    applyEdgeWeight<T, RD, HASINFO>(j, nL, info, rBak, lossKind, lossD2, u);
    for (int k = 0; k < PD; ++k) {
      T v = T(0);
      for (int rr = 0; rr < RD; ++rr) v += jpv[rr][k] * u[rr];
      t[k] = v;
    }
  } else {
    using TV = typename PackVec<T>::type;
    constexpr int VEC = PackVec<T>::VEC;
    constexpr int NGH = (CD * PD + VEC - 1) / VEC;
    const TV* src = (const TV*)Hpl;
    TV buf[NGH];
    for (int g = 0; g < NGH; ++g) buf[g] = src[(int64_t)g * nL + j];
    for (int i = 0; i < CD; ++i)
      for (int k = 0; k < PD; ++k) hplv[i][k] = pkHpl<T, PD>(buf, i, k);
    for (int k = 0; k < PD; ++k) t[k] = T(0);
    for (int i = 0; i < CD; ++i) {
      const T xi = xc[i];
      for (int k = 0; k < PD; ++k) t[k] += hplv[i][k] * xi;
    }
  }
}

// Per-edge E-contribution out[cam] += M w  (M = Jc^T W Jp or Hpl).  The
// weight is read again rather than kept in registers across the scan.
template <typename T, int CD, int PD, int RD, bool IMP, bool HASINFO>
__device__ inline void fusedScatter(int64_t j, int64_t nL,
                                    const int* __restrict__ camOf,
                                    const T* __restrict__ info,
                                    const T* __restrict__ rBak, int lossKind,
                                    T lossD2, const T (&jcv)[RD][CD],
                                    const T (&jpv)[RD][PD],
                                    const T (&hplv)[CD][PD], const T (&wv)[PD],
                                    T* __restrict__ out) {
  T* oc = out + (int64_t)camOf[j] * CD;
  if (IMP) {
    T u[RD];
    for (int rr = 0; rr < RD; ++rr) {
      T v = T(0);
      for (int k = 0; k < PD; ++k) v += jpv[rr][k] * wv[k];
      u[rr] = v;
    }
    applyEdgeWeight<T, RD, HASINFO>(j, nL, info, rBak, lossKind, lossD2, u);
    for (int i = 0; i < CD; ++i) {
      T v = T(0);
      for (int rr = 0; rr < RD; ++rr) v += jcv[rr][i] * u[rr];
      atomicAdd(&oc[i], v);
    }
  } else {
    for (int i = 0; i < CD; ++i) {
      T v = T(0);
      for (int k = 0; k < PD; ++k) v += hplv[i][k] * wv[k];
      atomicAdd(&oc[i], v);
    }
  }
}

}  // namespace
}  // namespace megba
