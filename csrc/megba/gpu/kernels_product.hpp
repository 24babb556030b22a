// Schur product kernels: E^T x, Cinv and E w as separate passes, their fused
// window forms, the LDS single-pass apply and its row reduce.
#pragma once

#include "../analytical.hpp"
#include "edge_ops.hpp"
#include "gpu_common.hpp"
#include "rc_tile.hpp"

namespace megba {
namespace {

// ---------------------------------------------------------------------------
// Packed-J layout for the per-iteration implicit products
// ---------------------------------------------------------------------------
// The grad-major J layout ([k][nL], one 4/8-byte load per value) makes the
// two matrix-free PCG kernels instruction-ISSUE-bound: ~24 scalar loads
// per edge dominate the ~80-instruction inner loop (measured ~2x the byte
// floor on final13682-fp32, profiles/r01_final13682_implicit_fp32.md).
// Repacking the 24 per-edge J values into 16-byte vector groups
// ([group][nL][VEC], VEC = 16B/sizeof(T)) turns them into NG=24/VEC
// dwordx4 loads (6 for fp32, 12 for fp64), still fully coalesced across
// the 64 consecutive-edge lanes.  The pack runs once per ACCEPTED LM step
// (its cost amortizes over the ~100 PCG iterations that read it); the
// packed buffers are single-buffered so the captured PCG graph needs no
// pointer indirection for them.
// (The standalone kPackJPrimary pass was folded into kAssembleEdge's
// register writes in r2.)

// Packed E^T x (implicit): kSpmvEtx's run scan over t_e = Jp^T W (Jc x)
// from the vector-group J.  The accepted r is read through the device
// pointer slots so a captured graph stays valid across accept-time flips.
template <typename T, int CD, int PD, int RD, bool HASINFO>
__global__ void kSpmvEtxPk(int64_t nL, const int* __restrict__ camOf,
                           const int* __restrict__ ptOf,
                           const T* __restrict__ Jpk,
                           const T* const* __restrict__ jSlots,
                           const T* __restrict__ info, int lossKind, T lossD2,
                           const T* __restrict__ xPad,
                           T* __restrict__ out) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int RW = RD * (RD + 1) / 2;
  constexpr int CR = CD * RD, PR = PD * RD;
  constexpr int NG = PackedEdge<T, CD, PD, RD, true>::NG;
  const T* rBak = jSlots[2];
  const int lane = threadIdx.x & 63;
  const int64_t nWork = ((nL + kBlk - 1) / kBlk) * (int64_t)kBlk;
  for (int64_t j0 = blockIdx.x * (int64_t)kBlk + threadIdx.x; j0 < nWork;
       j0 += (int64_t)gridDim.x * kBlk) {
    const bool active = j0 < nL;
    const int64_t j = active ? j0 : nL - 1;
    const int pt = ptOf[j];
    T o[PD];
    for (int k = 0; k < PD; ++k) o[k] = T(0);
    if (active) {
      constexpr int XP = PackedEdge<T, CD, PD, RD, true>::XP;
      const TV* xv4 = (const TV*)(xPad + (int64_t)camOf[j] * XP);
      TV xbuf[XP / VEC];
#pragma unroll
      for (int l = 0; l < XP / VEC; ++l) xbuf[l] = xv4[l];
      TV buf[NG];
      const TV* src = (const TV*)Jpk;
#pragma unroll
      for (int g = 0; g < NG; ++g) buf[g] = src[(int64_t)g * nL + j];
      T u[RD];
#pragma unroll
      for (int rr = 0; rr < RD; ++rr) {
        T v = T(0);
#pragma unroll
        for (int i = 0; i < CD; ++i) {
          const int k = i * RD + rr;
          v += buf[k / VEC][k % VEC] * xbuf[i / VEC][i % VEC];
        }
        u[rr] = v;
      }
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
#pragma unroll
      for (int k = 0; k < PD; ++k) {
        T v = T(0);
#pragma unroll
        for (int rr = 0; rr < RD; ++rr) {
          const int kk = CR + k * RD + rr;
          v += buf[kk / VEC][kk % VEC] * u[rr];
        }
        o[k] = v;
      }
    }
    waveSegScan(pt, lane, o);
    if (runTailTiled(pt, lane, active, j0 == nL - 1))
      for (int k = 0; k < PD; ++k) atomicAdd(&out[PD * pt + k], o[k]);
  }
}

// Scan-free E^T x variant (env MEGBA_ETX_ATOMIC=1): PD atomicAdds per
// edge instead of the wave segmented scan + tail atomics.  The scan costs
// ~16 dependent shuffle instructions per edge; the atomics serialize on
// the ~degree-5 same-point runs.  Which wins is measured, not assumed.
template <typename T, int CD, int PD, int RD, bool HASINFO>
__global__ void kSpmvEtxPkAtomic(int64_t nL, const int* __restrict__ camOf,
                                 const int* __restrict__ ptOf,
                                 const T* __restrict__ Jpk,
                                 const T* const* __restrict__ jSlots,
                                 const T* __restrict__ info, int lossKind,
                                 T lossD2, const T* __restrict__ xPad,
                                 T* __restrict__ out) {
  const T* rBak = jSlots[2];
  for (int64_t j = blockIdx.x * (int64_t)kBlk + threadIdx.x; j < nL;
       j += (int64_t)gridDim.x * kBlk) {
    const int pt = ptOf[j];
    using PE = PackedEdge<T, CD, PD, RD, true>;
    typename PackVec<T>::type xbuf[PE::NX], buf[PE::NG];
    loadXPadded<T>(xPad, camOf[j], xbuf);
    loadGroups<T>(Jpk, nL, j, buf);
    T t[PD];
    packedEtx<T, CD, PD, RD, HASINFO>(buf, xbuf, j, nL, info, rBak, lossKind,
                                      lossD2, t);
    for (int k = 0; k < PD; ++k) atomicAdd(&out[PD * pt + k], t[k]);
  }
}

// ---------------------------------------------------------------------------
// E w chunk kernels (kSpmvEx, kSpmvExPk): one wave per <=256-row chunk of
// one camera's cam-sorted rows
// ---------------------------------------------------------------------------
// This wave's chunk: its camera and row range [lo, hi); false past the table.
__device__ __forceinline__ bool exChunk(int nChunks,
                                        const int* __restrict__ chCam,
                                        const int* __restrict__ chLo,
                                        const int* __restrict__ chHi,
                                        int& cam, int& lo, int& hi) {
  const int chunk = blockIdx.x;
  if (chunk >= nChunks) return false;
  cam = chCam[chunk];
  lo = chLo[chunk];
  hi = chHi[chunk];
  return true;
}

// w is stored 4-padded (stride 4 elements, 16B/32B aligned) so the
// per-edge gather is 1 (fp32) or 2 (fp64) vector loads instead of PD
// scalar loads — the gather is the TA-request hot spot of these kernels.
template <typename T>
constexpr int kWPadVecs = (4 * (int)sizeof(T) + 15) / 16;
template <typename T>
__device__ __forceinline__ void loadWPadded(
    const T* __restrict__ w, int pt,
    typename PackVec<T>::type (&wbuf)[kWPadVecs<T>]) {
  using TV = typename PackVec<T>::type;
  const TV* wp4 = (const TV*)(w + (int64_t)pt * 4);
#pragma unroll
  for (int l = 0; l < kWPadVecs<T>; ++l) wbuf[l] = wp4[l];
}

// Lane 0 (which holds the wave sum) adds the chunk's CD values to its camera.
template <typename T, int CD>
__device__ __forceinline__ void exFlush(const T (&acc)[CD], int cam,
                                        T* __restrict__ out) {
  if (threadIdx.x == 0) {
    T* oc = out + (int64_t)cam * CD;
    for (int i = 0; i < CD; ++i) atomicAdd(&oc[i], acc[i]);
  }
}

// Packed E w over the cam-sorted [wJc(CR), Jp(PR)] groups.
template <typename T, int CD, int PD, int RD>
__global__ __launch_bounds__(64) void kSpmvExPk(
    int nChunks, const int* __restrict__ chCam, const int* __restrict__ chLo,
    const int* __restrict__ chHi, const int* __restrict__ ptOfCam,
    const T* __restrict__ JCamPk, int64_t nL, const T* __restrict__ w,
    T* __restrict__ out) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int CR = CD * RD, PR = PD * RD;
  constexpr int NG = PackedEdge<T, CD, PD, RD, true>::NG;
  int cam, lo, hi;
  if (!exChunk(nChunks, chCam, chLo, chHi, cam, lo, hi)) return;
  T acc[CD];
  for (int i = 0; i < CD; ++i) acc[i] = T(0);
  const TV* src = (const TV*)JCamPk;
  for (int j = lo + (int)threadIdx.x; j < hi; j += 64) {
    TV wbuf[kWPadVecs<T>];
    loadWPadded<T>(w, ptOfCam[j], wbuf);
    TV buf[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) buf[g] = src[(int64_t)g * nL + j];
    T u[RD];
#pragma unroll
    for (int rr = 0; rr < RD; ++rr) {
      T v = T(0);
#pragma unroll
      for (int k = 0; k < PD; ++k) {
        const int kk = CR + k * RD + rr;
        v += buf[kk / VEC][kk % VEC] * wbuf[k / VEC][k % VEC];
      }
      u[rr] = v;
    }
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      T v = T(0);
#pragma unroll
      for (int rr = 0; rr < RD; ++rr) {
        const int k = i * RD + rr;
        v += buf[k / VEC][k % VEC] * u[rr];
      }
      acc[i] += v;
    }
  }
  waveSumDown(acc);
  exFlush<T, CD>(acc, cam, out);
}

// ---------------------------------------------------------------------------
// Schur SpMV pieces
// ---------------------------------------------------------------------------
// temp[3*pt] = Hpl^T x per local point (fully local, no collective): one
// thread per primary-order edge (coalesced Hpl vector-group reads; the
// replicated camera vector x is L2-resident), wave segmented-scan over the
// point runs, atomics only at run tails.  Explicit mode only; the
// matrix-free product is kSpmvEtxPk.
template <typename T, int CD, int PD, int RD>
__global__ void kSpmvEtx(int64_t nL, const int* __restrict__ camOf,
                         const int* __restrict__ ptOf,
                         const T* __restrict__ Hpl, const T* __restrict__ x,
                         T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nWork = ((nL + kBlk - 1) / kBlk) * (int64_t)kBlk;
  for (int64_t j0 = blockIdx.x * (int64_t)kBlk + threadIdx.x; j0 < nWork;
       j0 += (int64_t)gridDim.x * kBlk) {
    const bool active = j0 < nL;
    const int64_t j = active ? j0 : nL - 1;
    const int pt = ptOf[j];
    T o[PD];
    for (int k = 0; k < PD; ++k) o[k] = T(0);
    if (active) {
      const T* xc = x + (int64_t)camOf[j] * CD;
      typename PackVec<T>::type buf[PackedEdge<T, CD, PD, RD, false>::NG];
      loadGroups<T>(Hpl, nL, j, buf);
      packedHplTx<T, CD, PD>(buf, [&](int i) { return xc[i]; }, o);
    }
    waveSegScan(pt, lane, o);
    if (runTailTiled(pt, lane, active, j0 == nL - 1))
      for (int k = 0; k < PD; ++k) atomicAdd(&out[PD * pt + k], o[k]);
  }
}

// out[9*cam] += E w partials: one wave per <=256-row chunk of one camera's
// cam-sorted rows; per-lane partials, wave-wide shuffle reduce, one
// atomicAdd set per chunk.  Caller allreduces 9*ncam (the ONLY per-PCG-
// iteration collective).
template <typename T, int CD, int PD>
__global__ __launch_bounds__(64) void kSpmvEx(
    int nChunks, const int* __restrict__ chCam, const int* __restrict__ chLo,
    const int* __restrict__ chHi, const int* __restrict__ ptOfCam,
    const T* __restrict__ HplCam, int64_t nL, const T* __restrict__ w,
    T* __restrict__ out) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int NGH = (CD * PD + VEC - 1) / VEC;
  int cam, lo, hi;
  if (!exChunk(nChunks, chCam, chLo, chHi, cam, lo, hi)) return;
  T acc[CD];
  for (int i = 0; i < CD; ++i) acc[i] = T(0);
  const TV* src = (const TV*)HplCam;
  for (int j = lo + (int)threadIdx.x; j < hi; j += 64) {
    TV wbuf[kWPadVecs<T>];
    loadWPadded<T>(w, ptOfCam[j], wbuf);
    TV buf[NGH];
#pragma unroll
    for (int g = 0; g < NGH; ++g) buf[g] = src[(int64_t)g * nL + j];
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      T v = T(0);
#pragma unroll
      for (int k = 0; k < PD; ++k) {
        const int kk = i * PD + k;
        v += buf[kk / VEC][kk % VEC] * wbuf[k / VEC][k % VEC];
      }
      acc[i] += v;
    }
  }
  waveSumDown(acc);
  exFlush<T, CD>(acc, cam, out);
}

// ---------------------------------------------------------------------------
// Fused Schur apply:  out[CD*ncam] += E Cinv E^T x  in ONE pass.
// ---------------------------------------------------------------------------
// The separate-pass pipeline (kSpmvEtx -> applyCinv -> kSpmvEx) reads the
// per-edge J/Hpl data twice per PCG iteration and gathers the 3*npt w
// vector by point id from the cam-sorted pass — on big-fp32 problems that
// gather fetches a full 64 B line for 12 used bytes and was measured at
// ~2x the byte floor (profiles/r01_final13682_implicit_fp32.md).  Here the
// edges are processed in primary (pt,cam)-sorted order in WINDOWS of <=64
// edges aligned to point-run boundaries (host-built table), one wave per
// window:
//   1. each lane evaluates its edge's t_e = Jp^T W (Jc x)  (x is the
//      replicated CD*ncam vector, L2-resident),
//   2. a wave segmented-scan sums t_e over each point run; the run tail
//      applies the PD x PD Cinv block: w_p = Cinv t_p,
//   3. w_p is broadcast back to the run's lanes (tail-lane shuffle) and
//      each lane scatters its edge's E-contribution Jc^T W (Jp w_p) with
//      CD atomicAdds into the small L2-resident camera vector.
// J (or Hpl) is read ONCE, w never exists in HBM, and the scan/broadcast
// replace both the temp round-trip and the gather.  Point runs longer
// than 64 edges (high-degree landmarks) fall back to the classic path:
// their windows only accumulate t partials into `temp` (phase 1 flag);
// kFusedLongW then applies Cinv for those points and kFusedLongScatter
// finishes their E-contributions.
// The per-edge and per-run steps (fusedLoadEdge / fusedScatter, the window
// scan, Cinv at the tail, the tail broadcast) are in edge_ops.hpp; what is
// left in each window kernel is its loop and its sink.
template <typename T, int CD, int PD, int RD, bool IMP, bool HASINFO>
__global__ __launch_bounds__(256) void kSchurFused(
    int nWin, const int64_t* __restrict__ winLo,
    const int64_t* __restrict__ winHi, const unsigned char* __restrict__ winFlag,
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ Hpl, const T* const* __restrict__ jSlots,
    const T* __restrict__ info, int lossKind, T lossD2,
    const T* __restrict__ xPad, const T* __restrict__ HllInv,
    T* __restrict__ temp, T* __restrict__ out) {
  constexpr int PP = PD * PD;
  const T* Jc = IMP ? jSlots[0] : nullptr;
  const T* Jp = IMP ? jSlots[1] : nullptr;
  const T* rBak = IMP ? jSlots[2] : nullptr;
  const int lane = threadIdx.x & 63;
  for (int w = blockIdx.x * 4 + ((int)threadIdx.x >> 6); w < nWin;
       w += (int)gridDim.x * 4) {
    const int64_t lo = winLo[w], hi = winHi[w];
    const bool active = lo + lane < hi;
    const int64_t j = active ? lo + lane : hi - 1;
    const int pt = ptOf[j];
    T jcv[RD][CD], jpv[RD][PD], hplv[CD][PD], t[PD];
    for (int k = 0; k < PD; ++k) t[k] = T(0);
    if (active)
      fusedLoadEdge<T, CD, PD, RD, IMP, HASINFO>(
          j, nL, camOf, Hpl, Jc, Jp, info, rBak, lossKind, lossD2, xPad,
          jcv, jpv, hplv, t);
    waveSegScan(pt, lane, t);
    const bool tail = runTailWindow(pt, lane, active, lo, hi);
    if (winFlag[w]) {
      // segment of a >64-edge run: partials only (finished by the long-run
      // kernels)
      if (tail)
        for (int k = 0; k < PD; ++k) atomicAdd(&temp[PD * pt + k], t[k]);
      continue;
    }
    T wv[PD];
    for (int k = 0; k < PD; ++k) wv[k] = T(0);
    if (tail) cinvApply<T, PD>(HllInv + (int64_t)pt * PP, t, wv);
    tailBroadcast(tail, lane, wv);
    if (active)
      fusedScatter<T, CD, PD, RD, IMP, HASINFO>(
          j, nL, camOf, info, rBak, lossKind, lossD2, jcv, jpv, hplv, wv,
          out);
  }
}

// Fused E^T x + Cinv over run-aligned windows (the winning half of the
// kSchurFused experiment): each window's runs are complete, so the run
// TAIL applies the PD x PD Cinv block to the scanned t_p and stores
// w_p = Cinv E^T x straight into the 4-padded w vector — no temp
// round-trip, no zeroing, no atomics, and the separate Cinv pass
// disappears.  Long (>64-edge) runs fall back to temp partials finished
// by kFusedLongW.  E w then proceeds from wPad as usual (the gather-side
// alternative, a fused scatter, measured 5x worse — Experiment 1).
template <typename T, int CD, int PD, int RD, bool IMP, bool HASINFO>
__global__ __launch_bounds__(256) void kEtxCinvFused(
    int nWin, const int64_t* __restrict__ winLo,
    const int64_t* __restrict__ winHi, const unsigned char* __restrict__ winFlag,
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ Hpl, const T* const* __restrict__ jSlots,
    const T* __restrict__ info, int lossKind, T lossD2,
    const T* __restrict__ xPad, const T* __restrict__ HllInv,
    T* __restrict__ temp, T* __restrict__ wPad) {
  constexpr int PP = PD * PD;
  const T* Jc = IMP ? jSlots[0] : nullptr;
  const T* Jp = IMP ? jSlots[1] : nullptr;
  const T* rBak = IMP ? jSlots[2] : nullptr;
  const int lane = threadIdx.x & 63;
  for (int w = blockIdx.x * 4 + ((int)threadIdx.x >> 6); w < nWin;
       w += (int)gridDim.x * 4) {
    const int64_t lo = winLo[w], hi = winHi[w];
    const bool active = lo + lane < hi;
    const int64_t j = active ? lo + lane : hi - 1;
    const int pt = ptOf[j];
    T jcv[RD][CD], jpv[RD][PD], hplv[CD][PD], t[PD];
    for (int k = 0; k < PD; ++k) t[k] = T(0);
    if (active)
      fusedLoadEdge<T, CD, PD, RD, IMP, HASINFO>(
          j, nL, camOf, Hpl, Jc, Jp, info, rBak, lossKind, lossD2, xPad,
          jcv, jpv, hplv, t);
    waveSegScan(pt, lane, t);
    const bool tail = runTailWindow(pt, lane, active, lo, hi);
    if (winFlag[w]) {
      if (tail)
        for (int k = 0; k < PD; ++k) atomicAdd(&temp[PD * pt + k], t[k]);
      continue;
    }
    if (tail)
      cinvApplyPad<T, PD>(HllInv + (int64_t)pt * PP, t,
                          wPad + (int64_t)pt * 4);
  }
}

// Long-run phase 2: w_p = Cinv temp_p for the listed high-degree points,
// stored into the 4-padded w vector.
template <typename T, int PD>
__global__ void kFusedLongW(int nPts, const int* __restrict__ longPts,
                            const T* __restrict__ HllInv,
                            const T* __restrict__ temp, T* __restrict__ w,
                            int wStride) {
  constexpr int PP = PD * PD;
  for (int idx = blockIdx.x * (int)blockDim.x + (int)threadIdx.x; idx < nPts;
       idx += (int)gridDim.x * (int)blockDim.x) {
    const int pt = longPts[idx];
    const T* tp = temp + PD * pt;
    T* wp = w + (int64_t)wStride * pt;
    cinvApply<T, PD>(HllInv + (int64_t)pt * PP, tp, wp);
  }
}

// Long-run phase 3: finish the flagged windows' E-contributions with w
// read from the global vector.
template <typename T, int CD, int PD, int RD, bool IMP, bool HASINFO>
__global__ __launch_bounds__(256) void kFusedLongScatter(
    int nFlag, const int* __restrict__ flagWins,
    const int64_t* __restrict__ winLo, const int64_t* __restrict__ winHi,
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ Hpl, const T* const* __restrict__ jSlots,
    const T* __restrict__ info, int lossKind, T lossD2,
    const T* __restrict__ xPad, const T* __restrict__ w,
    T* __restrict__ out) {
  const T* Jc = IMP ? jSlots[0] : nullptr;
  const T* Jp = IMP ? jSlots[1] : nullptr;
  const T* rBak = IMP ? jSlots[2] : nullptr;
  const int lane = threadIdx.x & 63;
  for (int f = blockIdx.x * 4 + ((int)threadIdx.x >> 6); f < nFlag;
       f += (int)gridDim.x * 4) {
    const int wi = flagWins[f];
    const int64_t lo = winLo[wi], hi = winHi[wi];
    if (lo + lane >= hi) continue;
    const int64_t j = lo + lane;
    const int pt = ptOf[j];
    T jcv[RD][CD], jpv[RD][PD], hplv[CD][PD], t[PD];
    fusedLoadEdge<T, CD, PD, RD, IMP, HASINFO>(
        j, nL, camOf, Hpl, Jc, Jp, info, rBak, lossKind, lossD2, xPad, jcv,
        jpv, hplv, t);
    T wv[PD];
    for (int k = 0; k < PD; ++k) wv[k] = w[PD * pt + k];
    fusedScatter<T, CD, PD, RD, IMP, HASINFO>(
        j, nL, camOf, info, rBak, lossKind, lossD2, jcv, jpv, hplv, wv,
        out);
  }
}

// ---------------------------------------------------------------------------
// Single-pass Schur apply with an LDS-resident camera accumulator
// ---------------------------------------------------------------------------
// kSchurFused reads J once but loses to the two-pass pipeline because its
// scatter is CD address-divergent GLOBAL atomics per edge.  When the whole
// camera-side output (CD*ncam values of T) fits one CU's LDS, a persistent
// workgroup per CU keeps a private copy of it in LDS, scatters with LDS
// atomics (native ds_add_f64 / ds_add_f32) and writes its copy out once:
//   - workgroup b of G owns the contiguous window slice
//     [nWin*b/G, nWin*(b+1)/G) of the run-aligned window table, its waves
//     stride through the slice (one contiguous stream of the pt-sorted J),
//   - per window the math is kSchurFused's (t_e, segmented scan, Cinv at the
//     run tail, tail-mask broadcast); the implicit edge comes from the
//     PACKED primary (vector-group loads, as kSpmvEtxPk) and stays in
//     registers for the scatter side,
//   - flagged windows (segments of >64-edge runs) only add their t
//     partials to `temp`; kFusedLongW / kFusedLongScatter finish them on
//     the global output after the flush,
//   - the flush is plain coalesced stores to row b of rows[G][nc];
//     kLdsRowsReduce sums the G rows in fixed order and OVERWRITES out, so
//     the cross-workgroup sum is order-fixed and out needs no memset.
// A workgroup with an empty slice still zeroes and flushes its row.
template <typename T, int CD, int PD, int RD, bool IMP, bool HASINFO>
__global__ __launch_bounds__(1024) void kSchurFusedLds(
    int nWin, const int64_t* __restrict__ winLo,
    const int64_t* __restrict__ winHi, const unsigned char* __restrict__ winFlag,
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ Hpl, const T* __restrict__ Jpk,
    const T* const* __restrict__ jSlots, const T* __restrict__ info,
    int lossKind, T lossD2, const T* __restrict__ xPad,
    const T* __restrict__ HllInv, T* __restrict__ temp, int nc,
    T* __restrict__ rows) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int PP = PD * PD;
  constexpr int RW = RD * (RD + 1) / 2;
  constexpr int CR = CD * RD, PR = PD * RD;
  constexpr int NG = PackedEdge<T, CD, PD, RD, IMP>::NG;
  constexpr int XP = PackedEdge<T, CD, PD, RD, IMP>::XP;
  extern __shared__ __align__(16) unsigned char ldsRaw[];
  T* acc = reinterpret_cast<T*>(ldsRaw);
  for (int i = (int)threadIdx.x; i < nc; i += (int)blockDim.x) acc[i] = T(0);
  __syncthreads();
  const T* rBak = IMP ? jSlots[2] : nullptr;
  const TV* src = (const TV*)(IMP ? Jpk : Hpl);
  const int lane = threadIdx.x & 63;
  const int nWave = (int)blockDim.x >> 6;
  const int wBeg = (int)((int64_t)nWin * blockIdx.x / gridDim.x);
  const int wEnd = (int)((int64_t)nWin * (blockIdx.x + 1) / gridDim.x);
  for (int w = wBeg + ((int)threadIdx.x >> 6); w < wEnd; w += nWave) {
    const int64_t lo = winLo[w], hi = winHi[w];
    const bool flagged = winFlag[w] != 0;
    const bool active = lo + lane < hi;
    const int64_t j = active ? lo + lane : hi - 1;
    const int pt = ptOf[j];
    const int cam = camOf[j];
    TV buf[NG];
    T iw[RW];
    T lw = T(1);
    T t[PD];
    for (int k = 0; k < PD; ++k) t[k] = T(0);
    if (active) {
      const TV* xv4 = (const TV*)(xPad + (int64_t)cam * XP);
      TV xbuf[XP / VEC];
#pragma unroll
      for (int l = 0; l < XP / VEC; ++l) xbuf[l] = xv4[l];
      // The packed groups are read once per apply, by one lane each, so they
      // are loaded non-temporal: the intent is that the stream leaves what
      // every apply re-reads (HllInv, camOf/ptOf, the rows) in the last-level
      // cache.  Measured on Venice in profiles/r05_pcg_fusion.md.
#pragma unroll
      for (int g = 0; g < NG; ++g)
        buf[g] = __builtin_nontemporal_load(&src[(int64_t)g * nL + j]);
      if (IMP) {
        T u[RD];
#pragma unroll
        for (int rr = 0; rr < RD; ++rr) {
          T v = T(0);
#pragma unroll
          for (int i = 0; i < CD; ++i) {
            const int k = i * RD + rr;
            v += buf[k / VEC][k % VEC] * xbuf[i / VEC][i % VEC];
          }
          u[rr] = v;
        }
        if (HASINFO) {
          for (int k = 0; k < RW; ++k) iw[k] = info[RW * j + k];
          T wu[RD];
          for (int i = 0; i < RD; ++i) {
            T v = T(0);
            for (int k = 0; k < RD; ++k) v += iw[symIdx<RD>(i, k)] * u[k];
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
          lw = lossWeight(lossKind, lossD2, ss);
          for (int rr = 0; rr < RD; ++rr) u[rr] *= lw;
        }
#pragma unroll
        for (int k = 0; k < PD; ++k) {
          T v = T(0);
#pragma unroll
          for (int rr = 0; rr < RD; ++rr) {
            const int kk = CR + k * RD + rr;
            v += buf[kk / VEC][kk % VEC] * u[rr];
          }
          t[k] = v;
        }
      } else {
#pragma unroll
        for (int i = 0; i < CD; ++i) {
          const T xi = xbuf[i / VEC][i % VEC];
#pragma unroll
          for (int k = 0; k < PD; ++k) {
            const int kk = i * PD + k;
            t[k] += buf[kk / VEC][kk % VEC] * xi;
          }
        }
      }
    }
    // segmented inclusive scan over the window's point runs
    for (int off = 1; off < 64; off <<= 1) {
      const int ppt = __shfl_up(pt, off, 64);
      const bool join = lane >= off && ppt == pt;
      if (__ballot(join) == 0ull) break;
      T a[PD];
      for (int k = 0; k < PD; ++k) a[k] = __shfl_up(t[k], off, 64);
      if (join)
        for (int k = 0; k < PD; ++k) t[k] += a[k];
    }
    const int nextPt = __shfl_down(pt, 1, 64);
    const bool tail = active && (lo + lane == hi - 1 || nextPt != pt);
    if (flagged) {
      if (tail)
        for (int k = 0; k < PD; ++k) atomicAdd(&temp[PD * pt + k], t[k]);
      continue;
    }
    T wv[PD];
    for (int k = 0; k < PD; ++k) wv[k] = T(0);
    if (tail) {
      const T* inv = HllInv + (int64_t)pt * PP;
      for (int i = 0; i < PD; ++i) {
        T v = T(0);
        for (int k = 0; k < PD; ++k) v += inv[i * PD + k] * t[k];
        wv[i] = v;
      }
    }
    // broadcast w_p from the run tail back to every lane of the run
    const unsigned long long tails = __ballot(tail);
    const unsigned long long from = tails >> lane;
    const int tl = from ? lane + __ffsll((long long)from) - 1 : lane;
    for (int k = 0; k < PD; ++k) wv[k] = __shfl(wv[k], tl, 64);
    if (!active) continue;
    T* oc = acc + cam * CD;
    if (IMP) {
      T u[RD];
#pragma unroll
      for (int rr = 0; rr < RD; ++rr) {
        T v = T(0);
#pragma unroll
        for (int k = 0; k < PD; ++k) {
          const int kk = CR + k * RD + rr;
          v += buf[kk / VEC][kk % VEC] * wv[k];
        }
        u[rr] = v;
      }
      if (HASINFO) {
        T wu[RD];
        for (int i = 0; i < RD; ++i) {
          T v = T(0);
          for (int k = 0; k < RD; ++k) v += iw[symIdx<RD>(i, k)] * u[k];
          wu[i] = v;
        }
        for (int i = 0; i < RD; ++i) u[i] = wu[i];
      }
      if (lossKind)
        for (int rr = 0; rr < RD; ++rr) u[rr] *= lw;
#pragma unroll
      for (int i = 0; i < CD; ++i) {
        T v = T(0);
#pragma unroll
        for (int rr = 0; rr < RD; ++rr) {
          const int k = i * RD + rr;
          v += buf[k / VEC][k % VEC] * u[rr];
        }
        atomicAdd(&oc[i], v);
      }
    } else {
#pragma unroll
      for (int i = 0; i < CD; ++i) {
        T v = T(0);
#pragma unroll
        for (int k = 0; k < PD; ++k) {
          const int kk = i * PD + k;
          v += buf[kk / VEC][kk % VEC] * wv[k];
        }
        atomicAdd(&oc[i], v);
      }
    }
  }
  __syncthreads();
  T* row = rows + (int64_t)blockIdx.x * nc;
  for (int i = (int)threadIdx.x; i < nc; i += (int)blockDim.x) row[i] = acc[i];
}

// ---------------------------------------------------------------------------
// Recomputed-J form of the LDS single-pass apply (BAL (9,3,2), implicit)
// ---------------------------------------------------------------------------
// For the built-in BAL residual the 24 J values an edge streams in
// kSchurFusedLds are a pure function of the accepted camera and point.
// kBalSnapshot keeps that linearisation point per accepted step: one
// balCameraPart row per camera (the transcendentals, once per camera) and
// the 4-padded points of the local shard.  kSchurFusedLdsRc then rebuilds
// [Jc, Jp] per edge with balEdgePart (J = dres/dP [dP/daa, I, .] and
// Jp = dres/dP R, one reciprocal) instead of loading the packed groups;
// window slices, scan, Cinv, broadcast, weighting, LDS scatter and flush are
// kSchurFusedLds's.  Flagged windows and the long-run finishers keep using
// the stored grad-major J.
//
// Camera data lives in one row table camRow[ncam][RcRow<T>::LEN]
// (rc_tile.hpp): kBalSnapshot writes the balCameraPart row, and the writers
// of the padded x (kBetaPPad, kPadX) put the product's input behind it, so an
// edge's whole camera side is one 64-byte-aligned row.  The cameras of a
// window are all different as a rule, and a per-lane load of 16 bytes then
// touches 64 cache lines per wave instruction.  The STAGED instance loads
// every 64-byte segment of the window's 64 rows once, four neighbouring lanes
// per segment, and hands each lane its own row through a wave-private LDS
// tile behind the accumulator (one segment of the 64 rows at a time,
// rcTileSlot's layout).  The per-lane instance keeps the two tables it had
// (camera rows at a kBalCamRow stride, x in the XP-padded vector): on the
// 192-byte rows its loads measured slower.  The tile is written and read by one wave only, so a
// wavefront-scope fence orders it; the window loop holds no block barrier.
template <typename T>
__global__ void kBalSnapshot(int ncam, int ptLo, int npL,
                             const T* __restrict__ params,
                             T* __restrict__ camRow, int camStride,
                             T* __restrict__ ptAcc) {
  const T* pts = params + (int64_t)ncam * 9;
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)ncam + npL; idx += (int64_t)gridDim.x * kBlk) {
    if (idx < ncam) {
      T row[kBalCamRow];
      balCameraPart<T>(params + idx * 9, row);
      for (int k = 0; k < kBalCamRow; ++k) camRow[idx * camStride + k] = row[k];
    } else {
      const int64_t p = ptLo + (idx - ncam);
      for (int k = 0; k < 3; ++k) ptAcc[p * 4 + k] = pts[p * 3 + k];
      ptAcc[p * 4 + 3] = T(0);
    }
  }
}

// Workgroups of at most 512 threads: holding next window's indices and the
// Cinv block across the edge arithmetic takes 164-178 VGPRs in fp64, which
// 16 waves per CU cannot have without scratch (profiles/kernel_resources.md).
constexpr int kLdsRcMaxThreads = 512;
template <typename T, bool HASINFO, bool STAGED>
__global__ __launch_bounds__(kLdsRcMaxThreads) void kSchurFusedLdsRc(
    int nWin, const int64_t* __restrict__ winLo,
    const int64_t* __restrict__ winHi, const unsigned char* __restrict__ winFlag,
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ camRow, int camStride, const T* __restrict__ xPad,
    int xStride, const T* __restrict__ ptAcc,
    const unsigned char* __restrict__ camFixed,
    const unsigned char* __restrict__ ptFixed,
    const T* const* __restrict__ jSlots, const T* __restrict__ info,
    int lossKind, T lossD2, const T* __restrict__ HllInv,
    T* __restrict__ temp, int nc, T* __restrict__ rows) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int CD = 9, PD = 3, RD = 2;
  constexpr int PP = PD * PD;
  constexpr int RW = RD * (RD + 1) / 2;
  constexpr int XP = PackedEdge<T, CD, PD, RD, true>::XP;
  constexpr int LEN = RcRow<T>::LEN;
  constexpr int SEGS = RcRow<T>::SEGS;
  // 16-byte chunks of a row that an edge consumes: camera part, then x
  constexpr int NUSE = (kRcXOff + XP) / VEC;
  static_assert(kRcXOff % VEC == 0 && kRcXOff >= kBalCamRow &&
                    kRcXOff + XP <= LEN && VEC * (int)sizeof(T) == kRcChunkBytes,
                "row layout");
  extern __shared__ __align__(16) unsigned char ldsRaw[];
  T* acc = reinterpret_cast<T*>(ldsRaw);
  for (int i = (int)threadIdx.x; i < nc; i += (int)blockDim.x) acc[i] = T(0);
  __syncthreads();
  const T* rBak = jSlots[2];
  const int lane = threadIdx.x & 63;
  const int nWave = (int)blockDim.x >> 6;
  [[maybe_unused]] unsigned char* tile =
      ldsRaw + rcTileOffset(nc, (int)sizeof(T)) +
      ((int)threadIdx.x >> 6) * kRcTileBytes;
  const int wBeg = (int)((int64_t)nWin * blockIdx.x / gridDim.x);
  const int wEnd = (int)((int64_t)nWin * (blockIdx.x + 1) / gridDim.x);
  // With J gone the window is a chain of dependent memory latencies: table
  // -> ptOf/camOf -> gathers -> arithmetic -> scan -> Cinv.  The indices are
  // therefore loaded one window ahead and the tail lanes fetch Cinv before
  // the arithmetic, which leaves the gathers as the one exposed latency.
  const auto loadWindowTable = [&](int wi, int64_t& l, int64_t& h, bool& f) {
    l = winLo[wi];
    h = winHi[wi];
    f = winFlag[wi] != 0;
  };
  const auto loadWindowEdges = [&](int64_t l, int64_t h, int& p, int& c) {
    const int64_t jj = l + lane < h ? l + lane : h - 1;
    p = ptOf[jj];
    c = camOf[jj];
  };
  const auto loadWindow = [&](int wi, int64_t& l, int64_t& h, bool& f, int& p,
                              int& c) {
    loadWindowTable(wi, l, h, f);
    loadWindowEdges(l, h, p, c);
  };
  int w = wBeg + ((int)threadIdx.x >> 6);
  int64_t lo = 0, hi = 0, loN = 0, hiN = 0;
  bool flagged = false, flaggedN = false;
  int pt = 0, cam = 0, ptN = 0, camN = 0;
  if (w < wEnd) loadWindow(w, lo, hi, flagged, pt, cam);
  for (; w < wEnd; w += nWave, lo = loN, hi = hiN, flagged = flaggedN,
                   pt = ptN, cam = camN) {
    const bool active = lo + lane < hi;
    const int64_t j = active ? lo + lane : hi - 1;
    const bool tail = runTailWindow(pt, lane, active, lo, hi);
    T inv[PP];
    if (tail && !flagged)
      for (int k = 0; k < PP; ++k) inv[k] = HllInv[(int64_t)pt * PP + k];
    // an edge with a fixed end has Jc = 0 or Jp = 0 (kForward): both its
    // t_e = Jp^T W Jc x and its scatter Jc^T W Jp w are exactly zero
    const bool live = active && !(camFixed && camFixed[cam]) &&
                      !(ptFixed && ptFixed[pt]);
    T jc[RD][CD], jp[RD][PD];
    T iw[RW];
    T lw = T(1);
    T t[PD];
    for (int k = 0; k < PD; ++k) t[k] = T(0);
    // rbuf: this lane's camera row in 16-byte chunks
    TV rbuf[STAGED ? SEGS * kRcSegChunks : NUSE], pbuf[4 / VEC];
    [[maybe_unused]] TV gbuf[STAGED ? SEGS : 1][kRcSegChunks];
    if constexpr (STAGED) {
      // All 64 lanes load, whatever active / live say: the clamped j gives
      // every lane a valid camera, and a lane fetches for its neighbours.
      // Instruction i of segment s: this lane loads chunk lane % 4 of
      // segment s of the row of lane 16 i + lane / 4, so a lane quad reads
      // 64 contiguous, 64-byte-aligned bytes.
      const TV* src[kRcSegChunks];
#pragma unroll
      for (int i = 0; i < kRcSegChunks; ++i) {
        const int ci = __shfl(cam, 16 * i + (lane >> 2), 64);
        src[i] = (const TV*)(camRow + (int64_t)ci * LEN) + (lane & 3);
      }
#pragma unroll
      for (int s = 0; s < SEGS; ++s)
#pragma unroll
        for (int i = 0; i < kRcSegChunks; ++i)
          gbuf[s][i] = src[i][s * kRcSegChunks];
    } else if (live) {
      // per-lane: camera part and x from wherever the engine keeps them
      // (camStride / xStride), as before the row table
      const TV* xv4 = (const TV*)(xPad + (int64_t)cam * xStride);
#pragma unroll
      for (int l = 0; l < XP / VEC; ++l) rbuf[kRcXOff / VEC + l] = xv4[l];
      const TV* cv = (const TV*)(camRow + (int64_t)cam * camStride);
#pragma unroll
      for (int l = 0; l < kBalCamRow / VEC; ++l) rbuf[l] = cv[l];
    }
    if (live) {
      const TV* pv = (const TV*)(ptAcc + (int64_t)pt * 4);
#pragma unroll
      for (int l = 0; l < 4 / VEC; ++l) pbuf[l] = pv[l];
    }
    // The staged instance reads the next window's table entry without a
    // branch (clamped to the slice) and its edges after the tile rounds: the
    // waits on the row segments then count the loads issued behind them
    // instead of draining them, and ptOf / camOf stay in flight across the
    // arithmetic.
    if constexpr (STAGED)
      loadWindowTable(w + nWave < wEnd ? w + nWave : w, loN, hiN, flaggedN);
    else if (w + nWave < wEnd)
      loadWindow(w + nWave, loN, hiN, flaggedN, ptN, camN);
    if constexpr (STAGED) {
      // every load above is issued before the first tile round
      __builtin_amdgcn_sched_barrier(0);
      // One segment of the 64 rows at a time through the wave's tile: four
      // 128-bit stores of what this lane fetched, four 128-bit loads of its
      // own row.  A wave's LDS operations complete in order; the fences keep
      // the compiler from moving them across each other.
#pragma unroll
      for (int s = 0; s < SEGS; ++s) {
#pragma unroll
        for (int i = 0; i < kRcSegChunks; ++i)
          *(TV*)(tile + rcTileSlot(16 * i + (lane >> 2), lane & 3)) =
              gbuf[s][i];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < kRcSegChunks; ++k)
          rbuf[s * kRcSegChunks + k] =
              *(const TV*)(tile + rcTileSlot(lane, k));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      loadWindowEdges(loN, hiN, ptN, camN);
    }
    if (live) {
      T row[kBalCamRow], X[4];
#pragma unroll
      for (int k = 0; k < kBalCamRow; ++k) row[k] = rbuf[k / VEC][k % VEC];
#pragma unroll
      for (int k = 0; k < 4; ++k) X[k] = pbuf[k / VEC][k % VEC];
      const T noMeas[RD] = {T(0), T(0)};
      T res[RD];  // unused: the accepted residual is read from rBak
      balEdgePart<T>(row, X, noMeas, res, jc, jp);
      T u[RD];
#pragma unroll
      for (int rr = 0; rr < RD; ++rr) {
        T v = T(0);
#pragma unroll
        for (int i = 0; i < CD; ++i)
          v += jc[rr][i] * rbuf[(kRcXOff + i) / VEC][(kRcXOff + i) % VEC];
        u[rr] = v;
      }
      if (HASINFO) {
        for (int k = 0; k < RW; ++k) iw[k] = info[RW * j + k];
        T wu[RD];
        for (int i = 0; i < RD; ++i) {
          T v = T(0);
          for (int k = 0; k < RD; ++k) v += iw[symIdx<RD>(i, k)] * u[k];
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
        lw = lossWeight(lossKind, lossD2, ss);
        for (int rr = 0; rr < RD; ++rr) u[rr] *= lw;
      }
#pragma unroll
      for (int k = 0; k < PD; ++k) {
        T v = T(0);
#pragma unroll
        for (int rr = 0; rr < RD; ++rr) v += jp[rr][k] * u[rr];
        t[k] = v;
      }
    }
    waveSegScan(pt, lane, t);
    if (flagged) {
      if (tail)
        for (int k = 0; k < PD; ++k) atomicAdd(&temp[PD * pt + k], t[k]);
      continue;
    }
    T wv[PD];
    for (int k = 0; k < PD; ++k) wv[k] = T(0);
    if (tail) cinvApply<T, PD>(inv, t, wv);
    tailBroadcast(tail, lane, wv);
    if (!live) continue;
    T* oc = acc + cam * CD;
    T u[RD];
#pragma unroll
    for (int rr = 0; rr < RD; ++rr) {
      T v = T(0);
#pragma unroll
      for (int k = 0; k < PD; ++k) v += jp[rr][k] * wv[k];
      u[rr] = v;
    }
    if (HASINFO) {
      T wu[RD];
      for (int i = 0; i < RD; ++i) {
        T v = T(0);
        for (int k = 0; k < RD; ++k) v += iw[symIdx<RD>(i, k)] * u[k];
        wu[i] = v;
      }
      for (int i = 0; i < RD; ++i) u[i] = wu[i];
    }
    if (lossKind)
      for (int rr = 0; rr < RD; ++rr) u[rr] *= lw;
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      T v = T(0);
#pragma unroll
      for (int rr = 0; rr < RD; ++rr) v += jc[rr][i] * u[rr];
      atomicAdd(&oc[i], v);
    }
  }
  __syncthreads();
  T* row = rows + (int64_t)blockIdx.x * nc;
  for (int i = (int)threadIdx.x; i < nc; i += (int)blockDim.x) row[i] = acc[i];
}

// Column sum over the G workgroup rows, in fixed order.  64 columns per
// block of kLdsRedWaves waves; every thread calls it with its column
// blockIdx.x * 64 + lane.  Each wave sums a contiguous share of the G rows,
// and wave 0 combines the shares through LDS in fixed order: the sum is
// returned to wave 0's lanes with col < nc, T(0) to everyone else.
constexpr int kLdsRedWaves = 16;
template <typename T>
__device__ __forceinline__ T ldsRowsColumnSum(int G, int nc,
                                              const T* __restrict__ rows,
                                              int col) {
  __shared__ T sm[kLdsRedWaves][64];
  const int lane = threadIdx.x & 63;
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
  T v = T(0);
  if (q == 0 && col < nc) {
    v = sm[0][lane];
    for (int k = 1; k < kLdsRedWaves; ++k) v += sm[k][lane];
  }
  return v;
}

// out[i] = sum over the G workgroup rows (overwrites out).
template <typename T>
__global__ __launch_bounds__(64 * kLdsRedWaves) void kLdsRowsReduce(
    int G, int nc, const T* __restrict__ rows, T* __restrict__ out) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const T v = ldsRowsColumnSum<T>(G, nc, rows, col);
  if (threadIdx.x < 64 && col < nc) out[col] = v;
}

// Block-diagonal matvec, one thread per output row.
// MODE 0: y = A x;  MODE 1: y = A x - y  (the reference's rw=1,dw=-1 gemv).
template <typename T, int D, int MODE>
__global__ void kBlockDiagMatVec(int nBlk, const T* __restrict__ A,
                                 const T* __restrict__ x, T* __restrict__ y) {
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)nBlk * D; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t b = idx / D;
    const T s = blockRowDot<T, D>(A, b, (int)(idx % D), x + b * D);
    y[idx] = (MODE == 0) ? s : s - y[idx];
  }
}

// Cinv apply writing the 4-padded w layout read by kSpmvExPk: one thread
// per point, whole padded slot written as 16/32-byte vector stores.
template <typename T, int PD>
__global__ void kCinvPad(int nBlk, const T* __restrict__ A,
                         const T* __restrict__ x, T* __restrict__ yPad) {
  for (int64_t b = blockIdx.x * (int64_t)kBlk + threadIdx.x; b < nBlk;
       b += (int64_t)gridDim.x * kBlk)
    cinvApplyPad<T, PD>(A + b * PD * PD, x + b * PD, yPad + b * 4);
}

// Pad the CD-stride camera vector to a 16B-aligned XP stride (one vector
// store per camera) so the E^T x per-edge gather is XP/VEC vector loads
// instead of CD divergent scalar loads.  The XP values of camera c go to
// dst + c * stride + off: (dXPad_, XP, 0) for the padded vector, and the x
// columns of the recompute path's camera row table (stride and off whole
// 16-byte groups).
template <typename T, int CD>
__global__ void kPadX(int ncam, const T* __restrict__ x, T* __restrict__ dst,
                      int stride, int off) {
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int XP = (CD + VEC - 1) / VEC * VEC;
  for (int64_t c = blockIdx.x * (int64_t)kBlk + threadIdx.x; c < ncam;
       c += (int64_t)gridDim.x * kBlk) {
    const T* xc = x + c * CD;
    TV* o = (TV*)(dst + c * stride + off);
    for (int l = 0; l < XP / VEC; ++l) {
      TV v;
      for (int q = 0; q < VEC; ++q) {
        const int k = l * VEC + q;
        v[q] = k < CD ? xc[k] : T(0);
      }
      o[l] = v;
    }
  }
}

}  // namespace
}  // namespace megba
