// Assembly kernels: per-edge pass + cam-sorted slab, camera-block
// accumulation, the cam-sorted finalize copies, damping and block inverses.
#pragma once

#include "../smallmat.hpp"
#include "edge_ops.hpp"
#include "gpu_common.hpp"

namespace megba {
namespace {

// ---------------------------------------------------------------------------
// Assembly
// ---------------------------------------------------------------------------
// Slab row layout (T values), written at the edge's CAM-sorted position:
//   [0..CD*PD)                    Hpl block (EXPL only)
//   [JCOFF..JCOFF+CD*RD)          Jc rows (col-major groups: jc[col][row])
//   [WROFF..WROFF+RD)             weighted residual rows
//   [WJCOFF..WJCOFF+CD*RD)        weighted Jc rows (HASINFO only)
//   [JPOFF..JPOFF+PD*RD)          Jp rows (implicit only)
template <int CD, int PD, int RD, bool EXPL, bool HASINFO>
struct SlabLayout {
  static constexpr int JCOFF = EXPL ? CD * PD : 0;
  static constexpr int WROFF = JCOFF + CD * RD;
  static constexpr int WJCOFF = WROFF + RD;
  static constexpr int JPOFF = WJCOFF + (HASINFO ? CD * RD : 0);
  static constexpr int SW = JPOFF + (EXPL ? 0 : PD * RD);
};

// Per-edge pass, primary ((pt,cam)-sorted) order: Hpl grad-major (for E^T x),
// the cam-sorted slab row, and the point-side Hll/g_p via a wave-level
// segmented scan (atomics only at point-run tails).
template <typename T, int CD, int PD, int RD, bool HASINFO, bool EXPL>
__global__ void kAssembleEdge(int64_t nL, const int* __restrict__ camOf,
                              const int* __restrict__ ptOf,
                              const T* __restrict__ r, const T* __restrict__ Jc,
                              const T* __restrict__ Jp,
                              const T* __restrict__ info, T* __restrict__ Hll,
                              T* __restrict__ Hpl, T* __restrict__ g, int ncam,
                              const int* __restrict__ camPos,
                              T* __restrict__ slab, int lossKind, T lossD2,
                              T* __restrict__ jPk) {
  using L = SlabLayout<CD, PD, RD, EXPL, HASINFO>;
  constexpr int RW = RD * (RD + 1) / 2;   // packed info entries
  constexpr int PH = PD * (PD + 1) / 2;   // packed Hll entries
  T* gp = g + (int64_t)ncam * CD;
  const int lane = threadIdx.x & 63;
  const int64_t nWork = ((nL + kBlk - 1) / kBlk) * (int64_t)kBlk;
  for (int64_t e0i = blockIdx.x * (int64_t)kBlk + threadIdx.x; e0i < nWork;
       e0i += (int64_t)gridDim.x * kBlk) {
    const bool active = e0i < nL;
    const int64_t e = active ? e0i : nL - 1;
    const int pt = ptOf[e];
    T hllP[PH], gpP[PD];
    for (int k = 0; k < PH; ++k) hllP[k] = T(0);
    for (int k = 0; k < PD; ++k) gpP[k] = T(0);
    if (active) {
      T jc[RD][CD], jp[RD][PD], rr[RD];
      for (int k = 0; k < CD; ++k)
        for (int row = 0; row < RD; ++row)
          jc[row][k] = Jc[((int64_t)(k * RD + row)) * nL + e];
      for (int k = 0; k < PD; ++k)
        for (int row = 0; row < RD; ++row)
          jp[row][k] = Jp[((int64_t)(k * RD + row)) * nL + e];
      for (int row = 0; row < RD; ++row) rr[row] = r[(int64_t)row * nL + e];
      T wjp[RD][PD], wr[RD];
      T wjc[RD][CD];
      if (HASINFO) {
        // HASINFO also covers robust-loss runs without an information
        // matrix (info == nullptr -> identity), since both need the
        // weighted Jc rows stored separately in the slab.
        T W[RW];
        if (info) {
          for (int k = 0; k < RW; ++k) W[k] = info[RW * e + k];
        } else {
          for (int k = 0; k < RW; ++k) W[k] = T(0);
          for (int i = 0; i < RD; ++i) W[symIdx<RD>(i, i)] = T(1);
        }
        if (lossKind) {
          T ss = T(0);
          for (int row = 0; row < RD; ++row) ss += rr[row] * rr[row];
          const T w = lossWeight(lossKind, lossD2, ss);
          for (int k = 0; k < RW; ++k) W[k] *= w;
        }
        for (int i = 0; i < RD; ++i) {
          for (int k = 0; k < CD; ++k) {
            T v = T(0);
            for (int j = 0; j < RD; ++j) v += W[symIdx<RD>(i, j)] * jc[j][k];
            wjc[i][k] = v;
          }
          for (int k = 0; k < PD; ++k) {
            T v = T(0);
            for (int j = 0; j < RD; ++j) v += W[symIdx<RD>(i, j)] * jp[j][k];
            wjp[i][k] = v;
          }
          T v = T(0);
          for (int j = 0; j < RD; ++j) v += W[symIdx<RD>(i, j)] * rr[j];
          wr[i] = v;
        }
      } else {
        for (int i = 0; i < RD; ++i) {
          for (int k = 0; k < PD; ++k) wjp[i][k] = jp[i][k];
          wr[i] = rr[i];
        }
      }
      T* row = slab + (int64_t)camPos[e] * L::SW;
      if (EXPL) {
        // Hpl stored as 16-byte vector groups ([group][nL][VEC]) so the
        // per-iteration E^T x / E w reads are dwordx4 loads (r2, same
        // treatment as the implicit packed J — profiles/r02_gather_bands.md)
        constexpr int VEC = PackVec<T>::VEC;
        constexpr int NGH = PackedEdge<T, CD, PD, RD, false>::NG;
        T v[NGH * VEC];
        for (int k = 0; k < NGH * VEC; ++k) v[k] = T(0);
        for (int a = 0; a < CD; ++a)
          for (int b = 0; b < PD; ++b) {
            T acc = T(0);
            for (int i = 0; i < RD; ++i) acc += jc[i][a] * wjp[i][b];
            v[a * PD + b] = acc;
            row[a * PD + b] = acc;
          }
        using TV = typename PackVec<T>::type;
        TV* o = (TV*)Hpl;
        for (int g = 0; g < NGH; ++g) {
          TV vv;
          for (int q = 0; q < VEC; ++q) vv[q] = v[g * VEC + q];
          o[(int64_t)g * nL + e] = vv;
        }
      }
      for (int k = 0; k < CD; ++k)
        for (int i = 0; i < RD; ++i) row[L::JCOFF + k * RD + i] = jc[i][k];
      for (int i = 0; i < RD; ++i) row[L::WROFF + i] = wr[i];
      if (HASINFO)
        for (int k = 0; k < CD; ++k)
          for (int i = 0; i < RD; ++i) row[L::WJCOFF + k * RD + i] = wjc[i][k];
      if (!EXPL) {
        for (int k = 0; k < PD; ++k)
          for (int i = 0; i < RD; ++i) row[L::JPOFF + k * RD + i] = jp[i][k];
        // primary-order packed [Jc, Jp] copy for the per-iteration E^T x
        // reads — written here from registers (the J values are already
        // loaded), replacing a separate full-pass pack kernel.
        {
          using TV = typename PackVec<T>::type;
          constexpr int VEC = PackVec<T>::VEC;
          constexpr int CR = CD * RD, PR = PD * RD;
          constexpr int NGJ = PackedEdge<T, CD, PD, RD, true>::NG;
          TV* o = (TV*)jPk;
          for (int gI = 0; gI < NGJ; ++gI) {
            TV v;
            for (int q = 0; q < VEC; ++q) {
              const int k = gI * VEC + q;
              v[q] = k < CR ? jc[k % RD][k / RD]
                            : (k < CR + PR ? jp[(k - CR) % RD][(k - CR) / RD]
                                           : T(0));
            }
            o[(int64_t)gI * nL + e] = v;
          }
        }
      }
      // point-side contributions (packed upper)
      for (int a = 0; a < PD; ++a)
        for (int b = a; b < PD; ++b) {
          T v = T(0);
          for (int i = 0; i < RD; ++i) v += jp[i][a] * wjp[i][b];
          hllP[symIdx<PD>(a, b)] = v;
        }
      for (int k = 0; k < PD; ++k) {
        T v = T(0);
        for (int i = 0; i < RD; ++i) v += jp[i][k] * wr[i];
        gpP[k] = -v;
      }
    }
    // segmented scan over the wave's point runs: edge_ops.hpp's waveSegScan
    // written out for the two arrays, because routing it through the helper
    // lowered this kernel's occupancy (profiles/r04_edge_ops_refactor.md)
    for (int off = 1; off < 64; off <<= 1) {
      const int ppt = __shfl_up(pt, off, 64);
      const bool join = lane >= off && ppt == pt;
      if (__ballot(join) == 0ull) break;
      T aH[PH], aG[PD];
      for (int k = 0; k < PH; ++k) aH[k] = __shfl_up(hllP[k], off, 64);
      for (int k = 0; k < PD; ++k) aG[k] = __shfl_up(gpP[k], off, 64);
      if (join) {
        for (int k = 0; k < PH; ++k) hllP[k] += aH[k];
        for (int k = 0; k < PD; ++k) gpP[k] += aG[k];
      }
    }
    const int nextPt = __shfl_down(pt, 1, 64);
    const bool tail = active && (lane == 63 || nextPt != pt || e0i == nL - 1);
    if (tail) {
      T* H = Hll + (int64_t)pt * PD * PD;
      for (int i = 0; i < PD; ++i)
        for (int j = 0; j < PD; ++j)
          atomicAdd(&H[i * PD + j], hllP[symIdx<PD>(i, j)]);
      for (int k = 0; k < PD; ++k)
        atomicAdd(&gp[(int64_t)pt * PD + k], gpP[k]);
    }
  }
}

// Camera blocks: one 128-thread block per <=256-row chunk of one camera's
// cam-sorted slab rows.  Rows are contiguous, staged through LDS in 128-row
// tiles; threads 0..CD*CD-1 each own one Hpp element, the next CD one g_c
// element; one atomicAdd per output per chunk.
template <typename T, int CD, int PD, int RD, bool HASINFO, bool EXPL>
__global__ __launch_bounds__(128) void kAssembleCam(
    int nChunks, const int* __restrict__ chCam, const int* __restrict__ chLo,
    const int* __restrict__ chHi, const T* __restrict__ slab,
    T* __restrict__ Hpp, T* __restrict__ g) {
  using L = SlabLayout<CD, PD, RD, EXPL, HASINFO>;
  constexpr int CC = CD * CD;
  constexpr int CR = CD * RD;
  constexpr int TE = 128;
  constexpr int ST = CR + RD + (HASINFO ? CR : 0);  // jc + wr (+ wjc)
  __shared__ T lds[TE * ST];
  const int chunk = blockIdx.x;
  if (chunk >= nChunks) return;
  const int cam = chCam[chunk];
  const int lo = chLo[chunk], hi = chHi[chunk];
  const int t = threadIdx.x;
  T acc = T(0);
  const int ti = t < CC ? t / CD : t - CC;
  const int tj = t < CC ? t % CD : 0;
  for (int s0 = lo; s0 < hi; s0 += TE) {
    const int nt = min(TE, hi - s0);
    for (int idx = t; idx < nt * ST; idx += 128) {
      const int row = idx / ST;
      const int k = idx % ST;
      const T* src = slab + (int64_t)(s0 + row) * L::SW + L::JCOFF;
      lds[row * ST + k] = src[k];
    }
    __syncthreads();
    if (t < CC + CD) {
      const int woff = HASINFO ? CR + RD : 0;  // weighted rows (== raw w/o)
      for (int e = 0; e < nt; ++e) {
        const T* row = lds + e * ST;
        if (t < CC) {
          T v = T(0);
          for (int i = 0; i < RD; ++i)
            v += row[ti * RD + i] * row[woff + tj * RD + i];
          acc += v;
        } else {
          T v = T(0);
          for (int i = 0; i < RD; ++i) v += row[ti * RD + i] * row[CR + i];
          acc -= v;
        }
      }
    }
    __syncthreads();
  }
  if (t < CC)
    atomicAdd(&Hpp[(int64_t)cam * CC + ti * CD + tj], acc);
  else if (t < CC + CD)
    atomicAdd(&g[(int64_t)cam * CD + ti], acc);
}

// MFMA experiment (reference anchor
// build_linear_system.cu:88-146): the per-chunk Hpp accumulation
// Hpp += Jc^T (W Jc) is a K-reduction GEMM with M=N=9, K=2*rows.  One
// v_mfma_f64_16x16x4_f64 per 4 K-rows computes the whole 16x16 tile
// (rows 9..15 zero-padded); the g_c = -Jc^T wr partial rides along as a
// free 10th B column.  Env-gated (MEGBA_MFMA=1), fp64 BAL dims only.
// Four interleaved accumulators break the dependent-MFMA latency chain.
typedef double megba_d4 __attribute__((ext_vector_type(4)));
template <typename T, int CD, int PD, int RD, bool HASINFO, bool EXPL>
__global__ __launch_bounds__(64) void kAssembleCamMfma(
    int nChunks, const int* __restrict__ chCam, const int* __restrict__ chLo,
    const int* __restrict__ chHi, const T* __restrict__ slab,
    T* __restrict__ Hpp, T* __restrict__ g) {
  static_assert(std::is_same<T, double>::value && CD == 9 && PD == 3 &&
                    RD == 2,
                "MFMA assembly path is fp64 BAL (9,3,2) only");
  using L = SlabLayout<CD, PD, RD, EXPL, HASINFO>;
  constexpr int CR = CD * RD;                       // 18
  constexpr int ST = CR + RD + (HASINFO ? CR : 0);  // jc + wr (+ wjc)
  constexpr int TE = 128;
  __shared__ T lds[TE * ST];
  const int chunk = blockIdx.x;
  if (chunk >= nChunks) return;
  const int cam = chCam[chunk];
  const int lo = chLo[chunk], hi = chHi[chunk];
  const int l = (int)threadIdx.x;
  const int i = l & 15;        // A row (camera col) / D col
  const int kq = l >> 4;       // K quarter within each MFMA's K=4
  constexpr int woff = HASINFO ? CR + RD : 0;
  megba_d4 acc[4];
  for (int a = 0; a < 4; ++a) acc[a] = megba_d4{0.0, 0.0, 0.0, 0.0};
  for (int s0 = lo; s0 < hi; s0 += TE) {
    const int nt = min(TE, hi - s0);
    for (int idx = l; idx < nt * ST; idx += 64) {
      const int row = idx / ST;
      const int k = idx % ST;
      lds[row * ST + k] = slab[(int64_t)(s0 + row) * L::SW + L::JCOFF + k];
    }
    __syncthreads();
    const int K = nt * RD;  // edge-rows in this tile
    for (int k0 = 0; k0 < K; k0 += 16) {
      // 4 MFMAs per iteration, one per accumulator -> 4-deep independence
      for (int a = 0; a < 4; ++a) {
        const int kr = k0 + 4 * a + kq;  // this lane's K index
        T av = T(0), bv = T(0);
        if (kr < K) {
          const int e = kr >> 1;        // RD == 2
          const int r = kr & 1;
          const T* row = lds + e * ST;
          if (i < 9) {
            av = row[i * 2 + r];          // Jc[k][i]
            bv = row[woff + i * 2 + r];   // (W Jc)[k][j=i]
          } else if (i == 9) {
            bv = row[CR + r];             // wr[k] -> g column
          }
        }
        acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[a], 0, 0,
                                                      0);
      }
    }
    __syncthreads();
  }
  for (int a = 1; a < 4; ++a) acc[0] += acc[a];
  // C/D map for v_mfma_f64_16x16x4_f64 (probed on hardware,
  // tools/mfma_probe.hip): col = lane&15, row = 4*reg + (lane>>4).
  for (int v = 0; v < 4; ++v) {
    const int row = v * 4 + kq;
    const int col = i;
    if (row < 9) {
      if (col < 9)
        atomicAdd(&Hpp[(int64_t)cam * 81 + row * 9 + col], acc[0][v]);
      else if (col == 9)
        atomicAdd(&g[(int64_t)cam * 9 + row], -acc[0][v]);
    }
  }
}

// Explicit only: stream the slab's Hpl blocks out as a cam-sorted grad-major
// copy for the E*w kernel (contiguous reads, coalesced writes).
template <typename T, int CD, int PD, int RD, bool HASINFO>
__global__ void kFinalizeCam(int64_t nL, const T* __restrict__ slab,
                             T* __restrict__ HplCam) {
  using L = SlabLayout<CD, PD, RD, true, HASINFO>;
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int NGH = PackedEdge<T, CD, PD, RD, false>::NG;
  TV* o = (TV*)HplCam;
  for (int64_t j = blockIdx.x * (int64_t)kBlk + threadIdx.x; j < nL;
       j += (int64_t)gridDim.x * kBlk) {
    const T* row = slab + j * L::SW;
    for (int g = 0; g < NGH; ++g) {
      TV v;
      for (int q = 0; q < VEC; ++q) {
        const int k = g * VEC + q;
        v[q] = k < CD * PD ? row[k] : T(0);
      }
      o[(int64_t)g * nL + j] = v;
    }
  }
}

// (The r01 grad-major implicit copies kFinalizeCamImp / kSpmvExImpG were
// replaced by the packed vector-group kernels below in r2 —
// profiles/r02_gather_bands.md.)

// Cam-sorted packed finalize: slab -> [wJc, Jp] vector groups.
template <typename T, int CD, int PD, int RD, bool HASINFO>
__global__ void kFinalizeCamImpPk(int64_t nL, const T* __restrict__ slab,
                                  T* __restrict__ JCamPk) {
  using L = SlabLayout<CD, PD, RD, false, HASINFO>;
  using TV = typename PackVec<T>::type;
  constexpr int VEC = PackVec<T>::VEC;
  constexpr int CR = CD * RD, PR = PD * RD;
  constexpr int NG = PackedEdge<T, CD, PD, RD, true>::NG;
  constexpr int woff = HASINFO ? L::WJCOFF : L::JCOFF;
  TV* o = (TV*)JCamPk;
  for (int64_t j = blockIdx.x * (int64_t)kBlk + threadIdx.x; j < nL;
       j += (int64_t)gridDim.x * kBlk) {
    const T* row = slab + j * L::SW;
    for (int g = 0; g < NG; ++g) {
      TV v;
      for (int q = 0; q < VEC; ++q) {
        const int k = g * VEC + q;
        v[q] = k < CR ? row[woff + k]
                      : (k < CR + PR ? row[L::JPOFF + (k - CR)] : T(0));
      }
      o[(int64_t)g * nL + j] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Damping, block inverse
// ---------------------------------------------------------------------------
template <typename T, int D>
__global__ void kDamp(int64_t nElem, const T* __restrict__ H, T* __restrict__ Hd,
                      T f, const unsigned char* __restrict__ fixed) {
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < nElem;
       i += (int64_t)gridDim.x * kBlk) {
    const int within = (int)(i % (D * D));
    const bool diag = within / D == within % D;
    if (fixed && fixed[i / (D * D)]) {
      // fixed vertex: identity block => deltaX = 0 for it (J columns are
      // already zeroed by the forward kernels)
      Hd[i] = diag ? T(1) : T(0);
      continue;
    }
    const T v = H[i];
    Hd[i] = diag ? v * f : v;
  }
}

template <typename T, int D>
__global__ void kInvert(int nBlk, const T* __restrict__ Hd, T* __restrict__ Hinv,
                        int* fail) {
  for (int64_t b = blockIdx.x * (int64_t)kBlk + threadIdx.x; b < nBlk;
       b += (int64_t)gridDim.x * kBlk) {
    if (!spdInvertPacked<T, D>(Hd + b * D * D, Hinv + b * D * D))
      atomicOr(fail, 1);  // rare: retried by kInvertJitter
  }
}

// Rare path: retry semi-definite blocks with a growing relative diagonal
// jitter (matches the CPU oracle); launched only if kInvert reported failure
// so its register/scratch cost stays off the hot path.
template <typename T, int D>
__global__ void kInvertJitter(int nBlk, const T* __restrict__ Hd,
                              T* __restrict__ Hinv, int* fail) {
  for (int64_t b = blockIdx.x * (int64_t)kBlk + threadIdx.x; b < nBlk;
       b += (int64_t)gridDim.x * kBlk) {
    const T* a = Hd + b * D * D;
    T* out = Hinv + b * D * D;
    if (spdInvertPacked<T, D>(a, out)) continue;
    T buf[D * D];
    T mx = T(0);
    for (int i = 0; i < D; ++i) {
      const T ad = (T)fabs((double)a[i * D + i]);
      mx = ad > mx ? ad : mx;
    }
    const T eps = (mx > T(0) ? mx : T(1)) * T(1e-10);
    bool ok = false;
    T jit = eps;
    for (int k = 0; k < 40 && !ok; ++k, jit *= T(10)) {
      for (int i = 0; i < D * D; ++i) buf[i] = a[i];
      for (int i = 0; i < D; ++i) buf[i * D + i] += jit;
      ok = spdInvertPacked<T, D>(buf, out);
    }
    if (!ok) atomicOr(fail + 1, 1);
  }
}

}  // namespace
}  // namespace megba
