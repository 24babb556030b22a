// Forming the dense Schur complement S = HppD - E Cinv E^T on the GPU
// (Engine::denseSchurFactor; the factorization itself is dense_chol.hip).
//
// Two kernels.  kDenseEdgeBlocks writes, per edge, the CD x PD block
// W = Jc^T L Jp the batched E products apply (from the cam-sorted packed
// groups: [wJc, Jp] in implicit mode, Hpl in explicit mode) in primary order
// and Y = W Cinv in cam-sorted order.  kDenseSchurForm then gives camera j's
// column block to one workgroup: it walks camera j's cam-sorted edges, for
// each of them the run of its point, and sums -W_i Y_j^T for the cameras
// i >= j of a row tile in LDS, so every S block is written to memory once,
// with plain stores.  On one rank S is bitwise reproducible from run to run.
#pragma once

#include "edge_ops.hpp"
#include "gpu_common.hpp"

namespace megba {
namespace {

// Most cameras of a row tile: CD * CD doubles each in static LDS.
template <int CD>
constexpr int kDenseTileCams = (60 * 1024) / (CD * CD * 8);

template <typename T, int CD, int PD, int RD, bool IMP>
__global__ void kDenseEdgeBlocks(int64_t nL, const int* __restrict__ camPos,
                                 const int* __restrict__ ptOf,
                                 const T* __restrict__ camPk,
                                 const T* __restrict__ HllInv,
                                 double* __restrict__ Wp,
                                 double* __restrict__ Yc) {
  using PE = PackedEdge<T, CD, PD, RD, IMP>;
  using TV = typename PackVec<T>::type;
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    const int64_t pos = camPos[e];
    TV buf[PE::NG];
    loadGroups<T>(camPk, nL, pos, buf);
    const T* inv = HllInv + (int64_t)ptOf[e] * PD * PD;
    double* w = Wp + e * (CD * PD);
    double* y = Yc + pos * (CD * PD);
#pragma unroll
    for (int i = 0; i < CD; ++i) {
      T row[PD];
#pragma unroll
      for (int q = 0; q < PD; ++q) {
        if constexpr (IMP) {
          T v = T(0);
#pragma unroll
          for (int rr = 0; rr < RD; ++rr)
            v += pkJc<T, RD>(buf, i, rr) * pkJp<T, CD, RD>(buf, q, rr);
          row[q] = v;
        } else {
          row[q] = pkHpl<T, PD>(buf, i, q);
        }
        w[i * PD + q] = (double)row[q];
      }
#pragma unroll
      for (int q = 0; q < PD; ++q) {
        T v = T(0);
#pragma unroll
        for (int t = 0; t < PD; ++t) v += row[t] * inv[t * PD + q];
        y[i * PD + q] = (double)v;
      }
    }
  }
}

// Column block of camera j = blockIdx.x.  camRow: cam-sorted row range of
// every camera; ptRow: primary edge range of every local point (relative to
// the shard's first edge); S has leading dimension ld and is written at the
// blocks (i, j), i >= j, only.  tileCams <= kDenseTileCams<CD>.
//
// Every wave walks all edges of camera j, 64 at a time for the index loads,
// and within a point's run takes the cameras i of the tile with
// (i - base) % waves == its own number; its lanes then own the CD * CD
// entries of that block.  One wave alone adds to an accumulator, in edge
// order: no atomics, and the same sums in the same order in every run.
template <int CD, int PD>
__global__ __launch_bounds__(kBlk) void kDenseSchurForm(
    int ncam, int tileCams, const int* __restrict__ camRow,
    const int* __restrict__ ptOfCam, const int64_t* __restrict__ ptRow,
    int ptLo, const int* __restrict__ camOf, const double* __restrict__ Wp,
    const double* __restrict__ Yc, double* __restrict__ S, int64_t ld) {
  constexpr int CC = CD * CD, CP = CD * PD;
  __shared__ double acc[kDenseTileCams<CD> * CC];
  const int j = (int)blockIdx.x;
  const int lo = camRow[j], hi = camRow[j + 1];
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, nWaves = kBlk >> 6;
  for (int base = j; base < ncam; base += tileCams) {
    const int top = base + tileCams < ncam ? base + tileCams : ncam;
    for (int idx = tid; idx < (top - base) * CC; idx += kBlk) acc[idx] = 0.0;
    __syncthreads();
    for (int pos0 = lo; pos0 < hi; pos0 += 64) {
      long long myR0 = 0, myR1 = 0;
      if (pos0 + lane < hi) {
        const int p = ptOfCam[pos0 + lane] - ptLo;
        myR0 = ptRow[p];
        myR1 = ptRow[p + 1];
      }
      const int cnt = hi - pos0 < 64 ? hi - pos0 : 64;
      for (int t = 0; t < cnt; ++t) {
        const long long r0 = __shfl(myR0, t, 64), r1 = __shfl(myR1, t, 64);
        const double* y = Yc + (int64_t)(pos0 + t) * CP;
        for (long long c0 = r0; c0 < r1; c0 += 64) {
          const int cam = c0 + lane < r1 ? camOf[c0 + lane] : -1;
          unsigned long long mine = __ballot(
              cam >= base && cam < top && (cam - base) % nWaves == wave);
          while (mine) {
            const int b = __ffsll((long long)mine) - 1;
            mine &= mine - 1;
            const int i = __shfl(cam, b, 64);
            const double* w = Wp + (c0 + b) * CP;
            for (int rc = lane; rc < CC; rc += 64) {
              const double* wr = w + (rc / CD) * PD;
              const double* yc = y + (rc % CD) * PD;
              double v = 0.0;
#pragma unroll
              for (int q = 0; q < PD; ++q) v += wr[q] * yc[q];
              acc[(i - base) * CC + rc] -= v;
            }
          }
        }
      }
    }
    __syncthreads();
    for (int idx = tid; idx < (top - base) * CC; idx += kBlk) {
      const int i = base + idx / CC, rc = idx % CC;
      S[((int64_t)i * CD + rc / CD) * ld + (int64_t)j * CD + rc % CD] =
          acc[idx];
    }
    __syncthreads();
  }
}

// S_cc += HppD_c for every camera: the replicated blocks go in once, after
// the partial sums of the ranks are added up.
template <typename T, int CD>
__global__ void kDenseAddDiag(int ncam, const T* __restrict__ HppD,
                              double* __restrict__ S, int64_t ld) {
  for (int64_t idx = blockIdx.x * (int64_t)kBlk + threadIdx.x;
       idx < (int64_t)ncam * CD * CD; idx += (int64_t)gridDim.x * kBlk) {
    const int64_t c = idx / (CD * CD);
    const int rc = (int)(idx % (CD * CD));
    S[(c * CD + rc / CD) * ld + c * CD + rc % CD] += (double)HppD[idx];
  }
}

}  // namespace
}  // namespace megba
