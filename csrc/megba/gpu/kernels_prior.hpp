// Gaussian unary priors on the GPU (math in ../prior.hpp).
//
// State is component-major for every kind: idx[m], mean[D][m],
// info[D(D+1)/2][m], r[2][D][m] and, for the centre kind, J[2][18][m], so a
// wave's loads and stores of one component are contiguous.  A prior touches
// only its own vertex's diagonal block and g slice, and there is at most one
// prior of a kind per vertex, so assembly needs no atomics; the two camera
// kinds run as consecutive kernels on the engine stream.  The scalar
// accumulations follow kForward: block tree, one double atomicAdd per block.
// `acc == nullptr` (a rank that does not count a replicated kind) skips the
// accumulation but still writes r/J.
#pragma once

#include <hip/hip_runtime.h>

#include "../prior.hpp"
#include "gpu_common.hpp"

namespace megba {
namespace {

// Every thread of the block must call this (acc is block-uniform).
__device__ inline void priorBlockAdd(double local, double* acc) {
  __shared__ double sm[kBlk];
  if (acc == nullptr) return;
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int s = kBlk / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(acc, sm[0]);
}

// v^T L v with entry k's packed information read component by component.
template <typename T, int D>
__device__ inline T priorQuad(const T* __restrict__ info, int64_t m, int64_t k,
                              const T* v) {
  T q = T(0);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    T s = T(0);
#pragma unroll
    for (int j = 0; j < D; ++j) s += info[packedIdx<D>(i, j) * m + k] * v[j];
    q += v[i] * s;
  }
  return q;
}

// Parameter priors (camera block or point): r = x[idx] - mean.
template <typename T, int D>
__global__ void kPriorParamForward(int64_t m, const int* __restrict__ idx,
                                   const T* __restrict__ x,
                                   const T* __restrict__ mean,
                                   const T* __restrict__ info,
                                   T* __restrict__ r, double* acc) {
  double local = 0.0;
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * kBlk) {
    const T* xv = x + (int64_t)idx[k] * D;
    T v[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      v[i] = xv[i] - mean[i * m + k];
      r[i * m + k] = v[i];
    }
    local += (double)priorQuad<T, D>(info, m, k, v);
  }
  priorBlockAdd(local, acc);
}

// Centre prior: r = C(cam) - centre and the 3x6 J by jets (cameraCentre).
// The Jet<T,6> Rodrigues chain wants more than the 128 VGPRs the default
// 1024-thread bound leaves (it spilled 52 B/lane in fp64); the launch is
// always kBlk wide.
template <typename T, int CD>
__global__ void __launch_bounds__(kBlk) kPriorCentreForward(int64_t m, const int* __restrict__ idx,
                                    const T* __restrict__ cams,
                                    const T* __restrict__ centre,
                                    const T* __restrict__ info,
                                    T* __restrict__ r, T* __restrict__ J,
                                    double* acc) {
  double local = 0.0;
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * kBlk) {
    const T* cp = cams + (int64_t)idx[k] * CD;
    T cam[6], C[3], Jl[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) cam[i] = cp[i];
    cameraCentre<T>(cam, C, Jl);
    T v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[a] = C[a] - centre[a * m + k];
      r[a * m + k] = v[a];
    }
#pragma unroll
    for (int q = 0; q < 18; ++q) J[q * m + k] = Jl[q];
    local += (double)priorQuad<T, 3>(info, m, k, v);
  }
  priorBlockAdd(local, acc);
}

// H[v] += L, g[v] -= L r for the parameter priors (J = I).  PER_ROW: one
// thread per (row, prior), row-major over priors so lanes stay contiguous;
// otherwise one thread per prior.
template <typename T, int D, bool PER_ROW>
__global__ void kPriorParamAssemble(int64_t m, const int* __restrict__ idx,
                                    const T* __restrict__ info,
                                    const T* __restrict__ r,
                                    const unsigned char* __restrict__ fixed,
                                    T* __restrict__ H, T* __restrict__ g) {
  const int64_t n = PER_ROW ? m * D : m;
  for (int64_t t = blockIdx.x * (int64_t)kBlk + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * kBlk) {
    const int64_t k = PER_ROW ? t % m : t;
    const int v = idx[k];
    if (fixed && fixed[v]) continue;
    const int iLo = PER_ROW ? (int)(t / m) : 0;
    const int iHi = PER_ROW ? iLo + 1 : D;
    for (int i = iLo; i < iHi; ++i) {
      T* hRow = H + (int64_t)v * D * D + i * D;
      T lr = T(0);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const T l = info[packedIdx<D>(i, j) * m + k];
        hRow[j] += l;
        lr += l * r[j * m + k];
      }
      g[(int64_t)v * D + i] -= lr;
    }
  }
}

// Hpp[c] += J^T L J on the leading 6x6, g[c] -= J^T L r: one thread per
// (row i < 6, prior).
template <typename T, int CD>
__global__ void kPriorCentreAssemble(int64_t m, const int* __restrict__ idx,
                                     const T* __restrict__ info,
                                     const T* __restrict__ r,
                                     const T* __restrict__ J,
                                     const unsigned char* __restrict__ fixed,
                                     T* __restrict__ Hpp, T* __restrict__ g) {
  for (int64_t t = blockIdx.x * (int64_t)kBlk + threadIdx.x; t < m * 6;
       t += (int64_t)gridDim.x * kBlk) {
    const int64_t k = t % m;
    const int i = (int)(t / m);
    const int c = idx[k];
    if (fixed && fixed[c]) continue;
    // u = L J[:, i]
    T col[3], u[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) col[a] = J[(a * 6 + i) * m + k];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      u[b] = T(0);
#pragma unroll
      for (int a = 0; a < 3; ++a) u[b] += info[packedIdx<3>(b, a) * m + k] * col[a];
    }
    T* hRow = Hpp + (int64_t)c * CD * CD + i * CD;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      T s = T(0);
#pragma unroll
      for (int b = 0; b < 3; ++b) s += u[b] * J[(b * 6 + j) * m + k];
      hRow[j] += s;
    }
    T gs = T(0);
#pragma unroll
    for (int b = 0; b < 3; ++b) gs += u[b] * r[b * m + k];
    g[(int64_t)c * CD + i] -= gs;
  }
}

// sum (dx[idx] + r)^T L (dx[idx] + r) over the accepted r; a fixed vertex
// does not move, so its term stays r^T L r.
template <typename T, int D>
__global__ void kPriorParamRho(int64_t m, const int* __restrict__ idx,
                               const T* __restrict__ info,
                               const T* __restrict__ r,
                               const unsigned char* __restrict__ fixed,
                               const T* __restrict__ dx, double* acc) {
  double local = 0.0;
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * kBlk) {
    const int v = idx[k];
    const bool fix = fixed && fixed[v];
    T a[D];
#pragma unroll
    for (int i = 0; i < D; ++i)
      a[i] = r[i * m + k] + (fix ? T(0) : dx[(int64_t)v * D + i]);
    local += (double)priorQuad<T, D>(info, m, k, a);
  }
  priorBlockAdd(local, acc);
}

// sum (J dx[c] + r)^T L (J dx[c] + r) with the accepted r and J.
template <typename T, int CD>
__global__ void kPriorCentreRho(int64_t m, const int* __restrict__ idx,
                                const T* __restrict__ info,
                                const T* __restrict__ r,
                                const T* __restrict__ J,
                                const unsigned char* __restrict__ fixed,
                                const T* __restrict__ dx, double* acc) {
  double local = 0.0;
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * kBlk) {
    const int c = idx[k];
    const bool fix = fixed && fixed[c];
    T a[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      a[b] = r[b * m + k];
      if (!fix) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
          a[b] += J[(b * 6 + i) * m + k] * dx[(int64_t)c * CD + i];
      }
    }
    local += (double)priorQuad<T, 3>(info, m, k, a);
  }
  priorBlockAdd(local, acc);
}

}  // namespace
}  // namespace megba
