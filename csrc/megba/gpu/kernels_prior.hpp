// Gaussian unary priors on the GPU: one kernel per phase, a grid-stride loop
// over the per-entry function of ../prior.hpp (layout and kinds there).
//
// A prior touches only its own vertex's diagonal block and g slice, and there
// is at most one prior of a kind per vertex, so assembly needs no atomics;
// the two camera kinds run as consecutive kernels on the engine stream.  The
// scalar accumulations end like kForward (blockSumAtomicAdd).  `acc ==
// nullptr` (a rank that does not count a replicated kind) skips the
// accumulation but still writes r/J.
//
// The view's pointers arrive as separate __restrict__ kernel arguments (a
// struct member cannot carry the qualifier) and are bundled here.  Every
// launch is kBlk wide.
#pragma once

#include <hip/hip_runtime.h>

#include "../prior.hpp"
#include "gpu_common.hpp"

namespace megba {
namespace {

// r (and J) at the parameters x; sum r^T L r into acc.  The centre kind's
// Jet<T,6> Rodrigues chain wants more than the 128 VGPRs the default
// 1024-thread bound leaves (it spilled 52 B/lane in fp64).
template <typename T, typename Kind>
__global__ void __launch_bounds__(kBlk)
    kPriorForward(int64_t m, const int* __restrict__ idx,
                  const T* __restrict__ mean, const T* __restrict__ info,
                  T* __restrict__ r, T* __restrict__ J,
                  const T* __restrict__ x, double* acc) {
  const PriorView<T> p{m, idx, mean, info, r, J};
  double local = 0.0;
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * kBlk)
    local += (double)priorEvaluate<Kind>(p, k, x);
  if (acc) blockSumAtomicAdd(local, acc);
}

// H[v] += J^T L J, g[v] -= J^T L r.  PER_ROW: one thread per (row, prior),
// row-major over priors so lanes stay contiguous; otherwise one thread per
// prior.
template <typename T, typename Kind, bool PER_ROW>
__global__ void kPriorAssemble(int64_t m, const int* __restrict__ idx,
                               const T* __restrict__ info, T* __restrict__ r,
                               T* __restrict__ J,
                               const unsigned char* __restrict__ fixed,
                               T* __restrict__ H, T* __restrict__ g) {
  const PriorView<T> p{m, idx, nullptr, info, r, J};
  const int64_t n = PER_ROW ? m * Kind::ROWS : m;
  for (int64_t t = blockIdx.x * (int64_t)kBlk + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * kBlk) {
    const int64_t k = PER_ROW ? t % m : t;
    if (fixed && fixed[idx[k]]) continue;
    const int iLo = PER_ROW ? (int)(t / m) : 0;
    const int iHi = PER_ROW ? iLo + 1 : Kind::ROWS;
    for (int i = iLo; i < iHi; ++i) priorAssembleRow<Kind>(p, k, i, H, g);
  }
}

// sum (J dx + r)^T L (J dx + r) over the accepted r (and J) into acc.
template <typename T, typename Kind>
__global__ void kPriorRho(int64_t m, const int* __restrict__ idx,
                          const T* __restrict__ info, T* __restrict__ r,
                          T* __restrict__ J,
                          const unsigned char* __restrict__ fixed,
                          const T* __restrict__ dx, double* acc) {
  const PriorView<T> p{m, idx, nullptr, info, r, J};
  double local = 0.0;
  for (int64_t k = blockIdx.x * (int64_t)kBlk + threadIdx.x; k < m;
       k += (int64_t)gridDim.x * kBlk)
    local += (double)priorModel<Kind>(p, k, fixed && fixed[idx[k]], dx);
  if (acc) blockSumAtomicAdd(local, acc);
}

}  // namespace
}  // namespace megba
