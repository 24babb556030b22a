// Shared by every GPU header: error-check macros, the launch shape
// constants and the fixed-shape deterministic reductions.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <string>

#include "../common.hpp"

namespace megba {

#ifndef HIP_CHECK
#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    MEGBA_CHECK(_e == hipSuccess,                                           \
                std::string("HIP error: ") + hipGetErrorString(_e) + " @ " #expr); \
  } while (0)
#endif

#ifndef RCCL_CHECK
#define RCCL_CHECK(expr)                                                    \
  do {                                                                      \
    ncclResult_t _e = (expr);                                               \
    MEGBA_CHECK(_e == ncclSuccess,                                          \
                std::string("RCCL error: ") + ncclGetErrorString(_e) + " @ " #expr); \
  } while (0)
#endif

namespace {

constexpr int kBlk = 256;
constexpr int kRedBlocks = 256;  // fixed -> deterministic reductions

inline int gridFor(int64_t n) {
  int64_t g = (n + kBlk - 1) / kBlk;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ---------------------------------------------------------------------------
// Reductions
// ---------------------------------------------------------------------------
enum class ROp { Dot, SumSq, AbsMax };

// Block tree over one double per thread: max for AbsMax, sum otherwise.
// Every thread of a kBlk-wide block must call it and every thread gets the
// block's result.  The tree halves from kBlk / 2, which fixes the summation
// order.  It ends behind a barrier, so it can be called again right away.
template <ROp OP>
__device__ inline double blockReduce(double v) {
  __shared__ double sm[kBlk];
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = kBlk / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      if (OP == ROp::AbsMax)
        sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
      else
        sm[threadIdx.x] += sm[threadIdx.x + s];
    }
    __syncthreads();
  }
  const double total = sm[0];
  __syncthreads();
  return total;
}
__device__ inline double blockSum(double v) {
  return blockReduce<ROp::Dot>(v);
}

// Reduce a partial array (one value per block of an earlier kernel): thread t
// takes part[t], part[t + kBlk], ... in that order, then the block tree.
template <ROp OP>
__device__ inline double partialsReduce(const double* __restrict__ part,
                                        int nb) {
  double v = 0.0;
  for (int i = threadIdx.x; i < nb; i += kBlk) {
    if (OP == ROp::AbsMax)
      v = fmax(v, part[i]);
    else
      v += part[i];
  }
  return blockReduce<OP>(v);
}
__device__ inline double partialsSum(const double* __restrict__ part,
                                     int nb) {
  return partialsReduce<ROp::Dot>(part, nb);
}

// Tail of the kernels that sum one double per thread into a scalar: block
// tree, then one atomicAdd per block.
__device__ inline void blockSumAtomicAdd(double local, double* acc) {
  const double total = blockSum(local);
  if (threadIdx.x == 0) atomicAdd(acc, total);
}

// num / den, 0 where den is 0: the PCG scalars beta = rho / rhoPrev and
// alpha = rho / p.q.
__device__ inline double safeRatio(double num, double den) {
  return den != 0.0 ? num / den : 0.0;
}

template <typename T, ROp OP>
__global__ void kRedPartial(const T* a, const T* b, int64_t n, double* part) {
  double v = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlk) {
    const double x = (double)a[i];
    if (OP == ROp::Dot)
      v += x * (double)b[i];
    else if (OP == ROp::SumSq)
      v += x * x;
    else
      v = fmax(v, fabs(x));
  }
  const double total = blockReduce<OP>(v);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

template <ROp OP>
__global__ void kRedFinal(const double* part, int nb, double* out) {
  const double total = partialsReduce<OP>(part, nb);
  if (threadIdx.x == 0) *out = total;
}

}  // namespace
}  // namespace megba
