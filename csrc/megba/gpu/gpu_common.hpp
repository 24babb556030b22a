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
// Tail of the kernels that sum one double per thread into a scalar: block
// tree, then one atomicAdd per block.  Every thread of a kBlk-wide block must
// call it.
__device__ inline void blockSumAtomicAdd(double local, double* acc) {
  __shared__ double sm[kBlk];
  sm[threadIdx.x] = local;
  __syncthreads();
  for (int s = kBlk / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(acc, sm[0]);
}

enum class ROp { Dot, SumSq, AbsMax };

template <typename T, ROp OP>
__global__ void kRedPartial(const T* a, const T* b, int64_t n, double* part) {
  __shared__ double sm[kBlk];
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
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

template <ROp OP>
__global__ void kRedFinal(const double* part, int nb, double* out) {
  __shared__ double sm[kBlk];
  double v = 0.0;
  for (int i = threadIdx.x; i < nb; i += kBlk) {
    if (OP == ROp::AbsMax)
      v = fmax(v, part[i]);
    else
      v += part[i];
  }
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
  if (threadIdx.x == 0) *out = sm[0];
}

}  // namespace
}  // namespace megba
