// Dense fp64 Cholesky and triangular solves for gfx950 (dense_chol.hpp).
//
// Right-looking blocked factorization of the lower triangle with 64 x 64
// tiles, three kernels per panel k:
//   kFactorDiag    one workgroup, the diagonal tile resident in LDS: factors
//                  it, checks every pivot, inverts the factored tile
//   kPanel         A_ik := A_ik inv(L_kk)^T, one tile per workgroup
//   kTrailingMfma  A_ij -= L_ik L_jk^T for the tiles i >= j > k on
//                  v_mfma_f64_16x16x4_f64, operands staged through LDS
// The stored inverses of the diagonal tiles turn the panel solve and the
// substitution steps of solve() into products.
#include "dense_chol.hpp"

#include <cmath>

namespace megba {
namespace dense {
namespace {

constexpr int T = kTile;
constexpr int LD = T + 1;   // LDS row stride of a whole tile
constexpr int HK = 32;      // k-half staged at a time by the product kernels
constexpr int LH = HK + 1;  // its LDS row stride
constexpr int KMAX = kMaxRhs;  // most right-hand sides of solve()
constexpr int kThreads = 256;

typedef double d4 __attribute__((ext_vector_type(4)));

__global__ void kIdentityTail(double* __restrict__ A, int64_t np, int64_t n) {
  const int64_t i = n + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < np) A[i * np + i] = 1.0;
}

__global__ void kSaveDiag(const double* __restrict__ A, int64_t np,
                          double* __restrict__ diag0,
                          FactorWords* __restrict__ words) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < np) diag0[i] = A[i * np + i];
  if (i == 0) {
    words->failRow = -1;
    words->pad = 0;
    words->minRatio = 1.0;
    words->failRatio = 0.0;
  }
}

// Diagonal tile kb: L_kk in place (upper part zeroed) and inv(L_kk) into
// invDiag.  A pivot d fails when it is not finite, not positive or below
// pivotTol * diag0; the first failure is recorded and every later call
// returns at once, so the words hold the state at the first failing row.
__global__ __launch_bounds__(kThreads) void kFactorDiag(
    double* __restrict__ A, int64_t np, int kb,
    const double* __restrict__ diag0, double pivotTol,
    double* __restrict__ invDiag, FactorWords* __restrict__ words) {
  __shared__ double a[T * LD];
  __shared__ double ldiag[T];
  if (words->failRow >= 0) return;
  const int tid = (int)threadIdx.x;
  const int64_t k0 = (int64_t)kb * T;
  double* tile = A + k0 * np + k0;
  for (int idx = tid; idx < T * T; idx += kThreads) {
    const int i = idx / T, c = idx % T;
    a[i * LD + c] = c <= i ? tile[(int64_t)i * np + c] : 0.0;
  }
  double minR = 1.0;
  for (int j = 0; j < T; ++j) {
    __syncthreads();
    const double d = a[j * LD + j];
    const double s0 = diag0[k0 + j];
    const double ratio = d / s0;
    if (!(d > 0.0) || isinf(d) || d < pivotTol * s0) {
      if (tid == 0) {
        words->failRow = (int)(k0 + j);
        words->failRatio = ratio;
        words->minRatio = fmin(words->minRatio, minR);
      }
      return;
    }
    minR = fmin(minR, ratio);
    const double l = sqrt(d);
    __syncthreads();  // every thread has read the pivot
    if (tid == j) a[j * LD + j] = l;
    if (tid > j && tid < T) a[tid * LD + j] /= l;
    __syncthreads();
    for (int idx = tid; idx < T * T; idx += kThreads) {
      const int i = idx / T, c = idx % T;
      if (c > j && c <= i) a[i * LD + c] -= a[i * LD + j] * a[c * LD + j];
    }
  }
  __syncthreads();
  if (tid == 0) words->minRatio = fmin(words->minRatio, minR);
  if (tid < T) ldiag[tid] = a[tid * LD + tid];
  __syncthreads();
  // inv(L): thread c solves L x = e_c and keeps x_i, i > c, in the unused
  // upper triangle at a[c][i]; x_c replaces the diagonal at the end
  double xc = 0.0;
  if (tid < T) {
    const int c = tid;
    xc = 1.0 / ldiag[c];
    for (int i = c + 1; i < T; ++i) {
      double s = -a[i * LD + c] * xc;
      for (int t = c + 1; t < i; ++t) s -= a[i * LD + t] * a[c * LD + t];
      a[c * LD + i] = s / ldiag[i];
    }
  }
  __syncthreads();
  double* inv = invDiag + (int64_t)kb * T * T;
  for (int idx = tid; idx < T * T; idx += kThreads) {
    const int i = idx / T, c = idx % T;
    const double lv = c < i ? a[i * LD + c] : (c == i ? ldiag[i] : 0.0);
    const double iv = c < i ? a[c * LD + i] : (c == i ? 1.0 / ldiag[i] : 0.0);
    tile[(int64_t)i * np + c] = lv;
    inv[idx] = iv;
  }
}

// Stage the k-half [t0, t0 + HK) of a T-row tile (row stride ld) into LDS.
__device__ __forceinline__ void stageHalf(const double* __restrict__ src,
                                          int64_t ld, int t0,
                                          double* __restrict__ dst) {
  for (int idx = (int)threadIdx.x; idx < T * HK; idx += kThreads) {
    const int r = idx / HK, t = idx % HK;
    dst[r * LH + t] = src[(int64_t)r * ld + t0 + t];
  }
}

// Tile (kb + 1 + blockIdx.x, kb) := A_ik inv(L_kk)^T.  Thread (r, c0): row r,
// 16 columns from c0.
__global__ __launch_bounds__(kThreads) void kPanel(
    double* __restrict__ A, int64_t np, int kb,
    const double* __restrict__ invDiag) {
  __shared__ double As[T * LH];
  __shared__ double Is[T * LH];
  const int ti = kb + 1 + (int)blockIdx.x;
  double* tile = A + (int64_t)ti * T * np + (int64_t)kb * T;
  const double* inv = invDiag + (int64_t)kb * T * T;
  const int r = (int)threadIdx.x >> 2, c0 = ((int)threadIdx.x & 3) * 16;
  double acc[16];
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) acc[cc] = 0.0;
  for (int t0 = 0; t0 < T; t0 += HK) {
    stageHalf(tile, np, t0, As);
    stageHalf(inv, T, t0, Is);
    __syncthreads();
    for (int t = 0; t < HK; ++t) {
      const double av = As[r * LH + t];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) acc[cc] += av * Is[(c0 + cc) * LH + t];
    }
    __syncthreads();  // also: the tile is fully read before it is written
  }
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) tile[(int64_t)r * np + c0 + cc] = acc[cc];
}

// Tile (i, j) -= L_ik L_jk^T, i = kb + 1 + blockIdx.y >= j = kb + 1 +
// blockIdx.x.  Four waves; wave w owns rows [16 w, 16 w + 16) of the tile
// and keeps four independent 16 x 16 accumulators, one per column block.
// Lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] of a 16x16x4 step
// and holds D[(l >> 4) + 4 v][l & 15] in register v (tools/mfma_probe.hip).
__global__ __launch_bounds__(kThreads) void kTrailingMfma(
    double* __restrict__ A, int64_t np, int kb) {
  const int tj = kb + 1 + (int)blockIdx.x, ti = kb + 1 + (int)blockIdx.y;
  if (tj > ti) return;
  __shared__ double As[T * LH];
  __shared__ double Bs[T * LH];
  const double* La = A + (int64_t)ti * T * np + (int64_t)kb * T;
  const double* Lb = A + (int64_t)tj * T * np + (int64_t)kb * T;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
  d4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = d4{0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < T; t0 += HK) {
    stageHalf(La, np, t0, As);
    stageHalf(Lb, np, t0, Bs);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < HK; kk += 4) {
      const double av = As[(16 * wave + lr) * LH + kk + lk];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const double bv = Bs[(16 * nb + lr) * LH + kk + lk];
        acc[nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  double* C = A + (int64_t)ti * T * np + (int64_t)tj * T;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 16 * wave + lk + 4 * v, col = 16 * nb + lr;
      // a diagonal tile keeps its upper triangle untouched
      if (ti != tj || col <= row) C[(int64_t)row * np + col] -= acc[nb][v];
    }
}

// ---- substitution ----------------------------------------------------------
// Y[g][c] (np x k row-major) from the [cam][kb][cd] layout; zero past n.
__global__ void kGatherRhs(const double* __restrict__ R, int64_t np, int64_t n,
                           int cd, int kb, int k, double* __restrict__ Y) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       idx < np * k; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = idx / k;
    const int c = (int)(idx % k);
    Y[idx] = g < n ? R[((g / cd) * kb + c) * cd + g % cd] : 0.0;
  }
}

// The rows below n of Y into the [cam][kb][xStride] layout.
__global__ void kScatterX(const double* __restrict__ Y, int64_t n, int cd,
                          int kb, int k, int xStride, double* __restrict__ X) {
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       idx < n * k; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = idx / k;
    const int c = (int)(idx % k);
    X[((g / cd) * kb + c) * xStride + g % cd] = Y[idx];
  }
}

// One step of the forward (L y = b) or backward (L^T x = y) substitution at
// tile row kblk.  Every workgroup forms x_k = inv(L_kk) src_k (transposed
// for BWD) from the finished rows of src; workgroup 0 stores it to dst, the
// others subtract their tile's product with x_k from their own rows of src:
// row kblk + blockIdx.x forward, row kblk - blockIdx.x backward.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void kSubstStep(
    const double* __restrict__ L, const double* __restrict__ invDiag,
    int64_t np, int kblk, int k, double* __restrict__ src,
    double* __restrict__ dst) {
  __shared__ double Ls[T * LD];
  __shared__ double yk[T * KMAX];
  __shared__ double xk[T * KMAX];
  const int tid = (int)threadIdx.x;
  const double* inv = invDiag + (int64_t)kblk * T * T;
  for (int idx = tid; idx < T * T; idx += kThreads)
    Ls[(idx / T) * LD + idx % T] = inv[idx];
  for (int idx = tid; idx < T * k; idx += kThreads)
    yk[idx] = src[(int64_t)kblk * T * k + idx];
  __syncthreads();
  for (int idx = tid; idx < T * k; idx += kThreads) {
    const int r = idx % T, c = idx / T;
    double s = 0.0;
    for (int t = 0; t < T; ++t)
      s += (BWD ? Ls[t * LD + r] : Ls[r * LD + t]) * yk[t * k + c];
    xk[r * k + c] = s;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    for (int idx = tid; idx < T * k; idx += kThreads)
      dst[(int64_t)kblk * T * k + idx] = xk[idx];
    return;
  }
  const int i = BWD ? kblk - (int)blockIdx.x : kblk + (int)blockIdx.x;
  const double* tile = BWD ? L + (int64_t)kblk * T * np + (int64_t)i * T
                           : L + (int64_t)i * T * np + (int64_t)kblk * T;
  for (int idx = tid; idx < T * T; idx += kThreads)
    Ls[(idx / T) * LD + idx % T] = tile[(int64_t)(idx / T) * np + idx % T];
  __syncthreads();
  for (int idx = tid; idx < T * k; idx += kThreads) {
    const int r = idx % T, c = idx / T;
    double s = 0.0;
    for (int t = 0; t < T; ++t)
      s += (BWD ? Ls[t * LD + r] : Ls[r * LD + t]) * xk[t * k + c];
    src[((int64_t)i * T + r) * k + c] -= s;
  }
}

inline int gridOf(int64_t n) {
  const int64_t g = (n + kThreads - 1) / kThreads;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

void identityTail(double* A, int64_t np, int64_t n, hipStream_t s) {
  if (np > n)
    hipLaunchKernelGGL(kIdentityTail, dim3(gridOf(np - n)), dim3(kThreads), 0,
                       s, A, np, n);
}

void factor(double* A, int64_t np, double* invDiag, double* diag0,
            double pivotTol, FactorWords* words, hipStream_t s,
            float* phaseMs) {
  const int nb = (int)(np / T);
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (phaseMs) {
    (void)hipEventCreate(&ev[0]);
    (void)hipEventCreate(&ev[1]);
  }
  // launch() between two events when the phases are timed
  const auto timed = [&](int phase, auto&& launch) {
    if (!phaseMs) {
      launch();
      return;
    }
    (void)hipEventRecord(ev[0], s);
    launch();
    (void)hipEventRecord(ev[1], s);
    (void)hipEventSynchronize(ev[1]);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
    phaseMs[phase] += ms;
  };
  hipLaunchKernelGGL(kSaveDiag, dim3((unsigned)((np + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, A, np, diag0, words);
  for (int kb = 0; kb < nb; ++kb) {
    timed(0, [&] {
      hipLaunchKernelGGL(kFactorDiag, dim3(1), dim3(kThreads), 0, s, A, np, kb,
                         diag0, pivotTol, invDiag, words);
    });
    const int m = nb - kb - 1;
    if (m == 0) break;
    timed(1, [&] {
      hipLaunchKernelGGL(kPanel, dim3(m), dim3(kThreads), 0, s, A, np, kb,
                         invDiag);
    });
    timed(2, [&] {
      hipLaunchKernelGGL(kTrailingMfma, dim3(m, m), dim3(kThreads), 0, s, A,
                         np, kb);
    });
  }
  if (phaseMs) {
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
  }
}

void solve(const double* L, const double* invDiag, int64_t np, int64_t n,
           const double* R, double* X, double* work, int cd, int kb, int k,
           int xStride, hipStream_t s) {
  const int nb = (int)(np / T);
  if (k < 1 || k > kMaxRhs) return;  // kSubstStep's LDS holds kMaxRhs columns
  double* y = work;           // right-hand sides, then the solution
  double* z = work + np * k;  // the forward solution
  hipLaunchKernelGGL(kGatherRhs, dim3(gridOf(np * k)), dim3(kThreads), 0, s, R,
                     np, n, cd, kb, k, y);
  for (int kblk = 0; kblk < nb; ++kblk)
    hipLaunchKernelGGL(kSubstStep<false>, dim3(nb - kblk), dim3(kThreads), 0,
                       s, L, invDiag, np, kblk, k, y, z);
  for (int kblk = nb - 1; kblk >= 0; --kblk)
    hipLaunchKernelGGL(kSubstStep<true>, dim3(kblk + 1), dim3(kThreads), 0, s,
                       L, invDiag, np, kblk, k, z, y);
  hipLaunchKernelGGL(kScatterX, dim3(gridOf(n * k)), dim3(kThreads), 0, s, y,
                     n, cd, kb, k, xStride, X);
}

}  // namespace dense
}  // namespace megba
