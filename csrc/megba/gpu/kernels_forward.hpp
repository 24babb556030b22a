// Forward kernels: the fused register-autodiff residual + Jacobian pass, its
// value-share and analytical variants, and the custom-edge gather / repack.
#pragma once

#include "../analytical.hpp"
#include "../bal_functor.hpp"
#include "gpu_common.hpp"

namespace megba {
namespace {

// ---------------------------------------------------------------------------
// Forward (fused register autodiff)
// ---------------------------------------------------------------------------
// Generic fused-autodiff forward: each observation is handled by
// LANES = ceil((CD+PD)/3) consecutive work items, each carrying a Jet<T,3>
// slice of the CD+PD-wide dual part.
template <typename T, int CD, int PD, int RD>
__global__ __launch_bounds__(256, 2) void kForward(
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ params, int ncam, const T* __restrict__ meas,
    const unsigned char* __restrict__ camFixed,
    const unsigned char* __restrict__ ptFixed, T* __restrict__ rOut,
    T* __restrict__ Jc, T* __restrict__ Jp, double* chi2Acc, int lossKind,
    T lossD2, const T* __restrict__ intr3) {
  using J3 = Jet<T, 3>;
  constexpr int GW = CD + PD;
  constexpr int LANES = (GW + 2) / 3;
  double chi2 = 0.0;
  const T* ptsBase = params + (int64_t)ncam * CD;
  const int64_t nWork = nL * LANES;
  T intr[3] = {intr3[0], intr3[1], intr3[2]};
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < nWork;
       i += (int64_t)gridDim.x * kBlk) {
    const int64_t e = i / LANES;
    const int sub = (int)(i % LANES);   // this lane's 3-wide gradient slice
    const int base = 3 * sub;           // gradient columns [base,base+3)
    const T* cp = params + (int64_t)camOf[e] * CD;
    const T* pp = ptsBase + (int64_t)ptOf[e] * PD;
    J3 cam[CD], pt[PD], res[RD];
    for (int k = 0; k < CD; ++k) cam[k] = J3::leaf(cp[k], k - base);
    for (int k = 0; k < PD; ++k) pt[k] = J3::leaf(pp[k], CD + k - base);
    T m[RD];
    for (int k = 0; k < RD; ++k) m[k] = meas[RD * e + k];
    builtinResidual<T, J3, CD, PD, RD>(cam, pt, m, intr, res);
    const bool cfix = camFixed && camFixed[camOf[e]];
    const bool pfix = ptFixed && ptFixed[ptOf[e]];
    for (int row = 0; row < RD; ++row) {
      for (int j = 0; j < 3; ++j) {
        const int col = base + j;
        if (col >= GW) break;
        if (col < CD)
          Jc[((int64_t)(col * RD + row)) * nL + e] =
              cfix ? T(0) : res[row].d[j];
        else
          Jp[((int64_t)((col - CD) * RD + row)) * nL + e] =
              pfix ? T(0) : res[row].d[j];
      }
      if (sub == 0) rOut[(int64_t)row * nL + e] = res[row].v;
    }
    if (sub == 0) {
      double ss = 0.0;
      for (int row = 0; row < RD; ++row)
        ss += (double)res[row].v * (double)res[row].v;
      chi2 += (double)lossRho(lossKind, lossD2, (T)ss);
    }
  }
  blockSumAtomicAdd(chi2, chi2Acc);
}

// Value-share forward experiment (env MEGBA_FWD_VS=1,
// BAL (9,3,2) only): the 4 gradient lanes of an edge recompute the whole
// VALUE chain of the reprojection; the dual math needs every intermediate
// value on every lane, so only the EXPENSIVE scalar values (sqrt, sincos,
// two reciprocals — the transcendental tail of the chain) are computed
// once on the edge's leader lane and broadcast with __shfl; their jets
// are then assembled from the analytic derivative rules.  Cheap mul/add
// values stay redundantly computed (a shuffle costs as much as an FMA).
template <typename T>
__global__ __launch_bounds__(256, 2) void kForwardVS(
    int64_t nL, const int* __restrict__ camOf, const int* __restrict__ ptOf,
    const T* __restrict__ params, int ncam, const T* __restrict__ meas,
    const unsigned char* __restrict__ camFixed,
    const unsigned char* __restrict__ ptFixed, T* __restrict__ rOut,
    T* __restrict__ Jc, T* __restrict__ Jp, double* chi2Acc, int lossKind,
    T lossD2) {
  using J3 = Jet<T, 3>;
  double chi2 = 0.0;
  const T* ptsBase = params + (int64_t)ncam * 9;
  const int64_t nWork = nL * 4;
  const int lane = (int)threadIdx.x & 63;
  const int leader = lane & ~3;
  for (int64_t i = blockIdx.x * (int64_t)kBlk + threadIdx.x; i < nWork;
       i += (int64_t)gridDim.x * kBlk) {
    const int64_t e = i >> 2;
    const int sub = (int)(i & 3);
    const int base = 3 * sub;
    const T* cp = params + (int64_t)camOf[e] * 9;
    const T* pp = ptsBase + (int64_t)ptOf[e] * 3;
    J3 cam[9], pt[3], res[2];
    for (int k = 0; k < 9; ++k) cam[k] = J3::leaf(cp[k], k - base);
    for (int k = 0; k < 3; ++k) pt[k] = J3::leaf(pp[k], 9 + k - base);
    const T m[2] = {meas[2 * e], meas[2 * e + 1]};
    // ---- Rodrigues with shared transcendental values ----
    const J3 theta2 =
        cam[0] * cam[0] + cam[1] * cam[1] + cam[2] * cam[2];
    J3 P[3];
    if (theta2.v > T(1e-14)) {  // edge-uniform branch
      T thv = T(0), stv = T(0), ctv = T(0), thInvV = T(0);
      if (sub == 0) {
        thv = ::sqrt(theta2.v);
        stv = ::sin(thv);
        ctv = ::cos(thv);
        thInvV = T(1) / thv;
      }
      stv = __shfl(stv, leader, 64);
      ctv = __shfl(ctv, leader, 64);
      thInvV = __shfl(thInvV, leader, 64);
      // jets from the analytic rules: d(sqrt) = d(theta2)/(2 theta) etc.
      J3 theta, sinth, costh, thetaInv;
      theta.v = thv == T(0) ? (thv = T(1) / thInvV) : thv;  // non-leader thv
      const T half = T(0.5) * thInvV;
      for (int k = 0; k < 3; ++k) theta.d[k] = theta2.d[k] * half;
      sinth.v = stv;
      costh.v = ctv;
      thetaInv.v = thInvV;
      const T mInv2 = -thInvV * thInvV;
      for (int k = 0; k < 3; ++k) {
        sinth.d[k] = ctv * theta.d[k];
        costh.d[k] = -stv * theta.d[k];
        thetaInv.d[k] = mInv2 * theta.d[k];
      }
      const J3 w0 = cam[0] * thetaInv;
      const J3 w1 = cam[1] * thetaInv;
      const J3 w2 = cam[2] * thetaInv;
      const J3 wxp0 = w1 * pt[2] - w2 * pt[1];
      const J3 wxp1 = w2 * pt[0] - w0 * pt[2];
      const J3 wxp2 = w0 * pt[1] - w1 * pt[0];
      const J3 wdp =
          (w0 * pt[0] + w1 * pt[1] + w2 * pt[2]) * (T(1) - costh);
      P[0] = pt[0] * costh + wxp0 * sinth + w0 * wdp;
      P[1] = pt[1] * costh + wxp1 * sinth + w1 * wdp;
      P[2] = pt[2] * costh + wxp2 * sinth + w2 * wdp;
    } else {
      P[0] = pt[0] + (cam[1] * pt[2] - cam[2] * pt[1]);
      P[1] = pt[1] + (cam[2] * pt[0] - cam[0] * pt[2]);
      P[2] = pt[2] + (cam[0] * pt[1] - cam[1] * pt[0]);
    }
    P[0] += cam[3];
    P[1] += cam[4];
    P[2] += cam[5];
    // shared reciprocal of the depth
    T invNegZv = T(0);
    if (sub == 0) invNegZv = T(-1) / P[2].v;
    invNegZv = __shfl(invNegZv, leader, 64);
    J3 invNegZ;
    invNegZ.v = invNegZv;
    const T q = invNegZv * invNegZv;  // d(-1/z) = z' / z^2
    for (int k = 0; k < 3; ++k) invNegZ.d[k] = q * P[2].d[k];
    const J3 xp = P[0] * invNegZ;
    const J3 yp = P[1] * invNegZ;
    const J3 r2 = xp * xp + yp * yp;
    const J3 distortion = T(1) + r2 * (cam[7] + cam[8] * r2);
    const J3 scaled = cam[6] * distortion;
    res[0] = scaled * xp - m[0];
    res[1] = scaled * yp - m[1];
    // ---- identical epilogue to kForward ----
    const bool cfix = camFixed && camFixed[camOf[e]];
    const bool pfix = ptFixed && ptFixed[ptOf[e]];
    for (int row = 0; row < 2; ++row) {
      for (int j = 0; j < 3; ++j) {
        const int col = base + j;
        if (col < 9)
          Jc[((int64_t)(col * 2 + row)) * nL + e] =
              cfix ? T(0) : res[row].d[j];
        else
          Jp[((int64_t)((col - 9) * 2 + row)) * nL + e] =
              pfix ? T(0) : res[row].d[j];
      }
      if (sub == 0) rOut[(int64_t)row * nL + e] = res[row].v;
    }
    if (sub == 0)
      chi2 += (double)lossRho(lossKind, lossD2,
                              res[0].v * res[0].v + res[1].v * res[1].v);
  }
  blockSumAtomicAdd(chi2, chi2Acc);
}

// Analytical-derivative forward: one thread per edge, closed-form residual +
// 2x12 Jacobian (reference C11, src/geo/analytical_derivatives.cu).
// BAL (9,3,2) only; the engine refuses analytical mode for other dims.
template <typename T>
__global__ void kForwardAnalytical(int64_t nL, const int* __restrict__ camOf,
                                   const int* __restrict__ ptOf,
                                   const T* __restrict__ params, int ncam,
                                   const T* __restrict__ meas,
                                   const unsigned char* __restrict__ camFixed,
                                   const unsigned char* __restrict__ ptFixed,
                                   T* __restrict__ rOut, T* __restrict__ Jc,
                                   T* __restrict__ Jp, double* chi2Acc,
                                   int lossKind, T lossD2) {
  double chi2 = 0.0;
  const T* ptsBase = params + (int64_t)ncam * 9;
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    const T* cp = params + (int64_t)camOf[e] * 9;
    const T* pp = ptsBase + (int64_t)ptOf[e] * 3;
    const T m[2] = {meas[2 * e], meas[2 * e + 1]};
    T res[2], jc[2][9], jp[2][3];
    balAnalytical<T>(cp, pp, m, res, jc, jp);
    chi2 += (double)lossRho(lossKind, lossD2,
                            res[0] * res[0] + res[1] * res[1]);
    const bool cfix = camFixed && camFixed[camOf[e]];
    const bool pfix = ptFixed && ptFixed[ptOf[e]];
    for (int row = 0; row < 2; ++row) {
      rOut[(int64_t)row * nL + e] = res[row];
      for (int col = 0; col < 9; ++col)
        Jc[((int64_t)(col * 2 + row)) * nL + e] = cfix ? T(0) : jc[row][col];
      for (int col = 0; col < 3; ++col)
        Jp[((int64_t)(col * 2 + row)) * nL + e] = pfix ? T(0) : jp[row][col];
    }
  }
  blockSumAtomicAdd(chi2, chi2Acc);
}

// chi2 with a robust loss, from the residual buffers (custom-edge path).
template <typename T, int RD>
__global__ void kChi2Loss(int64_t nL, const T* __restrict__ r, int lossKind,
                          T lossD2, double* acc) {
  double local = 0.0;
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    T ss = T(0);
    for (int row = 0; row < RD; ++row) {
      const T rv = r[(int64_t)row * nL + e];
      ss += rv * rv;
    }
    local += (double)lossRho(lossKind, lossD2, ss);
  }
  blockSumAtomicAdd(local, acc);
}

// Custom-edge support: gather parameter leaves, repack residual JetVectors.
template <typename T, int CD, int PD>
__global__ void kGatherLeaves(int64_t nL, const int* __restrict__ camOf,
                              const int* __restrict__ ptOf,
                              const T* __restrict__ params, int ncam,
                              T* __restrict__ leaf /*[CD+PD][nL]*/) {
  const T* ptsBase = params + (int64_t)ncam * CD;
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    const T* cp = params + (int64_t)camOf[e] * CD;
    const T* pp = ptsBase + (int64_t)ptOf[e] * PD;
    for (int k = 0; k < CD; ++k) leaf[(int64_t)k * nL + e] = cp[k];
    for (int k = 0; k < PD; ++k) leaf[(int64_t)(CD + k) * nL + e] = pp[k];
  }
}

template <typename T, int CD, int PD, int RD>
__global__ void kRepackRes(int64_t nL, int row, const T* __restrict__ rv,
                           const T* __restrict__ rg /*[CD+PD][nL]*/,
                           const int* __restrict__ camOf,
                           const int* __restrict__ ptOf,
                           const unsigned char* __restrict__ camFixed,
                           const unsigned char* __restrict__ ptFixed,
                           T* __restrict__ rOut, T* __restrict__ Jc,
                           T* __restrict__ Jp) {
  for (int64_t e = blockIdx.x * (int64_t)kBlk + threadIdx.x; e < nL;
       e += (int64_t)gridDim.x * kBlk) {
    rOut[(int64_t)row * nL + e] = rv[e];
    const bool cfix = camFixed && camFixed[camOf[e]];
    const bool pfix = ptFixed && ptFixed[ptOf[e]];
    for (int k = 0; k < CD; ++k)
      Jc[((int64_t)(k * RD + row)) * nL + e] =
          cfix ? T(0) : rg[(int64_t)k * nL + e];
    for (int k = 0; k < PD; ++k)
      Jp[((int64_t)(k * RD + row)) * nL + e] =
          pfix ? T(0) : rg[(int64_t)(CD + k) * nL + e];
  }
}

}  // namespace
}  // namespace megba
