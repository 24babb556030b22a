// Gaussian unary priors: the small math shared by the CPU and GPU engines.
//
// Three kinds, each a sparse list with at most one entry per vertex:
//   camera parameter prior  r = cam[c] - mean          (camDim)
//   point prior (GCP)       r = pt[p] - mean           (ptDim)
//   camera-centre prior     r = C(cam[c]) - centre     (3), C = -R(aa)^T t
// Every entry carries a symmetric information matrix, packed upper-
// triangular row by row (D(D+1)/2 values, the per-edge `info` convention).
// A prior adds r^T L r to chi^2, J^T L J to the vertex's own diagonal block
// and -J^T L r to its slice of g; the coupling block E is untouched, so the
// Schur paths (which consume HppD, HllInv and g) need no change.
#pragma once

#include "bal_functor.hpp"
#include "jet.hpp"

namespace megba {

// Position of (i, j) in the packed-upper row-major storage of a DxD
// symmetric matrix.
template <int D>
MEGBA_HD constexpr int packedIdx(int i, int j) {
  const int a = i < j ? i : j;
  const int b = i < j ? j : i;
  return a * D - a * (a - 1) / 2 + (b - a);
}

// out = W in for the packed symmetric W.
template <typename T, int D>
MEGBA_HD inline void symApply(const T* W, const T* in, T* out) {
  for (int i = 0; i < D; ++i) {
    T s = T(0);
    for (int j = 0; j < D; ++j) s += W[packedIdx<D>(i, j)] * in[j];
    out[i] = s;
  }
}

// v^T W v for the packed symmetric W.
template <typename T, int D>
MEGBA_HD inline T symQuad(const T* W, const T* v) {
  T q = T(0);
  for (int i = 0; i < D; ++i) {
    T s = T(0);
    for (int j = 0; j < D; ++j) s += W[packedIdx<D>(i, j)] * v[j];
    q += v[i] * s;
  }
  return q;
}

// Camera centre C = -R(aa)^T t of a BAL-convention camera (params 0..2
// angle-axis, 3..5 t) and its 3x6 Jacobian J[a*6 + i] = dC_a / dcam_i, by
// forward-mode jets through the same Rodrigues rotation the reprojection
// residual uses: R(aa)^T = R(-aa), so C = -rotate(-aa, t).
template <typename T>
MEGBA_HD inline void cameraCentre(const T* cam, T C[3], T J[18]) {
  using J6 = Jet<T, 6>;
  J6 naa[3], t[3], out[3];
  for (int i = 0; i < 3; ++i) {
    naa[i] = -J6::leaf(cam[i], i);
    t[i] = J6::leaf(cam[3 + i], 3 + i);
  }
  angleAxisRotatePoint<T, J6>(naa, t, out);
  for (int a = 0; a < 3; ++a) {
    C[a] = -out[a].v;
    for (int i = 0; i < 6; ++i) J[a * 6 + i] = -out[a].d[i];
  }
}

}  // namespace megba
