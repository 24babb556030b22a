// Gaussian unary priors: the per-entry math, once, for the CPU and GPU
// engines.
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
//
// Both engines keep a kind's m local entries component-major -- idx[m],
// mean[D][m], info[D(D+1)/2][m], r[D][m] and, for the centre kind, J[18][m]
// -- so a GPU wave's accesses to one component are contiguous.  A kind policy
// (ParamKind, CentreKind) says what r and J are; the three phases of an LM
// step are one per-entry function each (priorEvaluate, priorAssembleRow,
// priorModel), which the CPU engine loops over and the GPU kernels
// grid-stride over.
#pragma once

#include "bal_functor.hpp"
#include "jet.hpp"
#include "problem.hpp"

namespace megba {

// Position of (i, j) in the packed-upper row-major storage of a DxD
// symmetric matrix.
template <int D>
MEGBA_HD constexpr int packedIdx(int i, int j) {
  const int a = i < j ? i : j;
  const int b = i < j ? j : i;
  return a * D - a * (a - 1) / 2 + (b - a);
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

// One kind's local entries, non-owning.  r and J point at the buffer set in
// use (current or accepted); J is null for the parameter kinds.
template <typename T>
struct PriorView {
  int64_t m;
  const int* idx;
  const T* mean;
  const T* info;
  T* r;
  T* J;
};

// Parameter prior on a D-wide vertex: r = x[v] - mean, J = I.
template <int D_>
struct ParamKind {
  static constexpr int D = D_;     // residual width
  static constexpr int VD = D_;    // vertex width: x, dx, g stride; H is VDxVD
  static constexpr int ROWS = D_;  // rows of the vertex's block it touches
  static constexpr bool kHasJ = false;
};

// Centre prior on a CD-wide BAL camera: r = C(cam) - centre, 3x6 J on the
// leading six parameters.
template <int CD>
struct CentreKind {
  static constexpr int D = 3;
  static constexpr int VD = CD;
  static constexpr int ROWS = 6;
  static constexpr bool kHasJ = true;
};

// v^T L v with entry k's information.
template <int D, typename T>
MEGBA_HD inline T priorQuadForm(const PriorView<T>& p, int64_t k, const T* v) {
  T q = T(0);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    T s = T(0);
#pragma unroll
    for (int j = 0; j < D; ++j)
      s += p.info[packedIdx<D>(i, j) * p.m + k] * v[j];
    q += v[i] * s;
  }
  return q;
}

// Forward: writes entry k's r (and J) at the vertex parameters x (the base
// of the kind's vertex array) and returns r^T L r.
template <typename Kind, typename T>
MEGBA_HD inline T priorEvaluate(const PriorView<T>& p, int64_t k, const T* x) {
  const T* xv = x + (int64_t)p.idx[k] * Kind::VD;
  T v[Kind::D];
  if constexpr (Kind::kHasJ) {
    T cam[6], C[3], Jl[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) cam[i] = xv[i];
    cameraCentre<T>(cam, C, Jl);
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = C[a] - p.mean[a * p.m + k];
#pragma unroll
    for (int q = 0; q < 18; ++q) p.J[q * p.m + k] = Jl[q];
  } else {
#pragma unroll
    for (int i = 0; i < Kind::D; ++i) v[i] = xv[i] - p.mean[i * p.m + k];
  }
#pragma unroll
  for (int i = 0; i < Kind::D; ++i) p.r[i * p.m + k] = v[i];
  return priorQuadForm<Kind::D>(p, k, v);
}

// Assembly: adds row i (< Kind::ROWS) of J^T L J to the block of entry k's
// vertex in H and subtracts row i of J^T L r from its slice of g.  The caller
// skips fixed vertices.
template <typename Kind, typename T>
MEGBA_HD inline void priorAssembleRow(const PriorView<T>& p, int64_t k, int i,
                                      T* H, T* g) {
  constexpr int D = Kind::D, VD = Kind::VD;
  const int64_t m = p.m;
  const int64_t v = p.idx[k];
  T* hRow = H + v * VD * VD + i * VD;
  T gs = T(0);
  if constexpr (Kind::kHasJ) {
    // u = L J[:, i]
    T col[D], u[D];
#pragma unroll
    for (int a = 0; a < D; ++a) col[a] = p.J[(a * 6 + i) * m + k];
#pragma unroll
    for (int b = 0; b < D; ++b) {
      u[b] = T(0);
#pragma unroll
      for (int a = 0; a < D; ++a)
        u[b] += p.info[packedIdx<D>(b, a) * m + k] * col[a];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      T s = T(0);
#pragma unroll
      for (int b = 0; b < D; ++b) s += u[b] * p.J[(b * 6 + j) * m + k];
      hRow[j] += s;
    }
#pragma unroll
    for (int b = 0; b < D; ++b) gs += u[b] * p.r[b * m + k];
  } else {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const T l = p.info[packedIdx<D>(i, j) * m + k];
      hRow[j] += l;
      gs += l * p.r[j * m + k];
    }
  }
  g[v * VD + i] -= gs;
}

// Gain ratio: (J dx + r)^T L (J dx + r) of entry k, dx the base of the kind's
// step array; a fixed vertex does not move, so its term stays r^T L r.
template <typename Kind, typename T>
MEGBA_HD inline T priorModel(const PriorView<T>& p, int64_t k, bool isFixed,
                             const T* dx) {
  constexpr int D = Kind::D;
  const T* dv = dx + (int64_t)p.idx[k] * Kind::VD;
  T a[D];
#pragma unroll
  for (int b = 0; b < D; ++b) {
    if constexpr (Kind::kHasJ) {
      a[b] = p.r[b * p.m + k];
      if (!isFixed) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a[b] += p.J[(b * 6 + i) * p.m + k] * dv[i];
      }
    } else {
      a[b] = p.r[b * p.m + k] + (isFixed ? T(0) : dv[b]);
    }
  }
  return priorQuadForm<D>(p, k, a);
}

// Host side: a PriorList's entries with vertex in [lo, hi), component-major
// as above, identity information where the list carries none.  The engines
// cast to their scalar type and allocate r and J.
struct PackedPrior {
  int64_t m = 0;
  std::vector<int> idx;
  std::vector<double> mean, info;
};

template <int D>
inline PackedPrior packPriorList(const PriorList& l, int lo, int hi) {
  constexpr int W = D * (D + 1) / 2;
  std::vector<size_t> keep;
  for (size_t k = 0; k < l.idx.size(); ++k)
    if (l.idx[k] >= lo && l.idx[k] < hi) keep.push_back(k);
  PackedPrior s;
  const size_t m = keep.size();
  s.m = (int64_t)m;
  s.idx.resize(m);
  s.mean.resize(m * D);
  s.info.resize(m * W);
  for (size_t q = 0; q < m; ++q) {
    const size_t k = keep[q];
    s.idx[q] = l.idx[k];
    for (int i = 0; i < D; ++i) s.mean[i * m + q] = l.mean[k * D + i];
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j)
        s.info[packedIdx<D>(i, j) * m + q] =
            l.info.empty() ? (i == j ? 1.0 : 0.0)
                           : l.info[k * W + packedIdx<D>(i, j)];
  }
  return s;
}

}  // namespace megba
