// Host-side problem container and index construction.
//
// Capability anchor: the reference's BaseProblem/HessianEntrance/EdgeVector
// index build (/root/reference/src/problem/base_problem.cpp:96-214,
// src/linear_system/schur_LM_linear_system.cpp:20-84).  Redesign:
// observations are globally counting-sorted by (point, camera) once on the
// host, and ranks take contiguous chunks ALIGNED TO POINT BOUNDARIES.  That
// makes every point (and its Hll block, g_p entries, Cinv apply, E^T x
// reduction and back-substitution) local to exactly one rank; only the small
// camera-side vectors (9*ncam) are replicated and allreduced.  The reference
// replicates the POINT side instead and pays a 3*npt-word allreduce per PCG
// iteration (its site A4) — on Venice that is 24 MB/iteration vs 128 KB
// here, a ~190x traffic reduction tuned for xGMI's per-link ring bandwidth.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "common.hpp"

namespace megba {

// Raw problem as handed over from Python (original observation order).
// Block dims are carried here (default BAL 9/3/2); the reference's
// runtime-dim analogue is ProblemOption.N + per-kernel cameraDim/pointDim/
// resDim arguments (include/common.h:27-46, build_linear_system.cu:48-146).
// One kind of Gaussian unary prior (prior.hpp): a sparse list over vertices,
// at most one entry per vertex.  D = camDim (camera parameter prior), ptDim
// (point prior) or 3 (camera-centre prior).
struct PriorList {
  std::vector<int> idx;      // m vertex ids
  std::vector<double> mean;  // m*D ([entry][D])
  // optional m * D*(D+1)/2 packed-upper symmetric information matrices;
  // empty = identity.  Positive semi-definiteness beyond a non-negative
  // diagonal is the caller's responsibility.
  std::vector<double> info;
  bool empty() const { return idx.empty(); }
};

struct BAProblemHost {
  int ncam = 0;
  int npt = 0;
  int64_t nobs = 0;
  int camDim = 9;
  int ptDim = 3;
  int resDim = 2;
  std::vector<double> cams;  // ncam*camDim
  std::vector<double> pts;   // npt*ptDim
  std::vector<int> camIdx;   // nobs
  std::vector<int> ptIdx;    // nobs
  std::vector<double> meas;  // nobs*resDim ([obs][resDim])
  // optional nobs * resDim*(resDim+1)/2 packed-upper symmetric per-edge
  // information matrix (RD=2: w00,w01,w11); empty = identity
  std::vector<double> info;
  std::vector<uint8_t> camFixed;  // optional ncam (g2o-style fixed vertices)
  std::vector<uint8_t> ptFixed;   // optional npt
  // optional soft unary constraints (beyond the reference)
  PriorList camPrior;     // r = cam[c] - mean
  PriorList ptPrior;      // r = pt[p] - mean (ground control points)
  PriorList centerPrior;  // r = C(cam[c]) - centre (GPS), BAL cameras only
  bool hasPriors() const {
    return !camPrior.empty() || !ptPrior.empty() || !centerPrior.empty();
  }
};

// Reject malformed prior lists.  `customForward`: the problem is solved with
// a user-defined residual, whose camera parametrisation is unknown.
inline void validatePriors(const BAProblemHost& p, bool customForward) {
  const auto check = [](const PriorList& l, int nVert, int D,
                        const std::string& what) {
    const size_t m = l.idx.size();
    const size_t W = (size_t)D * (D + 1) / 2;
    MEGBA_CHECK(l.mean.size() == m * D,
                what + " prior: mean must be (m, " + std::to_string(D) + ")");
    MEGBA_CHECK(l.info.empty() || l.info.size() == m * W,
                what + " prior: info must be (m, " + std::to_string(W) +
                    ") packed-upper symmetric");
    std::vector<char> seen((size_t)nVert, 0);
    for (size_t k = 0; k < m; ++k) {
      const int v = l.idx[k];
      MEGBA_CHECK(v >= 0 && v < nVert, what + " prior: index out of range");
      MEGBA_CHECK(!seen[v], what + " prior: duplicate index");
      seen[v] = 1;
    }
    for (const double x : l.mean)
      MEGBA_CHECK(std::isfinite(x), what + " prior: non-finite mean");
    for (const double x : l.info)
      MEGBA_CHECK(std::isfinite(x), what + " prior: non-finite info");
    if (!l.info.empty())
      for (size_t k = 0; k < m; ++k)
        for (int i = 0; i < D; ++i)
          MEGBA_CHECK(l.info[k * W + (size_t)(i * D - i * (i - 1) / 2)] >= 0.0,
                      what + " prior: negative diagonal in info");
  };
  check(p.camPrior, p.ncam, p.camDim, "camera");
  check(p.ptPrior, p.npt, p.ptDim, "point");
  check(p.centerPrior, p.ncam, 3, "camera-centre");
  MEGBA_CHECK(p.centerPrior.empty() ||
                  (!customForward && (p.camDim == 9 || p.camDim == 6) &&
                   p.ptDim == 3 && p.resDim == 2),
              "camera-centre prior needs the built-in BAL residual ((9,3,2) "
              "or (6,3,2), no custom forward): params 0..5 must be "
              "angle-axis and t");
}

struct ProblemIndex {
  int ncam = 0, npt = 0;
  int64_t nobs = 0;
  int resDim = 2;
  // Arrays in (point, camera)-sorted order:
  std::vector<int> camOf, ptOf;     // nobs
  std::vector<double> measSorted;   // nobs*resDim
  std::vector<double> infoSorted;   // nobs*resDim*(resDim+1)/2 or empty
  std::vector<int64_t> ptRowPtr;    // npt+1: edge range of each point
  std::vector<int64_t> split;       // worldSize+1 edge partition (point-aligned)
  std::vector<int> ptSplit;         // worldSize+1 point-id partition
  std::vector<int64_t> perm;        // sorted position -> original observation id
};

inline ProblemIndex buildIndex(const BAProblemHost& p, int worldSize) {
  MEGBA_CHECK(p.ncam > 0 && p.npt > 0 && p.nobs > 0, "empty problem");
  MEGBA_CHECK((int64_t)p.camIdx.size() == p.nobs && (int64_t)p.ptIdx.size() == p.nobs,
              "index array size mismatch");
  ProblemIndex ix;
  ix.ncam = p.ncam;
  ix.npt = p.npt;
  ix.nobs = p.nobs;
  ix.resDim = p.resDim;
  const int rd = p.resDim;
  const int rw = rd * (rd + 1) / 2;
  const int64_t n = p.nobs;

  // Stable counting sort: by camera, then by point -> (pt, cam) order.
  std::vector<int64_t> tmpPerm(n), cnt;
  {
    cnt.assign((size_t)p.ncam + 1, 0);
    for (int64_t e = 0; e < n; ++e) {
      const int c = p.camIdx[e];
      MEGBA_CHECK(c >= 0 && c < p.ncam, "camera index out of range");
      cnt[c + 1]++;
    }
    for (int v = 0; v < p.ncam; ++v) cnt[v + 1] += cnt[v];
    for (int64_t e = 0; e < n; ++e) tmpPerm[cnt[p.camIdx[e]]++] = e;
  }
  ix.perm.resize(n);
  {
    cnt.assign((size_t)p.npt + 1, 0);
    for (int64_t e = 0; e < n; ++e) {
      const int pt = p.ptIdx[e];
      MEGBA_CHECK(pt >= 0 && pt < p.npt, "point index out of range");
      cnt[pt + 1]++;
    }
    for (int v = 0; v < p.npt; ++v) cnt[v + 1] += cnt[v];
    ix.ptRowPtr.assign(cnt.begin(), cnt.end());  // prefix before scatter
    for (int64_t k = 0; k < n; ++k) {
      const int64_t e = tmpPerm[k];
      ix.perm[cnt[p.ptIdx[e]]++] = e;
    }
  }

  ix.camOf.resize(n);
  ix.ptOf.resize(n);
  ix.measSorted.resize(n * rd);
  const bool hasInfo = !p.info.empty();
  if (hasInfo) ix.infoSorted.resize(n * rw);
  for (int64_t k = 0; k < n; ++k) {
    const int64_t e = ix.perm[k];
    ix.camOf[k] = p.camIdx[e];
    ix.ptOf[k] = p.ptIdx[e];
    for (int d = 0; d < rd; ++d) ix.measSorted[rd * k + d] = p.meas[rd * e + d];
    if (hasInfo)
      for (int d = 0; d < rw; ++d)
        ix.infoSorted[rw * k + d] = p.info[rw * e + d];
  }

  // Every vertex must be observed (else its Hessian block is singular).
  {
    std::vector<char> seenCam((size_t)p.ncam, 0);
    for (int64_t k = 0; k < n; ++k) seenCam[ix.camOf[k]] = 1;
    for (int c = 0; c < p.ncam; ++c)
      MEGBA_CHECK(seenCam[c], "camera with no observations");
    for (int v = 0; v < p.npt; ++v)
      MEGBA_CHECK(ix.ptRowPtr[v + 1] > ix.ptRowPtr[v],
                  "point with no observations");
  }

  // Balanced contiguous partition, aligned to point boundaries so each
  // point's whole edge run lives on one rank.
  MEGBA_CHECK(worldSize <= p.npt, "more ranks than points");
  ix.split.resize(worldSize + 1);
  ix.ptSplit.resize(worldSize + 1);
  ix.split[0] = 0;
  ix.ptSplit[0] = 0;
  int prevPt = 0;
  for (int r = 1; r < worldSize; ++r) {
    const int64_t target = (n * r) / worldSize;
    // first point whose run starts at or after target
    int lo = prevPt, hi = p.npt;
    while (lo < hi) {
      const int mid = (lo + hi) / 2;
      if (ix.ptRowPtr[mid] < target)
        lo = mid + 1;
      else
        hi = mid;
    }
    lo = std::max(lo, prevPt + 1);  // at least one point per rank
    // ...and leave at least one point for every later rank (a skewed
    // distribution can otherwise push the split past npt).
    lo = std::min(lo, p.npt - (worldSize - r));
    ix.ptSplit[r] = lo;
    ix.split[r] = ix.ptRowPtr[lo];
    prevPt = lo;
  }
  ix.ptSplit[worldSize] = p.npt;
  ix.split[worldSize] = n;
  return ix;
}

}  // namespace megba
