// Host-side edge tables of the GPU engine: the point-band camera chunk table
// and the run-aligned window table.  Plain std::vector in, plain std::vector
// out; no device code, so they are testable without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../problem.hpp"

namespace megba {

// Cam-sorted view of the local edges [e0, e1) and its chunk table.
struct CamChunks {
  std::vector<int> camPos;   // primary edge -> cam-sorted slab row
  std::vector<int> ptOfCam;  // cam-sorted row -> point id
  std::vector<int> chCam, chLo, chHi;  // chunk: camera, rows [chLo, chHi)
};

// Default band width in points: ~2 MB of 4-padded w, raised to the occupancy
// floor that keeps >=64 edges (one full wave pass) per (cam, band) chunk on
// average, or the chunk waves run mostly empty (synth20k measured 694 vs
// 605 ms/step when 20k cams x 153 bands shattered the table into 16-edge
// chunks).
inline int defaultBandPts(size_t elemBytes, int64_t nLocal, int ncam, int npt) {
  int bandPts = (2 << 20) / (4 * (int)elemBytes);
  const int64_t occFloor = nLocal > 0 ? (int64_t)64 * npt * ncam / nLocal : 0;
  if (occFloor > bandPts) bandPts = (int)std::min<int64_t>(occFloor, npt);
  return bandPts;
}

// Point-band blocking: each camera's slab rows are pt-sorted (the cursor
// scatter preserves the primary order), so cutting chunks at point-band
// boundaries and ordering chunks band-major makes every concurrently-
// resident chunk gather w from the SAME ~2 MB slice — small enough to stay
// in the XCD L2 instead of being flushed by the streamed J reads (PMC: 78%
// SQ_WAIT on the unbanded gather, profiles/r02_gather_bands.md).  A chunk
// holds at most chunkRows rows of one camera inside one band; bandPts < 1
// means one band (the whole problem, table unchanged).
inline CamChunks buildCamChunks(const ProblemIndex& ix, int64_t e0, int64_t e1,
                                int ncam, int npt, int chunkRows,
                                int bandPts) {
  const int64_t nL = e1 - e0;
  CamChunks t;
  t.camPos.resize(nL);
  t.ptOfCam.resize(nL);
  std::vector<int> rowPtr(ncam + 1, 0);
  for (int64_t e = 0; e < nL; ++e) rowPtr[ix.camOf[e0 + e] + 1]++;
  for (int c = 0; c < ncam; ++c) rowPtr[c + 1] += rowPtr[c];
  std::vector<int> cursor(rowPtr.begin(), rowPtr.end() - 1);
  for (int64_t e = 0; e < nL; ++e) {
    const int pos = cursor[ix.camOf[e0 + e]]++;
    t.camPos[e] = pos;
    t.ptOfCam[pos] = ix.ptOf[e0 + e];
  }
  if (bandPts < 1) bandPts = npt;
  const int nBands = (npt + bandPts - 1) / bandPts;
  std::vector<int> cBand;
  for (int c = 0; c < ncam; ++c) {
    int s = rowPtr[c];
    while (s < rowPtr[c + 1]) {
      const int band = t.ptOfCam[s] / bandPts;
      const int bandEndPt = (band + 1) * bandPts;
      int e = s;
      const int lim = std::min(s + chunkRows, rowPtr[c + 1]);
      while (e < lim && t.ptOfCam[e] < bandEndPt) ++e;
      t.chCam.push_back(c);
      t.chLo.push_back(s);
      t.chHi.push_back(e);
      cBand.push_back(band);
      s = e;
    }
  }
  if (nBands > 1) {
    // stable band-major order
    const size_t n = t.chCam.size();
    std::vector<int> ord(n);
    for (size_t i = 0; i < n; ++i) ord[i] = (int)i;
    std::stable_sort(ord.begin(), ord.end(),
                     [&](int a, int b) { return cBand[a] < cBand[b]; });
    std::vector<int> c2(n), l2(n), h2(n);
    for (size_t i = 0; i < n; ++i) {
      c2[i] = t.chCam[ord[i]];
      l2[i] = t.chLo[ord[i]];
      h2[i] = t.chHi[ord[i]];
    }
    t.chCam.swap(c2);
    t.chLo.swap(l2);
    t.chHi.swap(h2);
  }
  return t;
}

// Run-aligned windows over the local edges (positions relative to e0) of the
// points [ptLo, ptHi): an unflagged window holds <=64 edges and whole point
// runs only; a run longer than 64 edges is cut into consecutive flagged
// windows of <=64 edges (listed in flagWins, its point in longPts) that the
// long-run kernels finish.
struct RunWindows {
  std::vector<int64_t> winLo, winHi;
  std::vector<unsigned char> winFlag;
  std::vector<int> flagWins, longPts;
};

inline RunWindows buildRunWindows(const ProblemIndex& ix, int64_t e0, int ptLo,
                                  int ptHi) {
  RunWindows w;
  int64_t cur = -1;
  for (int p = ptLo; p < ptHi; ++p) {
    const int64_t lo = ix.ptRowPtr[p] - e0;
    const int64_t hi = ix.ptRowPtr[p + 1] - e0;
    const int64_t len = hi - lo;
    if (len > 64) {
      w.longPts.push_back(p);
      for (int64_t ss = lo; ss < hi; ss += 64) {
        w.flagWins.push_back((int)w.winLo.size());
        w.winLo.push_back(ss);
        w.winHi.push_back(std::min(ss + 64, hi));
        w.winFlag.push_back(1);
      }
      cur = -1;
      continue;
    }
    if (cur >= 0 && w.winHi[cur] - w.winLo[cur] + len <= 64) {
      w.winHi[cur] = hi;
    } else {
      cur = (int64_t)w.winLo.size();
      w.winLo.push_back(lo);
      w.winHi.push_back(hi);
      w.winFlag.push_back(0);
    }
  }
  return w;
}

}  // namespace megba
