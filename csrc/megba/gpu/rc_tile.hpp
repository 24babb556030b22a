// Camera row table and wave-private LDS tile of the recomputed-J Schur
// product (kSchurFusedLdsRc).  Host and device constants only, so the slot
// function is testable without a GPU.
#pragma once

#include "../jet.hpp"

namespace megba {

// One row per camera, cut in 64-byte segments so that every row starts on a
// 64-byte boundary:
//   [0, kRcXOff)           balCameraPart row (kBalSnapshot, per accepted step)
//   [kRcXOff, kRcXOff + 9) the product's input x for that camera
//   rest                   zeros, written once at allocation
constexpr int kRcSegBytes = 64;
constexpr int kRcChunkBytes = 16;
constexpr int kRcSegChunks = kRcSegBytes / kRcChunkBytes;
constexpr int kRcXOff = 12;
template <typename T>
struct RcRow {
  // 24 doubles (192 B, three segments) / 32 floats (128 B, two segments)
  static constexpr int LEN = sizeof(T) == 8 ? 24 : 32;
  static constexpr int SEGS = LEN * (int)sizeof(T) / kRcSegBytes;
};

// The staged gather moves one segment of 64 rows at a time through a tile of
// 64 rows x 64 B per wave.
constexpr int kRcTileRows = 64;
constexpr int kRcTileBytes = kRcTileRows * kRcSegBytes;

// Dynamic LDS of the staged instance: the nc accumulators, then one tile per
// wave from this byte offset on, 16-byte aligned for the 128-bit LDS
// accesses.  Kernel and host sizing both take it from here.
MEGBA_HD constexpr long long rcTileOffset(long long nc, int elemBytes) {
  return (nc * elemBytes + 15) / 16 * 16;
}
MEGBA_HD constexpr long long rcStagedLdsBytes(long long nc, int elemBytes,
                                              int waves) {
  return rcTileOffset(nc, elemBytes) + (long long)waves * kRcTileBytes;
}

// Byte offset of 16-byte chunk `chunk` (0..3) of tile row `row` (0..63).
// Rows at a 64-byte pitch would put the 16 lanes of a ds_read_b128 group on
// four banks each; rotating the chunk by bits 2-3 of the row spreads a group
// over all 64 banks, and keeps the 8 lanes of a ds_write_b128 group (two
// neighbouring rows, four chunks each) on distinct banks too.
MEGBA_HD constexpr int rcTileSlot(int row, int chunk) {
  return row * kRcSegBytes + ((chunk ^ ((row >> 2) & 3)) * kRcChunkBytes);
}

}  // namespace megba
