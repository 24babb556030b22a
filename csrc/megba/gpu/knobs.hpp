// MEGBA_* environment knobs of the GPU engine, read once at engine
// construction (GpuKnobs::fromEnv) and immutable afterwards: the resolved
// PCG plan and the captured graph depend on them.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <optional>

namespace megba {

struct GpuKnobs {
  // boolean knobs: presence of the variable means on
  bool mfma = false;         // MEGBA_MFMA: MFMA camera assembly (fp64 BAL)
  bool fused = false;        // MEGBA_FUSED: one-pass kSchurFused product
  bool fwdVS = false;        // MEGBA_FWD_VS: value-share forward (BAL)
  bool etxAtomic = false;    // MEGBA_ETX_ATOMIC: scan-free E^T x
  bool etxFuse = false;      // MEGBA_ETXFUSE: force the fused window kernel
  bool noEtxFuse = false;    // MEGBA_NO_ETXFUSE: force the separate passes
  bool schurLds = false;     // MEGBA_SCHUR_LDS: force the LDS apply if eligible
  bool noSchurLds = false;   // MEGBA_NO_SCHUR_LDS: take the LDS apply out
  // MEGBA_SCHUR_RECOMPUTE: force the recomputed-J LDS apply if eligible (wins
  // over MEGBA_SCHUR_LDS); MEGBA_NO_SCHUR_RECOMPUTE: take it out
  bool schurRecompute = false;
  bool noSchurRecompute = false;
  // MEGBA_NO_RC_STAGE: the recompute apply gathers camera rows per lane
  // instead of through the staged, quad-coalesced LDS tile
  bool noRcStage = false;
  bool noPcgFuse = false;    // MEGBA_NO_PCG_FUSE: seven-kernel PCG body
  bool noGraph = false;      // MEGBA_NO_GRAPH: no hipGraph capture
  bool forceRccl = false;    // MEGBA_FORCE_RCCL: world-1 RCCL communicator
  bool tuneVerbose = false;  // MEGBA_TUNE_VERBOSE: report the Schur path
  // MEGBA_DENSE_PROFILE: time the kernels of the dense Cholesky one by one
  bool denseProfile = false;
  // numeric knobs: unset = engine default
  std::optional<int64_t> schurLdsMaxBytes;  // MEGBA_SCHUR_LDS_MAX_BYTES (atoll)
  std::optional<int> schurLdsThreads;       // MEGBA_SCHUR_LDS_THREADS (atoi)
  std::optional<int> chunk;                 // MEGBA_CHUNK (atoi)
  std::optional<int> band;                  // MEGBA_BAND (atoi)
  // MEGBA_DENSE_TILE_CAMS: cameras per LDS row tile of kDenseSchurForm
  // (lowered in tests so that small problems take several tiles)
  std::optional<int> denseTileCams;

  static GpuKnobs fromEnv() {
    const auto on = [](const char* name) { return getenv(name) != nullptr; };
    const auto num = [](const char* name) -> std::optional<int> {
      const char* v = getenv(name);
      return v ? std::optional<int>(std::atoi(v)) : std::nullopt;
    };
    GpuKnobs k;
    k.mfma = on("MEGBA_MFMA");
    k.fused = on("MEGBA_FUSED");
    k.fwdVS = on("MEGBA_FWD_VS");
    k.etxAtomic = on("MEGBA_ETX_ATOMIC");
    k.etxFuse = on("MEGBA_ETXFUSE");
    k.noEtxFuse = on("MEGBA_NO_ETXFUSE");
    k.schurLds = on("MEGBA_SCHUR_LDS");
    k.noSchurLds = on("MEGBA_NO_SCHUR_LDS");
    k.schurRecompute = on("MEGBA_SCHUR_RECOMPUTE");
    k.noSchurRecompute = on("MEGBA_NO_SCHUR_RECOMPUTE");
    k.noRcStage = on("MEGBA_NO_RC_STAGE");
    k.noPcgFuse = on("MEGBA_NO_PCG_FUSE");
    k.noGraph = on("MEGBA_NO_GRAPH");
    k.forceRccl = on("MEGBA_FORCE_RCCL");
    k.tuneVerbose = on("MEGBA_TUNE_VERBOSE");
    k.denseProfile = on("MEGBA_DENSE_PROFILE");
    if (const char* v = getenv("MEGBA_SCHUR_LDS_MAX_BYTES"))
      k.schurLdsMaxBytes = std::atoll(v);
    k.schurLdsThreads = num("MEGBA_SCHUR_LDS_THREADS");
    k.chunk = num("MEGBA_CHUNK");
    k.band = num("MEGBA_BAND");
    k.denseTileCams = num("MEGBA_DENSE_TILE_CAMS");
    return k;
  }
};

}  // namespace megba
