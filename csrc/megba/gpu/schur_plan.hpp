// Which kernels one PCG iteration launches, as pure host arithmetic on the
// knobs, two eligibility bits, the local edge count and four timings.  No HIP
// include: GpuEngine (gpu_engine_impl.hpp) supplies the probe launches and the
// timings, tests/test_schur_plan_cpu.py drives the same functions through the
// bindings without a device.
#pragma once

#include <cstdint>
#include <optional>

#include "knobs.hpp"

namespace megba {

// Which kernels form the local E Cinv E^T x product of a PCG iteration.
enum class SchurPath {
  Lds,           // kSchurFusedLds + row reduce (single pass, LDS accumulator)
  LdsRecompute,  // kSchurFusedLdsRc: Lds with the BAL J rebuilt per edge
  FusedEtx,      // kEtxCinvFused, then E w (default)
  Separate,      // E^T x, Cinv, E w as separate passes
  OnePass,       // kSchurFused (MEGBA_FUSED)
};

inline const char* schurPathName(SchurPath p) {
  switch (p) {
    case SchurPath::Lds: return "lds";
    case SchurPath::LdsRecompute: return "lds-recompute";
    case SchurPath::FusedEtx: return "fused-etx";
    case SchurPath::Separate: return "separate";
    case SchurPath::OnePass: break;
  }
  return "one-pass";
}

// What one PCG iteration launches.  Resolved once at the first solve
// (GpuEngine::resolvePlan) and immutable afterwards: the captured hipGraph
// of the PCG body depends on every field.
struct PcgPlan {
  SchurPath path = SchurPath::FusedEtx;
  bool rotatedBody = true;         // four-kernel body (else seven-kernel)
  bool productReadsPad = true;     // the product reads dXPad_, not p
  bool mergeReduceBApply = false;  // kLdsReduceBApplyDot ends the product
};

// The paths the tuner may return.  Which of the two-pass variants wins is
// problem-dependent (Venice wins fused in both dtypes, final13682-fp32 wins
// separate, profiles/r02_gather_bands.md Exp 6), so from 200 k local edges
// on, and unless a knob forces one, the candidates are timed on the real
// data.  Below that launch noise decides, and the default stays.  The two
// LDS applies are candidates where they are eligible (GpuEngine::
// setupSchurLds; MEGBA_NO_SCHUR_LDS / MEGBA_NO_SCHUR_RECOMPUTE act there) and
// either forced or the engine is tuning; MEGBA_SCHUR_RECOMPUTE wins over
// MEGBA_SCHUR_LDS, which in turn takes the recompute form out of the tuning.
struct SchurCandidates {
  SchurPath twoPass;  // Separate under MEGBA_NO_ETXFUSE, else FusedEtx
  bool tuning;        // no forced two-pass variant and nL >= 200000
  bool lds, ldsForced;
  bool rc, rcForced;  // LdsRecompute
};

inline SchurCandidates schurCandidates(const GpuKnobs& k, bool ldsEligible,
                                       bool rcEligible, int64_t nL) {
  SchurCandidates c;
  c.twoPass = k.noEtxFuse ? SchurPath::Separate : SchurPath::FusedEtx;
  c.tuning = !(k.noEtxFuse || k.etxFuse) && nL >= 200000;
  c.ldsForced = k.schurLds;
  c.rcForced = k.schurRecompute;
  c.lds = ldsEligible && (c.ldsForced || c.tuning);
  c.rc = rcEligible && (c.rcForced || (c.tuning && !c.ldsForced));
  return c;
}

// The decision that needs no timing: a path, or nullopt for "time the
// candidates", and then which LDS forms to time next to the two-pass paths.
struct SchurUntimed {
  std::optional<SchurPath> path;
  bool lds, rc;  // still candidates: a candidate that does not launch is out
};
// launches(path) makes the first launch of an LDS candidate and says whether
// the runtime took it; it is called for candidates only, the recompute form
// first and the plain one after the early returns.
template <typename Probe>
SchurUntimed schurPathUntimed(SchurCandidates c, Probe&& launches) {
  if (c.rc) c.rc = launches(SchurPath::LdsRecompute);
  if (c.rcForced && c.rc) return {SchurPath::LdsRecompute, c.lds, c.rc};
  // nothing to choose: a forced two-pass variant, or the launch-noise regime
  if (!c.ldsForced && !c.tuning) return {c.twoPass, c.lds, c.rc};
  if (c.lds) c.lds = launches(SchurPath::Lds);
  if (c.ldsForced)
    return {c.lds ? SchurPath::Lds : c.twoPass, c.lds, c.rc};
  return {std::nullopt, c.lds, c.rc};
}

// The order of the four timings.
constexpr SchurPath kTimedPaths[4] = {SchurPath::FusedEtx, SchurPath::Separate,
                                      SchurPath::Lds, SchurPath::LdsRecompute};

// The decision from the timings ms[4] in kTimedPaths order; the two-pass
// paths are always timed, the LDS ones where they stayed candidates.
// Fused-etx wins a tie with separate; an LDS apply must be strictly faster
// than the better two-pass path, the recompute form than the plain one too.
inline SchurPath schurPathFromTimings(const float ms[4], bool ldsTimed,
                                      bool rcTimed) {
  const int best2 = ms[0] <= ms[1] ? 0 : 1;
  if (rcTimed && ms[3] < ms[best2] && (!ldsTimed || ms[3] < ms[2]))
    return SchurPath::LdsRecompute;
  return ldsTimed && ms[2] < ms[best2] ? SchurPath::Lds : kTimedPaths[best2];
}

inline PcgPlan makePcgPlan(SchurPath tuned, const GpuKnobs& k, bool implicit,
                           int nLongPts, bool allreduceIsNoop) {
  PcgPlan plan;
  plan.path = k.fused ? SchurPath::OnePass : tuned;
  plan.rotatedBody = !k.noPcgFuse;
  // only the explicit separate-pass kSpmvEtx reads the unpadded vector
  plan.productReadsPad = implicit || plan.path != SchurPath::Separate;
  // row reduce, B-apply and dot in one kernel when nothing sits between
  // them: LDS path, no long-run finishers, no collective
  plan.mergeReduceBApply =
      plan.rotatedBody &&
      (plan.path == SchurPath::Lds || plan.path == SchurPath::LdsRecompute) &&
      nLongPts == 0 && allreduceIsNoop;
  return plan;
}

}  // namespace megba
