// MI355X (gfx950) engine: HIP kernels + host orchestration + RCCL collectives.
//
// Kernel / distribution design (MI355X-first redesign, not a port —
// behavioural anchors cite /root/reference):
//  * Observations are (point, camera)-sorted and partitioned on POINT
//    boundaries: each rank owns its points outright, so the whole point side
//    (Hll, g_p, Cinv, E^T x, back-substitution) is communication-free and
//    the only per-PCG-iteration collective is an allreduce of the replicated
//    camera vector (9*ncam = 128 KB on Venice).  The reference replicates
//    the point side instead and allreduces 3*npt words (24 MB on Venice)
//    per iteration (its sites A1/A3-A6) — a ~190x traffic reduction sized
//    for xGMI's per-link ring bandwidth.
//  * kForward fuses the ENTIRE vectorised-autodiff forward pass into one
//    kernel: each observation is handled by 4 consecutive lanes, each lane
//    carrying a Jet<T,3> slice of the 12-wide dual part, so every
//    intermediate of the reprojection expression lives in VGPRs.  The
//    reference launches ~1 CUDA kernel per elementary op and streams
//    (N+1)*nItem doubles through HBM each time
//    (src/operator/jet_vector_math_impl.cu).
//  * Assembly transports the camera-side per-edge data through a cam-sorted
//    edge-major slab (contiguous ~400 B per edge, ~1 line-fetch per 64 B)
//    instead of per-element transpose gathers (8x amplification) or
//    per-element atomics (the all-atomic version measured 40.8 ms on
//    Venice-5M, profiles/r01_venice_single_gpu.md).  Point-side Hll/g_p
//    accumulate with a wave-level segmented scan over the point-sorted runs
//    — atomics only at segment tails.
//  * Control-flow scalars (rho, p^T q, norms) use fixed-shape two-pass
//    deterministic reductions so every rank takes identical PCG branches.
//  * r2 additions: every kernel and the engine are templated over the
//    block dims (camDim, ptDim, resDim) — instantiation TUs
//    gpu_dims_*.hip, runtime dispatch in gpu_engine.hip; the per-
//    iteration product kernels read 16-byte packed vector-group J/Hpl
//    layouts with 4-padded w and XP-padded x gathers; the camera-chunk
//    table is point-band-blocked so the gathered w slice stays
//    L2-resident; the PCG body is hipGraph-captured (incl. the RCCL
//    allreduce) with device pointer-slot indirection for the double-
//    buffered J set; fused-vs-separate E^T x + Cinv is auto-tuned per
//    problem.  Measured history: profiles/r02_gather_bands.md.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <optional>
#include <type_traits>
#include <utility>
#include <vector>

#include "../jv/jetvector.hpp"
#include "edge_ops.hpp"
#include "edge_tables.hpp"
#include "gpu_common.hpp"
#include "gpu_engine.hpp"
#include "kernels_assemble.hpp"
#include "kernels_forward.hpp"
#include "kernels_pcg.hpp"
#include "kernels_prior.hpp"
#include "kernels_product.hpp"
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

// What one PCG iteration launches.  Resolved once at the first solve
// (GpuEngine::resolvePlan) and immutable afterwards: the captured hipGraph
// of the PCG body depends on every field.
struct PcgPlan {
  SchurPath path = SchurPath::FusedEtx;
  bool rotatedBody = true;         // four-kernel body (else seven-kernel)
  bool productReadsPad = true;     // the product reads dXPad_, not p
  bool mergeReduceBApply = false;  // kLdsReduceBApplyDot ends the product
};

// ===========================================================================
// Host engine
// ===========================================================================
template <typename T, int CD, int PD, int RD>
class GpuEngine final : public Engine<T> {
  static constexpr int GW = CD + PD;            // gradient width
  static constexpr int CC = CD * CD;            // Hpp block
  static constexpr int PP = PD * PD;            // Hll block
  static constexpr int CP = CD * PD;            // Hpl block
  static constexpr int CR = CD * RD;            // Jc values per edge
  static constexpr int PR = PD * RD;            // Jp values per edge
  static constexpr int RW = RD * (RD + 1) / 2;  // packed info entries
  static constexpr bool kBalDims = CD == 9 && PD == 3 && RD == 2;
  using PkJ = PackedEdge<T, CD, PD, RD, true>;   // implicit [Jc, Jp] groups
  using PkH = PackedEdge<T, CD, PD, RD, false>;  // explicit Hpl groups

 public:
  GpuEngine(const BAProblemHost& prob, const ProblemIndex& ix,
            const ProblemOption& opt, const std::string& rcclId,
            CustomForward<T> customForward, HostAllreduce<T> hostAllreduce,
            HostAllreduce<double> hostAllreduceScalar)
      : knobs_(GpuKnobs::fromEnv()),
        customFwd_(std::move(customForward)),
        hostAr_(std::move(hostAllreduce)),
        hostArD_(std::move(hostAllreduceScalar)),
        rank_(opt.rank),
        world_(opt.worldSize),
        ncam_(ix.ncam),
        npt_(ix.npt),
        analytical_(opt.diff == DiffMode::ANALYTICAL),
        implicit_(opt.schur == SchurMode::IMPLICIT),
        lossKind_((int)opt.loss),
        lossD2_((T)(opt.lossDelta * opt.lossDelta)) {
    MEGBA_CHECK(!analytical_ || (CD == 9 && PD == 3 && RD == 2),
                "analytical diff is only available for the BAL (9,3,2) model");
    MEGBA_CHECK(customFwd_ || hasBuiltinResidual(CD, PD, RD),
                "no built-in residual for these dims: provide custom_forward");
    HIP_CHECK(hipSetDevice(opt.deviceIndex));
    HIP_CHECK(hipStreamCreate(&stream_));
    e0_ = ix.split[rank_];
    e1_ = ix.split[rank_ + 1];
    nL_ = e1_ - e0_;
    ptLo_ = ix.ptSplit[rank_];
    ptHi_ = ix.ptSplit[rank_ + 1];
    npL_ = ptHi_ - ptLo_;
    nc_ = (int64_t)ncam_ * CD;
    np_ = (int64_t)npt_ * PD;
    dim_ = nc_ + np_;
    hasInfo_ = !ix.infoSorted.empty();
    {
      double h[3] = {opt.intr[0], opt.intr[1], opt.intr[2]};
      dIntr_ = dalloc<T>(3);
      upCast(dIntr_, h, 3);
    }

    if (world_ > 1) {
      if (rcclId.empty() && hostAr_) {
        // gloo-backed testing fallback (several ranks may share one GPU)
      } else {
        MEGBA_CHECK(rcclId.size() == sizeof(ncclUniqueId),
                    "worldSize>1 requires the RCCL unique id (or a host "
                    "allreduce fallback)");
        ncclUniqueId id;
        std::memcpy(&id, rcclId.data(), sizeof(id));
        RCCL_CHECK(ncclCommInitRank(&comm_, world_, id, rank_));
        hasComm_ = true;
      }
    } else if (knobs_.forceRccl) {
      // 1-GPU hardening mode: run a real world-1 RCCL communicator so
      // ncclCommInitRank, every ncclAllReduce call site and RCCL-under-
      // hipGraph-capture are exercised on a single GPU (the multi-rank
      // collective SEQUENCE is identical; only the ring is trivial).
      ncclUniqueId id;
      if (rcclId.size() == sizeof(id))
        std::memcpy(&id, rcclId.data(), sizeof(id));
      else
        RCCL_CHECK(ncclGetUniqueId(&id));
      RCCL_CHECK(ncclCommInitRank(&comm_, 1, id, 0));
      hasComm_ = true;
    }

    // Static per-edge data (primary = (pt,cam)-sorted order).
    dCamOf_ = dalloc<int>(nL_);
    dPtOf_ = dalloc<int>(nL_);
    up(dCamOf_, ix.camOf.data() + e0_, nL_);
    up(dPtOf_, ix.ptOf.data() + e0_, nL_);
    if (!prob.camFixed.empty()) {
      dCamFixed_ = dalloc<unsigned char>(ncam_);
      up(dCamFixed_, prob.camFixed.data(), ncam_);
    }
    if (!prob.ptFixed.empty()) {
      dPtFixed_ = dalloc<unsigned char>(npt_);
      up(dPtFixed_, prob.ptFixed.data(), npt_);
    }
    dMeas_ = dalloc<T>(nL_ * RD);
    upCast(dMeas_, ix.measSorted.data() + RD * e0_, nL_ * RD);
    if (customFwd_) {
      dLeaf_ = dalloc<T>(nL_ * GW);
      dMeasSplit_ = dalloc<T>(nL_ * RD);
      std::vector<T> ms(nL_ * RD);
      for (int64_t e = 0; e < nL_; ++e)
        for (int r = 0; r < RD; ++r)
          ms[(int64_t)r * nL_ + e] = (T)ix.measSorted[RD * (e0_ + e) + r];
      up(dMeasSplit_, ms.data(), nL_ * RD);
    }
    if (hasInfo_) {
      dInfo_ = dalloc<T>(nL_ * RW);
      upCast(dInfo_, ix.infoSorted.data() + RW * e0_, nL_ * RW);
    }

    // Parameters (cameras replicated; this rank maintains its point shard).
    dParams_ = dalloc<T>(dim_);
    dParamsBak_ = dalloc<T>(dim_);
    {
      std::vector<T> h(dim_);
      for (int64_t i = 0; i < nc_; ++i) h[i] = (T)prob.cams[i];
      for (int64_t i = 0; i < np_; ++i) h[nc_ + i] = (T)prob.pts[i];
      up(dParams_, h.data(), dim_);
      HIP_CHECK(hipMemcpyAsync(dParamsBak_, dParams_, dim_ * sizeof(T),
                               hipMemcpyDeviceToDevice, stream_));
    }

    // Residual / Jacobian double-buffer (current + accepted).
    for (int s = 0; s < 2; ++s) {
      dR_[s] = dalloc<T>(nL_ * RD);
      dJc_[s] = dalloc<T>(nL_ * CR);
      dJp_[s] = dalloc<T>(nL_ * PR);
    }

    // Linear system (full-size global indexing; only this rank's point
    // ranges of Hll/g_p/temp are maintained).
    dHpp_ = dalloc<T>((int64_t)ncam_ * CC);
    dHll_ = dalloc<T>((int64_t)npt_ * PP);
    dG_ = dalloc<T>(dim_);
    dGBak_ = dalloc<T>(dim_);
    dHppD_ = dalloc<T>((int64_t)ncam_ * CC);
    dHllD_ = dalloc<T>((int64_t)npt_ * PP);
    dHppInv_ = dalloc<T>((int64_t)ncam_ * CC);
    dHllInv_ = dalloc<T>((int64_t)npt_ * PP);
    dDeltaX_ = dalloc<T>(dim_);
    dDeltaXBak_ = dalloc<T>(dim_);
    HIP_CHECK(hipMemsetAsync(dDeltaX_, 0, dim_ * sizeof(T), stream_));
    HIP_CHECK(hipMemsetAsync(dDeltaXBak_, 0, dim_ * sizeof(T), stream_));

    // PCG workspace.
    dP_ = dalloc<T>(nc_);
    dRr_ = dalloc<T>(nc_);
    dZ_ = dalloc<T>(nc_);
    dQ_ = dalloc<T>(nc_);
    dV_ = dalloc<T>(nc_);
    dXBak_ = dalloc<T>(nc_);
    dXBakPrev_ = dalloc<T>(nc_);
    HIP_CHECK(hipMemsetAsync(dXBak_, 0, nc_ * sizeof(T), stream_));
    HIP_CHECK(hipMemsetAsync(dXBakPrev_, 0, nc_ * sizeof(T), stream_));
    dW_ = dalloc<T>(np_);
    dTemp_ = dalloc<T>(np_);
    HIP_CHECK(hipMemsetAsync(dW_, 0, np_ * sizeof(T), stream_));

    // Partial-sum scratch: big enough for both the fixed-shape two-pass
    // reductions (kRedBlocks) and the fused B-apply+dot grid over nc_.
    // The rotated PCG body adds two more producers: one rho partial per
    // kUpdateXRPrecond block and one p.q partial per 64 columns.
    partCap_ = std::max({kRedBlocks, bApplyDotGrid(), precondGrid(),
                         ldsReduceGrid()});
    dPart_ = dalloc<double>(partCap_ + 8);
    dPartQ_ = dalloc<double>(partCap_);
    dFail_ = dalloc<int>(2);
    HIP_CHECK(hipHostMalloc((void**)&hScalar_, sizeof(double)));

    // Cam-sorted view of the local edges: slab positions + chunk table.
    {
      // cam-chunk rows default 256 (MEGBA_CHUNK), band default ~2 MB of
      // padded w (MEGBA_BAND)
      const CamChunks t = buildCamChunks(
          ix, e0_, e1_, ncam_, npt_, knobs_.chunk.value_or(256),
          knobs_.band ? *knobs_.band
                      : defaultBandPts(sizeof(T), nL_, ncam_, npt_));
      nChunks_ = (int)t.chCam.size();
      dCamPos_ = upNew(t.camPos);
      dPtOfCam_ = upNew(t.ptOfCam);
      dChCam_ = upNew(t.chCam);
      dChLo_ = upNew(t.chLo);
      dChHi_ = upNew(t.chHi);
    }
    // Run-aligned windows (<=64 edges, whole point runs) for the fused
    // Schur apply; runs longer than 64 edges are flagged and finished by
    // the long-run kernels.
    {
      const RunWindows w = buildRunWindows(ix, e0_, ptLo_, ptHi_);
      nWin_ = (int)w.winLo.size();
      nFlagWins_ = (int)w.flagWins.size();
      nLongPts_ = (int)w.longPts.size();
      dWinLo_ = upNew(w.winLo);
      dWinHi_ = upNew(w.winHi);
      dWinFlag_ = upNew(w.winFlag);
      if (nFlagWins_ > 0) dFlagWins_ = upNew(w.flagWins);
      if (nLongPts_ > 0) dLongPts_ = upNew(w.longPts);
    }
    dSlab_ = dalloc<T>(nL_ * slabWidth());
    dJSlots_ = dalloc<const T*>(3);
    updateJSlots();
    // packed vector-group layouts (16B groups; padded to a full group)
    if (implicit_) {
      dJPk_ = dalloc<T>(nL_ * PkJ::NG * PkJ::VEC);
      dJCamPk_ = dalloc<T>(nL_ * PkJ::NG * PkJ::VEC);
    }
    dXPad_ = dalloc<T>((int64_t)ncam_ * PkJ::XP);
    dWPad_ = dalloc<T>((int64_t)npt_ * 4);
    if (!implicit_) {
      dHpl_ = dalloc<T>(nL_ * PkH::NG * PkH::VEC);
      dHplCam_ = dalloc<T>(nL_ * PkH::NG * PkH::VEC);
    }
    setupSchurLds(opt.deviceIndex);
    // Unary priors: nothing is allocated for an empty kind.  Camera kinds
    // are replicated; point priors go to the rank that owns the point.
    initPrior<CD>(camPr_, prob.camPrior, 0, ncam_, 0);
    initPrior<3>(ctrPr_, prob.centerPrior, 0, ncam_, 18);
    initPrior<PD>(ptPr_, prob.ptPrior, ptLo_, ptHi_, 0);
    hasPriors_ = camPr_.m + ctrPr_.m + ptPr_.m > 0;
    sync();
  }

  ~GpuEngine() override {
    if (hScalar_) (void)hipHostFree(hScalar_);
    if (pcgGraphExec_) (void)hipGraphExecDestroy(pcgGraphExec_);
    for (void* p : allocs_) (void)hipFree(p);
    if (hasComm_) (void)ncclCommDestroy(comm_);
    (void)hipStreamDestroy(stream_);
  }

  double forward() override {
    freshCur_ = true;
    if (customFwd_) return forwardCustom();
    zeroScalar();
    if (analytical_) {
      // compile the analytical launch only for its valid dims
      if constexpr (CD == 9 && PD == 3 && RD == 2)
        hipLaunchKernelGGL(kForwardAnalytical<T>, dim3(gridFor(nL_)),
                           dim3(kBlk), 0, stream_, nL_, dCamOf_, dPtOf_,
                           dParams_, ncam_, dMeas_, dCamFixed_, dPtFixed_,
                           dR_[cur_], dJc_[cur_], dJp_[cur_], scalarPtr(),
                           lossKind_, lossD2_);
    } else {
      constexpr int LANES = (GW + 2) / 3;
      bool launched = false;
      if constexpr (CD == 9 && PD == 3 && RD == 2) {
        if (knobs_.fwdVS) {
          hipLaunchKernelGGL(kForwardVS<T>, dim3(gridFor(nL_ * 4)),
                             dim3(kBlk), 0, stream_, nL_, dCamOf_, dPtOf_,
                             dParams_, ncam_, dMeas_, dCamFixed_, dPtFixed_,
                             dR_[cur_], dJc_[cur_], dJp_[cur_], scalarPtr(),
                             lossKind_, lossD2_);
          launched = true;
        }
      }
      if (!launched)
        hipLaunchKernelGGL((kForward<T, CD, PD, RD>),
                           dim3(gridFor(nL_ * LANES)), dim3(kBlk), 0, stream_,
                           nL_, dCamOf_, dPtOf_, dParams_, ncam_, dMeas_,
                           dCamFixed_, dPtFixed_, dR_[cur_], dJc_[cur_],
                           dJp_[cur_], scalarPtr(), lossKind_, lossD2_,
                           dIntr_);
    }
    if (hasPriors_) priorForward();
    return globalScalar(ncclSum);
  }

  void acceptForward() override {
    cur_ ^= 1;          // accepted set = dX_[cur_^1]
    freshCur_ = false;  // the (new) current buffers are not yet written
    updateJSlots();
    // the recompute path rebuilds J from the point it was evaluated at, which
    // dParams_ holds now and stops holding at the next updateParams()
    if (rcEligible_ && (!plan_ || plan_->path == SchurPath::LdsRecompute))
      snapshotAccepted();
  }

  // Camera part of the row table and 4-padded local points of the accepted
  // linearisation point (kBalSnapshot), read by kSchurFusedLdsRc alone.
  void snapshotAccepted() {
    if constexpr (kBalDims)
      hipLaunchKernelGGL(kBalSnapshot<T>, dim3(gridFor((int64_t)ncam_ + npL_)),
                         dim3(kBlk), 0, stream_, ncam_, ptLo_, npL_, dParams_,
                         dCamRow_, rcCamStride(), dPtAcc_);
  }

  // Point the device slots at the accepted (bak) buffer set.
  void updateJSlots() {
    const int bak = cur_ ^ 1;
    hipLaunchKernelGGL(kSetPtrSlots<T>, dim3(1), dim3(1), 0, stream_,
                       dJSlots_, dJc_[bak], dJp_[bak], dR_[bak]);
  }

  double forwardCustom() {
    hipLaunchKernelGGL((kGatherLeaves<T, CD, PD>), dim3(gridFor(nL_)),
                       dim3(kBlk), 0, stream_, nL_, dCamOf_, dPtOf_, dParams_,
                       ncam_, dLeaf_);
    sync();  // JetVector ops run on the null stream
    std::vector<JetVec<T>> camL, ptL, ms, res;
    for (int k = 0; k < CD; ++k)
      camL.push_back(jvView<T>(dLeaf_ + (int64_t)k * nL_, nL_, GW, k, true));
    for (int k = 0; k < PD; ++k)
      ptL.push_back(
          jvView<T>(dLeaf_ + (int64_t)(CD + k) * nL_, nL_, GW, CD + k, true));
    for (int r = 0; r < RD; ++r)
      ms.push_back(jvView<T>(dMeasSplit_ + (int64_t)r * nL_, nL_, GW, -1, true));
    customFwd_(camL, ptL, ms, res);
    MEGBA_CHECK((int)res.size() == RD,
                "custom forward must return resDim residuals");
    HIP_CHECK(hipDeviceSynchronize());
    for (int r = 0; r < RD; ++r) {
      MEGBA_CHECK(res[r].kind() == JvKind::DENSE && res[r].nItem == nL_ &&
                      res[r].N == GW && res[r].onGpu,
                  "custom residual must be a dense GPU JetVector "
                  "(N=camDim+ptDim)");
      hipLaunchKernelGGL((kRepackRes<T, CD, PD, RD>), dim3(gridFor(nL_)),
                         dim3(kBlk), 0, stream_, nL_, r, res[r].value->ptr,
                         res[r].grad->ptr, dCamOf_, dPtOf_, dCamFixed_,
                         dPtFixed_, dR_[cur_], dJc_[cur_], dJp_[cur_]);
    }
    if (lossKind_) {
      zeroScalar();
      hipLaunchKernelGGL((kChi2Loss<T, RD>), dim3(gridFor(nL_)), dim3(kBlk),
                         0, stream_, nL_, dR_[cur_], lossKind_, lossD2_,
                         scalarPtr());
    } else {
      reduceDetAsync(dR_[cur_], dR_[cur_], nL_ * RD, ROp::SumSq, scalarPtr());
    }
    // after the edge chi^2: reduceDetAsync overwrites the accumulator
    if (hasPriors_) priorForward();
    return globalScalar(ncclSum);
  }

  void buildLinearSystem() override {
    const int bak = cur_ ^ 1;
    HIP_CHECK(hipMemsetAsync(dHpp_, 0, (int64_t)ncam_ * CC * sizeof(T), stream_));
    HIP_CHECK(hipMemsetAsync(dHll_ + (int64_t)ptLo_ * PP, 0,
                             (int64_t)npL_ * PP * sizeof(T), stream_));
    HIP_CHECK(hipMemsetAsync(dG_, 0, nc_ * sizeof(T), stream_));
    HIP_CHECK(hipMemsetAsync(dG_ + nc_ + (int64_t)ptLo_ * PD, 0,
                             (int64_t)npL_ * PD * sizeof(T), stream_));
    dispatchAssemble(bak);
    if (!implicit_)
      dispatchBool(weighted(), [&](auto weightedTag) {
        hipLaunchKernelGGL(
            (kFinalizeCam<T, CD, PD, RD, decltype(weightedTag)::value>),
            dim3(gridFor(nL_)), dim3(kBlk), 0, stream_, nL_, dSlab_, dHplCam_);
      });
    else
      dispatchBool(weighted(), [&](auto weightedTag) {
        hipLaunchKernelGGL(
            (kFinalizeCamImpPk<T, CD, PD, RD, decltype(weightedTag)::value>),
            dim3(gridFor(nL_)), dim3(kBlk), 0, stream_, nL_, dSlab_, dJCamPk_);
      });
    // Only the small camera-side quantities cross ranks (the reference
    // allreduced Hpp, Hll AND g, its site A1).
    allreduce(dHpp_, (int64_t)ncam_ * CC, ncclSum);
    allreduce(dG_, nc_, ncclSum);
    // Prior terms go in after the allreduce: every rank adds the same
    // replicated camera terms once; point terms stay on the owning shard.
    if (hasPriors_) priorAssemble();
    sync();
  }

  void backupParams() override {
    HIP_CHECK(hipMemcpyAsync(dParamsBak_, dParams_, dim_ * sizeof(T),
                             hipMemcpyDeviceToDevice, stream_));
  }
  void rollbackParams() override {
    HIP_CHECK(hipMemcpyAsync(dParams_, dParamsBak_, dim_ * sizeof(T),
                             hipMemcpyDeviceToDevice, stream_));
  }
  void backupGDx() override {
    HIP_CHECK(hipMemcpyAsync(dDeltaXBak_, dDeltaX_, dim_ * sizeof(T),
                             hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(dGBak_, dG_, dim_ * sizeof(T),
                             hipMemcpyDeviceToDevice, stream_));
  }
  void rollbackGDx() override {
    HIP_CHECK(hipMemcpyAsync(dDeltaX_, dDeltaXBak_, dim_ * sizeof(T),
                             hipMemcpyDeviceToDevice, stream_));
    HIP_CHECK(hipMemcpyAsync(dG_, dGBak_, dim_ * sizeof(T),
                             hipMemcpyDeviceToDevice, stream_));
  }

  void processDiag(double region) override {
    const T f = T(1) + T(1) / (T)region;
    hipLaunchKernelGGL((kDamp<T, CD>), dim3(gridFor((int64_t)ncam_ * CC)),
                       dim3(kBlk), 0, stream_, (int64_t)ncam_ * CC, dHpp_,
                       dHppD_, f, dCamFixed_);
    hipLaunchKernelGGL((kDamp<T, PD>), dim3(gridFor((int64_t)npL_ * PP)),
                       dim3(kBlk), 0, stream_, (int64_t)npL_ * PP,
                       dHll_ + (int64_t)ptLo_ * PP, dHllD_ + (int64_t)ptLo_ * PP,
                       f, dPtFixed_ ? dPtFixed_ + ptLo_ : nullptr);
  }

  int solveLinear(const SolverOptionPCG& opt) override {
    // Block inverses (preconditioner replicated; Cinv on the local shard).
    HIP_CHECK(hipMemsetAsync(dFail_, 0, 2 * sizeof(int), stream_));
    hipLaunchKernelGGL((kInvert<T, CD>), dim3(gridFor(ncam_)), dim3(kBlk), 0,
                       stream_, ncam_, dHppD_, dHppInv_, dFail_);
    hipLaunchKernelGGL((kInvert<T, PD>), dim3(gridFor(npL_)), dim3(kBlk), 0,
                       stream_, npL_, dHllD_ + (int64_t)ptLo_ * PP,
                       dHllInv_ + (int64_t)ptLo_ * PP, dFail_);
    int fail[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(fail, dFail_, 2 * sizeof(int),
                             hipMemcpyDeviceToHost, stream_));
    sync();
    if (fail[0]) {
      hipLaunchKernelGGL((kInvertJitter<T, CD>), dim3(gridFor(ncam_)),
                         dim3(kBlk), 0, stream_, ncam_, dHppD_, dHppInv_,
                         dFail_);
      hipLaunchKernelGGL((kInvertJitter<T, PD>), dim3(gridFor(npL_)),
                         dim3(kBlk), 0, stream_, npL_,
                         dHllD_ + (int64_t)ptLo_ * PP,
                         dHllInv_ + (int64_t)ptLo_ * PP, dFail_);
      HIP_CHECK(hipMemcpyAsync(fail, dFail_, 2 * sizeof(int),
                               hipMemcpyDeviceToHost, stream_));
      sync();
      MEGBA_CHECK(!fail[1], "singular Hessian block");
    }

    if (!plan_) plan_ = resolvePlan();
    const T* gc = dG_;
    const T* gp = dG_ + nc_;
    // v = gc/world - E Cinv gp  (partial, then the CD*ncam allreduce)
    cinvThenEx(gp, dV_);
    hipLaunchKernelGGL(kVMake<T>, dim3(gridFor(nc_)), dim3(kBlk), 0, stream_,
                       nc_, gc, T(1) / T(world_), dV_);
    allreduce(dV_, nc_, ncclSum);
    // Warm start: x = deltaX camera part (in place in dDeltaX_).
    T* x = dDeltaX_;
    schurApply({x, false}, dQ_, /*withDot=*/false);
    hipLaunchKernelGGL(kSub<T>, dim3(gridFor(nc_)), dim3(kBlk), 0, stream_, nc_,
                       dV_, dQ_, dRr_);

    // The loop body is value-uniform (beta/alpha live on-device; the first
    // iteration gets beta = rho/INF = 0 against a zeroed p), so it is
    // captured once as a hipGraph and replayed with ONE host interaction per
    // iteration: the rho readback that drives the reference's refuse/tol
    // control flow.  Refuse semantics are preserved with a two-deep x backup
    // (the body runs speculatively; on refuse x is restored to the value two
    // updates back, exactly what the reference's pre-update check restores).
    HIP_CHECK(hipMemsetAsync(dP_, 0, nc_ * sizeof(T), stream_));
    hipLaunchKernelGGL(kSetScalar, dim3(1), dim3(1), 0, stream_, slotRhoPrev(),
                       INFINITY);
    // Rotated body: the first z = Binv r and rho partials come from here,
    // every later one from the tail of the previous body.
    if (plan_->rotatedBody)
      hipLaunchKernelGGL((kPrecondRho<T, CD>), dim3(precondGrid()), dim3(kBlk),
                         0, stream_, ncam_, dHppInv_, dRr_, dZ_, dPart_);
    int n = 0;
    double rho = 0.0, rhoMin = INFINITY;
    bool done = false;
    ensurePcgGraph();
    // Fixed-work mode (tol<=0 with refuse disabled, the bench contract):
    // rho steers nothing, so skip the per-iteration host readback and
    // enqueue all maxIter bodies back-to-back — ONE host sync per solve
    // instead of one per iteration (the N=8 constant-term killer).
    const bool fixedWork = opt.tol <= 0.0 && opt.refuseRatio >= 1e29;
    if (fixedWork) {
      for (; n < opt.maxIter; ++n) {
        if (pcgGraphExec_)
          HIP_CHECK(hipGraphLaunch(pcgGraphExec_, stream_));
        else
          pcgBody();
      }
    } else {
      while (!done && n < opt.maxIter) {
        if (pcgGraphExec_) {
          HIP_CHECK(hipGraphLaunch(pcgGraphExec_, stream_));
        } else {
          pcgBody();
        }
        rho = readScalar(slotRho());
        if (rho > opt.refuseRatio * rhoMin) {
          HIP_CHECK(hipMemcpyAsync(x, dXBakPrev_, nc_ * sizeof(T),
                                   hipMemcpyDeviceToDevice, stream_));
          break;
        }
        rhoMin = rhoMin < rho ? rhoMin : rho;
        ++n;
        done = std::abs(rho) < opt.tol;
      }
    }
    // Back-substitution: deltaX_p = Cinv (g_p - E^T x), fully local.
    spmvEtx({x, false}, dTemp_);
    hipLaunchKernelGGL((kBackSub<T, PD>), dim3(gridFor(npL_)), dim3(kBlk), 0,
                       stream_, npL_, dHllInv_ + (int64_t)ptLo_ * PP,
                       gp + (int64_t)ptLo_ * PD, dTemp_ + (int64_t)ptLo_ * PD,
                       dDeltaX_ + nc_ + (int64_t)ptLo_ * PD);
    sync();
    return n;
  }

  double deltaXL2() override {
    const double camSS = reduceDet(dDeltaX_, dDeltaX_, nc_, ROp::SumSq);
    reduceDetAsync(dDeltaX_ + nc_ + (int64_t)ptLo_ * PD,
                   dDeltaX_ + nc_ + (int64_t)ptLo_ * PD, (int64_t)npL_ * PD,
                   ROp::SumSq, scalarPtr());
    return std::sqrt(camSS + globalScalar(ncclSum));
  }
  double xL2() override {
    const double camSS = reduceDet(dParams_, dParams_, nc_, ROp::SumSq);
    reduceDetAsync(dParams_ + nc_ + (int64_t)ptLo_ * PD,
                   dParams_ + nc_ + (int64_t)ptLo_ * PD, (int64_t)npL_ * PD,
                   ROp::SumSq, scalarPtr());
    return std::sqrt(camSS + globalScalar(ncclSum));
  }
  double gInf() override {
    const double camMax = reduceDet(dG_, dG_, nc_, ROp::AbsMax);
    reduceDetAsync(dG_ + nc_ + (int64_t)ptLo_ * PD,
                   dG_ + nc_ + (int64_t)ptLo_ * PD, (int64_t)npL_ * PD,
                   ROp::AbsMax, scalarPtr());
    const double ptMax = globalScalar(ncclMax);
    return camMax > ptMax ? camMax : ptMax;
  }

  void updateParams() override {
    hipLaunchKernelGGL(kAddAssign<T>, dim3(gridFor(nc_)), dim3(kBlk), 0,
                       stream_, nc_, dDeltaX_, dParams_);
    hipLaunchKernelGGL(kAddAssign<T>, dim3(gridFor((int64_t)npL_ * PD)),
                       dim3(kBlk), 0, stream_, (int64_t)npL_ * PD,
                       dDeltaX_ + nc_ + (int64_t)ptLo_ * PD,
                       dParams_ + nc_ + (int64_t)ptLo_ * PD);
  }

  double rhoDenominator(double chi2Backup) override {
    const int bak = cur_ ^ 1;
    zeroScalar();
    if (implicit_) {
      // packed accepted J + padded deltaX camera vector
      padX(dDeltaX_, xPadDst());
      hipLaunchKernelGGL((kRhoDenomPk<T, CD, PD, RD>), dim3(gridFor(nL_)),
                         dim3(kBlk), 0, stream_, nL_, dCamOf_, dPtOf_,
                         dR_[bak], dJPk_, dXPad_, dDeltaX_ + nc_,
                         scalarPtr(), lossKind_, lossD2_);
    } else {
      hipLaunchKernelGGL((kRhoDenom<T, CD, PD, RD>), dim3(gridFor(nL_)),
                         dim3(kBlk), 0, stream_, nL_, dCamOf_, dPtOf_,
                         dR_[bak], dJc_[bak], dJp_[bak], dDeltaX_,
                         dDeltaX_ + nc_, scalarPtr(), lossKind_, lossD2_);
    }
    if (hasPriors_) priorRho();
    return globalScalar(ncclSum) - chi2Backup;
  }

  void getParams(double* cams, double* pts) override {
    std::vector<T> hc(nc_);
    HIP_CHECK(hipMemcpy(hc.data(), dParams_, nc_ * sizeof(T),
                        hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nc_; ++i) cams[i] = (double)hc[i];
    if (world_ > 1 && (hasComm_ || hostAr_)) {
      // point shards: zero the non-local entries, allreduce-sum.
      if (!dPtMerge_) dPtMerge_ = dalloc<T>(np_);
      T* tmp = dPtMerge_;
      HIP_CHECK(hipMemsetAsync(tmp, 0, np_ * sizeof(T), stream_));
      HIP_CHECK(hipMemcpyAsync(tmp + (int64_t)ptLo_ * PD,
                               dParams_ + nc_ + (int64_t)ptLo_ * PD,
                               (int64_t)npL_ * PD * sizeof(T),
                               hipMemcpyDeviceToDevice, stream_));
      allreduce(tmp, np_, ncclSum);
      sync();
      std::vector<T> h(np_);
      HIP_CHECK(hipMemcpy(h.data(), tmp, np_ * sizeof(T), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < np_; ++i) pts[i] = (double)h[i];
      return;
    }
    std::vector<T> h(np_);
    HIP_CHECK(hipMemcpy(h.data(), dParams_ + nc_, np_ * sizeof(T),
                        hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < np_; ++i) pts[i] = (double)h[i];
  }

  DenseDump dump() const override {
    DenseDump d;
    d.e0 = e0_;
    d.e1 = e1_;
    // r/J of the LAST forward() (survives the acceptForward buffer swap)
    const int fw = freshCur_ ? cur_ : (cur_ ^ 1);
    d.r = down(dR_[fw], nL_ * RD);
    d.Jc = down(dJc_[fw], nL_ * CR);
    d.Jp = down(dJp_[fw], nL_ * PR);
    d.Hpp = down(dHpp_, (int64_t)ncam_ * CC);
    d.Hll = down(dHll_, (int64_t)npt_ * PP);
    if (!implicit_) {
      // device Hpl is packed [group][nL][VEC]; dump as [e][CD][PD]
      constexpr int VEC = PkH::VEC;
      std::vector<double> gm = down(dHpl_, nL_ * PkH::NG * VEC);
      std::vector<double> o((size_t)nL_ * CP);
      for (int64_t e = 0; e < nL_; ++e)
        for (int k = 0; k < CP; ++k)
          o[e * CP + k] =
              gm[((int64_t)(k / VEC) * nL_ + e) * VEC + k % VEC];
      d.Hpl = o;
    }
    d.g = down(dG_, dim_);
    d.deltaX = down(dDeltaX_, dim_);
    // Dump layouts match the CPU engine: r [e][RD], Jc [e][RD][CD],
    // Jp [e][RD][PD] (the device layout is gradient-major; transpose here).
    d.r = transposeR(d.r);
    d.Jc = transposeJ(d.Jc, CD);
    d.Jp = transposeJ(d.Jp, PD);
    return d;
  }

 private:
  // ---- unary priors (kernels_prior.hpp) -----------------------------------
  // One kind's local entries in the layout of prior.hpp; r and the centre
  // kind's J are double-buffered on cur_ exactly like the edge r/J.
  struct DevPrior {
    int64_t m = 0;
    int* idx{};
    T *mean{}, *info{};  // identity information if the list has none
    T* r[2]{};
    T* J[2]{};           // centre kind only
    PriorView<T> view(int b) const { return {m, idx, mean, info, r[b], J[b]}; }
  };

  // Keep the entries whose vertex lies in [lo, hi) and upload them.
  template <int D>
  void initPrior(DevPrior& s, const PriorList& l, int lo, int hi, int jw) {
    const PackedPrior h = packPriorList<D>(l, lo, hi);
    const int64_t m = h.m;
    if (m == 0) return;
    s.m = m;
    s.idx = dalloc<int>(m);
    HIP_CHECK(hipMemcpy(s.idx, h.idx.data(), m * sizeof(int),
                        hipMemcpyHostToDevice));
    s.mean = dalloc<T>(h.mean.size());
    s.info = dalloc<T>(h.info.size());
    upCast(s.mean, h.mean.data(), h.mean.size());
    upCast(s.info, h.info.data(), h.info.size());
    for (int b = 0; b < 2; ++b) {
      s.r[b] = dalloc<T>(m * D);
      HIP_CHECK(hipMemsetAsync(s.r[b], 0, m * D * sizeof(T), stream_));
      if (jw > 0) {
        s.J[b] = dalloc<T>(m * jw);
        HIP_CHECK(hipMemsetAsync(s.J[b], 0, m * jw * sizeof(T), stream_));
      }
    }
  }

  // Grid of the kernels that end in one atomicAdd per block on the scalar
  // accumulator: capped, so a prior on every point of a Venice-sized
  // problem queues ~1e3 same-address atomics, not one per 256 points (the
  // uncapped forward took 55 us for 76 MB; the grid-stride loops cover the
  // rest).
  static int priorRedGrid(int64_t m) {
    const int g = gridFor(m);
    return g < 1024 ? g : 1024;
  }

  // What differs between the kinds at a launch: the vertex arrays the kind
  // lives on and where its scalars are counted.
  struct PriorSite {
    const T *x, *dx;
    T *H, *g;
    const unsigned char* fixed;
    double* acc;
  };

  // f(kind tag, per-row assembly tag, entries, site) for every non-empty
  // kind: camera parameters, centre, point.  The camera kinds are
  // replicated, so rank 0 alone counts their scalars; their assembly runs
  // one thread per block row, the point kind's one thread per prior.
  template <typename F>
  void forEachPrior(F&& f) {
    const PriorSite cam{dParams_, dDeltaX_, dHpp_, dG_, dCamFixed_,
                        rank_ == 0 ? scalarPtr() : nullptr};
    const PriorSite pt{dParams_ + nc_, dDeltaX_ + nc_, dHll_, dG_ + nc_,
                       dPtFixed_, scalarPtr()};
    if (camPr_.m > 0) f(ParamKind<CD>{}, std::true_type{}, camPr_, cam);
    if constexpr (CD >= 6) {
      if (ctrPr_.m > 0) f(CentreKind<CD>{}, std::true_type{}, ctrPr_, cam);
    }
    if (ptPr_.m > 0) f(ParamKind<PD>{}, std::false_type{}, ptPr_, pt);
  }

  // r (and the centre J) at the current parameters into the current set;
  // adds this rank's share of sum r^T L r to the scalar accumulator.
  void priorForward() {
    forEachPrior([&](auto kind, auto, const DevPrior& s, const PriorSite& at) {
      const PriorView<T> p = s.view(cur_);
      hipLaunchKernelGGL((kPriorForward<T, decltype(kind)>),
                         dim3(priorRedGrid(p.m)), dim3(kBlk), 0, stream_, p.m,
                         p.idx, p.mean, p.info, p.r, p.J, at.x, at.acc);
    });
  }

  // J^T L J and -J^T L r of the accepted set onto the vertices' own blocks.
  void priorAssemble() {
    forEachPrior([&](auto kind, auto perRow, const DevPrior& s,
                     const PriorSite& at) {
      using Kind = decltype(kind);
      constexpr bool PER_ROW = decltype(perRow)::value;
      const PriorView<T> p = s.view(cur_ ^ 1);
      hipLaunchKernelGGL((kPriorAssemble<T, Kind, PER_ROW>),
                         dim3(gridFor(PER_ROW ? p.m * Kind::ROWS : p.m)),
                         dim3(kBlk), 0, stream_, p.m, p.idx, p.info, p.r, p.J,
                         at.fixed, at.H, at.g);
    });
  }

  // The priors' share of the gain-ratio model, from the accepted set.
  void priorRho() {
    forEachPrior([&](auto kind, auto, const DevPrior& s, const PriorSite& at) {
      const PriorView<T> p = s.view(cur_ ^ 1);
      hipLaunchKernelGGL((kPriorRho<T, decltype(kind)>),
                         dim3(priorRedGrid(p.m)), dim3(kBlk), 0, stream_, p.m,
                         p.idx, p.info, p.r, p.J, at.fixed, at.dx, at.acc);
    });
  }

  bool weighted() const { return hasInfo_ || lossKind_ != 0; }
  int slabWidth() const {
    // must match SlabLayout<CD, PD, RD, EXPL, weighted()>::SW
    return (implicit_ ? 0 : CP) + CR + RD + (weighted() ? CR : 0) +
           (implicit_ ? PR : 0);
  }
  void dispatchAssemble(int bak) {
    auto launch = [&](auto weightedTag, auto explTag) {
      constexpr bool HI = decltype(weightedTag)::value;
      constexpr bool EX = decltype(explTag)::value;
      hipLaunchKernelGGL((kAssembleEdge<T, CD, PD, RD, HI, EX>),
                         dim3(gridFor(nL_)), dim3(kBlk), 0, stream_, nL_,
                         dCamOf_, dPtOf_, dR_[bak], dJc_[bak], dJp_[bak],
                         dInfo_, dHll_, dHpl_, dG_, ncam_, dCamPos_, dSlab_,
                         lossKind_, lossD2_, dJPk_);
      if (nChunks_ > 0) {
        if constexpr (std::is_same<T, double>::value && CD == 9 && PD == 3 &&
                      RD == 2) {
          if (knobs_.mfma) {
            hipLaunchKernelGGL((kAssembleCamMfma<T, CD, PD, RD, HI, EX>),
                               dim3(nChunks_), dim3(64), 0, stream_,
                               nChunks_, dChCam_, dChLo_, dChHi_, dSlab_,
                               dHpp_, dG_);
            return;
          }
        }
        hipLaunchKernelGGL((kAssembleCam<T, CD, PD, RD, HI, EX>),
                           dim3(nChunks_), dim3(128), 0, stream_, nChunks_,
                           dChCam_, dChLo_, dChHi_, dSlab_, dHpp_, dG_);
      }
    };
    dispatchBool(weighted(), [&](auto weightedTag) {
      dispatchBool(!implicit_,
                   [&](auto explTag) { launch(weightedTag, explTag); });
    });
  }
  // f(tag) with a runtime bool as an integral_constant tag.
  template <typename F>
  static decltype(auto) dispatchBool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
  }
  template <typename U>
  U* dalloc(int64_t n) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, (n > 0 ? n : 1) * sizeof(U)));
    allocs_.push_back(p);
    return (U*)p;
  }
  // Allocate a device array for a host table and upload it.
  template <typename U>
  U* upNew(const std::vector<U>& h) {
    U* d = dalloc<U>((int64_t)h.size());
    up(d, h.data(), (int64_t)h.size());
    return d;
  }
  template <typename U>
  void up(U* dst, const U* src, int64_t n) {
    if (n > 0)
      HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(U), hipMemcpyHostToDevice,
                               stream_));
  }
  void upCast(T* dst, const double* src, int64_t n) {
    std::vector<T> h(n);
    for (int64_t i = 0; i < n; ++i) h[i] = (T)src[i];
    if (n > 0)
      HIP_CHECK(hipMemcpy(dst, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  std::vector<double> down(const T* src, int64_t n) const {
    std::vector<T> h(n);
    HIP_CHECK(hipMemcpy(h.data(), (void*)src, n * sizeof(T), hipMemcpyDeviceToHost));
    return std::vector<double>(h.begin(), h.end());
  }
  std::vector<double> transposeR(const std::vector<double>& v) const {
    std::vector<double> o(v.size());
    for (int64_t e = 0; e < nL_; ++e)
      for (int row = 0; row < RD; ++row) o[RD * e + row] = v[row * nL_ + e];
    return o;
  }
  std::vector<double> transposeJ(const std::vector<double>& v,
                                 int cols) const {
    std::vector<double> o(v.size());
    for (int64_t e = 0; e < nL_; ++e)
      for (int col = 0; col < cols; ++col)
        for (int row = 0; row < RD; ++row)
          o[e * cols * RD + row * cols + col] =
              v[((int64_t)(col * RD + row)) * nL_ + e];
    return o;
  }
  void sync() { HIP_CHECK(hipStreamSynchronize(stream_)); }
  double* scalarPtr() { return dPart_ + partCap_; }
  double* slotRho() { return dPart_ + partCap_ + 1; }
  double* slotRhoPrev() { return dPart_ + partCap_ + 4; }
  void zeroScalar() {
    HIP_CHECK(hipMemsetAsync(scalarPtr(), 0, sizeof(double), stream_));
  }
  // Read the device scalar accumulator, allreducing across ranks first.
  double globalScalar(ncclRedOp_t op) {
    if (hasComm_) {
      RCCL_CHECK(ncclAllReduce(scalarPtr(), scalarPtr(), 1, ncclDouble, op,
                               comm_, stream_));
      return readScalar(scalarPtr());
    }
    if ((hostArD_ || hostAr_) && world_ > 1) {
      // Host-callback fallback: reduce in full double (the device
      // accumulator already is double) so fp32 multi-rank runs don't lose
      // precision in chi2/deltaXL2/gInf.
      double h = readScalar(scalarPtr());
      if (hostArD_) {
        hostArD_(&h, 1, op == ncclMax ? 'm' : 's');
        return h;
      }
      T v = (T)h;
      hostAr_(&v, 1, op == ncclMax ? 'm' : 's');
      return (double)v;
    }
    return readScalar(scalarPtr());
  }
  double readScalar(double* dptr) {
    // pinned-host destination: the PCG loop does one of these per iteration
    HIP_CHECK(hipMemcpyAsync(hScalar_, dptr, sizeof(double),
                             hipMemcpyDeviceToHost, stream_));
    sync();
    return *hScalar_;
  }
  // No communicator and no host callback: allreduce() does nothing.
  bool allreduceIsNoop() const {
    return !hasComm_ && (world_ == 1 || !hostAr_);
  }
  void allreduce(T* buf, int64_t n, ncclRedOp_t op) {
    if (n == 0 || (world_ == 1 && !hasComm_)) return;
    if (hasComm_) {
      RCCL_CHECK(ncclAllReduce(buf, buf, n,
                               sizeof(T) == 8 ? ncclDouble : ncclFloat, op,
                               comm_, stream_));
      return;
    }
    if (!hostAr_) return;
    // gloo-backed testing fallback: bounce through the host.
    sync();
    std::vector<T> h(n);
    HIP_CHECK(hipMemcpy(h.data(), buf, n * sizeof(T), hipMemcpyDeviceToHost));
    hostAr_(h.data(), n, op == ncclMax ? 'm' : 's');
    HIP_CHECK(hipMemcpy(buf, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  void reduceDetAsync(const T* a, const T* b, int64_t n, ROp op, double* out) {
    const auto launch = [&](auto opTag) {
      constexpr ROp OP = decltype(opTag)::value;
      hipLaunchKernelGGL((kRedPartial<T, OP>), dim3(kRedBlocks), dim3(kBlk), 0,
                         stream_, a, b, n, dPart_);
      hipLaunchKernelGGL((kRedFinal<OP>), dim3(1), dim3(kBlk), 0, stream_,
                         dPart_, kRedBlocks, out);
    };
    switch (op) {
      case ROp::Dot: launch(std::integral_constant<ROp, ROp::Dot>{}); break;
      case ROp::SumSq: launch(std::integral_constant<ROp, ROp::SumSq>{}); break;
      case ROp::AbsMax: launch(std::integral_constant<ROp, ROp::AbsMax>{}); break;
    }
  }
  double reduceDet(const T* a, const T* b, int64_t n, ROp op) {
    reduceDetAsync(a, b, n, op, scalarPtr());
    return readScalar(scalarPtr());
  }
  template <int D, int MODE>
  void blockMatVec(int nBlk, const T* A, const T* xv, T* yv) {
    hipLaunchKernelGGL((kBlockDiagMatVec<T, D, MODE>),
                       dim3(gridFor((int64_t)nBlk * D)), dim3(kBlk), 0, stream_,
                       nBlk, A, xv, yv);
  }
  // w_local = Cinv * in_local  (pointers offset to the local shard)
  void applyCinv(const T* in, T* out) {
    blockMatVec<PD, 0>(npL_, dHllInv_ + (int64_t)ptLo_ * PP,
                       in + (int64_t)ptLo_ * PD, out + (int64_t)ptLo_ * PD);
  }
  // The kernels of one PCG iteration.  Resolved once, at the first solve, and
  // never written again: the captured PCG graph bakes in what it selects.
  PcgPlan resolvePlan() {
    const SchurPath tuned = chooseSchurPath();
    // MEGBA_TUNE_VERBOSE reports the tuner's choice (the tests read it
    // back), also when MEGBA_FUSED then overrides the product
    if (knobs_.tuneVerbose)
      fprintf(stderr, "# schur path: %s\n",
              tuned == SchurPath::Lds            ? "lds"
              : tuned == SchurPath::LdsRecompute ? "lds-recompute"
              : tuned == SchurPath::FusedEtx     ? "fused-etx"
                                                 : "separate");
    if (knobs_.tuneVerbose && tuned == SchurPath::LdsRecompute)
      fprintf(stderr, "# schur recompute gather: %s\n",
              rcStaged_ ? "staged" : "per-lane");
    PcgPlan plan;
    plan.path = knobs_.fused ? SchurPath::OnePass : tuned;
    plan.rotatedBody = !knobs_.noPcgFuse;
    // only the explicit separate-pass kSpmvEtx reads the unpadded vector
    plan.productReadsPad = implicit_ || plan.path != SchurPath::Separate;
    // row reduce, B-apply and dot in one kernel when nothing sits between
    // them: LDS path, no long-run finishers, no collective
    plan.mergeReduceBApply = plan.rotatedBody &&
                             (plan.path == SchurPath::Lds ||
                              plan.path == SchurPath::LdsRecompute) &&
                             nLongPts_ == 0 && allreduceIsNoop();
    return plan;
  }
  // One-time measured choice between the fused E^T x + Cinv window kernel
  // and the separate-pass pipeline: which wins is problem-dependent
  // (Venice wins fused in BOTH dtypes, final13682-fp32 wins separate —
  // profiles/r02_gather_bands.md Exp 6), so unless an env override is
  // set, time 3 local Schur applies each way on the real data and keep
  // the faster.  Only the LOCAL part runs (no collective), so ranks may
  // even pick differently without breaking lockstep: q partials are
  // per-rank inputs to the allreduce either way.
  //
  // The LDS single-pass apply (schurFusedLdsEcE) is a third candidate when
  // the camera vector fits the per-workgroup LDS limit (setupSchurLds).
  // MEGBA_SCHUR_LDS forces it on when eligible (also the way problems below
  // the tuning threshold reach it), MEGBA_NO_SCHUR_LDS removes it; forcing
  // one of the two-pass variants (MEGBA_NO_ETXFUSE / MEGBA_ETXFUSE) leaves
  // it out as well.
  //
  // The recomputed-J form of the LDS apply (SchurPath::LdsRecompute) is a
  // fourth candidate under its own eligibility (setupSchurLds) and the same
  // rules: MEGBA_SCHUR_RECOMPUTE forces it when eligible and then wins over
  // MEGBA_SCHUR_LDS, MEGBA_NO_SCHUR_RECOMPUTE removes it, and where it is
  // not eligible its forcing knob changes nothing.
  SchurPath chooseSchurPath() {
    const SchurPath twoPass =
        knobs_.noEtxFuse ? SchurPath::Separate : SchurPath::FusedEtx;
    const bool twoPassForced = knobs_.noEtxFuse || knobs_.etxFuse;
    const bool ldsForced = knobs_.schurLds;
    const bool rcForced = knobs_.schurRecompute;
    const bool tuning = !twoPassForced && nL_ >= 200000;
    bool lds = ldsEligible_ && (!twoPassForced || ldsForced);
    bool rc = rcEligible_ && (rcForced || (tuning && !ldsForced));
    if (rc) {
      // first launch outside any graph capture, as for the LDS apply below
      (void)hipGetLastError();
      schurFusedLdsEcE({dDeltaX_, false}, dQ_, false, /*recompute=*/true);
      if (hipGetLastError() != hipSuccess) rc = false;
    }
    if (rcForced && rc) return SchurPath::LdsRecompute;
    // nothing to choose: a forced two-pass variant, or the launch-noise
    // regime, where the default stays
    if (!ldsForced && !tuning) return twoPass;
    if (lds) {
      // first launch happens here, outside any graph capture: a launch the
      // runtime refuses (LDS size) drops the candidate instead of failing
      (void)hipGetLastError();
      schurFusedLdsEcE({dDeltaX_, false}, dQ_);
      if (hipGetLastError() != hipSuccess) lds = false;
    }
    if (ldsForced) return lds ? SchurPath::Lds : twoPass;
    hipEvent_t ev[2];
    HIP_CHECK(hipEventCreate(&ev[0]));
    HIP_CHECK(hipEventCreate(&ev[1]));
    float ms[4] = {0, 0, 0, 0};
    const SchurPath variants[4] = {SchurPath::FusedEtx, SchurPath::Separate,
                                   SchurPath::Lds, SchurPath::LdsRecompute};
    const bool timed[4] = {true, true, lds, rc};
    for (int variant = 0; variant < 4; ++variant) {
      if (!timed[variant]) continue;
      // warm-up then timed triple (dQ_/dWPad_/dTemp_ are scratch)
      localSchurEcE(variants[variant], {dDeltaX_, false}, dQ_);
      HIP_CHECK(hipEventRecord(ev[0], stream_));
      for (int k = 0; k < 3; ++k)
        localSchurEcE(variants[variant], {dDeltaX_, false}, dQ_);
      HIP_CHECK(hipEventRecord(ev[1], stream_));
      HIP_CHECK(hipEventSynchronize(ev[1]));
      HIP_CHECK(hipEventElapsedTime(&ms[variant], ev[0], ev[1]));
    }
    const int best2 = ms[0] <= ms[1] ? 0 : 1;
    const bool useLds = lds && ms[2] < ms[best2];
    if (knobs_.tuneVerbose)
      fprintf(stderr,
              "# schur autotune: fused-etx %.3f ms, separate %.3f ms, "
              "lds %.3f ms (3 applies each)\n",
              ms[0], ms[1], lds ? ms[2] : -1.0f);
    if (knobs_.tuneVerbose && rc)
      fprintf(stderr, "# schur recompute: %.3f ms (3 applies)\n", ms[3]);
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    // the recompute candidate only when it is the fastest of all
    if (rc && ms[3] < ms[best2] && (!lds || ms[3] < ms[2]))
      return SchurPath::LdsRecompute;
    return useLds ? SchurPath::Lds : variants[best2];
  }

  // f(impTag, infoTag) with this engine's (implicit_, hasInfo_) as
  // integral_constant tags: the three combinations the product kernels are
  // instantiated for (the explicit Hpl already carries the weights).
  template <typename F>
  decltype(auto) dispatchMode(F&& f) const {
    using TrueT = std::integral_constant<bool, true>;
    using FalseT = std::integral_constant<bool, false>;
    if (implicit_ && hasInfo_) return f(TrueT{}, TrueT{});
    if (implicit_) return f(TrueT{}, FalseT{});
    return f(FalseT{}, FalseT{});
  }
  // Kernel handle of the kSchurFusedLds instance this engine launches.
  const void* schurLdsKernel() const {
    return dispatchMode([](auto im, auto hi) {
      return (const void*)kSchurFusedLds<T, CD, PD, RD, decltype(im)::value,
                                         decltype(hi)::value>;
    });
  }
  // The same for kSchurFusedLdsRc, which exists for the BAL dims only.
  // staged: the instance that gathers the camera rows through LDS tiles.
  const void* schurLdsRcKernel(bool staged) const {
    if constexpr (kBalDims)
      return dispatchBool(hasInfo_, [&](auto infoTag) {
        constexpr bool HI = decltype(infoTag)::value;
        return staged ? (const void*)kSchurFusedLdsRc<T, HI, true>
                      : (const void*)kSchurFusedLdsRc<T, HI, false>;
      });
    return nullptr;
  }
  // Dynamic LDS of kSchurFusedLdsRc: the accumulators, and for the staged
  // instance one tile per wave behind them.
  size_t rcLdsBytes(bool staged) const {
    return staged ? (size_t)rcStagedLdsBytes(nc_, (int)sizeof(T),
                                             rcThreads_ / 64)
                  : (size_t)nc_ * sizeof(T);
  }
  void launchSchurLdsRc() {
    [[maybe_unused]] const PadDst d = padDstFor(SchurPath::LdsRecompute);
    if constexpr (kBalDims)
      dispatchBool(hasInfo_, [&](auto infoTag) {
        dispatchBool(rcStaged_, [&](auto stagedTag) {
          hipLaunchKernelGGL(
              (kSchurFusedLdsRc<T, decltype(infoTag)::value,
                                decltype(stagedTag)::value>),
              dim3(numCU_), dim3(rcThreads_), rcLdsBytes(rcStaged_), stream_,
              nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_, dPtOf_,
              dCamRow_, rcCamStride(), d.p + d.off, d.stride, dPtAcc_,
              dCamFixed_, dPtFixed_,
              (const T* const*)dJSlots_, dInfo_, lossKind_, lossD2_, dHllInv_,
              dTemp_, (int)nc_, dLdsRows_);
        });
      });
  }
  // Grid of the one-wave-per-window kernels (4 waves per block).
  static int windowGrid(int nWin) {
    const int g = (nWin + 3) / 4 < 8192 ? (nWin + 3) / 4 : 8192;
    return g < 1 ? 1 : g;
  }
  // Input vector of a product, and whether the path's padded copy of it
  // (padDstFor) is already written (the rotated PCG body's kBetaPPad does).
  struct XIn {
    const T* v;
    bool padReady;
  };
  // Grid of the LDS row reduce = number of p.q partials it can write.
  int ldsReduceGrid() const { return (int)((nc_ + 63) / 64); }
  // Grid of kBApplyDot = number of p.q partials it writes.
  int bApplyDotGrid() const { return gridFor(nc_); }
  // Where the padded copy of a product's input goes: the XP-stride vector
  // dXPad_, or for the staged recompute path the x columns of its camera row
  // table.
  struct PadDst {
    T* p;
    int stride, off;
  };
  PadDst xPadDst() const { return {dXPad_, PkJ::XP, 0}; }
  PadDst padDstFor(SchurPath path) const {
    if (path == SchurPath::LdsRecompute && rcStaged_)
      return {dCamRow_, RcRow<T>::LEN, kRcXOff};
    return xPadDst();
  }
  // Row stride of the recompute path's camera table: whole 64-byte-aligned
  // rows for the staged gather; the per-lane instance keeps bare
  // balCameraPart rows and reads x from dXPad_ (measured faster for its
  // loads than the wide rows, profiles/r09_rc_staged_gather.md).
  int rcCamStride() const { return rcStaged_ ? RcRow<T>::LEN : kBalCamRow; }
  void padX(const T* x, PadDst d) {
    hipLaunchKernelGGL((kPadX<T, CD>), dim3(gridFor(ncam_)), dim3(kBlk), 0,
                       stream_, ncam_, x, d.p, d.stride, d.off);
  }
  // Common start of the window passes: the padded copy of x where the path
  // reads it unless it is ready, and a zeroed temp when >64-edge runs will
  // add partials to it.  The long-run finishers read dXPad_ on every path,
  // so with such runs the staged recompute path fills that as well.
  void windowPrologue(XIn x, SchurPath path) {
    if (!x.padReady) padX(x.v, padDstFor(path));
    if (nLongPts_ > 0 && path == SchurPath::LdsRecompute && rcStaged_)
      padX(x.v, xPadDst());
    if (nLongPts_ > 0)
      hipLaunchKernelGGL(kZeroRange<T>, dim3(gridFor((int64_t)npL_ * PD)),
                         dim3(kBlk), 0, stream_, dTemp_ + (int64_t)ptLo_ * PD,
                         (int64_t)npL_ * PD);
  }
  // w_p = Cinv temp_p for the >64-edge points, into w at the given stride.
  void longRunW(T* w, int stride) {
    if (nLongPts_ > 0)
      hipLaunchKernelGGL((kFusedLongW<T, PD>), dim3(gridFor(nLongPts_)),
                         dim3(kBlk), 0, stream_, nLongPts_, dLongPts_,
                         dHllInv_, dTemp_, w, stride);
  }
  // Finish the flagged windows of a single-pass apply on the global output.
  void finishLongRuns(T* out) {
    if (nLongPts_ == 0) return;
    longRunW(dW_, PD);
    dispatchMode([&](auto impTag, auto infoTag) {
      constexpr bool IM = decltype(impTag)::value;
      constexpr bool HI = decltype(infoTag)::value;
      hipLaunchKernelGGL((kFusedLongScatter<T, CD, PD, RD, IM, HI>),
                         dim3(windowGrid(nFlagWins_)), dim3(256), 0, stream_,
                         nFlagWins_, dFlagWins_, dWinLo_, dWinHi_, nL_,
                         dCamOf_, dPtOf_, dHpl_, (const T* const*)dJSlots_,
                         dInfo_, lossKind_, lossD2_, dXPad_, dW_, out);
    });
  }
  // Eligibility of the LDS single-pass apply: the camera vector must fit
  // the runtime's per-workgroup LDS limit (MEGBA_SCHUR_LDS_MAX_BYTES lowers
  // it for testing) and the kernel's dynamic-LDS attribute must be raised
  // once, before any graph capture.  Any failure just leaves the existing
  // paths in charge.
  void setupSchurLds(int deviceIndex) {
    ldsEligible_ = false;
    if (knobs_.noSchurLds || nWin_ == 0) return;
    int cus = 0, lim = 0, optin = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              deviceIndex) != hipSuccess ||
        hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock,
                              deviceIndex) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin,
                              deviceIndex) != hipSuccess) {
      (void)hipGetLastError();
      optin = 0;
    }
    int64_t limit = lim > optin ? lim : optin;
    if (knobs_.schurLdsMaxBytes && *knobs_.schurLdsMaxBytes < limit)
      limit = *knobs_.schurLdsMaxBytes;
    const int64_t need = nc_ * (int64_t)sizeof(T);
    if (cus < 1 || need > limit) return;
    if (hipFuncSetAttribute(schurLdsKernel(),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)need) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    numCU_ = cus;
    if (knobs_.schurLdsThreads) {
      // development knob: workgroup size variants (multiple of 64, <=1024)
      const int n = *knobs_.schurLdsThreads / 64 * 64;
      if (n >= 64 && n <= 1024) ldsThreads_ = n;
    }
    dLdsRows_ = dalloc<T>((int64_t)numCU_ * nc_);
    ldsEligible_ = true;
    // Recomputed-J form: built-in BAL residual, implicit mode.  Its buffers
    // are allocated here, once, so the captured PCG graph sees stable
    // pointers; acceptForward fills them.
    if constexpr (kBalDims) {
      if (!implicit_ || customFwd_ || knobs_.noSchurRecompute) return;
      if (hipFuncSetAttribute(schurLdsRcKernel(false),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)need) != hipSuccess) {
        (void)hipGetLastError();
        return;
      }
      // its own workgroup size: 512 measured faster than 1024 and is the
      // kernel's launch bound; the development knob applies up to that
      rcThreads_ = ldsThreads_ < kLdsRcMaxThreads && knobs_.schurLdsThreads
                       ? ldsThreads_
                       : kLdsRcMaxThreads;
      // the row table's pad columns are zeroed here and never written again
      dCamRow_ = dalloc<T>((int64_t)ncam_ * RcRow<T>::LEN);
      dPtAcc_ = dalloc<T>((int64_t)npt_ * 4);
      HIP_CHECK(hipMemsetAsync(dCamRow_, 0,
                               (int64_t)ncam_ * RcRow<T>::LEN * sizeof(T),
                               stream_));
      HIP_CHECK(hipMemsetAsync(dPtAcc_, 0, (int64_t)npt_ * 4 * sizeof(T),
                               stream_));
      rcEligible_ = true;
      // Staged gather: the per-wave tiles must fit behind the accumulators
      // (MEGBA_NO_RC_STAGE takes it out); otherwise the per-lane instance
      // runs and nothing else changes.
      const int64_t stagedNeed = (int64_t)rcLdsBytes(true);
      if (!knobs_.noRcStage && stagedNeed <= limit) {
        if (hipFuncSetAttribute(schurLdsRcKernel(true),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)stagedNeed) == hipSuccess)
          rcStaged_ = true;
        else
          (void)hipGetLastError();
      }
    }
  }

  // out = E Cinv E^T x (local part) in one pass over the primary-sorted J
  // with a per-workgroup LDS accumulator; out is fully overwritten.  With
  // bApplyDot the row reduce carries on to out = HppD x - out and the x.out
  // partials (dPartQ_), which needs nLongPts_ == 0.
  // With recompute the window kernel is kSchurFusedLdsRc, which rebuilds the
  // implicit edge from the accepted snapshot instead of reading dJPk_.
  void schurFusedLdsEcE(XIn x, T* out, bool bApplyDot = false,
                        bool recompute = false) {
    windowPrologue(x, recompute ? SchurPath::LdsRecompute : SchurPath::Lds);
    const size_t ldsBytes = (size_t)nc_ * sizeof(T);
    if (recompute)
      launchSchurLdsRc();
    else
      dispatchMode([&](auto impTag, auto infoTag) {
        constexpr bool IM = decltype(impTag)::value;
        constexpr bool HI = decltype(infoTag)::value;
        hipLaunchKernelGGL((kSchurFusedLds<T, CD, PD, RD, IM, HI>),
                           dim3(numCU_), dim3(ldsThreads_), ldsBytes, stream_,
                           nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_,
                           dPtOf_, dHpl_, dJPk_, (const T* const*)dJSlots_,
                           dInfo_, lossKind_, lossD2_, dXPad_, dHllInv_,
                           dTemp_, (int)nc_, dLdsRows_);
      });
    if (bApplyDot) {
      hipLaunchKernelGGL((kLdsReduceBApplyDot<T, CD>), dim3(ldsReduceGrid()),
                         dim3(64 * kLdsRedWaves), 0, stream_, numCU_, (int)nc_,
                         dLdsRows_, dHppD_, x.v, out, dPartQ_);
      return;
    }
    hipLaunchKernelGGL(kLdsRowsReduce<T>, dim3(ldsReduceGrid()),
                       dim3(64 * kLdsRedWaves), 0, stream_, numCU_, (int)nc_,
                       dLdsRows_, out);
    finishLongRuns(out);
  }

  // local (collective-free) E Cinv E^T x into out on the given path: one of
  // the tuner's four candidates (schurApply launches OnePass itself)
  void localSchurEcE(SchurPath path, XIn x, T* out) {
    switch (path) {
      case SchurPath::Lds:
        schurFusedLdsEcE(x, out);
        break;
      case SchurPath::LdsRecompute:
        schurFusedLdsEcE(x, out, false, /*recompute=*/true);
        break;
      case SchurPath::FusedEtx:
        etxCinv(x);
        spmvEx(dWPad_, out);
        break;
      case SchurPath::Separate:
        spmvEtx(x, dTemp_);
        cinvThenEx(dTemp_, out);
        break;
      case SchurPath::OnePass:
        MEGBA_CHECK(false, "OnePass is not a tuning candidate");
    }
  }

  // w = Cinv in, then out += E w.  w is stored 4-padded so the E-side
  // gather is a single aligned vector load per edge (both modes).
  void cinvThenEx(const T* in, T* out) {
    hipLaunchKernelGGL((kCinvPad<T, PD>), dim3(gridFor(npL_)), dim3(kBlk),
                       0, stream_, npL_, dHllInv_ + (int64_t)ptLo_ * PP,
                       in + (int64_t)ptLo_ * PD,
                       dWPad_ + (int64_t)ptLo_ * 4);
    spmvEx(dWPad_, out);
  }
  void spmvEtx(XIn x, T* out) {
    hipLaunchKernelGGL(kZeroRange<T>, dim3(gridFor((int64_t)npL_ * PD)),
                       dim3(kBlk), 0, stream_, out + (int64_t)ptLo_ * PD,
                       (int64_t)npL_ * PD);
    if (!implicit_) {
      hipLaunchKernelGGL((kSpmvEtx<T, CD, PD, RD>), dim3(gridFor(nL_)),
                         dim3(kBlk), 0, stream_, nL_, dCamOf_, dPtOf_, dHpl_,
                         x.v, out);
      return;
    }
    // 16B-aligned padded copy of x: the per-edge camera gather becomes
    // XP/VEC vector loads instead of CD divergent scalar loads.
    if (!x.padReady) padX(x.v, xPadDst());
    dispatchMode([&](auto, auto infoTag) {
      constexpr bool HI = decltype(infoTag)::value;
      const auto kernel = knobs_.etxAtomic
                              ? kSpmvEtxPkAtomic<T, CD, PD, RD, HI>
                              : kSpmvEtxPk<T, CD, PD, RD, HI>;
      hipLaunchKernelGGL(kernel, dim3(gridFor(nL_)), dim3(kBlk), 0, stream_,
                         nL_, dCamOf_, dPtOf_, dJPk_,
                         (const T* const*)dJSlots_, dInfo_, lossKind_,
                         lossD2_, dXPad_, out);
    });
  }
  void spmvEx(const T* wv, T* out) {
    HIP_CHECK(hipMemsetAsync(out, 0, nc_ * sizeof(T), stream_));
    if (implicit_) {
      if (nChunks_ == 0) return;
      hipLaunchKernelGGL((kSpmvExPk<T, CD, PD, RD>), dim3(nChunks_),
                         dim3(64), 0, stream_, nChunks_, dChCam_, dChLo_,
                         dChHi_, dPtOfCam_, dJCamPk_, nL_, wv, out);
      return;
    }
    if (nChunks_ > 0)
      hipLaunchKernelGGL((kSpmvEx<T, CD, PD>), dim3(nChunks_), dim3(64), 0,
                         stream_, nChunks_, dChCam_, dChLo_, dChHi_,
                         dPtOfCam_, dHplCam_, nL_, wv, out);
  }
  // One full PCG iteration (captured as a hipGraph when possible).
  // vs round 1: the p^T q dot partial is fused into the B-apply, the
  // two-deep x backup rotation is fused into kUpdateXR, and the standalone
  // kRedPartial pass + dXBakPrev memcpy are gone (~2 launches + one full
  // read pass over p,q per iteration — part of the N=8 constant term,
  // PLAN_r02 item 3).
  void pcgBody() {
    if (plan_->rotatedBody) {
      pcgBodyRotated();
      return;
    }
    const int rhoGrid = gridFor(nc_) < kRedBlocks ? gridFor(nc_) : kRedBlocks;
    hipLaunchKernelGGL((kPrecondRho<T, CD>), dim3(rhoGrid), dim3(kBlk), 0,
                       stream_, ncam_, dHppInv_, dRr_, dZ_, dPart_);
    hipLaunchKernelGGL(kXpbySBeta<T>, dim3(gridFor(nc_)), dim3(kBlk), 0,
                       stream_, nc_, dZ_, dPart_, rhoGrid, slotRhoPrev(),
                       slotRho(), dP_);
    const int nPartQ = schurApply({dP_, false}, dQ_, /*withDot=*/true);
    hipLaunchKernelGGL(kUpdateXRAlpha<T>, dim3(gridFor(nc_)), dim3(kBlk), 0,
                       stream_, nc_, dPart_, rhoGrid, dPartQ_, nPartQ,
                       slotRhoPrev(), dP_, dQ_, dDeltaX_, dXBak_, dXBakPrev_,
                       dRr_);
  }

  // Blocks of kUpdateXRPrecond (kBlk / CD whole cameras each) = number of
  // rho partials in the rotated body.
  int precondGrid() const {
    constexpr int CPB = kBlk / CD;
    return ncam_ > 0 ? (ncam_ + CPB - 1) / CPB : 1;
  }
  // The rotated body (default; MEGBA_NO_PCG_FUSE=1 keeps the one above).
  // z and the rho partials of the current residual already exist: from the
  // kPrecondRho before the loop, or from the previous body's last kernel.
  //   A  kBetaPPad:         rho -> slotRho(), beta, p = z + beta p, padded p
  //                         (padDstFor: dXPad_ or the camera row table)
  //      product            (skips its own kPadX)
  //   B  kLdsReduceBApplyDot when eligible, else reduce .. kBApplyDot
  //   C  kUpdateXRPrecond:  alpha, rho -> slotRhoPrev(), x/xBak/xBakPrev/r,
  //                         z = Binv r_new, next rho partials
  void pcgBodyRotated() {
    const int nbR = precondGrid();
    if (plan_->productReadsPad) {
      const PadDst d = padDstFor(plan_->path);
      hipLaunchKernelGGL((kBetaPPad<T, CD>),
                         dim3(gridFor((int64_t)ncam_ * PkJ::XP)), dim3(kBlk),
                         0, stream_, ncam_, dZ_, dPart_, nbR, slotRhoPrev(),
                         slotRho(), dP_, d.p, d.stride, d.off);
    } else {
      hipLaunchKernelGGL(kXpbySBeta<T>, dim3(gridFor(nc_)), dim3(kBlk), 0,
                         stream_, nc_, dZ_, dPart_, nbR, slotRhoPrev(),
                         slotRho(), dP_);
    }
    const int nPartQ =
        schurApply({dP_, plan_->productReadsPad}, dQ_, /*withDot=*/true);
    hipLaunchKernelGGL((kUpdateXRPrecond<T, CD>), dim3(nbR), dim3(kBlk), 0,
                       stream_, ncam_, slotRho(), dPartQ_, nPartQ,
                       slotRhoPrev(), dP_, dQ_, dDeltaX_, dXBak_, dXBakPrev_,
                       dRr_, dHppInv_, dZ_, dPart_);
  }

  // Capture the PCG body as a hipGraph, once.  The implicit path reads the
  // double-buffered accepted J set through device pointer slots (dJSlots_),
  // so accept-time buffer flips never invalidate the graph.  Multi-rank
  // RCCL collectives are captured too (ncclAllReduce is stream-ordered on
  // stream_); any capture failure falls back to the eager path permanently.
  void ensurePcgGraph() {
    if (pcgGraphExec_ || pcgGraphFailed_ || knobs_.noGraph) return;
    // host-callback collectives (gloo testing fallback) cannot be captured
    if (world_ > 1 && !hasComm_) return;
    sync();
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) !=
        hipSuccess) {
      pcgGraphFailed_ = true;
      (void)hipGetLastError();
      return;
    }
    bool ok = true;
    try {
      pcgBody();
    } catch (...) {
      ok = false;
    }
    if (hipStreamEndCapture(stream_, &graph) != hipSuccess || !ok || !graph) {
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      pcgGraphFailed_ = true;
      return;
    }
    hipGraphExec_t exec = nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
      (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      pcgGraphFailed_ = true;
      return;
    }
    (void)hipGraphDestroy(graph);
    pcgGraphExec_ = exec;
  }

  // out = E Cinv E^T x in one fused pass (see kSchurFused; measured
  // negative, kept env-gated).
  void schurFusedEcE(XIn x, T* out) {
    HIP_CHECK(hipMemsetAsync(out, 0, nc_ * sizeof(T), stream_));
    windowPrologue(x, SchurPath::OnePass);
    dispatchMode([&](auto impTag, auto infoTag) {
      constexpr bool IM = decltype(impTag)::value;
      constexpr bool HI = decltype(infoTag)::value;
      hipLaunchKernelGGL((kSchurFused<T, CD, PD, RD, IM, HI>),
                         dim3(windowGrid(nWin_)), dim3(256), 0, stream_,
                         nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_,
                         dPtOf_, dHpl_, (const T* const*)dJSlots_, dInfo_,
                         lossKind_, lossD2_, dXPad_, dHllInv_, dTemp_, out);
    });
    finishLongRuns(out);
  }

  // w = Cinv E^T x into the 4-padded w vector, one fused window pass
  // (default path; see kEtxCinvFused).
  void etxCinv(XIn x) {
    windowPrologue(x, SchurPath::FusedEtx);
    dispatchMode([&](auto impTag, auto infoTag) {
      constexpr bool IM = decltype(impTag)::value;
      constexpr bool HI = decltype(infoTag)::value;
      hipLaunchKernelGGL((kEtxCinvFused<T, CD, PD, RD, IM, HI>),
                         dim3(windowGrid(nWin_)), dim3(256), 0, stream_,
                         nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_,
                         dPtOf_, dHpl_, (const T* const*)dJSlots_, dInfo_,
                         lossKind_, lossD2_, dXPad_, dHllInv_, dTemp_,
                         dWPad_);
    });
    longRunW(dWPad_, 4);
  }

  // q = S x = HppD x - E Cinv E^T x  (ONE CD*ncam allreduce; the reference's
  // site A4 needed an additional 3*npt allreduce here).  withDot fuses the
  // x^T q dot partials into the B-apply pass (used by the PCG body) and
  // returns how many partials it wrote to dPartQ_ (0 without withDot).
  int schurApply(XIn x, T* q, bool withDot) {
    if (withDot && plan_->mergeReduceBApply) {
      schurFusedLdsEcE(x, q, /*bApplyDot=*/true,
                       plan_->path == SchurPath::LdsRecompute);
      return ldsReduceGrid();
    }
    if (plan_->path == SchurPath::OnePass)
      schurFusedEcE(x, q);
    else
      localSchurEcE(plan_->path, x, q);
    allreduce(q, nc_, ncclSum);
    if (withDot) {
      hipLaunchKernelGGL((kBApplyDot<T, CD>), dim3(bApplyDotGrid()),
                         dim3(kBlk), 0, stream_, ncam_, dHppD_, x.v, q,
                         dPartQ_);
      return bApplyDotGrid();
    }
    blockMatVec<CD, 1>(ncam_, dHppD_, x.v, q);
    return 0;
  }

  hipStream_t stream_{};
  ncclComm_t comm_{};
  bool hasComm_ = false;
  // MEGBA_* environment knobs, fixed at construction (knobs.hpp)
  const GpuKnobs knobs_;
  // Kernels of one PCG iteration, resolved at the first solve (resolvePlan)
  std::optional<PcgPlan> plan_;
  CustomForward<T> customFwd_;
  HostAllreduce<T> hostAr_;
  HostAllreduce<double> hostArD_;
  int rank_, world_, ncam_, npt_;
  int ptLo_ = 0, ptHi_ = 0, npL_ = 0;
  int64_t e0_ = 0, e1_ = 0, nL_ = 0, nc_ = 0, np_ = 0, dim_ = 0;
  bool hasInfo_ = false;
  bool analytical_ = false;
  bool implicit_ = false;
  int lossKind_ = 0;
  T lossD2_ = T(1);
  // LDS single-pass Schur apply (kSchurFusedLds): eligible when the camera
  // vector fits the per-workgroup LDS limit (setupSchurLds, construction);
  // chosen by chooseSchurPath or forced with MEGBA_SCHUR_LDS.
  bool ldsEligible_ = false;
  int numCU_ = 0;
  int ldsThreads_ = 1024;
  T* dLdsRows_{};  // [numCU_][nc_] per-workgroup flush rows
  // Recomputed-J LDS apply (kSchurFusedLdsRc): eligibility and the snapshot
  // of the accepted linearisation point that acceptForward refreshes.
  bool rcEligible_ = false;
  int rcThreads_ = kLdsRcMaxThreads;
  bool rcStaged_ = false;  // the LDS-staged gather instance runs
  // [ncam_][RcRow<T>::LEN] camera row table (rc_tile.hpp): balCameraPart
  // row, then the product's padded input x, then zeros
  T* dCamRow_{};
  T* dPtAcc_{};   // [npt_][4] accepted points, 4-padded, global point id
  int nWin_ = 0, nFlagWins_ = 0, nLongPts_ = 0;
  int64_t* dWinLo_{};
  int64_t* dWinHi_{};
  unsigned char* dWinFlag_{};
  int* dFlagWins_{};
  int* dLongPts_{};
  DevPrior camPr_, ctrPr_, ptPr_;  // camera parameter / centre / point priors
  bool hasPriors_ = false;
  int cur_ = 0;
  bool freshCur_ = false;  // current r/J buffers hold the last forward()
  int nChunks_ = 0;
  int *dCamOf_{}, *dPtOf_{}, *dChCam_{}, *dChLo_{}, *dChHi_{}, *dFail_{};
  int *dCamPos_{}, *dPtOfCam_{};
  T *dMeas_{}, *dInfo_{}, *dLeaf_{}, *dMeasSplit_{}, *dIntr_{};
  unsigned char *dCamFixed_{}, *dPtFixed_{};
  T *dParams_{}, *dParamsBak_{};
  T *dR_[2]{}, *dJc_[2]{}, *dJp_[2]{};
  T *dHpp_{}, *dHll_{}, *dHpl_{}, *dHplCam_{}, *dSlab_{}, *dG_{}, *dGBak_{};
  T *dJPk_{}, *dJCamPk_{};  // implicit: packed [J..] vector groups
  T* dWPad_{};              // 4-padded w for the E-side gather
  T* dXPad_{};              // implicit: XP-padded x for the E^T-side gather
  T *dHppD_{}, *dHllD_{}, *dHppInv_{}, *dHllInv_{};
  T *dDeltaX_{}, *dDeltaXBak_{};
  T *dP_{}, *dRr_{}, *dZ_{}, *dQ_{}, *dV_{}, *dW_{}, *dTemp_{}, *dXBak_{},
      *dXBakPrev_{}, *dPtMerge_{};
  hipGraphExec_t pcgGraphExec_{};
  bool pcgGraphFailed_ = false;
  const T** dJSlots_{};  // device slots: accepted {Jc, Jp, r} pointers
  int partCap_ = kRedBlocks;
  double* dPart_{};
  double* dPartQ_{};
  double* hScalar_{};
  std::vector<void*> allocs_;
};

// Per-dims factory, explicitly instantiated by the gpu_dims_*.hip TUs.
template <typename T, int CD, int PD, int RD>
std::unique_ptr<Engine<T>> makeGpuEngineDims(const BAProblemHost& prob,
                                             const ProblemIndex& ix,
                                             const ProblemOption& opt,
                                             const std::string& rcclId,
                                             CustomForward<T> customForward,
                                             HostAllreduce<T> hostAllreduce,
                                             HostAllreduce<double> hostArD) {
  return std::make_unique<GpuEngine<T, CD, PD, RD>>(
      prob, ix, opt, rcclId, std::move(customForward),
      std::move(hostAllreduce), std::move(hostArD));
}

}  // namespace megba
