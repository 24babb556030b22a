// MI355X (gfx950) engine: HIP kernels + host orchestration + RCCL collectives.
//
// Kernel / distribution design (MI355X-first redesign, not a port):
//  * Observations are (point, camera)-sorted and partitioned on POINT
//    boundaries: each rank owns its points outright, so the whole point side
//    (Hll, g_p, Cinv, E^T x, back-substitution) is communication-free and
//    the only per-PCG-iteration collective is an allreduce of the replicated
//    camera vector (9*ncam = 128 KB on Venice).  The reference replicates
//    the point side instead and allreduces 3*npt words (24 MB on Venice)
//    per iteration (its sites A1/A3-A6) — a ~190x traffic reduction sized
//    for xGMI's per-link ring bandwidth.
//  * Control-flow scalars (rho, p^T q, norms) use fixed-shape two-pass
//    deterministic reductions so every rank takes identical PCG branches.
// The fused forward kernel, the slab assembly, the packed layouts, the
// captured PCG body and the choice of the Schur product: docs/INTERNALS.md
// sections 4 to 6.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <optional>
#include <type_traits>
#include <utility>
#include <vector>

#include "../jv/jetvector.hpp"
#include "dense_chol.hpp"
#include "edge_ops.hpp"
#include "edge_tables.hpp"
#include "gpu_common.hpp"
#include "gpu_engine.hpp"
#include "kernels_assemble.hpp"
#include "kernels_batch.hpp"
#include "kernels_dense.hpp"
#include "kernels_forward.hpp"
#include "kernels_pcg.hpp"
#include "kernels_prior.hpp"
#include "kernels_product.hpp"
#include "knobs.hpp"
#include "schur_plan.hpp"

namespace megba {

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
    hCamFixed_ = prob.camFixed;
    hPtFixed_ = prob.ptFixed;
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
      copyD2D(dParamsBak_, dParams_, dim_);
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
    zero(dDeltaX_, dim_);
    zero(dDeltaXBak_, dim_);

    // PCG workspace.
    dP_ = dalloc<T>(nc_);
    dRr_ = dalloc<T>(nc_);
    dZ_ = dalloc<T>(nc_);
    dQ_ = dalloc<T>(nc_);
    dV_ = dalloc<T>(nc_);
    dXBak_ = dalloc<T>(nc_);
    dXBakPrev_ = dalloc<T>(nc_);
    zero(dXBak_, nc_);
    zero(dXBakPrev_, nc_);
    dW_ = dalloc<T>(np_);
    dTemp_ = dalloc<T>(np_);
    zero(dW_, np_);

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
      // dense Schur route: cam-sorted row range of every camera and the
      // primary edge range of every local point (uploaded at first use)
      hCamRow_.assign(ncam_ + 1, 0);
      for (int64_t e = 0; e < nL_; ++e) hCamRow_[ix.camOf[e0_ + e] + 1]++;
      for (int c = 0; c < ncam_; ++c) hCamRow_[c + 1] += hCamRow_[c];
      hPtRow_.resize(npL_ + 1);
      for (int q = 0; q <= npL_; ++q)
        hPtRow_[q] = ix.ptRowPtr[ptLo_ + q] - e0_;
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
    if (bb_.hRho) (void)hipHostFree(bb_.hRho);
    if (pcgGraphExec_) (void)hipGraphExecDestroy(pcgGraphExec_);
    freeDense();
    for (void* p : allocs_) (void)hipFree(p);
    if (hasComm_) (void)ncclCommDestroy(comm_);
    (void)hipStreamDestroy(stream_);
  }

  double forward() override {
    freshCur_ = true;
    if (customFwd_) return forwardCustom();
    zeroScalar();
    // `lanes` threads per observation; kForward alone takes the intrinsics
    const auto fwd = [&](auto kernel, int lanes, auto... intr) {
      launchN(kernel, nL_ * lanes, nL_, dCamOf_, dPtOf_, dParams_, ncam_,
              dMeas_, dCamFixed_, dPtFixed_, dR_[cur_], dJc_[cur_], dJp_[cur_],
              scalarPtr(), lossKind_, lossD2_, intr...);
    };
    // the analytical and value-share kernels exist for the BAL dims only
    // (the constructor refuses analytical_ on any other dims)
    bool launched = false;
    if constexpr (kBalDims) {
      launched = analytical_ || knobs_.fwdVS;
      if (analytical_)
        fwd(kForwardAnalytical<T>, 1);
      else if (knobs_.fwdVS)
        fwd(kForwardVS<T>, 4);
    }
    if (!launched) fwd(kForward<T, CD, PD, RD>, (GW + 2) / 3, dIntr_);
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
      launchN(kBalSnapshot<T>, (int64_t)ncam_ + npL_, ncam_, ptLo_, npL_,
              dParams_, dCamRow_, rcCamStride(), dPtAcc_);
  }

  // Point the device slots at the accepted (bak) buffer set.
  void updateJSlots() {
    const int bak = cur_ ^ 1;
    launch(kSetPtrSlots<T>, 1, 1, 0, dJSlots_, dJc_[bak], dJp_[bak], dR_[bak]);
  }

  double forwardCustom() {
    launchN(kGatherLeaves<T, CD, PD>, nL_, nL_, dCamOf_, dPtOf_, dParams_,
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
      launchN(kRepackRes<T, CD, PD, RD>, nL_, nL_, r, res[r].value->ptr,
              res[r].grad->ptr, dCamOf_, dPtOf_, dCamFixed_, dPtFixed_,
              dR_[cur_], dJc_[cur_], dJp_[cur_]);
    }
    if (lossKind_) {
      zeroScalar();
      launchN(kChi2Loss<T, RD>, nL_, nL_, dR_[cur_], lossKind_, lossD2_,
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
    zero(dHpp_, (int64_t)ncam_ * CC);
    zero(shard(dHll_, PP), (int64_t)npL_ * PP);
    zero(dG_, nc_);
    zero(shard(dG_ + nc_, PD), (int64_t)npL_ * PD);
    dispatchAssemble(bak);
    dispatchBool(weighted(), [&](auto weightedTag) {
      constexpr bool HI = decltype(weightedTag)::value;
      if (!implicit_)
        launchN(kFinalizeCam<T, CD, PD, RD, HI>, nL_, nL_, dSlab_, dHplCam_);
      else
        launchN(kFinalizeCamImpPk<T, CD, PD, RD, HI>, nL_, nL_, dSlab_,
                dJCamPk_);
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

  void backupParams() override { copyD2D(dParamsBak_, dParams_, dim_); }
  void rollbackParams() override { copyD2D(dParams_, dParamsBak_, dim_); }
  void backupGDx() override {
    copyD2D(dDeltaXBak_, dDeltaX_, dim_);
    copyD2D(dGBak_, dG_, dim_);
  }
  void rollbackGDx() override {
    copyD2D(dDeltaX_, dDeltaXBak_, dim_);
    copyD2D(dG_, dGBak_, dim_);
  }

  void processDiag(double region) override {
    const T f = T(1) + T(1) / (T)region;
    launchN(kDamp<T, CD>, (int64_t)ncam_ * CC, (int64_t)ncam_ * CC, dHpp_,
            dHppD_, f, dCamFixed_);
    launchN(kDamp<T, PD>, (int64_t)npL_ * PP, (int64_t)npL_ * PP,
            shard(dHll_, PP), shard(dHllD_, PP), f,
            dPtFixed_ ? dPtFixed_ + ptLo_ : nullptr);
  }

  // Block inverses (preconditioner replicated; Cinv on the local shard).
  void invertForSolve(const SolverOptionPCG& opt) {
    HIP_CHECK(hipMemsetAsync(dFail_, 0, 2 * sizeof(int), stream_));
    int fail[2] = {0, 0};
    invertBlocks(kInvert<T, CD>, kInvert<T, PD>, fail);
    if (opt.refuseJitter) {
      // point blocks are rank-local: agree on the outcome before raising
      double failed = fail[0] ? 1.0 : 0.0;
      if (world_ > 1) {
        launch(kSetScalar, 1, 1, 0, scalarPtr(), failed);
        failed = globalScalar(ncclMax);
      }
      MEGBA_CHECK(failed == 0.0,
                  "covariance: singular Hessian block (a plain block "
                  "inversion failed and the jitter retry is refused)");
    } else if (fail[0]) {
      invertBlocks(kInvertJitter<T, CD>, kInvertJitter<T, PD>, fail);
      MEGBA_CHECK(!fail[1], "singular Hessian block");
    }
  }

  int solveLinear(const SolverOptionPCG& opt) override {
    invertForSolve(opt);
    if (!plan_) plan_ = resolvePlan();
    const T* gc = dG_;
    const T* gp = dG_ + nc_;
    // v = gc/world - E Cinv gp  (partial, then the CD*ncam allreduce)
    cinvThenEx(gp, dV_);
    launchN(kVMake<T>, nc_, nc_, gc, T(1) / T(world_), dV_);
    allreduce(dV_, nc_, ncclSum);
    // Warm start: x = deltaX camera part (in place in dDeltaX_).
    T* x = dDeltaX_;
    schurApply({x, false}, dQ_, /*withDot=*/false);
    launchN(kSub<T>, nc_, nc_, dV_, dQ_, dRr_);

    // The loop body is value-uniform (beta/alpha live on-device; the first
    // iteration gets beta = rho/INF = 0 against a zeroed p), so it is
    // captured once as a hipGraph and replayed with ONE host interaction per
    // iteration: the rho readback that drives the reference's refuse/tol
    // control flow.  Refuse semantics are preserved with a two-deep x backup
    // (the body runs speculatively; on refuse x is restored to the value two
    // updates back, exactly what the reference's pre-update check restores).
    zero(dP_, nc_);
    launch(kSetScalar, 1, 1, 0, slotRhoPrev(), INFINITY);
    // Rotated body: the first z = Binv r and rho partials come from here,
    // every later one from the tail of the previous body.
    if (plan_->rotatedBody)
      launch(kPrecondRho<T, CD>, precondGrid(), kBlk, 0, ncam_, dHppInv_,
             dRr_, dZ_, dPart_);
    int n = 0;
    double rho = 0.0, rhoMin = INFINITY, rho0 = 0.0;
    bool done = false;
    relStopHit_ = false;
    ensurePcgGraph();
    // Fixed-work mode (tol<=0 with refuse disabled, the bench contract):
    // rho steers nothing, so skip the per-iteration host readback and
    // enqueue all maxIter bodies back-to-back — ONE host sync per solve
    // instead of one per iteration (the N=8 constant-term killer).
    const bool fixedWork =
        opt.tol <= 0.0 && opt.refuseRatio >= 1e29 && opt.relTol <= 0.0;
    if (fixedWork) {
      for (; n < opt.maxIter; ++n) {
        if (pcgGraphExec_) {
          HIP_CHECK(hipGraphLaunch(pcgGraphExec_, stream_));
          ++this->products_;  // the replayed body's schurApply
        } else {
          pcgBody();
        }
      }
    } else {
      while (!done && n < opt.maxIter) {
        if (pcgGraphExec_) {
          HIP_CHECK(hipGraphLaunch(pcgGraphExec_, stream_));
          ++this->products_;
        } else {
          pcgBody();
        }
        rho = readScalar(slotRho());
        if (rho > opt.refuseRatio * rhoMin) {
          copyD2D(x, dXBakPrev_, nc_);
          break;
        }
        rhoMin = rhoMin < rho ? rhoMin : rho;
        if (n == 0) rho0 = std::abs(rho);
        ++n;
        done = std::abs(rho) < opt.tol;
        if (opt.relTol > 0.0 && std::abs(rho) < opt.relTol * rho0)
          done = relStopHit_ = true;
      }
    }
    // Back-substitution: deltaX_p = Cinv (g_p - E^T x), fully local.
    spmvEtx({x, false}, dTemp_);
    launchN(kBackSub<T, PD>, npL_, npL_, shard(dHllInv_, PP), shard(gp, PD),
            shard(dTemp_, PD), shard(dDeltaX_ + nc_, PD));
    sync();
    return n;
  }

  double deltaXL2() override {
    return std::sqrt(reduceVec(dDeltaX_, ROp::SumSq));
  }
  double xL2() override { return std::sqrt(reduceVec(dParams_, ROp::SumSq)); }
  double gInf() override { return reduceVec(dG_, ROp::AbsMax); }

  void updateParams() override {
    launchN(kAddAssign<T>, nc_, nc_, dDeltaX_, dParams_);
    launchN(kAddAssign<T>, (int64_t)npL_ * PD, (int64_t)npL_ * PD,
            shard(dDeltaX_ + nc_, PD), shard(dParams_ + nc_, PD));
  }

  double rhoDenominator(double chi2Backup) override {
    const int bak = cur_ ^ 1;
    zeroScalar();
    if (implicit_) {
      // packed accepted J + padded deltaX camera vector
      padX(dDeltaX_, xPadDst());
      launchN(kRhoDenomPk<T, CD, PD, RD>, nL_, nL_, dCamOf_, dPtOf_, dR_[bak],
              dJPk_, dXPad_, dDeltaX_ + nc_, scalarPtr(), lossKind_, lossD2_);
    } else {
      launchN(kRhoDenom<T, CD, PD, RD>, nL_, nL_, dCamOf_, dPtOf_, dR_[bak],
              dJc_[bak], dJp_[bak], dDeltaX_, dDeltaX_ + nc_, scalarPtr(),
              lossKind_, lossD2_);
    }
    if (hasPriors_) priorRho();
    return globalScalar(ncclSum) - chi2Backup;
  }

  void getParams(double* cams, double* pts) override {
    downTo(cams, dParams_, nc_);
    const T* src = dParams_ + nc_;
    if (world_ > 1 && (hasComm_ || hostAr_)) {
      // point shards: zero the non-local entries, allreduce-sum.
      if (!dPtMerge_) dPtMerge_ = dalloc<T>(np_);
      zero(dPtMerge_, np_);
      copyD2D(shard(dPtMerge_, PD), shard(src, PD), (int64_t)npL_ * PD);
      allreduce(dPtMerge_, np_, ncclSum);
      sync();
      src = dPtMerge_;
    }
    downTo(pts, src, np_);
  }

  // ---- other right-hand sides (covariance.hpp) -----------------------------
  EngineShape shape() const override { return {ncam_, npt_, CD, PD}; }
  bool isFixed(bool camera, int id) const override {
    const std::vector<uint8_t>& f = camera ? hCamFixed_ : hPtFixed_;
    return !f.empty() && f[id] != 0;
  }
  void setUnitRhs(int64_t row) override {
    MEGBA_CHECK(row >= 0 && row < dim_, "unit right-hand side out of range");
    zero(dG_, dim_);
    zero(dDeltaX_, dim_);
    const bool mine = row < nc_ || (row >= nc_ + (int64_t)ptLo_ * PD &&
                                    row < nc_ + (int64_t)ptHi_ * PD);
    if (mine) launch(kSetElement<T>, 1, 1, 0, dG_, row, T(1));
  }
  void readDeltaXRows(const int64_t* rows, int n, double* out) override {
    if (n <= 0) return;
    for (int i = 0; i < n; ++i)
      MEGBA_CHECK(rows[i] >= 0 && rows[i] < dim_, "deltaX row out of range");
    if (n > rowCap_) {
      // a request is a few vertex blocks; grown buffers are freed with the rest
      rowCap_ = n;
      dRowIdx_ = dalloc<int64_t>(n);
      dRowOut_ = dalloc<double>(n);
    }
    HIP_CHECK(hipMemcpyAsync(dRowIdx_, rows, n * sizeof(int64_t),
                             hipMemcpyHostToDevice, stream_));
    // a replicated camera row counts once in the sum: rank 0 supplies it
    launchN(kGatherRows<T>, n, n, dDeltaX_, dRowIdx_, nc_,
            nc_ + (int64_t)ptLo_ * PD, nc_ + (int64_t)ptHi_ * PD, rank_ == 0,
            dRowOut_);
    if (hasComm_)
      RCCL_CHECK(ncclAllReduce(dRowOut_, dRowOut_, n, ncclDouble, ncclSum,
                               comm_, stream_));
    HIP_CHECK(hipMemcpyAsync(out, dRowOut_, n * sizeof(double),
                             hipMemcpyDeviceToHost, stream_));
    sync();
    if (hasComm_ || world_ == 1) return;
    if (hostArD_) {
      hostArD_(out, (size_t)n, 's');
    } else if (hostAr_) {
      std::vector<T> t(out, out + n);
      hostAr_(t.data(), (size_t)n, 's');
      for (int i = 0; i < n; ++i) out[i] = (double)t[i];
    }
  }
  void saveLinearState() override {
    if (!dGSaved_) {
      dGSaved_ = dalloc<T>(dim_);
      dDeltaXSaved_ = dalloc<T>(dim_);
    }
    copyD2D(dGSaved_, dG_, dim_);
    copyD2D(dDeltaXSaved_, dDeltaX_, dim_);
  }
  void restoreLinearState() override {
    MEGBA_CHECK(dGSaved_ != nullptr, "no saved linear state");
    copyD2D(dG_, dGSaved_, dim_);
    copyD2D(dDeltaX_, dDeltaXSaved_, dim_);
    sync();
  }
  bool relStopHit() const override { return relStopHit_; }

  // ---- batched multi-column PCG (kernels_batch.hpp) -------------------------
  // Compiled for fp64 only (all covariance() can reach), at the widths PD
  // and CD, for the implicit and the explicit product.
  int maxBatch() const override {
    return std::is_same<T, double>::value ? CD : 1;
  }

  void solveUnitBatch(const int64_t* rhsRows, int k, const SolverOptionPCG& opt,
                      const int64_t* readRows, int n, double* out, int* iters,
                      uint8_t* converged) override {
    // the batched loop has the relTol stop alone: no refuse rule and no
    // absolute tol, which is how computeCovariance solves
    const bool plain =
        opt.refuseRatio >= 1e29 && opt.tol <= 0.0 && opt.relTol > 0.0;
    if (k < 2 || k > maxBatch() || n <= 0 || !plain) {
      Engine<T>::solveUnitBatch(rhsRows, k, opt, readRows, n, out, iters,
                                converged);
      return;
    }
    if constexpr (std::is_same<T, double>::value) {
      for (int c = 0; c < k; ++c)
        MEGBA_CHECK(rhsRows[c] >= 0 && rhsRows[c] < dim_,
                    "unit right-hand side out of range");
      for (int i = 0; i < n; ++i)
        MEGBA_CHECK(readRows[i] >= 0 && readRows[i] < dim_,
                    "deltaX row out of range");
      dispatchWidth(k, [&](auto kb) {
        solveBatchW<decltype(kb)::value>(rhsRows, k, opt, readRows, n, out,
                                         iters, converged);
      });
    }
  }

  void schurApplyColumns(const double* X, int k, bool batched,
                         double* out) override {
    MEGBA_CHECK(k >= 1, "schur_apply: X needs at least one column");
    MEGBA_CHECK(!batched || (maxBatch() > 1 && k <= maxBatch()),
                "schur_apply: this engine has no batched product of that "
                "width (max_batch())");
    invertForSolve(SolverOptionPCG{});
    if (!batched) {
      if (!plan_) plan_ = resolvePlan();
      std::vector<T> col(nc_);
      for (int c = 0; c < k; ++c) {
        for (int64_t i = 0; i < nc_; ++i) col[i] = (T)X[i * k + c];
        up(dV_, col.data(), nc_);
        schurApply({dV_, false}, dQ_, /*withDot=*/false);
        sync();
        const std::vector<double> q = down(dQ_, nc_);
        for (int64_t i = 0; i < nc_; ++i) out[i * k + c] = q[i];
      }
      return;
    }
    if constexpr (std::is_same<T, double>::value) {
      dispatchWidth(k, [&](auto kb) {
        constexpr int KB = decltype(kb)::value;
        constexpr int XP = PkJ::XP;
        ensureBatchBufs(0);
        std::vector<T> h((size_t)ncam_ * KB * XP, T(0));
        for (int64_t cam = 0; cam < ncam_; ++cam)
          for (int c = 0; c < k; ++c)
            for (int i = 0; i < CD; ++i)
              h[(cam * KB + c) * XP + i] = (T)X[(cam * CD + i) * k + c];
        up(bb_.P, h.data(), (int64_t)h.size());
        schurApplyB<KB>(k);
        sync();
        const std::vector<double> q = down(bb_.Q, (int64_t)ncam_ * KB * CD);
        for (int64_t cam = 0; cam < ncam_; ++cam)
          for (int c = 0; c < k; ++c)
            for (int i = 0; i < CD; ++i)
              out[(cam * CD + i) * k + c] = q[(cam * KB + c) * CD + i];
      });
    }
  }

  // ---- dense Cholesky of the Schur complement -------------------------------
  // kernels_dense.hpp forms S, dense_chol.hip factors it and solves; fp64.
  DenseFactorInfo denseSchurFactor(double pivotTol) override {
    DenseFactorInfo info;
    if constexpr (std::is_same<T, double>::value) {
      const auto t0 = std::chrono::steady_clock::now();
      formDenseSchur();
      const auto t1 = std::chrono::steady_clock::now();
      info = factorDense(pivotTol);
      const auto t2 = std::chrono::steady_clock::now();
      info.formMs = std::chrono::duration<double, std::milli>(t1 - t0).count();
      info.factorMs =
          std::chrono::duration<double, std::milli>(t2 - t1).count();
      denseReady_ = info.ok;
    } else {
      MEGBA_CHECK(false, "the dense Schur route needs dtype float64");
    }
    return info;
  }

  void solveUnitDense(const int64_t* rhsRows, int k, const int64_t* readRows,
                      int n, double* out) override {
    MEGBA_CHECK(denseReady_, "solveUnitDense: no dense Schur factor");
    MEGBA_CHECK(k >= 1 && k <= (CD > PD ? CD : PD) && n > 0,
                "solveUnitDense: too many columns");
    for (int c = 0; c < k; ++c)
      MEGBA_CHECK(rhsRows[c] >= 0 && rhsRows[c] < dim_,
                  "unit right-hand side out of range");
    for (int i = 0; i < n; ++i)
      MEGBA_CHECK(readRows[i] >= 0 && readRows[i] < dim_,
                  "deltaX row out of range");
    static_assert((CD > PD ? CD : PD) <= dense::kMaxRhs,
                  "dense::solve carries at most kMaxRhs columns");
    if constexpr (std::is_same<T, double>::value) {
      // solveBatchW with the iteration loop replaced by two substitutions
      dispatchWidth(k, [&](auto kb) {
        constexpr int KB = decltype(kb)::value;
        ensureBatchBufs(n);
        unitRhsB<KB>(rhsRows, k);
        dense::solve(dn_.S, dn_.inv, dn_.np, nc_, bb_.R, bb_.X, dn_.work, CD,
                     KB, k, PkJ::XP, stream_);
        readRowsB<KB>(k, readRows, n, out);
      });
    }
  }

  void releaseDenseSchur() override { freeDense(); }

  void denseSchurMatrix(double* out) override {
    if constexpr (std::is_same<T, double>::value) {
      formDenseSchur();
      const int64_t np = dn_.np;
      std::vector<double> h((size_t)np * np);
      HIP_CHECK(hipMemcpy(h.data(), dn_.S, h.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
      freeDense();
      for (int64_t i = 0; i < nc_; ++i)
        for (int64_t j = 0; j <= i; ++j)
          out[i * nc_ + j] = out[j * nc_ + i] = h[i * np + j];
    } else {
      MEGBA_CHECK(false, "the dense Schur route needs dtype float64");
    }
  }

  DenseFactorInfo denseCholesky(double* A, int n, double pivotTol) override {
    freeDense();
    allocDense(n, /*edgeBlocks=*/false);
    const int64_t np = dn_.np;
    std::vector<double> h((size_t)np * np, 0.0);
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j <= i; ++j) h[i * np + j] = A[i * (int64_t)n + j];
    HIP_CHECK(hipMemcpyAsync(dn_.S, h.data(), h.size() * sizeof(double),
                             hipMemcpyHostToDevice, stream_));
    dense::identityTail(dn_.S, np, n, stream_);
    const DenseFactorInfo info = factorDense(pivotTol);
    HIP_CHECK(hipMemcpy(h.data(), dn_.S, h.size() * sizeof(double),
                        hipMemcpyDeviceToHost));
    freeDense();
    for (int64_t i = 0; i < n; ++i)
      for (int64_t j = 0; j < n; ++j) A[i * (int64_t)n + j] = h[i * np + j];
    return info;
  }

 private:
  // Buffers of the batched PCG in the layouts of kernels_batch.hpp, sized for
  // the widest batch (CD columns) and allocated at the first batched call.
  struct BatchBufs {
    T *P{}, *X{};             // [cam][KB][XP]
    T *R{}, *Z{}, *Q{};       // [cam][KB][CD]
    T* temp{};                // [pt][KB][PD]
    T* W{};                   // [pt][KB][4]
    double *part{}, *partQ{};  // [KB][nbR], [KB][nbQ]
    double *rho{}, *rhoPrev{};  // per column
    int* done{};                // per column: frozen
    int64_t* rhs{};             // the columns' unit rows
    int64_t* rowIdx{};          // requested rows and their values
    double* rowOut{};
    int rowCap = 0;
    int nbR = 0, nbQ = 0;
    double* hRho{};  // pinned: the per-iteration readback, then hDone
    int* hDone{};
  };

  // f(width tag): the narrowest compiled width that holds k columns.
  template <typename F>
  static void dispatchWidth(int k, F&& f) {
    if (k <= PD)
      f(std::integral_constant<int, PD>{});
    else
      f(std::integral_constant<int, CD>{});
  }
  template <typename K, typename... A>
  void launchGrid(K kernel, dim3 grid, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlk), 0, stream_, args...);
  }

  void ensureBatchBufs(int nRows) {
    constexpr int KBM = CD;
    BatchBufs& b = bb_;
    if (!b.P) {
      b.nbR = precondGrid();
      b.nbQ = bApplyDotGrid();
      b.P = dalloc<T>((int64_t)ncam_ * KBM * PkJ::XP);
      b.X = dalloc<T>((int64_t)ncam_ * KBM * PkJ::XP);
      b.R = dalloc<T>((int64_t)ncam_ * KBM * CD);
      b.Z = dalloc<T>((int64_t)ncam_ * KBM * CD);
      b.Q = dalloc<T>((int64_t)ncam_ * KBM * CD);
      b.temp = dalloc<T>((int64_t)npt_ * KBM * PD);
      b.W = dalloc<T>((int64_t)npt_ * KBM * 4);
      b.part = dalloc<double>((int64_t)KBM * b.nbR);
      b.partQ = dalloc<double>((int64_t)KBM * b.nbQ);
      b.rho = dalloc<double>(KBM);
      b.rhoPrev = dalloc<double>(KBM);
      b.done = dalloc<int>(KBM);
      b.rhs = dalloc<int64_t>(KBM);
      HIP_CHECK(hipHostMalloc((void**)&b.hRho,
                              KBM * (sizeof(double) + sizeof(int))));
      b.hDone = (int*)(b.hRho + KBM);
    }
    if (nRows > b.rowCap) {
      b.rowCap = nRows;
      b.rowIdx = dalloc<int64_t>(nRows);
      b.rowOut = dalloc<double>((int64_t)nRows * KBM);
    }
  }

  template <int KB>
  void zeroTempB() {
    zero(bb_.temp + (int64_t)ptLo_ * KB * PD, (int64_t)npL_ * KB * PD);
  }
  // temp = E^T x for the k columns of x ([cam][KB][XP]); temp is zeroed first
  template <int KB>
  void etxB(const T* x, int k) {
    zeroTempB<KB>();
    if (!implicit_) {
      launchN(kSpmvEtxB<T, CD, PD, RD, KB>, nL_, nL_, dCamOf_, dPtOf_, dHpl_,
              x, k, bb_.temp);
      return;
    }
    dispatchBool(hasInfo_, [&](auto infoTag) {
      launchN(kSpmvEtxPkB<T, CD, PD, RD, decltype(infoTag)::value, KB>, nL_,
              nL_, dCamOf_, dPtOf_, dJPk_, (const T* const*)dJSlots_, dInfo_,
              lossKind_, lossD2_, x, k, bb_.temp);
    });
  }
  // W = Cinv temp, Q = E W summed over the ranks
  template <int KB>
  void cinvThenExB(int k) {
    launchN(kCinvPadB<T, PD, KB>, (int64_t)npL_ * KB, npL_,
            shard(dHllInv_, PP), bb_.temp + (int64_t)ptLo_ * KB * PD, k,
            bb_.W + (int64_t)ptLo_ * KB * 4);
    zero(bb_.Q, (int64_t)ncam_ * KB * CD);
    if (nChunks_ > 0 && implicit_)
      launch(kSpmvExPkB<T, CD, PD, RD, KB>, nChunks_, 64, 0, nChunks_, dChCam_,
             dChLo_, dChHi_, dPtOfCam_, dJCamPk_, nL_, bb_.W, k, bb_.Q);
    else if (nChunks_ > 0)
      launch(kSpmvExB<T, CD, PD, RD, KB>, nChunks_, 64, 0, nChunks_, dChCam_,
             dChLo_, dChHi_, dPtOfCam_, dHplCam_, nL_, bb_.W, k, bb_.Q);
    allreduce(bb_.Q, (int64_t)ncam_ * KB * CD, ncclSum);
  }
  // Q = S P for the k columns of P, with the p.q partials: schurApply's
  // batched sibling, one allreduce of the whole product buffer.
  template <int KB>
  void schurApplyB(int k) {
    ++this->products_;
    etxB<KB>(bb_.P, k);
    cinvThenExB<KB>(k);
    launchGrid(kBApplyDotB<T, CD, KB>, dim3(bb_.nbQ, k), ncam_, dHppD_, bb_.P,
               bb_.Q, bb_.partQ);
  }

  // The batched PCG: the rotated body of pcgBodyRotated per column, eager
  // launches, one readback of the k rho values per iteration.  A column
  // stops when |rho| < relTol |rho_0|; its iteration count is taken then and
  // its done flag freezes it (alpha = 0, p kept), so x, r and p no longer
  // change while the other columns go on.
  template <int KB>
  void solveBatchW(const int64_t* rhsRows, int k, const SolverOptionPCG& opt,
                   const int64_t* readRows, int n, double* out, int* iters,
                   uint8_t* converged) {
    invertForSolve(opt);
    ensureBatchBufs(n);
    BatchBufs& b = bb_;
    const int64_t padN = (int64_t)ncam_ * KB * PkJ::XP;
    for (int c = 0; c < k; ++c) {
      b.hDone[c] = 0;
      iters[c] = 0;
      converged[c] = 0;
    }
    HIP_CHECK(hipMemcpyAsync(b.done, b.hDone, k * sizeof(int),
                             hipMemcpyHostToDevice, stream_));
    zero(b.P, padN);
    unitRhsB<KB>(rhsRows, k);
    // x = 0: r = v without a product
    for (int c = 0; c < k; ++c)
      launch(kSetScalar, 1, 1, 0, b.rhoPrev + c, INFINITY);
    const dim3 gridR(b.nbR, k), gridQ(b.nbQ, k);
    launchGrid(kPrecondRhoB<T, CD, KB>, gridR, ncam_, dHppInv_, b.R, b.Z,
               b.part);
    std::vector<double> rho0(k, 0.0);
    int nDone = 0;
    for (int it = 0; it < opt.maxIter && nDone < k; ++it) {
      launchGrid(kBetaPB<T, CD, KB>, gridQ, ncam_, b.Z, b.part, b.nbR,
                 b.rhoPrev, b.done, b.rho, b.P);
      schurApplyB<KB>(k);
      launchGrid(kUpdateXRPrecondB<T, CD, KB>, gridR, ncam_, b.rho, b.partQ,
                 b.nbQ, b.done, b.rhoPrev, b.P, b.Q, b.X, b.R, dHppInv_, b.Z,
                 b.part);
      HIP_CHECK(hipMemcpyAsync(b.hRho, b.rho, k * sizeof(double),
                               hipMemcpyDeviceToHost, stream_));
      sync();
      bool changed = false;
      for (int c = 0; c < k; ++c) {
        if (b.hDone[c]) continue;
        const double rho = std::abs(b.hRho[c]);
        if (it == 0) rho0[c] = rho;
        iters[c] = it + 1;
        if (rho < opt.relTol * rho0[c]) {
          b.hDone[c] = 1;
          converged[c] = 1;
          ++nDone;
          changed = true;
        }
      }
      if (changed && nDone < k)
        HIP_CHECK(hipMemcpyAsync(b.done, b.hDone, k * sizeof(int),
                                 hipMemcpyHostToDevice, stream_));
    }
    readRowsB<KB>(k, readRows, n, out);
  }

  // The k unit right-hand sides in R and x = 0 in X:
  // v = g_c - E Cinv g_p as solveLinear forms it; a camera unit is the same
  // on every rank and needs no 1 / world.
  template <int KB>
  void unitRhsB(const int64_t* rhsRows, int k) {
    BatchBufs& b = bb_;
    const int64_t padN = (int64_t)ncam_ * KB * PkJ::XP;
    const int64_t plainN = (int64_t)ncam_ * KB * CD;
    bool anyPoint = false;
    for (int c = 0; c < k; ++c) anyPoint = anyPoint || rhsRows[c] >= nc_;
    HIP_CHECK(hipMemcpyAsync(b.rhs, rhsRows, k * sizeof(int64_t),
                             hipMemcpyHostToDevice, stream_));
    zero(b.X, padN);
    zero(b.R, plainN);
    if (anyPoint) zeroTempB<KB>();
    launch(kSetUnitsB<T, CD, PD, KB>, 1, 64, 0, k, b.rhs, nc_, ptLo_, ptHi_,
           b.R, b.temp);
    if (anyPoint) {
      cinvThenExB<KB>(k);
      launchN(kSubAssign<T>, plainN, plainN, b.Q, b.R);
    }
  }

  // Rows readRows[0..n) of the k solutions in X, summed over the ranks:
  // back-substitution on the requested rows only (kGatherRowsB).
  template <int KB>
  void readRowsB(int k, const int64_t* readRows, int n, double* out) {
    BatchBufs& b = bb_;
    etxB<KB>(b.X, k);
    HIP_CHECK(hipMemcpyAsync(b.rowIdx, readRows, n * sizeof(int64_t),
                             hipMemcpyHostToDevice, stream_));
    const int64_t nOut = (int64_t)n * k;
    launchN(kGatherRowsB<T, CD, PD, KB>, nOut, n, k, b.rowIdx, b.rhs, b.X,
            b.temp, dHllInv_, nc_, ptLo_, ptHi_, rank_ == 0, b.rowOut);
    if (hasComm_)
      RCCL_CHECK(ncclAllReduce(b.rowOut, b.rowOut, nOut, ncclDouble, ncclSum,
                               comm_, stream_));
    HIP_CHECK(hipMemcpyAsync(out, b.rowOut, nOut * sizeof(double),
                             hipMemcpyDeviceToHost, stream_));
    sync();
    if (hasComm_ || world_ == 1) return;
    if (hostArD_) {
      hostArD_(out, (size_t)nOut, 's');
    } else if (hostAr_) {
      std::vector<T> t(out, out + nOut);
      hostAr_(t.data(), (size_t)nOut, 's');
      for (int64_t i = 0; i < nOut; ++i) out[i] = (double)t[i];
    }
  }

  // ---- dense Schur route -----------------------------------------------------
  // Device buffers of the dense route, held from denseSchurFactor to
  // releaseDenseSchur.
  struct DenseBufs {
    int64_t np = 0;            // padded dimension
    double* S{};               // np x np: S, then its factor L
    double* inv{};             // inverses of L's diagonal tiles
    double* diag0{};           // diagonal of S before the elimination
    double* work{};            // dense::solve scratch
    dense::FactorWords* words{};
    double *Wp{}, *Yc{};       // per-edge blocks of kDenseEdgeBlocks
  };

  void freeDense() {
    for (void* p : {(void*)dn_.S, (void*)dn_.inv, (void*)dn_.diag0,
                    (void*)dn_.work, (void*)dn_.words, (void*)dn_.Wp,
                    (void*)dn_.Yc})
      if (p) (void)hipFree(p);
    dn_ = DenseBufs{};
    denseReady_ = false;
  }

  // Buffers for an n x n system, after comparing their size with the free
  // device memory.
  void allocDense(int64_t n, bool edgeBlocks) {
    const int64_t np = dense::paddedDim(n);
    const int64_t kMax = CD > PD ? CD : PD;
    const int64_t edgeBytes = edgeBlocks ? 2 * nL_ * CP * 8 : 0;
    const int64_t need = 8 * np * np + 8 * np * dense::kTile +
                         8 * np * (1 + 2 * kMax) + edgeBytes;
    size_t freeB = 0, totalB = 0;
    HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
    MEGBA_CHECK((size_t)need <= freeB,
                "covariance: the dense Schur complement needs " +
                    std::to_string(need) + " bytes (8 n^2 with n = " +
                    std::to_string(n) + ") and the device has " +
                    std::to_string(freeB) +
                    " bytes free; use method=\"pcg\"");
    const auto get = [&](int64_t count) {
      void* p = nullptr;
      HIP_CHECK(hipMalloc(&p, (count > 0 ? count : 1) * sizeof(double)));
      return (double*)p;
    };
    dn_.np = np;
    dn_.S = get(np * np);
    dn_.inv = get(np * dense::kTile);
    dn_.diag0 = get(np);
    dn_.work = get(2 * np * kMax);
    dn_.words = (dense::FactorWords*)get(4);
    if (edgeBlocks) {
      dn_.Wp = get(nL_ * CP);
      dn_.Yc = get(nL_ * CP);
    }
  }

  // dn_.S = HppD - E Cinv E^T (lower triangle, identity tail) after
  // buildLinearSystem() and processDiag(): this rank's partial, the sum over
  // the ranks, then the replicated camera blocks once.
  void formDenseSchur() {
    SolverOptionPCG noJitter;
    noJitter.refuseJitter = true;
    invertForSolve(noJitter);
    freeDense();
    allocDense(nc_, /*edgeBlocks=*/true);
    if (!dCamEdgeRow_) {
      dCamEdgeRow_ = upNew(hCamRow_);
      dPtEdgeRow_ = upNew(hPtRow_);
    }
    const int64_t np = dn_.np;
    HIP_CHECK(hipMemsetAsync(dn_.S, 0, np * np * sizeof(double), stream_));
    if (nL_ > 0) {
      const T* camPk = implicit_ ? dJCamPk_ : dHplCam_;
      dispatchBool(implicit_, [&](auto impTag) {
        launchN(kDenseEdgeBlocks<T, CD, PD, RD, decltype(impTag)::value>, nL_,
                nL_, dCamPos_, dPtOf_, camPk, dHllInv_, dn_.Wp, dn_.Yc);
      });
    }
    int tile = kDenseTileCams<CD>;
    if (knobs_.denseTileCams && *knobs_.denseTileCams >= 1 &&
        *knobs_.denseTileCams < tile)
      tile = *knobs_.denseTileCams;
    launch(kDenseSchurForm<CD, PD>, ncam_, kBlk, 0, ncam_, tile, dCamEdgeRow_,
           dPtOfCam_, dPtEdgeRow_, ptLo_, dCamOf_, dn_.Wp, dn_.Yc, dn_.S, np);
    if constexpr (std::is_same<T, double>::value)
      allreduce(dn_.S, np * np, ncclSum);
    launchN(kDenseAddDiag<T, CD>, (int64_t)ncam_ * CC, ncam_, dHppD_, dn_.S,
            np);
    dense::identityTail(dn_.S, np, nc_, stream_);
    sync();
  }

  // Factor dn_.S in place and read the outcome back, once.
  DenseFactorInfo factorDense(double pivotTol) {
    // MEGBA_DENSE_PROFILE: time the three kernels with events (a sync per
    // launch, so the factorization as a whole runs slower)
    float phaseMs[3] = {0, 0, 0};
    dense::factor(dn_.S, dn_.np, dn_.inv, dn_.diag0, pivotTol, dn_.words,
                  stream_, knobs_.denseProfile ? phaseMs : nullptr);
    dense::FactorWords w;
    HIP_CHECK(hipMemcpyAsync(&w, dn_.words, sizeof(w), hipMemcpyDeviceToHost,
                             stream_));
    sync();
    DenseFactorInfo info;
    info.ok = w.failRow < 0;
    info.failRow = w.failRow;
    info.minPivotRatio = w.minRatio;
    info.failPivotRatio = w.failRatio;
    if (knobs_.denseProfile) info.trailingMs = phaseMs[2];
    return info;
  }

 public:
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
      zero(s.r[b], m * D);
      if (jw > 0) {
        s.J[b] = dalloc<T>(m * jw);
        zero(s.J[b], m * jw);
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
      launch(kPriorForward<T, decltype(kind)>, priorRedGrid(p.m), kBlk, 0,
             p.m, p.idx, p.mean, p.info, p.r, p.J, at.x, at.acc);
    });
  }

  // J^T L J and -J^T L r of the accepted set onto the vertices' own blocks.
  void priorAssemble() {
    forEachPrior([&](auto kind, auto perRow, const DevPrior& s,
                     const PriorSite& at) {
      using Kind = decltype(kind);
      constexpr bool PER_ROW = decltype(perRow)::value;
      const PriorView<T> p = s.view(cur_ ^ 1);
      launchN(kPriorAssemble<T, Kind, PER_ROW>,
              PER_ROW ? p.m * Kind::ROWS : p.m, p.m, p.idx, p.info, p.r, p.J,
              at.fixed, at.H, at.g);
    });
  }

  // The priors' share of the gain-ratio model, from the accepted set.
  void priorRho() {
    forEachPrior([&](auto kind, auto, const DevPrior& s, const PriorSite& at) {
      const PriorView<T> p = s.view(cur_ ^ 1);
      launch(kPriorRho<T, decltype(kind)>, priorRedGrid(p.m), kBlk, 0, p.m,
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
    auto assemble = [&](auto weightedTag, auto explTag) {
      constexpr bool HI = decltype(weightedTag)::value;
      constexpr bool EX = decltype(explTag)::value;
      launchN(kAssembleEdge<T, CD, PD, RD, HI, EX>, nL_, nL_, dCamOf_, dPtOf_,
              dR_[bak], dJc_[bak], dJp_[bak], dInfo_, dHll_, dHpl_, dG_, ncam_,
              dCamPos_, dSlab_, lossKind_, lossD2_, dJPk_);
      if (nChunks_ > 0) {
        if constexpr (std::is_same<T, double>::value && CD == 9 && PD == 3 &&
                      RD == 2) {
          if (knobs_.mfma) {
            launch(kAssembleCamMfma<T, CD, PD, RD, HI, EX>, nChunks_, 64, 0,
                   nChunks_, dChCam_, dChLo_, dChHi_, dSlab_, dHpp_, dG_);
            return;
          }
        }
        launch(kAssembleCam<T, CD, PD, RD, HI, EX>, nChunks_, 128, 0, nChunks_,
               dChCam_, dChLo_, dChHi_, dSlab_, dHpp_, dG_);
      }
    };
    dispatchBool(weighted(), [&](auto weightedTag) {
      dispatchBool(!implicit_,
                   [&](auto explTag) { assemble(weightedTag, explTag); });
    });
  }
  // f(tag) with a runtime bool as an integral_constant tag.
  template <typename F>
  static decltype(auto) dispatchBool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
  }
  // Every kernel launch goes through these two: on stream_, and for a kernel
  // over n items gridFor(n) blocks of kBlk threads without dynamic LDS.
  template <typename K, typename... A>
  void launch(K kernel, int grid, int block, size_t ldsBytes, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), ldsBytes, stream_,
                       args...);
  }
  template <typename K, typename... A>
  void launchN(K kernel, int64_t n, A... args) {
    launch(kernel, gridFor(n), kBlk, 0, args...);
  }
  // This rank's point shard of a point-indexed array of `width` per point.
  template <typename U>
  U* shard(U* base, int width) const {
    return base + (int64_t)ptLo_ * width;
  }
  void zero(T* p, int64_t n) {
    HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), stream_));
  }
  void copyD2D(T* dst, const T* src, int64_t n) {
    HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToDevice,
                             stream_));
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
  void downTo(double* dst, const T* src, int64_t n) const {
    std::vector<T> h(n);
    HIP_CHECK(hipMemcpy(h.data(), (void*)src, n * sizeof(T), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) dst[i] = (double)h[i];
  }
  std::vector<double> down(const T* src, int64_t n) const {
    std::vector<double> o(n);
    downTo(o.data(), src, n);
    return o;
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
    const auto reduce = [&](auto opTag) {
      constexpr ROp OP = decltype(opTag)::value;
      launch(kRedPartial<T, OP>, kRedBlocks, kBlk, 0, a, b, n, dPart_);
      launch(kRedFinal<OP>, 1, kBlk, 0, dPart_, kRedBlocks, out);
    };
    switch (op) {
      case ROp::Dot: reduce(std::integral_constant<ROp, ROp::Dot>{}); break;
      case ROp::SumSq: reduce(std::integral_constant<ROp, ROp::SumSq>{}); break;
      case ROp::AbsMax: reduce(std::integral_constant<ROp, ROp::AbsMax>{}); break;
    }
  }
  double reduceDet(const T* a, const T* b, int64_t n, ROp op) {
    reduceDetAsync(a, b, n, op, scalarPtr());
    return readScalar(scalarPtr());
  }
  // Sum of squares or abs-max of a dim_ vector: the replicated camera part
  // here, this rank's point shard combined across the ranks.
  double reduceVec(const T* v, ROp op) {
    const double cam = reduceDet(v, v, nc_, op);
    const T* pts = shard(v + nc_, PD);
    reduceDetAsync(pts, pts, (int64_t)npL_ * PD, op, scalarPtr());
    if (op == ROp::SumSq) return cam + globalScalar(ncclSum);
    const double ptMax = globalScalar(ncclMax);
    return cam > ptMax ? cam : ptMax;
  }
  // Block inverses of HppD and of this rank's HllD with the given kernel pair
  // (kInvert, or kInvertJitter for the retry), then the failure flags.
  template <typename KC, typename KP>
  void invertBlocks(KC camKernel, KP ptKernel, int fail[2]) {
    launchN(camKernel, ncam_, ncam_, dHppD_, dHppInv_, dFail_);
    launchN(ptKernel, npL_, npL_, shard(dHllD_, PP), shard(dHllInv_, PP),
            dFail_);
    HIP_CHECK(hipMemcpyAsync(fail, dFail_, 2 * sizeof(int),
                             hipMemcpyDeviceToHost, stream_));
    sync();
  }
  template <int D, int MODE>
  void blockMatVec(int nBlk, const T* A, const T* xv, T* yv) {
    launchN(kBlockDiagMatVec<T, D, MODE>, (int64_t)nBlk * D, nBlk, A, xv, yv);
  }
  // The kernels of one PCG iteration.  Resolved once, at the first solve, and
  // never written again: the captured PCG graph bakes in what it selects.
  PcgPlan resolvePlan() {
    const SchurPath tuned = chooseSchurPath();
    // MEGBA_TUNE_VERBOSE reports the tuner's choice (the tests read it
    // back), also when MEGBA_FUSED then overrides the product
    if (knobs_.tuneVerbose)
      fprintf(stderr, "# schur path: %s\n", schurPathName(tuned));
    if (knobs_.tuneVerbose && tuned == SchurPath::LdsRecompute)
      fprintf(stderr, "# schur recompute gather: %s\n",
              rcStaged_ ? "staged" : "per-lane");
    return makePcgPlan(tuned, knobs_, implicit_, nLongPts_, allreduceIsNoop());
  }
  // The device half of the choice that schur_plan.hpp describes: the first
  // launch of each LDS candidate, and where nothing is forced 3 local Schur
  // applies per candidate, timed on the real data.  Only the LOCAL part runs
  // (no collective), so ranks may even pick differently without breaking
  // lockstep: q partials are per-rank inputs to the allreduce either way.
  SchurPath chooseSchurPath() {
    // first launch happens here, outside any graph capture: a launch the
    // runtime refuses (LDS size) drops the candidate instead of failing
    const auto launches = [&](SchurPath path) {
      (void)hipGetLastError();
      localSchurEcE(path, {dDeltaX_, false}, dQ_);
      return hipGetLastError() == hipSuccess;
    };
    // c.lds, c.rc: the LDS forms that are timed next to the two-pass paths
    const SchurUntimed c = schurPathUntimed(
        schurCandidates(knobs_, ldsEligible_, rcEligible_, nL_), launches);
    if (c.path) return *c.path;
    hipEvent_t ev[2];
    HIP_CHECK(hipEventCreate(&ev[0]));
    HIP_CHECK(hipEventCreate(&ev[1]));
    float ms[4] = {0, 0, 0, 0};
    const bool timed[4] = {true, true, c.lds, c.rc};
    for (int variant = 0; variant < 4; ++variant) {
      if (!timed[variant]) continue;
      // warm-up then timed triple (dQ_/dWPad_/dTemp_ are scratch)
      localSchurEcE(kTimedPaths[variant], {dDeltaX_, false}, dQ_);
      HIP_CHECK(hipEventRecord(ev[0], stream_));
      for (int k = 0; k < 3; ++k)
        localSchurEcE(kTimedPaths[variant], {dDeltaX_, false}, dQ_);
      HIP_CHECK(hipEventRecord(ev[1], stream_));
      HIP_CHECK(hipEventSynchronize(ev[1]));
      HIP_CHECK(hipEventElapsedTime(&ms[variant], ev[0], ev[1]));
    }
    if (knobs_.tuneVerbose)
      fprintf(stderr,
              "# schur autotune: fused-etx %.3f ms, separate %.3f ms, "
              "lds %.3f ms (3 applies each)\n",
              ms[0], ms[1], c.lds ? ms[2] : -1.0f);
    if (knobs_.tuneVerbose && c.rc)
      fprintf(stderr, "# schur recompute: %.3f ms (3 applies)\n", ms[3]);
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return schurPathFromTimings(ms, c.lds, c.rc);
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
  // Dynamic LDS of the LDS applies: the accumulators, and for the staged
  // kSchurFusedLdsRc instance one tile per wave behind them.
  size_t ldsBytes(bool staged = false) const {
    return staged ? (size_t)rcStagedLdsBytes(nc_, (int)sizeof(T),
                                             rcThreads_ / 64)
                  : (size_t)nc_ * sizeof(T);
  }
  void launchSchurLdsRc() {
    [[maybe_unused]] const PadDst d = padDstFor(SchurPath::LdsRecompute);
    if constexpr (kBalDims)
      dispatchBool(hasInfo_, [&](auto infoTag) {
        dispatchBool(rcStaged_, [&](auto stagedTag) {
          launch(kSchurFusedLdsRc<T, decltype(infoTag)::value,
                                  decltype(stagedTag)::value>,
                 numCU_, rcThreads_, ldsBytes(rcStaged_), nWin_, dWinLo_,
                 dWinHi_, dWinFlag_, nL_, dCamOf_, dPtOf_, dCamRow_,
                 rcCamStride(), d.p + d.off, d.stride, dPtAcc_, dCamFixed_,
                 dPtFixed_, (const T* const*)dJSlots_, dInfo_, lossKind_,
                 lossD2_, dHllInv_, dTemp_, (int)nc_, dLdsRows_);
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
    launchN(kPadX<T, CD>, ncam_, ncam_, x, d.p, d.stride, d.off);
  }
  // Common start of the window passes: the padded copy of x where the path
  // reads it unless it is ready, and a zeroed temp when >64-edge runs will
  // add partials to it.  The long-run finishers read dXPad_ on every path,
  // so with such runs the staged recompute path fills that as well.
  void windowPrologue(XIn x, SchurPath path) {
    if (!x.padReady) padX(x.v, padDstFor(path));
    if (nLongPts_ > 0 && path == SchurPath::LdsRecompute && rcStaged_)
      padX(x.v, xPadDst());
    if (nLongPts_ > 0) zeroShard(dTemp_);
  }
  // Zero this rank's shard of a PD-wide point vector.
  void zeroShard(T* v) {
    launchN(kZeroRange<T>, (int64_t)npL_ * PD, shard(v, PD),
            (int64_t)npL_ * PD);
  }
  // w_p = Cinv temp_p for the >64-edge points, into w at the given stride.
  void longRunW(T* w, int stride) {
    if (nLongPts_ > 0)
      launchN(kFusedLongW<T, PD>, nLongPts_, nLongPts_, dLongPts_, dHllInv_,
              dTemp_, w, stride);
  }
  // Finish the flagged windows of a single-pass apply on the global output.
  void finishLongRuns(T* out) {
    if (nLongPts_ == 0) return;
    longRunW(dW_, PD);
    dispatchMode([&](auto impTag, auto infoTag) {
      constexpr bool IM = decltype(impTag)::value;
      constexpr bool HI = decltype(infoTag)::value;
      launch(kFusedLongScatter<T, CD, PD, RD, IM, HI>,
             windowGrid(nFlagWins_), 256, 0, nFlagWins_, dFlagWins_, dWinLo_,
             dWinHi_, nL_, dCamOf_, dPtOf_, dHpl_, (const T* const*)dJSlots_,
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
    const int64_t need = (int64_t)ldsBytes();
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
      zero(dCamRow_, (int64_t)ncam_ * RcRow<T>::LEN);
      zero(dPtAcc_, (int64_t)npt_ * 4);
      rcEligible_ = true;
      // Staged gather: the per-wave tiles must fit behind the accumulators
      // (MEGBA_NO_RC_STAGE takes it out); otherwise the per-lane instance
      // runs and nothing else changes.
      const int64_t stagedNeed = (int64_t)ldsBytes(true);
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
  // path is Lds or LdsRecompute; for the latter the window kernel is
  // kSchurFusedLdsRc, which rebuilds the implicit edge from the accepted
  // snapshot instead of reading dJPk_.
  void schurFusedLdsEcE(XIn x, T* out, SchurPath path,
                        bool bApplyDot = false) {
    windowPrologue(x, path);
    if (path == SchurPath::LdsRecompute)
      launchSchurLdsRc();
    else
      dispatchMode([&](auto impTag, auto infoTag) {
        constexpr bool IM = decltype(impTag)::value;
        constexpr bool HI = decltype(infoTag)::value;
        launch(kSchurFusedLds<T, CD, PD, RD, IM, HI>, numCU_, ldsThreads_,
               ldsBytes(), nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_,
               dPtOf_, dHpl_, dJPk_, (const T* const*)dJSlots_, dInfo_,
               lossKind_, lossD2_, dXPad_, dHllInv_, dTemp_, (int)nc_,
               dLdsRows_);
      });
    if (bApplyDot) {
      launch(kLdsReduceBApplyDot<T, CD>, ldsReduceGrid(), 64 * kLdsRedWaves, 0,
             numCU_, (int)nc_, dLdsRows_, dHppD_, x.v, out, dPartQ_);
      return;
    }
    launch(kLdsRowsReduce<T>, ldsReduceGrid(), 64 * kLdsRedWaves, 0, numCU_,
           (int)nc_, dLdsRows_, out);
    finishLongRuns(out);
  }

  // local (collective-free) E Cinv E^T x into out on the given path; the
  // tuner passes its four candidates, never OnePass
  void localSchurEcE(SchurPath path, XIn x, T* out) {
    switch (path) {
      case SchurPath::Lds:
      case SchurPath::LdsRecompute:
        schurFusedLdsEcE(x, out, path);
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
        schurFusedEcE(x, out);
        break;
    }
  }

  // w = Cinv in, then out += E w.  w is stored 4-padded so the E-side
  // gather is a single aligned vector load per edge (both modes).
  void cinvThenEx(const T* in, T* out) {
    launchN(kCinvPad<T, PD>, npL_, npL_, shard(dHllInv_, PP), shard(in, PD),
            shard(dWPad_, 4));
    spmvEx(dWPad_, out);
  }
  void spmvEtx(XIn x, T* out) {
    zeroShard(out);
    if (!implicit_) {
      launchN(kSpmvEtx<T, CD, PD, RD>, nL_, nL_, dCamOf_, dPtOf_, dHpl_, x.v,
              out);
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
      launchN(kernel, nL_, nL_, dCamOf_, dPtOf_, dJPk_,
              (const T* const*)dJSlots_, dInfo_, lossKind_, lossD2_, dXPad_,
              out);
    });
  }
  void spmvEx(const T* wv, T* out) {
    zero(out, nc_);
    if (implicit_) {
      if (nChunks_ == 0) return;
      launch(kSpmvExPk<T, CD, PD, RD>, nChunks_, 64, 0, nChunks_, dChCam_,
             dChLo_, dChHi_, dPtOfCam_, dJCamPk_, nL_, wv, out);
      return;
    }
    if (nChunks_ > 0)
      launch(kSpmvEx<T, CD, PD>, nChunks_, 64, 0, nChunks_, dChCam_, dChLo_,
             dChHi_, dPtOfCam_, dHplCam_, nL_, wv, out);
  }
  // One full PCG iteration (captured as a hipGraph when possible): the
  // rotated body, or the seven-kernel one below (docs/INTERNALS.md section 6).
  void pcgBody() {
    if (plan_->rotatedBody) {
      pcgBodyRotated();
      return;
    }
    const int rhoGrid = gridFor(nc_) < kRedBlocks ? gridFor(nc_) : kRedBlocks;
    launch(kPrecondRho<T, CD>, rhoGrid, kBlk, 0, ncam_, dHppInv_, dRr_, dZ_,
           dPart_);
    launchN(kXpbySBeta<T>, nc_, nc_, dZ_, dPart_, rhoGrid, slotRhoPrev(),
            slotRho(), dP_);
    const int nPartQ = schurApply({dP_, false}, dQ_, /*withDot=*/true);
    launchN(kUpdateXRAlpha<T>, nc_, nc_, dPart_, rhoGrid, dPartQ_, nPartQ,
            slotRhoPrev(), dP_, dQ_, dDeltaX_, dXBak_, dXBakPrev_, dRr_);
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
      launchN(kBetaPPad<T, CD>, (int64_t)ncam_ * PkJ::XP, ncam_, dZ_, dPart_,
              nbR, slotRhoPrev(), slotRho(), dP_, d.p, d.stride, d.off);
    } else {
      launchN(kXpbySBeta<T>, nc_, nc_, dZ_, dPart_, nbR, slotRhoPrev(),
              slotRho(), dP_);
    }
    const int nPartQ =
        schurApply({dP_, plan_->productReadsPad}, dQ_, /*withDot=*/true);
    launch(kUpdateXRPrecond<T, CD>, nbR, kBlk, 0, ncam_, slotRho(), dPartQ_,
           nPartQ, slotRhoPrev(), dP_, dQ_, dDeltaX_, dXBak_, dXBakPrev_, dRr_,
           dHppInv_, dZ_, dPart_);
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
    const int64_t productsBefore = this->products_;
    try {
      pcgBody();
    } catch (...) {
      ok = false;
    }
    this->products_ = productsBefore;  // captured, not applied
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
    zero(out, nc_);
    windowPrologue(x, SchurPath::OnePass);
    dispatchMode([&](auto impTag, auto infoTag) {
      constexpr bool IM = decltype(impTag)::value;
      constexpr bool HI = decltype(infoTag)::value;
      launch(kSchurFused<T, CD, PD, RD, IM, HI>, windowGrid(nWin_), 256, 0,
             nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_, dPtOf_, dHpl_,
             (const T* const*)dJSlots_, dInfo_, lossKind_, lossD2_, dXPad_,
             dHllInv_, dTemp_, out);
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
      launch(kEtxCinvFused<T, CD, PD, RD, IM, HI>, windowGrid(nWin_), 256, 0,
             nWin_, dWinLo_, dWinHi_, dWinFlag_, nL_, dCamOf_, dPtOf_, dHpl_,
             (const T* const*)dJSlots_, dInfo_, lossKind_, lossD2_, dXPad_,
             dHllInv_, dTemp_, dWPad_);
    });
    longRunW(dWPad_, 4);
  }

  // q = S x = HppD x - E Cinv E^T x  (ONE CD*ncam allreduce; the reference's
  // site A4 needed an additional 3*npt allreduce here).  withDot fuses the
  // x^T q dot partials into the B-apply pass (used by the PCG body) and
  // returns how many partials it wrote to dPartQ_ (0 without withDot).
  int schurApply(XIn x, T* q, bool withDot) {
    ++this->products_;
    if (withDot && plan_->mergeReduceBApply) {
      schurFusedLdsEcE(x, q, plan_->path, /*bApplyDot=*/true);
      return ldsReduceGrid();
    }
    localSchurEcE(plan_->path, x, q);
    allreduce(q, nc_, ncclSum);
    if (withDot) {
      launch(kBApplyDot<T, CD>, bApplyDotGrid(), kBlk, 0, ncam_, dHppD_, x.v,
             q, dPartQ_);
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
  T *dGSaved_{}, *dDeltaXSaved_{};  // saveLinearState, allocated on first use
  int64_t* dRowIdx_{};              // readDeltaXRows: requested rows
  double* dRowOut_{};               //   and their values
  int rowCap_ = 0;
  std::vector<uint8_t> hCamFixed_, hPtFixed_;  // host copies for isFixed
  bool relStopHit_ = false;
  BatchBufs bb_;  // batched PCG, allocated at the first batched call
  DenseBufs dn_;  // dense Schur route
  bool denseReady_ = false;
  std::vector<int> hCamRow_;       // cam-sorted row range of every camera
  std::vector<int64_t> hPtRow_;    // local edge range of every local point
  int* dCamEdgeRow_{};
  int64_t* dPtEdgeRow_{};
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
