// Python bindings for megba_amd.
// The Python layer supplies the raw problem (numpy arrays) and, for
// multi-process CPU runs, an in-place allreduce callback (torch.distributed
// gloo); the GPU path uses RCCL natively (gpu/gpu_engine.hip).
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <memory>

#include "megba/bal_functor.hpp"
#include "megba/common.hpp"
#include "megba/covariance.hpp"
#include "megba/custom.hpp"
#include "megba/jv/jetvector.hpp"
#include "megba/cpu_engine.hpp"
#include "megba/engine.hpp"
#include "megba/lm.hpp"
#include "megba/problem.hpp"
#include "megba/gpu/edge_tables.hpp"  // host-only
#include "megba/gpu/rc_tile.hpp"      // host-only
#include "megba/gpu/schur_plan.hpp"   // host-only

#ifdef MEGBA_WITH_GPU
#include "megba/gpu/gpu_engine.hpp"
#endif

namespace py = pybind11;
using namespace megba;

namespace {

// Python-facing JetVector (fp64).
struct PyJetVec {
  JetVec<double> v;
};

template <typename T>
HostAllreduce<T> wrapAllreduce(py::object fn) {
  if (fn.is_none()) return nullptr;
  // Keep the callable alive in the closure; reacquire the GIL per call.
  auto holder = std::make_shared<py::object>(std::move(fn));
  return [holder](T* data, std::size_t n, char op) {
    py::gil_scoped_acquire gil;
    py::array arr(py::dtype::of<T>(), {(py::ssize_t)n}, {(py::ssize_t)sizeof(T)},
                  data, py::none());
    (*holder)(arr, op == 'm' ? "max" : "sum");
  };
}

struct PyProblem {
  BAProblemHost prob;
  ProblemIndex ix;
  ProblemOption opt;
  std::unique_ptr<Engine<double>> engD;
  std::unique_ptr<Engine<float>> engF;
  bool isDouble = true;

  PyProblem(py::array_t<double, py::array::c_style | py::array::forcecast> cams,
            py::array_t<double, py::array::c_style | py::array::forcecast> pts,
            py::array_t<int, py::array::c_style | py::array::forcecast> camIdx,
            py::array_t<int, py::array::c_style | py::array::forcecast> ptIdx,
            py::array_t<double, py::array::c_style | py::array::forcecast> meas,
            py::object info, py::object camFixed, py::object ptFixed) {
    // Block dims are inferred from the array shapes (reference analogue:
    // ProblemOption.N, include/common.h:27-46).  Compiled set:
    // camDim in {9,6,4}, ptDim = 3, resDim in {2,3}.
    MEGBA_CHECK(cams.ndim() == 2 && (cams.shape(1) == 9 || cams.shape(1) == 6 ||
                                     cams.shape(1) == 4),
                "cams must be (ncam, 9|6|4)");
    MEGBA_CHECK(pts.ndim() == 2 && pts.shape(1) == 3, "pts must be (npt,3)");
    MEGBA_CHECK(meas.ndim() == 2 && (meas.shape(1) == 2 || meas.shape(1) == 3),
                "meas must be (nobs, 2|3)");
    prob.camDim = (int)cams.shape(1);
    prob.ptDim = (int)pts.shape(1);
    prob.resDim = (int)meas.shape(1);
    prob.ncam = (int)cams.shape(0);
    prob.npt = (int)pts.shape(0);
    prob.nobs = (int64_t)meas.shape(0);
    prob.cams.assign(cams.data(), cams.data() + cams.size());
    prob.pts.assign(pts.data(), pts.data() + pts.size());
    prob.camIdx.assign(camIdx.data(), camIdx.data() + camIdx.size());
    prob.ptIdx.assign(ptIdx.data(), ptIdx.data() + ptIdx.size());
    prob.meas.assign(meas.data(), meas.data() + meas.size());
    if (!info.is_none()) {
      const int rw = prob.resDim * (prob.resDim + 1) / 2;
      auto infoArr = py::cast<
          py::array_t<double, py::array::c_style | py::array::forcecast>>(info);
      MEGBA_CHECK(infoArr.ndim() == 2 && infoArr.shape(1) == rw &&
                      infoArr.shape(0) == prob.nobs,
                  "info must be (nobs, resDim*(resDim+1)/2) packed-upper "
                  "symmetric (RD=2: w00,w01,w11)");
      prob.info.assign(infoArr.data(), infoArr.data() + infoArr.size());
    }
    auto readMask = [](py::object o, int n, std::vector<uint8_t>& dst) {
      if (o.is_none()) return;
      auto arr = py::cast<
          py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>(o);
      MEGBA_CHECK((int)arr.size() == n, "fixed mask size mismatch");
      dst.assign(arr.data(), arr.data() + arr.size());
    };
    readMask(camFixed, prob.ncam, prob.camFixed);
    readMask(ptFixed, prob.npt, prob.ptFixed);
  }

  // Record one kind of unary prior (kind: 0 camera parameters, 1 point,
  // 2 camera centre).  Only "too late" is refused here; everything about the
  // arrays is judged by build(), which knows the model the dims select.
  std::string priorShapeErr[3];
  void setPrior(int kind,
                py::array_t<int, py::array::c_style | py::array::forcecast> idx,
                py::array_t<double, py::array::c_style | py::array::forcecast>
                    mean,
                py::object info) {
    MEGBA_CHECK(!engD && !engF, "priors must be set before build()");
    PriorList& l = kind == 0 ? prob.camPrior
                   : kind == 1 ? prob.ptPrior
                               : prob.centerPrior;
    const int D = kind == 0 ? prob.camDim : kind == 1 ? prob.ptDim : 3;
    const py::ssize_t m = idx.size();
    l.idx.assign(idx.data(), idx.data() + m);
    l.mean.assign(mean.data(), mean.data() + mean.size());
    l.info.clear();
    std::string err;
    if (idx.ndim() != 1) err = "prior idx must be one-dimensional";
    if (mean.ndim() != 2 || mean.shape(0) != m || mean.shape(1) != D)
      err = "prior mean must be (len(idx), " + std::to_string(D) + ")";
    if (!info.is_none()) {
      auto arr = py::cast<
          py::array_t<double, py::array::c_style | py::array::forcecast>>(info);
      const int W = D * (D + 1) / 2;
      if (arr.ndim() != 2 || arr.shape(0) != m || arr.shape(1) != W)
        err = "prior info must be (len(idx), " + std::to_string(W) +
              ") packed-upper symmetric (see pack_sym)";
      l.info.assign(arr.data(), arr.data() + arr.size());
      // an empty list means identity: keep a malformed empty array an error
      if (arr.size() == 0 && m > 0) err = "prior info is empty";
    }
    priorShapeErr[kind] = err;
  }

  void build(const std::string& device, const std::string& dtype, int rank,
             int worldSize, int deviceIndex, const std::string& diff,
             const std::string& schur, const std::string& loss,
             double lossDelta, py::object allreduce, py::object rcclId,
             py::object customForward, py::object intrinsics) {
    opt.rank = rank;
    opt.worldSize = worldSize;
    opt.deviceIndex = deviceIndex;
    opt.camDim = prob.camDim;
    opt.ptDim = prob.ptDim;
    opt.resDim = prob.resDim;
    if (!intrinsics.is_none()) {
      auto arr = py::cast<
          py::array_t<double, py::array::c_style | py::array::forcecast>>(
          intrinsics);
      MEGBA_CHECK(arr.size() == 3, "intrinsics must be [f, k1, k2]");
      for (int i = 0; i < 3; ++i) opt.intr[i] = arr.data()[i];
    }
    MEGBA_CHECK(!customForward.is_none() ||
                    hasBuiltinResidual(prob.camDim, prob.ptDim, prob.resDim),
                "no built-in residual for (camDim,ptDim,resDim) = (" +
                    std::to_string(prob.camDim) + "," +
                    std::to_string(prob.ptDim) + "," +
                    std::to_string(prob.resDim) +
                    "): provide custom_forward (built-ins: (9,3,2) BAL, "
                    "(6,3,2) BAL fixed-intrinsics, (6,3,3) SE3 point)");
    MEGBA_CHECK(diff != "analytical" ||
                    (prob.camDim == 9 && prob.resDim == 2),
                "analytical diff is only available for the BAL (9,3,2) "
                "model");
    MEGBA_CHECK(device == "cpu" || device == "gpu", "device must be cpu|gpu");
    MEGBA_CHECK(dtype == "float64" || dtype == "float32",
                "dtype must be float64|float32");
    MEGBA_CHECK(diff == "auto" || diff == "analytical",
                "diff must be auto|analytical");
    MEGBA_CHECK(schur == "explicit" || schur == "implicit",
                "schur must be explicit|implicit");
    opt.device = device == "gpu" ? Device::GPU : Device::CPU;
    opt.diff = diff == "analytical" ? DiffMode::ANALYTICAL : DiffMode::AUTO;
    opt.schur = schur == "implicit" ? SchurMode::IMPLICIT : SchurMode::EXPLICIT;
    opt.loss = loss == "huber" ? LossKind::HUBER
               : loss == "cauchy" ? LossKind::CAUCHY
                                  : LossKind::NONE;
    MEGBA_CHECK(loss == "none" || loss == "huber" || loss == "cauchy",
                "loss must be none|huber|cauchy");
    opt.lossDelta = lossDelta;
    isDouble = dtype != "float32";
    MEGBA_CHECK(customForward.is_none() || isDouble,
                "custom_forward requires float64");
    for (const std::string& err : priorShapeErr) MEGBA_CHECK(err.empty(), err);
    validatePriors(prob, !customForward.is_none());
    CustomForward<double> cf = wrapCustomForward(customForward);
    ix = buildIndex(prob, worldSize);
    if (opt.device == Device::CPU) {
      // A CPU world>1 run without an allreduce hook would silently skip
      // every reduction (each collective is guarded by `if (ar_)`) and
      // produce wrong Hpp/g/chi2 per rank; refuse it like the GPU path
      // refuses a missing rccl_id.
      MEGBA_CHECK(worldSize == 1 || !allreduce.is_none(),
                  "CPU world_size>1 requires an allreduce callback");
      if (isDouble)
        engD = makeCpuEngine<double>(prob, ix, opt,
                                     wrapAllreduce<double>(allreduce), cf,
                                     wrapAllreduce<double>(allreduce));
      else
        engF = makeCpuEngine<float>(prob, ix, opt, wrapAllreduce<float>(allreduce),
                                    nullptr, wrapAllreduce<double>(allreduce));
    } else {
#ifdef MEGBA_WITH_GPU
      std::string id;
      if (!rcclId.is_none()) id = py::cast<std::string>(rcclId);
      if (isDouble)
        engD = makeGpuEngine<double>(prob, ix, opt, id, cf,
                                     wrapAllreduce<double>(allreduce),
                                     wrapAllreduce<double>(allreduce));
      else
        engF = makeGpuEngine<float>(prob, ix, opt, id, nullptr,
                                    wrapAllreduce<float>(allreduce),
                                    wrapAllreduce<double>(allreduce));
#else
      MEGBA_CHECK(false, "built without GPU support");
#endif
    }
  }

  static CustomForward<double> wrapCustomForward(py::object fn);

  template <typename F>
  auto withEngine(F&& f) {
    MEGBA_CHECK(engD || engF, "call build() first");
    if (isDouble) return f(*engD);
    return f(*engF);
  }

  py::dict solve(int maxIter, double tau, double eps1, double eps2,
                 int solverMaxIter, double solverTol, double refuseRatio,
                 bool forceIterations, bool verbose) {
    AlgoOptionLM a;
    a.maxIter = maxIter;
    a.initialRegion = tau;
    a.epsilon1 = eps1;
    a.epsilon2 = eps2;
    a.forceIterations = forceIterations;
    a.verbose = verbose;
    SolverOptionPCG s;
    s.maxIter = solverMaxIter;
    s.tol = solverTol;
    s.refuseRatio = refuseRatio;
    LMReport rep;
    {
      py::gil_scoped_release rel;
      if (isDouble)
        rep = runLM<double>(*engD, a, s);
      else
        rep = runLM<float>(*engF, a, s);
    }
    py::dict d;
    d["final_chi2"] = rep.finalChi2;
    d["accepted"] = rep.acceptedSteps;
    d["rejected"] = rep.rejectedSteps;
    d["total_ms"] = rep.totalMs;
    py::list iters;
    for (const auto& it : rep.iters) {
      py::dict e;
      e["iter"] = it.iter;
      e["accepted"] = it.accepted;
      e["chi2"] = it.chi2;
      e["elapsed_ms"] = it.elapsedMs;
      e["pcg_iters"] = it.pcgIters;
      iters.append(e);
    }
    d["iters"] = iters;
    return d;
  }

  // Step-level LM control (bench.py times exact step counts with this).
  std::unique_ptr<LMSession<double>> sessD;
  std::unique_ptr<LMSession<float>> sessF;
  double lmInit(int maxIter, double tau, double eps1, double eps2,
                int solverMaxIter, double solverTol, double refuseRatio,
                bool forceIterations, bool verbose) {
    AlgoOptionLM a;
    a.maxIter = maxIter;
    a.initialRegion = tau;
    a.epsilon1 = eps1;
    a.epsilon2 = eps2;
    a.forceIterations = forceIterations;
    a.verbose = verbose;
    SolverOptionPCG so;
    so.maxIter = solverMaxIter;
    so.tol = solverTol;
    so.refuseRatio = refuseRatio;
    py::gil_scoped_release rel;
    if (isDouble) {
      sessD = std::make_unique<LMSession<double>>(*engD, a, so);
      return sessD->init();
    }
    sessF = std::make_unique<LMSession<float>>(*engF, a, so);
    return sessF->init();
  }
  py::dict lmStep() {
    MEGBA_CHECK(sessD || sessF, "lm_init first");
    IterLog log;
    {
      py::gil_scoped_release rel;
      log = isDouble ? sessD->step() : sessF->step();
    }
    py::dict e;
    e["iter"] = log.iter;
    e["accepted"] = log.accepted;
    e["chi2"] = log.chi2;
    e["elapsed_ms"] = log.elapsedMs;
    e["pcg_iters"] = log.pcgIters;
    e["stopped"] = isDouble ? sessD->stopped() : sessF->stopped();
    return e;
  }

  // Fine-grained steps for tests.
  double forward() {
    return withEngine([&](auto& e) { return e.forward(); });
  }
  void acceptForward() {
    withEngine([&](auto& e) { e.acceptForward(); return 0; });
  }
  void buildLinearSystem() {
    py::gil_scoped_release rel;
    withEngine([&](auto& e) { e.buildLinearSystem(); return 0; });
  }
  void processDiag(double region) {
    withEngine([&](auto& e) { e.processDiag(region); return 0; });
  }
  int solveLinear(int maxIter, double tol, double refuseRatio, double relTol) {
    SolverOptionPCG s;
    s.maxIter = maxIter;
    s.tol = tol;
    s.refuseRatio = refuseRatio;
    s.relTol = relTol;
    py::gil_scoped_release rel;
    return withEngine([&](auto& e) { return e.solveLinear(s); });
  }

  // Marginal covariance of the given vertices (covariance.hpp).
  py::dict covariance(const std::vector<int>& camIds,
                      const std::vector<int>& ptIds, double tol, int maxIter,
                      bool strict, int batch, const std::string& method,
                      py::object pivotTol, bool cross) {
    MEGBA_CHECK(engD || engF, "call build() first");
    // H's condition number is about 5e11 already on a 12-camera problem
    MEGBA_CHECK(isDouble, "covariance needs dtype float64");
    CovarianceOption o;
    o.tol = tol;
    o.maxIter = maxIter;
    o.strict = strict;
    o.batch = batch;
    if (method != "pcg" && method != "dense")
      throw py::value_error("megba: covariance method must be pcg|dense");
    o.method = method == "dense" ? CovarianceMethod::Dense
                                 : CovarianceMethod::Pcg;
    if (!pivotTol.is_none()) o.pivotTol = py::cast<double>(pivotTol);
    o.cross = cross;
    CovarianceResult r;
    {
      py::gil_scoped_release rel;
      r = computeCovariance(*engD, camIds, ptIds, o);
    }
    py::dict d;
    if (cross) {
      py::array_t<double> joint({r.n, r.n});
      std::copy(r.joint.begin(), r.joint.end(), joint.mutable_data());
      d["joint"] = joint;
    } else {
      d["joint"] = py::none();
      d["blocks"] = py::array_t<double>((py::ssize_t)r.blocks.size(),
                                        r.blocks.data());
    }
    d["method"] = method;
    d["min_pivot_ratio"] = r.minPivotRatio;
    d["pivot_tol"] = o.pivotTol;
    if (o.method == CovarianceMethod::Dense) {
      py::dict ms;
      ms["form"] = r.formMs;
      ms["factor"] = r.factorMs;
      ms["trailing"] = r.trailingMs;
      ms["solve"] = r.solveMs;
      d["dense_ms"] = ms;
    }
    d["iters"] = py::array_t<int>((py::ssize_t)r.iters.size(), r.iters.data());
    py::array_t<bool> conv((py::ssize_t)r.converged.size());
    for (size_t i = 0; i < r.converged.size(); ++i)
      conv.mutable_data()[i] = r.converged[i] != 0;
    d["converged"] = conv;
    d["asymmetry"] = r.asymmetry;
    d["products"] = r.products;
    return d;
  }
  // Most columns a batched covariance solve carries at once (1: column loop).
  int maxBatch() {
    MEGBA_CHECK(engD || engF, "call build() first");
    return isDouble ? engD->maxBatch() : engF->maxBatch();
  }
  // S X for the columns of X (Engine::schurApplyColumns, a test hook).
  py::array_t<double> schurApply(
      py::array_t<double, py::array::c_style | py::array::forcecast> X,
      bool batched) {
    MEGBA_CHECK(engD, "schur_apply needs a built float64 problem");
    const EngineShape sh = engD->shape();
    MEGBA_CHECK(X.ndim() == 2 &&
                    X.shape(0) == (py::ssize_t)sh.ncam * sh.camDim &&
                    X.shape(1) >= 1,
                "schur_apply: X must be (camDim * ncam, k)");
    const int k = (int)X.shape(1);
    py::array_t<double> out({X.shape(0), X.shape(1)});
    {
      py::gil_scoped_release rel;
      engD->schurApplyColumns(X.data(), k, batched, out.mutable_data());
    }
    return out;
  }
  // The dense S the engine forms for method="dense" (a test hook).
  py::array_t<double> denseSchur() {
    MEGBA_CHECK(engD, "dense_schur needs a built float64 problem");
    const EngineShape sh = engD->shape();
    const py::ssize_t n = (py::ssize_t)sh.ncam * sh.camDim;
    py::array_t<double> out({n, n});
    {
      py::gil_scoped_release rel;
      engD->denseSchurMatrix(out.mutable_data());
    }
    return out;
  }
  // Cholesky of the caller's matrix with the engine's factorization (a test
  // hook): (L, fail_row, min_pivot_ratio).
  py::tuple denseCholesky(
      py::array_t<double, py::array::c_style | py::array::forcecast> A,
      py::object pivotTol) {
    MEGBA_CHECK(engD, "dense_cholesky needs a built float64 problem");
    MEGBA_CHECK(A.ndim() == 2 && A.shape(0) == A.shape(1) && A.shape(0) >= 1,
                "dense_cholesky: A must be square");
    const int n = (int)A.shape(0);
    py::array_t<double> L({A.shape(0), A.shape(1)});
    std::copy(A.data(), A.data() + A.size(), L.mutable_data());
    const double tol = pivotTol.is_none() ? CovarianceOption{}.pivotTol
                                          : py::cast<double>(pivotTol);
    DenseFactorInfo info;
    {
      py::gil_scoped_release rel;
      info = engD->denseCholesky(L.mutable_data(), n, tol);
    }
    return py::make_tuple(L, info.failRow, info.minPivotRatio);
  }
  void updateParams() {
    withEngine([&](auto& e) { e.updateParams(); return 0; });
  }
  double rhoDenominator(double chi2) {
    return withEngine([&](auto& e) { return e.rhoDenominator(chi2); });
  }
  double deltaXL2() { return withEngine([&](auto& e) { return e.deltaXL2(); }); }
  double xL2() { return withEngine([&](auto& e) { return e.xL2(); }); }
  double gInf() { return withEngine([&](auto& e) { return e.gInf(); }); }

  py::tuple getParams() {
    py::array_t<double> cams({prob.ncam, prob.camDim});
    py::array_t<double> pts({prob.npt, prob.ptDim});
    withEngine([&](auto& e) {
      e.getParams(cams.mutable_data(), pts.mutable_data());
      return 0;
    });
    return py::make_tuple(cams, pts);
  }

  py::dict dump() {
    DenseDump dd = withEngine([&](auto& e) { return e.dump(); });
    py::dict d;
    auto toArr = [](std::vector<double>& v) {
      return py::array_t<double>((py::ssize_t)v.size(), v.data());
    };
    d["e0"] = dd.e0;
    d["e1"] = dd.e1;
    d["r"] = toArr(dd.r);
    d["Jc"] = toArr(dd.Jc);
    d["Jp"] = toArr(dd.Jp);
    d["Hpp"] = toArr(dd.Hpp);
    d["Hll"] = toArr(dd.Hll);
    d["Hpl"] = toArr(dd.Hpl);
    d["g"] = toArr(dd.g);
    d["deltaX"] = toArr(dd.deltaX);
    return d;
  }

  py::dict indexInfo() {
    py::dict d;
    d["ncam"] = ix.ncam;
    d["npt"] = ix.npt;
    d["nobs"] = ix.nobs;
    d["cam_of"] = py::array_t<int>((py::ssize_t)ix.camOf.size(), ix.camOf.data());
    d["pt_of"] = py::array_t<int>((py::ssize_t)ix.ptOf.size(), ix.ptOf.data());
    d["pt_rowptr"] =
        py::array_t<int64_t>((py::ssize_t)ix.ptRowPtr.size(), ix.ptRowPtr.data());
    d["pt_split"] = py::array_t<int>((py::ssize_t)ix.ptSplit.size(), ix.ptSplit.data());
    d["split"] = py::array_t<int64_t>((py::ssize_t)ix.split.size(), ix.split.data());
    d["perm"] = py::array_t<int64_t>((py::ssize_t)ix.perm.size(), ix.perm.data());
    return d;
  }
};

}  // namespace

namespace {

PyJetVec mkJv(py::array_t<double, py::array::c_style | py::array::forcecast> value,
              py::object grad, int N, int grad_pos, bool gpu) {
  const int64_t n = value.size();
  const double* gptr = nullptr;
  py::array_t<double, py::array::c_style | py::array::forcecast> garr;
  if (!grad.is_none()) {
    garr = py::cast<py::array_t<double, py::array::c_style | py::array::forcecast>>(grad);
    MEGBA_CHECK(garr.size() == (py::ssize_t)(N * n), "grad must be (N, nItem)");
    gptr = garr.data();
  }
  return PyJetVec{jvFromHost<double>(value.data(), gptr, n, N, grad_pos, gpu)};
}

py::tuple jvDownload(const PyJetVec& a) {
  py::array_t<double> value((py::ssize_t)a.v.nItem);
  py::array_t<double> grad({(py::ssize_t)a.v.N, (py::ssize_t)a.v.nItem});
  jvToHost<double>(a.v, value.mutable_data(), grad.mutable_data());
  return py::make_tuple(value, grad);
}

std::vector<JetVec<double>> jvList(py::sequence seq) {
  std::vector<JetVec<double>> out;
  for (auto h : seq) out.push_back(py::cast<PyJetVec&>(h).v);
  return out;
}

py::list jvWrap(const std::vector<JetVec<double>>& vs) {
  py::list out;
  for (const auto& v : vs) out.append(PyJetVec{v});
  return out;
}

CustomForward<double> PyProblem::wrapCustomForward(py::object fn) {
  if (fn.is_none()) return nullptr;
  auto holder = std::make_shared<py::object>(std::move(fn));
  return [holder](const std::vector<JetVec<double>>& camL,
                  const std::vector<JetVec<double>>& ptL,
                  const std::vector<JetVec<double>>& meas,
                  std::vector<JetVec<double>>& res) {
    py::gil_scoped_acquire gil;
    py::list c, p, m;
    for (const auto& v : camL) c.append(PyJetVec{v});
    for (const auto& v : ptL) p.append(PyJetVec{v});
    for (const auto& v : meas) m.append(PyJetVec{v});
    py::object out = (*holder)(c, p, m);
    py::sequence seq = py::cast<py::sequence>(out);
    res.clear();
    for (auto h : seq) res.push_back(py::cast<PyJetVec&>(h).v);
  };
}

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "megba_amd core (MI355X-native distributed bundle adjustment)";

  py::class_<PyJetVec>(m, "JetVector")
      .def(py::init(&mkJv), py::arg("value"), py::arg("grad") = py::none(),
           py::arg("N") = 0, py::arg("grad_pos") = -1, py::arg("gpu") = false)
      .def_property_readonly("n_item", [](const PyJetVec& a) { return a.v.nItem; })
      .def_property_readonly("N", [](const PyJetVec& a) { return a.v.N; })
      .def("to_numpy", &jvDownload);
  m.def("jv_scalar", [](double s, int N) { return PyJetVec{jvScalar<double>(s, N)}; });
  m.def("jv_pool_trim", []() { jvPoolTrim(); });
  m.def("jv_add", [](const PyJetVec& a, const PyJetVec& b) { return PyJetVec{jvBinary(JvOp::Add, a.v, b.v)}; });
  m.def("jv_sub", [](const PyJetVec& a, const PyJetVec& b) { return PyJetVec{jvBinary(JvOp::Sub, a.v, b.v)}; });
  m.def("jv_mul", [](const PyJetVec& a, const PyJetVec& b) { return PyJetVec{jvBinary(JvOp::Mul, a.v, b.v)}; });
  m.def("jv_div", [](const PyJetVec& a, const PyJetVec& b) { return PyJetVec{jvBinary(JvOp::Div, a.v, b.v)}; });
  m.def("jv_neg", [](const PyJetVec& a) { return PyJetVec{jvUnary(JvUnary::Neg, a.v)}; });
  m.def("jv_abs", [](const PyJetVec& a) { return PyJetVec{jvUnary(JvUnary::Abs, a.v)}; });
  m.def("jv_sin", [](const PyJetVec& a) { return PyJetVec{jvUnary(JvUnary::Sin, a.v)}; });
  m.def("jv_cos", [](const PyJetVec& a) { return PyJetVec{jvUnary(JvUnary::Cos, a.v)}; });
  m.def("jv_sqrt", [](const PyJetVec& a) { return PyJetVec{jvUnary(JvUnary::Sqrt, a.v)}; });
  m.def("jv_angle_axis_to_rotation", [](py::sequence aa) { return jvWrap(jvAngleAxisToRotation(jvList(aa))); });
  m.def("jv_normalize_angle", [](const PyJetVec& t) { return PyJetVec{jvNormalizeAngle(t.v)}; });
  m.def("jv_rotation2d", [](const PyJetVec& t) { return jvWrap(jvRotation2D(t.v)); });
  m.def("jv_quaternion_to_rotation", [](py::sequence q) { return jvWrap(jvQuaternionToRotation(jvList(q))); });
  m.def("jv_rotation_to_quaternion", [](py::sequence R) { return jvWrap(jvRotationToQuaternion(jvList(R))); });
  m.def("jv_normalize_quaternion", [](py::sequence q) { return jvWrap(jvNormalizeQuaternion(jvList(q))); });
  m.def("jv_radial_distortion", [](py::sequence p, py::sequence intr) { return PyJetVec{jvRadialDistortion(jvList(p), jvList(intr))}; });

  py::class_<PyProblem>(m, "Problem")
      .def(py::init<py::array_t<double, py::array::c_style | py::array::forcecast>,
                    py::array_t<double, py::array::c_style | py::array::forcecast>,
                    py::array_t<int, py::array::c_style | py::array::forcecast>,
                    py::array_t<int, py::array::c_style | py::array::forcecast>,
                    py::array_t<double, py::array::c_style | py::array::forcecast>,
                    py::object, py::object, py::object>(),
           py::arg("cams"), py::arg("pts"), py::arg("cam_idx"),
           py::arg("pt_idx"), py::arg("meas"), py::arg("info") = py::none(),
           py::arg("cam_fixed") = py::none(), py::arg("pt_fixed") = py::none())
      .def("build", &PyProblem::build, py::arg("device") = "cpu",
           py::arg("dtype") = "float64", py::arg("rank") = 0,
           py::arg("world_size") = 1, py::arg("device_index") = 0,
           py::arg("diff") = "auto", py::arg("schur") = "explicit",
           py::arg("loss") = "none", py::arg("loss_delta") = 1.0,
           py::arg("allreduce") = py::none(), py::arg("rccl_id") = py::none(),
           py::arg("custom_forward") = py::none(),
           py::arg("intrinsics") = py::none())
      .def("set_prior", &PyProblem::setPrior, py::arg("kind"), py::arg("idx"),
           py::arg("mean"), py::arg("info") = py::none())
      .def("solve", &PyProblem::solve, py::arg("max_iter") = 20,
           py::arg("tau") = 1e4, py::arg("epsilon1") = 1.0,
           py::arg("epsilon2") = 1e-10, py::arg("solver_max_iter") = 100,
           py::arg("solver_tol") = 1e-1, py::arg("solver_refuse_ratio") = 1.0,
           py::arg("force_iterations") = false, py::arg("verbose") = true)
      .def("lm_init", &PyProblem::lmInit, py::arg("max_iter") = 1000000,
           py::arg("tau") = 1e4, py::arg("epsilon1") = 1.0,
           py::arg("epsilon2") = 1e-10, py::arg("solver_max_iter") = 100,
           py::arg("solver_tol") = 1e-1, py::arg("solver_refuse_ratio") = 1.0,
           py::arg("force_iterations") = false, py::arg("verbose") = false)
      .def("lm_step", &PyProblem::lmStep)
      .def("forward", &PyProblem::forward)
      .def("accept_forward", &PyProblem::acceptForward)
      .def("build_linear_system", &PyProblem::buildLinearSystem)
      .def("process_diag", &PyProblem::processDiag)
      .def("solve_linear", &PyProblem::solveLinear, py::arg("max_iter") = 100,
           py::arg("tol") = 1e-1, py::arg("refuse_ratio") = 1.0,
           py::arg("rel_tol") = 0.0)
      .def("covariance", &PyProblem::covariance, py::arg("cam_idx"),
           py::arg("pt_idx"), py::arg("tol") = 1e-10,
           py::arg("max_iter") = 2000, py::arg("strict") = true,
           py::arg("batch") = 1, py::arg("method") = "pcg",
           py::arg("pivot_tol") = py::none(), py::arg("cross") = true)
      .def("max_batch", &PyProblem::maxBatch)
      .def("dense_schur", &PyProblem::denseSchur)
      .def("dense_cholesky", &PyProblem::denseCholesky, py::arg("A"),
           py::arg("pivot_tol") = py::none())
      .def("schur_apply", &PyProblem::schurApply, py::arg("X"),
           py::arg("batched") = true)
      .def("update_params", &PyProblem::updateParams)
      .def("rho_denominator", &PyProblem::rhoDenominator)
      .def("delta_x_l2", &PyProblem::deltaXL2)
      .def("x_l2", &PyProblem::xL2)
      .def("g_inf", &PyProblem::gInf)
      .def("get_params", &PyProblem::getParams)
      .def("dump", &PyProblem::dump)
      .def("index_info", &PyProblem::indexInfo);

  // Debug view of the GPU engine's host-built edge tables for one rank of a
  // (cam_idx, pt_idx) problem; runs on the host only.
  m.def(
      "gpu_edge_tables",
      [](py::array_t<int, py::array::c_style | py::array::forcecast> camIdx,
         py::array_t<int, py::array::c_style | py::array::forcecast> ptIdx,
         int ncam, int npt, int rank, int world, int chunkRows, int bandPts) {
        MEGBA_CHECK(camIdx.size() == ptIdx.size(), "index array size mismatch");
        MEGBA_CHECK(rank >= 0 && rank < world, "rank out of range");
        MEGBA_CHECK(chunkRows >= 1, "chunk_rows must be positive");
        BAProblemHost p;
        p.ncam = ncam;
        p.npt = npt;
        p.nobs = camIdx.size();
        p.camIdx.assign(camIdx.data(), camIdx.data() + p.nobs);
        p.ptIdx.assign(ptIdx.data(), ptIdx.data() + p.nobs);
        p.meas.assign((size_t)p.nobs * p.resDim, 0.0);
        const ProblemIndex ix = buildIndex(p, world);
        const int64_t e0 = ix.split[rank], e1 = ix.split[rank + 1];
        const int ptLo = ix.ptSplit[rank], ptHi = ix.ptSplit[rank + 1];
        const CamChunks c =
            buildCamChunks(ix, e0, e1, ncam, npt, chunkRows, bandPts);
        const RunWindows w = buildRunWindows(ix, e0, ptLo, ptHi);
        const auto arr = [](const auto& v) {
          using U = typename std::decay_t<decltype(v)>::value_type;
          return py::array_t<U>((py::ssize_t)v.size(), v.data());
        };
        py::dict d;
        d["e0"] = e0;
        d["e1"] = e1;
        d["pt_lo"] = ptLo;
        d["pt_hi"] = ptHi;
        // the rank's edges in primary (pt, cam)-sorted order
        d["cam_of"] = arr(std::vector<int>(ix.camOf.begin() + e0,
                                           ix.camOf.begin() + e1));
        d["pt_of"] = arr(std::vector<int>(ix.ptOf.begin() + e0,
                                          ix.ptOf.begin() + e1));
        d["cam_pos"] = arr(c.camPos);
        d["pt_of_cam"] = arr(c.ptOfCam);
        d["ch_cam"] = arr(c.chCam);
        d["ch_lo"] = arr(c.chLo);
        d["ch_hi"] = arr(c.chHi);
        d["win_lo"] = arr(w.winLo);
        d["win_hi"] = arr(w.winHi);
        d["win_flag"] = arr(w.winFlag);
        d["flag_wins"] = arr(w.flagWins);
        d["long_pts"] = arr(w.longPts);
        return d;
      },
      py::arg("cam_idx"), py::arg("pt_idx"), py::arg("ncam"), py::arg("npt"),
      py::arg("rank") = 0, py::arg("world") = 1, py::arg("chunk_rows") = 256,
      py::arg("band_pts") = 0);

  // Slot function of the recompute product's LDS tile (rc_tile.hpp): byte
  // offset of 16-byte chunk `chunk` of tile row `row`; host only.
  m.def(
      "rc_tile_slot",
      [](int row, int chunk) {
        MEGBA_CHECK(row >= 0 && row < kRcTileRows, "row out of range");
        MEGBA_CHECK(chunk >= 0 && chunk < kRcSegChunks, "chunk out of range");
        return rcTileSlot(row, chunk);
      },
      py::arg("row"), py::arg("chunk"));
  m.attr("rc_tile_bytes") = kRcTileBytes;
  // Dynamic LDS the staged instance needs for nc accumulators of elem_bytes
  // each and `waves` waves per workgroup.
  m.def(
      "rc_staged_lds_bytes",
      [](long long nc, int elemBytes, int waves) {
        return rcStagedLdsBytes(nc, elemBytes, waves);
      },
      py::arg("nc"), py::arg("elem_bytes"), py::arg("waves"));

  // The GPU engine's choice of the Schur product and its PCG plan
  // (schur_plan.hpp) as pure functions: the knobs are keywords, the probe
  // launches and timings arguments; nothing reads the environment or a device.
  py::enum_<SchurPath>(m, "SchurPath")
      .value("Lds", SchurPath::Lds)
      .value("LdsRecompute", SchurPath::LdsRecompute)
      .value("FusedEtx", SchurPath::FusedEtx)
      .value("Separate", SchurPath::Separate)
      .value("OnePass", SchurPath::OnePass);
  m.def("schur_path_name", &schurPathName);
  // -> (path or None for "time the candidates", probe launches made in
  // order, whether lds / lds-recompute are candidates afterwards)
  m.def(
      "schur_path_untimed",
      [](long long nL, bool ldsEligible, bool rcEligible, bool ldsLaunches,
         bool rcLaunches, bool etxFuse, bool noEtxFuse, bool schurLds,
         bool schurRecompute) {
        GpuKnobs k;
        k.etxFuse = etxFuse;
        k.noEtxFuse = noEtxFuse;
        k.schurLds = schurLds;
        k.schurRecompute = schurRecompute;
        std::vector<SchurPath> probes;
        const SchurUntimed u = schurPathUntimed(
            schurCandidates(k, ldsEligible, rcEligible, nL), [&](SchurPath p) {
              probes.push_back(p);
              return p == SchurPath::Lds ? ldsLaunches : rcLaunches;
            });
        return py::make_tuple(u.path, probes, u.lds, u.rc);
      },
      py::arg("n_local_edges"), py::arg("lds_eligible"),
      py::arg("rc_eligible"), py::arg("lds_launches") = true,
      py::arg("rc_launches") = true, py::arg("etxfuse") = false,
      py::arg("no_etxfuse") = false, py::arg("schur_lds") = false,
      py::arg("schur_recompute") = false);
  // ms = [fused-etx, separate, lds, lds-recompute]
  m.def(
      "schur_path_from_timings",
      [](std::array<float, 4> ms, bool ldsTimed, bool rcTimed) {
        return schurPathFromTimings(ms.data(), ldsTimed, rcTimed);
      },
      py::arg("ms"), py::arg("lds_timed"), py::arg("rc_timed"));
  // -> (path, rotatedBody, productReadsPad, mergeReduceBApply)
  m.def(
      "pcg_plan",
      [](SchurPath tuned, bool implicit, int nLongPts, bool allreduceIsNoop,
         bool fused, bool noPcgFuse) {
        GpuKnobs k;
        k.fused = fused;
        k.noPcgFuse = noPcgFuse;
        const PcgPlan p =
            makePcgPlan(tuned, k, implicit, nLongPts, allreduceIsNoop);
        return py::make_tuple(p.path, p.rotatedBody, p.productReadsPad,
                              p.mergeReduceBApply);
      },
      py::arg("tuned"), py::arg("implicit"), py::arg("n_long_pts"),
      py::arg("allreduce_is_noop"), py::arg("fused") = false,
      py::arg("no_pcg_fuse") = false);

#ifdef MEGBA_WITH_GPU
  m.attr("has_gpu_support") = true;
  m.def("rccl_unique_id", []() { return py::bytes(rcclUniqueIdString()); });
  m.def("rccl_preflight",
        [](py::bytes id, int rank, int world, int deviceIndex,
           double timeoutSec) {
          std::string s = id;
          py::gil_scoped_release rel;
          return rcclPreflight(s, rank, world, deviceIndex, timeoutSec);
        },
        py::arg("id"), py::arg("rank"), py::arg("world"),
        py::arg("device_index") = 0, py::arg("timeout_sec") = 120.0);
  m.def("hip_device_count", []() { return hipDeviceCountSafe(); });
  m.def("device_synchronize", []() {
    py::gil_scoped_release rel;
    deviceSynchronize();
  });
  m.def("hip_mem_info", []() {
    auto p = hipMemInfoSafe();
    return py::make_tuple(p.first, p.second);
  });
#else
  m.attr("has_gpu_support") = false;
#endif
}
