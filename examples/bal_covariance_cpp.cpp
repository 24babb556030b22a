// Native C++ example of marginal covariances: "how good are these camera
// positions?" for a scene georeferenced with GPS-style camera-centre priors.
//
// The covariance of a vertex is its diagonal block of H^-1, H the
// Gauss-Newton Hessian with the prior terms (covariance.hpp).  This example
// puts a centre prior on every camera of a BAL problem, which fixes the
// gauge, and checks that
//   * the graph API (GraphProblem::covariance) and the driver over an
//     array-built engine (computeCovariance) give the same matrix,
//   * the dense Cholesky route (CovarianceMethod::Dense) agrees with the PCG,
//   * every variance on the diagonal is positive, and
//   * priors 100x tighter shrink the variance of every camera centre,
//     J_C Sigma J_C^T with J_C the centre's Jacobian,
// -- a self-verifying example.
//
// Build: python build.py            (emits examples/bal_covariance_cpp)
// Run:   examples/bal_covariance_cpp --path problem.txt [--device gpu|cpu]
#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "megba/common.hpp"
#include "megba/covariance.hpp"
#include "megba/cpu_engine.hpp"
#include "megba/graph_api.hpp"
#include "megba/prior.hpp"
#include "megba/problem.hpp"

using namespace megba;

static BAProblemHost loadBal(const std::string& path) {
  std::ifstream f(path);
  MEGBA_CHECK(f.good(), "cannot open " + path);
  BAProblemHost p;
  f >> p.ncam >> p.npt >> p.nobs;
  p.camIdx.resize(p.nobs);
  p.ptIdx.resize(p.nobs);
  p.meas.resize(p.nobs * 2);
  for (int64_t i = 0; i < p.nobs; ++i)
    f >> p.camIdx[i] >> p.ptIdx[i] >> p.meas[2 * i] >> p.meas[2 * i + 1];
  p.cams.resize((size_t)p.ncam * 9);
  for (auto& v : p.cams) f >> v;
  p.pts.resize((size_t)p.npt * 3);
  for (auto& v : p.pts) f >> v;
  MEGBA_CHECK(f.good() || f.eof(), "truncated BAL file");
  return p;
}

// The problem with a centre prior of information w * I at every camera's
// current centre.
static BAProblemHost withCentrePriors(const BAProblemHost& raw, double w) {
  BAProblemHost prob = raw;
  for (int i = 0; i < raw.ncam; ++i) {
    double C[3], J[18];
    cameraCentre<double>(&raw.cams[9 * i], C, J);
    prob.centerPrior.idx.push_back(i);
    prob.centerPrior.mean.insert(prob.centerPrior.mean.end(), C, C + 3);
    for (double v : {w, 0.0, 0.0, w, 0.0, w}) prob.centerPrior.info.push_back(v);
  }
  validatePriors(prob, false);
  return prob;
}

// Covariance of every camera block and of point 0 through the driver.
static CovarianceResult viaDriver(
    const BAProblemHost& prob, const ProblemOption& opt, int batch = 1,
    CovarianceMethod method = CovarianceMethod::Pcg, bool cross = true) {
  const ProblemIndex ix = buildIndex(prob, 1);
  std::unique_ptr<Engine<double>> eng;
  if (opt.device == Device::CPU)
    eng = makeCpuEngine<double>(prob, ix, opt, nullptr, nullptr);
  else
    eng = makeGpuEngine<double>(prob, ix, opt, std::string(), nullptr);
  std::vector<int> cams(prob.ncam);
  for (int i = 0; i < prob.ncam; ++i) cams[i] = i;
  CovarianceOption copt;
  copt.batch = batch;
  copt.method = method;
  copt.cross = cross;
  return computeCovariance(*eng, cams, {0}, copt);
}

// diag(J_C Sigma_cam J_C^T) of camera i: the variances of its centre.
static void centreVariance(const BAProblemHost& prob,
                           const CovarianceResult& cov, int i, double out[3]) {
  double C[3], J[18];
  cameraCentre<double>(&prob.cams[9 * i], C, J);
  for (int a = 0; a < 3; ++a) {
    out[a] = 0.0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c)
        out[a] += J[a * 6 + r] * J[a * 6 + c] *
                  cov.joint[(size_t)(9 * i + r) * cov.n + 9 * i + c];
  }
}

int main(int argc, char** argv) {
  std::string path, device = "gpu";
  for (int i = 1; i < argc; ++i) {
    auto arg = [&](const char* name) {
      return std::strcmp(argv[i], name) == 0 && i + 1 < argc;
    };
    if (arg("--path")) path = argv[++i];
    else if (arg("--device")) device = argv[++i];
    else path.clear(), i = argc;
  }
  if (path.empty()) {
    std::cerr << "usage: bal_covariance_cpp --path problem.txt "
                 "[--device gpu|cpu]\n";
    return 2;
  }
  const BAProblemHost raw = loadBal(path);
  std::cout << "problem: " << raw.ncam << " cams, " << raw.npt << " pts, "
            << raw.nobs << " obs; device=" << device << "\n";
  ProblemOption opt;
  opt.device = device == "cpu" ? Device::CPU : Device::GPU;
  const double w = 1e2;

  // --- array API + driver --------------------------------------------------
  const BAProblemHost loose = withCentrePriors(raw, w);
  const CovarianceResult covLoose = viaDriver(loose, opt);
  const CovarianceResult covTight =
      viaDriver(withCentrePriors(raw, 100.0 * w), opt);
  const int n = covLoose.n;
  MEGBA_CHECK(n == 9 * raw.ncam + 3, "unexpected covariance size");

  // --- graph API -----------------------------------------------------------
  std::vector<BaseVertex> camVs, ptVs;
  camVs.reserve(raw.ncam);
  ptVs.reserve(raw.npt);
  for (int i = 0; i < raw.ncam; ++i)
    camVs.emplace_back(VertexKind::CAMERA, &raw.cams[9 * i]);
  for (int i = 0; i < raw.npt; ++i)
    ptVs.emplace_back(VertexKind::POINT, &raw.pts[3 * i]);
  GraphProblem graph;
  for (auto& v : camVs) graph.appendVertex(&v);
  for (auto& v : ptVs) graph.appendVertex(&v);
  for (int64_t k = 0; k < raw.nobs; ++k) {
    ReprojectionEdge e;
    e.appendVertex(&camVs[raw.camIdx[k]])
        .appendVertex(&ptVs[raw.ptIdx[k]])
        .setMeasurement(raw.meas[2 * k], raw.meas[2 * k + 1]);
    graph.appendEdge(e);
  }
  for (int i = 0; i < raw.ncam; ++i) {
    CameraCenterPriorEdge e;
    e.appendVertex(&camVs[i])
        .setMeasurement({loose.centerPrior.mean[3 * i],
                         loose.centerPrior.mean[3 * i + 1],
                         loose.centerPrior.mean[3 * i + 2]})
        .setInformation({w, 0, 0, w, 0, w});
    graph.appendEdge(e);
  }
  // the point first: the graph result follows the order of the request
  std::vector<BaseVertex*> request = {&ptVs[0]};
  for (auto& v : camVs) request.push_back(&v);
  const CovarianceResult covGraph = graph.covariance(request, opt);
  MEGBA_CHECK(covGraph.n == n, "graph covariance size mismatch");

  double scale = 0.0, diff = 0.0;
  for (double v : covLoose.joint) scale = std::max(scale, std::fabs(v));
  const auto inGraph = [&](int i) { return i < n - 3 ? i + 3 : i - (n - 3); };
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      diff = std::max(
          diff, std::fabs(covLoose.joint[(size_t)i * n + j] -
                          covGraph.joint[(size_t)inGraph(i) * n + inGraph(j)]));
  std::cout << "graph vs driver: max difference " << diff << " of " << scale
            << "; asymmetry " << covLoose.asymmetry << "\n";
  MEGBA_CHECK(diff <= 1e-9 * scale, "graph and driver covariances differ");

  // --- batched columns ------------------------------------------------------
  // batch = camDim solves the 9 columns of a camera block together where the
  // engine has a batched product (the GPU engine's matrix-free mode); any
  // other engine runs the column loop.  Either way the matrix is the same.
  ProblemOption optImplicit = opt;
  optImplicit.schur = SchurMode::IMPLICIT;
  const CovarianceResult covOne = viaDriver(loose, optImplicit, 1);
  const CovarianceResult covBatch = viaDriver(loose, optImplicit, raw.camDim);
  double diffBatch = 0.0;
  for (size_t i = 0; i < covOne.joint.size(); ++i)
    diffBatch =
        std::max(diffBatch, std::fabs(covOne.joint[i] - covBatch.joint[i]));
  std::cout << "batch=" << raw.camDim << " vs batch=1: max difference "
            << diffBatch << " of " << scale << "; Schur products "
            << covBatch.products << " vs " << covOne.products << "\n";
  MEGBA_CHECK(diffBatch <= 1e-9 * scale,
              "batched and column-loop covariances differ");
  MEGBA_CHECK(covBatch.products <= covOne.products,
              "the batched run applied more Schur products");

  // --- dense Cholesky of the Schur complement -------------------------------
  // method = Dense factors the camera system once and solves every column
  // exactly; it must agree with the PCG result.  With cross = false only the
  // vertices' own blocks come back.
  const CovarianceResult covDense =
      viaDriver(loose, opt, 1, CovarianceMethod::Dense);
  double diffDense = 0.0;
  for (size_t i = 0; i < covLoose.joint.size(); ++i)
    diffDense =
        std::max(diffDense, std::fabs(covLoose.joint[i] - covDense.joint[i]));
  std::cout << "dense vs pcg: max difference " << diffDense << " of " << scale
            << "; min pivot ratio " << covDense.minPivotRatio << "\n";
  MEGBA_CHECK(diffDense <= 1e-9 * scale, "dense and PCG covariances differ");
  MEGBA_CHECK(covDense.products == 0, "the dense route applied a product");
  const CovarianceResult covOwn =
      viaDriver(loose, opt, 1, CovarianceMethod::Dense, /*cross=*/false);
  MEGBA_CHECK(covOwn.joint.empty() &&
                  covOwn.blocks.size() == (size_t)81 * raw.ncam + 9,
              "cross = false must return the blocks alone");
  double diffOwn = 0.0;
  for (int c = 0; c < raw.ncam; ++c)
    for (int r = 0; r < 9; ++r)
      for (int k = 0; k < 9; ++k)
        diffOwn = std::max(
            diffOwn,
            std::fabs(covOwn.blocks[(size_t)81 * c + 9 * r + k] -
                      covDense.joint[(size_t)(9 * c + r) * n + 9 * c + k]));
  MEGBA_CHECK(diffOwn <= 1e-12 * scale, "cross = false blocks differ");

  for (int i = 0; i < n; ++i)
    MEGBA_CHECK(covLoose.joint[(size_t)i * n + i] > 0.0,
                "non-positive variance at row " + std::to_string(i));

  double worst = 0.0;
  for (int i = 0; i < raw.ncam; ++i) {
    double a[3], b[3];
    centreVariance(raw, covLoose, i, a);
    centreVariance(raw, covTight, i, b);
    for (int k = 0; k < 3; ++k) {
      MEGBA_CHECK(b[k] > 0.0 && b[k] < a[k],
                  "tighter priors did not shrink the centre variance of "
                  "camera " + std::to_string(i));
      worst = std::max(worst, b[k] / a[k]);
    }
  }
  std::cout << "centre std of camera 0: " << [&] {
    double a[3];
    centreVariance(raw, covLoose, 0, a);
    return std::sqrt(a[0] + a[1] + a[2]);
  }() << "; tight/loose variance ratio at most " << worst << "\n";
  std::cout << "COVARIANCE_OK\n";
  return 0;
}
