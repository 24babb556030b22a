// Native C++ example of Gaussian unary priors: georeferencing a
// reconstruction with GPS-style camera-centre priors plus one ground control
// point and one camera parameter prior.
//
// Reprojection error is blind to a rigid translation of the whole scene
// (X += d, t -= R d), so a bundle adjustment without priors leaves a shifted
// start shifted.  This example shifts a BAL problem by d, puts a centre
// prior at every camera's original centre, and checks that
//   * the graph API (CameraCenterPriorEdge / PointPriorEdge /
//     CameraPriorEdge) and the array API (BAProblemHost::*Prior) give the
//     same LM trajectory, and
//   * the solved centres end closer to the prior centres than |d|
// -- a self-verifying example.
//
// Build: python build.py            (emits examples/bal_priors_cpp)
// Run:   examples/bal_priors_cpp --path problem.txt [--device gpu|cpu]
#include <cmath>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "megba/common.hpp"
#include "megba/cpu_engine.hpp"
#include "megba/graph_api.hpp"
#include "megba/lm.hpp"
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

static std::vector<double> centres(const std::vector<double>& cams, int ncam) {
  std::vector<double> c((size_t)ncam * 3);
  double J[18];
  for (int i = 0; i < ncam; ++i) cameraCentre<double>(&cams[9 * i], &c[3 * i], J);
  return c;
}

static double meanDist(const std::vector<double>& a,
                       const std::vector<double>& b) {
  double s = 0;
  const size_t n = a.size() / 3;
  for (size_t i = 0; i < n; ++i)
    s += std::sqrt(std::pow(a[3 * i] - b[3 * i], 2) +
                   std::pow(a[3 * i + 1] - b[3 * i + 1], 2) +
                   std::pow(a[3 * i + 2] - b[3 * i + 2], 2));
  return s / (double)n;
}

int main(int argc, char** argv) {
  std::string path, device = "gpu";
  int maxIter = 10;
  for (int i = 1; i < argc; ++i) {
    auto arg = [&](const char* name) {
      return std::strcmp(argv[i], name) == 0 && i + 1 < argc;
    };
    if (arg("--path")) path = argv[++i];
    else if (arg("--device")) device = argv[++i];
    else if (arg("--max_iter")) maxIter = std::atoi(argv[++i]);
    else path.clear(), i = argc;
  }
  if (path.empty()) {
    std::cerr << "usage: bal_priors_cpp --path problem.txt "
                 "[--device gpu|cpu] [--max_iter N]\n";
    return 2;
  }
  BAProblemHost raw = loadBal(path);
  std::cout << "problem: " << raw.ncam << " cams, " << raw.npt << " pts, "
            << raw.nobs << " obs; device=" << device << "\n";

  // GPS fixes and one surveyed point, taken before the scene is shifted.
  const std::vector<double> gps = centres(raw.cams, raw.ncam);
  const std::vector<double> gcp(raw.pts.begin(), raw.pts.begin() + 3);
  const std::vector<double> cam0(raw.cams.begin(), raw.cams.begin() + 9);

  // Rigid translation: X += d, t -= R d leaves every reprojection unchanged.
  const double d[3] = {5.0, -3.0, 2.0};
  const double dNorm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int i = 0; i < raw.npt; ++i)
    for (int k = 0; k < 3; ++k) raw.pts[3 * i + k] += d[k];
  for (int i = 0; i < raw.ncam; ++i) {
    using J0 = Jet<double, 1>;
    J0 aa[3], dv[3], Rd[3];
    for (int k = 0; k < 3; ++k) {
      aa[k] = J0(raw.cams[9 * i + k]);
      dv[k] = J0(d[k]);
    }
    angleAxisRotatePoint<double, J0>(aa, dv, Rd);
    for (int k = 0; k < 3; ++k) raw.cams[9 * i + 3 + k] -= Rd[k].v;
  }

  const std::vector<double> gpsInfo = {1e4, 0, 0, 1e4, 0, 1e4};
  std::vector<double> camInfo;  // weak diagonal prior on camera 0's block
  for (int i = 0; i < 9; ++i)
    for (int j = i; j < 9; ++j) camInfo.push_back(i == j ? 1e-2 : 0.0);

  ProblemOption opt;
  opt.device = device == "cpu" ? Device::CPU : Device::GPU;
  AlgoOptionLM algo;
  algo.maxIter = maxIter;
  algo.verbose = false;
  SolverOptionPCG sopt;
  sopt.maxIter = 100;
  sopt.tol = 1e-8;
  sopt.refuseRatio = 1e6;

  // --- graph API ----------------------------------------------------------
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
        .setMeasurement({gps[3 * i], gps[3 * i + 1], gps[3 * i + 2]})
        .setInformation(gpsInfo);
    graph.appendEdge(e);
  }
  {
    PointPriorEdge e;  // identity information
    e.appendVertex(&ptVs[0]).setMeasurement(gcp);
    graph.appendEdge(e);
    CameraPriorEdge c;
    c.appendVertex(&camVs[0]).setMeasurement(cam0).setInformation(camInfo);
    graph.appendEdge(c);
  }
  const LMReport viaGraph = graph.solve(opt, algo, sopt);

  // --- array API ----------------------------------------------------------
  BAProblemHost prob = raw;
  for (int i = 0; i < raw.ncam; ++i) {
    prob.centerPrior.idx.push_back(i);
    prob.centerPrior.info.insert(prob.centerPrior.info.end(), gpsInfo.begin(),
                                 gpsInfo.end());
  }
  prob.centerPrior.mean = gps;
  prob.ptPrior.idx = {0};
  prob.ptPrior.mean = gcp;
  prob.camPrior.idx = {0};
  prob.camPrior.mean = cam0;
  prob.camPrior.info = camInfo;
  validatePriors(prob, false);
  const ProblemIndex ix = buildIndex(prob, 1);
  std::unique_ptr<Engine<double>> eng;
  if (opt.device == Device::CPU)
    eng = makeCpuEngine<double>(prob, ix, opt, nullptr, nullptr);
  else
    eng = makeGpuEngine<double>(prob, ix, opt, std::string(), nullptr);
  const LMReport viaArrays = runLM<double>(*eng, algo, sopt);

  MEGBA_CHECK(viaGraph.iters.size() == viaArrays.iters.size(),
              "trajectory length mismatch");
  for (size_t k = 0; k < viaGraph.iters.size(); ++k) {
    const double r =
        std::fabs(viaGraph.iters[k].chi2 - viaArrays.iters[k].chi2) /
        std::max(viaArrays.iters[k].chi2, 1e-30);
    MEGBA_CHECK(r < 1e-9, "graph/array trajectories differ at iter " +
                              std::to_string(k));
  }
  MEGBA_CHECK(viaGraph.finalChi2 < viaGraph.iters[0].chi2,
              "the solve did not reduce chi2");

  std::vector<double> solved((size_t)raw.ncam * 9);
  for (int i = 0; i < raw.ncam; ++i)
    for (int k = 0; k < 9; ++k) solved[9 * i + k] = camVs[i].estimation[k];
  const double before = meanDist(centres(raw.cams, raw.ncam), gps);
  const double after = meanDist(centres(solved, raw.ncam), gps);
  std::cout << "chi2 " << viaGraph.iters[0].chi2 << " -> "
            << viaGraph.finalChi2 << "\n";
  std::cout << "mean centre distance to GPS: " << before << " -> " << after
            << " (|d| = " << dNorm << ")\n";
  MEGBA_CHECK(after < dNorm, "centre priors did not pull the cameras back");
  std::cout << "PRIORS_OK\n";
  return 0;
}
