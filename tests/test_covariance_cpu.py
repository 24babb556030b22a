"""Marginal covariances (covariance.hpp) on the CPU engine: unit right-hand
side Schur PCG solves against the numpy inverse of the dense Hessian, fixed
vertices, a missing datum, the state a running LM session keeps, the relative
stop of solve_linear, the errors, and the graph and C++ forms."""
import numpy as np
import pytest

import megba_amd as mb
from covariance_common import (CAM_IDX, CPU_BOUND, PT_IDX, block_scaled_error,
                               check_against_oracle, dense_hessian, linearise,
                               lm_run, make, oracle, request_rows,
                               run_cpp_covariance)
from priors_common import INTR, bal_case, case_632, make_priors, with_priors


# ---- dense oracle ----------------------------------------------------------
@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_oracle_bal(schur):
    params, _ = oracle("bal")
    check_against_oracle(make("bal", schur=schur, params=params), "bal",
                         CPU_BOUND)


def test_oracle_632():
    params, _ = oracle("632")
    check_against_oracle(make("632", params=params), "632", CPU_BOUND)


# ---- fixed vertices --------------------------------------------------------
def test_fixed_vertices():
    """Two fixed cameras are the datum.  A fixed vertex has zero rows and
    columns; in the oracle its block counts as identity, which decouples it."""
    args = bal_case()[0]
    cam_fixed = np.zeros(len(args[0]), dtype=np.uint8)
    cam_fixed[[0, 5]] = 1
    p = mb.BAProblem(*args, cam_fixed=cam_fixed).build(device="cpu")
    cov = p.covariance(cam_idx=[5, 2], pt_idx=PT_IDX)
    joint = cov["joint"]
    assert np.all(joint[:9, :] == 0.0) and np.all(joint[:, :9] == 0.0)
    assert np.all(cov["iters"][:9] == 0) and np.all(cov["iters"][9:] > 0)
    assert cov["converged"].all()
    linearise(p)
    rows = request_rows(9, len(args[0]), [5, 2], PT_IDX)
    ref = np.linalg.inv(dense_hessian(p))[np.ix_(rows, rows)]
    err = block_scaled_error(joint[9:, 9:], ref[9:, 9:], 9, n_cam=1)
    print("fixed: error", err)
    assert err <= CPU_BOUND
    np.testing.assert_array_equal(cov["cam_cov"][1], joint[9:18, 9:18])


# ---- no datum --------------------------------------------------------------
def test_no_datum():
    """No priors and nothing fixed: H is singular, the solves cannot
    converge, and that is what the caller is told.  Calibrated cameras: every
    requested row (pose, point) moves under the 7-dof gauge."""
    args = case_632()[0]
    p = mb.BAProblem(*args).build(device="cpu", intrinsics=INTR)
    with pytest.raises(RuntimeError, match=r"megba:.*gauge"):
        p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200)
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200,
                       strict=False)
    print("no datum: iters", cov["iters"])
    assert not cov["converged"].any()


def test_no_datum_bal_intrinsics():
    """The same on (9,3,2) cameras.  Pose and point columns do not converge.
    The f, k1, k2 columns do (in 45 iterations where a datum needs 41): the
    gauge does not move the intrinsics, so e_f is orthogonal to H's null
    space, the system is consistent and CG reaches its pseudo-inverse
    solution.  strict=True raises all the same."""
    args = bal_case()[0]
    p = mb.BAProblem(*args).build(device="cpu")
    with pytest.raises(RuntimeError, match=r"megba:.*gauge"):
        p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200)
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200,
                       strict=False)
    print("no datum: iters", cov["iters"])
    gauge_rows = np.r_[0:6, 9:15, 18:24]
    assert not cov["converged"][gauge_rows].any()


# ---- state -----------------------------------------------------------------
def test_lm_state_preserved():
    """covariance() after an accepted and after a rejected step leaves the
    LM session where it was.  The CPU engine is deterministic for a fixed
    thread count, so two plain runs are equal and the comparison is exact;
    should they differ, their spread is the tolerance."""
    plain, acc, pcg, _ = lm_run()
    again = lm_run()[0]
    spread = np.abs(plain - again).max()
    print("accepted", acc, "spread of two plain runs", spread)
    assert acc[0] and not acc[1]
    for after in (1, 2):
        chis, acc2, pcg2, cov = lm_run(call_after=after)
        assert cov["iters"].min() > 0
        assert acc2 == acc and pcg2 == pcg
        if spread == 0.0:
            np.testing.assert_array_equal(chis, plain)
        else:
            assert np.abs(chis - plain).max() <= spread


# ---- relative stop ---------------------------------------------------------
def _assembled_bal():
    args, priors = bal_case()
    p = with_priors(args, priors)
    p.build(device="cpu")
    linearise(p)
    p.process_diag(1e4)
    return p


def test_rel_tol_zero_changes_nothing():
    runs = []
    for kw in ({}, {"rel_tol": 0.0}):
        p = _assembled_bal()
        n = p.solve_linear(max_iter=100, tol=0.1, refuse_ratio=1.0, **kw)
        runs.append((n, p.dump()["deltaX"]))
    assert runs[0][0] == runs[1][0] > 0
    np.testing.assert_array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("rel", [1e-4, 1e-8])
def test_rel_tol_stops_at_first_rho_below(rel):
    """Block-Jacobi PCG on the Schur complement of the dumped, damped system
    in numpy: the engine stops after the first iteration k whose
    rho_k / rho_0 is below rel_tol (2 iterations for 1e-4, 24 for 1e-8)."""
    p = _assembled_bal()
    n = p.solve_linear(max_iter=100, tol=0.0, refuse_ratio=1e30, rel_tol=rel)
    d = p.dump()
    H = dense_hessian(p)
    nc = 9 * 12
    f = 1.0 + 1.0 / 1e4
    Hd = H.copy()
    Hd[np.diag_indices_from(Hd)] *= f
    B, E, C = Hd[:nc, :nc], Hd[:nc, nc:], Hd[nc:, nc:]
    Cinv = np.linalg.inv(C)  # block diagonal
    S = B - E @ Cinv @ E.T
    Minv = np.zeros_like(B)
    for c in range(12):
        s = slice(9 * c, 9 * c + 9)
        Minv[s, s] = np.linalg.inv(B[s, s])
    g = d["g"]
    x = np.zeros(nc)
    r = g[:nc] - E @ Cinv @ g[nc:]
    ratios, rho0, rho_prev, pv, stop = [], None, None, None, None
    for k in range(100):
        z = Minv @ r
        rho = r @ z
        rho0 = rho if k == 0 else rho0
        pv = z if k == 0 else z + rho / rho_prev * pv
        q = S @ pv
        alpha = rho / (pv @ q)
        x = x + alpha * pv
        r = r - alpha * q
        rho_prev = rho
        ratios.append(rho / rho0)
        if rho / rho0 < rel:
            stop = k + 1
            break
    print("rho_k / rho_0:", ratios)
    # the deciding ratios are not borderline, so rounding cannot move the stop
    assert ratios[-1] < 0.9 * rel and min(ratios[:-1]) > 1.1 * rel
    assert n == stop
    assert stop > 10 or rel == 1e-4
    np.testing.assert_allclose(d["deltaX"][:nc], x, rtol=1e-6,
                               atol=1e-9 * np.abs(x).max())


# ---- errors ----------------------------------------------------------------
def test_errors():
    args, priors = bal_case()
    p = with_priors(args, priors)
    with pytest.raises(RuntimeError, match="megba:"):
        p.covariance(cam_idx=[0])  # before build()
    p.build(device="cpu")
    with pytest.raises(RuntimeError, match="megba:.*duplicate"):
        p.covariance(cam_idx=[1, 1])
    with pytest.raises(RuntimeError, match="megba:.*duplicate"):
        p.covariance(pt_idx=[5, 2, 5])
    with pytest.raises(RuntimeError, match="megba:.*out of range"):
        p.covariance(cam_idx=[12])
    with pytest.raises(RuntimeError, match="megba:.*out of range"):
        p.covariance(pt_idx=[-1])
    p32 = with_priors(args, priors)
    p32.build(device="cpu", dtype="float32")
    with pytest.raises(RuntimeError, match="megba:.*float64"):
        p32.covariance(cam_idx=[0])


# ---- graph API -------------------------------------------------------------
def test_graph_api_matches_array_api():
    from megba_amd import graph as G
    args, priors = bal_case()
    cams, pts, ci, pi, meas = args
    cvs = [G.CameraVertex(c) for c in cams]
    pvs = [G.PointVertex(q) for q in pts]
    g = G.GraphProblem()
    for v in cvs + pvs:
        g.append_vertex(v)
    for c, q, m in zip(ci, pi, meas):
        g.append_edge(G.ReprojectionEdge(m).append_vertex(cvs[c])
                      .append_vertex(pvs[q]))
    for key, edge, vs in (("cam", G.CameraPriorEdge, cvs),
                          ("pt", G.PointPriorEdge, pvs),
                          ("ctr", G.CameraCenterPriorEdge, cvs)):
        for i, mean, L in zip(*priors[key]):
            g.append_edge(edge(mean, L).append_vertex(vs[i]))
    # mixed order: point, camera, camera, point
    got = g.covariance([pvs[100], cvs[7], cvs[0], pvs[3]], schur="implicit")
    ref = with_priors(args, priors).build(device="cpu", schur="implicit") \
        .covariance(cam_idx=[7, 0], pt_idx=[100, 3])["joint"]
    at = list(range(18, 21)) + list(range(0, 18)) + list(range(21, 24))
    np.testing.assert_array_equal(got, ref[np.ix_(at, at)])
    with pytest.raises(ValueError, match="megba:"):
        g.covariance([G.CameraVertex(cams[0])])


# ---- custom forward --------------------------------------------------------
def test_custom_forward_edges():
    """Only the engine interface is used: a (4,3,2) custom-forward problem
    with camera and point priors against its dense oracle."""
    from test_generic_dims import _wp_forward
    from test_priors_gpu import _problem_432
    args = _problem_432()
    priors = make_priors(args, n_cam=6, n_pt=20, n_ctr=0,
                         custom_forward=_wp_forward)
    p = with_priors(args, priors)
    p.build(device="cpu", custom_forward=_wp_forward)
    cov = p.covariance(cam_idx=[0, 4], pt_idx=[3, 40])
    linearise(p)
    rows = request_rows(4, 6, [0, 4], [3, 40])
    ref = np.linalg.inv(dense_hessian(p))[np.ix_(rows, rows)]
    err = block_scaled_error(cov["joint"], ref, 4)
    print("custom forward: error", err)
    assert err <= CPU_BOUND


# ---- C++ example -----------------------------------------------------------
def test_cpp_covariance_example_cpu(tmp_path):
    run_cpp_covariance("cpu", tmp_path)
