"""Gaussian unary priors (camera parameters, points, camera centres) on the
CPU engine, checked against numpy in fp64."""
import numpy as np
import pytest

import megba_amd as mb
from priors_common import (INTR, assembled, bal_case, case_632, centre_np,
                           centres_np, rodrigues, run_cpp_priors, with_priors)


def _quad(L, r):
    return float(np.einsum("ki,kij,kj->", r, L, r))


def _prior_chi2(args, priors):
    cams, pts = args[0], args[1]
    s = 0.0
    if "cam" in priors:
        i, m, L = priors["cam"]
        s += _quad(L, cams[i] - m)
    if "pt" in priors:
        i, m, L = priors["pt"]
        s += _quad(L, pts[i] - m)
    if "ctr" in priors:
        i, m, L = priors["ctr"]
        s += _quad(L, centres_np(cams[i]) - m)
    return s


def _assembled_with(args, priors, **build_kw):
    p = with_priors(args, priors)
    p.build(device="cpu", **build_kw)
    p.chi0 = p.forward()
    p.accept_forward()
    p.build_linear_system()
    return p


def test_pack_sym():
    M = np.arange(9.0).reshape(3, 3)
    M = M + M.T
    np.testing.assert_array_equal(mb.pack_sym(M),
                                  [M[0, 0], M[0, 1], M[0, 2], M[1, 1],
                                   M[1, 2], M[2, 2]])
    assert mb.pack_sym(np.stack([M, 2 * M])).shape == (2, 6)


@pytest.mark.parametrize("case", ["bal", "632"])
def test_chi2_increment(case):
    """forward() with priors minus forward() without = sum r^T L r."""
    args, priors = bal_case() if case == "bal" else case_632()
    kw = {} if case == "bal" else dict(intrinsics=INTR)
    base = assembled(args, **kw).chi0
    p = with_priors(args, priors)
    p.build(device="cpu", **kw)
    total = p.forward()
    want = _prior_chi2(args, priors)
    assert want > 1e-3 * base  # the priors are not negligible
    assert abs((total - base) - want) <= 1e-12 * total


def test_assembly_increment():
    """Parameter priors add L to their own Hpp/Hll block and -L (x - mean)
    to their g slice; every other entry is bit-identical."""
    args, priors = bal_case()
    priors = {k: priors[k] for k in ("cam", "pt")}
    cams, pts = args[0], args[1]
    ncam, npt = len(cams), len(pts)
    d0 = assembled(args).dump()
    d1 = _assembled_with(args, priors).dump()
    for key, n, dim, kind, x in (("Hpp", ncam, 9, "cam", cams),
                                 ("Hll", npt, 3, "pt", pts)):
        idx, mean, L = priors[kind]
        h0 = d0[key].reshape(n, dim, dim)
        h1 = d1[key].reshape(n, dim, dim)
        off = ncam * 9 if kind == "pt" else 0
        g0 = d0["g"][off:off + n * dim].reshape(n, dim)
        g1 = d1["g"][off:off + n * dim].reshape(n, dim)
        rest = np.setdiff1d(np.arange(n), idx)
        np.testing.assert_array_equal(h1[rest], h0[rest])
        np.testing.assert_array_equal(g1[rest], g0[rest])
        for k, v in enumerate(idx):
            np.testing.assert_allclose(
                h1[v] - h0[v], L[k], rtol=0,
                atol=1e-10 * np.abs(h0[v]).max(), err_msg=f"{key}[{v}]")
            np.testing.assert_allclose(
                g1[v] - g0[v], -L[k] @ (x[v] - mean[k]), rtol=0,
                atol=1e-10 * np.abs(g0[v]).max(), err_msg=f"g {kind}[{v}]")
    np.testing.assert_array_equal(d1["Hpl"], d0["Hpl"])


def _centre_jac_fd(cam):
    """3x6 dC/dcam[:6] by central differences, h = 1e-6 max(1, |x|)."""
    J = np.zeros((3, 6))
    for i in range(6):
        h = 1e-6 * max(1.0, abs(cam[i]))
        a, b = cam.copy(), cam.copy()
        a[i] += h
        b[i] -= h
        J[:, i] = (centre_np(a) - centre_np(b)) / (2 * h)
    return J


@pytest.mark.parametrize("case", ["bal", "632"])
def test_centre_prior_jacobian(case):
    """The centre prior's Hpp/g increment is J^T L J / -J^T L r with J from
    central differences of a numpy C(cam).  Bound: 1e-6 of the largest entry
    of the compared product.  The difference quotient's own error is about
    1e-12 (truncation) + eps |C| / h ~ 2e-9 (rounding) relative to |J| ~ 1;
    through the products (at most 18 terms, two J factors) that stays under
    1e-7, so 1e-6 leaves an order of magnitude."""
    args, priors = bal_case() if case == "bal" else case_632()
    kw = {} if case == "bal" else dict(intrinsics=INTR)
    priors = {"ctr": priors["ctr"]}
    cams = args[0]
    ncam, cd = cams.shape
    d0 = assembled(args, **kw).dump()
    d1 = _assembled_with(args, priors, **kw).dump()
    dH = (d1["Hpp"] - d0["Hpp"]).reshape(ncam, cd, cd)
    dg = (d1["g"] - d0["g"])[:ncam * cd].reshape(ncam, cd)
    idx, mean, L = priors["ctr"]
    rest = np.setdiff1d(np.arange(ncam), idx)
    assert np.all(dH[rest] == 0) and np.all(dg[rest] == 0)
    np.testing.assert_array_equal(d1["Hll"], d0["Hll"])
    for k, c in enumerate(idx):
        J = _centre_jac_fd(cams[c])
        r = centre_np(cams[c]) - mean[k]
        wantH = np.zeros((cd, cd))
        wantH[:6, :6] = J.T @ L[k] @ J
        wantg = np.zeros(cd)
        wantg[:6] = -J.T @ L[k] @ r
        # rounding of the one add onto the existing block comes on top
        h0 = np.abs(d0["Hpp"].reshape(ncam, cd, cd)[c]).max()
        np.testing.assert_allclose(
            dH[c], wantH, rtol=0,
            atol=1e-6 * np.abs(wantH).max() + 1e-10 * h0)
        g0 = np.abs(d0["g"][:ncam * cd].reshape(ncam, cd)[c]).max()
        np.testing.assert_allclose(
            dg[c], wantg, rtol=0,
            atol=1e-6 * np.abs(wantg).max() + 1e-10 * g0)
        # the intrinsics rows/columns get exact zeros
        assert np.all(dH[c][6:, :] == 0) and np.all(dH[c][:, 6:] == 0)


def _dense_system(p, args, priors, region):
    """Dense damped normal equations + prior terms from the dumped J."""
    cams, pts = args[0], args[1]
    ncam, npt = len(cams), len(pts)
    d = p.dump()
    ii = p.index_info()
    nL = len(ii["cam_of"])
    Jc = d["Jc"].reshape(nL, 2, 9)
    Jp = d["Jp"].reshape(nL, 2, 3)
    r = d["r"].reshape(nL, 2)
    dim = ncam * 9 + npt * 3
    J = np.zeros((2 * nL, dim))
    for e in range(nL):
        c, q = ii["cam_of"][e], ii["pt_of"][e]
        J[2 * e:2 * e + 2, 9 * c:9 * c + 9] = Jc[e]
        J[2 * e:2 * e + 2, ncam * 9 + 3 * q:ncam * 9 + 3 * q + 3] = Jp[e]
    H = J.T @ J
    g = -J.T @ r.reshape(-1)
    terms = []  # (columns, Jprior, L, r) of every prior
    i, m, L = priors["cam"]
    for k, c in enumerate(i):
        terms.append((np.arange(9 * c, 9 * c + 9), np.eye(9), L[k],
                      cams[c] - m[k]))
    i, m, L = priors["pt"]
    for k, q in enumerate(i):
        o = ncam * 9 + 3 * q
        terms.append((np.arange(o, o + 3), np.eye(3), L[k], pts[q] - m[k]))
    i, m, L = priors["ctr"]
    for k, c in enumerate(i):
        terms.append((np.arange(9 * c, 9 * c + 6), _centre_jac_fd(cams[c]),
                      L[k], centre_np(cams[c]) - m[k]))
    for cols, Jq, L, rq in terms:
        H[np.ix_(cols, cols)] += Jq.T @ L @ Jq
        g[cols] -= Jq.T @ L @ rq
    Hd = H + np.diag(np.diag(H)) / region
    return J, r.reshape(-1), terms, Hd, g


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_step_matches_dense_oracle(schur):
    """deltaX against a direct dense solve of the damped normal equations
    with the prior terms added in numpy; rho_denominator against the dense
    quadratic model evaluated at the engine's own deltaX (so the comparison
    is of the model, not of the solve)."""
    args, priors = bal_case()
    p = _assembled_with(args, priors, schur=schur)
    chi = p.chi0
    J, r, terms, Hd, g = _dense_system(p, args, priors, 1e4)
    p.process_diag(1e4)
    p.solve_linear(max_iter=400, tol=0.0, refuse_ratio=1e30)
    dx = p.dump()["deltaX"]
    want = np.linalg.solve(Hd, g)
    np.testing.assert_allclose(dx, want, rtol=0,
                               atol=1e-7 * np.abs(dx).max())
    p.update_params()
    model = float(np.sum((J @ dx + r) ** 2))
    for cols, Jq, L, rq in terms:
        a = Jq @ dx[cols] + rq
        model += float(a @ L @ a)
    np.testing.assert_allclose(p.rho_denominator(chi), model - chi, rtol=1e-9)


def _shifted(args, d):
    """Rigid translation X += d, t -= R d: every reprojection is unchanged."""
    cams, pts = args[0].copy(), args[1].copy()
    pts += d
    for c in cams:
        c[3:6] -= rodrigues(c[:3]) @ d
    return (cams, pts) + tuple(args[2:])


def test_centre_priors_fix_the_gauge():
    args = mb.synthesize_bal(12, 120, 1100, seed=3)
    d = np.array([5.0, -3.0, 2.0])
    gps = centres_np(args[0])
    sh = _shifted(args, d)
    # the shift is invisible to the reprojection error
    a = mb.BAProblem(*args).build(device="cpu").forward()
    b = mb.BAProblem(*sh).build(device="cpu").forward()
    np.testing.assert_allclose(b, a, rtol=1e-9)
    kw = dict(max_iter=10, verbose=False)

    p = mb.BAProblem(*sh)
    p.set_camera_center_prior(np.arange(12), gps,
                              np.tile(mb.pack_sym(1e4 * np.eye(3)), (12, 1)))
    p.build(device="cpu")
    rep = p.solve(**kw)
    assert rep["final_chi2"] < rep["iters"][0]["chi2"]
    dist = np.linalg.norm(centres_np(p.params()[0]) - gps, axis=1).mean()
    assert dist < np.linalg.norm(d)

    # control: without priors only LM noise moves the centres
    q = mb.BAProblem(*sh).build(device="cpu")
    q.solve(**kw)
    free = np.linalg.norm(centres_np(q.params()[0]) - gps, axis=1).mean()
    assert abs(free - np.linalg.norm(d)) < 0.1 * np.linalg.norm(d)
    print("mean centre distance: priors", dist, "free", free)


def test_priors_on_fixed_vertices():
    """A prior on a fixed vertex: constant r^T L r in chi2, exact zeros in
    H and g, parameters bit-equal after the solve."""
    args, priors = bal_case()
    cams, pts = args[0], args[1]
    cam_fixed = np.zeros(len(cams), dtype=np.uint8)
    pt_fixed = np.zeros(len(pts), dtype=np.uint8)
    c, q, g = priors["cam"][0][0], priors["pt"][0][0], priors["ctr"][0][0]
    cam_fixed[[c, g]] = 1
    pt_fixed[q] = 1
    only = {k: tuple(a[:1] for a in priors[k]) for k in priors}
    fx = dict(cam_fixed=cam_fixed, pt_fixed=pt_fixed)

    def run(pr):
        p = with_priors(args, pr, **fx)
        p.build(device="cpu")
        chi = p.forward()
        p.accept_forward()
        p.build_linear_system()
        d = p.dump()
        p.process_diag(1e4)
        p.solve_linear(max_iter=50, tol=1e-12, refuse_ratio=1e30)
        p.update_params()
        rho = p.rho_denominator(chi)
        return p, chi, d, rho

    p0, chi0, d0, rho0 = run({})
    p1, chi1, d1, rho1 = run(only)
    want = _prior_chi2(args, only)
    assert want > 0
    assert abs((chi1 - chi0) - want) <= 1e-12 * chi1
    for key in ("Hpp", "Hll", "g"):
        np.testing.assert_array_equal(d1[key], d0[key])
    # the constant cancels inside rho_denominator
    np.testing.assert_allclose(rho1, rho0, rtol=1e-9)
    s = with_priors(args, only, **fx)
    s.build(device="cpu")
    s.solve(max_iter=5, verbose=False)
    c2, p2 = s.params()
    np.testing.assert_array_equal(c2[[c, g]], cams[[c, g]])
    np.testing.assert_array_equal(p2[q], pts[q])
    assert np.any(c2[cam_fixed == 0] != cams[cam_fixed == 0])


def _fresh():
    return mb.BAProblem(*mb.synthesize_bal(6, 40, 300, seed=1))


@pytest.mark.parametrize("name,setup", [
    ("index high", lambda p: p.set_camera_prior([6], np.zeros((1, 9)))),
    ("index negative", lambda p: p.set_point_prior([-1], np.zeros((1, 3)))),
    ("duplicate", lambda p: p.set_point_prior([3, 3], np.zeros((2, 3)))),
    ("mean shape", lambda p: p.set_camera_prior([0, 1], np.zeros((2, 6)))),
    ("mean transposed", lambda p: p.set_point_prior([0, 1, 2],
                                                    np.zeros((3, 3)).T[:, :2])),
    ("mean flat", lambda p: p.set_point_prior([0], np.zeros(3))),
    ("info shape", lambda p: p.set_point_prior([0], np.zeros((1, 3)),
                                               np.ones((1, 9)))),
    ("info rows", lambda p: p.set_point_prior([0, 1], np.zeros((2, 3)),
                                              np.ones((1, 6)))),
    ("nan mean", lambda p: p.set_camera_center_prior(
        [0], np.array([[0.0, np.nan, 0.0]]))),
    ("inf info", lambda p: p.set_point_prior(
        [0], np.zeros((1, 3)), np.array([[1, 0, 0, np.inf, 0, 1.0]]))),
    ("negative diagonal", lambda p: p.set_point_prior(
        [0], np.zeros((1, 3)), np.array([[1, 0, 0, -1e-3, 0, 1.0]]))),
])
def test_validation_errors(name, setup):
    p = _fresh()
    setup(p)
    with pytest.raises(RuntimeError, match="megba:"):
        p.build(device="cpu")


def test_centre_prior_needs_the_bal_camera():
    # custom forward: the camera parametrisation is unknown
    def never_called(cam, pt, meas):
        raise AssertionError("build() must refuse before any forward")
    p = _fresh()
    p.set_camera_center_prior([0], np.zeros((1, 3)))
    with pytest.raises(RuntimeError, match="megba:.*centre"):
        p.build(device="cpu", custom_forward=never_called)
    # (6,3,3) has a built-in residual but is not in the supported table
    cams, pts, ci, pi, meas = mb.synthesize_bal(6, 40, 300, seed=1)
    p = mb.BAProblem(cams[:, :6].copy(), pts, ci, pi,
                     np.zeros((len(ci), 3)))
    p.set_camera_center_prior([0], np.zeros((1, 3)))
    with pytest.raises(RuntimeError, match="megba:.*centre"):
        p.build(device="cpu")
    # a camera parameter prior on the same dims is fine
    p = mb.BAProblem(cams[:, :6].copy(), pts, ci, pi,
                     np.zeros((len(ci), 3)))
    p.set_camera_prior([0], cams[:1, :6])
    p.build(device="cpu")


def test_setters_raise_after_build():
    p = _fresh()
    p.set_point_prior([0], np.zeros((1, 3)))
    p.build(device="cpu")
    for call in (lambda: p.set_point_prior([1], np.zeros((1, 3))),
                 lambda: p.set_camera_prior([1], np.zeros((1, 9))),
                 lambda: p.set_camera_center_prior([1], np.zeros((1, 3)))):
        with pytest.raises(RuntimeError, match="megba:.*before build"):
            call()


def test_graph_api_matches_array_api():
    from megba_amd.graph import (CameraCenterPriorEdge, CameraPriorEdge,
                                 CameraVertex, GraphProblem, PointPriorEdge,
                                 PointVertex, ReprojectionEdge)
    args, priors = bal_case()
    cams, pts, ci, pi, meas = args
    kw = dict(max_iter=5, solver_tol=1e-8, solver_max_iter=150,
              solver_refuse_ratio=1e6, verbose=False)
    p = with_priors(args, priors)
    p.build(device="cpu")
    ref = p.solve(**kw)

    g = GraphProblem()
    cvs = [CameraVertex(c) for c in cams]
    pvs = [PointVertex(x) for x in pts]
    for c, q, m in zip(ci, pi, meas):
        g.append_edge(ReprojectionEdge(m).append_vertex(cvs[c])
                      .append_vertex(pvs[q]))
    for cls, kind, vs in ((CameraPriorEdge, "cam", cvs),
                          (PointPriorEdge, "pt", pvs),
                          (CameraCenterPriorEdge, "ctr", cvs)):
        idx, mean, L = priors[kind]
        for k, v in enumerate(idx):
            # full and packed information are both accepted
            info = L[k] if k % 2 else mb.pack_sym(L[k])
            g.append_edge(cls(mean[k], info).append_vertex(vs[v]))
    rep = g.solve(device="cpu", **kw)
    # Both runs hand the engine identical arrays; what differs is the
    # rounding of the OpenMP chi2 reduction (order not fixed between runs),
    # which enters the next step through the trust-region update.  That is
    # ~1e-16 relative per step; 1e-9 leaves room for five steps of growth
    # and is far below any real difference between the two APIs.
    np.testing.assert_allclose([i["chi2"] for i in rep["iters"]],
                               [i["chi2"] for i in ref["iters"]], rtol=1e-9)
    c2, p2 = p.params()
    np.testing.assert_allclose(np.stack([v.estimation for v in cvs]), c2,
                               rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.stack([v.estimation for v in pvs]), p2,
                               rtol=1e-9, atol=1e-12)
    # a prior edge wants exactly one vertex of its own kind
    with pytest.raises(ValueError):
        PointPriorEdge(np.zeros(3)).append_vertex(cvs[0])
    with pytest.raises(ValueError):
        GraphProblem().append_edge(PointPriorEdge(np.zeros(3)))
    # priors alone do not make a problem
    lone = GraphProblem()
    lone.append_edge(PointPriorEdge(np.zeros(3)).append_vertex(
        PointVertex(np.zeros(3))))
    lone.append_vertex(CameraVertex(np.zeros(9)))
    with pytest.raises(ValueError):
        lone.solve(device="cpu", verbose=False)


def test_cpp_priors_example_cpu(tmp_path):
    run_cpp_priors("cpu", tmp_path)
