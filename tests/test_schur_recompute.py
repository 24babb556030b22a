"""GPU tests for the recomputed-J LDS Schur apply (kSchurFusedLdsRc,
MEGBA_SCHUR_RECOMPUTE=1): kSchurFusedLds with the packed [Jc, Jp] loads
replaced by the closed-form BAL edge part evaluated from a snapshot of the
accepted cameras and points.  Every case solves the same damped system with
the default path and with the recompute path and compares deltaX; the
engine's MEGBA_TUNE_VERBOSE line tells which path actually ran.
"""
import os

import numpy as np
import pytest

import megba_amd as mb

RC = {"MEGBA_SCHUR_RECOMPUTE": "1"}
LDS = {"MEGBA_SCHUR_LDS": "1"}


class _Env:
    def __init__(self, env):
        self.env = dict(env)
        self.env.setdefault("MEGBA_TUNE_VERBOSE", "1")

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _solve(env, args, info=None, schur="implicit", dtype="float64",
           problem_kw=None, **build_kw):
    with _Env(env):
        p = mb.BAProblem(*args, info=info, **(problem_kw or {}))
        p.build(device="gpu", dtype=dtype, schur=schur, **build_kw)
        p.forward()
        p.accept_forward()
        p.build_linear_system()
        p.process_diag(1e4)
        n = p.solve_linear(max_iter=30, tol=0.0, refuse_ratio=1e30)
        return n, p.dump()["deltaX"]


def _path(capfd):
    """Path names the engines built since the last call reported."""
    err = capfd.readouterr().err
    return [ln.split(":", 1)[1].strip() for ln in err.splitlines()
            if ln.startswith("# schur path:")]


def _pair(capfd, args, info=None, rc_env=RC, expect="lds-recompute",
          **kw):
    """Default path against the recompute path; returns both deltaX."""
    capfd.readouterr()
    n1, dx1 = _solve({}, args, info=info, **kw)
    assert _path(capfd) == ["fused-etx"]
    n2, dx2 = _solve(rc_env, args, info=info, **kw)
    assert _path(capfd) == [expect]
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    np.testing.assert_allclose(dx2, dx1, rtol=1e-6, atol=1e-9 * scale)
    return dx1, dx2


@pytest.mark.gpu
@pytest.mark.parametrize("diff", ["auto", "analytical"])
def test_recompute_matches_default(capfd, diff):
    _pair(capfd, mb.synthesize_bal(24, 400, 3600, seed=14), diff=diff)


def _long_run_problem():
    rng = np.random.default_rng(8)
    cams, pts, ci, pi, meas = mb.synthesize_bal(90, 300, 6000, seed=15)
    # steal one edge from every camera for point 0 -> degree 90 > 64,
    # touching only points that keep >= 3 observations
    counts = np.bincount(pi, minlength=300)
    taken = 0
    for e in rng.permutation(len(pi)):
        if taken >= 90:
            break
        if pi[e] != 0 and counts[pi[e]] > 3:
            counts[pi[e]] -= 1
            pi[e] = 0
            ci[e] = taken % 90
            taken += 1
    assert np.bincount(pi, minlength=300)[0] > 64
    return cams, pts, ci, pi, meas


@pytest.mark.gpu
def test_recompute_long_run_point(capfd):
    """A landmark with >64 observations: flagged windows and the stored-J
    long-run finishers beside recomputed edges."""
    _pair(capfd, _long_run_problem())


def _weighted_problem():
    rng = np.random.default_rng(9)
    args = mb.synthesize_bal(20, 300, 2600, seed=16)
    w = rng.uniform(0.5, 2.0, (len(args[2]), 2))
    info = np.stack([w[:, 0], 0.1 * np.ones(len(w)), w[:, 1]], axis=1)
    return args, info


@pytest.mark.gpu
def test_recompute_weighted_info(capfd):
    args, info = _weighted_problem()
    _pair(capfd, args, info=info)


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_recompute_robust_loss(capfd, loss):
    args, info = _weighted_problem()
    _pair(capfd, args, info=info, loss=loss, loss_delta=1.5)


@pytest.mark.gpu
def test_recompute_starved_grid(capfd):
    """Fewer windows than workgroups: most workgroups flush a zero row."""
    _pair(capfd, mb.synthesize_bal(6, 40, 240, seed=3))


@pytest.mark.gpu
def test_recompute_fixed_vertices(capfd):
    """Fixed cameras / points: their edges contribute exact zeros, and the
    fixed entries of deltaX stay exactly 0."""
    cams, pts, ci, pi, meas = mb.synthesize_bal(12, 120, 1100, seed=3)
    cam_fixed = np.zeros(12, dtype=np.uint8)
    cam_fixed[:3] = 1
    pt_fixed = np.zeros(120, dtype=np.uint8)
    pt_fixed[::10] = 1
    _, dx = _pair(capfd, (cams, pts, ci, pi, meas),
                  problem_kw=dict(cam_fixed=cam_fixed, pt_fixed=pt_fixed))
    dxc = dx[:12 * 9].reshape(12, 9)
    dxp = dx[12 * 9:].reshape(120, 3)
    assert np.all(dxc[cam_fixed == 1] == 0.0)
    assert np.all(dxp[pt_fixed == 1] == 0.0)
    assert np.any(dxc[cam_fixed == 0] != 0.0)


def _small_angle_problem():
    """One camera with aa exactly zero, one just under the theta2 <= 1e-14
    guard, measurements regenerated to be consistent with them."""
    cams, pts, ci, pi, meas0 = mb.synthesize_bal(6, 60, 500, seed=2)
    cams[0, :3] = 0.0
    cams[1, :3] = [9e-8, 0.0, 0.0]  # theta2 = 8.1e-15
    assert cams[1, :3] @ cams[1, :3] <= 1e-14
    p = mb.BAProblem(cams, pts, ci, pi, np.zeros_like(meas0))
    p.build(device="cpu")
    p.forward()
    r_sorted = p.dump()["r"].reshape(-1, 2)
    r = np.empty_like(r_sorted)
    r[p.index_info()["perm"]] = r_sorted
    meas = r + np.random.default_rng(21).normal(0, 0.5, r.shape)
    return cams, pts, ci, pi, meas


def test_small_angle_problem_solves_cpu():
    """The small-angle problem is usable: the CPU engine alone gives a finite,
    non-zero deltaX on it."""
    p = mb.BAProblem(*_small_angle_problem())
    p.build(device="cpu", schur="implicit", diff="analytical")
    p.forward()
    p.accept_forward()
    p.build_linear_system()
    p.process_diag(1e4)
    p.solve_linear(max_iter=30, tol=0.0, refuse_ratio=1e30)
    dx = p.dump()["deltaX"]
    assert np.all(np.isfinite(dx)) and np.abs(dx).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("diff", ["auto", "analytical"])
def test_recompute_small_angles(capfd, diff):
    dx1, dx2 = _pair(capfd, _small_angle_problem(), diff=diff)
    assert np.all(np.isfinite(dx2))


def _two_solves(env, args):
    with _Env(env):
        p = mb.BAProblem(*args)
        p.build(device="gpu", schur="implicit")
        p.forward()
        p.accept_forward()
        p.build_linear_system()
        p.process_diag(1e4)
        n1 = p.solve_linear(max_iter=30, tol=0.0, refuse_ratio=1e30)
        p.update_params()
        n2 = p.solve_linear(max_iter=30, tol=0.0, refuse_ratio=1e30)
        return n1, n2, p.dump()["deltaX"]


@pytest.mark.gpu
def test_recompute_reads_the_accepted_snapshot(capfd):
    """A second solve after update_params(), without a new forward, still
    applies the J of the accepted point: it must match the stored-J LDS
    engine, which it cannot if the kernel reads the live parameters."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    capfd.readouterr()
    a = _two_solves(LDS, args)
    b = _two_solves(RC, args)
    assert _path(capfd) == ["lds", "lds-recompute"]
    assert a[:2] == b[:2]
    scale = np.abs(a[2]).max() or 1.0
    np.testing.assert_allclose(b[2], a[2], rtol=1e-6, atol=1e-9 * scale)


def _dims632_problem():
    """(6,3,2) problem with shared intrinsics: (args, intrinsics)."""
    intr = [420.0, -1e-7, 3e-13]
    cams9, pts, ci, pi, meas0 = mb.synthesize_bal(12, 110, 950, seed=12)
    cams9[:, 6:9] = intr
    p = mb.BAProblem(cams9, pts, ci, pi, np.zeros_like(meas0))
    p.build(device="cpu")
    p.forward()
    r_sorted = p.dump()["r"].reshape(-1, 2)
    r = np.empty_like(r_sorted)
    r[p.index_info()["perm"]] = r_sorted
    meas = r + np.random.default_rng(112).normal(0, 0.5, r.shape)
    return (cams9[:, :6].copy(), pts, ci, pi, meas), intr


def _bal_forward(cam, pt, meas):
    from megba_amd import jv
    cam, pt, meas = jv.wrap(cam), jv.wrap(pt), jv.wrap(meas)
    R = jv.angle_axis_to_rotation(cam[0:3])
    P = [R[3 * i] * pt[0] + R[3 * i + 1] * pt[1] + R[3 * i + 2] * pt[2]
         + cam[3 + i] for i in range(3)]
    px = -P[0] / P[2]
    py = -P[1] / P[2]
    fr = jv.radial_distortion([px, py], cam[6:9])
    return ((fr * px - meas[0]).raw, (fr * py - meas[1]).raw)


def _ineligible_cases():
    bal = mb.synthesize_bal(24, 400, 3600, seed=14)
    args632, intr = _dims632_problem()
    need = 24 * 9 * 8
    return {
        "explicit": (bal, {}, dict(schur="explicit")),
        "dims632": (args632, {}, dict(intrinsics=intr)),
        "custom_forward": (mb.synthesize_bal(12, 120, 1100, seed=3), {},
                           dict(custom_forward=_bal_forward)),
        "lds_one_byte_short": (
            bal, {"MEGBA_SCHUR_LDS_MAX_BYTES": str(need - 1)}, {}),
        "excluded_by_env": (bal, {"MEGBA_NO_SCHUR_RECOMPUTE": "1"}, {}),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["explicit", "dims632", "custom_forward",
                                  "lds_one_byte_short", "excluded_by_env"])
def test_recompute_ineligible_keeps_the_path(capfd, case):
    """Where the path is not eligible its forcing knob changes nothing."""
    args, env, kw = _ineligible_cases()[case]
    capfd.readouterr()
    n1, dx1 = _solve(env, args, **kw)
    without = _path(capfd)
    n2, dx2 = _solve(dict(env, **RC), args, **kw)
    with_knob = _path(capfd)
    assert len(without) == 1 and with_knob == without
    assert "lds-recompute" not in with_knob
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    np.testing.assert_allclose(dx2, dx1, rtol=1e-6, atol=1e-9 * scale)


@pytest.mark.gpu
def test_recompute_wins_over_lds_knob(capfd):
    """Both forcing knobs set: recompute wins; MEGBA_SCHUR_LDS alone still
    resolves to lds."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    _pair(capfd, args, rc_env=dict(RC, **LDS))
    _pair(capfd, args, rc_env=LDS, expect="lds")


def _traj(device, env, steps=4):
    with _Env(env):
        cams, pts, ci, pi, meas = mb.synthesize_bal(20, 300, 2600, seed=5)
        p = mb.BAProblem(cams, pts, ci, pi, meas)
        p.build(device=device, schur="implicit")
        chis = [p.lm_init(force_iterations=True, solver_tol=0.0,
                          solver_refuse_ratio=1e30, solver_max_iter=40)]
        accepted = 0
        for _ in range(steps):
            log = p.lm_step()
            chis.append(log["chi2"])
            accepted += bool(log["accepted"])
        return np.asarray(chis), accepted


def test_trajectory_has_an_accepted_step_cpu():
    """The graph-vs-eager trajectory below goes through acceptForward (and so
    through a fresh snapshot) after the first solve."""
    _, accepted = _traj("cpu", {})
    assert accepted >= 1


@pytest.mark.gpu
def test_recompute_graph_matches_eager(capfd):
    capfd.readouterr()
    a, acc_a = _traj("gpu", RC)
    b, acc_b = _traj("gpu", dict(RC, MEGBA_NO_GRAPH="1"))
    assert _path(capfd) == ["lds-recompute", "lds-recompute"]
    assert acc_a >= 1 and acc_a == acc_b
    np.testing.assert_allclose(a, b, rtol=2e-5)


# fp32: the bound comes from a rounding-level change of J that the project
# already has, not from the recompute kernel.  On this problem the default
# path with diff="auto" and the default path with diff="analytical" differ by
# FP32_DIFFMODE_DEV * max|deltaX| (measured on MI355X on the commit before
# this path existed: 4.7331e-4, with max|deltaX| = 1.878; two diff="auto"
# runs agree bit for bit there); the recompute path is allowed four times
# that against the default path, 1.8932e-3.
FP32_DIFFMODE_DEV = 4.7331e-4
FP32_BOUND = 4 * FP32_DIFFMODE_DEV


@pytest.mark.gpu
def test_recompute_fp32(capfd):
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    capfd.readouterr()
    n1, dx1 = _solve({}, args, dtype="float32")
    n2, dx2 = _solve(RC, args, dtype="float32")
    assert _path(capfd) == ["fused-etx", "lds-recompute"]
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    dev = np.abs(dx2 - dx1).max() / scale
    print("fp32 recompute-vs-default deviation / max|deltaX|:", dev,
          "max|deltaX|:", scale)
    assert dev <= FP32_BOUND
