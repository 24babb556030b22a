"""GPU tests for the staged camera-row gather of the recomputed-J Schur
product (kSchurFusedLdsRc<.., STAGED>): the camera rows of a window are loaded
once per 64-byte segment by lane quads and handed to the lanes through a
wave-private LDS tile, instead of eleven 16-byte loads per lane.

Every case solves the same damped system three times and compares deltaX of
the staged recompute path against two references: the default path
(fused-etx; forced with MEGBA_ETXFUSE where the problem is large enough for
the auto-tuner to run) and the per-lane recompute path
(MEGBA_NO_RC_STAGE=1).  Tolerance: that of test_schur_recompute.py::_pair.
LDS atomic order makes bit equality impossible; a wrong row or chunk is an
O(1) error.  The engine's MEGBA_TUNE_VERBOSE lines tell which path and which
gather instance ran.
"""
import os

import numpy as np
import pytest

import megba_amd as mb

pytestmark = pytest.mark.gpu

RC = {"MEGBA_SCHUR_RECOMPUTE": "1"}
PER_LANE = dict(RC, MEGBA_NO_RC_STAGE="1")


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


def _ready(args, info=None, dtype="float64", problem_kw=None, **build_kw):
    """A built problem with its damped linear system, under env."""
    p = mb.BAProblem(*args, info=info, **(problem_kw or {}))
    p.build(device="gpu", dtype=dtype, schur="implicit", **build_kw)
    p.forward()
    p.accept_forward()
    p.build_linear_system()
    p.process_diag(1e4)
    return p


def _solve(env, args, two_solves=False, max_iter=30, **kw):
    with _Env(env):
        p = _ready(args, **kw)
        n = [p.solve_linear(max_iter=max_iter, tol=0.0, refuse_ratio=1e30)]
        if two_solves:
            p.update_params()
            n.append(p.solve_linear(max_iter=max_iter, tol=0.0,
                                    refuse_ratio=1e30))
        return n, p.dump()["deltaX"]


def _report(capfd):
    """(paths, gather instances) the engines built since the last call
    reported."""
    err = capfd.readouterr().err

    def pick(prefix):
        return [ln.split(":", 1)[1].strip() for ln in err.splitlines()
                if ln.startswith(prefix)]
    return pick("# schur path:"), pick("# schur recompute gather:")


def _close(dx, ref):
    scale = np.abs(ref).max() or 1.0
    np.testing.assert_allclose(dx, ref, rtol=1e-6, atol=1e-9 * scale)


def _triple(capfd, args, extra_env=None, ref_env=None, staged_env=None,
            expect_gather="staged", **kw):
    """Default path, per-lane recompute, staged recompute: returns the three
    deltaX after checking the staged one against the other two."""
    extra = extra_env or {}
    capfd.readouterr()
    n0, dx0 = _solve(dict(ref_env or {}), args, **kw)
    assert _report(capfd) == (["fused-etx"], [])
    n1, dx1 = _solve(dict(PER_LANE, **extra), args, **kw)
    assert _report(capfd) == (["lds-recompute"], ["per-lane"])
    n2, dx2 = _solve(dict(staged_env or RC, **extra), args, **kw)
    assert _report(capfd) == (["lds-recompute"], [expect_gather])
    assert n0 == n1 == n2
    assert np.abs(dx0).max() > 0
    _close(dx2, dx0)
    _close(dx2, dx1)
    return dx0, dx1, dx2


def test_few_cameras(capfd):
    """Three cameras: most lanes of a quad group want the same row.

    The reduced system has 27 unknowns, so CG is run for 20 iterations: from
    iteration 27 on it has nothing left to reduce and divides rounding noise
    by rounding noise on every path (the stored-J lds path, which this change
    does not touch, is then 3.9e-4 of max|deltaX| away from the default path,
    against 1.2e-12 at 20 iterations; measured on MI355X)."""
    _triple(capfd, mb.synthesize_bal(3, 60, 400, seed=4), max_iter=20)


def test_starved_grid_partial_window(capfd):
    """Fewer windows than workgroups, and the last window has an inactive
    tail whose lanes still load for their neighbours."""
    _triple(capfd, mb.synthesize_bal(6, 40, 240, seed=3))


def test_several_trips_one_wave(capfd):
    """One wave per workgroup makes several trips: the tile is reused across
    windows."""
    _triple(capfd, mb.synthesize_bal(40, 8000, 40000, seed=5),
            extra_env={"MEGBA_SCHUR_LDS_THREADS": "64"})


def test_several_trips_default_workgroup(capfd):
    """About 18 windows per 512-thread workgroup: its waves make 2 or 3
    trips, so they leave the window loop at different times.  300 k edges are
    over the auto-tune threshold, hence the forced fused-etx reference."""
    _triple(capfd, mb.synthesize_bal(60, 60000, 300000, seed=6),
            ref_env={"MEGBA_ETXFUSE": "1"})


def test_fixed_vertices(capfd):
    """Lanes of fixed cameras / points are not live but still load for their
    neighbours; the fixed entries of deltaX stay exactly 0."""
    cams, pts, ci, pi, meas = mb.synthesize_bal(12, 120, 1100, seed=3)
    cam_fixed = np.zeros(12, dtype=np.uint8)
    cam_fixed[:3] = 1
    pt_fixed = np.zeros(120, dtype=np.uint8)
    pt_fixed[::10] = 1
    _, _, dx = _triple(capfd, (cams, pts, ci, pi, meas),
                       problem_kw=dict(cam_fixed=cam_fixed, pt_fixed=pt_fixed))
    dxc = dx[:12 * 9].reshape(12, 9)
    dxp = dx[12 * 9:].reshape(120, 3)
    assert np.all(dxc[cam_fixed == 1] == 0.0)
    assert np.all(dxp[pt_fixed == 1] == 0.0)
    assert np.any(dxc[cam_fixed == 0] != 0.0)


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


def test_long_run_point(capfd):
    """A landmark with >64 observations: flagged windows beside staged ones,
    and the XP-padded x filled for the long-run finishers."""
    _triple(capfd, _long_run_problem())


def test_long_run_point_seven_kernel_body(capfd):
    """The same with kPadX as the writer of both x copies."""
    _triple(capfd, _long_run_problem(),
            extra_env={"MEGBA_NO_PCG_FUSE": "1"})


def _weighted_problem():
    rng = np.random.default_rng(9)
    args = mb.synthesize_bal(20, 300, 2600, seed=16)
    w = rng.uniform(0.5, 2.0, (len(args[2]), 2))
    info = np.stack([w[:, 0], 0.1 * np.ones(len(w)), w[:, 1]], axis=1)
    return args, info


def test_weighted_info_and_huber(capfd):
    """The HASINFO instance, without and with a robust loss."""
    args, info = _weighted_problem()
    _triple(capfd, args, info=info)
    _triple(capfd, args, info=info, loss="huber", loss_delta=1.5)


# test_schur_recompute.py::test_recompute_fp32's bound: four times the
# deviation between diff="auto" and diff="analytical" of the default path on
# this problem, as a share of max|deltaX| (measured before the recompute
# path existed).
FP32_BOUND = 4 * 4.7331e-4


def test_fp32(capfd):
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    capfd.readouterr()
    n0, dx0 = _solve({}, args, dtype="float32")
    n1, dx1 = _solve(PER_LANE, args, dtype="float32")
    n2, dx2 = _solve(RC, args, dtype="float32")
    assert _report(capfd) == (["fused-etx", "lds-recompute", "lds-recompute"],
                              ["per-lane", "staged"])
    assert n0 == n1 == n2
    scale = np.abs(dx0).max() or 1.0
    for name, ref in (("default", dx0), ("per-lane", dx1)):
        dev = np.abs(dx2 - ref).max() / scale
        print(f"fp32 staged-vs-{name} deviation / max|deltaX|:", dev)
        assert dev <= FP32_BOUND


def test_two_solves(capfd):
    """A solve, update_params(), a second solve without a new forward: the
    row table still holds the accepted camera part, and the new x."""
    _triple(capfd, mb.synthesize_bal(24, 400, 3600, seed=14), two_solves=True)


def _traj(env, steps=4):
    with _Env(env):
        cams, pts, ci, pi, meas = mb.synthesize_bal(20, 300, 2600, seed=5)
        p = mb.BAProblem(cams, pts, ci, pi, meas)
        p.build(device="gpu", schur="implicit")
        chis = [p.lm_init(force_iterations=True, solver_tol=0.0,
                          solver_refuse_ratio=1e30, solver_max_iter=40)]
        accepted = 0
        for _ in range(steps):
            log = p.lm_step()
            chis.append(log["chi2"])
            accepted += bool(log["accepted"])
        return np.asarray(chis), accepted


def test_graph_matches_eager(capfd):
    """LM trajectories (accepted steps refresh the camera part of the rows):
    captured graph against eager launches, and against the per-lane gather."""
    capfd.readouterr()
    a, acc_a = _traj(RC)
    b, acc_b = _traj(dict(RC, MEGBA_NO_GRAPH="1"))
    c, acc_c = _traj(PER_LANE)
    assert _report(capfd) == (["lds-recompute"] * 3,
                              ["staged", "staged", "per-lane"])
    assert acc_a >= 1 and acc_a == acc_b == acc_c
    np.testing.assert_allclose(a, b, rtol=2e-5)
    np.testing.assert_allclose(a, c, rtol=2e-5)


def test_eager_delta_x(capfd):
    """MEGBA_NO_GRAPH=1: solve_linear captures the PCG body as a graph by
    default, so this is the case that launches it eagerly.  deltaX against
    the default path and the per-lane gather, and against the graph run."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    _, _, dx_eager = _triple(capfd, args, extra_env={"MEGBA_NO_GRAPH": "1"})
    _, dx_graph = _solve(RC, args)
    assert _report(capfd) == (["lds-recompute"], ["staged"])
    _close(dx_eager, dx_graph)


def test_seven_kernel_body(capfd):
    """MEGBA_NO_PCG_FUSE=1: kPadX, not kBetaPPad, writes x into the row
    table.  Also against the rotated body."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    _, _, dx7 = _triple(capfd, args, extra_env={"MEGBA_NO_PCG_FUSE": "1"})
    _, dx4 = _solve(RC, args)
    assert _report(capfd) == (["lds-recompute"], ["staged"])
    _close(dx7, dx4)


def test_fallback_when_the_tiles_do_not_fit(capfd):
    """LDS limit one byte short of accumulator + one tile: the accumulator
    fits, the tiles do not.  The per-lane instance runs with the same result
    and the path is still lds-recompute."""
    ncam = 24
    args = mb.synthesize_bal(ncam, 400, 3600, seed=14)
    short = {"MEGBA_SCHUR_LDS_MAX_BYTES": str(ncam * 9 * 8 + 4095)}
    _triple(capfd, args, staged_env=dict(RC, **short),
            expect_gather="per-lane")


@pytest.mark.parametrize("ncam,threads", [(24, None), (23, None), (23, 192)])
def test_eligibility_boundary(capfd, ncam, threads):
    """The staged instance needs the accumulators, rounded up to 16 bytes,
    plus 4096 bytes per wave: it runs at exactly that limit and not one byte
    below.  23 cameras make the accumulators (1656 B) end off a 16-byte
    boundary; 192 threads are three waves instead of the default eight."""
    args = mb.synthesize_bal(ncam, 400, 3600, seed=14)
    waves = (threads or 512) // 64
    need = (ncam * 9 * 8 + 15) // 16 * 16 + waves * 4096
    env = dict(RC)
    if threads:
        env["MEGBA_SCHUR_LDS_THREADS"] = str(threads)
    capfd.readouterr()
    _, dx_ref = _solve({}, args)
    _, dx_lane = _solve(dict(env, MEGBA_SCHUR_LDS_MAX_BYTES=str(need - 1)),
                        args)
    _, dx_staged = _solve(dict(env, MEGBA_SCHUR_LDS_MAX_BYTES=str(need)),
                          args)
    assert _report(capfd) == (["fused-etx", "lds-recompute", "lds-recompute"],
                              ["per-lane", "staged"])
    _close(dx_lane, dx_ref)
    _close(dx_staged, dx_ref)
    _close(dx_staged, dx_lane)
