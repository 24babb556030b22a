"""GPU tests for the rotated PCG body with merged vector kernels
(kBetaPPad, kLdsReduceBApplyDot, kUpdateXRPrecond).  Every case solves the
same damped system with MEGBA_NO_PCG_FUSE=1 (the seven-kernel body) and
without it and compares iteration counts and deltaX; the engine's
MEGBA_TUNE_VERBOSE line tells which Schur path ran.  The two bodies differ
through partial-sum order and multiply-add fusing only, so the bounds are
those tests/test_schur_lds.py uses between two of the engine's own paths.
"""
import os

import numpy as np
import pytest

import megba_amd as mb

pytestmark = pytest.mark.gpu

NOFUSE = {"MEGBA_NO_PCG_FUSE": "1"}
LDS = {"MEGBA_SCHUR_LDS": "1"}
SEP = {"MEGBA_NO_ETXFUSE": "1"}
PATHS = {"default": ({}, "fused-etx"), "lds": (LDS, "lds"),
         "separate": (SEP, "separate")}

# fp32 bound of tests/test_schur_lds.py on the seed-14 problem, relative to
# max|deltaX|: four times the deviation between two paths of the code before
# the LDS kernel existed (1.8714e-4, measured on MI355X).
FP32_BOUND = 7.4856e-4


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


def _solve(env, schur, args, info=None, dtype="float64", device="gpu",
           max_iter=30, tol=0.0, refuse_ratio=1e30, **build_kw):
    with _Env(env):
        p = mb.BAProblem(*args, info=info)
        p.build(device=device, dtype=dtype, schur=schur, **build_kw)
        p.forward()
        p.accept_forward()
        p.build_linear_system()
        p.process_diag(1e4)
        n = p.solve_linear(max_iter=max_iter, tol=tol,
                           refuse_ratio=refuse_ratio)
        return n, p.dump()["deltaX"]


def _path(capfd):
    """Path names the engines built since the last call reported."""
    err = capfd.readouterr().err
    return [ln.split(":", 1)[1].strip() for ln in err.splitlines()
            if ln.startswith("# schur path:")]


def _close64(dx, ref):
    scale = np.abs(ref).max() or 1.0
    print("max|dx - ref| / max|ref|:", np.abs(dx - ref).max() / scale)
    np.testing.assert_allclose(dx, ref, rtol=1e-6, atol=1e-9 * scale)


def _pair(capfd, schur, args, env, expect, **kw):
    """Unfused body against fused body on one Schur path."""
    capfd.readouterr()
    n1, dx1 = _solve(dict(env, **NOFUSE), schur, args, **kw)
    n2, dx2 = _solve(env, schur, args, **kw)
    assert _path(capfd) == [expect, expect]
    assert n1 == n2
    _close64(dx2, dx1)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_fused_matches_unfused(capfd, schur, path):
    """nc = 216 is no multiple of 64 and camera 7 straddles the first
    64-column block edge of kLdsReduceBApplyDot."""
    env, expect = PATHS[path]
    _pair(capfd, schur, mb.synthesize_bal(24, 400, 3600, seed=14), env,
          expect)


def test_fused_fp32_lds(capfd):
    """fp32: the 12-wide pad with three zero lanes."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    capfd.readouterr()
    n1, dx1 = _solve(dict(LDS, **NOFUSE), "implicit", args, dtype="float32")
    n2, dx2 = _solve(LDS, "implicit", args, dtype="float32")
    assert _path(capfd) == ["lds", "lds"]
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    dev = np.abs(dx2 - dx1).max() / scale
    print("fp32 fused-vs-unfused deviation / max|deltaX|:", dev)
    assert dev <= FP32_BOUND


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


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_fused_several_camera_blocks_and_long_run(capfd, schur):
    """90 cameras: kUpdateXRPrecond runs four blocks of whole cameras, the
    last one partial.  The >64-edge point keeps the long-run finishers
    between the row reduce and the B-apply, so those stay separate."""
    _pair(capfd, schur, _long_run_problem(), LDS, "lds")


def test_fused_fewer_cameras_than_one_block(capfd):
    """6 cameras: one partial kUpdateXRPrecond block; most LDS workgroups
    own an empty slice."""
    _pair(capfd, "implicit", mb.synthesize_bal(6, 40, 240, seed=3), LDS,
          "lds")


def _dims632_problem():
    """(6,3,2) problem with shared intrinsics and 50 cameras, more than the
    42 one kUpdateXRPrecond block owns at CD = 6: (args, intrinsics)."""
    intr = [420.0, -1e-7, 3e-13]
    cams9, pts, ci, pi, meas0 = mb.synthesize_bal(50, 300, 3000, seed=12)
    cams9[:, 6:9] = intr
    # measurements consistent with the shared intrinsics, plus noise
    p = mb.BAProblem(cams9, pts, ci, pi, np.zeros_like(meas0))
    p.build(device="cpu")
    p.forward()
    r_sorted = p.dump()["r"].reshape(-1, 2)
    r = np.empty_like(r_sorted)
    r[p.index_info()["perm"]] = r_sorted
    meas = r + np.random.default_rng(112).normal(0, 0.5, r.shape)
    return (cams9[:, :6].copy(), pts, ci, pi, meas), intr


@pytest.fixture(scope="module")
def dims632():
    return _dims632_problem()


@pytest.mark.parametrize("path", ["default", "lds"])
@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_fused_cd6(capfd, dims632, schur, path):
    """CD = 6: no pad lanes in fp64, 42 cameras per block."""
    args, intr = dims632
    env, expect = PATHS[path]
    _pair(capfd, schur, args, env, expect, intrinsics=intr)


def _weighted_problem():
    rng = np.random.default_rng(9)
    args = mb.synthesize_bal(20, 300, 2600, seed=16)
    w = rng.uniform(0.5, 2.0, (len(args[2]), 2))
    info = np.stack([w[:, 0], 0.1 * np.ones(len(w)), w[:, 1]], axis=1)
    return args, info


def test_fused_weighted_huber(capfd):
    args, info = _weighted_problem()
    _pair(capfd, "implicit", args, LDS, "lds", info=info, loss="huber",
          loss_delta=1.5)


def test_fused_forced_communicator(capfd):
    """A real world-1 communicator: the allreduce sits between the row
    reduce and the B-apply, so those stay separate."""
    env = dict(LDS, MEGBA_FORCE_RCCL="1")
    _pair(capfd, "implicit", mb.synthesize_bal(24, 400, 3600, seed=14), env,
          "lds")


def test_nontemporal_stream_several_windows_per_workgroup(capfd):
    """The LDS kernel streams the packed J with non-temporal loads.  On the
    small problems every workgroup owns at most one window; here (the size
    of the three-way autotune test) each owns several.  There is no switch
    for the load policy, so the comparison is against the two-pass path,
    whose kernels load J with the default policy, at the bound
    tests/test_schur_lds.py sets between these two paths."""
    args = mb.synthesize_bal(50, 30000, 210000, seed=23)
    capfd.readouterr()
    n1, dx1 = _solve({"MEGBA_NO_SCHUR_LDS": "1", "MEGBA_ETXFUSE": "1"},
                     "implicit", args)
    n2, dx2 = _solve(LDS, "implicit", args)
    assert _path(capfd) == ["fused-etx", "lds"]
    assert n1 == n2
    _close64(dx2, dx1)


# Refuse and tol control flow: after body n the host reads the rho of the
# residual before update n, whichever kernel published it.  The seed is one
# on which the CPU engine and the seven-kernel GPU body return the same
# counts for both solves.
CONTROL_SEED = 5


@pytest.mark.parametrize("knobs", [
    dict(max_iter=500, tol=1e-12, refuse_ratio=1.0),
    dict(max_iter=500, tol=1e-8, refuse_ratio=1e18),
], ids=["refuse", "tol"])
@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_fused_refuse_and_tol_match_cpu(schur, knobs):
    args = mb.synthesize_bal(8, 60, 460, seed=CONTROL_SEED)
    n_cpu, dx_cpu = _solve({}, schur, args, device="cpu", **knobs)
    n_gpu, dx_gpu = _solve({}, schur, args, **knobs)
    print("iterations cpu/gpu:", n_cpu, n_gpu)
    assert n_gpu == n_cpu
    _close64(dx_gpu, dx_cpu)


def _traj(schur, env, steps=4):
    with _Env(env):
        cams, pts, ci, pi, meas = mb.synthesize_bal(20, 300, 2600, seed=5)
        p = mb.BAProblem(cams, pts, ci, pi, meas)
        p.build(device="gpu", schur=schur)
        chis = [p.lm_init(force_iterations=True, solver_tol=0.0,
                          solver_refuse_ratio=1e30, solver_max_iter=40)]
        for _ in range(steps):
            chis.append(p.lm_step()["chi2"])
        return np.asarray(chis)


@pytest.mark.parametrize("schur,env,expect", [
    ("implicit", LDS, "lds"), ("explicit", {}, "fused-etx")])
def test_fused_graph_eager_and_unfused_trajectories(capfd, schur, env,
                                                    expect):
    """Four LM steps: a stale padded copy or a stale partial surviving from
    one step into the next would show against the eager run or against the
    seven-kernel body."""
    capfd.readouterr()
    a = _traj(schur, env)
    b = _traj(schur, dict(env, MEGBA_NO_GRAPH="1"))
    c = _traj(schur, dict(env, **NOFUSE))
    assert _path(capfd) == [expect] * 3
    np.testing.assert_allclose(a, b, rtol=2e-5)
    np.testing.assert_allclose(a, c, rtol=2e-5)
