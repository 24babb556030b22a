"""GPU tests for the LDS single-pass Schur apply (kSchurFusedLds,
MEGBA_SCHUR_LDS=1): one pass over the pt-sorted J with a per-workgroup
camera accumulator in LDS, flushed to per-workgroup rows and summed in
fixed order.  Every case solves the same damped system with the default
two-pass path and with the LDS path and compares deltaX; the engine's
MEGBA_TUNE_VERBOSE line tells which path actually ran.
"""
import os

import numpy as np
import pytest

import megba_amd as mb

pytestmark = pytest.mark.gpu

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


def _solve(env, schur, args, info=None, dtype="float64", **build_kw):
    with _Env(env):
        p = mb.BAProblem(*args, info=info)
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


def _pair(capfd, schur, args, info=None, lds_env=LDS, expect="lds",
          **build_kw):
    capfd.readouterr()
    n1, dx1 = _solve({}, schur, args, info=info, **build_kw)
    assert _path(capfd) == ["fused-etx"]
    n2, dx2 = _solve(lds_env, schur, args, info=info, **build_kw)
    assert _path(capfd) == [expect]
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    np.testing.assert_allclose(dx2, dx1, rtol=1e-6, atol=1e-9 * scale)


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_lds_matches_default(capfd, schur):
    _pair(capfd, schur, mb.synthesize_bal(24, 400, 3600, seed=14))


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
def test_lds_long_run_point(capfd, schur):
    """A landmark with >64 observations: flagged windows, temp partials and
    the global long-run finishers after the flush."""
    _pair(capfd, schur, _long_run_problem())


def _weighted_problem():
    rng = np.random.default_rng(9)
    args = mb.synthesize_bal(20, 300, 2600, seed=16)
    w = rng.uniform(0.5, 2.0, (len(args[2]), 2))
    info = np.stack([w[:, 0], 0.1 * np.ones(len(w)), w[:, 1]], axis=1)
    return args, info


def test_lds_weighted_info(capfd):
    args, info = _weighted_problem()
    _pair(capfd, "implicit", args, info=info)


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_lds_robust_loss(capfd, loss):
    args, info = _weighted_problem()
    _pair(capfd, "implicit", args, info=info, loss=loss, loss_delta=1.5)


def test_lds_starved_grid(capfd):
    """Fewer windows than workgroups: most workgroups own an empty slice and
    flush a zero row."""
    _pair(capfd, "implicit", mb.synthesize_bal(6, 40, 240, seed=3))


def _dims632_problem():
    """(6,3,2) problem with shared intrinsics: (args, intrinsics)."""
    intr = [420.0, -1e-7, 3e-13]
    cams9, pts, ci, pi, meas0 = mb.synthesize_bal(12, 110, 950, seed=12)
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


def test_lds_other_block_dims(capfd):
    """(6,3,2): the LDS index cam*CD+i with CD != 9."""
    args, intr = _dims632_problem()
    for schur in ("explicit", "implicit"):
        _pair(capfd, schur, args, intrinsics=intr)


def test_lds_fallback_when_over_limit(capfd):
    """A camera vector over the (lowered) LDS limit keeps today's path even
    when the LDS path is forced."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    need = 24 * 9 * 8
    env = dict(LDS, MEGBA_SCHUR_LDS_MAX_BYTES=str(need - 1))
    _pair(capfd, "implicit", args, lds_env=env, expect="fused-etx")
    # exactly at the limit it is eligible
    env = dict(LDS, MEGBA_SCHUR_LDS_MAX_BYTES=str(need))
    _pair(capfd, "implicit", args, lds_env=env, expect="lds")


def test_lds_excluded_by_env(capfd):
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    env = dict(LDS, MEGBA_NO_SCHUR_LDS="1")
    _pair(capfd, "implicit", args, lds_env=env, expect="fused-etx")


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


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_lds_graph_matches_eager(capfd, schur):
    capfd.readouterr()
    a = _traj(schur, LDS)
    b = _traj(schur, dict(LDS, MEGBA_NO_GRAPH="1"))
    assert _path(capfd) == ["lds", "lds"]
    np.testing.assert_allclose(a, b, rtol=2e-5)


def test_lds_three_way_autotune(capfd):
    """Just above the 200k-edge threshold the first solve times LDS
    single-pass, fused E^T x + Cinv and separate passes on the real data."""
    capfd.readouterr()
    with _Env({}):
        cams, pts, ci, pi, meas = mb.synthesize_bal(50, 30000, 210000,
                                                    seed=23)
        p = mb.BAProblem(cams, pts, ci, pi, meas)
        p.build(device="gpu", schur="implicit")
        chi0 = p.lm_init(force_iterations=True, solver_tol=0.0,
                         solver_refuse_ratio=1e30, solver_max_iter=30)
        log = p.lm_step()
    err = capfd.readouterr().err
    tune = [ln for ln in err.splitlines() if ln.startswith("# schur autotune")]
    assert len(tune) == 1
    # all three candidates were timed (an ineligible LDS path prints -1)
    times = [float(t.split(" ms")[0].split()[-1])
             for t in tune[0].split(",")]
    assert len(times) == 3 and all(t > 0 for t in times), tune[0]
    assert np.isfinite(log["chi2"]) and log["chi2"] <= chi0


# fp32: the bound comes from the parent's own two paths, not from the LDS
# kernel.  On this problem the parent's default path and its MEGBA_FUSED=1
# path differ by at most FP32_PARENT_DEV * max|deltaX| (measured on MI355X:
# 1.8714e-4, with max|deltaX| = 1.878; two default runs of the parent agree
# bit for bit there); the LDS path is allowed four times that, 7.4856e-4.
FP32_PARENT_DEV = 1.8714e-4
FP32_BOUND = 4 * FP32_PARENT_DEV


def test_lds_fp32(capfd):
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    capfd.readouterr()
    n1, dx1 = _solve({}, "implicit", args, dtype="float32")
    n2, dx2 = _solve(LDS, "implicit", args, dtype="float32")
    assert _path(capfd) == ["fused-etx", "lds"]
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    dev = np.abs(dx2 - dx1).max() / scale
    print("fp32 lds-vs-default deviation / max|deltaX|:", dev)
    assert dev <= FP32_BOUND


# ---------------------------------------------------------------------------
# Separate-pass path (MEGBA_NO_ETXFUSE=1: kSpmvEtx / kSpmvEtxPk + kCinvPad)
# and its scan-free E^T x variant (MEGBA_ETX_ATOMIC=1: kSpmvEtxPkAtomic),
# value-checked against the default path like the LDS cases above.
# ---------------------------------------------------------------------------
SEP = {"MEGBA_NO_ETXFUSE": "1"}
SEP_ATOMIC = {"MEGBA_NO_ETXFUSE": "1", "MEGBA_ETX_ATOMIC": "1"}


def _sep_pair(capfd, schur, args, env=SEP, **kw):
    _pair(capfd, schur, args, lds_env=env, expect="separate", **kw)


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_separate_matches_default(capfd, schur):
    _sep_pair(capfd, schur, mb.synthesize_bal(24, 400, 3600, seed=14))


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_separate_long_run_point(capfd, schur):
    """A >64-edge run crosses wave edges in the block-tiled scan."""
    _sep_pair(capfd, schur, _long_run_problem())


def test_separate_weighted_info(capfd):
    args, info = _weighted_problem()
    _sep_pair(capfd, "implicit", args, info=info)


def test_separate_robust_loss(capfd):
    args, info = _weighted_problem()
    _sep_pair(capfd, "implicit", args, info=info, loss="huber",
              loss_delta=1.5)


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_separate_other_block_dims(capfd, schur):
    args, intr = _dims632_problem()
    _sep_pair(capfd, schur, args, intrinsics=intr)


def test_separate_atomic_matches_default(capfd):
    _sep_pair(capfd, "implicit", mb.synthesize_bal(24, 400, 3600, seed=14),
              env=SEP_ATOMIC)


def test_separate_atomic_robust_loss(capfd):
    args, info = _weighted_problem()
    _sep_pair(capfd, "implicit", args, env=SEP_ATOMIC, info=info,
              loss="huber", loss_delta=1.5)


# fp32, separate vs default: the bound comes from the code before the shared
# edge primitives existed.  There the separate-pass path and the default
# path differ on this problem by FP32_SEP_PARENT_DEV * max|deltaX| (measured
# on MI355X: 6.5575e-5, with max|deltaX| = 1.878); the separate path is
# allowed four times that, 2.6230e-4.
FP32_SEP_PARENT_DEV = 6.5575e-5
FP32_SEP_BOUND = 4 * FP32_SEP_PARENT_DEV


def test_separate_fp32(capfd):
    args = mb.synthesize_bal(24, 400, 3600, seed=14)
    capfd.readouterr()
    n1, dx1 = _solve({}, "implicit", args, dtype="float32")
    n2, dx2 = _solve(SEP, "implicit", args, dtype="float32")
    assert _path(capfd) == ["fused-etx", "separate"]
    assert n1 == n2
    scale = np.abs(dx1).max() or 1.0
    dev = np.abs(dx2 - dx1).max() / scale
    print("fp32 separate-vs-default deviation / max|deltaX|:", dev,
          "max|deltaX|:", scale)
    assert dev <= FP32_SEP_BOUND
