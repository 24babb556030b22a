"""Unary priors on the GPU engine (kernels_prior.hpp) against the fp64 CPU
oracle, through every Schur path, on a partial wave, and sharded over two
ranks.  A CPU-only test at the end pins what the LM trajectories of the
Schur-path test contain."""
import json

import numpy as np
import pytest

import megba_amd as mb
from priors_common import (INTR, Env, bal_case, case_632, make_priors,
                           run_cpp_priors, with_priors)


def _pair(args, priors, dtype="float64", **build_kw):
    pc = with_priors(args, priors)
    pc.build(device="cpu", **build_kw)
    pg = with_priors(args, priors)
    pg.build(device="gpu", dtype=dtype, **build_kw)
    return pc, pg


def _compare_stages(pc, pg):
    """forward chi2, the assembled blocks, one damped solve and the gain-
    ratio denominator, fp64 GPU against fp64 CPU."""
    c1, c2 = pc.forward(), pg.forward()
    print("chi2 cpu/gpu", c1, c2)
    np.testing.assert_allclose(c2, c1, rtol=1e-10)
    for p in (pc, pg):
        p.accept_forward()
        p.build_linear_system()
    d1, d2 = pc.dump(), pg.dump()
    for key in ("Hpp", "Hll", "g"):
        scale = np.abs(d1[key]).max() or 1.0
        np.testing.assert_allclose(d2[key], d1[key], rtol=1e-9,
                                   atol=1e-9 * scale, err_msg=key)
    for p in (pc, pg):
        p.process_diag(1e4)
        p.solve_linear(max_iter=500, tol=1e-14, refuse_ratio=1e18)
    dx1, dx2 = pc.dump()["deltaX"], pg.dump()["deltaX"]
    scale = np.abs(dx1).max()
    np.testing.assert_allclose(dx2, dx1, atol=1e-7 * scale)
    for p in (pc, pg):
        p.update_params()
    r1, r2 = pc.rho_denominator(c1), pg.rho_denominator(c2)
    print("rho denominator cpu/gpu", r1, r2)
    np.testing.assert_allclose(r2, r1, rtol=1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_gpu_matches_cpu_bal(schur):
    args, priors = bal_case()
    _compare_stages(*_pair(args, priors, schur=schur))


@pytest.mark.gpu
def test_gpu_matches_cpu_632():
    args, priors = case_632()
    _compare_stages(*_pair(args, priors, intrinsics=INTR))


def _problem_432():
    from test_generic_dims import _wp_np
    rng = np.random.default_rng(31)
    ncam, npt, nobs = 6, 50, 360
    cams = rng.normal(0, 0.1, (ncam, 4))
    pts = rng.normal(0, 1.0, (npt, 3))
    ci = rng.integers(0, ncam, nobs).astype(np.int32)
    pi = np.concatenate(
        [np.arange(npt), rng.integers(0, npt, nobs - npt)]).astype(np.int32)
    ci[:ncam] = np.arange(ncam)
    meas = np.array([_wp_np(cams[c], pts[q], np.zeros(2))
                     for c, q in zip(ci, pi)])
    meas += rng.normal(0, 0.01, meas.shape)
    return cams, pts, ci, pi, meas


@pytest.mark.gpu
def test_gpu_matches_cpu_432_custom_forward():
    """Custom forward: the edge chi2 is written by an overwriting reduction,
    the prior kernels accumulate after it.  No centre prior for these dims."""
    from test_generic_dims import _wp_forward
    args = _problem_432()
    priors = make_priors(args, n_cam=3, n_pt=20, n_ctr=0,
                         custom_forward=_wp_forward)
    _compare_stages(*_pair(args, priors, custom_forward=_wp_forward))


@pytest.mark.gpu
def test_gpu_fp32_stages_vs_fp64_oracle():
    args, priors = bal_case()
    pc, pg = _pair(args, priors, dtype="float32")
    c1, c2 = pc.forward(), pg.forward()
    np.testing.assert_allclose(c2, c1, rtol=2e-3)
    for p in (pc, pg):
        p.accept_forward()
        p.build_linear_system()
    d1, d2 = pc.dump(), pg.dump()
    for key in ("Hpp", "Hll", "g"):
        scale = np.abs(d1[key]).max() or 1.0
        np.testing.assert_allclose(d2[key], d1[key], rtol=2e-3,
                                   atol=2e-4 * scale, err_msg=key)


@pytest.mark.gpu
def test_gpu_partial_wave_tail():
    """65 point priors (one full wave plus one lane) and a one-element
    camera kind."""
    args = bal_case()[0]
    priors = make_priors(args, n_cam=1, n_pt=65, n_ctr=0, seed=11)
    assert len(priors["pt"][0]) == 65 and len(priors["cam"][0]) == 1
    _compare_stages(*_pair(args, priors))


@pytest.mark.gpu
def test_gpu_more_priors_than_the_reduction_grid():
    """The chi2 / rho kernels launch at most 1024 blocks of 256 and stride
    over the rest: 1024 * 256 + 77 point priors make threads take a second
    trip, the last of them in a partial wave."""
    npt = 1024 * 256 + 77
    args = mb.synthesize_bal(40, npt, 2 * npt + 40000, seed=5)
    pts = args[1]
    rng = np.random.default_rng(2)
    info = np.tile(mb.pack_sym(1e3 * np.eye(3)), (npt, 1))
    info[:, 1] = rng.uniform(-100, 100, npt)  # off-diagonals in use
    mean = pts + rng.normal(0, 0.01, pts.shape)
    eng = []
    for device in ("cpu", "gpu"):
        p = mb.BAProblem(*args)
        p.set_point_prior(np.arange(npt), mean, info)
        p.build(device=device, schur="implicit")
        chi = p.forward()
        p.accept_forward()
        p.build_linear_system()
        p.process_diag(1e4)
        p.solve_linear(max_iter=5, tol=0.0, refuse_ratio=1e30)
        p.update_params()
        eng.append((chi, p.rho_denominator(chi)))
    print(eng)
    np.testing.assert_allclose(eng[1][0], eng[0][0], rtol=1e-10)
    np.testing.assert_allclose(eng[1][1], eng[0][1], rtol=1e-8)


@pytest.mark.gpu
def test_gpu_priors_on_fixed_vertices():
    args, priors = bal_case()
    cam_fixed = np.zeros(len(args[0]), dtype=np.uint8)
    pt_fixed = np.zeros(len(args[1]), dtype=np.uint8)
    cam_fixed[[priors["cam"][0][0], priors["ctr"][0][0]]] = 1
    pt_fixed[priors["pt"][0][:3]] = 1
    pc = with_priors(args, priors, cam_fixed=cam_fixed, pt_fixed=pt_fixed)
    pc.build(device="cpu")
    pg = with_priors(args, priors, cam_fixed=cam_fixed, pt_fixed=pt_fixed)
    pg.build(device="gpu")
    _compare_stages(pc, pg)
    dx = pg.dump()["deltaX"]
    assert np.all(dx[:12 * 9].reshape(12, 9)[cam_fixed == 1] == 0.0)
    assert np.all(dx[12 * 9:].reshape(120, 3)[pt_fixed == 1] == 0.0)


# ---- every Schur path ------------------------------------------------------
PATHS = {
    "fused-etx": {},
    "lds": {"MEGBA_SCHUR_LDS": "1"},
    "lds-recompute": {"MEGBA_SCHUR_RECOMPUTE": "1"},
    "lds-recompute/per-lane": {"MEGBA_SCHUR_RECOMPUTE": "1",
                               "MEGBA_NO_RC_STAGE": "1"},
}
# Six-step trajectories that must hold an accepted and a rejected step
# (test_trajectories_reject_cpu): (synthesize_bal kw, make_priors kw, tau).
#
# "tau1e-2": tau is the trust region here (damping diag * (1 + 1/region)) and
# grows at most threefold per accepted step, so within six steps from 1e-2
# the damping never drops below 1 + 1/2.43.  Steps that short are only
# rejected where the Gauss-Newton model is badly wrong, i.e. where the term
# it drops, r^T L d2C/dx2, is large.  Of the three kinds only the centre
# prior is nonlinear, and that term grows with |r|: so its means are GPS
# fixes that contradict the reconstruction by 100 units, ten times the
# radius of the camera ring.  (With means near the estimate all six steps
# are accepted.)  The CPU engine then accepts, accepts, rejects a step that
# would raise chi2 by 15 %, and accepts three more.
#
# "tau1e6": a rougher start (ten times the default perturbation) and a wide
# region: accept, three rejects in a row, two accepts.
TRAJ = {
    "tau1e-2": (dict(), dict(ctr_offset=100.0), 1e-2),
    "tau1e6": (dict(cam_perturb=2e-2, pt_perturb=0.1), dict(), 1e6),
}


def _traj_case(name):
    synth_kw, prior_kw, tau = TRAJ[name]
    args = mb.synthesize_bal(24, 400, 3600, seed=14, **synth_kw)
    return args, make_priors(args, schur="implicit", **prior_kw), tau


def _lm_steps(device, args, priors, tau, env=None):
    with Env(env or {}):
        p = with_priors(args, priors)
        p.build(device=device, schur="implicit")
        chis = [p.lm_init(tau=tau, force_iterations=True, solver_tol=0.0,
                          solver_refuse_ratio=1e30, solver_max_iter=40)]
        acc = []
        for _ in range(6):
            log = p.lm_step()
            chis.append(log["chi2"])
            acc.append(bool(log["accepted"]))
        return acc, np.asarray(chis), p.dump()["deltaX"]


@pytest.mark.gpu
@pytest.mark.parametrize("traj", list(TRAJ))
def test_every_schur_path(capfd, traj):
    """Six LM steps with priors, a rejected one among them, through each
    Schur path: same accept/reject sequence and the same final deltaX as
    the default path."""
    args, priors, tau = _traj_case(traj)
    capfd.readouterr()
    ref = None
    for name, env in PATHS.items():
        acc, chis, dx = _lm_steps("gpu", args, priors, tau, env)
        err = capfd.readouterr().err
        ran = [ln.split(":", 1)[1].strip() for ln in err.splitlines()
               if ln.startswith("# schur path:")]
        assert ran == [name.split("/")[0]], (name, ran)
        if name.startswith("lds-recompute"):
            gather = "per-lane" if name.endswith("per-lane") else "staged"
            assert f"# schur recompute gather: {gather}" in err
        print(name, acc, chis)
        if ref is None:
            ref = (acc, dx)
            continue
        assert acc == ref[0], name
        scale = np.abs(ref[1]).max() or 1.0
        np.testing.assert_allclose(dx, ref[1], rtol=1e-6, atol=1e-9 * scale,
                                   err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("traj", list(TRAJ))
def test_rejecting_trajectory_tracks_cpu(traj):
    """The accepted set (edge r/J and prior r/J) survives rejected steps:
    the GPU trajectory equals the CPU one step by step."""
    args, priors, tau = _traj_case(traj)
    a1, c1, _ = _lm_steps("cpu", args, priors, tau)
    a2, c2, _ = _lm_steps("gpu", args, priors, tau)
    assert a1 == a2
    np.testing.assert_allclose(c2, c1, rtol=1e-5)


# ---- no priors -------------------------------------------------------------
@pytest.mark.gpu
def test_no_priors_tracks_cpu():
    """Guards the early-outs: nothing changes for a problem without priors."""
    args = mb.synthesize_bal(15, 200, 1800, seed=9)
    kw = dict(max_iter=8, tau=1e4, solver_tol=1e-6, solver_max_iter=300,
              solver_refuse_ratio=1e6, verbose=False)
    r1 = mb.BAProblem(*args).build(device="cpu").solve(**kw)
    r2 = mb.BAProblem(*args).build(device="gpu").solve(**kw)
    c1 = [it["chi2"] for it in r1["iters"]]
    c2 = [it["chi2"] for it in r2["iters"]]
    assert len(c1) == len(c2)
    np.testing.assert_allclose(c2, c1, rtol=1e-5)


# ---- world 2 on one device -------------------------------------------------
W2_SHAPE = (15, 160, 1400)
W2_KW = dict(max_iter=6, tau=1e4, solver_tol=1e-6, solver_max_iter=200,
             solver_refuse_ratio=1e6, verbose=False)


def _w2_case():
    args = mb.synthesize_bal(*W2_SHAPE, seed=11)
    return args, make_priors(args, n_cam=4, n_pt=50, n_ctr=4,
                             schur="implicit")


def _w2_worker(rank, world_size, port, out_path):
    import torch.distributed as dist
    from megba_amd.dist import gloo_allreduce_callback
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}",
                            rank=rank, world_size=world_size)
    try:
        args, priors = _w2_case()
        p = with_priors(args, priors)
        p.build(device="gpu", rank=rank, world_size=world_size,
                device_index=0, schur="implicit",
                allreduce=gloo_allreduce_callback())
        rep = p.solve(**W2_KW)
        c2, p2 = p.get_params()  # collective
        if rank == 0:
            np.save(out_path + ".pts.npy", p2)
            np.save(out_path + ".cams.npy", c2)
            with open(out_path, "w") as f:
                json.dump({"chis": [it["chi2"] for it in rep["iters"]],
                           "cut": int(p.index_info()["pt_split"][1])}, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_gpu_world2_single_device(tmp_path):
    import torch.multiprocessing as mp
    args, priors = _w2_case()
    p1 = with_priors(args, priors)
    p1.build(device="gpu", schur="implicit")
    rep = p1.solve(**W2_KW)
    ref = [it["chi2"] for it in rep["iters"]]
    c1, q1 = p1.get_params()
    out = tmp_path / "chis.json"
    mp.spawn(_w2_worker, args=(2, 29543, str(out)), nprocs=2, join=True)
    got = json.loads(out.read_text())
    idx = priors["pt"][0]
    assert (idx < got["cut"]).any() and (idx >= got["cut"]).any()
    assert len(got["chis"]) == len(ref)
    np.testing.assert_allclose(got["chis"], ref, rtol=1e-6)
    np.testing.assert_allclose(np.load(str(out) + ".pts.npy"), q1,
                               rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(np.load(str(out) + ".cams.npy"), c1,
                               rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
def test_cpp_priors_example_gpu(tmp_path):
    run_cpp_priors("gpu", tmp_path)


# ---- CPU: the trajectories above -------------------------------------------
@pytest.mark.parametrize("traj", list(TRAJ))
def test_trajectories_reject_cpu(traj):
    """Each trajectory of test_every_schur_path holds an accepted and a
    rejected step, and an accepted one after the first rejected one (so an
    assembly and a gain ratio read the accepted set after a reject)."""
    args, priors, tau = _traj_case(traj)
    acc = _lm_steps("cpu", args, priors, tau)[0]
    print(acc)
    assert any(acc) and not all(acc)
    assert any(acc[acc.index(False):])
