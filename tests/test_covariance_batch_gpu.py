"""covariance(batch=...) on the GPU engine: the batched Schur product against
dense numpy, the batched PCG against the dense oracle and against the column
loop (fixed vertices, no datum, a running LM session, two ranks on one
device), and the C++ example.

Product tolerance.  max|S X - ref| / max|ref| of the EXISTING product
(schur_apply(batched=False)) over the cases and widths of test_product,
measured on an MI355X: PRODUCT_MEASURED below (the batched kernels measured
PRODUCT_MEASURED_BATCHED on the same runs).  The bound for both paths is 10x
the figure of the existing path; the x10 covers the different summation
order, as covariance_common.GPU_BOUND does."""
import functools
import json

import numpy as np
import pytest

import megba_amd as mb
from covariance_common import (CAM_IDX, GPU_BOUND, PT_IDX, block_scaled_error,
                               dense_hessian, linearise, lm_run, make, oracle,
                               run_cpp_covariance)
from priors_common import (INTR, Env, bal_case, case_632, make_priors,
                           with_priors)

pytestmark = pytest.mark.gpu

PRODUCT_MEASURED = 1.7e-14          # existing path: 1.696e-14, b-chunk32 k=1
PRODUCT_MEASURED_BATCHED = 1.7e-14  # batched path: 1.696e-14, the same run
PRODUCT_BOUND = 10 * PRODUCT_MEASURED  # 1.7e-13


# ---- 1. product against dense numpy ----------------------------------------
def _long_run_args():
    """(80,150,1500) plus an observation of point 0 from every camera that
    does not see it yet: a run of 80 edges, which crosses a wave edge.  The
    same for the point whose run then straddles edge 256, a block edge."""
    cams, pts, ci, pi, meas = mb.synthesize_bal(80, 150, 1500, seed=5)
    ci, pi = np.asarray(ci), np.asarray(pi)

    def observe_from_all(q, ci, pi, meas):
        extra = np.setdiff1d(np.arange(len(cams)), ci[pi == q])
        return (np.r_[ci, extra], np.r_[pi, np.full(len(extra), q)],
                np.r_[meas, np.zeros((len(extra), 2))])

    ci, pi, meas = observe_from_all(0, ci, pi, meas)
    first = np.r_[0, np.cumsum(np.bincount(pi, minlength=len(pts)))]
    q = next(q for q in range(1, len(pts))
             if first[q] < 256 < first[q] + len(cams))
    ci, pi, meas = observe_from_all(int(q), ci, pi, meas)
    first = np.r_[0, np.cumsum(np.bincount(pi, minlength=len(pts)))]
    assert first[1] == 80 and first[q] < 256 < first[q + 1]
    return cams, pts, ci.astype(np.int32), pi.astype(np.int32), meas


def _weighted_kw():
    """Per-edge information, one fixed camera and one fixed point."""
    args = bal_case()[0]
    rng = np.random.default_rng(21)
    a = rng.normal(size=(len(args[2]), 2, 2))
    w = a @ a.transpose(0, 2, 1) + 2 * np.eye(2)
    cam_fixed = np.zeros(len(args[0]), dtype=np.uint8)
    pt_fixed = np.zeros(len(args[1]), dtype=np.uint8)
    cam_fixed[3] = pt_fixed[10] = 1
    return dict(info=np.stack([w[:, 0, 0], w[:, 0, 1], w[:, 1, 1]], axis=1),
                cam_fixed=cam_fixed, pt_fixed=pt_fixed)


# name -> (problem factory, build keywords, knobs at build time, Schur mode)
PRODUCT_CASES = {
    "a-bal": (lambda: with_priors(*bal_case()), {}, {}, "implicit"),
    "b-chunk32": (lambda: with_priors(*bal_case()), {}, {"MEGBA_CHUNK": "32"},
                  "implicit"),
    "c-long-run": (lambda: mb.BAProblem(*_long_run_args()), {}, {},
                   "implicit"),
    "d-weighted": (lambda: mb.BAProblem(*bal_case()[0], **_weighted_kw()),
                   {"loss": "huber"}, {}, "implicit"),
    "e-632": (lambda: with_priors(*case_632()), {"intrinsics": INTR}, {},
              "implicit"),
    # the explicit twins over Hpl
    "a-explicit": (lambda: with_priors(*bal_case()), {},
                   {"MEGBA_CHUNK": "32"}, "explicit"),
    "c-explicit": (lambda: mb.BAProblem(*_long_run_args()), {}, {},
                   "explicit"),
    "d-explicit": (lambda: mb.BAProblem(*bal_case()[0], **_weighted_kw()),
                   {"loss": "huber"}, {}, "explicit"),
    "e-explicit": (lambda: with_priors(*case_632()), {"intrinsics": INTR}, {},
                   "explicit"),
}


@functools.lru_cache(maxsize=None)
def _product_case(name):
    """(GPU problem ready for schur_apply, dense S) of a case, built once."""
    factory, build_kw, knobs, schur = PRODUCT_CASES[name]
    ref = factory().build(device="cpu", schur="explicit", **build_kw)
    linearise(ref)
    ref.process_diag(np.inf)
    H = dense_hessian(ref)
    nc = ref.cams.size
    S = H[:nc, :nc] - H[:nc, nc:] @ np.linalg.solve(H[nc:, nc:], H[nc:, :nc])
    S.setflags(write=False)
    with Env(knobs):
        p = factory().build(device="gpu", schur=schur, **build_kw)
    linearise(p)
    p.process_diag(np.inf)
    return p, S


@pytest.mark.parametrize("name", list(PRODUCT_CASES))
def test_product(name):
    p, S = _product_case(name)
    cd = p.cams.shape[1]
    assert p.max_batch() == cd
    rng = np.random.default_rng(8)
    worst = {False: 0.0, True: 0.0}
    for k in (1, 2, 3, cd):
        X = rng.normal(size=(S.shape[0], k))
        ref = S @ X
        for batched in (False, True):
            got = p.schur_apply(X, batched=batched)
            assert got.shape == X.shape
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"product {name} k={k} batched={batched}: {err:.3g}")
            worst[batched] = max(worst[batched], err)
    print(f"product {name}: existing {worst[False]:.3g}, batched "
          f"{worst[True]:.3g}, bound {PRODUCT_BOUND:.3g}")
    assert worst[False] <= PRODUCT_BOUND
    assert worst[True] <= PRODUCT_BOUND


def test_product_hook_checks():
    p, S = _product_case("a-bal")
    with pytest.raises(RuntimeError, match="megba:.*schur_apply"):
        p.schur_apply(np.zeros((S.shape[0], 10)), batched=True)
    with pytest.raises(RuntimeError, match="megba:.*schur_apply"):
        p.schur_apply(np.zeros((S.shape[0] + 1, 2)), batched=True)


# ---- 2. covariance against the oracle --------------------------------------
def _n_batches(cd, batch, n_cam=len(CAM_IDX), n_pt=len(PT_IDX)):
    """Batched solves of the request: a batch never spans two vertices."""
    w = min(batch, cd)
    return n_cam * -(-cd // w) + n_pt * -(-3 // w)


@pytest.mark.parametrize("name,schur,batch", [
    ("bal", "implicit", 9), ("bal", "implicit", 3), ("632", "implicit", 6),
    ("632", "implicit", 3), ("bal", "explicit", 9), ("632", "explicit", 3)])
def test_oracle_batched(name, schur, batch):
    params, ref = oracle(name)
    cd = params[0].shape[1]
    p = make(name, device="gpu", schur=schur, params=params)
    one = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=1)
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=batch)
    err = block_scaled_error(cov["joint"], ref, cd)
    nb = _n_batches(cd, batch)
    print(f"{name} {schur} batch={batch}: error {err:.3g} (bound "
          f"{GPU_BOUND:.3g}), iters {cov['iters']} against {one['iters']}, "
          f"products {cov['products']} in {nb} batches against "
          f"{one['products']}")
    assert cov["converged"].all()
    assert err <= GPU_BOUND
    np.testing.assert_array_equal(cov["joint"], cov["joint"].T)
    assert np.abs(cov["iters"] - one["iters"]).max() <= 1
    assert one["products"] == int((one["iters"] + 1).sum())
    assert cov["products"] <= nb * (cov["iters"].max() + 2)
    assert cov["products"] * 2 < cov["iters"].sum()  # really batched


def test_float32_has_no_batched_product():
    p = with_priors(*bal_case()).build(device="gpu", dtype="float32",
                                       schur="implicit")
    assert p.max_batch() == 1


# ---- 3. fixed vertices -----------------------------------------------------
def test_fixed_vertices():
    """Fixed cameras 0 and 5 are the only datum; camera 5 is requested."""
    args = bal_case()[0]
    cam_fixed = np.zeros(len(args[0]), dtype=np.uint8)
    cam_fixed[[0, 5]] = 1
    p = mb.BAProblem(*args, cam_fixed=cam_fixed).build(device="gpu",
                                                       schur="implicit")
    one = p.covariance(cam_idx=[5, 2], pt_idx=PT_IDX, batch=1)
    cov = p.covariance(cam_idx=[5, 2], pt_idx=PT_IDX, batch=9)
    joint = cov["joint"]
    assert np.all(joint[:9, :] == 0.0) and np.all(joint[:, :9] == 0.0)
    assert np.all(cov["iters"][:9] == 0) and np.all(cov["iters"][9:] > 0)
    assert cov["converged"].all()
    err = block_scaled_error(joint[9:, 9:], one["joint"][9:, 9:], 9, n_cam=1)
    print("fixed: batched against the column loop", err, "products",
          cov["products"])
    assert err <= GPU_BOUND
    # one camera batch and two point batches: the fixed camera is not solved
    assert cov["products"] <= 3 * (cov["iters"].max() + 2)


# ---- 4. no datum -----------------------------------------------------------
def test_no_datum_flags():
    """Without a datum the f, k1, k2 columns converge and the pose and point
    columns do not (test_covariance_cpu.py says why): converged columns
    freeze next to columns that never stop."""
    args = bal_case()[0]
    p = mb.BAProblem(*args).build(device="gpu", schur="implicit")
    one = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200,
                       strict=False, batch=1)
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200,
                       strict=False, batch=9)
    print("no datum: iters", cov["iters"], "against", one["iters"])
    np.testing.assert_array_equal(cov["converged"], one["converged"])
    assert cov["converged"][np.r_[6:9, 15:18]].all()
    assert not cov["converged"][np.r_[0:6, 9:15, 18:24]].any()
    with pytest.raises(RuntimeError, match=r"megba:.*gauge"):
        p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, max_iter=200, batch=9)


# ---- 5. state --------------------------------------------------------------
# test_covariance_gpu.py: two plain GPU runs of the trajectory differ by
# 2.0e-16 relative, and the tolerance is 10x that spread.
STATE_SPREAD = 2.0e-16


def test_lm_state_preserved():
    plain, acc, _, _ = lm_run(device="gpu")
    args = mb.synthesize_bal(24, 400, 3600, seed=14, cam_perturb=2e-2,
                             pt_perturb=0.1)
    p = with_priors(args, make_priors(args, schur="implicit"))
    p.build(device="gpu", schur="implicit")
    chis = [p.lm_init(tau=1e6, force_iterations=True, solver_tol=0.0,
                      solver_refuse_ratio=1e30, solver_max_iter=40)]
    acc2 = []
    for k in range(6):
        log = p.lm_step()
        chis.append(log["chi2"])
        acc2.append(bool(log["accepted"]))
        if k == 0:
            cov = p.covariance(cam_idx=[1, 20], pt_idx=[7, 399], strict=False,
                               batch=9)
    diff = (np.abs(np.array(chis) - plain) / plain).max()
    print("covariance(batch=9) after step 1: relative difference", diff,
          "iters", cov["iters"])
    assert cov["iters"].min() > 0
    assert acc2 == acc
    assert diff <= 10 * STATE_SPREAD


# ---- 6. world 2 on one device ----------------------------------------------
def _w2_worker(rank, world_size, port, out):
    import torch.distributed as dist
    from megba_amd.dist import gloo_allreduce_callback
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}",
                            rank=rank, world_size=world_size)
    try:
        params, _ = oracle("bal")
        p = make("bal", device="gpu", schur="implicit", params=params,
                 rank=rank, world_size=world_size, device_index=0,
                 allreduce=gloo_allreduce_callback())
        cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=9)
        np.save(f"{out}.joint{rank}.npy", cov["joint"])
        if rank == 0:
            with open(out, "w") as f:
                json.dump({"cut": int(p.index_info()["pt_split"][1]),
                           "products": int(cov["products"]),
                           "iters": [int(i) for i in cov["iters"]]}, f)
    finally:
        dist.destroy_process_group()


def test_world2_single_device(tmp_path):
    import torch.multiprocessing as mp
    params, ref = oracle("bal")
    out = str(tmp_path / "cov.json")
    mp.spawn(_w2_worker, args=(2, 29561, out), nprocs=2, join=True)
    info = json.loads(open(out).read())
    assert PT_IDX[0] < info["cut"] <= PT_IDX[1]  # one requested point per rank
    j0, j1 = (np.load(f"{out}.joint{r}.npy") for r in (0, 1))
    np.testing.assert_array_equal(j0, j1)
    err = block_scaled_error(j0, ref, 9)
    print("world 2 on one device, batch=9, against the oracle:", err, info)
    assert err <= GPU_BOUND
    assert info["products"] * 2 < sum(info["iters"])


# ---- 7. C++ example --------------------------------------------------------
def test_cpp_covariance_example_gpu(tmp_path):
    run_cpp_covariance("gpu", tmp_path)
