"""covariance(method="dense") on the GPU engine: the blocked Cholesky
(dense_cholesky) on random and on failing matrices, the formed Schur
complement (dense_schur) against dense numpy, the covariance against the numpy
oracle, and the checks of test_covariance_dense_cpu.py on the device.

Bounds: the Cholesky residual may be 10x numpy's own on the same matrix (a
different summation order); dense_schur shares PRODUCT_BOUND with the Schur
product tests; the covariance bound is covariance_common.GPU_BOUND (the numpy
dense-Schur route alone: 1.8e-11 on "bal", 7.6e-14 on "632", 5.8e-12 on the
80-camera case)."""
import functools
import json

import numpy as np
import pytest

import megba_amd as mb
from covariance_common import (CAM_IDX, GPU_BOUND, PT_IDX, block_scaled_error,
                               dense_hessian, linearise, make, oracle,
                               request_rows, run_cpp_covariance)
from priors_common import Env, bal_case, make_priors, with_priors
from test_covariance_batch_gpu import (PRODUCT_BOUND, PRODUCT_CASES,
                                       _long_run_args, _product_case)
from test_covariance_dense_cpu import (CHOL_SIZES, FAIL_CASES, _fixed_problem,
                                       check_cholesky, check_cholesky_failure,
                                       check_fixed, check_no_datum,
                                       lm_run_dense)

pytestmark = pytest.mark.gpu


# ---- 1. the factorization --------------------------------------------------
@pytest.fixture(scope="module")
def gpu_engine():
    return with_priors(*bal_case()).build(device="gpu", schur="implicit")


@pytest.mark.parametrize("n", CHOL_SIZES)
def test_dense_cholesky(gpu_engine, n):
    check_cholesky(gpu_engine, n)


@pytest.mark.parametrize("r,d", FAIL_CASES)
def test_dense_cholesky_failure(gpu_engine, r, d):
    check_cholesky_failure(gpu_engine, r, d)


# ---- 2. the formed S against dense numpy -----------------------------------
def check_schur(p, S, name):
    got = p.dense_schur()
    assert got.shape == S.shape
    np.testing.assert_array_equal(got, got.T)
    err = np.abs(got - S).max() / np.abs(S).max()
    print(f"dense_schur {name}: {err:.3g} (bound {PRODUCT_BOUND:.3g})")
    assert err <= PRODUCT_BOUND


@pytest.mark.parametrize("name", list(PRODUCT_CASES))
def test_dense_schur(name):
    p, S = _product_case(name)
    check_schur(p, S, name)


@pytest.mark.parametrize("schur", ["implicit", "explicit"])
def test_dense_schur_row_tiles(schur):
    """80 cameras in LDS row tiles of 32: three tiles, the last one ragged."""
    _, S = _product_case("c-long-run")
    with Env({"MEGBA_DENSE_TILE_CAMS": "32"}):
        p = mb.BAProblem(*_long_run_args()).build(device="gpu", schur=schur)
    linearise(p)
    p.process_diag(np.inf)
    check_schur(p, S, f"c-long-run, 32-camera tiles, {schur}")


# ---- 3. covariance against the numpy oracle --------------------------------
@pytest.mark.parametrize("name,schur", [("bal", "implicit"),
                                        ("bal", "explicit"),
                                        ("632", "implicit")])
def test_oracle(name, schur):
    params, ref = oracle(name)
    cd = params[0].shape[1]
    p = make(name, device="gpu", schur=schur, params=params)
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")
    err = block_scaled_error(cov["joint"], ref, cd)
    print(f"dense {name} {schur}: error {err:.3g} (bound {GPU_BOUND:.3g}), "
          f"min pivot ratio {cov['min_pivot_ratio']:.3g}")
    assert err <= GPU_BOUND
    assert cov["method"] == "dense" and cov["products"] == 0
    assert np.all(cov["iters"] == 0) and cov["converged"].all()
    assert cov["pivot_tol"] < cov["min_pivot_ratio"] <= 1
    np.testing.assert_array_equal(cov["joint"], cov["joint"].T)


BIG_CAMS, BIG_PTS = [0, 7, 79], [3, 100]


@functools.lru_cache(maxsize=None)
def big_case():
    """(80,150,1500) with priors, n = 720: eleven tiles and a ragged twelfth,
    S of condition 4e11.  -> (args, priors, inv(H) rows of the request)."""
    args = mb.synthesize_bal(80, 150, 1500, seed=5)
    priors = make_priors(args)
    ref = with_priors(args, priors).build(device="cpu", schur="explicit")
    linearise(ref)
    rows = request_rows(9, 80, cam_idx=BIG_CAMS, pt_idx=BIG_PTS)
    sub = np.linalg.inv(dense_hessian(ref))[np.ix_(rows, rows)]
    return args, priors, sub


@pytest.mark.parametrize("schur", ["implicit", "explicit"])
def test_oracle_eleven_tiles(schur):
    args, priors, ref = big_case()
    p = with_priors(args, priors).build(device="gpu", schur=schur)
    cov = p.covariance(cam_idx=BIG_CAMS, pt_idx=BIG_PTS, method="dense")
    err = block_scaled_error(cov["joint"], ref, 9, n_cam=len(BIG_CAMS))
    print(f"dense (80,150,1500) {schur}: error {err:.3g} (bound "
          f"{GPU_BOUND:.3g}), min pivot ratio {cov['min_pivot_ratio']:.3g}")
    assert err <= GPU_BOUND


# ---- 4. the CPU checks on the device ---------------------------------------
@pytest.mark.parametrize("method", ["pcg", "dense"])
def test_cross_false(method):
    p = make("bal", device="gpu", schur="implicit", params=oracle("bal")[0])
    full = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method=method)
    own = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method=method,
                       cross=False)
    assert own["joint"] is None
    for key in ("cam_cov", "pt_cov"):
        for a, b in zip(own[key], full[key]):
            np.testing.assert_array_equal(a, a.T)
            rel = np.abs(a - b).max() / np.abs(b).max()
            print(f"cross=False {method} {key}: {rel:.3g}")
            assert rel <= 1e-12
    assert own["converged"].all()


def test_fixed_cameras():
    check_fixed(_fixed_problem(device="gpu"), GPU_BOUND)


def test_no_datum():
    check_no_datum(mb.BAProblem(*bal_case()[0]).build(device="gpu",
                                                      schur="implicit"))


def test_lm_session_unchanged():
    plain, acc, pcg, _ = lm_run_dense(device="gpu")
    chis, acc2, _, cov = lm_run_dense(call_after=2, device="gpu")
    diff = (np.abs(chis - plain) / plain).max()
    print("covariance(method='dense') after step 2: relative difference",
          diff, "min pivot ratio", cov["min_pivot_ratio"])
    assert cov["converged"].all()
    assert acc2 == acc
    assert diff <= 1e-15


# ---- 5. world 2 on one device ----------------------------------------------
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
        cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")
        np.save(f"{out}.joint{rank}.npy", cov["joint"])
        if rank == 0:
            with open(out, "w") as f:
                json.dump({"cut": int(p.index_info()["pt_split"][1])}, f)
    finally:
        dist.destroy_process_group()


def test_world2_single_device(tmp_path):
    import torch.multiprocessing as mp
    params, ref = oracle("bal")
    one = make("bal", device="gpu", schur="implicit", params=params
               ).covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX,
                            method="dense")["joint"]
    out = str(tmp_path / "cov.json")
    mp.spawn(_w2_worker, args=(2, 29583, out), nprocs=2, join=True)
    info = json.loads(open(out).read())
    assert PT_IDX[0] < info["cut"] <= PT_IDX[1]  # one requested point per rank
    j0, j1 = (np.load(f"{out}.joint{r}.npy") for r in (0, 1))
    np.testing.assert_array_equal(j0, j1)
    e1, eo = block_scaled_error(j0, one, 9), block_scaled_error(j0, ref, 9)
    print("dense, world 2 on one device against world 1:", e1,
          "against the oracle:", eo)
    assert e1 <= GPU_BOUND and eo <= GPU_BOUND


# ---- 6. C++ example --------------------------------------------------------
def test_cpp_covariance_example_gpu(tmp_path):
    run_cpp_covariance("gpu", tmp_path)
