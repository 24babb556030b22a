"""covariance(method="dense") on the CPU engine: the dense Cholesky route
against the numpy oracle and against the PCG route, its result fields,
cross=False, fixed vertices, the no-datum failure, a running LM session, the
dense_schur / dense_cholesky hooks and two ranks over gloo.

The bounds are those of covariance_common (the numpy dense-Schur route alone
sits at 1.8e-11 on "bal" and 7.6e-14 on "632" against the numpy inverse)."""
import json

import numpy as np
import pytest

import megba_amd as mb
from covariance_common import (CAM_IDX, CPU_BOUND, PT_IDX, block_scaled_error,
                               dense_hessian, linearise, make, oracle,
                               request_rows)
from priors_common import bal_case, make_priors, with_priors

T = 64  # Cholesky tile
PRODUCT_BOUND = 1.7e-13  # tests/test_covariance_batch_gpu.py
PIVOT_TOL = float(np.sqrt(np.finfo(np.float64).eps))

CASES = [("bal", "explicit"), ("bal", "implicit"), ("632", "explicit"),
         ("632", "implicit")]


def _problem(name, schur):
    return make(name, schur=schur, params=oracle(name)[0])


# ---- oracle, PCG, fields ---------------------------------------------------
@pytest.mark.parametrize("name,schur", CASES)
def test_oracle(name, schur):
    params, ref = oracle(name)
    cd = params[0].shape[1]
    cov = _problem(name, schur).covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX,
                                           method="dense")
    err = block_scaled_error(cov["joint"], ref, cd)
    print(f"dense {name} {schur}: error {err:.3g} (bound {CPU_BOUND:.3g}), "
          f"min pivot ratio {cov['min_pivot_ratio']:.3g}")
    assert err <= CPU_BOUND


@pytest.mark.parametrize("name,schur", CASES)
def test_dense_against_pcg(name, schur):
    cd = oracle(name)[0][0].shape[1]
    p = _problem(name, schur)
    dense = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")
    pcg = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="pcg",
                       tol=1e-10)
    err = block_scaled_error(dense["joint"], pcg["joint"], cd)
    print(f"dense against pcg {name} {schur}: {err:.3g}")
    assert err <= 2 * CPU_BOUND


def test_result_fields():
    p = _problem("bal", "implicit")
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")
    n = 9 * len(CAM_IDX) + 3 * len(PT_IDX)
    assert cov["method"] == "dense"
    assert cov["iters"].shape == (n,) and np.all(cov["iters"] == 0)
    assert cov["converged"].shape == (n,) and cov["converged"].all()
    assert cov["products"] == 0
    assert PIVOT_TOL < cov["min_pivot_ratio"] <= 1
    np.testing.assert_array_equal(cov["joint"], cov["joint"].T)
    for i in range(len(CAM_IDX)):
        np.testing.assert_array_equal(
            cov["cam_cov"][i], cov["joint"][9 * i:9 * i + 9, 9 * i:9 * i + 9])
    for i in range(len(PT_IDX)):
        s = 9 * len(CAM_IDX) + 3 * i
        np.testing.assert_array_equal(cov["pt_cov"][i],
                                      cov["joint"][s:s + 3, s:s + 3])
    pcg = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX)
    assert pcg["method"] == "pcg" and np.isnan(pcg["min_pivot_ratio"])


@pytest.mark.parametrize("method", ["pcg", "dense"])
def test_cross_false(method):
    p = _problem("bal", "implicit")
    full = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method=method)
    own = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method=method,
                       cross=False)
    assert own["joint"] is None
    assert own["cam_cov"].shape == (len(CAM_IDX), 9, 9)
    assert own["pt_cov"].shape == (len(PT_IDX), 3, 3)
    for key in ("cam_cov", "pt_cov"):
        for a, b in zip(own[key], full[key]):
            np.testing.assert_array_equal(a, a.T)
            rel = np.abs(a - b).max() / np.abs(b).max()
            print(f"cross=False {method} {key}: {rel:.3g}")
            assert rel <= 1e-12
    assert own["asymmetry"] >= 0.0
    assert own["converged"].all()


# ---- fixed vertices, no datum ----------------------------------------------
def _fixed_problem(device="cpu", schur="implicit"):
    args = bal_case()[0]
    cam_fixed = np.zeros(len(args[0]), dtype=np.uint8)
    cam_fixed[[0, 5]] = 1
    return mb.BAProblem(*args, cam_fixed=cam_fixed).build(device=device,
                                                          schur=schur)


def fixed_reference():
    """inv(H) rows of camera 2 and the two points with cameras 0 and 5 fixed
    (dense_hessian puts an identity on a fixed vertex)."""
    ref = _fixed_problem(schur="explicit")
    linearise(ref)
    H = dense_hessian(ref)
    rows = request_rows(9, 12, cam_idx=[2])
    return np.linalg.inv(H)[np.ix_(rows, rows)]


def check_fixed(p, bound):
    cov = p.covariance(cam_idx=[0, 5, 2], pt_idx=PT_IDX, method="dense")
    joint = cov["joint"]
    assert np.all(joint[:18, :] == 0.0) and np.all(joint[:, :18] == 0.0)
    assert cov["converged"].all()
    err = block_scaled_error(joint[18:, 18:], fixed_reference(), 9, n_cam=1)
    print(f"fixed cameras: error {err:.3g} (bound {bound:.3g})")
    assert err <= bound


def test_fixed_cameras():
    check_fixed(_fixed_problem(), CPU_BOUND)


def check_no_datum(p):
    with pytest.raises(RuntimeError, match="positive definite"):
        p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense",
                       strict=False)
    assert not cov["converged"].any()
    assert np.isnan(cov["joint"]).all()
    own = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense",
                       strict=False, cross=False)
    assert not own["converged"].any()
    assert np.isnan(own["cam_cov"]).all() and np.isnan(own["pt_cov"]).all()


def test_no_datum():
    check_no_datum(mb.BAProblem(*bal_case()[0]).build(device="cpu",
                                                      schur="implicit"))


# ---- a running LM session --------------------------------------------------
def lm_run_dense(call_after=None, device="cpu"):
    """covariance_common.lm_run with covariance(method="dense")."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14, cam_perturb=2e-2,
                             pt_perturb=0.1)
    p = with_priors(args, make_priors(args, schur="implicit"))
    p.build(device=device, schur="implicit")
    chis = [p.lm_init(tau=1e6, force_iterations=True, solver_tol=0.0,
                      solver_refuse_ratio=1e30, solver_max_iter=40)]
    acc, pcg, cov = [], [], None
    for k in range(6):
        log = p.lm_step()
        chis.append(log["chi2"])
        acc.append(bool(log["accepted"]))
        pcg.append(log["pcg_iters"])
        if call_after == k + 1:
            cov = p.covariance(cam_idx=[1, 20], pt_idx=[7, 399],
                               method="dense", strict=False)
    return np.array(chis), acc, pcg, cov


def test_lm_session_unchanged():
    plain, acc, pcg, _ = lm_run_dense()
    chis, acc2, pcg2, cov = lm_run_dense(call_after=2)
    assert cov is not None and cov["converged"].all()
    np.testing.assert_array_equal(chis, plain)
    assert acc2 == acc and pcg2 == pcg


# ---- default route, arguments ----------------------------------------------
def test_default_route_unchanged():
    p = _problem("bal", "implicit")
    a = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX)
    b = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="pcg")
    for key in ("joint", "cam_cov", "pt_cov", "iters", "converged"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["asymmetry"] == b["asymmetry"] and a["products"] == b["products"]


def test_bad_arguments():
    p = _problem("bal", "implicit")
    with pytest.raises(ValueError):
        p.covariance(cam_idx=CAM_IDX, method="x")
    q = with_priors(*bal_case()).build(device="cpu", dtype="float32")
    with pytest.raises(RuntimeError, match="float64"):
        q.covariance(cam_idx=CAM_IDX, method="dense")


# ---- hooks -----------------------------------------------------------------
def numpy_schur(build_kw=None):
    """S = B - E C^-1 E^T of the "bal" case from the explicit CPU dump."""
    ref = with_priors(*bal_case()).build(device="cpu", schur="explicit")
    linearise(ref)
    ref.process_diag(np.inf)
    H = dense_hessian(ref)
    nc = ref.cams.size
    return H[:nc, :nc] - H[:nc, nc:] @ np.linalg.solve(H[nc:, nc:], H[nc:, :nc])


@pytest.mark.parametrize("schur", ["explicit", "implicit"])
def test_dense_schur_hook(schur):
    S = numpy_schur()
    p = with_priors(*bal_case()).build(device="cpu", schur=schur)
    linearise(p)
    p.process_diag(np.inf)
    got = p.dense_schur()
    np.testing.assert_array_equal(got, got.T)
    err = np.abs(got - S).max() / np.abs(S).max()
    print(f"dense_schur {schur}: {err:.3g} (bound {PRODUCT_BOUND:.3g})")
    assert err <= PRODUCT_BOUND


def spd_matrix(n):
    G = np.random.default_rng(0).normal(size=(n, n + 8))
    return G @ G.T + n * np.eye(n)


def ldl_matrix(n, r, d):
    """L0 D L0^T with D = I except D[r] = d: row r is the failing pivot."""
    rng = np.random.default_rng(1)
    L0 = np.tril(0.1 * rng.normal(size=(n, n)), -1) + np.eye(n)
    D = np.ones(n)
    D[r] = d
    return (L0 * D) @ L0.T


CHOL_SIZES = [1, T - 1, T, T + 1, 2 * T + 2, 720]
# (failing row, D[r]) at n = 2T+2: first row, inside the second panel, last
# row.  The pivot-ratio input cannot fail in row 0, where the pivot is S_00
# itself and the ratio exactly 1: its first-panel case is row 3.
FAIL_CASES = [(0, -1.0), (T + 6, -1.0), (2 * T + 1, -1.0),
              (3, 1e-12), (T + 6, 1e-12), (2 * T + 1, 1e-12)]


def check_cholesky(p, n):
    A = spd_matrix(n)
    Lnp = np.linalg.cholesky(A)
    own = np.abs(Lnp @ Lnp.T - A).max() / np.abs(A).max()
    L, fail_row, ratio = p.dense_cholesky(A)
    err = np.abs(L @ L.T - A).max() / np.abs(A).max()
    print(f"dense_cholesky n={n}: {err:.3g}, numpy {own:.3g}, min pivot "
          f"ratio {ratio:.3g}")
    assert fail_row == -1
    assert err <= 10 * own
    assert np.all(np.triu(L, 1) == 0.0)
    assert 0 < ratio <= 1


def check_cholesky_failure(p, r, d):
    n = 2 * T + 2
    _, fail_row, _ = p.dense_cholesky(ldl_matrix(n, r, d))
    assert fail_row == r


@pytest.fixture(scope="module")
def cpu_engine():
    return with_priors(*bal_case()).build(device="cpu")


@pytest.mark.parametrize("n", CHOL_SIZES)
def test_dense_cholesky(cpu_engine, n):
    check_cholesky(cpu_engine, n)


@pytest.mark.parametrize("r,d", FAIL_CASES)
def test_dense_cholesky_failure(cpu_engine, r, d):
    check_cholesky_failure(cpu_engine, r, d)


# ---- two ranks over gloo ---------------------------------------------------
PORT = 29573


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from megba_amd.dist import gloo_allreduce_callback
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}",
                            rank=rank, world_size=world)
    try:
        params, _ = oracle("bal")
        p = make("bal", params=params, rank=rank, world_size=world,
                 allreduce=gloo_allreduce_callback())
        cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")
        np.save(f"{out}.joint{rank}.npy", cov["joint"])
        if rank == 0:
            with open(out, "w") as f:
                json.dump({"split": [int(s) for s in
                                     p.index_info()["pt_split"]]}, f)
    finally:
        dist.destroy_process_group()


def test_world2_dense(tmp_path):
    import torch.multiprocessing as mp
    params, ref = oracle("bal")
    one = make("bal", params=params).covariance(
        cam_idx=CAM_IDX, pt_idx=PT_IDX, method="dense")["joint"]
    out = str(tmp_path / "cov.json")
    mp.spawn(_worker, args=(2, PORT, out), nprocs=2, join=True)
    cut = json.loads(open(out).read())["split"][1]
    assert PT_IDX[0] < cut <= PT_IDX[1]  # one requested point per rank
    j0, j1 = (np.load(f"{out}.joint{r}.npy") for r in (0, 1))
    np.testing.assert_array_equal(j0, j1)
    e1, eo = block_scaled_error(j0, one, 9), block_scaled_error(j0, ref, 9)
    print("dense, world 2 against world 1:", e1, "against the oracle:", eo)
    assert e1 <= CPU_BOUND and eo <= CPU_BOUND
