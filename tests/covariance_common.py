"""Shared pieces of the covariance tests: the dense numpy oracle, the cases
and the error bounds."""
import functools
import os
import subprocess

import numpy as np

import megba_amd as mb
from priors_common import (INTR, bal_case, case_632, make_priors,
                           with_priors)

CAM_IDX = [0, 7]
PT_IDX = [3, 100]

# Largest error of the CPU engine's joint matrix against the dense oracle at
# tol=1e-10, each vertex-block pair relative to max|oracle block|
# (block_scaled_error), measured over the three oracle cases of
# test_covariance_cpu.py: 5.38e-11 ((9,3,2) explicit), 5.37e-11 ((9,3,2)
# implicit) and 1.02e-11 ((6,3,2)).  The CPU bound is 10x the largest, the
# GPU bound 100x (the GPU sums in a different order).  Relative to the
# largest entry of the whole oracle matrix the same runs are at 1.8e-13.
CPU_MEASURED = 5.4e-11
CPU_BOUND = 10 * CPU_MEASURED
GPU_BOUND = 100 * CPU_MEASURED


def dense_hessian(p):
    """H of an explicit-mode world-1 engine from dump(): Hpp and Hll blocks
    on the diagonal, edge e's Hpl block between its camera and its point
    (dump() and index_info() share the sorted edge order; perm maps it back
    to the caller's).  A fixed vertex has all-zero blocks: identity there."""
    d, ix = p.dump(), p.index_info()
    ncam, npt = int(ix["ncam"]), int(ix["npt"])
    cd = int(round(np.sqrt(d["Hpp"].size / ncam)))
    nc = cd * ncam
    H = np.zeros((nc + 3 * npt, nc + 3 * npt))
    hpp = d["Hpp"].reshape(ncam, cd, cd)
    hll = d["Hll"].reshape(npt, 3, 3)
    for c in range(ncam):
        H[cd * c:cd * c + cd, cd * c:cd * c + cd] = (
            hpp[c] if np.any(hpp[c]) else np.eye(cd))
    for q in range(npt):
        s = nc + 3 * q
        H[s:s + 3, s:s + 3] = hll[q] if np.any(hll[q]) else np.eye(3)
    hpl = d["Hpl"].reshape(-1, cd, 3)
    assert len(hpl) == len(ix["perm"]) == len(ix["cam_of"])
    for e, (c, q) in enumerate(zip(ix["cam_of"], ix["pt_of"])):
        s = nc + 3 * q
        H[cd * c:cd * c + cd, s:s + 3] += hpl[e]
        H[s:s + 3, cd * c:cd * c + cd] += hpl[e].T
    return H


def request_rows(cd, ncam, cam_idx=CAM_IDX, pt_idx=PT_IDX):
    rows = [cd * c + i for c in cam_idx for i in range(cd)]
    rows += [cd * ncam + 3 * q + i for q in pt_idx for i in range(3)]
    return np.array(rows)


def linearise(p):
    p.forward()
    p.accept_forward()
    p.build_linear_system()


def make(name, device="cpu", schur="explicit", params=None, **build_kw):
    """Built problem of case `name`, at the given (cams, pts) or at the
    case's start."""
    if name == "bal":
        args, priors = bal_case()
    else:
        args, priors = case_632()
        build_kw["intrinsics"] = INTR
    if params is not None:
        args = (params[0], params[1]) + tuple(args[2:])
    p = with_priors(args, priors)
    p.build(device=device, schur=schur, **build_kw)
    return p


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(solved params, oracle sub-matrix) of a case: solve(max_iter=30) on the
    CPU, then the numpy inverse of the dense H at the solution.  Computed
    once; every engine under test starts from these parameters."""
    p = make(name)
    p.solve(max_iter=30, verbose=False)
    params = p.get_params()
    q = make(name, params=params)
    linearise(q)
    H = dense_hessian(q)
    w = np.linalg.eigvalsh(H)
    assert w[0] > 0, "oracle H is not positive definite"
    cd = params[0].shape[1]
    rows = request_rows(cd, len(params[0]))
    sub = np.linalg.inv(H)[np.ix_(rows, rows)]
    for a in (params[0], params[1], sub):
        a.setflags(write=False)
    return params, sub


def block_scaled_error(joint, ref, cd, n_cam=len(CAM_IDX)):
    """max over the vertex-block pairs of max|joint - ref| / max|ref block|:
    camera, point and cross blocks differ by orders of magnitude."""
    cuts = [cd * i for i in range(n_cam + 1)]
    cuts += list(range(cuts[-1] + 3, len(ref) + 1, 3))
    worst = 0.0
    for a0, a1 in zip(cuts[:-1], cuts[1:]):
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            blk = ref[a0:a1, b0:b1]
            err = np.abs(joint[a0:a1, b0:b1] - blk).max()
            worst = max(worst, err / np.abs(blk).max())
    return worst


def check_against_oracle(p, name, bound):
    """covariance() of the standard request on p against the oracle."""
    params, ref = oracle(name)
    cd = params[0].shape[1]
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, tol=1e-10)
    n = cd * len(CAM_IDX) + 3 * len(PT_IDX)
    assert cov["joint"].shape == (n, n)
    assert cov["converged"].all()
    err = block_scaled_error(cov["joint"], ref, cd)
    print(f"{name}: error {err:.3g} (bound {bound:.3g}), iters "
          f"{cov['iters'].min()}..{cov['iters'].max()}, asymmetry "
          f"{cov['asymmetry']:.3g}")
    assert err <= bound
    np.testing.assert_array_equal(cov["joint"], cov["joint"].T)
    assert cov["cam_cov"].shape == (len(CAM_IDX), cd, cd)
    assert cov["pt_cov"].shape == (len(PT_IDX), 3, 3)
    for i in range(len(CAM_IDX)):
        np.testing.assert_array_equal(
            cov["cam_cov"][i],
            cov["joint"][cd * i:cd * i + cd, cd * i:cd * i + cd])
    for i in range(len(PT_IDX)):
        s = cd * len(CAM_IDX) + 3 * i
        np.testing.assert_array_equal(cov["pt_cov"][i],
                                      cov["joint"][s:s + 3, s:s + 3])
    return cov


def lm_run(call_after=None, device="cpu"):
    """The six-step "tau1e6" trajectory of test_priors_gpu.py (accept, three
    rejects, two accepts); optionally covariance() after step `call_after`."""
    args = mb.synthesize_bal(24, 400, 3600, seed=14, cam_perturb=2e-2,
                             pt_perturb=0.1)
    priors = make_priors(args, schur="implicit")
    p = with_priors(args, priors)
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
                               strict=False)
    return np.array(chis), acc, pcg, cov


def run_cpp_covariance(device, tmp_path):
    """The native C++ covariance example is self-verifying."""
    binpath = "examples/bal_covariance_cpp"
    assert os.path.exists(binpath), "native example not built"
    cams, pts, ci, pi, meas = mb.synthesize_bal(10, 80, 700, seed=2)
    f = tmp_path / "prob.txt"
    mb.save_bal(f, cams, pts, ci, pi, meas)
    r = subprocess.run([binpath, "--path", str(f), "--device", device],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    assert "COVARIANCE_OK" in r.stdout
