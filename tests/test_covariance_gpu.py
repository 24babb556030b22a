"""Marginal covariances on the GPU engine: the unit right-hand side, the row
gather and the relative stop against the numpy inverse of the dense Hessian,
through every Schur path and PCG body, inside a running LM session, sharded
over two ranks on one device, and from the C++ example."""
import json

import numpy as np
import pytest

from covariance_common import (CAM_IDX, GPU_BOUND, PT_IDX, block_scaled_error,
                               check_against_oracle, lm_run, make, oracle,
                               run_cpp_covariance)
from priors_common import Env

pytestmark = pytest.mark.gpu


# ---- dense oracle ----------------------------------------------------------
@pytest.mark.parametrize("schur", ["implicit", "explicit"])
def test_oracle_bal(schur):
    params, _ = oracle("bal")
    check_against_oracle(make("bal", device="gpu", schur=schur, params=params),
                         "bal", GPU_BOUND)


def test_oracle_632():
    params, _ = oracle("632")
    check_against_oracle(make("632", device="gpu", params=params), "632",
                         GPU_BOUND)


# knob -> Schur path the engine must report.  The last two change the PCG
# body (no hipGraph capture; the seven-kernel body), not the product.
KNOBS = {
    "MEGBA_SCHUR_LDS": "lds",
    "MEGBA_SCHUR_RECOMPUTE": "lds-recompute",
    "MEGBA_NO_GRAPH": "fused-etx",
    "MEGBA_NO_PCG_FUSE": "fused-etx",
}


@pytest.mark.parametrize("knob", list(KNOBS))
def test_oracle_every_path(capfd, knob):
    params, _ = oracle("bal")
    capfd.readouterr()
    with Env({knob: "1"}):
        p = make("bal", device="gpu", schur="implicit", params=params)
        check_against_oracle(p, "bal", GPU_BOUND)
    err = capfd.readouterr().err
    ran = [ln.split(":", 1)[1].strip() for ln in err.splitlines()
           if ln.startswith("# schur path:")]
    assert ran == [KNOBS[knob]], (knob, ran)


# ---- state -----------------------------------------------------------------
# Largest relative difference between the chi2 lists of two plain GPU runs of
# the trajectory, measured on an MI355X: 2.0e-16, one unit in the last place
# (the runs with the call differed from a plain one by 1.3e-16).  The
# tolerance is 10x that spread.
STATE_SPREAD = 2.0e-16


def test_lm_state_preserved():
    plain, acc, pcg, _ = lm_run(device="gpu")
    again = lm_run(device="gpu")[0]
    spread = (np.abs(plain - again) / plain).max()
    print("accepted", acc, "relative spread of two plain runs", spread)
    assert acc[0] and not acc[1]
    for after in (1, 2):
        chis, acc2, _, cov = lm_run(call_after=after, device="gpu")
        diff = (np.abs(chis - plain) / plain).max()
        print("covariance() after step", after, "relative difference", diff,
              "iters", cov["iters"])
        assert cov["iters"].min() > 0
        assert acc2 == acc
        assert diff <= 10 * STATE_SPREAD


# ---- world 2 on one device -------------------------------------------------
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
        cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX)  # collective
        np.save(f"{out}.joint{rank}.npy", cov["joint"])
        if rank == 0:
            with open(out, "w") as f:
                json.dump([int(s) for s in p.index_info()["pt_split"]], f)
    finally:
        dist.destroy_process_group()


def test_world2_single_device(tmp_path):
    import torch.multiprocessing as mp
    params, ref = oracle("bal")
    out = str(tmp_path / "cov.json")
    mp.spawn(_w2_worker, args=(2, 29548, out), nprocs=2, join=True)
    cut = json.loads(open(out).read())[1]
    assert PT_IDX[0] < cut <= PT_IDX[1]  # one requested point per rank
    j0, j1 = (np.load(f"{out}.joint{r}.npy") for r in (0, 1))
    np.testing.assert_array_equal(j0, j1)
    err = block_scaled_error(j0, ref, 9)
    print("world 2 on one device against the oracle:", err)
    assert err <= GPU_BOUND


# ---- C++ example -----------------------------------------------------------
def test_cpp_covariance_example_gpu(tmp_path):
    run_cpp_covariance("gpu", tmp_path)
