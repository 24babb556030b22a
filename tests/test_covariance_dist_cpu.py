"""World-2 (gloo) covariance on the CPU engine: camera rows are replicated,
a point's rows come from the rank that owns it, and every rank ends with the
same joint matrix as an unsharded run."""
import json

import numpy as np

from covariance_common import (CAM_IDX, CPU_BOUND, PT_IDX, block_scaled_error,
                               make, oracle)

PORT = 29547


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from megba_amd.dist import gloo_allreduce_callback
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}",
                            rank=rank, world_size=world)
    try:
        params, _ = oracle("bal")
        p = make("bal", params=params, rank=rank, world_size=world,
                 allreduce=gloo_allreduce_callback())
        cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX)  # collective
        np.save(f"{out}.joint{rank}.npy", cov["joint"])
        if rank == 0:
            with open(out, "w") as f:
                json.dump({"split": [int(s) for s in
                                     p.index_info()["pt_split"]],
                           "iters": [int(i) for i in cov["iters"]]}, f)
    finally:
        dist.destroy_process_group()


def test_world2_covariance(tmp_path):
    import torch.multiprocessing as mp
    params, ref = oracle("bal")
    one = make("bal", params=params).covariance(cam_idx=CAM_IDX,
                                                pt_idx=PT_IDX)["joint"]
    out = str(tmp_path / "cov.json")
    mp.spawn(_worker, args=(2, PORT, out), nprocs=2, join=True)
    got = json.loads(open(out).read())
    cut = got["split"][1]
    assert PT_IDX[0] < cut <= PT_IDX[1]  # one requested point per rank
    j0, j1 = (np.load(f"{out}.joint{r}.npy") for r in (0, 1))
    np.testing.assert_array_equal(j0, j1)
    e1, eo = block_scaled_error(j0, one, 9), block_scaled_error(j0, ref, 9)
    print("world 2 against world 1:", e1, "against the oracle:", eo,
          "iters", got["iters"])
    assert e1 <= CPU_BOUND and eo <= CPU_BOUND
