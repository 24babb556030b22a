"""World-2 (gloo) coverage of the unary priors: the replicated camera kinds
must be counted once (chi2 / rho on rank 0, H / g after the allreduce) and
point priors on the rank that owns the point, so the sharded trajectory
equals the unsharded one."""
import json

import numpy as np

import megba_amd as mb
from priors_common import make_priors, with_priors

SEED = 23
SHAPE = (10, 90, 760)


def _case():
    args = mb.synthesize_bal(*SHAPE, seed=SEED)
    return args, make_priors(args, n_cam=4, n_pt=30, n_ctr=4)


def _run(rank, world, allreduce=None):
    args, priors = _case()
    p = with_priors(args, priors)
    p.build(device="cpu", rank=rank, world_size=world, allreduce=allreduce)
    rep = p.solve(max_iter=5, tau=1e4, solver_tol=1e-6, solver_max_iter=150,
                  solver_refuse_ratio=1e6, verbose=False)
    c, q = p.get_params()
    return [it["chi2"] for it in rep["iters"]], c, p.index_info()["pt_split"]


def _worker(rank, world, port, out):
    import torch.distributed as dist
    from megba_amd.dist import gloo_allreduce_callback
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}",
                            rank=rank, world_size=world)
    try:
        chis, c, split = _run(rank, world, gloo_allreduce_callback())
        if rank == 0:
            np.save(out + ".cams.npy", c)
            with open(out, "w") as f:
                json.dump({"chis": chis, "split": [int(s) for s in split]}, f)
    finally:
        dist.destroy_process_group()


def test_world2_priors(tmp_path):
    import torch.multiprocessing as mp
    ref, c1, _ = _run(0, 1)
    out = str(tmp_path / "priors.json")
    mp.spawn(_worker, args=(2, 29541, out), nprocs=2, join=True)
    got = json.loads(open(out).read())
    # both ranks own some of the point priors
    idx = _case()[1]["pt"][0]
    cut = got["split"][1]
    assert (idx < cut).any() and (idx >= cut).any()
    np.testing.assert_allclose(got["chis"], ref, rtol=1e-6)
    c2 = np.load(out + ".cams.npy")
    np.testing.assert_allclose(c2, c1, rtol=1e-5, atol=1e-8)
