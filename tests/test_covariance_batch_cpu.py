"""covariance(batch=...) on the CPU engine.  The CPU engine has no batched
product (max_batch() == 1), so batch > 1 is accepted and runs the same
column loop: bit-equal results.  `products` counts the applications of the
Schur product S p: each solved column applies it once for its initial
residual and once per PCG iteration."""
import numpy as np
import pytest

import megba_amd as mb
from covariance_common import CAM_IDX, PT_IDX, make, oracle
from priors_common import bal_case


def test_batch_equals_column_loop():
    params, _ = oracle("bal")
    p = make("bal", schur="implicit", params=params)
    assert p.max_batch() == 1
    one = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=1)
    nine = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=9)
    np.testing.assert_array_equal(one["joint"], nine["joint"])
    np.testing.assert_array_equal(one["iters"], nine["iters"])
    np.testing.assert_array_equal(one["converged"], nine["converged"])
    assert one["iters"].min() > 0  # every column was solved
    for cov in (one, nine):
        # initial residual + one per iteration, for every solved column
        assert cov["products"] == int((cov["iters"] + 1).sum())


def test_products_skip_fixed_vertices():
    """A fixed vertex is not solved and applies no product."""
    params, _ = oracle("bal")
    fixed = np.zeros(len(params[0]), dtype=np.uint8)
    fixed[CAM_IDX[0]] = 1
    args = bal_case()[0]
    p = mb.BAProblem(params[0], params[1], *args[2:], cam_fixed=fixed)
    p.build(device="cpu")
    cov = p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=3, strict=False,
                       max_iter=300)
    solved = cov["iters"] > 0
    assert not solved[:9].any() and solved[9:].all()
    assert cov["products"] == int((cov["iters"][solved] + 1).sum())


@pytest.mark.parametrize("batch", [0, -3])
def test_batch_below_one_raises(batch):
    params, _ = oracle("bal")
    p = make("bal", params=params)
    with pytest.raises(RuntimeError, match=r"megba:.*batch"):
        p.covariance(cam_idx=CAM_IDX, pt_idx=PT_IDX, batch=batch)
