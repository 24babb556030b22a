"""GPU test for the two-pass deterministic reductions (kRedPartial /
kRedFinal) behind the LM stopping criteria delta_x_l2(), x_l2() and g_inf().

Each is compared with numpy on the same engine's own vectors (dump() and
get_params()), so only the reduction is under test.  g_inf is a max of
absolute values: no rounding, and float -> double is exact, so it must be
equal.  The two norms are sums of n non-negative doubles taken in two
different orders (the squares themselves are the same doubles on both
sides); either order is within (n - 1) * 2**-53 of the exact sum, relatively,
so the two sums differ by less than n * 2**-52 and their square roots by half
of that.  The bound n * 2**-52 keeps a factor 2 of slack.
"""
import numpy as np
import pytest

import megba_amd as mb

pytestmark = pytest.mark.gpu

# 54 camera values: most threads and most of the 256 blocks are empty;
# 360 camera values: not a multiple of the 256-thread block.
PROBLEMS = {"cams6": (6, 40, 240, 3), "cams40": (40, 300, 2600, 5)}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_stopping_norms_match_numpy(name, dtype):
    ncam, npt, nobs, seed = PROBLEMS[name]
    p = mb.BAProblem(*mb.synthesize_bal(ncam, npt, nobs, seed=seed))
    p.build(device="gpu", dtype=dtype)
    p.forward()
    p.accept_forward()
    p.build_linear_system()
    p.process_diag(1e4)
    p.solve_linear(max_iter=30, tol=0.0, refuse_ratio=1e30)
    d = p.dump()
    dx, g = d["deltaX"], d["g"]
    cams, pts = p.get_params()
    x = np.concatenate([np.ravel(cams), np.ravel(pts)])
    n = ncam * 9 + npt * 3
    assert dx.size == n and g.size == n and x.size == n
    assert np.abs(dx).max() > 0 and np.abs(g).max() > 0

    g_inf = p.g_inf()
    print("g_inf gpu / numpy:", g_inf, np.abs(g).max())
    assert g_inf == np.abs(g).max()

    bound = n * 2.0 ** -52
    for label, got, v in (("delta_x_l2", p.delta_x_l2(), dx),
                          ("x_l2", p.x_l2(), x)):
        ref = np.sqrt(np.sum(v * v))
        dev = abs(got - ref) / ref
        print(label, "gpu / numpy / rel dev / bound:", got, ref, dev, bound)
        assert dev <= bound
