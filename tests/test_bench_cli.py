"""bench.py command line: --dump-outputs and --full (CPU engine, tiny shape)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _run(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--model", "tiny",
         "--device", "cpu", "--gpus", "1", "--steps", "2", "--warmup", "1",
         *extra],
        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_reproducible(tmp_path):
    """Same arguments -> same inputs -> the same dumped arrays; the dump is
    what params() returns after the last timed step."""
    import megba_amd as mb
    import bench
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run("--dump-outputs", str(a))
    _run("--dump-outputs", str(b), "--full")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1000.0) < 1e-6 * 1000.0
    shape = bench.MODELS["tiny"]
    assert sorted(os.listdir(a)) == ["cams.npy", "chi2.npy", "pts.npy"]
    total = 0
    for name, shp in (("cams", (shape["ncam"], 9)), ("pts", (shape["npt"], 3)),
                      ("chi2", (1,))):
        x, y = np.load(a / f"{name}.npy"), np.load(b / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == shp
        assert np.isfinite(x).all()
        # CPU engine, one rank: fixed summation order, so bit-identical
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    assert float(np.load(a / "chi2.npy")[0]) == d["config"]["final_chi2"]

    # independent replay of the same 3 LM steps through the Python API
    cams, pts, ci, pi, meas = mb.synthesize_bal(
        shape["ncam"], shape["npt"], shape["nobs"], seed=7)
    p = mb.BAProblem(cams, pts, ci, pi, meas)
    p.build(device="cpu", dtype="float64", schur="implicit")
    p.lm_init(tau=1e4, epsilon1=1.0, epsilon2=1e-10, solver_max_iter=100,
              solver_tol=0.0, solver_refuse_ratio=1e30, force_iterations=True)
    for _ in range(3):
        p.lm_step()
    c_ref, p_ref = p.params()
    np.testing.assert_array_equal(np.load(a / "cams.npy"), c_ref)
    np.testing.assert_array_equal(np.load(a / "pts.npy"), p_ref)
    # the steps moved the parameters: the dump is not the input
    assert not np.array_equal(p_ref, pts)


def test_dump_sampling_is_fixed_and_bounded(tmp_path):
    """An output over the byte budget is cut to a fixed seeded row sample."""
    import bench

    class FakeProblem:
        def params(self):
            rng = np.random.default_rng(0)
            return rng.normal(size=(5, 9)), rng.normal(size=(1000, 3))

    old = bench.DUMP_MAX_BYTES
    bench.DUMP_MAX_BYTES = 2 * 100 * 24   # 100 point rows fit
    try:
        for sub in ("a", "b"):
            bench.dump_outputs(str(tmp_path / sub), FakeProblem(),
                               {"chi2": 1.5}, rank=0)
    finally:
        bench.DUMP_MAX_BYTES = old
    rows = np.load(tmp_path / "a" / "pts_rows.npy")
    pts = np.load(tmp_path / "a" / "pts.npy")
    assert pts.shape == (100, 3) and rows.shape == (100,)
    assert (np.diff(rows) > 0).all() and rows.max() < 1000
    full = FakeProblem().params()[1]
    np.testing.assert_array_equal(pts, full[rows.astype(np.int64)])
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "pts_rows.npy"))
    assert np.load(tmp_path / "a" / "cams.npy").shape == (5, 9)
    assert not (tmp_path / "a" / "cams_rows.npy").exists()
