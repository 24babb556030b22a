"""Which Schur product path the engine resolves for each combination of the
MEGBA_* path knobs, read back from its MEGBA_TUNE_VERBOSE line.  The problem
is far below the 200 k-edge auto-tune threshold, so every row is decided by
the knobs alone.  The line reports the tuner's choice, which is why the
MEGBA_FUSED row still says fused-etx.
"""
import numpy as np
import pytest

import megba_amd as mb

pytestmark = pytest.mark.gpu

NCAM = 6
LDS_NEED = NCAM * 9 * 8  # bytes of the fp64 camera vector

TABLE = [
    ({}, "fused-etx"),
    ({"MEGBA_SCHUR_LDS": "1"}, "lds"),
    ({"MEGBA_SCHUR_LDS": "1", "MEGBA_NO_SCHUR_LDS": "1"}, "fused-etx"),
    ({"MEGBA_NO_ETXFUSE": "1"}, "separate"),
    ({"MEGBA_ETXFUSE": "1"}, "fused-etx"),
    ({"MEGBA_NO_ETXFUSE": "1", "MEGBA_SCHUR_LDS": "1"}, "lds"),
    ({"MEGBA_ETXFUSE": "1", "MEGBA_SCHUR_LDS": "1"}, "lds"),
    ({"MEGBA_SCHUR_LDS": "1",
      "MEGBA_SCHUR_LDS_MAX_BYTES": str(LDS_NEED - 1)}, "fused-etx"),
    ({"MEGBA_FUSED": "1"}, "fused-etx"),
    ({"MEGBA_NO_PCG_FUSE": "1", "MEGBA_SCHUR_LDS": "1"}, "lds"),
    ({"MEGBA_SCHUR_RECOMPUTE": "1"}, "lds-recompute"),
    ({"MEGBA_SCHUR_RECOMPUTE": "1", "MEGBA_NO_SCHUR_RECOMPUTE": "1"},
     "fused-etx"),
    ({"MEGBA_SCHUR_RECOMPUTE": "1", "MEGBA_SCHUR_LDS": "1"}, "lds-recompute"),
    ({"MEGBA_SCHUR_RECOMPUTE": "1", "MEGBA_SCHUR_LDS": "1",
      "MEGBA_NO_SCHUR_RECOMPUTE": "1"}, "lds"),
    ({"MEGBA_SCHUR_RECOMPUTE": "1", "MEGBA_NO_SCHUR_LDS": "1"}, "fused-etx"),
]

PATH_KNOBS = ["MEGBA_SCHUR_LDS", "MEGBA_NO_SCHUR_LDS", "MEGBA_NO_ETXFUSE",
              "MEGBA_ETXFUSE", "MEGBA_SCHUR_LDS_MAX_BYTES", "MEGBA_FUSED",
              "MEGBA_NO_PCG_FUSE", "MEGBA_SCHUR_RECOMPUTE",
              "MEGBA_NO_SCHUR_RECOMPUTE", "MEGBA_TUNE_VERBOSE"]


@pytest.fixture(scope="module")
def problem():
    return mb.synthesize_bal(NCAM, 40, 240, seed=3)


@pytest.mark.parametrize("env,expected", TABLE,
                         ids=["+".join(k[6:] for k in e) or "default"
                              for e, _ in TABLE])
def test_schur_path(capfd, monkeypatch, problem, env, expected):
    for k in PATH_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MEGBA_TUNE_VERBOSE", "1")
    capfd.readouterr()
    p = mb.BAProblem(*problem)
    p.build(device="gpu", dtype="float64", schur="implicit")
    p.forward()
    p.accept_forward()
    p.build_linear_system()
    p.process_diag(1e4)
    n = p.solve_linear(max_iter=5, tol=0.0, refuse_ratio=1e30)
    dx = p.dump()["deltaX"]
    err = capfd.readouterr().err
    paths = [ln.split(":", 1)[1].strip() for ln in err.splitlines()
             if ln.startswith("# schur path:")]
    assert paths == [expected]
    assert n == 5 and np.isfinite(dx).all()
