#!/usr/bin/env python3
"""What the unary priors cost per LM step on the GPU.

Runs the bench's Venice-shaped synthetic problem (fp64, implicit Schur,
fixed-work steps: 100 PCG iterations, early exits off) in three
configurations, in this order:

  none    no priors
  params  a point prior on every point and a parameter prior on every camera
  centre  a centre prior on every camera

and prints ms/step for each (device synchronised before each clock read) and
one JSON line.  --config runs a single configuration, e.g. under a profiler.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import megba_amd as mb  # noqa: E402

CONFIGS = ("none", "params", "centre")


def centres(cams):
    """C = -R(aa)^T t for every camera (vectorised Rodrigues)."""
    aa, t = cams[:, :3], cams[:, 3:6]
    th = np.linalg.norm(aa, axis=1, keepdims=True)
    w = aa / np.maximum(th, 1e-300)
    # R(-aa) t = t cos + (t x w) sin + w (w.t)(1 - cos)
    c, s = np.cos(th), np.sin(th)
    rt = t * c + np.cross(t, w) * s + w * np.sum(w * t, axis=1,
                                                  keepdims=True) * (1 - c)
    return -rt


def run(config, args, data):
    cams, pts, ci, pi, meas = data
    rng = np.random.default_rng(1)
    p = mb.BAProblem(cams, pts, ci, pi, meas)
    if config == "params":
        p.set_point_prior(
            np.arange(len(pts)), pts + rng.normal(0, 0.01, pts.shape),
            np.tile(mb.pack_sym(1e3 * np.eye(3)), (len(pts), 1)))
        p.set_camera_prior(
            np.arange(len(cams)), cams * (1 + 1e-4 * rng.normal(
                size=cams.shape)),
            np.tile(mb.pack_sym(np.eye(9)), (len(cams), 1)))
    elif config == "centre":
        p.set_camera_center_prior(
            np.arange(len(cams)),
            centres(cams) + rng.normal(0, 0.05, (len(cams), 3)),
            np.tile(mb.pack_sym(1e4 * np.eye(3)), (len(cams), 1)))
    p.build(device="gpu", dtype="float64", schur="implicit")
    p.lm_init(tau=1e4, epsilon1=1.0, epsilon2=1e-10, solver_max_iter=100,
              solver_tol=0.0, solver_refuse_ratio=1e30,
              force_iterations=True, verbose=False)
    from megba_amd import _core
    for _ in range(args.warmup):
        p.lm_step()
    _core.device_synchronize()
    accepted = 0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        accepted += bool(p.lm_step()["accepted"])
    _core.device_synchronize()
    ms = (time.perf_counter() - t0) * 1000 / args.steps
    print(f"{config:7s} {ms:8.3f} ms/step  ({accepted}/{args.steps} "
          "steps accepted)", flush=True)
    del p
    gc.collect()
    return dict(config=config, ms_per_step=ms, accepted=accepted)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="venice1778")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=CONFIGS, default=None)
    args = ap.parse_args()
    from bench import MODELS
    shape = MODELS[args.model]
    data = mb.synthesize_bal(shape["ncam"], shape["npt"], shape["nobs"],
                             seed=7)
    todo = (args.config,) if args.config else CONFIGS
    out = [run(c, args, data) for c in todo]
    print(json.dumps(dict(model=args.model, steps=args.steps, results=out)))


if __name__ == "__main__":
    main()
