#!/usr/bin/env python3
"""What a marginal covariance costs on the GPU.

Builds the bench's Venice-shaped synthetic problem (fp64, implicit Schur)
with a centre prior on every camera (the datum), takes a few LM steps, then
asks for the covariance of one camera and of one point (9 and 3 unit
right-hand side Schur PCG solves) at each --tol and each --batch (columns
solved together; 1 is the column loop).  Prints the PCG iterations of every
column, the Schur products applied (a batched application counts once), the
milliseconds per vertex block, per PCG iteration of a column and per product
(device synchronised before each clock read) and one JSON line.

--method dense takes the dense Cholesky route instead: it prints the
milliseconds of forming S and of factoring it with the achieved TF/s
(n^3 / 3 flops), the milliseconds per camera block and per point block of the
solves, min_pivot_ratio and the standard deviations; --tol and --batch do not
apply.  With MEGBA_DENSE_PROFILE=1 the share of the trailing-update kernel is
printed too (the kernels are then timed one by one, which slows the
factorization as a whole).  --all-cameras adds cross=False over every camera
and prints the total.  --formation times forming S with the dense kernels
against building it from ncam applications of the batched product on unit
columns (schur_apply(batched=True)).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import megba_amd as mb  # noqa: E402
from prior_overhead import centres  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="venice1778")
    ap.add_argument("--lm-steps", type=int, default=3)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--point", type=int, default=0)
    ap.add_argument("--tol", type=float, nargs="+",
                    default=[1e-10, 1e-8, 1e-6, 1e-4])
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--method", choices=["pcg", "dense"], default="pcg")
    ap.add_argument("--all-cameras", action="store_true")
    ap.add_argument("--formation", action="store_true")
    args = ap.parse_args()
    from bench import MODELS
    from megba_amd import _core
    shape = MODELS[args.model]
    cams, pts, ci, pi, meas = mb.synthesize_bal(shape["ncam"], shape["npt"],
                                                shape["nobs"], seed=7)
    rng = np.random.default_rng(1)
    p = mb.BAProblem(cams, pts, ci, pi, meas)
    p.set_camera_center_prior(
        np.arange(len(cams)),
        centres(cams) + rng.normal(0, 0.05, (len(cams), 3)),
        np.tile(mb.pack_sym(1e4 * np.eye(3)), (len(cams), 1)))
    p.build(device="gpu", dtype="float64", schur="implicit")
    p.lm_init(tau=1e4, solver_max_iter=100, solver_tol=0.0,
              solver_refuse_ratio=1e30, force_iterations=True, verbose=False)
    for _ in range(args.lm_steps):
        log = p.lm_step()
    print(f"{args.model}: {len(cams)} cams, {len(pts)} pts, {len(ci)} obs; "
          f"chi2 {log['chi2']:.6g} after {args.lm_steps} LM steps", flush=True)

    def timed(cam_idx, pt_idx, tol, batch, max_iter=args.max_iter):
        _core.device_synchronize()
        t0 = time.perf_counter()
        cov = p.covariance(cam_idx=cam_idx, pt_idx=pt_idx, tol=tol,
                           max_iter=max_iter, strict=False, batch=batch)
        _core.device_synchronize()
        return cov, (time.perf_counter() - t0) * 1000

    if args.method == "dense":
        dense_report(p, _core, args, len(cams))
        return

    # the first call pays the Schur path choice of the engine's first solve,
    # the first batched call the allocation of the batched buffers
    timed([args.camera], [args.point], args.tol[0], 1)
    for batch in args.batch:
        timed([args.camera], [args.point], args.tol[0], batch, max_iter=5)
    out = dict(model=args.model, max_iter=args.max_iter,
               max_batch=int(p.max_batch()), results=[])
    for tol in args.tol:
        print(f"tol {tol:g} (PCG stops on rho/rho_0 < {tol * tol:g}, or "
              f"after {args.max_iter} iterations)")
        for batch in args.batch:
            std = []
            for name, cams_, pts_ in (("camera", [args.camera], []),
                                      ("point", [], [args.point])):
                cov, ms = timed(cams_, pts_, tol, batch)
                its = [int(i) for i in cov["iters"]]
                products = int(cov["products"])
                print(f"  batch {batch} {name:6s} iters/column {its}  "
                      f"products {products}  converged "
                      f"{int(cov['converged'].sum())}/{len(its)}  asymmetry "
                      f"{cov['asymmetry']:.3g}")
                print(f"  {'':14s} {ms:9.1f} ms per block (relinearisation "
                      f"included), {ms / sum(its):6.3f} ms per PCG iteration "
                      f"of a column, {ms / products:6.3f} ms per product",
                      flush=True)
                std.append(np.sqrt(np.diag(cov["joint"])))
                out["results"].append(dict(
                    tol=tol, batch=batch, block=name, iters=its, ms=ms,
                    products=products,
                    converged=[bool(c) for c in cov["converged"]],
                    asymmetry=float(cov["asymmetry"])))
            print(f"  batch {batch} camera std (aa, t, f, k1, k2):",
                  np.array2string(std[0], precision=4))
            print(f"  batch {batch} point std:",
                  np.array2string(std[1], precision=4))
    print(json.dumps(out))


def dense_report(p, _core, args, ncam):
    cd = p.cams.shape[1]
    n = cd * ncam
    flops = n ** 3 / 3

    def timed(**kw):
        _core.device_synchronize()
        t0 = time.perf_counter()
        cov = p.covariance(method="dense", **kw)
        _core.device_synchronize()
        return cov, (time.perf_counter() - t0) * 1000

    # strict=True at the defaults: the call that raises on the PCG route
    timed(cam_idx=[args.camera], pt_idx=[args.point])  # allocations
    cov, ms = timed(cam_idx=[args.camera], pt_idx=[args.point])
    d = cov["dense_ms"]
    out = dict(model=args.model, method="dense", n=n, call_ms=ms,
               form_ms=d["form"], factor_ms=d["factor"],
               factor_tflops=flops / d["factor"] * 1e-9,
               min_pivot_ratio=float(cov["min_pivot_ratio"]))
    print(f"dense: n = {n}, S holds {8 * n * n / 1e9:.2f} GB; camera "
          f"{args.camera} and point {args.point} in {ms:.1f} ms "
          "(relinearisation included)")
    print(f"  formation {d['form']:.1f} ms, factorization {d['factor']:.1f} "
          f"ms = {out['factor_tflops']:.2f} TF/s, solves {d['solve']:.1f} ms, "
          f"min pivot ratio {cov['min_pivot_ratio']:.3g}")
    if d["trailing"] >= 0:
        out["trailing_ms"] = d["trailing"]
        print(f"  trailing update {d['trailing']:.1f} ms of the profiled "
              f"factorization = {flops / d['trailing'] * 1e-9:.2f} TF/s")
    for name, kw in (("camera", dict(cam_idx=[args.camera])),
                     ("point", dict(pt_idx=[args.point]))):
        c, _ = timed(**kw)
        out[name + "_block_ms"] = c["dense_ms"]["solve"]
        print(f"  {name} block {c['dense_ms']['solve']:.2f} ms; std",
              np.array2string(np.sqrt(np.diag(c["joint"])), precision=4))
    if args.all_cameras:
        c, ms = timed(cam_idx=list(range(ncam)), cross=False)
        out["all_cameras_ms"] = ms
        out["all_cameras_solve_ms"] = c["dense_ms"]["solve"]
        print(f"  all {ncam} cameras, cross=False: {ms:.1f} ms in all, "
              f"{c['dense_ms']['solve']:.1f} ms of it in the solves")
    if args.formation:
        p.forward()
        p.accept_forward()
        p.build_linear_system()
        p.process_diag(np.inf)
        X = np.zeros((n, cd))
        p.schur_apply(X, batched=True)  # allocations, path choice
        _core.device_synchronize()
        t0 = time.perf_counter()
        for c in range(ncam):
            X[:] = 0.0
            X[cd * c:cd * c + cd] = np.eye(cd)
            p.schur_apply(X, batched=True)
        _core.device_synchronize()
        out["products_ms"] = (time.perf_counter() - t0) * 1000
        print(f"  S from {ncam} batched products on unit columns: "
              f"{out['products_ms']:.1f} ms (host copies of the columns "
              f"included) against {d['form']:.1f} ms for the dense kernels")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
