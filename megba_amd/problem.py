"""High-level problem API (g2o/MegBA-style) + BAL text IO.

Mirrors the reference's user surface (BaseProblem + BAL_* example flags,
/root/reference/examples/BAL_Double.cpp:50-58): the same knob names
(world_size, max_iter, solver_tol, solver_refuse_ratio, solver_max_iter,
tau, epsilon1, epsilon2) with the same semantics.
"""
import numpy as np


class BAProblem:
    """A BAL-family bundle adjustment problem.

    Block dims are inferred from the array shapes; the compiled set is
    camDim in {9, 6, 4}, ptDim = 3, resDim in {2, 3} (the reference takes
    these as runtime kernel arguments, build_linear_system.cu:48-146).

    cams: (ncam, 9) BAL [angle-axis(3), t(3), f, k1, k2]  -- or (ncam, 6)
          calibrated [angle-axis(3), t(3)] (pass intrinsics= to build()),
          or (ncam, 4) with a custom_forward.
    pts:  (npt, 3)
    cam_idx/pt_idx: (nobs,) int
    meas: (nobs, 2) image observations, or (nobs, 3) for 3D residuals
          (e.g. the built-in (6,3,3) SE3 point-alignment model)
    info: optional (nobs, resDim*(resDim+1)/2) packed-upper symmetric
          information (resDim=2: [w00, w01, w11])
    """

    def __init__(self, cams, pts, cam_idx, pt_idx, meas, info=None,
                 cam_fixed=None, pt_fixed=None):
        from . import _core
        self.cams = np.ascontiguousarray(cams, dtype=np.float64)
        self.pts = np.ascontiguousarray(pts, dtype=np.float64)
        self.cam_idx = np.ascontiguousarray(cam_idx, dtype=np.int32)
        self.pt_idx = np.ascontiguousarray(pt_idx, dtype=np.int32)
        self.meas = np.ascontiguousarray(meas, dtype=np.float64)
        self.info = None if info is None else np.ascontiguousarray(
            info, dtype=np.float64)
        cf = None if cam_fixed is None else np.ascontiguousarray(
            cam_fixed, dtype=np.uint8)
        pf = None if pt_fixed is None else np.ascontiguousarray(
            pt_fixed, dtype=np.uint8)
        self._core = _core.Problem(self.cams, self.pts, self.cam_idx,
                                   self.pt_idx, self.meas, self.info, cf, pf)
        self._built = False

    # -- Gaussian unary priors (soft constraints) ---------------------------
    def _set_prior(self, kind, idx, mean, info):
        if self._built:
            raise RuntimeError("megba: priors must be set before build()")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        if info is not None:
            info = np.ascontiguousarray(info, dtype=np.float64)
        self._core.set_prior(kind, idx, mean, info)
        return self

    def set_camera_prior(self, idx, mean, info=None):
        """Soft constraint r = cams[idx] - mean on whole camera blocks.
        idx: (m,) camera ids, each at most once; mean: (m, camDim);
        info: optional (m, camDim*(camDim+1)/2) packed-upper symmetric
        information matrices (see pack_sym), None = identity.  Adds
        r^T info r to chi^2; no robust loss.  Arrays are checked by build().
        """
        return self._set_prior(0, idx, mean, info)

    def set_point_prior(self, idx, mean, info=None):
        """Soft constraint r = pts[idx] - mean (ground control points).
        mean: (m, 3); info: optional (m, 6) packed-upper symmetric."""
        return self._set_prior(1, idx, mean, info)

    def set_camera_center_prior(self, idx, center, info=None):
        """Soft constraint r = C(cams[idx]) - center on the camera centre
        C = -R(aa)^T t (GPS positions).  Built-in BAL residuals only
        ((ncam, 9) or (ncam, 6) cameras, no custom_forward).
        center: (m, 3); info: optional (m, 6) packed-upper symmetric."""
        return self._set_prior(2, idx, center, info)

    # -- build -------------------------------------------------------------
    def build(self, device="cpu", dtype="float64", rank=0, world_size=1,
              device_index=0, diff="auto", schur="explicit", loss="none",
              loss_delta=1.0, allreduce=None, rccl_id=None,
              custom_forward=None, intrinsics=None):
        """loss: robust loss ("none" | "huber" | "cauchy") with scale
        loss_delta -- IRLS reweighting, rho-consistent cost (beyond the
        reference, which has only the 2x2 information matrix).
        custom_forward: optional callable (cam_jvs[camDim], pt_jvs[3],
        meas_jvs[resDim]) -> resDim JetVectors, evaluated per forward pass
        (runtime user-defined edges; see megba_amd.jv helpers).
        intrinsics: [f, k1, k2] for the (6,3,2) fixed-intrinsics built-in."""
        self._core.build(device=device, dtype=dtype, rank=rank,
                         world_size=world_size, device_index=device_index,
                         diff=diff, schur=schur, loss=loss,
                         loss_delta=loss_delta, allreduce=allreduce,
                         rccl_id=rccl_id, custom_forward=custom_forward,
                         intrinsics=intrinsics)
        self._built = True
        return self

    # -- solve -------------------------------------------------------------
    def solve(self, max_iter=20, tau=1e4, epsilon1=1.0, epsilon2=1e-10,
              solver_max_iter=100, solver_tol=1e-1, solver_refuse_ratio=1.0,
              force_iterations=False, verbose=True):
        assert self._built, "call build() first"
        return self._core.solve(
            max_iter=max_iter, tau=tau, epsilon1=epsilon1, epsilon2=epsilon2,
            solver_max_iter=solver_max_iter, solver_tol=solver_tol,
            solver_refuse_ratio=solver_refuse_ratio,
            force_iterations=force_iterations, verbose=verbose)

    # -- marginal covariances ------------------------------------------------
    def covariance(self, cam_idx=None, pt_idx=None, tol=1e-10, max_iter=2000,
                   strict=True, batch=1, method="pcg", pivot_tol=None,
                   cross=True):
        """Marginal covariance of the given cameras and points at the current
        parameters: the matching sub-matrix of H^-1, H = J^T W J plus the
        prior terms (the Hessian the LM step uses, robust-loss weights and
        information matrices included).  It is the covariance under
        unit-variance weighted residuals; multiply by a variance factor
        chi^2 / dof yourself if you want one.

        Call it after build(), usually after solve().  float64 only.  The
        gauge must be fixed by priors or fixed vertices, otherwise H is
        singular and the solves do not converge.  One unit-right-hand-side
        Schur PCG solve per row of every requested block (9 per BAL camera,
        3 per point); tol is the relative residual each solve reaches.
        Fixed vertices get zero rows and columns.

        Returns a dict: "joint" (n, n) with n = camDim*len(cam_idx) +
        3*len(pt_idx), cameras first in the order given; "cam_cov"
        (m, camDim, camDim) and "pt_cov" (k, 3, 3), its diagonal blocks;
        "iters" and "converged" per column; "asymmetry",
        max|A - A^T| / max|A| of the raw columns before symmetrising, a free
        accuracy indicator.  strict=True raises if a column did not
        converge, strict=False returns with the flags set.  "products" counts
        the Schur products S p the engine applied during the call.

        batch > 1 solves up to that many columns of one vertex block together
        where the engine has a batched product: the float64 GPU engine with
        schur="implicit", up to camDim columns (max_batch()).  The columns
        then share every pass over J and "products" counts a batched
        application once.  Every other engine (the CPU engine, explicit
        mode) accepts batch > 1 and solves column by column.  batch=1 is the
        column loop.

        method="dense" forms the camera system S = B - E C^-1 E^T as a dense
        matrix, factors it once with a Cholesky and solves every column
        exactly: no tol / max_iter to guess (tol, max_iter and batch are
        ignored), "iters" all 0, "converged" all True, "products" 0.  It
        costs 8 * (camDim * ncam)^2 bytes while the call runs; prefer it
        with few cameras, a tight tolerance or many requested vertices.  A
        pivot below pivot_tol * S_ii (default sqrt(eps) ~ 1.5e-8) fails the
        factorization: strict=True raises "not positive definite",
        strict=False returns "converged" all False and NaN entries.  Unlike
        the PCG, which without a datum still converges on the intrinsics
        columns, the dense route then reports the whole system singular.
        "min_pivot_ratio" is the smallest L_ii^2 / S_ii (NaN for "pcg"),
        "method" the route taken.

        cross=False solves every block against its own rows only: "joint"
        is None, "cam_cov" / "pt_cov" are filled from the per-block solves
        and "asymmetry" is taken over the blocks.  Use it for the covariance
        of many vertices, where "joint" itself would be large.

        COLLECTIVE when world_size>1: every rank calls it with the same
        arguments and gets the same result.  An LM session in progress
        (lm_init / lm_step) continues unchanged afterwards."""
        if not self._built:
            raise RuntimeError("megba: call build() first")
        if method not in ("pcg", "dense"):
            raise ValueError("megba: covariance method must be 'pcg' or "
                             f"'dense', not {method!r}")
        cams = [] if cam_idx is None else [int(i) for i in cam_idx]
        pts = [] if pt_idx is None else [int(i) for i in pt_idx]
        out = self._core.covariance(cams, pts, tol=tol, max_iter=max_iter,
                                    strict=strict, batch=int(batch),
                                    method=method, pivot_tol=pivot_tol,
                                    cross=bool(cross))
        joint = out["joint"]
        cd = self.cams.shape[1]
        nc = cd * len(cams)
        if joint is None:
            blocks = out.pop("blocks")
            out["cam_cov"] = blocks[:cd * cd * len(cams)].reshape(
                len(cams), cd, cd).copy()
            out["pt_cov"] = blocks[cd * cd * len(cams):].reshape(
                len(pts), 3, 3).copy()
            return out
        out["cam_cov"] = np.array(
            [joint[cd * i:cd * (i + 1), cd * i:cd * (i + 1)]
             for i in range(len(cams))]).reshape(len(cams), cd, cd)
        out["pt_cov"] = np.array(
            [joint[nc + 3 * i:nc + 3 * (i + 1), nc + 3 * i:nc + 3 * (i + 1)]
             for i in range(len(pts))]).reshape(len(pts), 3, 3)
        return out

    # -- low-level steps (tests) -------------------------------------------
    def __getattr__(self, name):
        # Delegate fine-grained methods to the core object.
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._core, name)

    def params(self):
        """Solved parameters (cams, pts).  COLLECTIVE when world_size>1:
        every rank must call it (the point shards are merged with an
        allreduce)."""
        return self._core.get_params()


def pack_sym(M):
    """Pack full symmetric matrices (..., D, D) into the packed-upper
    row-major form (..., D*(D+1)/2) the `info` arguments take
    (D=2: [m00, m01, m11])."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim < 2 or M.shape[-1] != M.shape[-2]:
        raise ValueError("pack_sym expects (..., D, D)")
    iu = np.triu_indices(M.shape[-1])
    return np.ascontiguousarray(M[..., iu[0], iu[1]])


def load_bal(path):
    """Parse a BAL 'problem-*.txt' file (same format the reference examples
    read, /root/reference/examples/BAL_Double.cpp:74-139)."""
    with open(path) as f:
        header = f.readline().split()
        ncam, npt, nobs = int(header[0]), int(header[1]), int(header[2])
        text = f.read()
    try:
        body = np.fromstring(text, sep=" ")
    except Exception:  # numpy versions without text-mode fromstring
        body = np.array(text.split(), dtype=np.float64)
    obs = body[:nobs * 4].reshape(nobs, 4)
    cam_idx = obs[:, 0].astype(np.int32)
    pt_idx = obs[:, 1].astype(np.int32)
    meas = obs[:, 2:4].copy()
    rest = body[nobs * 4:]
    cams = rest[:ncam * 9].reshape(ncam, 9).copy()
    pts = rest[ncam * 9: ncam * 9 + npt * 3].reshape(npt, 3).copy()
    return cams, pts, cam_idx, pt_idx, meas


def save_bal(path, cams, pts, cam_idx, pt_idx, meas):
    ncam, npt, nobs = len(cams), len(pts), len(cam_idx)
    with open(path, "w") as f:
        f.write(f"{ncam} {npt} {nobs}\n")
        for i in range(nobs):
            f.write(f"{cam_idx[i]} {pt_idx[i]} {meas[i,0]:.17g} {meas[i,1]:.17g}\n")
        for row in np.asarray(cams).reshape(-1):
            f.write(f"{row:.17g}\n")
        for row in np.asarray(pts).reshape(-1):
            f.write(f"{row:.17g}\n")
