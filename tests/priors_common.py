"""Shared pieces of the unary-prior tests: a numpy camera centre, prior sets
scaled against the unprior'd Hessian blocks, and problem builders."""
import functools
import os
import subprocess

import numpy as np

import megba_amd as mb

SHAPE = (12, 120, 1100)
SEED = 3
INTR = [420.0, -1e-7, 3e-13]


def rodrigues(aa):
    th = np.linalg.norm(aa)
    K = np.array([[0, -aa[2], aa[1]], [aa[2], 0, -aa[0]],
                  [-aa[1], aa[0], 0]])
    if th < 1e-7:
        return np.eye(3) + K
    K = K / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def centre_np(cam):
    """C = -R(aa)^T t (independent of the engine's Rodrigues code)."""
    return -rodrigues(np.asarray(cam[:3])).T @ np.asarray(cam[3:6])


def centres_np(cams):
    return np.array([centre_np(c) for c in cams])


def rand_spd(rng, d):
    """Random SPD matrix with unit mean diagonal."""
    a = rng.normal(size=(d, d))
    m = a @ a.T + d * np.eye(d)
    return m / np.mean(np.diag(m))


def problem_632():
    """(6,3,2) arguments with measurements consistent with INTR."""
    cams9, pts, ci, pi, meas0 = mb.synthesize_bal(*SHAPE, seed=SEED)
    cams9[:, 6:9] = INTR
    p = mb.BAProblem(cams9, pts, ci, pi, np.zeros_like(meas0))
    p.build(device="cpu")
    p.forward()
    r_sorted = p.dump()["r"].reshape(-1, 2)
    r = np.empty_like(r_sorted)
    r[p.index_info()["perm"]] = r_sorted
    meas = r + np.random.default_rng(112).normal(0, 0.5, r.shape)
    return cams9[:, :6].copy(), pts, ci, pi, meas


def assembled(args, **build_kw):
    """CPU problem after forward/accept/build_linear_system."""
    p = mb.BAProblem(*args)
    p.build(device="cpu", **build_kw)
    p.chi0 = p.forward()
    p.accept_forward()
    p.build_linear_system()
    return p


def make_priors(args, n_cam=5, n_pt=40, n_ctr=5, seed=7, ctr_offset=None,
                **build_kw):
    """Prior sets for a problem: {"cam"|"pt"|"ctr": (idx, mean, L)} with L
    the full (m, D, D) information matrices.  Each L is a random SPD matrix
    scaled to 0.1 x the mean diagonal of that vertex's unprior'd Hessian
    block (for the centre kind: of the block's translation part, whose J is
    a rotation), so the prior is neither negligible nor dominant.  The means
    sit a little away from the current estimate so that r != 0; with
    ctr_offset the centre means sit exactly that far away instead, in a
    random direction."""
    cams, pts = args[0], args[1]
    ncam, cd = cams.shape
    npt = len(pts)
    rng = np.random.default_rng(seed)
    d = assembled(args, **build_kw).dump()
    hpp = d["Hpp"].reshape(ncam, cd, cd)
    hll = d["Hll"].reshape(npt, 3, 3)
    out = {}
    if n_cam:
        idx = np.sort(rng.choice(ncam, n_cam, replace=False)).astype(np.int32)
        L = np.array([0.1 * np.mean(np.diag(hpp[c])) * rand_spd(rng, cd)
                      for c in idx])
        mean = cams[idx] * (1 + 1e-3 * rng.normal(size=(n_cam, cd)))
        out["cam"] = (idx, mean, L)
    if n_pt:
        idx = np.sort(rng.choice(npt, n_pt, replace=False)).astype(np.int32)
        L = np.array([0.1 * np.mean(np.diag(hll[q])) * rand_spd(rng, 3)
                      for q in idx])
        mean = pts[idx] + 0.02 * rng.normal(size=(n_pt, 3))
        out["pt"] = (idx, mean, L)
    if n_ctr:
        idx = np.sort(rng.choice(ncam, n_ctr, replace=False)).astype(np.int32)
        L = np.array([0.1 * np.mean(np.diag(hpp[c])[3:6]) * rand_spd(rng, 3)
                      for c in idx])
        off = rng.normal(size=(n_ctr, 3))
        if ctr_offset is None:
            off *= 0.05
        else:
            off *= ctr_offset / np.linalg.norm(off, axis=1, keepdims=True)
        mean = centres_np(cams[idx]) + off
        out["ctr"] = (idx, mean, L)
    return out


def with_priors(args, priors, **problem_kw):
    """Unbuilt BAProblem carrying the given prior sets."""
    p = mb.BAProblem(*args, **problem_kw)
    if "cam" in priors:
        i, m, L = priors["cam"]
        p.set_camera_prior(i, m, mb.pack_sym(L))
    if "pt" in priors:
        i, m, L = priors["pt"]
        p.set_point_prior(i, m, mb.pack_sym(L))
    if "ctr" in priors:
        i, m, L = priors["ctr"]
        p.set_camera_center_prior(i, m, mb.pack_sym(L))
    return p


@functools.lru_cache(maxsize=None)
def bal_case():
    """The (12,120,1100) BAL problem with all three prior kinds."""
    args = mb.synthesize_bal(*SHAPE, seed=SEED)
    return args, make_priors(args)


@functools.lru_cache(maxsize=None)
def case_632():
    args = problem_632()
    return args, make_priors(args, intrinsics=INTR)


class Env:
    """Set MEGBA_* knobs for the engines built inside the block (they are
    read at construction); MEGBA_TUNE_VERBOSE makes the engine report the
    Schur path it resolved."""

    def __init__(self, env):
        self.env = dict(env)
        self.env.setdefault("MEGBA_TUNE_VERBOSE", "1")

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_cpp_priors(device, tmp_path):
    """The native C++ prior example is self-verifying: graph API against the
    array API, and centre priors pulling a shifted scene back."""
    binpath = "examples/bal_priors_cpp"
    assert os.path.exists(binpath), "native example not built"
    cams, pts, ci, pi, meas = mb.synthesize_bal(10, 80, 700, seed=2)
    f = tmp_path / "prob.txt"
    mb.save_bal(f, cams, pts, ci, pi, meas)
    r = subprocess.run([binpath, "--path", str(f), "--device", device],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    assert "PRIORS_OK" in r.stdout
