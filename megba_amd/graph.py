"""g2o-style incremental graph-construction API.

The reference's user-facing surface is a vertex/edge graph built one
element at a time (BaseProblem::appendVertex / appendEdge,
/root/reference/include/problem/base_problem.h:22-83; vertex/edge classes
/root/reference/include/vertex/base_vertex.h:27-230 and
/root/reference/include/edge/base_edge.h:26-163; usage pattern
/root/reference/examples/BAL_Double.cpp:60-164).  This module provides the
same construction style on top of the array-based `BAProblem` core: append
vertices and edges, `solve()`, then read each vertex's `.estimation`
(the reference's writeBack semantics, base_problem.cpp:250-272).
"""
import numpy as np

from .problem import BAProblem, pack_sym

CAMERA = 0
POINT = 1


class BaseVertex:
    """A parameter block.  kind: CAMERA (9|6|4 params — the compiled
    camDim set; see BAProblem) or POINT (3)."""

    def __init__(self, estimation, kind, fixed=False):
        est = np.asarray(estimation, dtype=np.float64).reshape(-1)
        ok = est.size in (9, 6, 4) if kind == CAMERA else est.size == 3
        if not ok:
            raise ValueError(f"vertex kind {kind} needs "
                             f"{'9|6|4' if kind == CAMERA else '3'} params, "
                             f"got {est.size}")
        self.estimation = est.copy()
        self.kind = kind
        self.fixed = bool(fixed)
        self._slot = None  # assigned by GraphProblem.append_vertex


class CameraVertex(BaseVertex):
    def __init__(self, estimation, fixed=False):
        super().__init__(estimation, CAMERA, fixed)


class PointVertex(BaseVertex):
    def __init__(self, estimation, fixed=False):
        super().__init__(estimation, POINT, fixed)


class ReprojectionEdge:
    """One observation: connect exactly one CameraVertex and one
    PointVertex (the reference only implements the 1-camera-1-point edge
    kind, base_edge.cpp:27-36), with a 2-d measurement and an optional
    symmetric 2x2 information matrix given as (i00, i01, i11)."""

    def __init__(self, measurement, information=None):
        m = np.asarray(measurement, dtype=np.float64).reshape(-1)
        if m.size != 2:
            raise ValueError("measurement must be 2-d")
        self.measurement = m.copy()
        if information is not None:
            information = np.asarray(information, dtype=np.float64).reshape(-1)
            if information.size != 3:
                raise ValueError("information must be (i00, i01, i11)")
        self.information = information
        self.vertices = []

    def append_vertex(self, v):
        if not isinstance(v, BaseVertex):
            raise TypeError("append_vertex expects a BaseVertex")
        self.vertices.append(v)
        return self


class _PriorEdge:
    """A Gaussian unary prior: one vertex, a measurement of dimension D and
    an optional DxD information matrix, given full or packed-upper
    (D*(D+1)/2 values); None = identity.  At most one prior of a kind per
    vertex."""

    _kind = None  # vertex kind the edge attaches to

    def __init__(self, measurement, information=None):
        self.measurement = np.asarray(measurement,
                                      dtype=np.float64).reshape(-1).copy()
        d = self.measurement.size
        if information is not None:
            information = np.asarray(information, dtype=np.float64)
            if information.shape == (d, d):
                information = pack_sym(information)
            information = information.reshape(-1)
            if information.size != d * (d + 1) // 2:
                raise ValueError("information must be (D, D) or packed-upper "
                                 "D*(D+1)/2 values")
        self.information = information
        self.vertices = []

    def append_vertex(self, v):
        if not isinstance(v, BaseVertex):
            raise TypeError("append_vertex expects a BaseVertex")
        if v.kind != self._kind:
            raise ValueError(f"{type(self).__name__} attaches to a "
                             f"{'Camera' if self._kind == CAMERA else 'Point'}"
                             "Vertex")
        if self.vertices:
            raise ValueError("a prior edge has exactly one vertex")
        self.vertices.append(v)
        return self


class CameraPriorEdge(_PriorEdge):
    """r = camera parameters - measurement (camDim values)."""
    _kind = CAMERA


class PointPriorEdge(_PriorEdge):
    """r = point - measurement (ground control point)."""
    _kind = POINT


class CameraCenterPriorEdge(_PriorEdge):
    """r = C(camera) - measurement, C = -R(aa)^T t (GPS position); built-in
    BAL residuals only."""
    _kind = CAMERA

    def __init__(self, measurement, information=None):
        super().__init__(measurement, information)
        if self.measurement.size != 3:
            raise ValueError("camera centre measurement must be 3-d")


class GraphProblem:
    """g2o-style problem graph.  append_vertex / append_edge / solve;
    after solve() every vertex's .estimation holds the optimized value."""

    def __init__(self):
        self._cams = []
        self._pts = []
        self._edges = []
        # unary prior edges by BAProblem setter name
        self._priors = {"set_camera_prior": [], "set_point_prior": [],
                        "set_camera_center_prior": []}

    def append_vertex(self, v):
        if not isinstance(v, BaseVertex):
            raise TypeError("append_vertex expects a BaseVertex")
        if v._slot is not None:
            raise ValueError("vertex already appended")
        if v.kind == CAMERA:
            v._slot = len(self._cams)
            self._cams.append(v)
        else:
            v._slot = len(self._pts)
            self._pts.append(v)
        return self

    def append_edge(self, e):
        if isinstance(e, _PriorEdge):
            if len(e.vertices) != 1:
                raise ValueError("a prior edge needs its vertex")
            if e.vertices[0]._slot is None:
                self.append_vertex(e.vertices[0])
            setter = ("set_camera_center_prior"
                      if isinstance(e, CameraCenterPriorEdge)
                      else "set_camera_prior" if e._kind == CAMERA
                      else "set_point_prior")
            self._priors[setter].append(e)
            return self
        kinds = sorted(v.kind for v in e.vertices)
        if kinds != [CAMERA, POINT]:
            raise ValueError("edge must connect exactly one CameraVertex "
                             "and one PointVertex")
        for v in e.vertices:
            if v._slot is None:
                self.append_vertex(v)
        self._edges.append(e)
        return self

    @property
    def n_vertices(self):
        return len(self._cams) + len(self._pts)

    @property
    def n_edges(self):
        return len(self._edges)

    def _assemble(self):
        if not self._edges:
            raise ValueError("no edges")
        cams = np.stack([v.estimation for v in self._cams])
        pts = np.stack([v.estimation for v in self._pts])
        nobs = len(self._edges)
        ci = np.empty(nobs, dtype=np.int32)
        pi = np.empty(nobs, dtype=np.int32)
        meas = np.empty((nobs, 2))
        any_info = any(e.information is not None for e in self._edges)
        info = np.zeros((nobs, 3)) if any_info else None
        if any_info:
            info[:, 0] = 1.0
            info[:, 2] = 1.0  # identity default for unweighted edges
        for k, e in enumerate(self._edges):
            for v in e.vertices:
                if v.kind == CAMERA:
                    ci[k] = v._slot
                else:
                    pi[k] = v._slot
            meas[k] = e.measurement
            if any_info and e.information is not None:
                info[k] = e.information
        cam_fixed = np.array([v.fixed for v in self._cams], dtype=np.uint8)
        pt_fixed = np.array([v.fixed for v in self._pts], dtype=np.uint8)
        kw = {}
        if cam_fixed.any():
            kw["cam_fixed"] = cam_fixed
        if pt_fixed.any():
            kw["pt_fixed"] = pt_fixed
        prob = BAProblem(cams, pts, ci, pi, meas, info=info, **kw)
        for setter, edges in self._priors.items():
            if not edges:
                continue
            idx = np.array([e.vertices[0]._slot for e in edges],
                           dtype=np.int32)
            mean = np.stack([e.measurement for e in edges])
            pinfo = None
            if any(e.information is not None for e in edges):
                d = mean.shape[1]
                eye = pack_sym(np.eye(d))  # default for unweighted priors
                pinfo = np.stack([eye if e.information is None
                                  else e.information for e in edges])
            getattr(prob, setter)(idx, mean, pinfo)
        return prob

    def covariance(self, vertices, device="cpu", diff="auto",
                   schur="explicit", loss="none", loss_delta=1.0,
                   custom_forward=None, intrinsics=None, tol=1e-10,
                   max_iter=2000, strict=True, batch=1, method="pcg",
                   pivot_tol=None, cross=True):
        """Joint marginal covariance of `vertices` (appended CameraVertex /
        PointVertex objects, any order, each once) at their current
        estimations; rows and columns follow the order of `vertices`.  Like
        solve() it builds the problem anew and keeps no engine; see
        BAProblem.covariance for what the matrix is and what batch, method
        and pivot_tol do.  With cross=False there is no joint matrix: the
        result is the list of the vertices' own blocks, in their order."""
        cams, pts = [], []
        for v in vertices:
            if not isinstance(v, BaseVertex):
                raise TypeError("covariance expects BaseVertex objects")
            own = self._cams if v.kind == CAMERA else self._pts
            if v._slot is None or v._slot >= len(own) or own[v._slot] is not v:
                raise ValueError("megba: covariance of a vertex that is not "
                                 "in this problem")
            (cams if v.kind == CAMERA else pts).append(v._slot)
        p = self._assemble()
        p.build(device=device, diff=diff, schur=schur, loss=loss,
                loss_delta=loss_delta, custom_forward=custom_forward,
                intrinsics=intrinsics)
        cov = p.covariance(cams, pts, tol=tol, max_iter=max_iter,
                           strict=strict, batch=batch, method=method,
                           pivot_tol=pivot_tol, cross=cross)
        if not cross:
            own = {CAMERA: iter(cov["cam_cov"]), POINT: iter(cov["pt_cov"])}
            return [next(own[v.kind]) for v in vertices]
        joint = cov["joint"]
        # array order (cameras first) -> the order of `vertices`
        cd = p.cams.shape[1]
        at, nc, ic, ip = [], cd * len(cams), 0, 0
        for v in vertices:
            if v.kind == CAMERA:
                at += range(cd * ic, cd * (ic + 1))
                ic += 1
            else:
                at += range(nc + 3 * ip, nc + 3 * (ip + 1))
                ip += 1
        return joint[np.ix_(at, at)]

    def solve(self, device="cpu", dtype="float64", diff="auto",
              schur="explicit", loss="none", loss_delta=1.0,
              custom_forward=None, intrinsics=None, **solve_kw):
        """Build, run LM, and write the result back into the vertices.
        solve_kw: max_iter, tau, epsilon1, epsilon2, solver_tol,
        solver_max_iter, solver_refuse_ratio, verbose (see BAProblem.solve).
        custom_forward/intrinsics: as in BAProblem.build (user-defined
        residuals; fixed intrinsics for 6-dof cameras).
        """
        p = self._assemble()
        p.build(device=device, dtype=dtype, diff=diff, schur=schur,
                loss=loss, loss_delta=loss_delta,
                custom_forward=custom_forward, intrinsics=intrinsics)
        report = p.solve(**solve_kw)
        cams, pts = p.get_params()
        for v, row in zip(self._cams, cams):
            v.estimation[:] = row
        for v, row in zip(self._pts, pts):
            v.estimation[:] = row
        return report
