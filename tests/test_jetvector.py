"""JetVector op layer: values/gradients vs a numpy dual-number oracle,
JPV and scalar operand kinds, geometry ops (CPU backend here; the GPU
backend is the same kernels compiled for gfx950, tested under -m gpu)."""
import numpy as np
import pytest

from megba_amd import _core


N = 4
NI = 257
rng = np.random.default_rng(0)


class Ref:
    """numpy forward-mode dual numbers, grad shape (N, nItem)."""

    def __init__(self, v, g=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.g = np.zeros((N, len(self.v))) if g is None else g

    @staticmethod
    def leaf(v, pos):
        r = Ref(v)
        r.g[pos] = 1.0
        return r

    def __add__(self, o):
        return Ref(self.v + o.v, self.g + o.g)

    def __sub__(self, o):
        return Ref(self.v - o.v, self.g - o.g)

    def __mul__(self, o):
        return Ref(self.v * o.v, self.g * o.v + self.v * o.g)

    def __truediv__(self, o):
        q = self.v / o.v
        return Ref(q, (self.g - q * o.g) / o.v)


def dense(gpu=False):
    v = rng.normal(size=NI) + 3.0
    g = rng.normal(size=(N, NI))
    return _core.JetVector(v, g, N=N, gpu=gpu), Ref(v, g.copy())


def jpv(pos, gpu=False):
    v = rng.normal(size=NI) + 3.0
    jv = _core.JetVector(v, None, N=N, grad_pos=pos, gpu=gpu)
    return jv, Ref.leaf(v, pos)


def check(jv, ref, rtol=1e-12):
    v, g = jv.to_numpy()
    np.testing.assert_allclose(v, ref.v, rtol=rtol, atol=1e-13)
    np.testing.assert_allclose(g, ref.g, rtol=rtol, atol=1e-13)


OPS = [( _core.jv_add, lambda a, b: a + b),
       (_core.jv_sub, lambda a, b: a - b),
       (_core.jv_mul, lambda a, b: a * b),
       (_core.jv_div, lambda a, b: a / b)]


def run_binary_suite(gpu):
    for op, ref_op in OPS:
        a, ra = dense(gpu)
        b, rb = dense(gpu)
        check(op(a, b), ref_op(ra, rb))
        # JPV operands
        c, rc = jpv(1, gpu)
        check(op(a, c), ref_op(ra, rc))
        check(op(c, b), ref_op(rc, rb))
        d, rd = jpv(3, gpu)
        check(op(c, d), ref_op(rc, rd))
        # scalar operands
        s = _core.jv_scalar(1.75, N)
        rs = Ref(np.full(NI, 1.75))
        check(op(a, s), ref_op(ra, rs))
        check(op(s, b), ref_op(rs, rb))
        # scalar x JPV and scalar x scalar (completes the reference's
        # 39-variant kind matrix, jet_vector_math_impl.cu dispatchers)
        check(op(c, s), ref_op(rc, rs))
        check(op(s, d), ref_op(rs, rd))
        # pure-scalar op yields a scalar JV (reference PURE_SCALAR_OP);
        # materialize it by adding a zero dense vector.
        ss = op(s, _core.jv_scalar(0.5, N))
        z, rz = dense(gpu)
        zero = _core.jv_sub(z, z)
        check(_core.jv_add(ss, zero),
              ref_op(rs, Ref(np.full(NI, 0.5))) + Ref(np.zeros(NI),
                                                      np.zeros((N, NI))))


def run_unary_suite(gpu):
    a, ra = dense(gpu)
    v, g = _core.jv_neg(a).to_numpy()
    np.testing.assert_allclose(v, -ra.v)
    np.testing.assert_allclose(g, -ra.g)
    v, g = _core.jv_sin(a).to_numpy()
    np.testing.assert_allclose(v, np.sin(ra.v))
    np.testing.assert_allclose(g, np.cos(ra.v) * ra.g)
    v, g = _core.jv_cos(a).to_numpy()
    np.testing.assert_allclose(v, np.cos(ra.v))
    np.testing.assert_allclose(g, -np.sin(ra.v) * ra.g)
    v, g = _core.jv_sqrt(a).to_numpy()
    np.testing.assert_allclose(v, np.sqrt(ra.v))
    np.testing.assert_allclose(g, 0.5 / np.sqrt(ra.v) * ra.g)
    b, rb = jpv(0, gpu)
    v, g = _core.jv_abs(b).to_numpy()
    np.testing.assert_allclose(v, np.abs(rb.v))
    np.testing.assert_allclose(g, np.sign(rb.v) * rb.g)


def test_binary_cpu():
    run_binary_suite(False)


def test_unary_cpu():
    run_unary_suite(False)


def test_angle_axis_geo_cpu():
    # R(aa) from the JetVector composition vs scipy-style rotation matrices,
    # and gradients vs finite differences.
    ni = 40
    aa_val = rng.normal(scale=0.6, size=(3, ni))
    aa = [_core.JetVector(aa_val[i], None, N=3, grad_pos=i) for i in range(3)]
    R = _core.jv_angle_axis_to_rotation(aa)
    assert len(R) == 9

    def rot(a):
        th = np.linalg.norm(a)
        w = a / th
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K

    for k in range(9):
        v, g = R[k].to_numpy()
        i, j = divmod(k, 3)
        for item in range(0, ni, 7):
            a = aa_val[:, item]
            np.testing.assert_allclose(v[item], rot(a)[i, j], rtol=1e-9)
            for d in range(3):
                eps = 1e-7
                ap, am = a.copy(), a.copy()
                ap[d] += eps
                am[d] -= eps
                fd = (rot(ap)[i, j] - rot(am)[i, j]) / (2 * eps)
                np.testing.assert_allclose(g[d, item], fd, atol=1e-6)


def test_quaternion_geo_cpu():
    ni = 30
    q_val = rng.normal(size=(4, ni))
    q = [_core.JetVector(q_val[i], None, N=4, grad_pos=i) for i in range(4)]
    qn = _core.jv_normalize_quaternion(q)
    R = _core.jv_quaternion_to_rotation(qn)
    for item in range(0, ni, 5):
        qq = q_val[:, item]
        qq = qq / np.linalg.norm(qq)
        w, x, y, z = qq
        Rref = np.array([
            [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        for k in range(9):
            v, _ = R[k].to_numpy()
            np.testing.assert_allclose(v[item], Rref.reshape(-1)[k], rtol=1e-9)
        # orthonormality
        Rm = np.array([R[k].to_numpy()[0][item] for k in range(9)]).reshape(3, 3)
        np.testing.assert_allclose(Rm @ Rm.T, np.eye(3), atol=1e-9)


def test_rotation2d_cpu():
    th_val = rng.normal(size=20)
    th = _core.JetVector(th_val, None, N=1, grad_pos=0)
    R = _core.jv_rotation2d(th)
    v0, g0 = R[0].to_numpy()
    v1, g1 = R[1].to_numpy()
    np.testing.assert_allclose(v0, np.cos(th_val))
    np.testing.assert_allclose(v1, -np.sin(th_val))
    np.testing.assert_allclose(g0[0], -np.sin(th_val))


def test_radial_distortion_cpu():
    ni = 25
    p = [_core.JetVector(rng.normal(size=ni), None, N=2, grad_pos=i)
         for i in range(2)]
    intr_val = np.stack([np.full(ni, 500.0), np.full(ni, 1e-3),
                         np.full(ni, 1e-6)])
    intr = [_core.JetVector(intr_val[i], None, N=2) for i in range(3)]
    fr = _core.jv_radial_distortion(p, intr)
    v, g = fr.to_numpy()
    pv = np.stack([p[0].to_numpy()[0], p[1].to_numpy()[0]])
    r2 = (pv ** 2).sum(axis=0)
    np.testing.assert_allclose(
        v, intr_val[0] * (1 + intr_val[1] * r2 + intr_val[2] * r2 ** 2))


@pytest.mark.gpu
def test_binary_gpu():
    run_binary_suite(True)


@pytest.mark.gpu
def test_unary_gpu():
    run_unary_suite(True)


@pytest.mark.gpu
def test_geo_gpu_matches_cpu():
    ni = 64
    aa_val = rng.normal(scale=0.6, size=(3, ni))
    for gpu in (False, True):
        aa = [_core.JetVector(aa_val[i], None, N=3, grad_pos=i, gpu=gpu)
              for i in range(3)]
        R = _core.jv_angle_axis_to_rotation(aa)
        out = [R[k].to_numpy() for k in range(9)]
        if not gpu:
            ref = out
    for k in range(9):
        np.testing.assert_allclose(out[k][0], ref[k][0], rtol=1e-12)
        np.testing.assert_allclose(out[k][1], ref[k][1], rtol=1e-12)


def test_rotation_to_quaternion_roundtrip_cpu():
    # q -> R -> q' must reproduce q (up to sign), values and gradients.
    ni = 64
    q_val = rng.normal(size=(4, ni))
    q_val /= np.linalg.norm(q_val, axis=0, keepdims=True)
    # force some items into each Shepperd branch via sign flips
    q_val[:, ::4] = np.abs(q_val[:, ::4])
    q = [_core.JetVector(q_val[i], None, N=4, grad_pos=i) for i in range(4)]
    R = _core.jv_quaternion_to_rotation(q)
    q2 = _core.jv_rotation_to_quaternion(R)
    v2 = np.stack([q2[k].to_numpy()[0] for k in range(4)])
    # fix sign per item (quaternion double cover)
    sign = np.sign((v2 * q_val).sum(axis=0))
    np.testing.assert_allclose(v2 * sign, q_val, atol=1e-9)
    # gradient check vs finite differences through the full chain
    def chain(qi):
        w, x, y, z = qi
        Rm = np.array([
            [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        t = np.trace(Rm)
        b = int(np.argmax([t, Rm[0, 0], Rm[1, 1], Rm[2, 2]]))
        if b == 0:
            s = np.sqrt(1 + t)
            return np.array([s / 2, (Rm[2, 1] - Rm[1, 2]) / (2 * s),
                             (Rm[0, 2] - Rm[2, 0]) / (2 * s),
                             (Rm[1, 0] - Rm[0, 1]) / (2 * s)])
        if b == 1:
            s = np.sqrt(1 + Rm[0, 0] - Rm[1, 1] - Rm[2, 2])
            return np.array([(Rm[2, 1] - Rm[1, 2]) / (2 * s), s / 2,
                             (Rm[1, 0] + Rm[0, 1]) / (2 * s),
                             (Rm[0, 2] + Rm[2, 0]) / (2 * s)])
        if b == 2:
            s = np.sqrt(1 - Rm[0, 0] + Rm[1, 1] - Rm[2, 2])
            return np.array([(Rm[0, 2] - Rm[2, 0]) / (2 * s),
                             (Rm[1, 0] + Rm[0, 1]) / (2 * s), s / 2,
                             (Rm[2, 1] + Rm[1, 2]) / (2 * s)])
        s = np.sqrt(1 - Rm[0, 0] - Rm[1, 1] + Rm[2, 2])
        return np.array([(Rm[1, 0] - Rm[0, 1]) / (2 * s),
                         (Rm[0, 2] + Rm[2, 0]) / (2 * s),
                         (Rm[2, 1] + Rm[1, 2]) / (2 * s), s / 2])

    grads = [q2[k].to_numpy()[1] for k in range(4)]
    eps = 1e-7
    for item in range(0, ni, 9):
        qi = q_val[:, item]
        for d in range(4):
            qp, qm = qi.copy(), qi.copy()
            qp[d] += eps
            qm[d] -= eps
            fd = (chain(qp) - chain(qm)) / (2 * eps)
            for k in range(4):
                np.testing.assert_allclose(grads[k][d, item], fd[k], atol=1e-5)


def test_normalize_angle_cpu():
    th = rng.normal(scale=6.0, size=50)
    j = _core.JetVector(th, None, N=1, grad_pos=0)
    out = _core.jv_normalize_angle(j)
    v, g = out.to_numpy()
    ref = th - 2 * np.pi * np.floor((th + np.pi) / (2 * np.pi))
    np.testing.assert_allclose(v, ref, atol=1e-12)
    assert (v > -np.pi - 1e-12).all() and (v <= np.pi + 1e-12).all()
    np.testing.assert_allclose(g[0], np.ones(50))
    # DENSE input with a random gradient, boundary values, JPV on the same
    # values: the gradient passes through unchanged.
    th, gin, (v, g), (vj, gj) = normalize_angle_cases(False)
    ref = th - 2 * np.pi * np.floor((th + np.pi) / (2 * np.pi))
    np.testing.assert_allclose(v, ref, atol=1e-12)
    assert (v >= -np.pi - 1e-12).all() and (v < np.pi + 1e-12).all()
    assert np.array_equal(g, gin)
    assert np.array_equal(vj, v)
    assert np.array_equal(gj, Ref.leaf(th, 1).g)


ANGLE_EDGES = np.array([-np.pi, np.pi, 3 * np.pi, 0.0])


def normalize_angle_cases(gpu):
    """normalize_angle of a DENSE and a JPV operand over random angles plus
    the wrap boundaries, exact and 1e-12 to either side."""
    r = np.random.default_rng(5)
    th = np.concatenate([r.normal(scale=6.0, size=50), ANGLE_EDGES,
                         ANGLE_EDGES - 1e-12, ANGLE_EDGES + 1e-12])
    gin = r.normal(size=(N, len(th)))
    d = _core.jv_normalize_angle(_core.JetVector(th, gin, N=N, gpu=gpu))
    j = _core.jv_normalize_angle(
        _core.JetVector(th, None, N=N, grad_pos=1, gpu=gpu))
    return th, gin, d.to_numpy(), j.to_numpy()


@pytest.mark.gpu
def test_normalize_angle_gpu_equals_cpu():
    # Same IEEE operations on both backends: bit for bit.
    _, _, (v, g), (vj, gj) = normalize_angle_cases(False)
    _, _, (v2, g2), (vj2, gj2) = normalize_angle_cases(True)
    assert np.array_equal(v2, v) and np.array_equal(g2, g)
    assert np.array_equal(vj2, vj) and np.array_equal(gj2, gj)


UNARY = [(_core.jv_neg, lambda v: -v, lambda v: -np.ones_like(v)),
         (_core.jv_abs, np.abs, np.sign),
         (_core.jv_sin, np.sin, np.cos),
         (_core.jv_cos, np.cos, lambda v: -np.sin(v)),
         (_core.jv_sqrt, np.sqrt, lambda v: 0.5 / np.sqrt(v))]


def run_unary_kinds(gpu):
    """All five unary ops on a DENSE and on a JPV operand."""
    r = np.random.default_rng(11)
    for op, f, df in UNARY:
        v = r.normal(size=NI) + 3.0
        if op is _core.jv_abs:
            v[::2] -= 6.0  # half the items negative
            assert (v < 0).sum() > NI // 4 and (v > 0).sum() > NI // 4
        if op is _core.jv_sqrt:
            v = np.abs(v) + 0.5
        g = r.normal(size=(N, NI))
        for jv_in, rin in (
                (_core.JetVector(v, g, N=N, gpu=gpu), Ref(v, g)),
                (_core.JetVector(v, None, N=N, grad_pos=2, gpu=gpu),
                 Ref.leaf(v, 2))):
            ov, og = op(jv_in).to_numpy()
            np.testing.assert_allclose(ov, f(v))
            np.testing.assert_allclose(og, df(v) * rin.g)


def test_unary_kinds_cpu():
    run_unary_kinds(False)


@pytest.mark.gpu
def test_unary_kinds_gpu():
    run_unary_kinds(True)


def rot2quat_case(gpu):
    """The q -> R -> q' chain of the round-trip test on fixed inputs; returns
    q and the (value, grad) pairs of q'."""
    ni = 64
    r = np.random.default_rng(3)
    q_val = r.normal(size=(4, ni))
    q_val /= np.linalg.norm(q_val, axis=0, keepdims=True)
    q_val[:, ::4] = np.abs(q_val[:, ::4])
    q = [_core.JetVector(q_val[i], None, N=4, grad_pos=i, gpu=gpu)
         for i in range(4)]
    q2 = _core.jv_rotation_to_quaternion(_core.jv_quaternion_to_rotation(q))
    return q_val, [q2[k].to_numpy() for k in range(4)]


def shepperd_branch(q_val):
    w, x, y, z = q_val
    r00 = 1 - 2 * (y * y + z * z)
    r11 = 1 - 2 * (x * x + z * z)
    r22 = 1 - 2 * (x * x + y * y)
    return np.argmax(np.stack([r00 + r11 + r22, r00, r11, r22]), axis=0)


@pytest.mark.gpu
def test_rotation_to_quaternion_gpu_equals_cpu():
    """GPU q -> R -> q' equals the CPU backend's to rtol=1e-12.

    The bound has no absolute floor, and the gradients of the minor
    components hold differences that cancel, to exactly 0 where q' does not
    depend on the parameter.  The rounding residue left there (order 1e-16)
    depends on whether a*b + c*d is fused; the Shepperd body is therefore
    compiled without FMA contraction, and every product feeding it here has
    a 0/1 or scalar factor, so the two backends agree bit for bit.  With a
    contracting device build 51, 31, 33 and 38 of the 256 gradient entries
    of q'[0..3] miss the bound (largest absolute difference 2.2e-16).
    """
    q_val, ref = rot2quat_case(False)
    _, out = rot2quat_case(True)
    # every Shepperd branch is taken by some items
    assert (np.bincount(shepperd_branch(q_val), minlength=4) >= 4).all()
    for k in range(4):
        for part in (0, 1):
            d = np.abs(out[k][part] - ref[k][part])
            bad = d > 1e-12 * np.abs(ref[k][part])
            print(f"q'[{k}] {'value' if part == 0 else 'grad'}: "
                  f"max abs diff {d.max():.3g}, {bad.sum()} of {d.size} "
                  f"beyond rtol, largest |ref| among them "
                  f"{np.abs(ref[k][part][bad]).max() if bad.any() else 0:.3g}")
    for k in range(4):
        np.testing.assert_allclose(out[k][0], ref[k][0], rtol=1e-12)
        np.testing.assert_allclose(out[k][1], ref[k][1], rtol=1e-12)


@pytest.mark.gpu
def test_binary_grid_stride_gpu():
    # One item more than 4096 blocks x 256 threads cover in one trip, plus an
    # odd tail: some threads take a second trip through the grid-stride loop.
    ni = 4096 * 256 + 257
    r = np.random.default_rng(7)
    av, ag, bv = r.normal(size=ni), r.normal(size=(1, ni)), r.normal(size=ni)
    a = _core.JetVector(av, ag, N=1, gpu=True)
    b = _core.JetVector(bv, None, N=1, grad_pos=0, gpu=True)
    v, g = _core.jv_mul(a, b).to_numpy()
    np.testing.assert_allclose(v, av * bv, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(g, ag * bv + av, rtol=1e-12, atol=1e-13)
