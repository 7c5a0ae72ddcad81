"""The scene set-up kernels of csrc/geometry.hip restated in numpy: ``pr_pose_matrices`` / ``pr_pose_matrices_backward``,
``pr_project_points``, ``pr_camera_rays``, ``pr_scene_setup`` / ``pr_scene_setup_backward``.  No torch, no GPU.

Every kernel is restated twice.

* In float64, from the definition: ``M = [R t; 0 1]`` with ``R = Ry (Rx Rz)`` and ``M^-1 = [R^T  -R^T t; 0 1]`` as matrix products;
  the pose backward as the reverse-mode adjoint of that product chain (``gRy = gR XZ^T``, ``gXZ = Ry^T gR``, ``gRx = gXZ Rz^T``,
  ``gRz = Rx^T gXZ``, each angle's gradient read off the four trigonometric entries of its factor) - NOT the kernel's
  ``<gR, dR / d angle>`` with three differentiated products; the projection as ``world = Ro p + to``, ``cam = Rc world + tc``,
  ``(-x / z f, y / z f)``, ``(v + size / 2) / size``; the rays as ``c2w[:, :3] (dx, dy, -1)``.  tests/test_scene_cpu.py holds these to torch
  autograd in float64, to the package's tensor formulation and to the recorded fixtures.
* In fp32, following the kernel's operation order with one rounding per operation (``np.float32``; the library is built with
  ``-ffp-contract=off``, the backward's ``fmaf`` is one rounding of the exact product-sum).  ``project_object``, ``k_camera_rays`` and the
  copies of ``k_scene_setup`` use only round-to-nearest ``mul / add / div``, comparisons and selects (``nan_min / nan_max / nan_clamp`` keep a
  NaN as ``torch.min / max / clamp`` do), so from the same fp32 matrices the device must give these restatements BIT FOR BIT (two NaNs count
  as equal).  The pose kernels call ``sinf / cosf``, which are not correctly rounded: there the fp32 restatement is a diagnostic and
  the float64 one is the judge.

Tolerances.  The pose chains are written once (``_pose_forward_chain``, ``_pose_backward_chain``) over an arithmetic: ``_F32`` gives the
fp32 restatement, ``_Bounded`` carries beside every float64 value a first-order bound of |fp32 - float64|: an operation adds
``u = 2^-24`` times the magnitude of its result - for a sum the sum of the ABSOLUTE values of its terms, not the cancelled sum - plus
``tiny = 2^-126`` (a result that is rounded or flushed in the subnormal range) to the propagated errors of its operands
(``|a| e_b + |b| e_a + e_a e_b`` for a product), and every ``sinf / cosf`` enters with the absolute error ``TRIG_ERR``.  The tolerances
``tol_*`` returned with the float64 results are these bounds.  Operation counts, read from the kernels (constants 0 and 1 are charged
like any operand, which only widens the bound by roundings that do not happen):

* ``pose_pair``: 6 trig calls; ``Rx Rz`` and ``Ry (Rx Rz)``: 27 products and 27 sums each (the accumulator starts from 0); the inverse's
  translation: 9 products, 9 sums and a negation (exact).  ``m[:3, 3] = t`` and the bottom rows are copies: tolerance 0.
* ``pose_backward``: 6 trig calls; ``Rx Rz``, ``Ry (Rx Rz)`` and the five products of the differentiated factors: 27 products and 18 sums each;
  ``gR``: 9 x (sum, product, difference); ``g_tr``: 3 x (3 products, 2 sums, a difference); three 9-term ``fmaf`` chains.
* ``k_scene_setup_bwd``: ``C`` sums per element of ``gv`` (from 0) in front of ``pose_backward``; ``C`` sums per style / deformation element:
  at most ``(C - 1) u sum_c |x_c|`` (``scene_setup_backward_float64`` returns it; one camera: exact).
* ``project_object`` (the same arithmetic gives its float64 bound): 2 x (9 products, 9 sums), 2 quotients, 2 products, then a sum and a
  quotient per coordinate; a box edge is a minimum / maximum (1-Lipschitz: the largest bound among the points that count) and a sum and
  a quotient; the clamps are 1-Lipschitz.

``TRIG_ERR`` cannot be derived here; it is measured on the GPU THROUGH ``pr_pose_matrices`` (tests/test_scene_gpu.py,
``test_trig_error_measured_through_the_kernel``): for angles ``(0, 0, a)`` the kernel's ``m[0][0]`` and ``m[1][0]`` are ``cosf(a)`` and ``sinf(a)``
exactly (every other factor is 0 or 1, so the products and sums are exact), likewise ``m[1][1], m[2][1]`` for ``(a, 0, 0)`` and
``m[0][0], m[0][2]`` for ``(0, a, 0)``; the error is taken against float64 ``sin / cos`` of the same fp32 angle over every angle the tests
draw (``trig_angles``, 17 388 of them, each on all three axes).  Measured on an MI355X: 6.541e-08, and the same 6.541e-08 at the large
angles alone (on ``large_1e2``); numpy's fp32 sine and cosine show 6.541e-08 on these angles too, about 0.55 ulp of a value next to 1.
``TRIG_ERR = 1.31e-07`` is twice that, the margin for angles not drawn.
Because the constant is measured through the kernel under test, a wrong trig call must not be able to widen its own tolerance: the
measured error at the large angles (the ``large_1e2`` and ``large_1e4`` families) has to stay below ``fast_trig_floor()``, the smallest -
over those two families - of the largest error a range-reduction-free fast intrinsic shows on the family's angles.  Such an intrinsic
(``__sinf``: the hardware sine of ``x / (2 pi)`` in revolutions) rounds ``x * fp32(1 / (2 pi))`` to fp32 first, which costs about ``1e-7 |x|``
in the angle: 1.37e-05 on ``large_1e2`` and 1.50e-03 on ``large_1e4`` (so the floor is 1.37e-05) against 6.5e-08 for ``sinf``.  ``fast_trig`` is that model;
tests/test_scene_cpu.py shows that a pose kernel built on it falls outside ``tol_*``.

Both test files draw their inputs from the functions at the end of this module, so the CPU file proves the tolerances on exactly what
the GPU file runs."""
import functools
from typing import NamedTuple, Optional

import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126
TRIG_ERR = 1.31e-07                # 2 x the error measured through pr_pose_matrices on an MI355X (module docstring)
BIG = F(1e20)                      # what a point behind the camera counts as in the box reduction
PR_MAX_OBJECTS = 8


# ---------------------------------------------------------------------------------------------------------------------
# the two arithmetics
class _F32:
    """``np.float32`` arrays: one rounding per operation.  ``fast``: sin / cos as a range-reduction-free intrinsic would give them."""

    def __init__(self, fast=False):
        self.fast = fast

    def const(self, x, n):
        return np.full(n, x, F)

    def lift(self, x):
        return np.asarray(x, F)

    def trig(self, a):
        a = np.asarray(a, F)
        with np.errstate(invalid="ignore"):
            if self.fast:
                c, s = fast_trig(a)
                return c.astype(F), s.astype(F)
            return np.cos(a, dtype=F), np.sin(a, dtype=F)

    add = staticmethod(lambda a, b: a + b)
    sub = staticmethod(lambda a, b: a - b)
    mul = staticmethod(lambda a, b: a * b)
    div = staticmethod(lambda a, b: a / b)
    neg = staticmethod(lambda a: -a)

    @staticmethod
    def fma(a, b, c):
        # (the product of two fp32 values is exact in float64; the sum rounds twice, to float64 and to fp32 - a diagnostic's precision)
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


class _Bounded:
    """``(value, bound)`` pairs of float64 arrays: the float64 result and a first-order bound of |fp32 chain - value| (module docstring)."""

    def __init__(self, trig_err=None):
        self.trig_err = TRIG_ERR if trig_err is None else trig_err

    def const(self, x, n):
        return np.full(n, float(x)), np.zeros(n)

    def lift(self, x):
        x = np.asarray(x, np.float64)
        return x, np.zeros(x.shape)

    def trig(self, a):
        a = np.asarray(a, np.float64)
        e = np.full(a.shape, self.trig_err)
        return (np.cos(a), e), (np.sin(a), e)

    @staticmethod
    def add(a, b):
        e = a[1] + b[1]
        return a[0] + b[0], e + U * (np.abs(a[0]) + np.abs(b[0]) + e) + TINY

    @staticmethod
    def sub(a, b):
        e = a[1] + b[1]
        return a[0] - b[0], e + U * (np.abs(a[0]) + np.abs(b[0]) + e) + TINY

    @staticmethod
    def mul(a, b):
        v = a[0] * b[0]
        e = np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1]
        return v, e + U * (np.abs(v) + e) + TINY

    @staticmethod
    def div(a, b):
        v = a[0] / b[0]
        e = (a[1] + np.abs(v) * b[1]) / np.maximum(np.abs(b[0]) - b[1], TINY)
        return v, e + U * (np.abs(v) + e) + TINY

    @staticmethod
    def neg(a):
        return -a[0], a[1]

    @staticmethod
    def fma(a, b, c):
        v = a[0] * b[0]
        e = np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1] + c[1]
        return v + c[0], e + U * (np.abs(v) + np.abs(c[0]) + e) + TINY


def fast_trig(a):
    """``(cos, sin)`` as a fast intrinsic without range reduction gives them, in float64: the hardware evaluates the sine of an angle in
    revolutions, so the argument is ``fp32(a * fp32(1 / (2 pi)))`` - a rounding of about ``1e-7 |a|`` in the angle."""
    rev = (np.asarray(a, F) * F(0.15915494309189535)).astype(np.float64)
    return np.cos(2.0 * np.pi * rev), np.sin(2.0 * np.pi * rev)


# ---------------------------------------------------------------------------------------------------------------------
# pose: the kernel's chains over an arithmetic
def _factors(ops, ax, ay, az):
    (cx, sx), (cy, sy), (cz, sz) = ops.trig(ax), ops.trig(ay), ops.trig(az)
    n = np.shape(ax)
    Z, O, neg = ops.const(0.0, n), ops.const(1.0, n), ops.neg
    rx = [O, Z, Z, Z, cx, neg(sx), Z, sx, cx]
    ry = [cy, Z, sy, Z, O, Z, neg(sy), Z, cy]
    rz = [cz, neg(sz), Z, sz, cz, Z, Z, Z, O]
    return (cx, sx, cy, sy, cz, sz), (rx, ry, rz), Z


def _mm_from_zero(ops, a, b, zero):
    """pose_pair's product: ``acc = 0; acc = acc + a[i][k] b[k][j]`` for k = 0, 1, 2."""
    out = []
    for i in range(3):
        for j in range(3):
            acc = zero
            for k in range(3):
                acc = ops.add(acc, ops.mul(a[i * 3 + k], b[k * 3 + j]))
            out.append(acc)
    return out


def _mm(ops, a, b):
    """mat3_mul: ``(a0 b0 + a1 b1) + a2 b2``."""
    return [ops.add(ops.add(ops.mul(a[i * 3], b[j]), ops.mul(a[i * 3 + 1], b[3 + j])), ops.mul(a[i * 3 + 2], b[6 + j]))
            for i in range(3) for j in range(3)]


def _pose_forward_chain(ops, rot, tr, mutant=None):
    """``pose_pair`` over ``ops``: the 3 x 3 rotation (9 entries) and the inverse's translation (3), each an array over the matrices."""
    _, (rx, ry, rz), zero = _factors(ops, rot[:, 0], rot[:, 1], rot[:, 2])
    if mutant == "rx_ry_rz":
        r = _mm_from_zero(ops, rx, _mm_from_zero(ops, ry, rz, zero), zero)
    else:
        r = _mm_from_zero(ops, ry, _mm_from_zero(ops, rx, rz, zero), zero)
    t = [ops.lift(tr[:, k]) for k in range(3)]
    u = []
    for a in range(3):
        acc = zero
        for k in range(3):
            acc = ops.add(acc, ops.mul(r[k * 3 + a], t[k]))
        u.append(acc if mutant == "inverse_plus_rt_t" else ops.neg(acc))
    return r, u


def _pose_backward_chain(ops, rot, tr, gm, gv, mutant=None, gv_err=None):
    """``pose_backward`` over ``ops``: ``g_rot`` (3) and ``g_tr`` (3).  ``gm`` / ``gv``: (n, 4, 4) gradients of the matrix / of its inverse, or
    None.  Only their first three rows are read.  ``gv_err`` (``_Bounded`` only): the bound that ``gv`` already carries."""
    (cx, sx, cy, sy, cz, sz), (rx, ry, rz), Z = _factors(ops, rot[:, 0], rot[:, 1], rot[:, 2])
    neg = ops.neg
    dx = [Z, Z, Z, Z, sx if mutant == "dx_sign" else neg(sx), neg(cx), Z, cx, neg(sx)]
    dy = [sy if mutant == "dy_sign" else neg(sy), Z, cy, Z, Z, Z, neg(cy), Z, neg(sy)]
    dz = [neg(sz), cz if mutant == "dz_sign" else neg(cz), Z, cz, neg(sz), Z, Z, Z, Z]
    xz = _mm(ops, rx, rz)
    r = _mm(ops, ry, xz)
    t = [ops.lift(tr[:, k]) for k in range(3)]
    def at(g, i, j):
        if g is None:
            return Z
        x = ops.lift(g[:, i, j])
        return (x[0], gv_err[:, i, j]) if (g is gv and gv_err is not None) else x
    gu = [at(gv, a, 3) for a in range(3)]
    gr, g_tr = [], []
    for k in range(3):
        for a in range(3):
            from_inverse = at(gv, k, a) if mutant == "gv_transposed" else at(gv, a, k)
            term = ops.add(at(gm, k, a), from_inverse)
            gr.append(term if mutant == "t_gu_dropped" else ops.sub(term, ops.mul(t[k], gu[a])))
        row = [r[a * 3 + k] for a in range(3)] if mutant == "rt_gu" else [r[k * 3 + a] for a in range(3)]
        rgu = ops.add(ops.add(ops.mul(row[0], gu[0]), ops.mul(row[1], gu[1])), ops.mul(row[2], gu[2]))
        g_tr.append(ops.sub(at(gm, k, 3), rgu))

    def dot(d):
        acc = Z
        for i in range(9):
            acc = ops.fma(gr[i], d[i], acc)
        return acc
    g_rot = [dot(_mm(ops, ry, _mm(ops, dx, rz))), dot(_mm(ops, dy, xz)), dot(_mm(ops, ry, _mm(ops, rx, dz)))]
    return g_rot, g_tr


# ---------------------------------------------------------------------------------------------------------------------
# pose: float64 from the definition
class Pose(NamedTuple):
    m: np.ndarray                  # (n, 4, 4)
    inv: np.ndarray                # (n, 4, 4)
    tol_m: Optional[np.ndarray] = None
    tol_inv: Optional[np.ndarray] = None


class PoseGrad(NamedTuple):
    g_rot: np.ndarray              # (n, 3)
    g_tr: np.ndarray               # (n, 3)
    tol_rot: Optional[np.ndarray] = None
    tol_tr: Optional[np.ndarray] = None


def _rotation_factors64(rot):
    rot = np.asarray(rot, np.float64)
    n = rot.shape[0]
    c, s = np.cos(rot), np.sin(rot)
    rx, ry, rz = (np.tile(np.eye(3), (n, 1, 1)) for _ in range(3))
    rx[:, 1, 1], rx[:, 1, 2], rx[:, 2, 1], rx[:, 2, 2] = c[:, 0], -s[:, 0], s[:, 0], c[:, 0]
    ry[:, 0, 0], ry[:, 0, 2], ry[:, 2, 0], ry[:, 2, 2] = c[:, 1], s[:, 1], -s[:, 1], c[:, 1]
    rz[:, 0, 0], rz[:, 0, 1], rz[:, 1, 0], rz[:, 1, 1] = c[:, 2], -s[:, 2], s[:, 2], c[:, 2]
    return c, s, rx, ry, rz


def _assemble(r, u, tr, dtype):
    """(n, 4, 4) matrix and inverse from the chain's 9 + 3 arrays."""
    n = tr.shape[0]
    m, inv = np.zeros((n, 4, 4), dtype), np.zeros((n, 4, 4), dtype)
    for a in range(3):
        for b in range(3):
            m[:, a, b] = r[a * 3 + b]
            inv[:, a, b] = r[b * 3 + a]
        inv[:, a, 3] = u[a]
    m[:, :3, 3] = tr
    m[:, 3, 3] = inv[:, 3, 3] = 1
    return m, inv


def pose_float64(rot, tr, trig_err=None) -> Pose:
    """``pr_pose_matrices`` in float64 from fp32 angles (n, 3) and translations (n, 3), with the tolerances of the fp32 kernel."""
    rot, tr = np.asarray(rot, np.float64).reshape(-1, 3), np.asarray(tr, np.float64).reshape(-1, 3)
    n = rot.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        _, _, rx, ry, rz = _rotation_factors64(rot)
        r = ry @ (rx @ rz)
        m, inv = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
        m[:, :3, :3], m[:, :3, 3], m[:, 3, 3] = r, tr, 1.0
        inv[:, :3, :3], inv[:, 3, 3] = r.transpose(0, 2, 1), 1.0
        inv[:, :3, 3] = -np.einsum("nka,nk->na", r, tr)
        rb, ub = _pose_forward_chain(_Bounded(trig_err), rot, tr)
        tol_m, tol_inv = _assemble([x[1] for x in rb], [x[1] for x in ub], np.zeros((n, 3)), np.float64)
        tol_m[:, 3, 3] = tol_inv[:, 3, 3] = 0.0
    return Pose(m, inv, tol_m, tol_inv)


def pose_fp32(rot, tr, mutant=None) -> Pose:
    """``pose_pair`` in ``np.float32`` (``np.sin / np.cos`` for ``sinf / cosf``: a diagnostic).  ``mutant``: a wrong kernel (test_scene_cpu.py)."""
    rot, tr = np.asarray(rot, F).reshape(-1, 3), np.asarray(tr, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r, u = _pose_forward_chain(_F32(fast=mutant == "fast_trig"), rot, tr, mutant)
    return Pose(*_assemble(r, u, tr, F))


def pose_backward_float64(rot, tr, gm, gi, trig_err=None, gi_err=None) -> PoseGrad:
    """``pr_pose_matrices_backward`` in float64 as the reverse-mode adjoint of ``R = Ry (Rx Rz)``, ``M = [R t; 0 1]``,
    ``M^-1 = [R^T u; 0 1]``, ``u = -R^T t``.  ``gm`` / ``gi``: (n, 4, 4) gradients of the matrix / of the inverse, either may be None.
    ``gi_err``: a bound that the fp32 ``gi`` already carries (the camera sum of ``k_scene_setup_bwd``)."""
    rot, tr = np.asarray(rot, np.float64).reshape(-1, 3), np.asarray(tr, np.float64).reshape(-1, 3)
    n = rot.shape[0]
    gm = None if gm is None else np.asarray(gm, np.float64).reshape(n, 4, 4)
    gi = None if gi is None else np.asarray(gi, np.float64).reshape(n, 4, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        c, s, rx, ry, rz = _rotation_factors64(rot)
        xz = rx @ rz
        r = ry @ xz
        g_r, g_t = np.zeros((n, 3, 3)), np.zeros((n, 3))
        if gm is not None:
            g_r += gm[:, :3, :3]
            g_t += gm[:, :3, 3]
        if gi is not None:
            gu = gi[:, :3, 3]
            g_r += gi[:, :3, :3].transpose(0, 2, 1)              # the inverse holds R^T
            g_r -= tr[:, :, None] * gu[:, None, :]               # u_a = -sum_k R[k][a] t[k]
            g_t -= np.einsum("nka,na->nk", r, gu)                # d u / d t = -R^T
        g_ry = g_r @ xz.transpose(0, 2, 1)
        g_xz = ry.transpose(0, 2, 1) @ g_r
        g_rx = g_xz @ rz.transpose(0, 2, 1)
        g_rz = rx.transpose(0, 2, 1) @ g_xz
        g_rot = np.stack([
            -s[:, 0] * g_rx[:, 1, 1] - c[:, 0] * g_rx[:, 1, 2] + c[:, 0] * g_rx[:, 2, 1] - s[:, 0] * g_rx[:, 2, 2],
            -s[:, 1] * g_ry[:, 0, 0] + c[:, 1] * g_ry[:, 0, 2] - c[:, 1] * g_ry[:, 2, 0] - s[:, 1] * g_ry[:, 2, 2],
            -s[:, 2] * g_rz[:, 0, 0] - c[:, 2] * g_rz[:, 0, 1] + c[:, 2] * g_rz[:, 1, 0] - s[:, 2] * g_rz[:, 1, 1]], axis=1)
        rb, tb = _pose_backward_chain(_Bounded(trig_err), rot, tr, gm, gi, gv_err=gi_err)
    return PoseGrad(g_rot, g_t, np.stack([x[1] for x in rb], 1), np.stack([x[1] for x in tb], 1))


def pose_backward_chain_float64(rot, tr, gm, gi) -> PoseGrad:
    """The VALUES of the bounded chain: the kernel's own formula in float64 (test_scene_cpu.py holds it to the adjoint above)."""
    rot, tr = np.asarray(rot, np.float64).reshape(-1, 3), np.asarray(tr, np.float64).reshape(-1, 3)
    rb, tb = _pose_backward_chain(_Bounded(), rot, tr, gm, gi)
    return PoseGrad(np.stack([x[0] for x in rb], 1), np.stack([x[0] for x in tb], 1))


def pose_backward_fp32(rot, tr, gm, gi, mutant=None) -> PoseGrad:
    """``pose_backward`` in ``np.float32``, the kernel's order (a diagnostic, and the carrier of the mutants)."""
    rot, tr = np.asarray(rot, F).reshape(-1, 3), np.asarray(tr, F).reshape(-1, 3)
    n = rot.shape[0]
    gm = None if gm is None else np.asarray(gm, F).reshape(n, 4, 4)
    gi = None if gi is None else np.asarray(gi, F).reshape(n, 4, 4)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        g_rot, g_tr = _pose_backward_chain(_F32(fast=mutant == "fast_trig"), rot, tr, gm, gi, mutant)
    return PoseGrad(np.stack(g_rot, 1), np.stack(g_tr, 1))


# ---------------------------------------------------------------------------------------------------------------------
# projection
class Projection(NamedTuple):
    points: np.ndarray             # (F, C, P, 2, K)
    boxes: Optional[np.ndarray]    # (F, C, 4, K) [left, top, right, bottom]; None: the axes variant
    cam_z: np.ndarray              # (F, C, K, P) camera-frame z of every point
    tol_points: Optional[np.ndarray] = None
    tol_boxes: Optional[np.ndarray] = None


def _project_chain(ops, pts, o2w, w2c, focals, height, width, mutant=None):
    """``project_object`` up to the unclamped normalised coordinates, broadcast to (F, C, K, P): px, py, cam z, nx, ny."""
    pt = [ops.lift(pts[None, None, :, :, j]) for j in range(3)]
    mo = [[ops.lift(o2w[:, None, :, None, a, j]) for j in range(4)] for a in range(3)]
    mc = [[ops.lift(w2c[:, :, None, None, a, j]) for j in range(4)] for a in range(3)]
    focal = ops.lift(focals[:, :, None, None])
    add, mul, div, neg = ops.add, ops.mul, ops.div, ops.neg
    through = lambda m, v: [add(add(add(mul(v[0], m[a][0]), mul(v[1], m[a][1])), mul(v[2], m[a][2])), m[a][3]) for a in range(3)]
    cam = through(mc, through(mo, pt))
    px = mul(div(neg(cam[0]), cam[2]), focal)
    py = neg(mul(div(neg(cam[1]), cam[2]), focal))
    w, h = (height, width) if mutant == "height_width_swapped" else (width, height)
    size = lambda v: ops.lift(np.asarray(v, F))
    nx = div(add(px, size(F(w) / F(2))), size(w))
    ny = div(add(py, size(F(h) / F(2))), size(h))
    return px, py, cam[2], nx, ny, (w, h)


def _arrange_points(nx, ny):
    return np.stack([nx, ny], -1).transpose(0, 1, 3, 4, 2)                   # (F, C, K, P, 2) -> (F, C, P, 2, K)


def project_fp32(pts, o2w, w2c, focals, height, width, boxes, mutant=None) -> Projection:
    """``k_project_points`` in ``np.float32``, operation for operation: the device must give these bits."""
    pts, o2w, w2c, focals = (np.asarray(a, F) for a in (pts, o2w, w2c, focals))
    ops = _F32()
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        px, py, z, nx, ny, (w, h) = _project_chain(ops, pts, o2w, w2c, focals, height, width, mutant)
        if not boxes:
            return Projection(_arrange_points(nx, ny), None, z)
        behind = (z >= 0) if mutant == "behind_includes_zero" else (z > 0)
        # (np.min / np.max / np.clip keep a NaN, as nan_min / nan_max / nan_clamp and torch.min / max / clamp do; fminf / fmaxf drop it)
        lowest, highest = (np.fmin.reduce, np.fmax.reduce) if mutant == "fminf_fmaxf" else (np.min, np.max)
        clamp = (lambda v: np.fmin(np.fmax(v, F(0)), F(1))) if mutant == "fminf_fmaxf" else (lambda v: np.clip(v, F(0), F(1)))
        if mutant == "second_pass_not_reduced":                     # the points past the first 64 (i += 64) left out of the reduction
            behind, px, py = behind[..., :64], px[..., :64], py[..., :64]
        elif mutant == "upper_lanes_not_reduced":                   # the d = 32 step of the shuffle tree missing: lanes 32 to 63 left out
            lanes = np.arange(z.shape[-1]) % 64 < 32
            behind, px, py = behind[..., lanes], px[..., lanes], py[..., lanes]
        edges = []
        for p, size, low in ((px, w, True), (py, h, True), (px, w, False), (py, h, False)):
            v = lowest(np.where(behind, BIG, p), axis=-1) if low else highest(np.where(behind, -BIG, p), axis=-1)
            edges.append(clamp((v + F(size) / F(2)) / F(size)))
        out = Projection(_arrange_points(clamp(nx), clamp(ny)), np.stack(edges, 2), z)
    assert out.points.dtype == F and out.boxes.dtype == F
    return out


def project_float64(pts, o2w, w2c, focals, height, width, boxes) -> Projection:
    """The projection in float64 from the definition (the same fp32 matrices), with the first-order bound of the fp32 kernel."""
    pts, o2w, w2c, focals = (np.asarray(a, np.float64) for a in (pts, o2w, w2c, focals))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        world = np.einsum("fkab,kpb->fkpa", o2w[:, :, :3, :3], pts) + o2w[:, :, None, :3, 3]             # (F, K, P, 3)
        cam = np.einsum("fcab,fkpb->fckpa", w2c[:, :, :3, :3], world) + w2c[:, :, None, None, :3, 3]     # (F, C, K, P, 3)
        f = focals[:, :, None, None]
        px, py, z = -cam[..., 0] / cam[..., 2] * f, cam[..., 1] / cam[..., 2] * f, cam[..., 2]
        size = np.array([width, height, width, height], np.float64)
        ops = _Bounded()
        bx, by, _, bnx, bny, _ = _project_chain(ops, pts, o2w, w2c, focals, height, width)
        nx, ny = (px + width / 2) / width, (py + height / 2) / height
        if not boxes:
            return Projection(_arrange_points(nx, ny), None, z, _arrange_points(bnx[1], bny[1]), None)
        behind = z > 0
        edges, tol_edges = [], []
        for p, b, a, low in ((px, bx, 0, True), (py, by, 1, True), (px, bx, 2, False), (py, by, 3, False)):
            v = np.where(behind, 1e20, p).min(-1) if low else np.where(behind, -1e20, p).max(-1)
            e = np.where(behind, 0.0, b[1]).max(-1)
            half = ops.lift(np.full(v.shape, size[a] / 2))
            nv, ne = ops.div(ops.add((v, e), half), ops.lift(np.full(v.shape, size[a])))
            edges.append(np.clip(nv, 0.0, 1.0))
            tol_edges.append(ne)
        return Projection(_arrange_points(np.clip(nx, 0.0, 1.0), np.clip(ny, 0.0, 1.0)), np.stack(edges, 2), z,
                          _arrange_points(bnx[1], bny[1]), np.stack(tol_edges, 2))


# ---------------------------------------------------------------------------------------------------------------------
# camera rays
class Rays(NamedTuple):
    origins: np.ndarray            # (N, 3)
    directions: np.ndarray         # (N, R, 3)
    normals: np.ndarray            # (N, 3)
    tol_directions: Optional[np.ndarray] = None


def _pixels(rows, cols, frames, per_frame, mutant=None):
    rows, cols = np.asarray(rows), np.asarray(cols)
    if per_frame:
        rows, cols = rows.reshape(frames, -1), cols.reshape(frames, -1)
        if mutant == "cols_of_r":
            cols = np.broadcast_to(cols[:1], cols.shape)              # cols[r] where cols[g] is due: every frame reads the first list
    else:
        rows, cols = rows.reshape(1, -1), cols.reshape(1, -1)
    return rows, cols


def camera_rays_fp32(c2w, focals, rows, cols, height, width, per_frame, mutant=None) -> Rays:
    """``k_camera_rays`` in ``np.float32``, operation for operation.  ``c2w``: (N, 3, 4); pixel lists (R) or, ``per_frame``, (N, R)."""
    c2w, focals = np.asarray(c2w, F).reshape(-1, 3, 4), np.asarray(focals, F).reshape(-1)
    rows, cols = _pixels(rows, cols, c2w.shape[0], per_frame, mutant)
    f = focals[:, None]
    dx = (cols.astype(F) - F(width) / F(2)) / f
    dy = -((rows.astype(F) - F(height) / F(2)) / f)
    m = c2w[:, None, :, :]
    directions = (dx[..., None] * m[..., 0] + dy[..., None] * m[..., 1]) + F(-1) * m[..., 2]
    assert directions.dtype == F
    return Rays(c2w[:, :, 3].copy(), directions, -c2w[:, :, 2])


def camera_rays_float64(c2w, focals, rows, cols, height, width, per_frame) -> Rays:
    """The rays in float64: ``c2w[:, :3] (dx, dy, -1)``; the bound is 2 quotient / 3 product / 2 sum roundings on the terms' magnitudes."""
    c2w, focals = np.asarray(c2w, np.float64).reshape(-1, 3, 4), np.asarray(focals, np.float64).reshape(-1)
    rows, cols = _pixels(rows, cols, c2w.shape[0], per_frame)
    d = np.stack(np.broadcast_arrays((cols - width / 2) / focals[:, None], -(rows - height / 2) / focals[:, None], -1.0), -1)   # (N, R, 3)
    directions = np.einsum("nab,nrb->nra", c2w[:, :, :3], d)
    tol = 5 * U * np.einsum("nab,nrb->nra", np.abs(c2w[:, :, :3]), np.abs(d)) + TINY
    return Rays(c2w[:, :, 3].copy(), directions, -c2w[:, :, 2], tol)


# ---------------------------------------------------------------------------------------------------------------------
# the fused scene set-up
def scene_setup_fp32(q, cam_m, cam_inv, obj_m, obj_inv, mutant=None):
    """``k_scene_setup`` from the pose matrices it is given (``pr_pose_matrices`` of the same poses: (F * C, 4, 4) of the cameras,
    (F * K, 4, 4) of the objects in (frame, object) order): every output in the kernel's layout, to be matched bit for bit."""
    Fr, C, K = q["frames"], q["cameras"], q["objects"]
    S, D = q["S"], q["D"]
    cam_m, cam_inv = (np.asarray(a, F).reshape(Fr, C, 4, 4) for a in (cam_m, cam_inv))
    obj_m, obj_inv = (np.asarray(a, F).reshape(Fr, K, 4, 4) for a in (obj_m, obj_inv))
    f1 = q["focals"].astype(F) * F(q["focal_multiplier"])
    render = f1 if q["upsample"] == 1.0 else f1 * F(q["upsample"])
    boxes = project_fp32(q["box_points"], obj_m, cam_inv, render, q["height"], q["width"], True)
    axes = project_fp32(q["axes_points"], obj_m, cam_inv, render if q["axes_with_upsampled_focals"] else f1, q["height"], q["width"], False)
    per_camera = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, None], (Fr, C) + a.shape[1:]))
    style = q["style"]
    if mutant == "style_k_s_swapped":
        style = style.reshape(Fr, K, S).transpose(0, 2, 1)                        # style[(f, k, s)] read where [(f, s, k)] is due
    return {"boxes": boxes.boxes, "projected": boxes.points, "axes": axes.points,
            "camera34": cam_m[:, :, :3, :].reshape(Fr * C, 3, 4).copy(), "render_focals": render.reshape(-1).astype(F),
            "w2o34": per_camera(obj_inv[:, :, :3, :]), "style_nks": per_camera(style.transpose(0, 2, 1)),
            "deformation_nkd": per_camera(q["deformation"].transpose(0, 2, 1)),
            "present": per_camera((q["in_scene"] != 0).astype(np.uint8))}


SETUP_FP32_OUTPUTS = ("boxes", "projected", "axes", "camera34", "render_focals", "w2o34", "style_nks", "deformation_nkd")   # the arena's order


class SetupGrad(NamedTuple):
    g_rot: np.ndarray              # (F, 3, K)
    g_tr: np.ndarray
    g_style: np.ndarray            # (F, S, K)
    g_deformation: np.ndarray      # (F, D, K)
    tol_rot: Optional[np.ndarray] = None
    tol_tr: Optional[np.ndarray] = None
    tol_style: Optional[np.ndarray] = None
    tol_deformation: Optional[np.ndarray] = None


def _camera_sum64(g, shape):
    """Sum over the cameras of (F * C, K, X) -> (F, X, K) and the bound of a C-term fp32 sum, ``(C - 1) u sum |x|``; None: zeros."""
    Fr, C, K, X = shape
    if g is None:
        return np.zeros((Fr, X, K)), np.zeros((Fr, X, K))
    g = np.asarray(g, np.float64).reshape(Fr, C, K, X)
    return g.sum(1).transpose(0, 2, 1), ((C - 1) * U * np.abs(g).sum(1)).transpose(0, 2, 1)


def scene_setup_backward_float64(frames, cameras, objects, S, D, obj_rot, obj_tr, g_w2o34, g_style_nks, g_deformation_nkd) -> SetupGrad:
    """``pr_scene_setup_backward`` in float64: the renderer's gradients summed over the cameras of a frame, permuted back to
    (frames, 3 | S | D, objects), the pose adjoint applied through the INVERSE (w2o is the inverse of the pose matrix)."""
    n = frames * objects
    rot = np.asarray(obj_rot, np.float64).reshape(frames, 3, objects).transpose(0, 2, 1).reshape(n, 3)
    tr = np.asarray(obj_tr, np.float64).reshape(frames, 3, objects).transpose(0, 2, 1).reshape(n, 3)
    gi = np.zeros((n, 4, 4))
    tol_gi = np.zeros((n, 4, 4))
    if g_w2o34 is not None:
        g = np.asarray(g_w2o34, np.float64).reshape(frames, cameras, objects, 3, 4)
        gi[:, :3, :] = g.sum(1).reshape(n, 3, 4)
        tol_gi[:, :3, :] = ((cameras - 1) * U * np.abs(g).sum(1)).reshape(n, 3, 4)    # (the camera sum's own bound enters the chain with gv)
    want = pose_backward_float64(rot, tr, None, gi, gi_err=tol_gi)
    back = lambda a: a.reshape(frames, objects, 3).transpose(0, 2, 1)
    g_style, tol_style = _camera_sum64(g_style_nks, (frames, cameras, objects, S))
    g_def, tol_def = _camera_sum64(g_deformation_nkd, (frames, cameras, objects, D))
    return SetupGrad(back(want.g_rot), back(want.g_tr), g_style, g_def, back(want.tol_rot), back(want.tol_tr), tol_style, tol_def)


def scene_setup_backward_fp32(frames, cameras, objects, S, D, obj_rot, obj_tr, g_w2o34, g_style_nks, g_deformation_nkd, mutant=None) -> SetupGrad:
    """``k_scene_setup_bwd`` in ``np.float32``: camera sums in order from 0, then ``pose_backward`` with the sum as the inverse's gradient."""
    n = frames * objects
    last = cameras - 1 if mutant == "last_camera_dropped" else cameras
    rot = np.asarray(obj_rot, F).reshape(frames, 3, objects).transpose(0, 2, 1).reshape(n, 3)
    tr = np.asarray(obj_tr, F).reshape(frames, 3, objects).transpose(0, 2, 1).reshape(n, 3)

    def camera_sum(g, X):
        acc = np.zeros((frames, objects, X), F)
        if g is not None:
            g = np.asarray(g, F).reshape(frames, cameras, objects, X)
            for c in range(last):
                acc = acc + g[:, c]
        return acc
    gi = np.zeros((n, 4, 4), F)
    gi[:, :3, :] = camera_sum(g_w2o34, 12).reshape(n, 3, 4)
    got = pose_backward_fp32(rot, tr, None, gi, mutant)
    back = lambda a: a.reshape(frames, objects, 3).transpose(0, 2, 1)
    return SetupGrad(back(got.g_rot), back(got.g_tr), camera_sum(g_style_nks, S).transpose(0, 2, 1), camera_sum(g_deformation_nkd, D).transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------------------------------------
# comparisons
def ratio(got, want, tol) -> float:
    """``max |got - want| / tol`` over the elements whose reference is finite (a tolerance of 0 demands equality)."""
    got, want, tol = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(tol, np.float64)
    finite = np.isfinite(want) & np.isfinite(tol)
    if not finite.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got[finite] - want[finite])
        r = np.where(err == 0, 0.0, err / tol[finite])
    return float(np.nan_to_num(r, nan=np.inf).max())


def bit_differences(a, b) -> int:
    """Elements of two fp32 arrays that differ in bits; two NaNs count as equal (sign and payload are the processor's choice)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the tests (CPU and GPU draw the same ones)
COUNTS = (1, 63, 64, 65, 129)
ANGLE_FAMILIES = ("uniform", "zeros", "near_half_pi_x", "large_1e2", "large_1e4", "denormal")
LARGE_ANGLE_FAMILIES = ("large_1e2", "large_1e4")
TRANSLATION_FAMILIES = ("zero", "unit", "scene")
ARMS = {"both": (True, True), "matrices_only": (True, False), "inverses_only": (False, True), "neither": (False, False)}


def pose_inputs(angles: str, translations: str, count: int):
    """fp32 angles and translations, (count, 3) each.  ``uniform``: +-pi; ``zeros``; ``near_half_pi_x``: x within 1e-3 of +-pi / 2 (cos x
    about 0), y and z uniform; ``large_1e2`` / ``large_1e4``: magnitudes of 0.5 to 2 times 1e2 / 1e4 with both signs (range reduction
    matters); ``denormal``: magnitudes of 1e-45 to 1e-39.  Translations: zero, about 1, about 60 (the workload's scenes)."""
    rng = np.random.default_rng([ANGLE_FAMILIES.index(angles), TRANSLATION_FAMILIES.index(translations), count])
    sign = lambda: rng.choice([-1.0, 1.0], (count, 3))
    if angles == "uniform":
        rot = rng.uniform(-np.pi, np.pi, (count, 3))
    elif angles == "zeros":
        rot = np.zeros((count, 3))
    elif angles == "near_half_pi_x":
        rot = rng.uniform(-np.pi, np.pi, (count, 3))
        rot[:, 0] = sign()[:, 0] * (np.pi / 2) + rng.uniform(-1e-3, 1e-3, count)
    elif angles in LARGE_ANGLE_FAMILIES:
        rot = sign() * rng.uniform(0.5, 2.0, (count, 3)) * float(angles[6:])
    elif angles == "denormal":
        rot = sign() * 10.0 ** rng.uniform(-45, -39, (count, 3))
    else:
        raise ValueError(angles)
    scale = {"zero": 0.0, "unit": 1.0, "scene": 60.0}[translations]
    return rot.astype(F), (rng.normal(size=(count, 3)) * scale).astype(F)


def pose_gradients(count: int, seed: int = 0):
    """Incoming gradients of the matrix and of the inverse, (count, 4, 4) fp32 each: normal draws scaled by 1e-2 to 10 per element,
    bottom rows zero (the kernel does not read them; the GPU test fills them with large values to show it)."""
    rng = np.random.default_rng([77, count, seed])
    out = []
    for _ in range(2):
        g = (rng.normal(size=(count, 4, 4)) * 10.0 ** rng.uniform(-2, 1, (count, 4, 4))).astype(F)
        g[:, 3, :] = 0
        out.append(g)
    return out


def trig_angles():
    """Every angle the pose tests draw, with the family of each: where ``TRIG_ERR`` is measured."""
    angles, family = [], []
    for k, fam in enumerate(ANGLE_FAMILIES):
        for t in TRANSLATION_FAMILIES:
            for n in COUNTS:
                a = pose_inputs(fam, t, n)[0].reshape(-1)
                angles.append(a)
                family.append(np.full(a.size, k))
    return np.concatenate(angles), np.concatenate(family)


@functools.lru_cache(maxsize=None)
def fast_trig_floor() -> float:
    """The smallest, over the large-angle families, of the largest error the fast intrinsic shows on the family's angles."""
    angles, family = trig_angles()
    floors = []
    for fam in LARGE_ANGLE_FAMILIES:
        a = angles[family == ANGLE_FAMILIES.index(fam)]
        c, s = fast_trig(a)
        floors.append(max(np.abs(c - np.cos(a.astype(np.float64))).max(), np.abs(s - np.sin(a.astype(np.float64))).max()))
    return float(min(floors))


def _rigid64(rng, angle, shift, shape):
    """Random rigid motions (shape + (4, 4)) in float64: Euler angles within +-angle, translations within +-shift."""
    n = int(np.prod(shape)) if shape else 1
    p = pose_float64(rng.uniform(-angle, angle, (n, 3)), rng.uniform(-shift, shift, (n, 3)))
    return p.m.reshape(tuple(shape) + (4, 4)), p.inv.reshape(tuple(shape) + (4, 4))


HEIGHT, WIDTH = 45, 64             # non-square, an odd height
EXTENT = 10.0                      # the size of the projected scenes
POINT_COUNTS = (1, 8, 63, 64, 65, 130)
PROJECTION_SHAPES = tuple((f, c, k) for f in (1, 3) for c in (1, 2) for k in (1, 3, 8))      # (frames, cameras, objects)
BEHIND_SHARE = 0.25


def projection_inputs(frames: int, cameras: int, objects: int, points: int):
    """Inputs of ``pr_project_points`` built from the camera side: camera-space points of (frame 0, camera 0) with depths |z| from 0.1
    to 1 extent - a quarter of them behind the camera (z > 0), every point of the last object (of more than one) behind - and x, y
    INSIDE the view frustum, scaled by the depth: ``|x| <= 0.6 |z| W / (2 f)``, likewise y, so that the box edges are minima and maxima
    of coordinates strictly inside the image (what a wrong reduction changes) instead of clamped constants.  Every third object
    (1, 4, 7) has a tenth of its points - at least one - 1.2 to 2.5 times outside the frustum: the clamps are exercised there.  The
    points are mapped back to object space through float64 inverses and rounded to fp32.  The other cameras and frames are that
    camera and those object poses moved by rigid motions IN CAMERA SPACE - three Euler angles within 0.01 each (under 0.03 rad
    together), shifts within 0.01 extent per axis - and the other focal lengths are within 0.85 to 1.2 of the first.  A point at
    depth d lies within 2.2 d of the camera, so one motion changes its z by less than 0.066 d + 0.018 extent and two by less than
    0.14 d + 0.036 extent: with d >= 0.1 extent every |cam.z| stays above 0.05 extent - the ``cam.z > 0`` decision holds with margin for
    every (frame, camera, point) by construction.
    Returns ``points (K, P, 3), o2w (F, K, 4, 4), w2c (F, C, 4, 4), focals (F, C)`` as fp32 and the all-behind object (or None)."""
    rng = np.random.default_rng([frames, cameras, objects, points])
    focals = rng.uniform(0.8, 1.5) * WIDTH * rng.uniform(0.85, 1.2, (frames, cameras))
    depth = rng.uniform(0.1, 1.0, (objects, points)) * EXTENT
    reach = rng.uniform(-0.6, 0.6, (objects, points, 2))
    for k in range(1, objects, 3):
        out = rng.choice(points, max(1, points // 10), replace=False)
        reach[k, out] = rng.choice([-1.0, 1.0], (out.size, 2)) * rng.uniform(1.2, 2.5, (out.size, 2))
    cam = np.empty((objects, points, 3))
    cam[..., :2] = reach * depth[..., None] * np.array([WIDTH, HEIGHT]) / (2 * focals[0, 0])
    behind = rng.random((objects, points)) < BEHIND_SHARE
    all_behind = objects - 1 if objects > 1 else None
    if all_behind is not None:
        behind[all_behind] = True
    cam[..., 2] = np.where(behind, depth, -depth)
    c2w0, w2c0 = _rigid64(rng, np.pi, 60.0, ())
    o2w0, w2o0 = _rigid64(rng, np.pi, 60.0, (objects,))
    homogeneous = np.concatenate([cam, np.ones((objects, points, 1))], -1)
    pts = np.einsum("kab,kpb->kpa", w2o0 @ c2w0, homogeneous)[..., :3]
    move_o, _ = _rigid64(rng, 0.01, 0.01 * EXTENT, (frames,))
    move_c, _ = _rigid64(rng, 0.01, 0.01 * EXTENT, (frames, cameras))
    move_o[0], move_c[0, 0] = np.eye(4), np.eye(4)
    o2w = np.einsum("ab,fbc,cd,kde->fkae", c2w0, move_o, w2c0, o2w0)
    w2c = move_c @ w2c0
    return pts.astype(F), o2w.astype(F), w2c.astype(F), focals.astype(F), all_behind


def unsaturated_share(boxes) -> float:
    """The share of box edges strictly between 0 and 1: edges that are a minimum or maximum of projected coordinates, not a clamp."""
    boxes = np.asarray(boxes)
    return float(((boxes > 0) & (boxes < 1)).mean())


def degenerate_projection_inputs():
    """Identity matrices and the axes points - (0, 0, 0) and (1, 0, 0) among them: ``cam.z == 0`` exactly for three of the four, the
    divisions yield NaN, -inf and +inf; the fourth lies behind the camera (z = 1)."""
    pts = np.array([[(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]], F)
    eye = np.eye(4, dtype=F)
    return pts, eye.reshape(1, 1, 4, 4).copy(), eye.reshape(1, 1, 4, 4).copy(), np.array([[48.0]], F)


RAY_HEIGHT, RAY_WIDTH = 45, 63     # both odd: half_h and half_w are true divisions
RAY_SHAPES = ((1, 1), (1, 255), (3, 85), (1, 256), (2, 128), (1, 257), (3, 171))          # frames x rays in {1, 255, 256, 257, 513}


def ray_inputs(frames: int, rays: int, per_frame: bool):
    """``c2w (N, 3, 4)``, focals (N), pixel rows / columns (R) or per frame (N, R), different from frame to frame: indices from 8 pixels
    outside the image on every side (the patch sampler's alignment produces negative and too-large ones)."""
    rng = np.random.default_rng([frames, rays, int(per_frame)])
    c2w = _rigid64(rng, np.pi, 60.0, (frames,))[0][:, :3, :].astype(F)
    focals = (rng.uniform(0.8, 1.5, frames) * RAY_WIDTH).astype(F)
    shape = (frames, rays) if per_frame else (rays,)
    rows = rng.integers(-8, RAY_HEIGHT + 8, shape).astype(np.int32)
    cols = rng.integers(-8, RAY_WIDTH + 8, shape).astype(np.int32)
    rows.reshape(-1)[0], cols.reshape(-1)[0] = -8, RAY_WIDTH + 7
    return c2w, focals, rows, cols


SETUP_SHAPES = ((1, 1, 1), (2, 2, 3), (3, 1, 8))           # (frames, cameras, objects)
SETUP_FEATURES = ((0, 0), (1, 37), (64, 64))               # (S, D): 8 x 64 = 512 elements exceed a 256-thread pass
SETUP_POINTS = (8, 68)


def setup_inputs(frames, cameras, objects, S, D, points, upsample=1.0, axes_with_upsampled_focals=0):
    """Inputs of ``pr_scene_setup`` in the scene tensors' layouts, as a dictionary (sizes and switches included); about a third of the
    objects absent.  The objects stand IN VIEW of their frame's first camera - centres 12 to 20 in front of it, within 0.2 / 0.12 of
    the depth sideways / upwards, box points within 1 of the centre, focal lengths short enough for the upsampled render focal - so that
    the boxes are minima and maxima of coordinates inside the image, not clamped constants; object 1 (of more than one) stands
    0.6 of its depth to the side, where the clamps act at the upsampled focal.  Further cameras of a frame are the first one moved a little."""
    rng = np.random.default_rng([frames, cameras, objects, S, D, points])
    f32 = lambda a: np.ascontiguousarray(a, F)
    cam_rot = np.repeat(rng.uniform(-np.pi, np.pi, (frames, 1, 3)), cameras, 1)
    cam_tr = np.repeat(rng.normal(size=(frames, 1, 3)) * 20.0, cameras, 1)
    cam_rot[:, 1:] += rng.uniform(-0.03, 0.03, (frames, cameras - 1, 3))
    cam_tr[:, 1:] += rng.uniform(-0.3, 0.3, (frames, cameras - 1, 3))
    cam_rot, cam_tr = f32(cam_rot), f32(cam_tr)
    depth = rng.uniform(12.0, 20.0, (frames, objects))
    centre = np.stack([rng.uniform(-0.2, 0.2, (frames, objects)) * depth, rng.uniform(-0.12, 0.12, (frames, objects)) * depth, -depth,
                       np.ones((frames, objects))], -1)
    if objects > 1:
        centre[:, 1, 0] = 0.6 * depth[:, 1]
    c2w = pose_float64(cam_rot[:, 0], cam_tr[:, 0]).m                                          # (F, 4, 4)
    obj_tr = np.einsum("fab,fkb->fak", c2w, centre)[:, :3, :]                                 # (F, 3, K)
    return {
        "frames": frames, "cameras": cameras, "objects": objects, "S": S, "D": D, "points": points, "height": HEIGHT, "width": WIDTH,
        "focal_multiplier": 0.75, "upsample": float(upsample), "axes_with_upsampled_focals": int(axes_with_upsampled_focals),
        "cam_rot": cam_rot, "cam_tr": cam_tr, "focals": f32(rng.uniform(0.5, 0.8, (frames, cameras)) * WIDTH),
        "obj_rot": f32(rng.uniform(-np.pi, np.pi, (frames, 3, objects))), "obj_tr": f32(obj_tr),
        "style": f32(rng.normal(size=(frames, S, objects))), "deformation": f32(rng.normal(size=(frames, D, objects))),
        "in_scene": (rng.random((frames, objects)) > 0.35).astype(np.uint8),
        "box_points": f32(rng.uniform(-1.0, 1.0, (objects, points, 3))),
        "axes_points": f32(np.tile(np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]), (objects, 1, 1))),
    }


def setup_pose_rows(q):
    """The poses of ``setup_inputs`` as ``pr_pose_matrices`` takes them: cameras (F * C, 3) and objects (F * K, 3) in (frame, object) order."""
    Fr, C, K = q["frames"], q["cameras"], q["objects"]
    rows = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1).reshape(Fr * K, 3))
    return q["cam_rot"].reshape(Fr * C, 3), q["cam_tr"].reshape(Fr * C, 3), rows(q["obj_rot"]), rows(q["obj_tr"])


def setup_gradients(frames, cameras, objects, S, D):
    """The renderer's gradients in its layouts, (F * C, K, 12 | S | D) fp32, with magnitudes that differ per camera (x 10 per camera)."""
    rng = np.random.default_rng([5, frames, cameras, objects, S, D])
    scale = (10.0 ** np.arange(cameras))[None, :, None, None]
    draw = lambda X: (rng.normal(size=(frames, cameras, objects, X)) * scale).astype(F).reshape(frames * cameras, objects, X)
    return draw(12), draw(S), draw(D)


def setup_backward_poses(frames, objects):
    rng = np.random.default_rng([6, frames, objects])
    return (rng.uniform(-np.pi, np.pi, (frames, 3, objects)).astype(F), (rng.normal(size=(frames, 3, objects)) * 20.0).astype(F))
