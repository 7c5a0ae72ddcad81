"""The scene set-up kernels of csrc/geometry.hip on the GPU (python -m pytest tests -m gpu), straight through the C ABI: ``pr_pose_matrices``,
``pr_pose_matrices_backward``, ``pr_project_points``, ``pr_camera_rays``, ``pr_scene_setup`` and ``pr_scene_setup_backward`` against the float64
restatements of tests/scene_reference.py within the tolerances derived there and, where the kernel is written with explicit
round-to-nearest operations only (projection, rays, the copies of the fused set-up), against the fp32 restatements bit for bit.  Every
input and every output lives in a NaN-poisoned allocation of its own with guard words on both sides (tests/poisoned.py); after EVERY call
every guard must be intact and every input unchanged bit for bit.  The fused set-up additionally writes into one arena packed as
``EnvironmentModel._scene_setup`` packs it, and must give the bits it gives into separate allocations.  The NULL arms - absent incoming
gradients, unwanted outputs, ``boxes = NULL`` - are called in every combination the argument checks allow.

Measured on an MI355X over the 1 967 calls of this module in one run (``_report`` prints them with ``pytest -s``; diagnostics, never
asserted).  Worst error / tolerance: ``m`` 0.302, ``inv`` 0.302, ``g_rot`` 0.230, ``g_tr`` 0.812 of ``pr_pose_matrices`` and its backward; projected
points 0.411 and boxes 0.230 of the float64 bound (and 0 bits off the fp32 restatement); ray directions 0.471; ``g_rot`` 0.196, ``g_tr`` 0.166,
``g_style`` 0.965 and ``g_deformation`` 0.953 of ``pr_scene_setup_backward``.  The fp32 restatements on the CPU give nearly the same figures on the same
inputs (0.302, 0.302, 0.224, 0.812; 0.411, 0.230; 0.196, 0.163, 0.965, 0.953), so the ratios near 1 are what honest fp32 arithmetic uses of
the bounds, not the kernels': the bound of a two-camera sum is ONE rounding, ``u |sum| <= u sum |x|``, which some of the sums all but
attain, and ``g_tr = gM[:, 3] - R gu`` ends in one subtraction whose rounding on ``|gM| + |R gu|`` is most of its bound (0.71 where the angles
are 0 and the trigonometry is exact).  ``sinf / cosf`` seen through the kernel: 6.541e-08 at most (the same at the large angles; the
fast-intrinsic floor is 1.372e-05), hence ``TRIG_ERR = 1.31e-07``.  Bits differing from the fp32 pose restatements (numpy's sine and
cosine are not the device's): 10 592 of 185 472 values of ``m, inv``, 11 915 of 156 960 of ``g_rot, g_tr``."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib
from tests import scene_reference as sr
from tests.helpers import projection_tensor_formulation as tensor_formulation
from tests.poisoned import Placed

pytestmark = pytest.mark.gpu

F = np.float32
# The largest error / tolerance per output family over every call of this module, and the elements whose bits differ from the fp32 pose
# restatements (the device's sinf / cosf are not numpy's: a diagnostic that is never asserted).
WORST = {k: 0.0 for k in ("pose_m", "pose_inv", "g_rot", "g_tr", "projected_points", "boxes", "ray_directions", "setup_g_rot", "setup_g_tr",
                          "setup_g_style", "setup_g_deformation")}
COUNT = {"calls": 0, "pose_bit_differences": 0, "pose_elements": 0, "pose_backward_bit_differences": 0, "pose_backward_elements": 0, "trig_error": 0.0,
         "trig_error_large": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the scene set-up kernels have no CPU fallback")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\nscene set-up kernels, {COUNT['calls']} calls: worst error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    print(f"sinf / cosf through pr_pose_matrices: largest error {COUNT['trig_error']:.3e} (large angles {COUNT['trig_error_large']:.3e}; TRIG_ERR "
          f"{sr.TRIG_ERR:.3e}, fast-intrinsic floor {sr.fast_trig_floor():.3e}); bits differing from the fp32 restatements: pose "
          f"{COUNT['pose_bit_differences']} of {COUNT['pose_elements']}, pose backward {COUNT['pose_backward_bit_differences']} of "
          f"{COUNT['pose_backward_elements']}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(x):
    return None if x is None else x.pointer


def _done(status, name, inputs):
    """After every call: the status, the queue drained, every input unchanged (``read`` inside checks its guards)."""
    _lib.check(status, name)
    torch.cuda.synchronize()
    COUNT["calls"] += 1
    for what, placed in inputs.items():
        if placed is not None:
            placed.unchanged(f"{name}: {what}")


def _worst(key, got, want, tol):
    r = sr.ratio(got, want, tol)
    WORST[key] = max(WORST[key], r)
    return r


def same_bits(a, b, what):
    differ = sr.bit_differences(a, b)
    assert differ == 0, f"{what}: {differ} of {np.size(a)} elements differ in bits, first at {np.flatnonzero(np.ravel(np.asarray(a, F).view(np.uint32) != np.asarray(b, F).view(np.uint32)))[:4]}"


# ---------------------------------------------------------------------------------------------------------------------
# pr_pose_matrices
def device_pose(rot, tr):
    rot, tr = np.asarray(rot, F).reshape(-1, 3), np.asarray(tr, F).reshape(-1, 3)
    n = rot.shape[0]
    R, T = Placed(rot), Placed(tr)
    M, V = Placed.poisoned(n * 16), Placed.poisoned(n * 16)
    _done(_lib.load().pr_pose_matrices(n, R.pointer, T.pointer, M.pointer, V.pointer, _stream()), "pr_pose_matrices", {"rotations": R, "translations": T})
    return sr.Pose(M.read("matrices").reshape(n, 4, 4), V.read("inverses").reshape(n, 4, 4))


@functools.lru_cache(maxsize=None)
def _pose_case(angles, translations, count):
    rot, tr = sr.pose_inputs(angles, translations, count)
    return rot, tr, sr.pose_float64(rot, tr), sr.pose_fp32(rot, tr)


def check_pose(got, rot, tr, want, what, rows=slice(None)):
    r = (_worst("pose_m", got.m[rows], want.m[rows], want.tol_m[rows]), _worst("pose_inv", got.inv[rows], want.inv[rows], want.tol_inv[rows]))
    assert np.isfinite(got.m[rows]).all() and np.isfinite(got.inv[rows]).all(), what
    assert max(r) <= 1.0, f"{what}: error / tolerance (m, inv) = {r}"
    bottom = np.array([0, 0, 0, 1], F)
    assert (got.m[:, 3, :] == bottom).all() and (got.inv[:, 3, :] == bottom).all(), f"{what}: bottom rows"
    same_bits(got.m[:, :3, 3], tr, f"{what}: m[:3, 3] against t")


@pytest.mark.parametrize("translations", sr.TRANSLATION_FAMILIES)
@pytest.mark.parametrize("angles", sr.ANGLE_FAMILIES)
def test_pose_matrices(angles, translations):
    """``m`` and ``inv`` within ``tol_*`` per element at counts around a 64-thread block, on every angle and translation family; the bottom
    rows are exactly ``0 0 0 1``, ``m[:3, 3]`` is ``t`` bit for bit, and a second call gives the same bits."""
    for count in sr.COUNTS:
        rot, tr, want, fp32 = _pose_case(angles, translations, count)
        got = device_pose(rot, tr)
        check_pose(got, rot, tr, want, f"{angles} {translations} {count}")
        COUNT["pose_bit_differences"] += sr.bit_differences(got.m, fp32.m) + sr.bit_differences(got.inv, fp32.inv)
        COUNT["pose_elements"] += 2 * got.m.size
        again = device_pose(rot, tr)
        same_bits(got.m, again.m, "m from call to call")
        same_bits(got.inv, again.inv, "inv from call to call")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_pose_matrices_non_finite_stays_in_its_matrix(bad):
    """A NaN or infinite angle or translation in one matrix (in the first and in the second block) leaves every other matrix finite
    and inside tolerance, and shows in its own."""
    for column in range(6):
        for victim in (3, 64):
            rot, tr = (a.copy() for a in sr.pose_inputs("uniform", "scene", 65))
            (rot if column < 3 else tr)[victim, column % 3] = bad
            got = device_pose(rot, tr)
            others = np.arange(65) != victim
            check_pose(got, rot, tr, sr.pose_float64(rot, tr), f"{bad} in column {column} of matrix {victim}", others)
            assert not (np.isfinite(got.m[victim]).all() and np.isfinite(got.inv[victim]).all())


def test_trig_error_measured_through_the_kernel():
    """``TRIG_ERR`` is twice the largest error of ``sinf / cosf`` as seen THROUGH the kernel on single-axis rotations (the other factors are 0
    and 1: products and sums are exact), over every angle the tests draw; and the error at the large angles stays below what a
    range-reduction-free intrinsic shows there, so that a wrong trig call cannot have widened its own tolerance."""
    angles, family = sr.trig_angles()
    a64 = angles.astype(np.float64)
    n = angles.size
    worst = np.zeros(n)
    for axis, (cos_at, sin_at) in enumerate((((1, 1), (2, 1)), ((0, 0), (0, 2)), ((0, 0), (1, 0)))):
        rot = np.zeros((n, 3), F)
        rot[:, axis] = angles
        r = device_pose(rot, np.zeros((n, 3), F)).m[:, :3, :3]
        worst = np.maximum(worst, np.abs(r[:, cos_at[0], cos_at[1]] - np.cos(a64)))
        worst = np.maximum(worst, np.abs(r[:, sin_at[0], sin_at[1]] - np.sin(a64)))
        # what makes the reading exact: the rotation holds that cosine and that sine, their copies, a 1 on the axis and zeros
        i, j = [k for k in range(3) if k != axis]
        assert (r[:, i, i] == r[:, j, j]).all() and (r[:, i, j] == -r[:, j, i]).all()
        rest = r.copy()
        rest[:, [i, i, j, j], [i, j, i, j]] = 0
        expected = np.zeros((3, 3), F)
        expected[axis, axis] = 1
        assert (rest == expected).all()
    large = np.isin(family, [sr.ANGLE_FAMILIES.index(f) for f in sr.LARGE_ANGLE_FAMILIES])
    COUNT["trig_error"], COUNT["trig_error_large"] = float(worst.max()), float(worst[large].max())
    print(f"\nsinf / cosf through the kernel: largest error {worst.max():.4e}, at the large angles {worst[large].max():.4e}; per family "
          + ", ".join(f"{f} {worst[family == k].max():.3e}" for k, f in enumerate(sr.ANGLE_FAMILIES)))
    assert 2 * worst.max() <= sr.TRIG_ERR, (worst.max(), sr.TRIG_ERR)
    assert worst[large].max() < sr.fast_trig_floor() and sr.TRIG_ERR < sr.fast_trig_floor(), (worst[large].max(), sr.fast_trig_floor())


def test_empty_calls_write_nothing():
    """``count == 0`` and ``frames == 0`` are no-ops: outputs that are passed all the same stay poisoned, guards included."""
    lib = _lib.load()
    rot, tr = sr.pose_inputs("uniform", "unit", 1)
    R, T = Placed(rot), Placed(tr)
    outputs = [Placed.poisoned(16) for _ in range(4)]
    a, b, c, d = (o.pointer for o in outputs)
    _done(lib.pr_pose_matrices(0, R.pointer, T.pointer, a, b, _stream()), "pr_pose_matrices", {"rotations": R, "translations": T})
    _done(lib.pr_pose_matrices_backward(0, R.pointer, T.pointer, a, b, c, d, _stream()), "pr_pose_matrices_backward", {})
    _done(lib.pr_project_points(0, 1, 1, 1, R.pointer, a, b, T.pointer, sr.HEIGHT, sr.WIDTH, c, d, _stream()), "pr_project_points", {})
    _done(lib.pr_scene_setup_backward(0, 1, 1, 1, 1, R.pointer, T.pointer, None, None, None, a, b, c, d, _stream()), "pr_scene_setup_backward", {})
    for o in outputs:
        o.unchanged("an output of an empty call")


# ---------------------------------------------------------------------------------------------------------------------
# pr_pose_matrices_backward
def device_pose_backward(rot, tr, gm, gi):
    n = rot.shape[0]
    R, T = Placed(rot), Placed(tr)
    GM, GI = (None if g is None else Placed(g) for g in (gm, gi))
    GR, GT = Placed.poisoned(n * 3), Placed.poisoned(n * 3)
    _done(_lib.load().pr_pose_matrices_backward(n, R.pointer, T.pointer, _ptr(GM), _ptr(GI), GR.pointer, GT.pointer, _stream()),
          "pr_pose_matrices_backward", {"rotations": R, "translations": T, "g_matrices": GM, "g_inverses": GI})
    return sr.PoseGrad(GR.read("g_rotations").reshape(n, 3), GT.read("g_translations").reshape(n, 3))


@functools.lru_cache(maxsize=None)
def _pose_backward_case(angles, translations, count, arm):
    rot, tr = sr.pose_inputs(angles, translations, count)
    gm, gi = (g if wanted else None for g, wanted in zip(sr.pose_gradients(count), sr.ARMS[arm]))
    return rot, tr, gm, gi, sr.pose_backward_float64(rot, tr, gm, gi), sr.pose_backward_fp32(rot, tr, gm, gi)


@pytest.mark.parametrize("arm", list(sr.ARMS))
@pytest.mark.parametrize("angles", sr.ANGLE_FAMILIES)
def test_pose_matrices_backward(angles, arm):
    """``g_rot`` and ``g_tr`` within ``tol_*`` PER ELEMENT (not relative to the tensor's maximum) with both incoming gradients, either alone
    and neither (exact zeros), on every family and count.  The bottom rows of the incoming gradients hold 1e30: the kernel must not
    read them - the result is bit for bit the one with zeros there."""
    for translations in sr.TRANSLATION_FAMILIES:
        for count in sr.COUNTS:
            rot, tr, gm, gi, want, fp32 = _pose_backward_case(angles, translations, count, arm)
            loud = [None if g is None else g.copy() for g in (gm, gi)]
            for g in loud:
                if g is not None:
                    g[:, 3, :] = 1e30
            got = device_pose_backward(rot, tr, *loud)
            what = f"{angles} {translations} {count} {arm}"
            r = (_worst("g_rot", got.g_rot, want.g_rot, want.tol_rot), _worst("g_tr", got.g_tr, want.g_tr, want.tol_tr))
            assert np.isfinite(got.g_rot).all() and np.isfinite(got.g_tr).all(), what
            assert max(r) <= 1.0, f"{what}: error / tolerance (g_rot, g_tr) = {r}"
            COUNT["pose_backward_bit_differences"] += sr.bit_differences(got.g_rot, fp32.g_rot) + sr.bit_differences(got.g_tr, fp32.g_tr)
            COUNT["pose_backward_elements"] += 2 * got.g_rot.size
            quiet = device_pose_backward(rot, tr, gm, gi)
            same_bits(got.g_rot, quiet.g_rot, f"{what}: g_rot with loud bottom rows")
            same_bits(got.g_tr, quiet.g_tr, f"{what}: g_tr with loud bottom rows")
            if arm == "neither":
                assert (got.g_rot == 0).all() and (got.g_tr == 0).all(), what


# ---------------------------------------------------------------------------------------------------------------------
# pr_project_points
def device_project(pts, o2w, w2c, focals, height, width, boxes):
    Fr, C, K, P = o2w.shape[0], w2c.shape[1], pts.shape[0], pts.shape[1]
    inputs = {"points": Placed(pts), "o2w": Placed(o2w), "w2c": Placed(w2c), "focals": Placed(focals)}
    out = Placed.poisoned(Fr * C * P * 2 * K)
    box = Placed.poisoned(Fr * C * 4 * K) if boxes else None
    _done(_lib.load().pr_project_points(Fr, C, K, P, inputs["points"].pointer, inputs["o2w"].pointer, inputs["w2c"].pointer, inputs["focals"].pointer,
                                        height, width, out.pointer, _ptr(box), _stream()), "pr_project_points", inputs)
    return out.read("projected").reshape(Fr, C, P, 2, K), None if box is None else box.read("boxes").reshape(Fr, C, 4, K)


@pytest.mark.parametrize("boxes", [True, False], ids=["boxes", "axes"])
@pytest.mark.parametrize("points", sr.POINT_COUNTS)
def test_project_points(points, boxes):
    """Points and boxes bit for bit the fp32 restatement and within the float64 bound, with 1 to 130 points per object (a wave is 64), 1 / 3 /
    8 objects, 1 / 2 cameras and 1 / 3 frames on a 45 x 64 image; every point counts (the inputs keep |cam.z| away from 0 by
    construction).  An object entirely behind the camera gives the box [1, 1, 0, 0]; coordinates outside the image are clamped with
    ``boxes`` and left as they are without."""
    outside = 0
    for frames, cameras, objects in sr.PROJECTION_SHAPES:
        pts, o2w, w2c, focals, all_behind = sr.projection_inputs(frames, cameras, objects, points)
        got_points, got_boxes = device_project(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
        fp32 = sr.project_fp32(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
        want = sr.project_float64(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
        what = f"{frames} frames {cameras} cameras {objects} objects {points} points"
        same_bits(got_points, fp32.points, f"{what}: projected points")
        assert np.isfinite(got_points).all(), what
        r = _worst("projected_points", got_points, want.points, want.tol_points)
        assert r <= 1.0, f"{what}: points error / tolerance {r}"
        if boxes:
            same_bits(got_boxes, fp32.boxes, f"{what}: boxes")
            r = _worst("boxes", got_boxes, want.boxes, want.tol_boxes)
            assert r <= 1.0, f"{what}: boxes error / tolerance {r}"
            assert got_points.min() >= 0 and got_points.max() <= 1 and got_boxes.min() >= 0 and got_boxes.max() <= 1
            if all_behind is not None:
                assert (got_boxes[:, :, :, all_behind] == np.array([1, 1, 0, 0], F)[None, None, :]).all(), what
            outside += int(((want.points == 0) | (want.points == 1)).sum())
        else:
            outside += int(((got_points < 0) | (got_points > 1)).sum())
    assert outside > 0          # (clamped coordinates with boxes, coordinates outside [0, 1] without: the inputs reach outside the image)


@pytest.mark.parametrize("boxes", [True, False], ids=["boxes", "axes"])
def test_project_points_where_cam_z_is_zero(boxes):
    """Identity matrices and the points (0, 0, 0) and (1, 0, 0): ``cam.z == 0`` exactly, the division yields NaN and -inf.  The tensor
    formulation is the contract: ``torch.min / max / clamp`` keep a NaN, so the kernel's reductions and clamps keep it too (with
    ``fminf / fmaxf``, which drop a NaN, the restatement gives the finite box [0, 1, 0, 1] and 0 for the NaN coordinates)."""
    pts, o2w, w2c, focals = sr.degenerate_projection_inputs()
    got_points, got_boxes = device_project(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
    on_device = lambda a: torch.from_numpy(a).cuda()
    want_points, want_boxes = tensor_formulation(on_device(pts), on_device(o2w), on_device(w2c), on_device(focals), sr.HEIGHT, sr.WIDTH, boxes)
    same_bits(got_points, want_points.cpu().numpy(), "points against the tensor formulation")
    fp32 = sr.project_fp32(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
    same_bits(got_points, fp32.points, "points against the fp32 restatement")
    assert np.isnan(got_points).any()
    if boxes:
        same_bits(got_boxes, want_boxes.cpu().numpy(), "box against the tensor formulation")
        same_bits(got_boxes, fp32.boxes, "box against the fp32 restatement")
        assert np.isnan(got_boxes).all()


# ---------------------------------------------------------------------------------------------------------------------
# pr_camera_rays
@pytest.mark.parametrize("per_frame", [False, True], ids=["shared_pixels", "per_frame_pixels"])
@pytest.mark.parametrize("shape", sr.RAY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_camera_rays(shape, per_frame):
    """Directions bit for bit the fp32 restatement with ``frames * rays`` at the seams of a 256-thread block (1, 255, 256, 257, 3 x 171: a
    frame boundary inside a block), shared and per-frame pixel lists (different per frame), an odd height and width, negative and
    too-large pixel indices; origins are ``c2w[:, 3]`` and normals ``-c2w[:, 2]`` bit for bit for EVERY frame (one lane writes them)."""
    frames, rays = shape
    c2w, focals, rows, cols = sr.ray_inputs(frames, rays, per_frame)
    inputs = {"c2w": Placed(c2w), "focals": Placed(focals), "rows": Placed(rows, dtype=np.int32), "cols": Placed(cols, dtype=np.int32)}
    origins, directions, normals = Placed.poisoned(frames * 3), Placed.poisoned(frames * rays * 3), Placed.poisoned(frames * 3)
    _done(_lib.load().pr_camera_rays(frames, rays, sr.RAY_HEIGHT, sr.RAY_WIDTH, int(per_frame), inputs["c2w"].pointer, inputs["focals"].pointer,
                                     inputs["rows"].pointer, inputs["cols"].pointer, origins.pointer, directions.pointer, normals.pointer, _stream()),
          "pr_camera_rays", inputs)
    fp32 = sr.camera_rays_fp32(c2w, focals, rows, cols, sr.RAY_HEIGHT, sr.RAY_WIDTH, per_frame)
    want = sr.camera_rays_float64(c2w, focals, rows, cols, sr.RAY_HEIGHT, sr.RAY_WIDTH, per_frame)
    got = directions.read("ray_directions").reshape(frames, rays, 3)
    same_bits(got, fp32.directions, "directions")
    assert _worst("ray_directions", got, want.directions, want.tol_directions) <= 1.0
    same_bits(origins.read("ray_origins").reshape(frames, 3), c2w[:, :, 3], "origins")
    same_bits(normals.read("focal_normals").reshape(frames, 3), -c2w[:, :, 2], "normals")


# ---------------------------------------------------------------------------------------------------------------------
# pr_scene_setup
def _setup_sizes(q):
    n, K, P, S, D = q["frames"] * q["cameras"], q["objects"], q["points"], q["S"], q["D"]
    return dict(zip(sr.SETUP_FP32_OUTPUTS, (n * 4 * K, n * P * 2 * K, n * 8 * K, n * 12, n, n * K * 12, n * K * S, n * K * D)))


def device_scene_setup(q, arena):
    """One ``pr_scene_setup``; the fp32 outputs in ONE poisoned arena, packed back to back in ``EnvironmentModel._scene_setup``'s order with
    guards only at its ends (``arena``), or each in an allocation of its own."""
    sizes = _setup_sizes(q)
    names = ("cam_rot", "cam_tr", "focals", "obj_rot", "obj_tr", "style", "deformation", "box_points", "axes_points")
    inputs = {k: Placed(q[k]) for k in names}
    inputs["in_scene"] = Placed(q["in_scene"], dtype=np.uint8)
    present = Placed.poisoned(q["frames"] * q["cameras"] * q["objects"], np.uint8)
    if arena:
        whole = Placed.poisoned(sum(sizes.values()))
        offsets = dict(zip(sizes, np.cumsum([0] + list(sizes.values())[:-1])))
        pointer = {k: whole.pointer + 4 * int(offsets[k]) for k in sizes}
    else:
        separate = {k: Placed.poisoned(v) for k, v in sizes.items()}
        pointer = {k: v.pointer for k, v in separate.items()}
    s = _lib.SceneSetup()
    s.frames, s.cameras, s.objects, s.box_points_per_object = q["frames"], q["cameras"], q["objects"], q["points"]
    s.style_features, s.deformation_features, s.height, s.width = q["S"], q["D"], q["height"], q["width"]
    s.focal_multiplier, s.upsample_factor, s.axes_with_upsampled_focals = q["focal_multiplier"], q["upsample"], q["axes_with_upsampled_focals"]
    s.camera_rotations, s.camera_translations, s.focals = inputs["cam_rot"].pointer, inputs["cam_tr"].pointer, inputs["focals"].pointer
    s.object_rotations, s.object_translations = inputs["obj_rot"].pointer, inputs["obj_tr"].pointer
    s.style, s.deformation, s.object_in_scene = inputs["style"].pointer, inputs["deformation"].pointer, inputs["in_scene"].pointer
    s.box_points, s.axes_points = inputs["box_points"].pointer, inputs["axes_points"].pointer
    s.boxes, s.projected_points, s.axes = pointer["boxes"], pointer["projected"], pointer["axes"]
    s.camera34, s.render_focals = pointer["camera34"], pointer["render_focals"]
    s.w2o34, s.style_nks, s.deformation_nkd, s.present = pointer["w2o34"], pointer["style_nks"], pointer["deformation_nkd"], present.pointer
    _done(_lib.load().pr_scene_setup(C.byref(s), _stream()), "pr_scene_setup", inputs)
    if arena:
        flat = whole.read("arena")
        out = {k: flat[int(offsets[k]):int(offsets[k]) + sizes[k]] for k in sizes}
    else:
        out = {k: v.read(k) for k, v in separate.items()}
    out["present"] = present.read("present")
    return out


@pytest.mark.parametrize("features", sr.SETUP_FEATURES, ids=lambda f: f"S{f[0]}_D{f[1]}")
@pytest.mark.parametrize("shape", sr.SETUP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scene_setup(shape, features):
    """The fused set-up against ``pr_pose_matrices`` run through the C ABI on the same poses: ``camera34`` and ``w2o34`` are its rows bit for
    bit (``w2o34`` once per camera), ``render_focals``, the boxes, the projected points and the axes are the fp32 restatement fed those
    device matrices bit for bit, ``style_nks``, ``deformation_nkd`` and ``present`` are the permuted inputs exactly - with 8 and 68 box points,
    both upsample factors and both focal choices of the axes, some objects absent, and 8 x 64 = 512 feature elements (two passes of the
    block).  Into one arena packed like ``_scene_setup``'s and into separate allocations the kernel writes the same values."""
    for points, upsample, flag in itertools.product(sr.SETUP_POINTS, (1.0, 2.0), (0, 1)):
        q = sr.setup_inputs(*shape, *features, points, upsample, flag)
        cam_rot, cam_tr, obj_rot, obj_tr = sr.setup_pose_rows(q)
        cam, obj = device_pose(cam_rot, cam_tr), device_pose(obj_rot, obj_tr)
        want = sr.scene_setup_fp32(q, cam.m, cam.inv, obj.m, obj.inv)
        packed, apart = device_scene_setup(q, arena=True), device_scene_setup(q, arena=False)
        what = f"{shape} {features} {points} points, upsample {upsample}, axes flag {flag}"
        for key in sr.SETUP_FP32_OUTPUTS:
            same_bits(apart[key], want[key].reshape(-1), f"{what}: {key}")
            same_bits(packed[key], apart[key], f"{what}: {key} in the arena against its own allocation")
        assert np.array_equal(apart["present"], want["present"].reshape(-1)) and np.array_equal(packed["present"], apart["present"]), what
        assert not q["in_scene"].all() or q["objects"] == 1           # (some objects absent)


# ---------------------------------------------------------------------------------------------------------------------
# pr_scene_setup_backward
@functools.lru_cache(maxsize=None)
def _setup_backward_case(shape, features, given):
    frames, cameras, objects = shape
    rot, tr = sr.setup_backward_poses(frames, objects)
    grads = tuple(g if wanted else None for g, wanted in zip(sr.setup_gradients(*shape, *features), given))
    return (rot, tr, grads, sr.scene_setup_backward_float64(*shape, *features, rot, tr, *grads),
            sr.scene_setup_backward_fp32(*shape, *features, rot, tr, *grads))


@pytest.mark.parametrize("features", sr.SETUP_FEATURES, ids=lambda f: f"S{f[0]}_D{f[1]}")
@pytest.mark.parametrize("shape", sr.SETUP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scene_setup_backward(shape, features):
    """Every combination of absent incoming gradients (``g_w2o34``, ``g_style_nks``, ``g_deformation_nkd``) and unwanted outputs (the pose pair,
    ``g_style``, ``g_deformation``) that the argument check allows, with incoming gradients ten times larger per camera: ``g_style`` and
    ``g_deformation`` within the bound of a ``C``-term fp32 sum of the float64 sum (one camera: equal), ``g_rot`` and ``g_tr`` within ``tol_*`` of
    the float64 adjoint through the inverse, an absent incoming gradient gives exact zeros.  An unwanted output is a NULL pointer - the ABI
    has no other way to switch one off -, so there is no buffer that could stay poisoned; buffers that are passed and must stay poisoned
    are those of the empty calls (``test_empty_calls_write_nothing``)."""
    frames, cameras, objects = shape
    S, D = features
    lib = _lib.load()
    for given in itertools.product((True, False), repeat=3):
        rot, tr, grads, want, fp32 = _setup_backward_case(shape, features, given)
        for wanted in itertools.product((True, False), repeat=3):
            inputs = {"object_rotations": Placed(rot), "object_translations": Placed(tr)}
            inputs.update({k: None if g is None else Placed(g) for k, g in zip(("g_w2o34", "g_style_nks", "g_deformation_nkd"), grads)})
            g_rot, g_tr = (Placed.poisoned(frames * 3 * objects) if wanted[0] else None for _ in range(2))
            g_style = Placed.poisoned(frames * S * objects) if wanted[1] else None
            g_def = Placed.poisoned(frames * D * objects) if wanted[2] else None
            _done(lib.pr_scene_setup_backward(frames, cameras, objects, S, D, inputs["object_rotations"].pointer, inputs["object_translations"].pointer,
                                              _ptr(inputs["g_w2o34"]), _ptr(inputs["g_style_nks"]), _ptr(inputs["g_deformation_nkd"]),
                                              _ptr(g_rot), _ptr(g_tr), _ptr(g_style), _ptr(g_def), _stream()), "pr_scene_setup_backward", inputs)
            what = f"{shape} {features} given {given} wanted {wanted}"
            if wanted[0]:
                got_rot, got_tr = g_rot.read("g_rotations").reshape(frames, 3, objects), g_tr.read("g_translations").reshape(frames, 3, objects)
                r = (_worst("setup_g_rot", got_rot, want.g_rot, want.tol_rot), _worst("setup_g_tr", got_tr, want.g_tr, want.tol_tr))
                assert np.isfinite(got_rot).all() and np.isfinite(got_tr).all() and max(r) <= 1.0, f"{what}: error / tolerance (g_rot, g_tr) = {r}"
                if not given[0]:
                    assert (got_rot == 0).all() and (got_tr == 0).all(), what
                COUNT["pose_backward_bit_differences"] += sr.bit_differences(got_rot, fp32.g_rot) + sr.bit_differences(got_tr, fp32.g_tr)
                COUNT["pose_backward_elements"] += 2 * got_rot.size
            for key, placed, X, was_given in (("g_style", g_style, S, given[1]), ("g_deformation", g_def, D, given[2])):
                if placed is None:
                    continue
                got = placed.read(key).reshape(frames, X, objects)
                r = _worst("setup_" + key, got, getattr(want, key), getattr(want, "tol_" + key[2:]))
                assert np.isfinite(got).all() and r <= 1.0, f"{what}: {key} error / tolerance {r}"
                same_bits(got, getattr(fp32, key), f"{what}: {key} against the fp32 sum")          # (plain sums in camera order)
                if not was_given:
                    assert (got == 0).all(), what
