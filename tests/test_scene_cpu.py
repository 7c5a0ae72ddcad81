"""The scene set-up restatements of tests/scene_reference.py, without a GPU: the float64 ones against torch autograd in float64, the
package's tensor formulation and the recorded fixtures; the fp32 ones inside the derived tolerances on every input the GPU tests
(tests/test_scene_gpu.py) use - the condition under which a kernel outside them is a finding about the kernel -; a list of wrong kernels,
each outside the tolerance (or off the bits) on a named input; and the error paths of the C ABI that need no device."""
import itertools
import os

import numpy as np
import pytest
import torch

from playableenvironments_amd import _lib
from playableenvironments_amd import environment_model as em
from tests import scene_reference as sr
from tests.helpers import projection_tensor_formulation as tensor_formulation

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(got, want, what, tol=1e-12):
    """Agreement of two float64 computations: 1e-12 of the largest magnitude (the results are sums of terms of that size)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), (what, np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------------------------------
# float64 against the package and the fixtures
@pytest.mark.parametrize("arm", list(sr.ARMS))
@pytest.mark.parametrize("translations", sr.TRANSLATION_FAMILIES)
@pytest.mark.parametrize("angles", ["uniform", "near_half_pi_x", "large_1e2"])
def test_float64_pose_matches_the_package_under_autograd(angles, translations, arm):
    """``pose_float64`` is ``euler_to_matrix`` / ``rigid_inverse`` and ``pose_backward_float64`` - the reverse-mode adjoint - is what torch autograd
    gives for them in float64, with both incoming gradients, either alone and neither; the kernel's own formula in float64 (the values
    of the bounded chain) is the same function."""
    rot, tr = sr.pose_inputs(angles, translations, 65)
    gm, gi = (g if wanted else None for g, wanted in zip(sr.pose_gradients(65), sr.ARMS[arm]))
    r = torch.from_numpy(rot.astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy(tr.astype(np.float64)).requires_grad_(True)
    m = em.euler_to_matrix(r, t)
    inv = em.rigid_inverse(m)
    want = sr.pose_float64(rot, tr)
    close(want.m, m.detach().numpy(), "m")
    close(want.inv, inv.detach().numpy(), "inv")
    loss = (m * 0).sum() + (inv * 0).sum()
    for out, g in ((m, gm), (inv, gi)):
        if g is not None:
            loud = g.astype(np.float64)
            loud[:, 3, :] = 1e30          # (the bottom rows are constants: no gradient flows through them)
            loss = loss + (out * torch.from_numpy(loud)).sum()
    loss.backward()
    got = sr.pose_backward_float64(rot, tr, gm, gi)
    close(got.g_rot, r.grad.numpy(), "g_rot")
    close(got.g_tr, t.grad.numpy(), "g_tr")
    chain = sr.pose_backward_chain_float64(rot, tr, gm, gi)
    close(chain.g_rot, got.g_rot, "the kernel's formula, g_rot")
    close(chain.g_tr, got.g_tr, "the kernel's formula, g_tr")
    if arm == "neither":
        assert (got.g_rot == 0).all() and (got.g_tr == 0).all()


@pytest.mark.parametrize("name", ["pose_math_minecraft.npz"])
def test_float64_pose_matches_the_recorded_fixtures(name):
    """``pose_float64`` against the reference's recorded pose math (its per-object ``torch.inverse`` path), to the tolerance test_cpu.py
    holds the package to on the same files."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "host", name)))
    cameras = sr.pose_float64(g["camera_rotations"].reshape(-1, 3), g["camera_translations"].reshape(-1, 3))
    np.testing.assert_allclose(cameras.inv.reshape(g["w2c"].shape), g["w2c"], rtol=1e-4, atol=1e-5)
    rows = lambda a: np.moveaxis(a, -1, -2).reshape(-1, 3)                      # (..., 3, K) -> (... x K, 3)
    objects = sr.pose_float64(rows(g["object_rotation_parameters"]), rows(g["object_translation_parameters"]))
    K = g["object_rotation_parameters"].shape[-1]
    lead = g["object_rotation_parameters"].shape[:-2]
    layout = lambda a: np.moveaxis(a.reshape(lead + (K, 4, 4)), -3, -1).reshape(g["o2w"].shape)       # (..., K, 4, 4) -> (..., 1, 4, 4, K)
    np.testing.assert_allclose(layout(objects.m), g["o2w"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(layout(objects.inv), g["w2o"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("boxes", [True, False], ids=["boxes", "axes"])
@pytest.mark.parametrize("shape", sr.PROJECTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float64_projection_matches_the_tensor_formulation(shape, boxes):
    """``project_float64`` against the package's tensor formulation on float64 CPU tensors: the box variant (reduced with +-1e20 where
    ``cam.z > 0``, clamped) with 65 points per object, the axes variant (4 points, the same for every object, unclamped)."""
    pts, o2w, w2c, focals, _ = sr.projection_inputs(*shape, 65 if boxes else 4)
    if not boxes:
        k = min(1, shape[2] - 1)                                                       # (object 1 reaches outside the view)
        pts = np.ascontiguousarray(np.broadcast_to(pts[k:k + 1], pts.shape))
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    want_points, want_boxes = tensor_formulation(t(pts), t(o2w), t(w2c), t(focals), sr.HEIGHT, sr.WIDTH, boxes)
    got = sr.project_float64(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
    close(got.points, want_points.numpy(), "points")
    if boxes:
        close(got.boxes, want_boxes.numpy(), "boxes")
        assert ((got.points == 0) | (got.points == 1)).any() or shape[2] == 1           # (clamped ...
    else:
        assert ((got.points < 0) | (got.points > 1)).any() or shape[2] == 1             # ... and not: a lone object stays inside the view)


@pytest.mark.parametrize("boxes", [True, False], ids=["boxes", "axes"])
def test_restatements_keep_a_nan_like_the_tensor_formulation(boxes):
    """``cam.z == 0``: the fp32 restatement (and with it the kernel it states) gives what the tensor formulation gives in fp32 on the
    CPU, NaNs in the same places - ``torch.min / max / clamp`` keep a NaN."""
    pts, o2w, w2c, focals = sr.degenerate_projection_inputs()
    want_points, want_boxes = tensor_formulation(*(torch.from_numpy(a) for a in (pts, o2w, w2c, focals)), sr.HEIGHT, sr.WIDTH, boxes)
    got = sr.project_fp32(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
    assert sr.bit_differences(got.points, want_points.numpy()) == 0 and np.isnan(got.points).any()
    if boxes:
        assert sr.bit_differences(got.boxes, want_boxes.numpy()) == 0 and np.isnan(got.boxes).all()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 inside the tolerances, on the inputs of the GPU file
@pytest.mark.parametrize("angles", sr.ANGLE_FAMILIES)
def test_fp32_pose_restatements_stay_inside_the_tolerances(angles):
    """Honest fp32 arithmetic (numpy's fp32 sine and cosine) stays inside ``tol_m, tol_inv, tol_rot, tol_tr`` on every family, count and arm."""
    worst = np.zeros(4)
    for translations in sr.TRANSLATION_FAMILIES:
        for count in sr.COUNTS:
            rot, tr = sr.pose_inputs(angles, translations, count)
            want, got = sr.pose_float64(rot, tr), sr.pose_fp32(rot, tr)
            worst[:2] = np.maximum(worst[:2], (sr.ratio(got.m, want.m, want.tol_m), sr.ratio(got.inv, want.inv, want.tol_inv)))
            assert (got.m[:, 3] == [0, 0, 0, 1]).all() and (got.inv[:, 3] == [0, 0, 0, 1]).all() and sr.bit_differences(got.m[:, :3, 3], tr) == 0
            for arm, wanted in sr.ARMS.items():
                gm, gi = (g if w else None for g, w in zip(sr.pose_gradients(count), wanted))
                want, got = sr.pose_backward_float64(rot, tr, gm, gi), sr.pose_backward_fp32(rot, tr, gm, gi)
                worst[2:] = np.maximum(worst[2:], (sr.ratio(got.g_rot, want.g_rot, want.tol_rot), sr.ratio(got.g_tr, want.g_tr, want.tol_tr)))
    print("fp32 pose restatements, worst error / tolerance (m, inv, g_rot, g_tr):", worst)
    assert worst.max() <= 1.0, worst


def test_fp32_projection_stays_inside_the_bound_and_decides_like_float64():
    """On every projection input of the GPU file: every |cam.z| is at least 1e-2 of the scene's extent, the fp32 restatement and the
    float64 one take the same ``cam.z > 0`` decision for EVERY point (none is left out of a comparison), a share of the points is behind
    the camera and the last object entirely, and the fp32 points and boxes are inside the float64 bound.  At every point count at
    least 0.4 of the box edges (0.25 per shape from 8 points on) lie strictly between 0 and 1."""
    worst, shares = np.zeros(2), {}
    for shape in sr.PROJECTION_SHAPES:
        for points in sr.POINT_COUNTS:
            pts, o2w, w2c, focals, all_behind = sr.projection_inputs(*shape, points)
            for boxes in (True, False):
                got = sr.project_fp32(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
                want = sr.project_float64(pts, o2w, w2c, focals, sr.HEIGHT, sr.WIDTH, boxes)
                assert np.abs(want.cam_z).min() >= 1e-2 * sr.EXTENT and np.array_equal(got.cam_z > 0, want.cam_z > 0)
                worst[0] = max(worst[0], sr.ratio(got.points, want.points, want.tol_points))
                if boxes:
                    worst[1] = max(worst[1], sr.ratio(got.boxes, want.boxes, want.tol_boxes))
                    if all_behind is not None:
                        assert (want.cam_z[:, :, all_behind] > 0).all()
                        assert (got.boxes[:, :, :, all_behind] == np.array([1, 1, 0, 0], F)).all()
                    # the box edges are minima / maxima of coordinates inside the image, not clamped constants: what a wrong reduction changes
                    shares.setdefault(points, []).append(sr.unsaturated_share(got.boxes))
                    assert points < 8 or shares[points][-1] >= 0.25, (shape, points, shares[points][-1])
                    assert ((got.points == 0) | (got.points == 1)).any() or shape[2] == 1          # (and the clamps act in every object 1)
            if shape[2] * points >= 64:
                assert 0 < (want.cam_z > 0).mean() < 1
    assert all(np.mean(v) >= 0.4 for v in shares.values()), {k: np.mean(v) for k, v in shares.items()}
    print("fp32 projection, worst error / bound (points, boxes):", worst)
    assert worst.max() <= 1.0, worst


def test_fp32_rays_stay_inside_the_bound():
    worst = 0.0
    for shape in sr.RAY_SHAPES:
        for per_frame in (False, True):
            c2w, focals, rows, cols = sr.ray_inputs(*shape, per_frame)
            got = sr.camera_rays_fp32(c2w, focals, rows, cols, sr.RAY_HEIGHT, sr.RAY_WIDTH, per_frame)
            want = sr.camera_rays_float64(c2w, focals, rows, cols, sr.RAY_HEIGHT, sr.RAY_WIDTH, per_frame)
            worst = max(worst, sr.ratio(got.directions, want.directions, want.tol_directions))
            assert rows.min() < 0 and cols.max() >= sr.RAY_WIDTH
            if per_frame and shape[0] > 1:
                assert not np.array_equal(cols[0], cols[1])
    assert worst <= 1.0, worst


def test_fp32_scene_setup_backward_stays_inside_the_tolerances():
    """The fused backward's restatement on the GPU file's shapes with every combination of absent incoming gradients."""
    worst = np.zeros(4)
    for shape in sr.SETUP_SHAPES:
        for features in sr.SETUP_FEATURES:
            rot, tr = sr.setup_backward_poses(shape[0], shape[2])
            for given in itertools.product((True, False), repeat=3):
                grads = [g if w else None for g, w in zip(sr.setup_gradients(*shape, *features), given)]
                want = sr.scene_setup_backward_float64(*shape, *features, rot, tr, *grads)
                got = sr.scene_setup_backward_fp32(*shape, *features, rot, tr, *grads)
                keys = ("rot", "tr", "style", "deformation")
                worst = np.maximum(worst, [sr.ratio(getattr(got, "g_" + k), getattr(want, "g_" + k), getattr(want, "tol_" + k)) for k in keys])
    print("fp32 set-up backward, worst error / tolerance (g_rot, g_tr, g_style, g_deformation):", worst)
    # (a two-camera sum is ONE rounding, whose bound u |sum| <= u sum |x| is attained: ratios close to 1 for the sums are the bound working)
    assert worst.max() <= 1.0, worst


def test_scene_setup_inputs_keep_the_boxes_off_the_clamps():
    """On every input of the fused set-up's GPU test at least half of the box edges lie strictly between 0 and 1 (the objects stand in
    view), and at the upsampled focal of the shapes with more than one object some are clamped."""
    for shape, points, upsample, flag in itertools.product(sr.SETUP_SHAPES, sr.SETUP_POINTS, (1.0, 2.0), (0, 1)):
        q = sr.setup_inputs(*shape, 1, 37, points, upsample, flag)
        cam_rot, cam_tr, obj_rot, obj_tr = sr.setup_pose_rows(q)
        cam, obj = sr.pose_fp32(cam_rot, cam_tr), sr.pose_fp32(obj_rot, obj_tr)
        boxes = sr.scene_setup_fp32(q, cam.m, cam.inv, obj.m, obj.inv)["boxes"]
        assert sr.unsaturated_share(boxes) >= 0.5, (shape, points, upsample, sr.unsaturated_share(boxes))
        if upsample == 2.0 and shape[2] > 1:
            assert ((boxes == 0) | (boxes == 1)).any(), (shape, points)


def test_trig_error_cannot_hide_a_fast_intrinsic():
    """The constant measured through the kernel is far below what a range-reduction-free intrinsic shows at the large angles."""
    assert 0 < sr.TRIG_ERR < sr.fast_trig_floor() / 10, (sr.TRIG_ERR, sr.fast_trig_floor())


# ---------------------------------------------------------------------------------------------------------------------
# wrong kernels
def _pose_forward_caught(mutant, angles, translations):
    rot, tr = sr.pose_inputs(angles, translations, 65)
    want, got = sr.pose_float64(rot, tr), sr.pose_fp32(rot, tr, mutant)
    return max(sr.ratio(got.m, want.m, want.tol_m), sr.ratio(got.inv, want.inv, want.tol_inv))


def _pose_backward_caught(mutant, angles, translations, arm):
    rot, tr = sr.pose_inputs(angles, translations, 65)
    gm, gi = (g if w else None for g, w in zip(sr.pose_gradients(65), sr.ARMS[arm]))
    want, got = sr.pose_backward_float64(rot, tr, gm, gi), sr.pose_backward_fp32(rot, tr, gm, gi, mutant)
    return max(sr.ratio(got.g_rot, want.g_rot, want.tol_rot), sr.ratio(got.g_tr, want.g_tr, want.tol_tr))


def _setup_backward_caught(mutant, shape, features):
    rot, tr = sr.setup_backward_poses(shape[0], shape[2])
    grads = sr.setup_gradients(*shape, *features)
    want = sr.scene_setup_backward_float64(*shape, *features, rot, tr, *grads)
    got = sr.scene_setup_backward_fp32(*shape, *features, rot, tr, *grads, mutant=mutant)
    return min(sr.ratio(getattr(got, "g_" + k), getattr(want, "g_" + k), getattr(want, "tol_" + k)) for k in ("rot", "tr", "style", "deformation"))


def _setup_bits_caught(mutant, shape, features):
    q = sr.setup_inputs(*shape, *features, 8)
    cam_rot, cam_tr, obj_rot, obj_tr = sr.setup_pose_rows(q)
    cam, obj = sr.pose_fp32(cam_rot, cam_tr), sr.pose_fp32(obj_rot, obj_tr)
    honest, wrong = (sr.scene_setup_fp32(q, cam.m, cam.inv, obj.m, obj.inv, mutant=m) for m in (None, mutant))
    return sr.bit_differences(honest["style_nks"], wrong["style_nks"])


def _projection_bits_caught(mutant, inputs, boxes=True):
    honest, wrong = (sr.project_fp32(*inputs, sr.HEIGHT, sr.WIDTH, boxes, mutant=m) for m in (None, mutant))
    return sr.bit_differences(honest.points, wrong.points) + (sr.bit_differences(honest.boxes, wrong.boxes) if boxes else 0)


def _projection_box_bits_caught(mutant, inputs):
    honest, wrong = (sr.project_fp32(*inputs, sr.HEIGHT, sr.WIDTH, True, mutant=m) for m in (None, mutant))
    assert sr.bit_differences(honest.points, wrong.points) == 0
    return sr.bit_differences(honest.boxes, wrong.boxes)


def _rays_bits_caught(mutant, shape):
    inputs = sr.ray_inputs(*shape, True)
    honest, wrong = (sr.camera_rays_fp32(*inputs, sr.RAY_HEIGHT, sr.RAY_WIDTH, True, mutant=m) for m in (None, mutant))
    return sr.bit_differences(honest.directions, wrong.directions)


# mutant -> (the input of the GPU file that catches it, how far outside: error / tolerance, or elements off the bits)
MUTANTS = {
    "dx_sign": ("pose backward, uniform angles, translations about 1, both gradients", lambda: _pose_backward_caught("dx_sign", "uniform", "unit", "both")),
    "dy_sign": ("pose backward, uniform angles, translations about 1, both gradients", lambda: _pose_backward_caught("dy_sign", "uniform", "unit", "both")),
    "dz_sign": ("pose backward, uniform angles, translations about 1, both gradients", lambda: _pose_backward_caught("dz_sign", "uniform", "unit", "both")),
    "gv_transposed": ("pose backward, uniform angles, zero translations, g_inverses only",
                      lambda: _pose_backward_caught("gv_transposed", "uniform", "zero", "inverses_only")),
    "t_gu_dropped": ("pose backward, uniform angles, translations about 60, g_inverses only",
                     lambda: _pose_backward_caught("t_gu_dropped", "uniform", "scene", "inverses_only")),
    "rt_gu": ("pose backward, uniform angles, zero translations, g_inverses only", lambda: _pose_backward_caught("rt_gu", "uniform", "zero", "inverses_only")),
    "last_camera_dropped": ("set-up backward, 2 frames x 2 cameras x 3 objects, S 1, D 37", lambda: _setup_backward_caught("last_camera_dropped", (2, 2, 3), (1, 37))),
    "style_k_s_swapped": ("set-up, 2 frames x 2 cameras x 3 objects, S 64", lambda: _setup_bits_caught("style_k_s_swapped", (2, 2, 3), (64, 64))),
    "rx_ry_rz": ("pose forward, uniform angles, zero translations", lambda: _pose_forward_caught("rx_ry_rz", "uniform", "zero")),
    "inverse_plus_rt_t": ("pose forward, uniform angles, translations about 1", lambda: _pose_forward_caught("inverse_plus_rt_t", "uniform", "unit")),
    "behind_includes_zero": ("projection, identity matrices and the axes points: cam.z == 0",
                             lambda: _projection_bits_caught("behind_includes_zero", sr.degenerate_projection_inputs())),
    "second_pass_not_reduced": ("projection, 3 frames x 2 cameras x 8 objects, 130 points: the points past the first 64 left out of the boxes",
                                lambda: _projection_box_bits_caught("second_pass_not_reduced", sr.projection_inputs(3, 2, 8, 130)[:4])),
    "upper_lanes_not_reduced": ("projection, 3 frames x 2 cameras x 8 objects, 65 points: lanes 32 to 63 left out of the boxes",
                                lambda: _projection_box_bits_caught("upper_lanes_not_reduced", sr.projection_inputs(3, 2, 8, 65)[:4])),
    "fminf_fmaxf": ("projection, identity matrices and the axes points: cam.z == 0, where fminf / fmaxf drop the NaN",
                    lambda: _projection_bits_caught("fminf_fmaxf", sr.degenerate_projection_inputs())),
    "height_width_swapped": ("projection, 1 frame x 1 camera x 1 object, 8 points, 45 x 64 image",
                             lambda: _projection_bits_caught("height_width_swapped", sr.projection_inputs(1, 1, 1, 8)[:4])),
    "cols_of_r": ("rays, 3 frames x 171 rays, per-frame pixel lists", lambda: _rays_bits_caught("cols_of_r", (3, 171))),
    "fast_trig": ("pose forward and backward, angles around 1e2, zero translations",
                  lambda: min(_pose_forward_caught("fast_trig", "large_1e2", "zero"), _pose_backward_caught("fast_trig", "large_1e2", "zero", "both"))),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_kernel_is_caught(mutant):
    """One sign flipped in each of ``dx, dy, dz``; ``gv[k * 4 + a]`` for ``gv[a * 4 + k]``; the ``-t[k] gu[a]`` term dropped; ``R^T gu`` for ``R gu`` in
    ``g_tr``; the last camera left out of the camera sum (every output of the fused backward is then outside); ``style`` read with K and S
    swapped; ``Rx (Ry Rz)``; ``+R^T t`` in the inverse; ``cam.z >= 0``; points past the first 64, or the lanes 32 to 63, left out of the box reduction; ``fminf / fmaxf``, which drop a NaN;
    height and width swapped in the normalisation; ``cols[r]`` for
    ``cols[g]``; sine and cosine from a range-reduction-free intrinsic: each falls outside the tolerance, or off the bits for the
    projection, the rays and the copies, on the named input of the GPU file."""
    where, caught = MUTANTS[mutant]
    by = caught()
    print(f"{mutant}: caught on [{where}] by {by:.4g}")
    assert by > 1.5, (mutant, where, by)


def test_the_honest_restatements_pass_where_the_mutants_fail():
    """The same measurements without a mutant: inside the tolerance, on the bits."""
    assert _pose_backward_caught(None, "uniform", "scene", "inverses_only") <= 1.0 and _pose_forward_caught(None, "large_1e2", "zero") <= 1.0
    assert _setup_bits_caught(None, (2, 2, 3), (64, 64)) == 0 and _rays_bits_caught(None, (3, 171)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# error paths that need no GPU
def test_scene_kernels_reject_bad_arguments_without_a_gpu(built_library):
    """Empty calls are no-ops and the argument checks of the fused backward answer before anything is enqueued."""
    lib = _lib.load()
    assert lib.pr_pose_matrices(0, None, None, None, None, None) == 0
    assert lib.pr_pose_matrices_backward(0, None, None, None, None, None, None, None) == 0
    assert lib.pr_project_points(0, 1, 1, 1, None, None, None, None, 45, 64, None, None, None) == 0
    backward = lambda frames, objects, rot, tr, g_rot, g_tr: lib.pr_scene_setup_backward(frames, 1, objects, 0, 0, rot, tr, None, None, None,
                                                                                           g_rot, g_tr, None, None, None)
    assert backward(0, 1, None, None, None, None) == 0
    assert backward(1, 1, 256, 256, 256, None) == -1
    assert b"come together" in lib.pr_last_error()
    assert backward(1, 1, 256, 256, None, 256) == -1
    assert b"come together" in lib.pr_last_error()
    assert backward(1, sr.PR_MAX_OBJECTS + 1, 256, 256, 256, 256) == -1
    assert b"bad sizes" in lib.pr_last_error()
    assert backward(1, 1, None, None, 256, 256) == -1
    assert b"NULL pose pointer" in lib.pr_last_error()
    assert sr.PR_MAX_OBJECTS == _lib.PR_MAX_OBJECTS
