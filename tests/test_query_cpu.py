"""Host-side checks of the point queries (pr_query_field): workspace sizes, refusals, the shape folding of
``RayBendingStyleNerfModel.forward`` and what the compiler made of the new kernels.  No GPU needed."""
import ctypes as C
import inspect
import os
import sys

import pytest
import torch

from playableenvironments_amd import ObjectComposer, _lib, configs, field_query
from playableenvironments_amd.modules import RayBendingStyleNerfModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_struct_host(cfg_model):
    """ObjectModel with the (host) pointers of a CPU composer: enough for the host-only checks, which never dereference them."""
    comp = ObjectComposer({"data": {"focal_length_multiplier": 1.0},
                           "model": {"apply_activation": False, "fix_object_overlaps": False, "static_object_models": 0,
                                     "object_parameters_encoder": [{"objects_count": 1}], "object_encoders": [{}],
                                     "object_models": [cfg_model]}})
    return comp, comp._model_struct(comp.object_models_coarse[0], 1)


def _query(groups=3, points=1500, features=True, skybox=False):
    q = _lib.Query()
    q.groups, q.points = groups, points
    for f in ("positions", "style", "deformation", "sigma", "displacement"):
        setattr(q, f, 256)
    if features:
        q.features = 256
    if skybox:
        q.ray_origins = q.ray_directions = 256
    return q


def _size(lib, q, s):
    size = C.c_size_t()
    status = lib.pr_query_workspace_size(C.byref(q), C.byref(s), C.byref(size))
    return status, size.value


def test_query_workspace_grows_with_the_points_and_shrinks_without_features(built_library):
    lib = built_library
    _keep, s = _model_struct_host(configs.tennis_config()["model"]["object_models"][2])
    sizes_m = [_size(lib, _query(points=m), s) for m in (1, 63, 64, 65, 257, 1500, 100000)]
    assert all(st == 0 for st, _ in sizes_m)
    assert all(a[1] <= b[1] for a, b in zip(sizes_m, sizes_m[1:])) and sizes_m[0][1] < sizes_m[-1][1]
    sizes_g = [_size(lib, _query(groups=g), s) for g in (1, 2, 3, 8, 64)]
    assert all(st == 0 for st, _ in sizes_g)
    assert all(a[1] < b[1] for a, b in zip(sizes_g, sizes_g[1:]))
    with_f, without = _size(lib, _query(), s), _size(lib, _query(features=False), s)
    assert with_f[0] == 0 and without[0] == 0 and without[1] < with_f[1]
    # the compact feature rows dominate: F floats per point, plus the records and the slot (5 words)
    per_point = with_f[1] / (3 * 1500)
    assert 192 * 4 <= per_point <= 192 * 4 + 64
    assert (with_f[1] - without[1]) >= 3 * 1500 * 192 * 4


def test_query_refusals_carry_a_message_and_precede_any_device_work(built_library):
    lib = built_library
    cfg = configs.tennis_config()
    _keep, s = _model_struct_host(cfg["model"]["object_models"][2])

    def refused(q, model=s, status=-1):
        st, _ = _size(lib, q, model)
        msg = lib.pr_last_error()
        assert st == status, (st, msg)
        assert msg
        # the call itself refuses the same way, before it touches the (fake) pointers or a device
        assert lib.pr_query_field(C.byref(q), C.byref(model), 256, 256, 1 << 40, None) == status
        return lib.pr_last_error()

    q = _query(groups=0)
    assert b"groups" in refused(q)
    q = _query(groups=-3)
    assert b"groups" in refused(q)
    q = _query(points=0)
    assert b"points" in refused(q)
    q = _query(groups=1 << 16, points=1 << 15)                 # G * M == 2^31
    assert b"2^31" in refused(q)
    q = _query(groups=1, points=(1 << 31) - 1)                 # the largest admitted call is sized without overflow
    st, size = _size(lib, q, s)
    assert st == 0 and size > ((1 << 31) - 1) * 192 * 4
    for field in ("positions", "style", "sigma"):
        q = _query()
        setattr(q, field, None)
        assert field.encode() in refused(q)
    q = _query()
    q.flags = _lib.PR_FLAG_CANONICAL_POSE
    assert _size(lib, q, s)[0] == 0
    for flags in (_lib.PR_FLAG_PERTURB, _lib.PR_FLAG_GATE_HEAD, _lib.PR_FLAG_CANONICAL_POSE | _lib.PR_FLAG_TRAIN_BN):
        q = _query()
        q.flags = flags
        assert b"flags" in refused(q)
    q = _query()
    q.precision = 7
    assert b"precision" in refused(q)
    for precision in (_lib.PR_PRECISION_FP32, _lib.PR_PRECISION_F16X3, _lib.PR_PRECISION_F16):
        q = _query()
        q.precision = precision
        assert _size(lib, q, s)[0] == 0
    # skybox models read the ray
    _keep2, sky = _model_struct_host(configs.minecraft_config()["model"]["object_models"][1])
    assert sky.kind == 1
    assert _size(lib, _query(skybox=True), sky)[0] == 0
    q = _query(skybox=True)
    q.ray_origins = None
    assert b"ray_origins" in refused(q, sky)
    q = _query(skybox=True)
    q.ray_directions = None
    assert b"ray_directions" in refused(q, sky)
    # workspace one byte short / misaligned / missing arguments
    q = _query()
    st, size = _size(lib, q, s)
    assert st == 0
    assert lib.pr_query_field(C.byref(q), C.byref(s), 256, 256, size - 1, None) == -2
    assert b"workspace too small" in lib.pr_last_error()
    assert lib.pr_query_field(C.byref(q), C.byref(s), 256, 257, size, None) == -1
    assert b"aligned" in lib.pr_last_error()
    assert lib.pr_query_field(C.byref(q), C.byref(s), None, 256, size, None) == -1
    assert b"packed" in lib.pr_last_error()
    assert lib.pr_query_field(None, C.byref(s), 256, 256, size, None) == -1
    assert lib.pr_query_workspace_size(C.byref(q), None, None) == -1


def test_forward_shape_folding():
    fold = field_query.fold_query_shapes
    # the composer's own shape: (N, R, P, 3) positions with (N, 1, S) codes -> N groups of R x P points
    f = fold((2, 5, 7, 3), (2, 1, 64), (2, 1, 8))
    assert (f["groups"], f["points"], f["split"], f["code_shape"], f["lead"]) == (2, 35, 1, [2], [2, 5, 7])
    # per-ray codes: every ray is a group
    f = fold((2, 5, 7, 3), (2, 5, 64), (2, 1, 8))
    assert (f["groups"], f["points"], f["code_shape"]) == (10, 7, [2, 5])
    # a broadcast in FRONT of a full dimension is expanded, not folded
    f = fold((2, 5, 7, 3), (1, 5, 64), (1, 5, 8))
    assert (f["groups"], f["points"], f["code_shape"]) == (10, 7, [2, 5])
    # one code for everything; codes with fewer leading dimensions; a flat (P, 3) list
    assert fold((4, 6, 9, 3), (1, 1, 64), (1, 1, 8))["groups"] == 1
    assert fold((4, 6, 9, 3), (1, 1, 64), (1, 1, 8))["points"] == 4 * 6 * 9
    assert (fold((4, 6, 9, 3), (64,), (8,))["groups"], fold((4, 6, 9, 3), (64,), (8,))["points"]) == (1, 216)
    f = fold((9, 3), (64,), (8,))
    assert (f["groups"], f["points"], f["code_shape"]) == (1, 9, [])
    f = fold((3, 1500, 1, 3), (3, 1, 64), (3, 1, 8))
    assert (f["groups"], f["points"]) == (3, 1500)
    assert fold((0, 5, 7, 3), (0, 1, 64), (0, 1, 8))["groups"] == 0
    for bad in (((2, 5, 7, 3), (3, 1, 64), (2, 1, 8)), ((2, 5, 7, 2), (2, 1, 64), (2, 1, 8)), ((3,), (64,), (8,)),
                ((5, 7, 3), (2, 5, 1, 64), (5, 8))):
        with pytest.raises(ValueError):
            fold(*bad)


def test_entry_points_keep_the_reference_signature_and_refuse_what_they_cannot_do():
    names = list(inspect.signature(RayBendingStyleNerfModel.forward).parameters)
    assert names == ["self", "ray_positions", "ray_origins", "ray_directions", "style", "deformation", "video_indexes", "canonical_pose"]
    comp = ObjectComposer(configs.tennis_config())
    model = comp.object_models_coarse[2]
    S, D = model.style_features, model.deformation_features
    args = (torch.zeros(1, 4, 2, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.zeros(1, 1, S), torch.zeros(1, 1, D))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
            model(*args)
        with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
            comp.query_object(2, torch.zeros(4, 3), torch.zeros(S), torch.zeros(D))
        comp.eval()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model(*args)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            comp.query_object(2, torch.zeros(4, 3), torch.zeros(S), torch.zeros(D))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            comp.density_grid(2, 4, torch.zeros(1, S), torch.zeros(1, D))


def test_stale_library_without_a_symbol_asks_for_a_rebuild(built_library, monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setitem(_lib.SYMBOLS, "pr_symbol_of_a_newer_header", (C.c_int, []))
    with pytest.raises(RuntimeError, match="rebuild"):
        _lib.load()
    monkeypatch.delitem(_lib.SYMBOLS, "pr_symbol_of_a_newer_header")
    assert _lib.load() is not None


def test_query_kernels_have_no_flat_accesses_and_the_density_only_loops_stay_pipelined(built_library):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    if not os.path.exists(isa_check.OBJDUMP):
        pytest.skip("llvm-objdump not found")
    counts = isa_check.memory_operations(_lib.library_path())
    for wanted in ("k_query_count", "k_query_fill", "k_query_scatter", "k_mlp_sigma", "k_mlp_split_sigma"):
        found = [k for k in counts if wanted in k]
        assert found, wanted
        for k in found:
            assert counts[k]["flat_load"] == 0 and counts[k]["flat_store"] == 0, (k, counts[k])
            assert counts[k]["global_load"] + counts[k]["global_store"] > 0, (k, counts[k])
    loops = isa_check.matrix_loops(_lib.library_path())
    for wanted in ("k_mlp_sigma", "k_mlp_split_sigma"):
        found = [k for k in loops if wanted in k]
        assert found, wanted                                          # the density-only kernels kept their matrix K loops
        for k in found:
            for loop in loops[k]:
                assert not any("vmcnt(0)" in w for w in loop["waits"]), (k, loop)
