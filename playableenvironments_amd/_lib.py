"""ctypes binding of libplayrender.so (the C ABI declared in include/playrender.h).

The library is built in-tree by ``__graft_entry__.build()`` (or ``make -C playableenvironments_amd/csrc``).
There is no CPU fallback: if the shared object is missing, ``load()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

PR_MAX_OBJECTS = 8
PR_MAX_LAYERS = 12
PR_MAX_OCTAVES = 16

PR_FLAG_PERTURB = 1
PR_FLAG_CANONICAL_POSE = 2
PR_FLAG_FIX_OVERLAPS = 4
PR_FLAG_NAIVE_MLP = 8
PR_FLAG_TRAIN_BN = 16
PR_FLAG_SAVE_FOR_BACKWARD = 32
PR_FLAG_GATE_HEAD = 64
PR_FLAG_DEFER_PROJECTION = 2048
PR_FLAG_DEVICE_NOISE = 128
PR_FLAG_DIVERGENCE_GRAD = 256
PR_FLAG_SIGMOID_FEATURES = 512
PR_FLAG_SPLIT_BACKWARD = 1024
PR_FLAG_GEOMETRY_ONLY = 4096
PR_PRECISION_FP32 = 0
PR_PRECISION_F16X3 = 1
PR_PRECISION_F16 = 2
PR_PROFILE_CATEGORIES = 8   # host array length of pr_profile_collect

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)


class Linear(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("out_features", C.c_int32), ("in_features", C.c_int32)]


class ObjectModel(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("has_bender", C.c_int32), ("positions", C.c_int32),
        ("style_features", C.c_int32), ("deformation_features", C.c_int32), ("output_features", C.c_int32),
        ("layers_width", C.c_int32), ("backbone_count", C.c_int32), ("skip_layer_idx", C.c_int32),
        ("octaves", C.c_int32), ("bender_width", C.c_int32), ("bender_count", C.c_int32),
        ("bender_skip", C.c_int32), ("bender_octaves", C.c_int32),
        ("bender_octave_weights", C.c_float * PR_MAX_OCTAVES),
        ("bbox", C.c_float * 6),
        ("empty_space_alpha", C.c_float), ("z_near_min", C.c_float), ("z_far_max", C.c_float), ("bn_eps", C.c_float),
        ("backbone", Linear * PR_MAX_LAYERS),
        ("alpha_head", Linear),
        ("head0", Linear),
        ("affine1", Linear), ("bn1_mean", C.c_void_p), ("bn1_var", C.c_void_p), ("bn1_batches", C.c_void_p),
        ("head3", Linear),
        ("affine4", Linear), ("bn4_mean", C.c_void_p), ("bn4_var", C.c_void_p), ("bn4_batches", C.c_void_p),
        ("head6", Linear),
        ("bender", Linear * PR_MAX_LAYERS),
        ("bender_out", Linear),
    ]


class Object(C.Structure):
    _fields_ = [("coarse", ObjectModel), ("packed_coarse", C.c_void_p), ("fine", ObjectModel), ("packed_fine", C.c_void_p)]


class Noise(C.Structure):
    _fields_ = [
        ("jitter", C.c_void_p * PR_MAX_OBJECTS), ("alpha", C.c_void_p * PR_MAX_OBJECTS),
        ("pdf", C.c_void_p * PR_MAX_OBJECTS), ("integrate", C.c_void_p * PR_MAX_OBJECTS),
        ("integrate_global", C.c_void_p), ("divergence", C.c_void_p * PR_MAX_OBJECTS),
    ]


class Entry(C.Structure):
    _fields_ = [
        ("integrated_features", C.c_void_p), ("opacity", C.c_void_p), ("weights", C.c_void_p), ("depth", C.c_void_p),
        ("disparity", C.c_void_p), ("integrated_displacements_magnitude", C.c_void_p), ("integrated_divergence", C.c_void_p),
    ]


ENTRY_FIELDS = [f[0] for f in Entry._fields_]


PR_MAX_DECODER_GROUPS = 4


class DecoderLayout(C.Structure):
    _fields_ = [("groups", C.c_int32), ("rays", C.c_int32 * PR_MAX_DECODER_GROUPS), ("width", C.c_int32 * PR_MAX_DECODER_GROUPS),
                ("channel_begin", C.c_int32 * PR_MAX_DECODER_GROUPS), ("channel_end", C.c_int32 * PR_MAX_DECODER_GROUPS),
                ("map", C.c_void_p * PR_MAX_DECODER_GROUPS)]


class Outputs(C.Structure):
    _fields_ = [
        ("object", Entry * PR_MAX_OBJECTS), ("global_", Entry),
        ("sample_t", C.c_void_p * PR_MAX_OBJECTS), ("sample_sigma", C.c_void_p * PR_MAX_OBJECTS),
        ("sample_slot", C.c_void_p * PR_MAX_OBJECTS), ("evaluated_samples", C.c_void_p), ("normalised_samples", C.c_void_p),
        ("sample_delta", C.c_void_p * PR_MAX_OBJECTS), ("head_samples", C.c_void_p),
        ("decoder", DecoderLayout),
    ]


class Call(C.Structure):
    _fields_ = [
        ("frames", C.c_int32), ("rays", C.c_int32), ("objects", C.c_int32), ("static_objects", C.c_int32),
        ("use_fine", C.c_int32), ("flags", C.c_uint32), ("precision", C.c_int32), ("reserved_", C.c_int32),
        ("ray_origins", C.c_void_p), ("ray_directions", C.c_void_p), ("w2o", C.c_void_p), ("style", C.c_void_p),
        ("deformation", C.c_void_p), ("object_in_scene", C.c_void_p),
        ("linspace_coarse", C.c_void_p * PR_MAX_OBJECTS), ("linspace_fine", C.c_void_p * PR_MAX_OBJECTS),
        ("positions_fine", C.c_int32 * PR_MAX_OBJECTS),
        ("noise_coarse", Noise), ("noise_fine", Noise),
        ("noise_seed", C.c_uint64), ("noise_ray_offset", C.c_int32), ("noise_total_rays", C.c_int32),
        ("noise_seed_device", C.c_void_p),
    ]


class EntryGrads(C.Structure):
    _fields_ = [("integrated_features", C.c_void_p), ("opacity", C.c_void_p), ("depth", C.c_void_p),
                ("integrated_displacements_magnitude", C.c_void_p), ("weights", C.c_void_p),
                ("integrated_divergence", C.c_void_p)]


GRAD_FIELDS = [f[0] for f in EntryGrads._fields_]


class OutputGrads(C.Structure):
    _fields_ = [("object", EntryGrads * PR_MAX_OBJECTS), ("global_", EntryGrads),
                ("sample_t", C.c_void_p * PR_MAX_OBJECTS), ("sample_delta", C.c_void_p * PR_MAX_OBJECTS)]


class LinearGrad(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p)]


class ModelGrads(C.Structure):
    _fields_ = [
        ("backbone", LinearGrad * PR_MAX_LAYERS), ("alpha_head", LinearGrad), ("head0", LinearGrad), ("affine1", LinearGrad),
        ("head3", LinearGrad), ("affine4", LinearGrad), ("head6", LinearGrad), ("bender", LinearGrad * PR_MAX_LAYERS),
        ("bender_out", LinearGrad),
    ]


class InputGrads(C.Structure):
    _fields_ = [("w2o", C.c_void_p), ("style", C.c_void_p), ("deformation", C.c_void_p), ("model", ModelGrads * PR_MAX_OBJECTS),
                ("model_fine", ModelGrads * PR_MAX_OBJECTS), ("ray_origins", C.c_void_p), ("ray_directions", C.c_void_p)]


class SampleGrads(C.Structure):
    """pr_sample_grads_t (include/playrender.h): the per-sample gradients of the compositing backward, per level."""
    _fields_ = [("sigma", C.c_void_p * PR_MAX_OBJECTS), ("t", C.c_void_p * PR_MAX_OBJECTS),
                ("displacement_magnitude", C.c_void_p * PR_MAX_OBJECTS), ("features", C.c_void_p * PR_MAX_OBJECTS),
                ("norm", C.c_void_p), ("feature_rows", C.c_void_p * PR_MAX_OBJECTS)]


class Query(C.Structure):
    """pr_query_t (include/playrender.h): a point query of one object model's fields."""
    _fields_ = [("groups", C.c_int32), ("points", C.c_int32), ("flags", C.c_uint32), ("precision", C.c_int32),
                ("positions", C.c_void_p), ("ray_origins", C.c_void_p), ("ray_directions", C.c_void_p), ("style", C.c_void_p),
                ("deformation", C.c_void_p), ("features", C.c_void_p), ("sigma", C.c_void_p), ("displacement", C.c_void_p),
                ("slot", C.c_void_p), ("counters", C.c_void_p)]


class OccupancyGrid(C.Structure):
    """pr_occupancy_grid_t (include/playrender.h)."""
    _fields_ = [("bits", C.c_void_p), ("cells", C.c_int32 * 3), ("words", C.c_int32)]


class Occupancy(C.Structure):
    """pr_occupancy_t (include/playrender.h)."""
    _fields_ = [("coarse", OccupancyGrid * PR_MAX_OBJECTS), ("fine", OccupancyGrid * PR_MAX_OBJECTS)]


class Retained(C.Structure):
    """pr_retained_t (include/playrender.h)."""
    _fields_ = [("object_mask", C.c_uint32), ("reserved_", C.c_uint32), ("host_key", C.c_uint64), ("cache", C.c_void_p),
                ("cache_bytes", C.c_size_t), ("reused", C.c_void_p)]


class FineGuide(C.Structure):
    """pr_fine_guide_t (include/playrender.h)."""
    _fields_ = [("object_mask", C.c_uint32), ("guard", C.c_int32), ("threshold", C.c_float), ("reserved_", C.c_uint32),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class Geometry(C.Structure):
    """pr_geometry_t (include/playrender.h)."""
    _fields_ = [("visibility", C.c_void_p), ("front_object", C.c_void_p)]


class Surface(C.Structure):
    """pr_surface_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("points", C.c_int32 * 3), ("level", C.c_float), ("flags", C.c_uint32), ("sigma", C.c_void_p),
                ("axis", C.c_void_p * 3), ("max_vertices", C.c_int32), ("max_triangles", C.c_int32), ("vertices", C.c_void_p),
                ("normals", C.c_void_p), ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p)]


COMPONENTS_CLOSE_BORDER = 1      # PR_COMPONENTS_CLOSE_BORDER
COMPONENTS_MAX_KEEP = 8          # PR_COMPONENTS_MAX_KEEP


class Components(C.Structure):
    """pr_components_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("points", C.c_int32 * 3), ("level", C.c_float), ("flags", C.c_uint32), ("min_points", C.c_int32),
                ("keep_largest", C.c_int32), ("fill", C.c_float), ("reserved_", C.c_uint32), ("sigma", C.c_void_p), ("labels", C.c_void_p),
                ("sizes", C.c_void_p), ("sigma_out", C.c_void_p), ("counts", C.c_void_p)]


BAND_MIN_STRIDE = 2              # PR_BAND_MIN_STRIDE
BAND_MAX_STRIDE = 64             # PR_BAND_MAX_STRIDE
BAND_MAX_GUARD = 8               # PR_BAND_MAX_GUARD


class Band(C.Structure):
    """pr_band_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("points", C.c_int32 * 3), ("level", C.c_float), ("flags", C.c_uint32), ("stride", C.c_int32),
                ("guard", C.c_int32), ("max_points", C.c_int32), ("reserved_", C.c_uint32), ("sigma", C.c_void_p), ("axis", C.c_void_p * 3),
                ("values", C.c_void_p), ("point_offsets", C.c_void_p), ("counts", C.c_void_p), ("active", C.c_void_p),
                ("point_index", C.c_void_p), ("positions", C.c_void_p), ("exact", C.c_void_p)]


SIMPLIFY_KEEP_DUPLICATES = 1     # PR_SIMPLIFY_KEEP_DUPLICATES
SIMPLIFY_MAX_CELLS = 1 << 21     # PR_SIMPLIFY_MAX_CELLS


class Simplify(C.Structure):
    """pr_simplify_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("origin", C.c_float * 3), ("cell", C.c_float * 3), ("cells", C.c_int32 * 3), ("max_vertices", C.c_int32),
                ("max_triangles", C.c_int32), ("reserved_", C.c_uint32), ("vertices", C.c_void_p), ("normals", C.c_void_p),
                ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p), ("out_vertices", C.c_void_p),
                ("out_normals", C.c_void_p), ("out_triangles", C.c_void_p), ("vertex_map", C.c_void_p), ("counts", C.c_void_p),
                ("out_vertex_offsets", C.c_void_p), ("out_triangle_offsets", C.c_void_p)]


RAYCAST_CULL_BACK = 1            # PR_RAYCAST_CULL_BACK
RAYCAST_MAX_AXIS_CELLS = 1024    # PR_RAYCAST_MAX_AXIS_CELLS
RAYCAST_MAX_CELLS = 1 << 21      # PR_RAYCAST_MAX_CELLS


class Raycast(C.Structure):
    """pr_raycast_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("origin", C.c_float * 3), ("cell", C.c_float * 3), ("cells", C.c_int32 * 3), ("max_references", C.c_int32),
                ("rays", C.c_int32), ("t_min", C.c_float), ("t_max", C.c_float), ("reserved_", C.c_uint32), ("vertices", C.c_void_p),
                ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p), ("cell_offsets", C.c_void_p),
                ("references", C.c_void_p), ("origins", C.c_void_p), ("directions", C.c_void_p), ("t", C.c_void_p),
                ("triangle", C.c_void_p), ("barycentric", C.c_void_p)]


class Closest(C.Structure):
    """pr_closest_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("origin", C.c_float * 3), ("cell", C.c_float * 3), ("cells", C.c_int32 * 3), ("max_references", C.c_int32),
                ("count", C.c_int32), ("max_distance", C.c_float), ("vertices", C.c_void_p), ("triangles", C.c_void_p),
                ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p), ("cell_offsets", C.c_void_p),
                ("references", C.c_void_p), ("points", C.c_void_p), ("distance", C.c_void_p), ("triangle", C.c_void_p),
                ("point", C.c_void_p), ("barycentric", C.c_void_p)]


class Inside(C.Structure):
    """pr_inside_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("origin", C.c_float * 3), ("cell", C.c_float * 3), ("cells", C.c_int32 * 3), ("max_references", C.c_int32),
                ("count", C.c_int32), ("axis", C.c_int32), ("vertices", C.c_void_p), ("triangles", C.c_void_p),
                ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p), ("cell_offsets", C.c_void_p),
                ("references", C.c_void_p), ("points", C.c_void_p), ("winding", C.c_void_p), ("crossings", C.c_void_p)]


class MeshAudit(C.Structure):
    """pr_mesh_audit_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p),
                ("counts", C.c_void_p), ("measures", C.c_void_p), ("labels", C.c_void_p)]


AUDIT_COUNTS = 12                # columns of pr_mesh_audit_t.counts
AUDIT_MEASURES = 8               # columns of pr_mesh_audit_t.measures


class MeshWeld(C.Structure):
    """pr_mesh_weld_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("attribute_width", C.c_int32), ("max_vertices", C.c_int32), ("max_triangles", C.c_int32), ("reserved_", C.c_uint32),
                ("vertices", C.c_void_p), ("normals", C.c_void_p), ("attributes", C.c_void_p), ("triangles", C.c_void_p),
                ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p), ("out_vertices", C.c_void_p),
                ("out_normals", C.c_void_p), ("out_attributes", C.c_void_p), ("out_triangles", C.c_void_p), ("vertex_map", C.c_void_p),
                ("triangle_map", C.c_void_p), ("counts", C.c_void_p), ("out_vertex_offsets", C.c_void_p),
                ("out_triangle_offsets", C.c_void_p)]


WELD_COMPACT_ONLY = 1            # PR_WELD_COMPACT_ONLY
WELD_COUNTS = 8                  # columns of pr_mesh_weld_t.counts
WELD_MAX_ATTRIBUTE_WIDTH = 4096


class MeshSmooth(C.Structure):
    """pr_mesh_smooth_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("steps", C.c_int32), ("max_degree", C.c_int32), ("lambda_", C.c_float), ("mu", C.c_float),
                ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p),
                ("pinned", C.c_void_p), ("out_vertices", C.c_void_p), ("out_normals", C.c_void_p), ("incidence_offsets", C.c_void_p),
                ("incidence", C.c_void_p), ("vertex_state", C.c_void_p), ("counts", C.c_void_p)]


SMOOTH_PIN_BORDER = 1            # PR_SMOOTH_PIN_BORDER
SMOOTH_COUNTS = 8                # columns of pr_mesh_smooth_t.counts
SMOOTH_MAX_STEPS = 4096
SMOOTH_MAX_DEGREE = 256


class MeshSample(C.Structure):
    """pr_mesh_sample_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("samples", C.c_int32), ("attribute_width", C.c_int32), ("seed", C.c_uint64), ("first_sample", C.c_uint64),
                ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p),
                ("normals", C.c_void_p), ("attributes", C.c_void_p), ("points", C.c_void_p), ("triangle", C.c_void_p),
                ("barycentric", C.c_void_p), ("out_normals", C.c_void_p), ("out_attributes", C.c_void_p), ("counts", C.c_void_p),
                ("measures", C.c_void_p)]


SAMPLE_FACE_NORMALS = 1          # PR_SAMPLE_FACE_NORMALS
SAMPLE_COUNTS = 4                # columns of pr_mesh_sample_t.counts
SAMPLE_MEASURES = 2              # columns of pr_mesh_sample_t.measures
SAMPLE_MAX_ATTRIBUTE_WIDTH = 4096


class MeshIntersect(C.Structure):
    """pr_mesh_intersect_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("origin", C.c_float * 3), ("cell", C.c_float * 3), ("cells", C.c_int32 * 3), ("max_references", C.c_int32),
                ("q_total_vertices", C.c_int32), ("q_total_triangles", C.c_int32), ("max_pairs", C.c_int32), ("reserved_", C.c_uint32),
                ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p),
                ("cell_offsets", C.c_void_p), ("references", C.c_void_p), ("q_vertices", C.c_void_p), ("q_triangles", C.c_void_p),
                ("q_vertex_offsets", C.c_void_p), ("q_triangle_offsets", C.c_void_p), ("transform", C.c_void_p), ("count", C.c_void_p),
                ("first", C.c_void_p), ("pair_offsets", C.c_void_p), ("pairs", C.c_void_p), ("segments", C.c_void_p)]


INTERSECT_SELF = 1               # PR_INTERSECT_SELF


class MeshPlace(C.Structure):
    """pr_mesh_place_t (include/playrender.h)."""
    _fields_ = [("groups", C.c_int32), ("total_vertices", C.c_int32), ("total_triangles", C.c_int32), ("flags", C.c_uint32),
                ("total_merged_vertices", C.c_int32), ("total_merged_triangles", C.c_int32), ("scale", C.c_float),
                ("regularisation", C.c_float), ("max_move", C.c_float * 3), ("reserved_", C.c_uint32),
                ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("vertex_offsets", C.c_void_p), ("triangle_offsets", C.c_void_p),
                ("vertex_map", C.c_void_p), ("merged_vertices", C.c_void_p), ("merged_vertex_offsets", C.c_void_p),
                ("merged_triangles", C.c_void_p), ("merged_triangle_offsets", C.c_void_p), ("out_vertices", C.c_void_p),
                ("counts", C.c_void_p)]


PLACE_COUNTS = 4                 # columns of pr_mesh_place_t.counts: moved, kept, skipped + invalid, turned


# every exported symbol of include/playrender.h : (restype, argtypes)
class SceneSetup(C.Structure):
    """pr_scene_setup_t (include/playrender.h)."""
    _fields_ = [("frames", C.c_int32), ("cameras", C.c_int32), ("objects", C.c_int32), ("box_points_per_object", C.c_int32),
                ("style_features", C.c_int32), ("deformation_features", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("focal_multiplier", C.c_float), ("upsample_factor", C.c_float), ("axes_with_upsampled_focals", C.c_int32),
                ("camera_rotations", C.c_void_p), ("camera_translations", C.c_void_p), ("focals", C.c_void_p),
                ("object_rotations", C.c_void_p), ("object_translations", C.c_void_p), ("style", C.c_void_p),
                ("deformation", C.c_void_p), ("object_in_scene", C.c_void_p), ("box_points", C.c_void_p), ("axes_points", C.c_void_p),
                ("boxes", C.c_void_p), ("projected_points", C.c_void_p), ("axes", C.c_void_p), ("camera34", C.c_void_p),
                ("render_focals", C.c_void_p), ("w2o34", C.c_void_p), ("style_nks", C.c_void_p), ("deformation_nkd", C.c_void_p),
                ("present", C.c_void_p)]


SYMBOLS = {
    "pr_packed_size": (C.c_int, [C.POINTER(ObjectModel), C.POINTER(C.c_size_t)]),
    "pr_pack_model": (C.c_int, [C.POINTER(ObjectModel), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_pack_models": (C.c_int, [C.c_int32, C.POINTER(C.POINTER(ObjectModel)), c_int32_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                 C.c_void_p]),
    "pr_workspace_size": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(C.c_size_t)]),
    "pr_render_forward": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(Outputs), C.POINTER(Outputs),
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_render_forward_culled": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(Occupancy), C.POINTER(Outputs), C.POINTER(Outputs),
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_retained_size": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.c_uint32, C.POINTER(C.c_size_t)]),
    "pr_retained_reset": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_render_forward_retained": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(Occupancy), C.POINTER(Retained),
                                             C.POINTER(Outputs), C.POINTER(Outputs), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_fine_guide_size": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.c_uint32, C.POINTER(C.c_size_t)]),
    "pr_render_forward_guided": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(Occupancy), C.POINTER(Retained),
                                           C.POINTER(FineGuide), C.POINTER(Outputs), C.POINTER(Outputs), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_render_geometry": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(Occupancy), C.POINTER(FineGuide), C.POINTER(Outputs),
                                     C.POINTER(Outputs), C.POINTER(Geometry), C.POINTER(Geometry), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_occupancy_build": (C.c_int, [C.c_void_p, C.c_int32, c_int32_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "pr_surface_workspace_size": (C.c_int, [C.POINTER(Surface), C.POINTER(C.c_size_t)]),
    "pr_extract_surface": (C.c_int, [C.POINTER(Surface), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_components_workspace_size": (C.c_int, [C.POINTER(Components), C.POINTER(C.c_size_t)]),
    "pr_label_components": (C.c_int, [C.POINTER(Components), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_band_workspace_size": (C.c_int, [C.POINTER(Band), C.POINTER(C.c_size_t)]),
    "pr_band_plan": (C.c_int, [C.POINTER(Band), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_band_fill": (C.c_int, [C.POINTER(Band), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_simplify_workspace_size": (C.c_int, [C.POINTER(Simplify), C.POINTER(C.c_size_t)]),
    "pr_simplify_mesh": (C.c_int, [C.POINTER(Simplify), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_raycast_workspace_size": (C.c_int, [C.POINTER(Raycast), C.POINTER(C.c_size_t)]),
    "pr_raycast_build": (C.c_int, [C.POINTER(Raycast), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_raycast_query": (C.c_int, [C.POINTER(Raycast), C.c_void_p]),
    "pr_closest_query": (C.c_int, [C.POINTER(Closest), C.c_void_p]),
    "pr_inside_query": (C.c_int, [C.POINTER(Inside), C.c_void_p]),
    "pr_mesh_audit_workspace_size": (C.c_int, [C.POINTER(MeshAudit), C.POINTER(C.c_size_t)]),
    "pr_mesh_audit": (C.c_int, [C.POINTER(MeshAudit), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_mesh_weld_workspace_size": (C.c_int, [C.POINTER(MeshWeld), C.POINTER(C.c_size_t)]),
    "pr_mesh_weld": (C.c_int, [C.POINTER(MeshWeld), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_mesh_smooth_workspace_size": (C.c_int, [C.POINTER(MeshSmooth), C.POINTER(C.c_size_t)]),
    "pr_mesh_smooth": (C.c_int, [C.POINTER(MeshSmooth), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_mesh_sample_workspace_size": (C.c_int, [C.POINTER(MeshSample), C.POINTER(C.c_size_t)]),
    "pr_mesh_sample": (C.c_int, [C.POINTER(MeshSample), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_mesh_intersect_workspace_size": (C.c_int, [C.POINTER(MeshIntersect), C.POINTER(C.c_size_t)]),
    "pr_mesh_intersect": (C.c_int, [C.POINTER(MeshIntersect), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_mesh_place_workspace_size": (C.c_int, [C.POINTER(MeshPlace), C.POINTER(C.c_size_t)]),
    "pr_mesh_place": (C.c_int, [C.POINTER(MeshPlace), C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_backward_workspace_size": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(C.c_size_t)]),
    "pr_render_backward": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(OutputGrads), C.POINTER(OutputGrads),
                                     C.POINTER(InputGrads), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_render_backward_exported": (C.c_int, [C.POINTER(Call), C.POINTER(Object), C.POINTER(OutputGrads), C.POINTER(OutputGrads),
                                              C.POINTER(InputGrads), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.POINTER(SampleGrads), C.POINTER(SampleGrads)]),
    "pr_camera_rays": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_expected_positions": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_noise_fill": (C.c_int, [C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "pr_roi_pool_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_roi_pool_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_query_workspace_size": (C.c_int, [C.POINTER(Query), C.POINTER(ObjectModel), C.POINTER(C.c_size_t)]),
    "pr_query_field": (C.c_int, [C.POINTER(Query), C.POINTER(ObjectModel), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pr_profile_enable": (C.c_int, [C.c_int]),
    "pr_profile_collect": (C.c_int, [C.POINTER(C.c_double), c_int32_p]),
    "pr_probe_mfma_f32": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]),
    "pr_probe_mfma_f16": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]),
    "pr_abi_version": (C.c_int, []),
    "pr_pose_matrices": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_pose_matrices_backward": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "pr_project_points": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_scene_setup": (C.c_int, [C.POINTER(SceneSetup), C.c_void_p]),
    "pr_scene_setup_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 10),
    "pr_patch_pixels": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                               C.c_float, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pr_graph_node_census": (C.c_int, [C.c_void_p, c_int32_p]),
    "pr_last_error": (C.c_char_p, []),
    "pr_device_info": (C.c_int, [c_int32_p, c_int32_p, C.c_char_p, C.c_size_t]),
}

_LIB: Optional[C.CDLL] = None


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libplayrender.so")


def load() -> C.CDLL:
    """Loads libplayrender.so (once) and sets the prototypes.  Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C playableenvironments_amd/csrc).  There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # a library built from older sources: the same advice as for an ABI mismatch, not a bare AttributeError
            raise RuntimeError(f"{path} does not export {name}: it was built from older sources "
                               "(rebuild: make -C playableenvironments_amd/csrc)") from None
        fn.restype = res
        fn.argtypes = args
    if lib.pr_abi_version() != 5:
        raise RuntimeError(f"libplayrender ABI version {lib.pr_abi_version()} != 5 (rebuild: make -C playableenvironments_amd/csrc)")
    _LIB = lib
    return lib


class PlayRenderError(RuntimeError):
    pass


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().pr_last_error()
        raise PlayRenderError(f"{what} failed with status {status}: {msg.decode() if msg else ''}")
