"""playableenvironments_amd - MI355X-native volumetric renderer for Playable Environments.

Public surface (mirrors the reference's modules for the renderer hot path only):
  ObjectComposer            drop-in for model/object_composer.py:ObjectComposer (forward, forward_expected_positions,
                            autograd through pr_render_backward)
  EnvironmentModel          model/environment_model.py:EnvironmentModel: every forward mode (scene encodings, observations,
                            scene-encoding-only, pose / keypoint consistency), render_full_frame_*, render_sharded
  encoders                  the object encoders / pose estimators that produce the renderer's inputs, with their
                            region-of-interest crop on a HIP kernel (roi_pool); batching: the pinned one-copy Batch path
  FrameGraph                a whole evaluation frame captured and replayed as one HIP graph
  geometry                  torch restatements of a geometry-only render's extra outputs (ObjectComposer.render_geometry,
                            EnvironmentModel.render_geometry_from_scene_encoding): per-object visibility, front object
  surface, Mesh             triangle meshes of density lattices on the device (marching tetrahedra: surface.extract_surface,
                            ObjectComposer.extract_mesh), with floater removal and capping on the same lattice
                            (surface.label_components, surface.clean_lattice); surface.refine_band / ObjectComposer.density_band
                            evaluate a lattice only in a band around the level set; surface.simplify_meshes reduces
                            extracted meshes by vertex clustering (extract_mesh(simplify=k)); surface.RayGrid casts rays
                            against them (closest hits on a cell grid) and finds the closest point of a mesh to a point
                            (RayGrid.closest, Mesh.distance_to) and whether a point lies inside one (RayGrid.winding /
                            contains / signed_distance: watertight, exact where the topology depends on it); RayGrid.intersect /
                            Mesh.intersections / Mesh.self_intersections / surface.collide find the triangle pairs in which
                            two meshes - or one mesh and itself - cut each other, with contact segments
  ray_sampling, wire_format pixel / ray samplers and the renderer <-> decoder tensor glue of the reference
  parallel                  frame shards, overlapped feature all-gather, gradient all-reduce (torch.distributed / RCCL)
  configs / synthetic       shipped renderer configurations and seeded synthetic scenes
"""
from . import batching, configs, encoders, geometry, parallel, ray_sampling, surface, synthetic, wire_format  # noqa: F401
from .environment_model import EnvironmentModel  # noqa: F401
from .frame_graph import FrameGraph  # noqa: F401
from .object_composer import ObjectComposer, ObjectIDsHelper  # noqa: F401
from .surface import Mesh, MeshContacts, RayGrid, clean_lattice, collide, label_components, simplify_meshes  # noqa: F401

__all__ = ["ObjectComposer", "ObjectIDsHelper", "EnvironmentModel", "FrameGraph", "configs", "synthetic", "parallel",
           "ray_sampling", "wire_format", "encoders", "batching", "geometry", "surface", "Mesh", "label_components",
           "clean_lattice", "simplify_meshes", "RayGrid", "MeshContacts", "collide"]
