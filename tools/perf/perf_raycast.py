"""Timing of the ray queries (GPU box): tennis player_1 at the benchmark scene's pose and codes, the 128^3 lattice of voxel centres,
level = the median in-box density (the set-up of perf_surface.py / perf_simplify.py); for the meshes simplify = 2, 4, 8 and three grids
each (the cluster grid of the mesh, one twice as coarse, and surface.bounding_grid with the cluster grid's cell counts): the counting and the emitting pr_raycast_build, and pr_raycast_query of
the 65 536 rays of the 256 x 256 benchmark camera in the object's frame - with R, the triangles per cell, the loose triangles, the
cells walked per ray and Mrays/s.  In the same run: the fp32 density-only query that fills the lattice (the build's yardstick) and
ObjectComposer.render_geometry of the same object and rays (what the cast approximates; reported, not a condition).

    python tools/perf/perf_raycast.py [timed calls, default 10] [report path, default profiles/raycast_report.json]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians with min - max.  The condition (DESIGN.md
section 12's rule for a front or back end): the emitting build takes at most 10 % of the density-only query of the lattice the mesh
came from, measured in the same run."""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from playableenvironments_amd import ObjectComposer, _lib, configs, surface, synthetic  # noqa: E402
from tests.helpers import composer_inputs, grid_pixels  # noqa: E402


def timed(fn, calls):
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def cells_walked(grid, origins, directions, t_hit):
    """The cells the query visits per ray, restated in torch fp32 (a measurement aid): the walk of the header from the clipped start
    to the first cell whose exit time reaches the reported t (or the clipped end, or the grid's border).  0 for a ray that never walks."""
    origin, cell = (torch.tensor(x, dtype=torch.float32, device=origins.device) for x in grid[:2])
    cells = list(grid[2])
    og, dg = (origins - origin) / cell, directions / cell
    top = torch.tensor(cells, dtype=torch.float32, device=origins.device)
    inf = torch.full_like(og[:, 0], float("inf"))
    moving = dg != 0
    ta, tb = (0 - og) / dg, (top - og) / dg
    tlo = torch.where(moving, torch.minimum(ta, tb), -inf[:, None]).amax(1).clamp_min(0.0)
    thi = torch.where(moving, torch.maximum(ta, tb), inf[:, None]).amin(1)
    walking = (tlo <= thi) & (moving | ((og >= 0) & (og <= top))).all(1) & moving.any(1) & torch.isfinite(og).all(1) & torch.isfinite(dg).all(1)
    i = torch.minimum((og + tlo[:, None] * dg).clamp_min(0), top - 1).nan_to_num(0).to(torch.int64)
    forward = (dg > 0).to(torch.int64)
    count = torch.zeros_like(tlo, dtype=torch.int64)
    for _ in range(sum(cells) + 1):
        if not bool(walking.any()):
            break
        te = torch.where(moving, ((i + forward).to(torch.float32) - og) / dg, inf[:, None])
        tout, axis = te.min(1)
        count += walking.to(torch.int64)
        walking = walking & ~((t_hit <= tout) | ~(tout < thi))
        step = torch.nn.functional.one_hot(axis, 3) * (2 * forward - 1)
        i = torch.where(walking[:, None], i + step, i)
        walking = walking & ((i >= 0) & (i < top.to(torch.int64))).all(1)
        i = i.clamp_min(0).minimum(top.to(torch.int64) - 1)
    return count


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    report_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "raycast_report.json")
    if not torch.cuda.is_available():
        raise RuntimeError("perf_raycast.py measures on a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cfg = configs.tennis_config()
    object_idx, edge = 2, 128                                        # player_1: NeRF + ray bender
    torch.manual_seed(0)
    comp = ObjectComposer(cfg)
    synthetic.randomize_module_state(comp, seed=0, step=20000, bender_scale=1e4)
    comp.eval().to(dev)
    comp.precision = "fp32"
    scene = synthetic.tennis_scene(seed=1234)                        # the benchmark's scene: camera, poses, codes
    inputs = [x.to(dev) for x in composer_inputs(cfg, scene, pixels=grid_pixels(256, 256, 256))]
    o, d, n, w2o, style_all, deformation_all, in_scene = inputs
    style = style_all[0, 0, 0, :, object_idx].reshape(1, -1).contiguous()
    deformation = deformation_all[0, 0, 0, :, object_idx].reshape(1, -1).contiguous()
    m = w2o[0, 0, 0, :, :, object_idx]
    directions = (d.reshape(-1, 3) @ m[:3, :3].T).contiguous()
    origins = (o.reshape(1, 3) @ m[:3, :3].T + m[:3, 3]).expand_as(directions).contiguous()
    N = directions.size(0)
    only = torch.zeros_like(in_scene)
    only[..., object_idx] = True
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(0)
    rows = []

    def measure(label, fn, **extra):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, calls)
        med = statistics.median(ms)
        row = {"config": label, "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4), "call_ms_max": round(max(ms), 4)}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return med

    verdicts = {}
    with torch.no_grad():
        query_ms = measure(f"{edge}^3 fp32 density-only query", lambda: comp.density_grid(object_idx, edge, style, deformation))
        geometry_ms = measure("render_geometry, player_1 alone, 65 536 rays, fp32",
                              lambda: comp.render_geometry(o, d, n, w2o, style_all, deformation_all, only, False), rays=N)
        sigma, _ = comp.density_grid(object_idx, edge, style, deformation)
        axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
        level = float(sigma.flatten()[::max(1, edge ** 3 // (1 << 20))].median())
        full = surface.extract_surface(sigma, axes, level)[0]
        del sigma
        for k in (2, 4, 8):
            mesh = full.simplified(*surface.lattice_cluster_grid(axes, k))
            V, T = mesh.vertices.size(0), mesh.triangles.size(0)
            offsets_in = torch.tensor([[0, V], [0, T]], dtype=torch.int32, device=dev)
            for which in ("cluster", "coarser", "bounding"):
                if which == "bounding":                            # the same number of cells around the mesh's own box: nothing lies on a face
                    grid = surface.bounding_grid([mesh], surface.lattice_cluster_grid(axes, k)[2])
                else:
                    grid = surface._ray_grid(*surface.lattice_cluster_grid(axes, k * (1 if which == "cluster" else 2)))
                lists = grid[2][0] * grid[2][1] * grid[2][2] + 1
                cell_offsets = torch.empty(lists + 1, dtype=torch.int32, device=dev)
                common = (mesh.vertices, mesh.triangles, offsets_in[0], offsets_in[1], V, T, *grid, cell_offsets)
                count = surface.raycast_struct(*common)
                size = C.c_size_t()
                _lib.check(lib.pr_raycast_workspace_size(C.byref(count), C.byref(size)), "pr_raycast_workspace_size")
                workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
                build = lambda s: _lib.check(lib.pr_raycast_build(C.byref(s), workspace.data_ptr(), size.value, stream), "pr_raycast_build")
                build(count)
                R = int(cell_offsets[lists])
                references = torch.empty(max(R, 1), dtype=torch.int32, device=dev)
                emit = surface.raycast_struct(*common, references=references)
                build(emit)
                per_cell = (cell_offsets[1:lists] - cell_offsets[:lists - 1]).to(torch.float32)
                occupied = per_cell[per_cell > 0]
                t = torch.empty((1, N), dtype=torch.float32, device=dev)
                triangle = torch.empty((1, N), dtype=torch.int32, device=dev)
                cast = surface.raycast_struct(*common, references=references, origins=origins[None], directions=directions[None], t=t,
                                              triangle=triangle)
                run_cast = lambda: _lib.check(lib.pr_raycast_query(C.byref(cast), stream), "pr_raycast_query")
                run_cast()
                walked = cells_walked(grid, origins, directions, t[0]).to(torch.float32)
                hit = triangle[0] >= 0
                sizes = dict(simplify=k, grid_cells=grid[2], vertices=V, triangles=T, references=R, loose=int(cell_offsets[lists] - cell_offsets[lists - 1]),
                             triangles_per_cell_mean=round(float(per_cell.mean()), 3),
                             triangles_per_occupied_cell_mean=round(float(occupied.mean()) if occupied.numel() else 0.0, 3),
                             triangles_per_cell_max=int(per_cell.max()), workspace_bytes=size.value)
                label = f"simplify {k}, {which} grid {grid[2][0]}^3"
                count_ms = measure(f"{label}: counting build", lambda: build(count), **sizes)
                emit_ms = measure(f"{label}: emitting build", lambda: build(emit), **sizes)
                cast_ms = measure(f"{label}: cast of 65 536 rays", run_cast, rays=N, hits=int(hit.sum()),
                                  cells_walked_per_ray_mean=round(float(walked.mean()), 2), cells_walked_per_ray_max=int(walked.max()), **sizes)
                verdicts[label] = {"counting_build_ms": round(count_ms, 4), "emitting_build_ms": round(emit_ms, 4),
                                   "density_only_query_ms": round(query_ms, 4), "share": round(emit_ms / query_ms, 6),
                                   "condition_at_most": 0.10, "met": bool(emit_ms <= 0.10 * query_ms), "cast_ms": round(cast_ms, 4),
                                   "mrays_per_s": round(N / cast_ms / 1e3, 1), "render_geometry_ms": round(geometry_ms, 4),
                                   "cast_share_of_render_geometry": round(cast_ms / geometry_ms, 6)}
                del workspace, references
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    report = {"device": props.name, "library_sha256": sha, "timed_calls": calls, "rows": rows, "condition": verdicts}
    print(json.dumps(report["condition"]))
    if report_path != "none":
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
