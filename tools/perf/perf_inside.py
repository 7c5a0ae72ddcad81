"""Timing of the inside / outside queries and the fidelity of the project's simplified meshes as solids (GPU box): tennis player_1 at
the benchmark scene's pose and codes, the 128^3 lattice of voxel centres, level = the median in-box density, capped (close_border) -
the set-up of perf_raycast.py / perf_closest.py.

For simplify = 8, 4, 2 with keep_duplicates=True, on the mesh's bounding grid (as many cells as the cluster grid), on all three axes:
pr_inside_query of (a) 65 536 uniform points in the grid's box, (b) as many points ON the mesh (the closest points of (a)), (c) the
128^3 lattice points.  Beside each, in the same run: pr_closest_query with max_distance = inf and the fp32 density-only field query
(query_object) of the same points; the cells walked per point (computed from the grid coordinates, as the kernel computes them); for
256 of the points, drawn at random, the share of edge evaluations that need the exact fallback, from the numpy reference
(tests/inside_reference.py); and for (c) the share of lattice points whose `contains` equals the inside mask of the capped lattice
the mesh came from - the fidelity of simplify = k as a solid.

    python tools/perf/perf_inside.py [timed calls, default 10] [report path, default profiles/inside_report.json]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians with min - max (closest and the field
query on the lattice points: one warm-up, three timed calls).  Nothing here is a condition: the query has no parent to be measured
against.  The report is rewritten after every point set."""
import ctypes as C
import hashlib
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from playableenvironments_amd import ObjectComposer, _lib, configs, surface, synthetic  # noqa: E402
from tests import inside_reference as ir  # noqa: E402
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


def cells_walked(grid, points, axis):
    """Per point the cells of its column that k_inside_query visits, from the grid coordinates in fp32 as the kernel computes them."""
    origin = torch.tensor(grid.origin, dtype=torch.float32, device=points.device)
    cell = torch.tensor(grid.cell, dtype=torch.float32, device=points.device)
    g = (points - origin) / cell
    i, j, k = (axis + 1) % 3, (axis + 2) % 3, axis
    column = (g[:, i] >= 0) & (g[:, i] < grid.cells[i]) & (g[:, j] >= 0) & (g[:, j] < grid.cells[j]) & (g[:, k] < grid.cells[k])
    start = torch.where(g[:, k] >= 0, g[:, k], torch.zeros_like(g[:, k])).to(torch.int64)
    return torch.where(column, grid.cells[k] - start, torch.zeros_like(start))


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    report_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "inside_report.json")
    if not torch.cuda.is_available():
        raise RuntimeError("perf_inside.py measures on a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cfg = configs.tennis_config()
    object_idx, edge, N = 2, 128, 65536                              # player_1: NeRF + ray bender
    torch.manual_seed(0)
    comp = ObjectComposer(cfg)
    synthetic.randomize_module_state(comp, seed=0, step=20000, bender_scale=1e4)
    comp.eval().to(dev)
    comp.precision = "fp32"
    scene = synthetic.tennis_scene(seed=1234)                        # the benchmark's scene: camera, poses, codes
    inputs = [x.to(dev) for x in composer_inputs(cfg, scene, pixels=grid_pixels(256, 256, 256))]
    style = inputs[4][0, 0, 0, :, object_idx].reshape(1, -1).contiguous()
    deformation = inputs[5][0, 0, 0, :, object_idx].reshape(1, -1).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(0)
    rows = []
    report = {"device": props.name, "timed_calls": calls, "meshes": {}, "rows": rows,
              "library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]}

    def save():
        if report_path != "none":
            with open(report_path, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")

    def measure(label, fn, warm=3, timed_calls=None, **extra):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, timed_calls or calls)
        row = {"config": label, "call_ms_median": round(statistics.median(ms), 4), "call_ms_min": round(min(ms), 4),
               "call_ms_max": round(max(ms), 4)}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return {"call_ms": row["call_ms_median"], "min": row["call_ms_min"], "max": row["call_ms_max"]}

    def inside_call(grid, points, axis):
        points = points.reshape(1, -1, 3).contiguous()
        winding = torch.empty((1, points.size(1)), dtype=torch.int32, device=dev)
        s = surface.inside_struct(grid.vertices, grid.triangles, grid.vertex_offsets, grid.triangle_offsets, grid.total_vertices,
                                  grid.total_triangles, grid.origin, grid.cell, grid.cells, grid.cell_offsets, references=grid.references,
                                  points=points, axis=axis, winding=winding)
        keep = (points,)
        return (lambda: (_lib.check(lib.pr_inside_query(C.byref(s), stream), "pr_inside_query"), keep)[0]), winding

    def closest_call(grid, points):
        points = points.reshape(1, -1, 3).contiguous()
        distance = torch.empty((1, points.size(1)), dtype=torch.float32, device=dev)
        s = surface.closest_struct(grid.vertices, grid.triangles, grid.vertex_offsets, grid.triangle_offsets, grid.total_vertices,
                                   grid.total_triangles, grid.origin, grid.cell, grid.cells, grid.cell_offsets, references=grid.references,
                                   points=points, distance=distance, max_distance=math.inf)
        keep = (points,)
        return lambda: (_lib.check(lib.pr_closest_query(C.byref(s), stream), "pr_closest_query"), keep)[0]

    with torch.no_grad():
        sigma, centres = comp.density_grid(object_idx, edge, style, deformation)
        axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
        level = float(sigma.flatten()[::max(1, edge ** 3 // (1 << 20))].median())
        capped, _ = surface.clean_lattice(sigma, level, close_border=True)
        solid = (capped > level).reshape(-1)
        decided = (capped != level).reshape(-1)
        lattice = centres.reshape(-1, 3).contiguous()
        report["lattice"] = {"edge": edge, "level": level, "inside_points": int(solid.sum()), "points_on_the_level": int((~decided).sum())}
        full = surface.extract_surface(capped, axes, level, normals=False)[0]
        report["full_mesh"] = {"vertices": full.vertices.size(0), "triangles": full.triangles.size(0)}
        generator = torch.Generator(device="cpu").manual_seed(0)
        for k in (8, 4, 2):
            cluster = surface.lattice_cluster_grid(axes, k)
            mesh = full.simplified(*cluster, keep_duplicates=True)
            grid = surface.RayGrid.build([mesh], *surface.bounding_grid([mesh], cluster[2]))
            sizes = dict(simplify=k, triangles=mesh.triangles.size(0), grid_cells=list(grid.cells), references=int(grid.references.numel()))
            origin = torch.tensor(grid.origin, dtype=torch.float32, device=dev)
            extent = torch.tensor([c * n for c, n in zip(grid.cell, grid.cells)], dtype=torch.float32, device=dev)
            uniform = (origin + torch.rand((N, 3), generator=generator).to(dev) * extent).contiguous()
            on_mesh = grid.closest(uniform, max_distance=math.inf, point=True).point[0].contiguous()
            entry = dict(sizes)
            report["meshes"][f"simplify {k}"] = entry
            host ={"vertices": mesh.vertices.cpu().numpy(), "triangles": mesh.triangles.cpu().numpy(),
                    "vertex_offsets": np.array([0, mesh.vertices.size(0)], np.int32), "triangle_offsets": np.array([0, mesh.triangles.size(0)], np.int32)}
            for name, points in (("uniform", uniform), ("on_mesh", on_mesh), ("lattice", lattice)):
                few = name == "lattice"
                figures = {"points": points.size(0)}
                pick = torch.randperm(points.size(0), generator=generator)[:256].sort().values.to(dev)
                sample = points[pick]
                for axis in range(3):
                    run, winding = inside_call(grid, points, axis)
                    figures[f"axis {axis}"] = measure(f"simplify {k}: inside, {points.size(0)} {name} points, axis {axis}", run, **sizes)
                    walked = cells_walked(grid, points, axis).float()
                    counters = {}
                    want = ir.rule(host, sample.cpu().numpy()[None], axis, counters=counters)
                    figures[f"axis {axis}"].update(
                        mpoints_per_s=round(points.size(0) / figures[f"axis {axis}"]["call_ms"] / 1e3, 1), inside=int((winding != 0).sum()),
                        windings=sorted(set(winding.unique().tolist())), cells_walked_mean=round(float(walked.mean()), 2),
                        cells_walked_max=int(walked.max()),
                        exact_fallback_share_of_edges=round(counters.get("exact", 0) / max(1, counters.get("edges", 0)), 4),
                        sample_equals_reference=bool(np.array_equal(winding[0, pick].cpu().numpy(), want["winding"][0])))
                    if few:
                        got = (winding[0] != 0)
                        figures[f"axis {axis}"]["share_equal_to_the_lattice_mask"] = round(float((got == solid).float().mean()), 6)
                        figures[f"axis {axis}"]["share_equal_where_not_on_the_level"] = round(float((got == solid)[decided].float().mean()), 6)
                entry[name] = figures
                save()
                figures["closest_inf"] = measure(f"simplify {k}: closest (inf), {points.size(0)} {name} points", closest_call(grid, points),
                                                 warm=1 if few else 3, timed_calls=3 if few else None, **sizes)
                inside_box = torch.minimum(torch.maximum(points, lattice[0]), lattice[-1])[None].contiguous()    # (the field's domain)
                field = lambda: comp.query_object(object_idx, inside_box, style, deformation, features=False)["sigma"]
                figures["field_query_fp32"] = measure(f"simplify {k}: density-only field query, {points.size(0)} {name} points", field,
                                                      warm=1 if few else 3, timed_calls=3 if few else None, **sizes)
                entry[name] = figures
                save()
            print(json.dumps({f"simplify {k}": entry}), flush=True)
    save()


if __name__ == "__main__":
    main()
