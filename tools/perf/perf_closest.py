"""Timing of the closest-point queries and the deviation of the project's approximate meshes (GPU box): tennis player_1 at the benchmark
scene's pose and codes, the 128^3 lattice of voxel centres, level = the median in-box density (the set-up of perf_raycast.py).

(a) pr_closest_query of the vertices of the simplify = 2, 4, 8 meshes against the grid of the unsimplified mesh and the reverse, and
    the same for the band extraction (stride 4, guard 1): the time, and the deviation itself - max, mean, 99th percentile in lattice
    steps (the smallest of the lattice's three steps).
(b) 65 536 points at 0, 1/4, 1 and 4 cells from the surface of the simplify = 8 and 4 meshes (random triangles' centroids moved along
    the normal, sides alternating) on their bounding grids, with radii of 1 cell, 8 cells and inf: the time and - on the simplify = 8
    mesh, for 256 of the points, from the numpy restatement of the walk (tests/closest_reference.py) - the cells and triangles tested
    per point.
(c) The same points by a brute-force torch expression over all triangles in chunks (what a user would write without the query), and
    pr_raycast_query of as many rays on the same grid.

    python tools/perf/perf_closest.py [timed calls, default 10] [report path, default profiles/closest_report.json]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians with min - max (the brute force: one
warm-up, three timed calls).  Nothing here is a condition: the query has no parent to be measured against."""
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
from tests import closest_reference as cr  # noqa: E402
from tests import raycast_reference as rr  # noqa: E402
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


def brute_force(points, vertices, triangles, pairs=1 << 23):
    """The distance of every point (N, 3) from the mesh by Ericson's closest point on every triangle, in torch, in chunks of points:
    the expression a user would write today.  Returns (N)."""
    tri = triangles.long()
    a, b, c = vertices[tri[:, 0]][None], vertices[tri[:, 1]][None], vertices[tri[:, 2]][None]
    ab, ac, bc = b - a, c - a, c - b
    out = torch.empty(points.size(0), dtype=torch.float32, device=points.device)
    rows = max(1, pairs // max(1, tri.size(0)))
    for r0 in range(0, points.size(0), rows):
        p = points[r0:r0 + rows, None, :]
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        denom = va + vb + vc
        v, w = vb / denom, vc / denom                                                      # interior
        on_bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = torch.where(on_bc, 1 - wbc, v), torch.where(on_bc, wbc, w)
        on_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = torch.where(on_ac, torch.zeros_like(v), v), torch.where(on_ac, d2 / (d2 - d6), w)
        at_c = (d6 >= 0) & (d5 <= d6)
        v, w = torch.where(at_c, torch.zeros_like(v), v), torch.where(at_c, torch.ones_like(w), w)
        on_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = torch.where(on_ab, d1 / (d1 - d3), v), torch.where(on_ab, torch.zeros_like(w), w)
        at_b = (d3 >= 0) & (d4 <= d3)
        v, w = torch.where(at_b, torch.ones_like(v), v), torch.where(at_b, torch.zeros_like(w), w)
        at_a = (d1 <= 0) & (d2 <= 0)
        v, w = torch.where(at_a, torch.zeros_like(v), v), torch.where(at_a, torch.zeros_like(w), w)
        r = ap - v[..., None] * ab - w[..., None] * ac
        out[r0:r0 + rows] = (r * r).sum(-1).nan_to_num(math.inf).amin(1).sqrt()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    report_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "closest_report.json")
    if not torch.cuda.is_available():
        raise RuntimeError("perf_closest.py measures on a GPU")
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
    stream = torch.cuda.current_stream(dev).cuda_stream
    props = torch.cuda.get_device_properties(0)
    rows = []

    def measure(label, fn, warm=3, timed_calls=None, **extra):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, timed_calls or calls)
        med = statistics.median(ms)
        row = {"config": label, "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4), "call_ms_max": round(max(ms), 4)}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return med

    def query(grid, points, radius):
        """(call, distance (1, N)) of pr_closest_query on preallocated outputs: what is timed is the library call alone."""
        points = points.reshape(1, -1, 3).contiguous()
        distance = torch.empty((1, points.size(1)), dtype=torch.float32, device=dev)
        triangle = torch.empty((1, points.size(1)), dtype=torch.int32, device=dev)
        s = surface.closest_struct(grid.vertices, grid.triangles, grid.vertex_offsets, grid.triangle_offsets, grid.total_vertices,
                                   grid.total_triangles, grid.origin, grid.cell, grid.cells, grid.cell_offsets, references=grid.references,
                                   points=points, distance=distance, triangle=triangle, max_distance=radius)
        keep = (points, triangle)
        return (lambda: (_lib.check(lib.pr_closest_query(C.byref(s), stream), "pr_closest_query"), keep)[0]), distance

    def deviation(label, mesh, grid, step):
        run, distance = query(grid, mesh.vertices, math.inf)
        ms = measure(label, run, points=mesh.vertices.size(0), triangles=grid.total_triangles, grid_cells=list(grid.cells))
        steps = distance[0] / step
        found = torch.isfinite(steps)
        figures = {"points": int(steps.numel()), "misses": int((~found).sum()), "max_steps": round(float(steps[found].max()), 4),
                   "mean_steps": round(float(steps[found].mean()), 4), "p99_steps": round(float(torch.quantile(steps[found][:1 << 24], 0.99)), 4),
                   "call_ms": round(ms, 4)}
        print(json.dumps({label: figures}), flush=True)
        return figures

    report = {"deviation": {}, "proximity": {}}
    with torch.no_grad():
        sigma, _ = comp.density_grid(object_idx, edge, style, deformation)
        axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
        step = min(float(a[1] - a[0]) for a in axes)
        level = float(sigma.flatten()[::max(1, edge ** 3 // (1 << 20))].median())
        full = surface.extract_surface(sigma, axes, level)[0]
        del sigma
        full_grid = surface.RayGrid.build([full], *surface.bounding_grid([full], 64))
        report["lattice_step"] = step
        report["full_mesh"] = {"vertices": full.vertices.size(0), "triangles": full.triangles.size(0)}
        # (a) the deviation of the approximations
        simplified = {}
        for k in (2, 4, 8):
            mesh = full.simplified(*surface.lattice_cluster_grid(axes, k))
            grid = surface.RayGrid.build([mesh], *surface.bounding_grid([mesh], surface.lattice_cluster_grid(axes, k)[2]))
            simplified[k] = (mesh, grid)
            report["deviation"][f"simplify {k} -> full"] = deviation(f"simplify {k}: its vertices against the full mesh, 64^3 grid", mesh, full_grid, step)
            report["deviation"][f"full -> simplify {k}"] = deviation(f"simplify {k}: the full mesh's vertices against it", full, grid, step)
        band = comp.extract_mesh(object_idx, edge, style, deformation, level=level, stride=4, guard=1, normals=False)[0]
        band_grid = surface.RayGrid.build([band], *surface.bounding_grid([band], 64))
        report["deviation"]["band -> full"] = deviation("stride 4, guard 1: its vertices against the full mesh, 64^3 grid", band, full_grid, step)
        report["deviation"]["full -> band"] = deviation("stride 4, guard 1: the full mesh's vertices against it", full, band_grid, step)
        del band_grid, band, full_grid
        # (b), (c) proximity
        generator = torch.Generator(device="cpu").manual_seed(0)
        for k in (8, 4):
            mesh, grid = simplified[k]
            cell = min(grid.cell)
            tri = mesh.triangles.long()
            a, b, c = (mesh.vertices[tri[:, j]] for j in range(3))
            normal = torch.linalg.cross(b - a, c - a)
            good = torch.nonzero(normal.norm(dim=1) > 0)[:, 0]
            pick = good[torch.randint(0, good.numel(), (N,), generator=generator).to(dev)]
            centroid = (a[pick] + b[pick] + c[pick]) / 3
            unit = normal[pick] / normal[pick].norm(dim=1, keepdim=True)
            side = torch.where(torch.arange(N, device=dev) % 2 == 0, 1.0, -1.0)[:, None]
            t = torch.empty((1, N), dtype=torch.float32, device=dev)
            cast = surface.raycast_struct(grid.vertices, grid.triangles, grid.vertex_offsets, grid.triangle_offsets, grid.total_vertices,
                                          grid.total_triangles, grid.origin, grid.cell, grid.cells, grid.cell_offsets, references=grid.references,
                                          origins=origins[None], directions=directions[None], t=t)
            sizes = dict(simplify=k, triangles=mesh.triangles.size(0), grid_cells=list(grid.cells), references=int(grid.references.numel()))
            cast_ms = measure(f"simplify {k}: cast of {N} rays on the same grid", lambda: _lib.check(lib.pr_raycast_query(C.byref(cast), stream), "cast"), **sizes)
            if k == 8:
                host = {"vertices": mesh.vertices.cpu().numpy(), "triangles": mesh.triangles.cpu().numpy(),
                        "vertex_offsets": np.array([0, mesh.vertices.size(0)], np.int32), "triangle_offsets": np.array([0, mesh.triangles.size(0)], np.int32)}
                lists = rr.grid_lists(host, grid.origin, grid.cell, grid.cells)
            for offset in (0.0, 0.25, 1.0, 4.0):
                points = (centroid + side * offset * cell * unit).contiguous()
                entry = {"cast_ms": round(cast_ms, 4)}
                for radius_cells in (1.0, 8.0, math.inf):
                    run, distance = query(grid, points, radius_cells * cell)
                    ms = measure(f"simplify {k}: {N} points {offset} cells from the surface, radius {radius_cells} cells", run, **sizes)
                    found = torch.isfinite(distance[0])
                    entry[f"radius {radius_cells}"] = {"call_ms": round(ms, 4), "mpoints_per_s": round(N / ms / 1e3, 1), "found": int(found.sum()),
                                                       "mean_distance_cells": round(float(distance[0][found].mean() / cell), 4) if bool(found.any()) else None}
                if k == 8:
                    sample = points[:: N // 256][:256].cpu().numpy()[None]
                    tables = cr.pair_table(host, sample)
                    for radius_cells in (1.0, 8.0, math.inf):
                        walked = cr.walk(host, grid.origin, grid.cell, grid.cells, sample, radius_cells * cell, tables, lists)
                        want = cr.closest(host, sample, radius_cells * cell, tables)
                        entry[f"radius {radius_cells}"].update(
                            cells_tested_mean=round(float(walked["cells_tested"].mean()), 1), cells_tested_max=int(walked["cells_tested"].max()),
                            triangles_tested_mean=round(float(walked["triangles_tested"].mean()), 1),
                            triangles_tested_max=int(walked["triangles_tested"].max()),
                            walk_equals_search=bool(np.array_equal(walked["distance"].view(np.int32), want["distance"].view(np.int32))
                                                    and np.array_equal(walked["triangle"], want["triangle"])))
                    del tables
                brute = lambda: brute_force(points, mesh.vertices, mesh.triangles)
                brute_ms = measure(f"simplify {k}: {N} points {offset} cells from the surface, brute-force torch over {mesh.triangles.size(0)} triangles",
                                   brute, warm=1, timed_calls=3, **sizes)
                run, distance = query(grid, points, math.inf)
                run()
                entry["brute_force_ms"] = round(brute_ms, 4)
                entry["brute_force_over_query_inf"] = round(brute_ms / entry["radius inf"]["call_ms"], 2)
                entry["largest_difference_from_brute_force_cells"] = round(float((brute() - distance[0]).abs().max() / cell), 6)
                report["proximity"][f"simplify {k}, {offset} cells"] = entry
                print(json.dumps({f"simplify {k}, {offset} cells": entry}), flush=True)
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    report.update({"device": props.name, "library_sha256": sha, "timed_calls": calls, "rows": rows})
    if report_path != "none":
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
