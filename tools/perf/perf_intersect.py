"""Timing of mesh intersection (GPU box): tennis player_1 at the benchmark scene's pose and codes, the 128^3 lattice of voxel centres,
level = the median in-box density, capped (close_border) - the set-up of perf_sample.py and its four WELDED meshes: the unsimplified
mesh and simplify = 8, 4, 2 with keep_duplicates=True, G = 1.

Every mesh is queried against a copy of itself under a rigid transform - a rotation of 10 degrees about z and a shift of 4 lattice
steps along x - on bounding_grid([mesh], 32), and beside it on bounding_grid([mesh], 128): the counting call, the emitting call with
segments (which counts again, as the contract says), and self mode (counting).  Beside them, in the same run, the fp32 density-only field query (query_object) of the same 128^3
lattice, and the project's rule for a front or back end (applied in every mesh section): the counting call plus the
emitting call at most 10 % of that query.  Per mesh also the pair counts and the list entries a query triangle visits (the sizes of
the lists of the cells its box overlaps, plus the loose list), mean and maximum.

    python tools/perf/perf_intersect.py [timed calls, default 20] [report path, default profiles/intersect_report.json]

Protocol: three warm-up calls per configuration, HIP events around every timed call on preallocated outputs and workspace, medians
with min - max (a call that takes 0.1 s or more: three timed calls).  The feature has no parent to be measured against.  The report
is rewritten after every mesh.

    python tools/perf/perf_intersect.py trace <simplify k or 0>
runs ten emitting calls on one mesh and nothing else - the command to put behind `rocprofv3 --kernel-trace --stats --`."""
import ctypes as C
import hashlib
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from playableenvironments_amd import ObjectComposer, _lib, configs, surface, synthetic  # noqa: E402
from tests.helpers import composer_inputs, grid_pixels  # noqa: E402

CELLS = 32
FINE_CELLS = 128


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


def visited_entries(grid, vertices, triangles):
    """Per query triangle the list entries its lane reads: the loose list plus the lists of the cells its box overlaps (torch, fp32
    grid coordinates as the kernel computes them; a statistic, not a contract)."""
    cells = grid.cells
    C1 = cells[0] * cells[1] * cells[2] + 1
    sizes = (grid.cell_offsets[1:C1 + 1] - grid.cell_offsets[:C1]).to(torch.int64)
    table = torch.zeros([n + 1 for n in cells], dtype=torch.int64, device=sizes.device)
    table[1:, 1:, 1:] = sizes[:-1].reshape(cells).cumsum(0).cumsum(1).cumsum(2)
    corner = vertices[triangles.long()]
    origin = torch.tensor(grid.origin, dtype=torch.float32, device=vertices.device)
    cell = torch.tensor(grid.cell, dtype=torch.float32, device=vertices.device)
    top = torch.tensor(cells, dtype=torch.float32, device=vertices.device)
    low, high = (corner.amin(1) - origin) / cell, (corner.amax(1) - origin) / cell
    inside = ((high >= 0) & (low < top)).all(dim=1)
    lo = low.clamp(min=0).minimum(top - 1).long()
    hi = torch.minimum(high.clamp(min=0), top).long().minimum(top.long() - 1) + 1
    at = lambda x, y, z: table[x[:, 0], y[:, 1], z[:, 2]]
    box = (at(hi, hi, hi) - at(lo, hi, hi) - at(hi, lo, hi) - at(hi, hi, lo) + at(lo, lo, hi) + at(lo, hi, lo) + at(hi, lo, lo) - at(lo, lo, lo))
    return torch.where(inside, box, torch.zeros_like(box)) + sizes[-1]


def main():
    trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
    only = int(sys.argv[2]) if trace else None
    calls = 10 if trace else int(sys.argv[1]) if len(sys.argv) > 1 else 20
    report_path = "none" if trace else sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "intersect_report.json")
    if not torch.cuda.is_available():
        raise RuntimeError("perf_intersect.py measures on a GPU")
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
    style = inputs[4][0, 0, 0, :, object_idx].reshape(1, -1).contiguous()
    deformation = inputs[5][0, 0, 0, :, object_idx].reshape(1, -1).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []
    report = {"device": torch.cuda.get_device_properties(0).name, "timed_calls": calls, "cells": CELLS, "meshes": {}, "rows": rows,
              "library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]}

    def save():
        if report_path != "none":
            with open(report_path, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")

    def measure(label, fn, **extra):
        fn()
        torch.cuda.synchronize()
        slow = timed(fn, 1)[0] > 100.0                                # a call of 0.1 s and more: one more warm-up, three timed calls
        for _ in range(1 if slow else 2):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, 3 if slow else calls)
        row = {"config": label, "call_ms_median": round(statistics.median(ms), 4), "call_ms_min": round(min(ms), 4),
               "call_ms_max": round(max(ms), 4)}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    def intersect_call(grid, mesh, transform, self_, P=None):
        """(run, outputs, workspace bytes): a counting call (P None) or an emitting call with segments and P rows, preallocated."""
        QT = mesh.triangles.size(0)
        out = {"count": torch.empty(QT, dtype=torch.int32, device=dev), "first": torch.empty(QT, dtype=torch.int32, device=dev),
               "pair_offsets": torch.empty(QT + 1, dtype=torch.int32, device=dev)}
        if P is not None:
            out["pairs"] = torch.empty((max(P, 1), 2), dtype=torch.int32, device=dev)
            out["segments"] = torch.empty((max(P, 1), 2, 3), dtype=torch.float32, device=dev)
        query = {} if self_ else dict(q_vertices=grid.vertices, q_triangles=grid.triangles, q_vertex_offsets=grid.vertex_offsets,
                                      q_triangle_offsets=grid.triangle_offsets, transform=transform)
        s = surface.intersect_struct(grid.vertices, grid.triangles, grid.vertex_offsets, grid.triangle_offsets, grid.total_vertices,
                                     grid.total_triangles, grid.origin, grid.cell, grid.cells, grid.cell_offsets, references=grid.references,
                                     self_=self_, **query, **out)
        if P is not None:
            s.max_pairs = P
        size = C.c_size_t()
        _lib.check(lib.pr_mesh_intersect_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_intersect_workspace_size")
        workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
        run = lambda: (_lib.check(lib.pr_mesh_intersect(C.byref(s), workspace.data_ptr(), size.value, stream), "pr_mesh_intersect"), transform)[0]
        return run, out, size.value

    with torch.no_grad():
        sigma, centres = comp.density_grid(object_idx, edge, style, deformation)
        axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
        step = min(float(a[1] - a[0]) for a in axes)
        level = float(sigma.flatten()[::max(1, edge ** 3 // (1 << 20))].median())
        capped, _ = surface.clean_lattice(sigma, level, close_border=True)
        lattice = centres.reshape(1, -1, 3).contiguous()
        report["lattice"] = {"edge": edge, "level": level, "step": step}
        full = surface.extract_surface(capped, axes, level, normals=True)[0]
        if not trace:
            field = measure("fp32 density-only field query of the 128^3 lattice",
                            lambda: comp.query_object(object_idx, lattice, style, deformation, features=False)["sigma"])
            report["field_query_ms"] = field["call_ms_median"]
        a = math.radians(10.0)
        transform = torch.tensor([[[math.cos(a), -math.sin(a), 0.0, 4 * step], [math.sin(a), math.cos(a), 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]],
                                 dtype=torch.float32, device=dev)
        report["transform"] = {"rotation_about_z_degrees": 10.0, "shift_x_steps": 4}
        for k in (8, 4, 2, 0):
            if trace and k != only:
                continue
            mesh = (full if k == 0 else full.simplified(*surface.lattice_cluster_grid(axes, k), keep_duplicates=True)).welded()
            name = "unsimplified" if k == 0 else f"simplify {k}"
            V, T = mesh.vertices.size(0), mesh.triangles.size(0)
            posed = mesh.vertices @ transform[0, :, :3].T + transform[0, :, 3]
            for cells in (CELLS, FINE_CELLS):                          # the contract's grid, and a finer one beside it
                if trace and cells != CELLS:
                    continue
                grid = surface.RayGrid.build([mesh], *surface.bounding_grid([mesh], cells))
                count_run, counted, workspace_bytes = intersect_call(grid, mesh, transform, False)
                count_run()
                P = int(counted["pair_offsets"][T])
                emit_run, emitted, _ = intersect_call(grid, mesh, transform, False, P)
                if trace:
                    for _ in range(calls):
                        emit_run()
                    torch.cuda.synchronize()
                    print(name, T, P)
                    continue
                label = f"{name}, {cells}^3 cells"
                counting = measure(f"{label}: counting call", count_run, simplify=k, vertices=V, triangles=T, workspace_bytes=workspace_bytes)
                emitting = measure(f"{label}: emitting call with segments", emit_run, simplify=k, pairs=P)
                visited = visited_entries(grid, posed, mesh.triangles)
                both = counting["call_ms_median"] + emitting["call_ms_median"]
                entry = {"vertices": V, "triangles": T, "cells": cells, "references": int(grid.references.numel()), "pairs": P,
                         "query_triangles_with_a_pair": int((counted["count"] > 0).sum()),
                         "list_entries_visited_per_query_mean": round(float(visited.double().mean()), 2),
                         "list_entries_visited_per_query_max": int(visited.max()), "workspace_bytes": workspace_bytes,
                         "counting_ms": counting["call_ms_median"], "emitting_ms": emitting["call_ms_median"],
                         "counting_plus_emitting_ms": round(both, 4), "share_of_the_field_query": round(both / report["field_query_ms"], 4),
                         "within_10_percent": both <= 0.1 * report["field_query_ms"]}
                if cells == CELLS:
                    self_run, own, _ = intersect_call(grid, mesh, None, True)
                    entry["self_ms"] = measure(f"{label}: self mode, counting call", self_run, simplify=k)["call_ms_median"]
                    entry["self_pairs"] = int(own["pair_offsets"][T]) // 2
                again = {key: x.clone() for key, x in emitted.items()}
                emit_run()
                torch.cuda.synchronize()
                entry["equal_bits_on_a_second_call"] = all(torch.equal(again[key].view(torch.int32), x.view(torch.int32)) for key, x in emitted.items())
                report["meshes"][label] = entry
                print(json.dumps({label: entry}), flush=True)
                save()
                del grid, count_run, emit_run, counted, emitted
    save()


if __name__ == "__main__":
    main()
