"""Timing of welding and compaction (GPU box): tennis player_1 at the benchmark scene's pose and codes, the 128^3 lattice of voxel
centres, level = the median in-box density, capped (close_border) - the set-up of perf_audit.py and its four meshes.

pr_mesh_weld, the emitting call with normals, a 192-wide attribute array and both maps, of the unsimplified mesh and of simplify = 8,
4, 2 with keep_duplicates=True, G = 1; beside it, in the same run, the fp32 density-only field query (query_object) of the same 128^3
lattice, and the project's rule for a front or back end (applied in 20 and 24): the call at most 10 % of that query.
Secondary, in the same run: what a user writes without the call - torch.unique(vertices, dim=0, return_inverse=True) and the index
arithmetic that re-indexes the triangles and gathers the rows - as a ratio; its output order differs, so there is no threshold.

    python tools/perf/perf_weld.py [timed calls, default 10] [report path, default profiles/weld_report.json]

Protocol: three warm-up calls per configuration, HIP events around every timed call on preallocated outputs and workspace, medians
with min - max.  The feature has no parent to be measured against.  The report is rewritten after every mesh.

    python tools/perf/perf_weld.py trace <simplify k or 0>
runs ten calls on one mesh and nothing else - the command to put behind `rocprofv3 --kernel-trace --stats --` for a kernel breakdown."""
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

WIDTH = 192


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


def main():
    trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
    only = int(sys.argv[2]) if trace else None
    calls = 10 if trace or len(sys.argv) < 2 else int(sys.argv[1])
    report_path = "none" if trace else sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weld_report.json")
    if not torch.cuda.is_available():
        raise RuntimeError("perf_weld.py measures on a GPU")
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
    report = {"device": torch.cuda.get_device_properties(0).name, "timed_calls": calls, "attribute_width": WIDTH, "meshes": {}, "rows": rows,
              "library_sha256": hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]}

    def save():
        if report_path != "none":
            with open(report_path, "w") as f:
                json.dump(report, f, indent=1)
                f.write("\n")

    def measure(label, fn, **extra):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, calls)
        row = {"config": label, "call_ms_median": round(statistics.median(ms), 4), "call_ms_min": round(min(ms), 4),
               "call_ms_max": round(max(ms), 4)}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    def weld_call(mesh, attributes):
        """(run, outputs, workspace bytes): a counting call sizes the outputs, `run` is the emitting call on them."""
        V, T = mesh.vertices.size(0), mesh.triangles.size(0)
        offsets = torch.tensor([[0, V], [0, T]], dtype=torch.int32).to(dev)
        out = {"counts": torch.empty((1, 8), dtype=torch.int32, device=dev), "out_vertex_offsets": torch.empty(2, dtype=torch.int32, device=dev),
               "out_triangle_offsets": torch.empty(2, dtype=torch.int32, device=dev)}
        common = (mesh.vertices.contiguous(), mesh.triangles.contiguous(), offsets[0], offsets[1], V, T)
        count = surface.weld_struct(*common, **out)
        size = C.c_size_t()
        _lib.check(lib.pr_mesh_weld_workspace_size(C.byref(count), C.byref(size)), "pr_mesh_weld_workspace_size")
        workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
        _lib.check(lib.pr_mesh_weld(C.byref(count), workspace.data_ptr(), size.value, stream), "pr_mesh_weld")
        out_v, out_t = int(out["out_vertex_offsets"][1]), int(out["out_triangle_offsets"][1])
        out.update(out_vertices=torch.empty((out_v, 3), device=dev), out_normals=torch.empty((out_v, 3), device=dev),
                   out_attributes=torch.empty((out_v, WIDTH), device=dev), out_triangles=torch.empty((out_t, 3), dtype=torch.int32, device=dev),
                   vertex_map=torch.empty(V, dtype=torch.int32, device=dev), triangle_map=torch.empty(T, dtype=torch.int32, device=dev))
        s = surface.weld_struct(*common, normals=mesh.normals.contiguous(), attributes=attributes, **out)
        keep = (offsets, mesh, common)
        run = lambda: (_lib.check(lib.pr_mesh_weld(C.byref(s), workspace.data_ptr(), size.value, stream), "pr_mesh_weld"), keep)[0]
        return run, out, size.value

    def by_hand(mesh, attributes):
        """torch.unique over the rows and the index arithmetic around it: one vertex per value (in sorted order, not the call's),
        triangles re-indexed, a == b / a == c dropped, unreferenced vertices compacted, rows gathered."""
        unique, inverse = torch.unique(mesh.vertices, dim=0, return_inverse=True)
        first = torch.full((unique.size(0),), mesh.vertices.size(0), dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, inverse, torch.arange(mesh.vertices.size(0), device=dev), "amin")      # the representative's row
        t = inverse[mesh.triangles.long()]
        t = t[(t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2])]
        used = torch.zeros(unique.size(0), dtype=torch.bool, device=dev)
        used[t.reshape(-1)] = True
        index = torch.cumsum(used, 0) - 1
        rows_kept = first[used]
        return unique[used], mesh.normals[rows_kept], attributes[rows_kept], index[t].to(torch.int32)

    with torch.no_grad():
        sigma, centres = comp.density_grid(object_idx, edge, style, deformation)
        axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
        level = float(sigma.flatten()[::max(1, edge ** 3 // (1 << 20))].median())
        capped, _ = surface.clean_lattice(sigma, level, close_border=True)
        lattice = centres.reshape(1, -1, 3).contiguous()
        report["lattice"] = {"edge": edge, "level": level}
        full = surface.extract_surface(capped, axes, level, normals=True)[0]
        if not trace:
            field = measure("fp32 density-only field query of the 128^3 lattice",
                            lambda: comp.query_object(object_idx, lattice, style, deformation, features=False)["sigma"])
            report["field_query_ms"] = field["call_ms_median"]
        for k in (0, 8, 4, 2):
            if trace and k != only:
                continue
            mesh = full if k == 0 else full.simplified(*surface.lattice_cluster_grid(axes, k), keep_duplicates=True)
            attributes = torch.randn((mesh.vertices.size(0), WIDTH), device=dev)
            run, out, workspace_bytes = weld_call(mesh, attributes)
            name = "unsimplified" if k == 0 else f"simplify {k}"
            if trace:
                for _ in range(calls):
                    run()
                torch.cuda.synchronize()
                print(name, out["counts"].tolist())
                continue
            row = measure(f"{name}: weld with normals, {WIDTH} attributes and both maps", run, simplify=k, vertices=mesh.vertices.size(0),
                          triangles=mesh.triangles.size(0), workspace_bytes=workspace_bytes)
            hand = measure(f"{name}: torch.unique and index arithmetic", lambda: by_hand(mesh, attributes), simplify=k)
            counts = out["counts"][0].tolist()
            entry = {"vertices": mesh.vertices.size(0), "triangles": mesh.triangles.size(0), "counts": counts, "workspace_bytes": workspace_bytes,
                     "weld_ms": row["call_ms_median"], "min": row["call_ms_min"], "max": row["call_ms_max"],
                     "share_of_the_field_query": round(row["call_ms_median"] / report["field_query_ms"], 4),
                     "within_10_percent": row["call_ms_median"] <= 0.1 * report["field_query_ms"],
                     "mvertices_per_s": round(mesh.vertices.size(0) / row["call_ms_median"] / 1e3, 1),
                     "torch_unique_ms": hand["call_ms_median"], "torch_unique_over_weld": round(hand["call_ms_median"] / row["call_ms_median"], 2),
                     "torch_unique_vertices": by_hand(mesh, attributes)[0].size(0)}
            again = {key: t.clone() for key, t in out.items()}
            run()
            torch.cuda.synchronize()
            entry["equal_bits_on_a_second_call"] = all(torch.equal(again[key].view(torch.int32), t.view(torch.int32)) for key, t in out.items())
            report["meshes"][name] = entry
            print(json.dumps({name: entry}), flush=True)
            save()
    save()


if __name__ == "__main__":
    main()
