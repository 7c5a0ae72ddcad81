"""Timing and effect of the quadric placement (GPU box): tennis player_1, the lattice of 128^3 voxel centres, level = the median in-box
density (the set-up of perf_simplify.py), simplify = 2, 4, 8 - the pr_mesh_place call against two yardsticks of the same run, the
emitting pr_simplify_mesh call on the same mesh and the fp32 density-only query that fills the lattice (DESIGN.md section 12's rule:
at most 10 % of it), and per level, for the mean and the quadric placement from the device meshes: audit().report() (area, volume),
compare_meshes against the unsimplified mesh (mean, rms, max, both directions), self_intersections() and the placement's counts.

    python tools/perf/perf_place.py [timed calls, default 20] [report path, default none] [edge, default 128]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians with min - max; the shader clock is
sampled while each configuration runs."""
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_telemetry  # noqa: E402
from playableenvironments_amd import ObjectComposer, _lib, configs, surface, synthetic  # noqa: E402


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
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    report_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "none" else None
    edge = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    if not torch.cuda.is_available():
        raise RuntimeError("perf_place.py measures on a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cfg = configs.tennis_config()
    object_idx = 2                                                   # player_1: NeRF + ray bender
    model_cfg = cfg["model"]["object_models"][object_idx]
    torch.manual_seed(0)
    comp = ObjectComposer(cfg)
    synthetic.randomize_module_state(comp, seed=0, step=20000, bender_scale=1e4)
    comp.eval().to(dev)
    comp.precision = "fp32"
    g = torch.Generator().manual_seed(1)
    style = torch.randn((1, model_cfg["style_features"]), generator=g).to(dev)
    deformation = torch.randn((1, model_cfg["deformation_features"]), generator=g).to(dev)
    props = torch.cuda.get_device_properties(0)
    card = gpu_telemetry.card_of_pci_address(props.pci_domain_id, props.pci_bus_id, props.pci_device_id)       # (None: no clock column)
    telemetry = gpu_telemetry.Telemetry(card) if card else None
    if telemetry:
        telemetry.start()
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []

    def measure(label, fn, **extra):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if telemetry:
            telemetry.label = label
        ms = timed(fn, calls)
        if telemetry:
            telemetry.label = None
        med = statistics.median(ms)
        row = {"config": label, "edge": edge, "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4), "call_ms_max": round(max(ms), 4)}
        row.update(extra)
        if telemetry:
            row["clock"] = telemetry.summary(label)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return med

    def quality(mesh, fine, max_distance):
        audit = mesh.audit().report()
        deviation = surface.compare_meshes(mesh, fine, samples=1 << 18, seed=7, max_distance=max_distance).report()
        side = lambda d: {k: d[k] for k in ("samples", "misses", "mean", "rms", "max")}
        return {"area": audit["area"], "signed_volume": audit["signed_volume"], "balanced": audit["balanced"], "shells": audit["shells"],
                "to_unsimplified": side(deviation["a_to_b"]), "from_unsimplified": side(deviation["b_to_a"]),
                "self_intersecting_pairs": mesh.self_intersections().report()["pairs"]}

    verdicts, meshes = {}, {}
    with torch.no_grad():
        query_ms = measure(f"{edge}^3 fp32 density-only query", lambda: comp.density_grid(object_idx, edge, style, deformation))
        sigma, _ = comp.density_grid(object_idx, edge, style, deformation)
        axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
        level = float(sigma.flatten()[::max(1, edge ** 3 // (1 << 20))].median())         # (median of a 1 M point subsample)
        fine = surface.extract_surface(sigma, axes, level)[0]
        del sigma
        V, T = fine.vertices.size(0), fine.triangles.size(0)
        fine_audit = fine.audit().report()
        meshes["unsimplified"] = {"vertices": V, "triangles": T, "area": fine_audit["area"], "signed_volume": fine_audit["signed_volume"],
                                  "self_intersecting_pairs": fine.self_intersections().report()["pairs"]}
        print(json.dumps(meshes["unsimplified"]), flush=True)
        offsets_in = torch.tensor([[0, V], [0, T]], dtype=torch.int32, device=dev)
        for k in (2, 4, 8):
            origin, cell, cells = surface.lattice_cluster_grid(axes, k)
            offsets = torch.empty((2, 2), dtype=torch.int32, device=dev)
            counts = torch.empty((1, 4), dtype=torch.int32, device=dev)
            common = (fine.vertices, fine.triangles, offsets_in[0], offsets_in[1], V, T, origin, cell, cells, counts, offsets[0], offsets[1])
            count = surface.simplify_struct(*common, normals=fine.normals)
            size = C.c_size_t()
            _lib.check(lib.pr_simplify_workspace_size(C.byref(count), C.byref(size)), "pr_simplify_workspace_size")
            workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
            _lib.check(lib.pr_simplify_mesh(C.byref(count), workspace.data_ptr(), size.value, stream), "pr_simplify_mesh")
            VO, TO = int(offsets[0, 1]), int(offsets[1, 1])
            out_v = torch.empty((VO, 3), dtype=torch.float32, device=dev)
            out_n = torch.empty((VO, 3), dtype=torch.float32, device=dev)
            out_t = torch.empty((max(TO, 1), 3), dtype=torch.int32, device=dev)
            vertex_map = torch.empty(V, dtype=torch.int32, device=dev)
            emit = surface.simplify_struct(*common, normals=fine.normals, out_vertices=out_v, out_normals=out_n, out_triangles=out_t,
                                           vertex_map=vertex_map)
            simplify = lambda: _lib.check(lib.pr_simplify_mesh(C.byref(emit), workspace.data_ptr(), size.value, stream), "pr_simplify_mesh")
            simplify()
            placed = torch.empty_like(out_v)
            place_counts = torch.empty((1, _lib.PLACE_COUNTS), dtype=torch.int32, device=dev)
            s = surface.place_struct(fine.vertices, fine.triangles, offsets_in[0], offsets_in[1], V, T, vertex_map, out_v, offsets[0], VO,
                                     placed, place_counts, scale=max(cell), max_move=cell, merged_triangles=out_t,
                                     merged_triangle_offsets=offsets[1], total_merged_triangles=TO)
            place_size = C.c_size_t()
            _lib.check(lib.pr_mesh_place_workspace_size(C.byref(s), C.byref(place_size)), "pr_mesh_place_workspace_size")
            place_workspace = torch.empty(place_size.value, dtype=torch.uint8, device=dev)
            place = lambda: _lib.check(lib.pr_mesh_place(C.byref(s), place_workspace.data_ptr(), place_size.value, stream), "pr_mesh_place")
            sizes = dict(simplify=k, cells=cells, vertices_in=V, triangles_in=T, vertices_out=VO, triangles_out=TO)
            simplify_ms = measure(f"{edge}^3 simplify {k} emit with normals and the vertex map", simplify, **sizes)
            place_ms = measure(f"{edge}^3 simplify {k} pr_mesh_place", place, workspace_bytes=place_size.value, **sizes)
            moved, kept, skipped, turned = place_counts[0].tolist()
            verdicts[f"{edge}^3 simplify {k}"] = {"place_ms": round(place_ms, 4), "simplify_emit_ms": round(simplify_ms, 4),
                                                  "share_of_simplify": round(place_ms / simplify_ms, 4),
                                                  "density_only_query_ms": round(query_ms, 4), "share_of_query": round(place_ms / query_ms, 5),
                                                  "condition_at_most": 0.10, "met": bool(place_ms <= 0.10 * query_ms)}
            mean = surface.Mesh(out_v, out_t[:TO], out_n)
            quadric = surface.Mesh(placed, out_t[:TO], out_n)
            max_distance = 2 * max(cell)
            meshes[f"simplify {k}"] = {"vertices": VO, "triangles": TO, "cell": cell, "moved": moved, "kept": kept,
                                       "skipped_or_invalid": skipped, "turned": turned, "mean": quality(mean, fine, max_distance),
                                       "quadric": quality(quadric, fine, max_distance)}
            print(json.dumps(meshes[f"simplify {k}"]), flush=True)
            del workspace, place_workspace
    if telemetry:
        telemetry.finish()
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    report = {"device": props.name, "library_sha256": sha, "timed_calls": calls, "rows": rows, "condition": verdicts, "meshes": meshes}
    print(json.dumps(report["condition"]))
    if report_path:
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
