"""Timing of the mesh simplification (GPU box): tennis player_1, lattices of 128^3 and 256^3 voxel centres, level = the median in-box
density (the set-up of perf_surface.py) - the fp32 density-only query that fills the lattice, the mesh of the lattice, and for
simplify = 2, 4, 8 (the lattice-aligned cluster grids of surface.lattice_cluster_grid) the count-only pr_simplify_mesh call and the
emitting call with normals, with the V and T reduction and the shader clock.

    python tools/perf/perf_simplify.py [timed calls, default 10] [report path, default none] [edges, default 128,256]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians with min - max; the shader clock is
sampled while each configuration runs.  The condition (DESIGN.md section 12's rule for a front or back end): the emitting call takes
at most 10 % of the density-only query of the same lattice, measured in the same run."""
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
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    report_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "none" else None
    edges = [int(e) for e in (sys.argv[3] if len(sys.argv) > 3 else "128,256").split(",")]
    if not torch.cuda.is_available():
        raise RuntimeError("perf_simplify.py measures on a GPU")
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

    def measure(label, fn, edge, **extra):
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

    verdicts = {}
    with torch.no_grad():
        for edge in edges:
            P = edge ** 3
            query_ms = measure(f"{edge}^3 fp32 density-only query", lambda: comp.density_grid(object_idx, edge, style, deformation), edge)
            sigma, _ = comp.density_grid(object_idx, edge, style, deformation)
            axes = comp._grid_axes(object_idx, [edge] * 3, False, dev)
            level = float(sigma.flatten()[::max(1, P // (1 << 20))].median())         # (median of a 1 M point subsample)
            mesh = surface.extract_surface(sigma, axes, level)[0]
            del sigma
            V, T = mesh.vertices.size(0), mesh.triangles.size(0)
            offsets_in = torch.tensor([[0, V], [0, T]], dtype=torch.int32, device=dev)
            for k in (2, 4, 8):
                grid = surface.lattice_cluster_grid(axes, k)
                offsets = torch.empty((2, 2), dtype=torch.int32, device=dev)
                counts = torch.empty((1, 4), dtype=torch.int32, device=dev)
                common = (mesh.vertices, mesh.triangles, offsets_in[0], offsets_in[1], V, T, *grid, counts, offsets[0], offsets[1])
                count = surface.simplify_struct(*common, normals=mesh.normals)
                size = C.c_size_t()
                _lib.check(lib.pr_simplify_workspace_size(C.byref(count), C.byref(size)), "pr_simplify_workspace_size")
                workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
                launch = lambda s: _lib.check(lib.pr_simplify_mesh(C.byref(s), workspace.data_ptr(), size.value, stream), "pr_simplify_mesh")
                launch(count)
                out_V, out_T = int(offsets[0, 1]), int(offsets[1, 1])
                clusters, proper, kept, outside = counts[0].tolist()
                out_v = torch.empty((out_V, 3), dtype=torch.float32, device=dev)
                out_n = torch.empty((out_V, 3), dtype=torch.float32, device=dev)
                out_t = torch.empty((max(out_T, 1), 3), dtype=torch.int32, device=dev)
                emit = surface.simplify_struct(*common, normals=mesh.normals, out_vertices=out_v, out_normals=out_n, out_triangles=out_t)
                sizes = dict(points=P, level=level, simplify=k, cells=grid[2], vertices_in=V, triangles_in=T, vertices_out=out_V,
                             triangles_out=out_T, non_degenerate_triangles=proper, vertex_reduction=round(V / max(out_V, 1), 2),
                             triangle_reduction=round(T / max(out_T, 1), 2), workspace_bytes=size.value)
                count_ms = measure(f"{edge}^3 simplify {k} count-only", lambda: launch(count), edge, **sizes)
                emit_ms = measure(f"{edge}^3 simplify {k} emit with normals", lambda: launch(emit), edge, **sizes)
                verdicts[f"{edge}^3 simplify {k}"] = {"count_only_ms": round(count_ms, 4), "emit_ms": round(emit_ms, 4),
                                                      "density_only_query_ms": round(query_ms, 4), "share": round(emit_ms / query_ms, 5),
                                                      "condition_at_most": 0.10, "met": bool(emit_ms <= 0.10 * query_ms)}
                del workspace, out_v, out_n, out_t
            del mesh
    if telemetry:
        telemetry.finish()
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    report = {"device": props.name, "library_sha256": sha, "timed_calls": calls, "rows": rows, "condition": verdicts}
    print(json.dumps(report["condition"]))
    if report_path:
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
