"""Timing of smoothing (GPU box): tennis player_1 at the benchmark scene's pose and codes, the 128^3 lattice of voxel centres, level =
the median in-box density, capped (close_border) - the set-up of perf_weld.py and its four meshes, WELDED.

pr_mesh_smooth with steps = 0 (lists + normals + CSR + state) and with steps = 20 (Taubin 0.5 / -0.53) of the unsimplified mesh and of
simplify = 8, 4, 2 with keep_duplicates=True, G = 1; beside it, in the same run, the fp32 density-only field query (query_object) of the
same 128^3 lattice, and the project's rule for a front or back end (applied in 20, 24 and 25): the steps = 0 call at most
10 % of that query.  The cost PER STEP is (steps = 20 - steps = 0) / 20, with its share of the HBM bandwidth from the bytes a step must
move: per movable vertex its list (4 k), the corners of its k triangles (12 k), its own position and the write (24); the 2 k
neighbour positions are counted once per vertex (12 V), as a cache that holds the mesh would deliver them.
Secondary, in the same run: what a user writes without the call - one Laplacian step with index_add_ over the directed edge list - as a
ratio to one step; its summation order differs (and it is not deterministic), so there is no threshold.

    python tools/perf/perf_smooth.py [timed calls, default 10] [report path, default profiles/smooth_report.json]

Protocol: three warm-up calls per configuration, HIP events around every timed call on preallocated outputs and workspace, medians
with min - max.  The feature has no parent to be measured against.  The report is rewritten after every mesh.

    python tools/perf/perf_smooth.py trace <simplify k or 0> <steps>
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

HBM_GB_PER_S = 8000.0                                                # MI355X: 8 TB/s peak
STEPS = 20


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
    only, only_steps = (int(sys.argv[2]), int(sys.argv[3])) if trace else (None, None)
    calls = 10 if trace or len(sys.argv) < 2 else int(sys.argv[1])
    report_path = "none" if trace else sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "smooth_report.json")
    if not torch.cuda.is_available():
        raise RuntimeError("perf_smooth.py measures on a GPU")
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
    report = {"device": torch.cuda.get_device_properties(0).name, "timed_calls": calls, "steps": STEPS, "meshes": {}, "rows": rows,
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

    def smooth_call(mesh, steps):
        """(run, outputs, workspace bytes) of the call with every output on preallocated tensors."""
        V, T = mesh.vertices.size(0), mesh.triangles.size(0)
        offsets = torch.tensor([[0, V], [0, T]], dtype=torch.int32).to(dev)
        out = {"out_vertices": torch.empty((V, 3), device=dev), "out_normals": torch.empty((V, 3), device=dev),
               "incidence_offsets": torch.empty(V + 1, dtype=torch.int32, device=dev), "incidence": torch.empty(3 * T, dtype=torch.int32, device=dev),
               "vertex_state": torch.empty(V, dtype=torch.int32, device=dev), "counts": torch.empty((1, 8), dtype=torch.int32, device=dev)}
        vertices, triangles = mesh.vertices.contiguous(), mesh.triangles.contiguous()
        s = surface.smooth_struct(vertices, triangles, offsets[0], offsets[1], V, T, out["out_vertices"], out["counts"], steps=steps,
                                  **{k: t for k, t in out.items() if k not in ("out_vertices", "counts")})
        size = C.c_size_t()
        _lib.check(lib.pr_mesh_smooth_workspace_size(C.byref(s), C.byref(size)), "pr_mesh_smooth_workspace_size")
        workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
        keep = (offsets, vertices, triangles)
        run = lambda: (_lib.check(lib.pr_mesh_smooth(C.byref(s), workspace.data_ptr(), size.value, stream), "pr_mesh_smooth"), keep)[0]
        return run, out, size.value

    def by_hand(mesh, edges):
        """One Laplacian step with index_add_ over the directed edges (a, b), (b, c), (c, a) of every triangle: on a closed manifold
        the same neighbours as the umbrella, each once; no border test, no mask, atomics in floating point."""
        v = mesh.vertices
        total = torch.zeros_like(v).index_add_(0, edges[0], v[edges[1]])
        degree = torch.zeros(v.size(0), device=dev).index_add_(0, edges[0], torch.ones(edges.size(1), device=dev))
        return v + 0.5 * (total / degree.clamp(min=1).unsqueeze(1) - v)

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
            mesh = (full if k == 0 else full.simplified(*surface.lattice_cluster_grid(axes, k), keep_duplicates=True)).welded()
            name = "unsimplified" if k == 0 else f"simplify {k}"
            if trace:
                run, out, _ = smooth_call(mesh, only_steps)
                for _ in range(calls):
                    run()
                torch.cuda.synchronize()
                print(name, out["counts"].tolist())
                continue
            V, T = mesh.vertices.size(0), mesh.triangles.size(0)
            run0, out0, workspace_bytes = smooth_call(mesh, 0)
            run20, out20, _ = smooth_call(mesh, STEPS)
            lists = measure(f"{name}: steps = 0 (lists, normals, CSR, state)", run0, simplify=k, vertices=V, triangles=T, workspace_bytes=workspace_bytes)
            smoothed = measure(f"{name}: steps = {STEPS}", run20, simplify=k)
            t = mesh.triangles.long()
            edges = torch.stack([torch.cat([t[:, 0], t[:, 1], t[:, 2]]), torch.cat([t[:, 1], t[:, 2], t[:, 0]])])
            hand = measure(f"{name}: one Laplacian step with index_add_", lambda: by_hand(mesh, edges), simplify=k)
            counts = out20["counts"][0].tolist()
            step_ms = (smoothed["call_ms_median"] - lists["call_ms_median"]) / STEPS
            entries = 3 * counts[0]                                   # list entries = sum of k
            step_bytes = 16 * entries + 24 * counts[2] + 12 * V
            entry = {"vertices": V, "triangles": T, "counts": counts, "workspace_bytes": workspace_bytes,
                     "steps_0_ms": lists["call_ms_median"], "min": lists["call_ms_min"], "max": lists["call_ms_max"],
                     "share_of_the_field_query": round(lists["call_ms_median"] / report["field_query_ms"], 4),
                     "within_10_percent": lists["call_ms_median"] <= 0.1 * report["field_query_ms"],
                     f"steps_{STEPS}_ms": smoothed["call_ms_median"], "per_step_us": round(step_ms * 1e3, 3), "per_step_bytes": step_bytes,
                     "per_step_share_of_hbm_bandwidth": round(step_bytes / max(step_ms, 1e-9) / 1e6 / HBM_GB_PER_S, 4),
                     "index_add_step_ms": hand["call_ms_median"], "index_add_step_over_one_step": round(hand["call_ms_median"] / max(step_ms, 1e-9), 2)}
            again = {key: x.clone() for key, x in out20.items()}
            run20()
            torch.cuda.synchronize()
            # (the header's one exception: the CSR segments of over-degree vertices hold the right set in an unspecified order)
            same = {key: torch.equal(again[key].view(torch.int32), x.view(torch.int32)) for key, x in out20.items()}
            entry["equal_bits_on_a_second_call"] = all(ok for key, ok in same.items() if key != "incidence" or counts[5] == 0)
            entry["incidence_equal_on_a_second_call"] = same["incidence"]
            report["meshes"][name] = entry
            print(json.dumps({name: entry}), flush=True)
            save()
    save()


if __name__ == "__main__":
    main()
