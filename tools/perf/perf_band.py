"""Timing of the band evaluation (GPU box): lattices of 128^3 and 256^3 points, stride 4, one guard cell, on two fields - a smooth ball
of radius 0.95 in [-1, 1]^3 through surface.refine_band's own calls with an analytic field, and tennis player_1 with synthetic weights at
the median in-box density.  Per field and size: the counting pr_band_plan call, the emitting one, pr_band_fill, the share of points
evaluated (skeleton + band), and the fp32 density-only query (ObjectComposer.query_object) of THAT MANY points.  Then, on player_1,
ObjectComposer.extract_mesh end to end at stride 4 against stride 0, at the median level and at the 0.99 quantile.

    python tools/perf/perf_band.py [timed calls, default 10] [report path, default none]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians with min - max; the shader clock is sampled
while each configuration runs.  The condition (DESIGN.md 12's rule): the two plan calls plus the fill call take at most 10 % of the
density-only query of the points the same call evaluated, measured in the same run.  Bytes moved (the model of DESIGN.md section 19),
reported against the 6.3 TB/s float4-copy figure, not gated: a counting call reads 32 B per cell and writes and reads back 2 B per cell
and 8 B per point block; the emitting call adds 16 B per band point; the fill reads 4 B per band point and writes 5 B per point."""
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

COPY_RATE_TBS = 6.3
STRIDE, GUARD = 4, 1


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
    report_path = sys.argv[2] if len(sys.argv) > 2 else None
    if not torch.cuda.is_available():
        raise RuntimeError("perf_band.py measures on a GPU")
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

    def measure(label, fn, edge, moved=None, **extra):
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
        if moved is not None:
            row["bytes_moved"] = int(moved)
            row["tb_per_s"] = round(moved / med / 1e9, 3)
            row["share_of_copy_rate"] = round(moved / med / 1e9 / COPY_RATE_TBS, 3)
        row.update(extra)
        if telemetry:
            row["clock"] = telemetry.summary(label)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return med

    def band_calls(name, edge, sigma, axes, level, evaluate, query_points):
        """Times the three library calls on a lattice whose skeleton is filled, and the density-only query of as many points as the
        skeleton and the band hold together (``query_points``: at least that many object-frame positions)."""
        P = edge ** 3
        skeleton = len(surface.skeleton_indices(edge, STRIDE)) ** 3
        point_offsets = torch.empty(2, dtype=torch.int32, device=dev)
        counts = torch.empty((1, 4), dtype=torch.int32, device=dev)
        count = surface.band_struct(sigma, axes, level, STRIDE, GUARD, point_offsets, counts)
        size = C.c_size_t()
        _lib.check(lib.pr_band_workspace_size(C.byref(count), C.byref(size)), "pr_band_workspace_size")
        workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
        launch = lambda fn, b: _lib.check(fn(C.byref(b), workspace.data_ptr(), size.value, stream), "pr_band")
        launch(lib.pr_band_plan, count)
        band = int(point_offsets[1])
        cells = int(counts[0, 0])
        positions = torch.empty((band, 3), dtype=torch.float32, device=dev)
        exact = torch.empty(sigma.shape, dtype=torch.uint8, device=dev)
        emit = surface.band_struct(sigma, axes, level, STRIDE, GUARD, point_offsets, counts, positions=positions)
        launch(lib.pr_band_plan, emit)
        values = evaluate(positions)
        fill = surface.band_struct(sigma, axes, level, STRIDE, GUARD, point_offsets, counts, values=values, exact=exact)
        sizes = dict(points=P, cells=cells, skeleton_points=skeleton, band_points=band, counts=counts[0].tolist(),
                     share_evaluated=round((skeleton + band) / P, 4), workspace_bytes=size.value)
        blocks = (P + 255) // 256
        count_ms = measure(f"{name} {edge}^3 plan, counting", lambda: launch(lib.pr_band_plan, count), edge, moved=34 * cells + 8 * blocks, **sizes)
        emit_ms = measure(f"{name} {edge}^3 plan, emitting", lambda: launch(lib.pr_band_plan, emit), edge,
                          moved=34 * cells + 8 * blocks + 16 * band, **sizes)
        fill_ms = measure(f"{name} {edge}^3 fill", lambda: launch(lib.pr_band_fill, fill), edge, moved=4 * band + 5 * P, **sizes)
        evaluated = skeleton + band
        pts = query_points[:evaluated]
        query_ms = measure(f"{name} {edge}^3 fp32 density-only query of the {evaluated} evaluated points",
                           lambda: comp.query_object(object_idx, pts, style[0], deformation[0], features=False), edge, **sizes)
        total = count_ms + emit_ms + fill_ms
        return {"plan_count_ms": round(count_ms, 4), "plan_emit_ms": round(emit_ms, 4), "fill_ms": round(fill_ms, 4),
                "band_calls_ms": round(total, 4), "density_only_query_ms": round(query_ms, 4), "evaluated_points": evaluated,
                "share_evaluated": sizes["share_evaluated"], "share": round(total / query_ms, 5), "condition_at_most": 0.10,
                "met": bool(total <= 0.10 * query_ms)}

    verdicts, end_to_end = {}, {}
    with torch.no_grad():
        for edge in (128, 256):
            n = [edge] * 3
            P = edge ** 3
            axes = comp._grid_axes(object_idx, n, False, dev)
            centres = comp._grid_centres(object_idx, n, False, dev).reshape(-1, 3)
            # a smooth ball of radius 0.95 in the lattice's own [-1, 1]^3 coordinates
            unit = [torch.linspace(-1, 1, edge, device=dev)] * 3
            ball = lambda p: 0.95 ** 2 - (p * p).sum(-1)
            sigma = ball(torch.stack(torch.meshgrid(*unit, indexing="ij"), dim=-1)).reshape(1, edge, edge, edge).contiguous()
            verdicts[f"ball {edge}^3"] = band_calls("ball", edge, sigma, unit, 0.0, ball, centres)
            # player_1, synthetic weights, level = the median density
            dense, _ = comp.density_grid(object_idx, edge, style, deformation)
            sub = dense.flatten()[::max(1, P // (1 << 20))]
            median, high = float(sub.median()), float(sub.quantile(0.99))
            lookup = lambda p: comp.query_object(object_idx, p, style[0], deformation[0], features=False)["sigma"]
            verdicts[f"player_1 {edge}^3"] = band_calls("player_1", edge, dense.clone(), axes, median, lookup, centres)
            del dense, sigma
            for label, level in (("median", median), ("0.99 quantile", high)):
                kw = dict(level=level, normals=True)
                dense_ms = measure(f"player_1 {edge}^3 extract_mesh stride 0, {label} level",
                                   lambda: comp.extract_mesh(object_idx, edge, style, deformation, **kw), edge, level=level)
                band_ms = measure(f"player_1 {edge}^3 extract_mesh stride {STRIDE}, {label} level",
                                  lambda: comp.extract_mesh(object_idx, edge, style, deformation, stride=STRIDE, guard=GUARD, **kw), edge, level=level)
                counts = comp.density_band(object_idx, edge, style, deformation, level=level, stride=STRIDE, guard=GUARD)[3][0].tolist()
                a = comp.extract_mesh(object_idx, edge, style, deformation, **kw)[0]
                b = comp.extract_mesh(object_idx, edge, style, deformation, stride=STRIDE, guard=GUARD, **kw)[0]
                end_to_end[f"player_1 {edge}^3 {label}"] = {
                    "level": level, "stride_0_ms": round(dense_ms, 3), f"stride_{STRIDE}_ms": round(band_ms, 3), "ratio": round(band_ms / dense_ms, 4),
                    "counts": counts, "share_evaluated": round((len(surface.skeleton_indices(edge, STRIDE)) ** 3 + counts[3]) / P, 4),
                    "vertices_stride_0": a.vertices.size(0), f"vertices_stride_{STRIDE}": b.vertices.size(0),
                    "same_mesh": bool(a.vertices.shape == b.vertices.shape and torch.equal(a.vertices, b.vertices)
                                      and torch.equal(a.triangles, b.triangles))}
                print(json.dumps(end_to_end[f"player_1 {edge}^3 {label}"]), flush=True)
    if telemetry:
        telemetry.finish()
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    report = {"device": props.name, "library_sha256": sha, "timed_calls": calls, "stride": STRIDE, "guard": GUARD,
              "copy_rate_tb_per_s": COPY_RATE_TBS, "rows": rows, "condition": verdicts, "end_to_end": end_to_end}
    print(json.dumps(report["condition"]))
    if report_path:
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
