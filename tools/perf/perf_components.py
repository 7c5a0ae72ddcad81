"""Timing of the component labelling (GPU box): lattices of 128^3 and 256^3 points, G = 1, two fields that stress opposite ends -
the fp32 density_grid of tennis player_1 with synthetic weights at its median (noise-like: very many components, many selection
candidates) and a smooth ball that fills most of the lattice (one huge component: the deepest union chains, the most contended root) -
each as labels only (labels + sizes), the full clean with keep_largest = 1 and with keep_largest = 8 (sigma_out only), beside the fp32
density-only query that fills the lattice.

    python tools/perf/perf_components.py [timed calls, default 10] [report path, default none]

Protocol (that of perf_surface.py): three warm-up calls per configuration, HIP events around every timed call, medians with
min - max; the shader clock is sampled while each configuration runs.  Bytes moved (the model of DESIGN.md section 18), per point:
init 4 read + 8 written, merge 4 read, flatten 4 read + 4 written, every selection pass 4 read, write 8 read (label and its root's
size) plus 4 per output written and 4 more read for sigma_out: 36 B labels only, 40 + 4 keep_largest B for a clean.  The merge
kernel's neighbour reads and atomics are served by the caches and are not in the model.  The condition: the full clean takes at most
10 % of the density-only query of the same lattice, measured in the same run.  The achieved bandwidth is reported against the
6.3 TB/s float4-copy figure, not gated."""
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
        raise RuntimeError("perf_components.py measures on a GPU")
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

    verdicts = {}
    with torch.no_grad():
        for edge in (128, 256):
            P = edge ** 3
            query_ms = measure(f"{edge}^3 fp32 density-only query", lambda: comp.density_grid(object_idx, edge, style, deformation), edge)
            field, _ = comp.density_grid(object_idx, edge, style, deformation)
            x = torch.linspace(-1, 1, edge, device=dev)
            ball = (0.95 ** 2 - x[:, None, None] ** 2 - x[None, :, None] ** 2 - x[None, None, :] ** 2)[None].contiguous()
            median = float(field.flatten()[::max(1, P // (1 << 20))].median())         # (median of a 1 M point subsample)
            labels = torch.empty((1, edge, edge, edge), dtype=torch.int32, device=dev)
            sizes = torch.empty_like(labels)
            out = torch.empty((1, edge, edge, edge), dtype=torch.float32, device=dev)
            counts = torch.empty((1, 4), dtype=torch.int32, device=dev)
            for name, sigma, level in (("player_1 at its median", field, median), ("ball", ball, 0.0)):
                structs = {"labels only": (surface.components_struct(sigma, level, counts, labels=labels, sizes=sizes), 36 * P),
                           "clean keep_largest=1": (surface.components_struct(sigma, level, counts, sigma_out=out, keep_largest=1), 44 * P),
                           "clean keep_largest=8": (surface.components_struct(sigma, level, counts, sigma_out=out, keep_largest=8), 72 * P)}
                size = C.c_size_t()
                _lib.check(lib.pr_components_workspace_size(C.byref(structs["labels only"][0]), C.byref(size)), "pr_components_workspace_size")
                workspace = torch.empty(size.value, dtype=torch.uint8, device=dev)
                launch = lambda c: _lib.check(lib.pr_label_components(C.byref(c), workspace.data_ptr(), size.value, stream), "pr_label_components")
                for what, (c, moved) in structs.items():
                    ms = measure(f"{edge}^3 {name}: {what}", lambda: launch(c), edge, moved=moved, level=level, workspace_bytes=size.value)
                    inside, components, kept, kept_points = counts.cpu().tolist()[0]
                    rows[-1].update(inside_points=inside, components=components, kept_components=kept, kept_points=kept_points)
                    if what != "labels only":
                        verdicts[f"{edge}^3 {name}: {what}"] = {"clean_ms": round(ms, 4), "density_only_query_ms": round(query_ms, 4),
                                                                "share": round(ms / query_ms, 5), "condition_at_most": 0.10,
                                                                "met": bool(ms <= 0.10 * query_ms)}
                del workspace
            del field, ball, labels, sizes, out
    if telemetry:
        telemetry.finish()
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    report = {"device": props.name, "library_sha256": sha, "timed_calls": calls, "copy_rate_tb_per_s": COPY_RATE_TBS, "rows": rows,
              "condition": verdicts}
    print(json.dumps(report["condition"]))
    if report_path:
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
