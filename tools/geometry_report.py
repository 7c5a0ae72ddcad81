#!/usr/bin/env python3
"""What a geometry-only render (ObjectComposer.render_geometry, pr_render_geometry) costs against the full render: writes
profiles/geometry_report.json.

Workloads (synthetic weights: randomize_module_state(seed=0, step=60000, alpha_bias=1.0, bender_scale=1e4), frame_replay = None):

    headline        bench.py's headline: tennis, 64 coarse + 128 resampled positions per ray, one 256 x 256 frame
    tennis_256      shipped tennis renderer, one 256 x 256 frame
    minecraft_256   shipped minecraft renderer, one 256 x 256 frame
    evaluator       shipped minecraft renderer, 288 x 512 frame, strided grids [4, 8] = 11 520 rays: the full render only, against
                    the parent commit's library (--parent-lib)

the headline in fp32 and f16x3, the others in fp32 (--precisions applies to all).  Variants, timed with device events, warmed,
ALTERNATING in one process, --repeats frames each, medians with min - max, the shader clock of the measured frames beside each:

    full           EnvironmentModel.render_full_frame_from_scene_encoding (the evaluator: the strided scene-encoding call)
    geometry       EnvironmentModel.render_geometry_from_scene_encoding
    parent_a / _b  (headline and evaluator, --parent-lib) `full` on a library built from the parent commit, twice per round: the
                   spread of two runs of the same library in the same process order is the noise margin of `full` against the parent

beside the per-category kernel times of pr_profile_collect (0 = MLP, 1 = compositing) of one frame per variant and the workspace
bytes pr_workspace_size asks for with and without PR_FLAG_GEOMETRY_ONLY.

    make -C playableenvironments_amd/csrc
    python tools/geometry_report.py [--parent-lib build/libplayrender_parent.so] [--workloads headline,evaluator]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOT_MEASURED = "not measured"
WORKLOADS = ("headline", "tennis_256", "minecraft_256", "evaluator")


def spread(values):
    return {"median_ms": round(statistics.median(values), 3), "min_ms": round(min(values), 3), "max_ms": round(max(values), 3),
            "repeats": len(values)}


def load_parent(path, _lib):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--precisions", default=None, help="default: fp32,f16x3 for the headline, fp32 for the other workloads")
    ap.add_argument("--parent-lib", default=None, help="libplayrender.so built from the parent commit (headline, evaluator: full against parent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_report.json"))
    args = ap.parse_args()

    from playableenvironments_amd import _lib, configs, synthetic
    from playableenvironments_amd.environment_model import EnvironmentModel
    import bench
    import gpu_telemetry

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    current = _lib.load()
    parent = load_parent(args.parent_lib, _lib) if args.parent_lib else None
    with open(_lib.library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    props = torch.cuda.get_device_properties(dev)
    card = gpu_telemetry.card_of_pci_address(props.pci_domain_id, props.pci_bus_id, props.pci_device_id)      # (None: no clock column)

    def workload(name):
        if name == "headline":
            return configs.tennis_config(hierarchical=(64, 128)), synthetic.tennis_scene, (256, 256), {}
        if name == "tennis_256":
            return configs.tennis_config(), synthetic.tennis_scene, (256, 256), {}
        if name == "minecraft_256":
            return configs.minecraft_config(), synthetic.minecraft_scene, (256, 256), {}
        if name == "evaluator":
            return configs.minecraft_config(), synthetic.minecraft_scene, (288, 512), {"patch_stride": [4, 8]}
        raise SystemExit(f"unknown workload {name!r} (expected one of {WORKLOADS})")

    report = {"library_sha256": sha, "repeats": args.repeats, "parent_library": bool(parent), "workloads": {}}
    for name in [w for w in args.workloads.split(",") if w]:
        cfg, make_scene, size, extra = workload(name)
        torch.manual_seed(0)
        model = EnvironmentModel(cfg)
        synthetic.randomize_module_state(model.object_composer, seed=0, step=60000, alpha_bias=1.0, bender_scale=1e4)
        model.eval().to(dev)
        model.frame_replay = None
        comp = model.object_composer
        scene = bench.to_device(make_scene(seed=1234, image_size=size), dev)
        scene_args = bench.scene_args(scene, size)
        entry = {"size": list(size), "precisions": {}}
        strided = bool(extra)
        if strided:
            entry["note"] = "strided grids: the full render against the parent commit only (the geometry entry renders whole frames)"

        def full_frame():
            with torch.no_grad():
                if strided:
                    return model(*scene_args, 0, False, mode="scene_encodings", **extra)
                return model.render_full_frame_from_scene_encoding(*scene_args, False)

        def geometry_frame():
            return model.render_geometry_from_scene_encoding(*scene_args)

        def workspace_sizes():
            """pr_workspace_size of the frame's renderer call with and without the geometry flag (the flags of an evaluation frame)"""
            sizes = {}
            seen = {}
            plain = comp._render

            def spy(*a, **k):
                out = plain(*a, **k)
                seen["geometry" if k.get("_geometry") else "full"] = int(comp._workspace.numel())
                return out

            for which, frame in (("geometry", geometry_frame), ("full", full_frame)):
                if which == "geometry" and strided:
                    continue
                comp._workspace = None
                comp._render = spy
                try:
                    frame()
                finally:
                    del comp._render
                torch.cuda.synchronize()
                sizes[which + "_bytes"] = seen.get(which, NOT_MEASURED)
            return sizes

        precisions = args.precisions.split(",") if args.precisions else (["fp32", "f16x3"] if name == "headline" else ["fp32"])
        for precision in [p for p in precisions if p]:
            comp.precision = precision

            def run(variant):
                _lib._LIB = parent if variant.startswith("parent") else current
                return geometry_frame() if variant == "geometry" else full_frame()

            variants = ["full"] + ([] if strided else ["geometry"])
            if parent is not None and name in ("headline", "evaluator"):
                variants += ["parent_a", "parent_b"]
            for v in variants:
                for _ in range(args.warmup):
                    run(v)
            torch.cuda.synchronize()
            telemetry = gpu_telemetry.Telemetry(card) if card else None
            if telemetry:
                telemetry.start()
            times = {v: [] for v in variants}
            for _ in range(args.repeats):
                for v in variants:
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    if telemetry:
                        telemetry.label = v
                    start.record()
                    run(v)
                    stop.record()
                    stop.synchronize()
                    if telemetry:
                        telemetry.label = None
                    times[v].append(start.elapsed_time(stop))
            if telemetry:
                telemetry.finish()
            _lib._LIB = current
            categories = {}
            for v in variants:
                if v.startswith("parent"):
                    continue
                current.pr_profile_enable(1)
                run(v)
                ms, launches = bench.profile_arrays()
                current.pr_profile_collect(ms, launches)
                current.pr_profile_enable(0)
                categories[v] = {"mlp_ms": round(ms[0], 3), "composite_ms": round(ms[1], 3), "milliseconds": [round(x, 3) for x in ms],
                                 "launches": list(launches)}     # (categories: include/playrender.h)
            result = {"variants": {}, "kernel_categories": categories, "workspace": workspace_sizes()}
            for v, t in times.items():
                result["variants"][v] = spread(t)
                clock = telemetry.summary(v) if telemetry else {}
                result["variants"][v]["sclk_mhz"] = clock.get("sclk_mhz", NOT_MEASURED)
                result["variants"][v]["sclk_samples"] = clock.get("samples", 0)
            full = result["variants"]["full"]
            if "geometry" in times:
                result["speedup_geometry_vs_full"] = round(full["median_ms"] / result["variants"]["geometry"]["median_ms"], 4)
                result["mlp_ms_geometry_over_full"] = round(categories["geometry"]["mlp_ms"] / categories["full"]["mlp_ms"], 4) \
                    if categories["full"]["mlp_ms"] > 0 else NOT_MEASURED
                ws = result["workspace"]
                if isinstance(ws.get("geometry_bytes"), int) and isinstance(ws.get("full_bytes"), int):
                    ws["geometry_over_full"] = round(ws["geometry_bytes"] / ws["full_bytes"], 4)
            else:
                result["speedup_geometry_vs_full"] = result["mlp_ms_geometry_over_full"] = NOT_MEASURED
            if "parent_a" in times:
                a, b = result["variants"]["parent_a"], result["variants"]["parent_b"]
                both = times["parent_a"] + times["parent_b"]
                lo, hi = min(a["median_ms"], b["median_ms"]), max(a["median_ms"], b["median_ms"])
                result["full_vs_parent"] = {"full_median_ms": full["median_ms"], "parent_a_median_ms": a["median_ms"],
                                            "parent_b_median_ms": b["median_ms"], "parent_medians_differ_by_ms": round(hi - lo, 3),
                                            "parent_frames_min_max_ms": [round(min(both), 3), round(max(both), 3)],
                                            "full_minus_nearer_parent_median_ms": round(min(full["median_ms"] - a["median_ms"],
                                                                                            full["median_ms"] - b["median_ms"], key=abs), 3),
                                            "within_spread_of_the_two_parent_runs": min(both) <= full["median_ms"] <= max(both)}
            else:
                result["full_vs_parent"] = NOT_MEASURED
            entry["precisions"][precision] = result
            print(name, precision, json.dumps(result), flush=True)
        report["workloads"][name] = entry
        del model, comp
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
