#!/usr/bin/env python3
"""What retaining the static objects' per-sample state does to evaluation frames: writes profiles/retention_report.json.

Workloads (synthetic weights: randomize_module_state(seed=0, step=60000, alpha_bias=1.0, bender_scale=1e4), frame_replay = None):

    minecraft_256   shipped minecraft renderer, one 256 x 256 frame
    tennis_256      shipped tennis renderer, one 256 x 256 frame
    evaluator       shipped minecraft renderer, 288 x 512 frame, strided grids [4, 8] = 11 520 rays
    headline        bench.py's headline: tennis, 64 coarse + 128 resampled positions per ray, one 256 x 256 frame

each in fp32 and f16x3.  Variants, timed with device events, warmed, ALTERNATING in one process, --repeats frames each:

    off        composer.retained = None
    populate   retention on, the caches invalidated before the frame (every object rendered, keys stored)
    reuse      retention on, the players move between frames (two scenes that differ in the dynamic objects only)
    parent     (headline only, --parent-lib) `off` on a library built from the parent commit

beside the evaluated-sample counts, the per-category kernel times of pr_profile_collect and the cache size.

    make -C playableenvironments_amd/csrc
    python tools/retention_report.py [--parent-lib build/libplayrender_parent.so] [--workloads headline,evaluator]
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

NOT_MEASURED = "not measured"
WORKLOADS = ("minecraft_256", "tennis_256", "evaluator", "headline")


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
    ap.add_argument("--precisions", default="fp32,f16x3")
    ap.add_argument("--parent-lib", default=None, help="libplayrender.so built from the parent commit (headline: off against parent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retention_report.json"))
    args = ap.parse_args()

    from playableenvironments_amd import _lib, configs, synthetic
    from playableenvironments_amd.environment_model import EnvironmentModel
    import bench

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    current = _lib.load()
    parent = load_parent(args.parent_lib, _lib) if args.parent_lib else None
    with open(_lib.library_path(), "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()

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

    report = {"library_sha256": sha, "repeats": args.repeats, "workloads": {}}
    for name in [w for w in args.workloads.split(",") if w]:
        cfg, make_scene, size, extra = workload(name)
        torch.manual_seed(0)
        model = EnvironmentModel(cfg)
        synthetic.randomize_module_state(model.object_composer, seed=0, step=60000, alpha_bias=1.0, bender_scale=1e4)
        model.eval().to(dev)
        model.frame_replay = None
        comp = model.object_composer
        static = comp.object_id_helper.static_objects_count
        scene = bench.to_device(make_scene(seed=1234, image_size=size), dev)
        moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in scene.items()}
        moved["object_translation_parameters"][..., static:] += 0.05           # the players move, the camera stands still
        scenes = [scene, moved]
        retained = comp.retain_objects()
        entry = {"size": list(size), "retained_objects": list(retained.objects), "precisions": {}}

        def frame(s):
            with torch.no_grad():
                return model(*bench.scene_args(s, size), 0, False, mode="scene_encodings", **extra)

        counts = {}
        plain_forward = comp.forward

        def counting_forward(*a, **k):
            out = plain_forward(*a, **k, _export=True)
            for ty in ("coarse", "fine"):
                if ty in out:
                    counts[ty] = out[ty].pop("_samples")[0]["evaluated"].cpu().tolist()
            return out

        def counted(s):
            comp.forward = counting_forward
            try:
                frame(s)
            finally:
                del comp.forward
            torch.cuda.synchronize()
            return dict(counts)

        for precision in [p for p in args.precisions.split(",") if p]:
            comp.precision = precision
            turn = [0]

            def select(variant):
                _lib._LIB = parent if variant == "parent" else current
                comp.retained = None if variant in ("off", "parent") else retained
                if variant == "populate":
                    retained.invalidate()
                if variant == "reuse":                     # its own counter: the players move between consecutive reuse frames
                    turn[0] += 1
                    return scenes[turn[0] & 1]
                return scene

            variants = ["off", "populate", "reuse"] + (["parent"] if parent is not None and name == "headline" else [])
            comp.retained = retained
            frame(scene)                                   # allocates the cache, packs the weights, sizes the workspace
            for v in variants:
                for _ in range(args.warmup):
                    frame(select(v))
            torch.cuda.synchronize()
            times = {v: [] for v in variants}
            for _ in range(args.repeats):
                for v in variants:
                    s = select(v)
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    frame(s)
                    stop.record()
                    stop.synchronize()
                    times[v].append(start.elapsed_time(stop))
            # evaluated samples and the per-category kernel times of one frame per variant (untimed)
            evaluated, categories = {}, {}
            for v in variants:
                if v == "parent":
                    continue
                if v == "reuse":
                    frame(select("reuse"))                 # (the frame before: the cache holds the static objects)
                evaluated[v] = counted(select(v))
                s = select(v)
                current.pr_profile_enable(1)
                frame(s)
                ms, launches = bench.profile_arrays()
                current.pr_profile_collect(ms, launches)
                current.pr_profile_enable(0)
                categories[v] = {"milliseconds": [round(x, 3) for x in ms], "launches": list(launches)}     # (categories: include/playrender.h)
            _lib._LIB = current
            comp.retained = None
            result = {"variants": {v: spread(t) for v, t in times.items()}, "evaluated_samples": evaluated, "kernel_categories": categories,
                      "cache_bytes": retained.bytes}
            off = result["variants"]["off"]
            result["populate_minus_off_median_ms"] = round(result["variants"]["populate"]["median_ms"] - off["median_ms"], 3)
            result["speedup_reuse_vs_off"] = round(off["median_ms"] / result["variants"]["reuse"]["median_ms"], 4)
            if "parent" in times:
                p = result["variants"]["parent"]
                result["off_vs_parent"] = {"off_minus_parent_median_ms": round(off["median_ms"] - p["median_ms"], 3),
                                           "off_spread_ms": round(off["max_ms"] - off["min_ms"], 3),
                                           "parent_spread_ms": round(p["max_ms"] - p["min_ms"], 3),
                                           "within_parent_spread": abs(off["median_ms"] - p["median_ms"]) <= p["max_ms"] - p["min_ms"]}
            else:
                result["off_vs_parent"] = NOT_MEASURED
            entry["precisions"][precision] = result
            retained.clear()
            print(name, precision, json.dumps(result), flush=True)
        report["workloads"][name] = entry
        del model, comp, retained
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
