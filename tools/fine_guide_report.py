#!/usr/bin/env python3
"""What the fine guide (composer.fine_guide, pr_render_forward_guided) does to evaluation frames: writes profiles/fine_guide_report.json.

Workloads (synthetic weights: randomize_module_state(seed=0, step=60000, alpha_bias=1.0, bender_scale=1e4), frame_replay = None):

    headline        bench.py's headline: tennis, 64 coarse + 128 resampled positions per ray, one 256 x 256 frame
    tennis_fine     the tennis renderer at its shipped position counts (4 + 4, 32 + 32) with the fine pass on, one 256 x 256 frame
    tennis_256      shipped tennis renderer, one 256 x 256 frame      } no fine pass in the shipped configuration: the guide has
    minecraft_256   shipped minecraft renderer, one 256 x 256 frame   } nothing to act on, only `off` is timed
    evaluator       shipped minecraft renderer, 288 x 512 frame, strided grids [4, 8] = 11 520 rays (no fine pass: off against parent)

each in fp32 and f16x3.  Variants, timed with device events, warmed, ALTERNATING in one process, --repeats frames each:

    off            composer.fine_guide = None
    guide          FineGuide() at its defaults (threshold 0.0, guard 1, every object with a fine model)
    guide_reuse    the guide plus retention of the static objects, the players moving between frames
    parent_a / _b  (headline and evaluator, --parent-lib) `off` on a library built from the parent commit, twice per round: the
                   spread of two runs of the same library in the same session

beside the evaluated-sample counts of the fine level, the per-category kernel times of pr_profile_collect (0 = MLP, 6 = k_resample
with its block-sum fill, 7 = k_fill) and the PSNR of the fine global integrated_features, guide against off - with the synthetic
weights as they are (coarse and fine fields unrelated: the worst case) and with the coarse weights copied into the fine models.

    make -C playableenvironments_amd/csrc
    python tools/fine_guide_report.py [--parent-lib build/libplayrender_parent.so] [--workloads headline,evaluator]
"""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOT_MEASURED = "not measured"
WORKLOADS = ("headline", "tennis_fine", "tennis_256", "minecraft_256", "evaluator")


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


def psnr(reference, other):
    mse = float(((reference.double() - other.double()) ** 2).mean())
    peak = float(reference.double().abs().max())
    if mse == 0.0:
        return "identical"
    return round(10.0 * math.log10(peak * peak / mse), 2) if peak > 0 else NOT_MEASURED


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--precisions", default="fp32,f16x3")
    ap.add_argument("--parent-lib", default=None, help="libplayrender.so built from the parent commit (headline, evaluator: off against parent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_guide_report.json"))
    args = ap.parse_args()

    from playableenvironments_amd import _lib, configs, synthetic
    from playableenvironments_amd.environment_model import EnvironmentModel
    from playableenvironments_amd.guidance import FineGuide
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
        if name == "tennis_fine":
            return configs.enable_fine(configs.tennis_config()), synthetic.tennis_scene, (256, 256), {}
        if name == "tennis_256":
            return configs.tennis_config(), synthetic.tennis_scene, (256, 256), {}
        if name == "minecraft_256":
            return configs.minecraft_config(), synthetic.minecraft_scene, (256, 256), {}
        if name == "evaluator":
            return configs.minecraft_config(), synthetic.minecraft_scene, (288, 512), {"patch_stride": [4, 8]}
        raise SystemExit(f"unknown workload {name!r} (expected one of {WORKLOADS})")

    report = {"library_sha256": sha, "repeats": args.repeats, "guide": {"threshold": 0.0, "guard": 1}, "workloads": {}}
    for name in [w for w in args.workloads.split(",") if w]:
        cfg, make_scene, size, extra = workload(name)
        torch.manual_seed(0)
        model = EnvironmentModel(cfg)
        synthetic.randomize_module_state(model.object_composer, seed=0, step=60000, alpha_bias=1.0, bender_scale=1e4)
        model.eval().to(dev)
        model.frame_replay = None
        comp = model.object_composer
        has_fine = all(m is not None for m in comp.object_models_fine)
        static = comp.object_id_helper.static_objects_count
        scene = bench.to_device(make_scene(seed=1234, image_size=size), dev)
        moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in scene.items()}
        moved["object_translation_parameters"][..., static:] += 0.05           # the players move, the camera stands still
        scenes = [scene, moved]
        retained = comp.retain_objects()
        guide = FineGuide()
        entry = {"size": list(size), "fine_pass": has_fine, "precisions": {}}
        if not has_fine:
            entry["note"] = "no fine pass in this configuration: the guide has nothing to act on"

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

        def fine_features(s):
            out = frame(s)
            torch.cuda.synchronize()
            return out["fine"]["global"]["integrated_features"].clone()

        for precision in [p for p in args.precisions.split(",") if p]:
            comp.precision = precision
            turn = [0]

            def select(variant):
                _lib._LIB = parent if variant.startswith("parent") else current
                comp.fine_guide = guide if variant.startswith("guide") else None
                comp.retained = retained if variant == "guide_reuse" else None
                if variant == "guide_reuse":               # its own counter: the players move between consecutive reuse frames
                    turn[0] += 1
                    return scenes[turn[0] & 1]
                return scene

            variants = ["off"] + (["guide", "guide_reuse"] if has_fine else [])
            if parent is not None and name in ("headline", "evaluator"):
                variants += ["parent_a", "parent_b"]
            for v in variants:
                for _ in range(args.warmup + (1 if v == "guide_reuse" else 0)):
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
                if v.startswith("parent"):
                    continue
                if v == "guide_reuse":
                    frame(select(v))                       # (the frame before: the cache holds the static objects)
                evaluated[v] = counted(select(v))
                s = select(v)
                current.pr_profile_enable(1)
                frame(s)
                ms, launches = bench.profile_arrays()
                current.pr_profile_collect(ms, launches)
                current.pr_profile_enable(0)
                categories[v] = {"mlp_ms": round(ms[0], 3), "resample_ms": round(ms[6], 3), "fill_ms": round(ms[7], 3),
                                 "milliseconds": [round(x, 3) for x in ms], "launches": list(launches)}     # (categories: include/playrender.h)
            result = {"variants": {v: spread(t) for v, t in times.items()}, "evaluated_samples": evaluated, "kernel_categories": categories}
            off = result["variants"]["off"]
            if has_fine:
                result["speedup_guide_vs_off"] = round(off["median_ms"] / result["variants"]["guide"]["median_ms"], 4)
                result["speedup_guide_reuse_vs_off"] = round(off["median_ms"] / result["variants"]["guide_reuse"]["median_ms"], 4)
                # quality, reported and not gated: the fine global features, guide against off
                select("off")
                reference = fine_features(scene)
                select("guide")
                quality = {"synthetic_weights_psnr_db": psnr(reference, fine_features(scene))}
                saved = [{k: v.clone() for k, v in m.state_dict().items()} for m in comp.object_models_fine]
                for coarse, fine in zip(comp.object_models_coarse, comp.object_models_fine):
                    fine.load_state_dict(coarse.state_dict())
                comp.weights_changed()
                select("off")
                reference = fine_features(scene)
                agree_off = counted(scene)
                select("guide")
                quality["fine_equals_coarse_psnr_db"] = psnr(reference, fine_features(scene))
                quality["fine_equals_coarse_evaluated_samples"] = {"off": agree_off, "guide": counted(scene)}
                for fine, state in zip(comp.object_models_fine, saved):
                    fine.load_state_dict(state)
                comp.weights_changed()
                result["quality"] = quality
            else:
                result["speedup_guide_vs_off"] = result["speedup_guide_reuse_vs_off"] = result["quality"] = NOT_MEASURED
            if "parent_a" in times:
                a, b = result["variants"]["parent_a"], result["variants"]["parent_b"]
                both = times["parent_a"] + times["parent_b"]
                lo, hi = min(a["median_ms"], b["median_ms"]), max(a["median_ms"], b["median_ms"])
                result["off_vs_parent"] = {"off_median_ms": off["median_ms"], "parent_a_median_ms": a["median_ms"], "parent_b_median_ms": b["median_ms"],
                                           "parent_medians_differ_by_ms": round(hi - lo, 3),
                                           "parent_frames_min_max_ms": [round(min(both), 3), round(max(both), 3)],
                                           "off_minus_nearer_parent_median_ms": round(min(abs(off["median_ms"] - a["median_ms"]),
                                                                                          abs(off["median_ms"] - b["median_ms"])), 3),
                                           "within_spread_of_the_two_parent_runs": min(both) <= off["median_ms"] <= max(both)}
            else:
                result["off_vs_parent"] = NOT_MEASURED
            _lib._LIB = current
            comp.fine_guide = comp.retained = None
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
