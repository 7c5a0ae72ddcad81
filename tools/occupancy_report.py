#!/usr/bin/env python3
"""What empty-space skipping does to the headline frame: writes profiles/occupancy_report.json.

The frame is bench.py's headline construction - BASELINE.json configs[1]: tennis, 64 coarse + 128 resampled positions per ray, one
256 x 256 frame (seed 1234), randomize_module_state(seed=0, step=60000, alpha_bias=0.0, bender_scale=1e4), frame_replay = None,
exact fp32.  The variants are timed with device events, warmed, ALTERNATING in one process (a drifting clock hits all of them):

    off      composer.occupancy = None
    ones     a grid of ones at the default resolution (what the lookup costs when nothing is culled)
    built    build_occupancy at its defaults
    follow   the same grid with follow = True (one build per frame)
    parent   `off` on a library built from the parent commit (--parent-lib; "not measured" without it)

    make -C playableenvironments_amd/csrc
    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/playableenvironments_amd/csrc OUT=$PWD/build/libplayrender_parent.so OBJDIR=/tmp/parent/obj
    python tools/occupancy_report.py --parent-lib build/libplayrender_parent.so
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOT_MEASURED = "not measured"


def load_parent(path, _lib):
    """The parent commit's library beside the current one: its prototypes are set for the symbols it has."""
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def spread(values):
    return {"median_ms": round(statistics.median(values), 3), "min_ms": round(min(values), 3), "max_ms": round(max(values), 3),
            "repeats": len(values)}


def psnr(reference, other):
    a, b = reference.double(), other.double()
    mse = float(((a - b) ** 2).mean())
    return None if mse == 0.0 else round(float(10.0 * torch.log10(a.abs().max() ** 2 / mse)), 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=12, help="timed frames per variant (>= 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--parent-lib", default=None, help="libplayrender.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_report.json"))
    args = ap.parse_args()
    if args.repeats < 10:
        ap.error("--repeats must be at least 10")

    from playableenvironments_amd import _lib, configs, synthetic
    from playableenvironments_amd.environment_model import EnvironmentModel
    import bench

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    current = _lib.load()
    parent = load_parent(args.parent_lib, _lib) if args.parent_lib else None

    cfg = configs.tennis_config(hierarchical=(64, 128))
    torch.manual_seed(0)
    model = EnvironmentModel(cfg)
    synthetic.randomize_module_state(model.object_composer, seed=0, step=60000, alpha_bias=0.0, bender_scale=1e4)
    model.eval().to(dev)
    model.frame_replay = None
    comp = model.object_composer
    size = (args.image, args.image)
    scene = bench.to_device(synthetic.tennis_scene(seed=1234, image_size=size), dev)
    codes = (scene["object_style"], scene["object_deformation"])

    counts = {}
    plain_forward = comp.forward

    def counting_forward(*a, **k):          # one untimed call per variant with the per-sample exports: the evaluated counts
        out = plain_forward(*a, **k, _export=True)
        for ty in ("coarse", "fine"):
            if ty in out:
                counts[ty] = out[ty].pop("_samples")[0]["evaluated"].cpu().tolist()
        return out

    def frame():
        with torch.no_grad():
            return model(*bench.scene_args(scene, size), 0, False, mode="scene_encodings")

    def timed_frame():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = frame()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop), out

    # ---- the grids ------------------------------------------------------------------------------------------------
    build_start, build_stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        built = comp.build_occupancy(*codes)          # (warm: packs the weights, sizes the workspace)
        torch.cuda.synchronize()
        build_times = []
        for _ in range(5):
            build_start.record()
            built.update(*codes)
            build_stop.record()
            build_stop.synchronize()
            build_times.append(build_start.elapsed_time(build_stop))
        follower = comp.build_occupancy(*codes)
        follower.follow = True
    ones = comp.occupancy_from_mask({key: torch.ones((built.frames,) + tuple(g["cells"]), dtype=torch.bool, device=dev)
                                     for key, g in built.grids.items()})

    def use(grid, lib=current):
        def select():
            comp.occupancy = grid
            _lib._LIB = lib
        return select

    variants = {"off": use(None), "ones": use(ones), "built": use(built), "follow": use(follower)}
    if parent is not None:
        variants["parent"] = use(None, parent)

    # ---- evaluated samples and the rendered features of every variant (untimed) -------------------------------------------
    evaluated, features = {}, {}
    for name, select in variants.items():
        select()
        comp.forward = counting_forward
        try:
            out = frame()
        finally:
            del comp.forward
        torch.cuda.synchronize()
        evaluated[name] = dict(counts)
        features[name] = {ty: out[ty]["global"]["integrated_features"].clone() for ty in ("coarse", "fine")}

    # ---- timing ---------------------------------------------------------------------------------------------------
    telemetry = None
    try:
        import gpu_telemetry
        props = torch.cuda.get_device_properties(dev)

        def load():
            tf, pms = C.c_double(), C.c_double()
            current.pr_probe_mfma_f32(20000, 1, C.byref(tf), C.byref(pms), None)
        card = gpu_telemetry.find_card(load, pci=(props.pci_domain_id, props.pci_bus_id, props.pci_device_id))
        if card is not None:
            telemetry = gpu_telemetry.Telemetry(card)
            telemetry.start()
    except Exception as error:
        print(f"occupancy_report: no clock telemetry ({type(error).__name__}: {error})", file=sys.stderr)

    for select in variants.values():
        select()
        for _ in range(args.warmup):
            frame()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    if telemetry is not None:
        telemetry.label = "timed"
    for _ in range(args.repeats):
        for name, select in variants.items():
            select()
            times[name].append(timed_frame()[0])
    if telemetry is not None:
        telemetry.label = None
        telemetry.finish()
    use(None)()

    # ---- the report -----------------------------------------------------------------------------------------------
    report = {
        "workload": "bench.py headline: tennis, 4 objects, 64 + 128 positions per ray, one %dx%d frame, exact fp32, eager" % size,
        "grid": dict(built.build, cells=list(next(iter(built.grids.values()))["cells"])),
        "variants": {name: spread(values) for name, values in times.items()},
        "build_ms": spread(build_times),
        "kept_cell_fraction": {f"object_{k}.{level}": round(v, 4) for (k, level), v in built.kept_fraction().items()},
        "evaluated_samples": evaluated,
        "culled_sample_fraction": {ty: [round(1.0 - b / a, 4) if a else 0.0 for a, b in zip(evaluated["off"][ty], evaluated["built"][ty])]
                                   for ty in evaluated["off"]},
        "psnr_built_vs_off_db": {ty: (psnr(features["off"][ty], features["built"][ty]) or "identical") for ty in features["off"]},
        "ones_equals_off": all(torch.equal(features["off"][ty], features["ones"][ty]) for ty in features["off"]),
        "follow_equals_built": all(torch.equal(features["built"][ty], features["follow"][ty]) for ty in features["off"]),
        "clock": telemetry.summary("timed") if telemetry is not None else NOT_MEASURED,
    }
    off = report["variants"]["off"]
    report["lookup_cost_ms"] = {"ones_minus_off_median": round(report["variants"]["ones"]["median_ms"] - off["median_ms"], 3),
                                "off_spread_ms": round(off["max_ms"] - off["min_ms"], 3)}
    report["speedup_built_vs_off"] = round(off["median_ms"] / report["variants"]["built"]["median_ms"], 4)
    report["speedup_follow_vs_off"] = round(off["median_ms"] / report["variants"]["follow"]["median_ms"], 4)
    if parent is not None:
        p = report["variants"]["parent"]
        report["off_vs_parent"] = {"off_minus_parent_median_ms": round(off["median_ms"] - p["median_ms"], 3),
                                   "parent_spread_ms": round(p["max_ms"] - p["min_ms"], 3),
                                   # the issue's criterion: |median(off) - median(parent)| within the width of the parent's own min-max spread
                                   "abs_median_difference_within_parent_spread_width": abs(off["median_ms"] - p["median_ms"]) <= p["max_ms"] - p["min_ms"],
                                   "off_median_between_parent_min_and_max": p["min_ms"] <= off["median_ms"] <= p["max_ms"],
                                   "parent_equals_off": all(torch.equal(features["off"][ty], features["parent"][ty]) for ty in features["off"])}
    else:
        report["off_vs_parent"] = NOT_MEASURED
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
