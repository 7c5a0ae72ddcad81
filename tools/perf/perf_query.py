"""Timing of the point queries (GPU box): a 128^3 grid (2.1 M points, all inside) of tennis player_1 through
ObjectComposer.query_object, with and without features, at the three precisions - points/s, the pr_profile_collect split
(category 0 = the MLP launch, 5 = the query's own kernels: count + scan + fill, scatter) - and, as the baseline a user has today
on the same GPU, oracle.render_oracle.object_model_forward on device tensors for the same points.

    python tools/perf/perf_query.py [grid edge, default 128] [timed calls, default 10]

Protocol: three warm-up calls per configuration, HIP events around every timed call, medians; the profiled calls run after the
timed ones (event pairs around every launch slow the host); the shader clock is sampled while each configuration runs."""
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
from oracle import render_oracle as ro  # noqa: E402
from playableenvironments_amd import ObjectComposer, _lib, configs, synthetic  # noqa: E402


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
    edge = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    if not torch.cuda.is_available():
        raise RuntimeError("perf_query.py measures on a GPU")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    cfg = configs.tennis_config()
    object_idx = 2                                                   # player_1: NeRF + ray bender
    model_cfg = cfg["model"]["object_models"][object_idx]
    torch.manual_seed(0)
    comp = ObjectComposer(cfg)
    synthetic.randomize_module_state(comp, seed=0, step=20000, bender_scale=1e4)
    comp.eval().to(dev)
    g = torch.Generator().manual_seed(1)
    style = torch.randn((1, model_cfg["style_features"]), generator=g).to(dev)
    deformation = torch.randn((1, model_cfg["deformation_features"]), generator=g).to(dev)
    with torch.no_grad():      # voxel centres, as ObjectComposer.density_grid places them
        box = torch.tensor(model_cfg["bounding_box"], device=dev)
        axes = [box[a, 0] + (torch.arange(edge, device=dev) + 0.5) * ((box[a, 1] - box[a, 0]) / edge) for a in range(3)]
        positions = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(1, -1, 3).contiguous()
    points = positions.shape[1]
    props = torch.cuda.get_device_properties(0)
    card = gpu_telemetry.card_of_pci_address(props.pci_domain_id, props.pci_bus_id, props.pci_device_id)       # (None: no clock column)
    telemetry = gpu_telemetry.Telemetry(card) if card else None
    if telemetry:
        telemetry.start()
    sha = hashlib.sha256(open(_lib.library_path(), "rb").read()).hexdigest()[:12]
    rows = []
    with torch.no_grad():
        for precision in ("fp32", "f16x3", "f16"):
            comp.precision = precision
            for features in (True, False):
                label = f"{precision}{'' if features else ' density-only'}"
                run = lambda: comp.query_object(object_idx, positions, style, deformation, features=features)
                for _ in range(3):
                    out = run()
                torch.cuda.synchronize()
                assert int(out["evaluated"][0]) == points, "the grid must lie inside the box"
                if telemetry:
                    telemetry.label = label
                ms = timed(run, calls)
                if telemetry:
                    telemetry.label = None
                lib.pr_profile_enable(1)
                for _ in range(calls):
                    run()
                torch.cuda.synchronize()
                lib.pr_profile_enable(0)
                cat_ms, cat_n = (C.c_double * _lib.PR_PROFILE_CATEGORIES)(), (C.c_int32 * _lib.PR_PROFILE_CATEGORIES)()
                _lib.check(lib.pr_profile_collect(cat_ms, cat_n), "pr_profile_collect")
                med = statistics.median(ms)
                row = {"config": label, "points": points, "call_ms_median": round(med, 3), "call_ms_min": round(min(ms), 3),
                       "call_ms_max": round(max(ms), 3), "mpoints_per_s": round(points / med / 1e3, 1),
                       "mlp_ms": round(cat_ms[0] / calls, 3), "query_kernels_ms": round(cat_ms[5] / calls, 3),
                       "query_share_of_mlp": round(cat_ms[5] / cat_ms[0], 4) if cat_ms[0] else None,
                       "ns_per_point_mlp": round(cat_ms[0] / calls * 1e6 / points, 3)}
                if telemetry:
                    row["clock"] = telemetry.summary(label)
                rows.append(row)
                print(json.dumps(row), flush=True)
        # the baseline a user has today: the oracle's op graph on device tensors (fp32 torch kernels)
        sd = {k: v.detach().clone() for k, v in comp.state_dict().items()}
        origins = torch.zeros((1, points, 3), device=dev)

        def baseline():
            return ro.object_model_forward(sd, f"object_models_coarse.{object_idx}.", model_cfg, positions.unsqueeze(-2), origins, origins,
                                           style.unsqueeze(1), deformation.unsqueeze(1), False, training=False)
        want = baseline()
        torch.cuda.synchronize()
        comp.precision = "fp32"
        got = comp.query_object(object_idx, positions, style, deformation)
        err = float((got["features"] - want[0].squeeze(-2)).abs().max())
        ms = timed(baseline, max(3, calls // 3))
        med = statistics.median(ms)
        row = {"config": "torch oracle on the device (fp32)", "points": points, "call_ms_median": round(med, 3),
               "mpoints_per_s": round(points / med / 1e3, 1), "max_abs_diff_of_fp32_query_features": err}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if telemetry:
        telemetry.finish()
    full = {r["config"]: r for r in rows}
    print(f"library sha256 {sha}, device {props.name}, grid {edge}^3 = {points} points")
    for p in ("fp32", "f16x3", "f16"):
        print(f"{p}: density-only / full = {full[p + ' density-only']['call_ms_median'] / full[p]['call_ms_median']:.3f}")


if __name__ == "__main__":
    main()
