"""Manual randomized sweep (GPU box): ObjectComposer.forward on the HIP renderer against the oracle over random network
shapes, sample counts, ray counts, frames, flags and absent objects.      python tests/gpu_fuzz.py [cases] [seed] [backward]
("backward": the gradients of pr_render_backward against torch.autograd through the oracle instead - training mode, every
differentiable output probed, camera-ray and divergence gradients included.)

A fixed-seed slice (40 forward + 20 backward cases, seed 0) runs in the driver's suite: tests/test_gpu.py::test_randomized_sweep_slice.

A backward case that exceeds the tolerance is classified before it counts as a failure: ill-conditioned (the ORACLE's own gradients
move that much under a 1e-6 parameter perturbation), a noise kink (relu(sigma + noise) at 0 within fp32 rounding: two other noise
realisations agree), or arbitrated in float64 (HIP no farther from the oracle's float64 autograd than 4 x the fp32 oracle).

Forward fields are compared at the parity tolerance of the suite (rtol 1e-4, atol 1e-5; every field, ``weights`` included);
perturbed cases replay the oracle's noise.  A HIERARCHICAL case that exceeds it (the inverse CDF turns last-bit differences of the
coarse weights into sample positions) is ARBITRATED instead of loosened: the oracle's op graph in float64 on the same weights,
inputs and noise is the exact result, and every field of the HIP render has to be no farther from it than 4 x the fp32 oracle is
("ok (arbitrated)"); anything else is a failure.  A single-pass case gets the same arbitration under its own label ("ok (arbitrated,
single pass)": the fp32 oracle itself is then that far from float64 - high-frequency encodings in front of shallow random layers).
Recorded (profiles/r05_sweep_forward_*): 1 such case in 1 340 (seeds 7, 11, 12, 13, 14), none in the suite's slice.
A hierarchical case of thousands of rays whose MAXIMA fail that arbitration is examined ray by ray ("ok (arbitrated, isolated rays)":
HIP has no more rays beyond the tolerance from float64 than the fp32 oracle has (+ 1) and the same typical error - single rays whose
uniform draw sits within rounding of a coarse-CDF edge land in the neighbouring bin on either fp32 side).  Recorded: 1 in the 80 large
forward cases of seeds 14 / 25 (profiles/r06_sweep_forward_large_40_seed25.log), none elsewhere."""
import os
import random
import sys
import traceback

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from playableenvironments_amd import _lib, configs, synthetic  # noqa: E402

if os.environ.get("PR_FUZZ_LIB"):      # a measurement / comparison build of the library (tools/build_variant.sh)
    _lib.library_path = lambda: os.path.abspath(os.environ["PR_FUZZ_LIB"])
from tests.helpers import arbitrate, bender_kink_margin, compare_results, composer_inputs, grid_pixels, poison_device_memory as poison  # noqa: E402
from tests.test_gpu import build, run_both, run_exact  # noqa: E402


def random_case(rng):
    world = rng.choice(["tennis", "minecraft"])
    base = configs.tennis_config() if world == "tennis" else configs.minecraft_config()
    layers = rng.randint(2, 8)
    bl = rng.randint(2, 6)
    shape = dict(width=rng.choice([16, 32, 48, 64, 96, 128, 256]), layers=layers, skip=rng.randint(1, layers - 1),
                 features=rng.choice([4, 8, 16, 32, 48, 64, 192]), octaves=rng.randint(1, 10),
                 bender_width=rng.choice([16, 32, 48, 64, 128]), bender_layers=bl, bender_skip=rng.randint(1, bl - 1),
                 bender_octaves=rng.randint(1, 6))
    hierarchical = world == "tennis" and rng.random() < 0.4
    positions = {}
    for o in base["model"]["object_models"]:
        if o["nerf_model"]["architecture"].lower().startswith("skybox") or o["positions_count_coarse"] == 1:
            continue
        pc = rng.randint(3, 40)
        positions[o["name"]] = (pc, rng.randint(1, 40) if hierarchical else o.get("positions_count_fine", 0))
    if base["model"]["fix_object_overlaps"]:
        # the overlap fix indexes a dynamic object's samples with the static object's count - 1: the reference (and the
        # library's argument check) needs static counts <= dynamic counts
        dynamic = min(pc for name, (pc, _) in positions.items() if name.startswith("player"))
        positions = {name: ((min(pc, dynamic), pf) if not name.startswith("player") else (pc, pf)) for name, (pc, pf) in positions.items()}
    rgb = rng.random() < 0.15          # colour-output models: 3 features through a sigmoid (apply_activation)
    if rgb:
        shape["features"] = 3
    cfg = configs.reduced_config(configs.enable_fine(base) if hierarchical else base, positions=positions, **shape)
    if rgb:
        cfg["model"]["apply_activation"] = True
        for o in cfg["model"]["object_models"]:
            o["empty_space_alpha"] = rng.choice([-3.5, -0.5])
    frames = rng.choice([(1, 1), (1, 2), (2, 1), (3, 1)])
    scene_fn = synthetic.tennis_scene if world == "tennis" else synthetic.minecraft_scene
    scene = scene_fn(batch=frames[0], observations=frames[1], seed=rng.randint(0, 10 ** 6))
    n = rng.choice([1, 2, 3, 5, 8, 13, 21] if os.environ.get("PR_FUZZ_LARGE") is None else [48, 64, 80, 96])   # rays = n * n
    inputs = list(composer_inputs(cfg, scene, pixels=grid_pixels(scene["image_size"][0], scene["image_size"][1], n)))
    if rng.random() < 0.3:       # an absent object in some frames
        ins = inputs[6].clone()
        ins[..., rng.randrange(ins.size(-1))] = False
        inputs[6] = ins
    flags = dict(perturb=rng.random() < 0.4, canonical=rng.random() < 0.2)
    return world, cfg, inputs, flags, hierarchical, shape, positions, frames, n


def oracle_sensitivity(cfg, scene, n, bias, perturb, keys, rays, eps=1e-6, trials=4):
    """How far the ORACLE's own gradients move when its parameters are perturbed by ``eps`` relative (same noise, same probes):
    the scale at which a comparison of this case is meaningful (ReLU / AABB / clamp decisions flip, train-mode batch
    statistics over few samples amplify)."""
    from oracle import render_oracle as ro
    from tests.test_gpu import _probe_loss
    comp = build(cfg, alpha_bias=bias).train()
    o, d, nrm, w2o, sty, dfm, ins = composer_inputs(cfg, scene, pixels=grid_pixels(scene["image_size"][0], scene["image_size"][1], n))
    K = w2o.size(-1)
    names = [k for k, _ in comp.named_parameters()]
    out = []
    rec, probes = {}, None
    for trial in range(1 + trials):
        sd = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
        if trial:
            g = torch.Generator().manual_seed(99 + trial)
            for k in names:
                sd[k] = sd[k] * (1 + eps * torch.randn(sd[k].shape, generator=g))
        for k in names:
            sd[k].requires_grad_(True)
        torch.manual_seed(123)
        want = ro.composer_forward(cfg, sd, o, d, nrm, w2o, sty, dfm, ins, perturb, training=True,
                                   noise=rec if trial else None, record_noise=None if trial else rec, stable_merge=True)
        if probes is None:
            gen = torch.Generator().manual_seed(7)
            probes = {(ty, nm, key): torch.randn(want[ty][nm][key].shape, generator=gen) for ty in ("coarse", "fine") if ty in want
                      for nm in [f"object_{k}" for k in range(K)] + ["global"] for key in keys}
        _probe_loss(want, probes, K).backward()
        out.append({k: sd[k].grad.clone() if sd[k].grad is not None else torch.zeros_like(sd[k]) for k in names})
    worst = 0.0
    for k in names:
        scale = float(out[0][k].abs().max())
        if scale > 0:
            worst = max(worst, max(float((out[0][k] - o[k]).abs().max()) for o in out[1:]) / scale)
    return worst


def divergence_kink_margin(cfg, scene, n, bias, perturb, absent, noise_seed=123):
    """tests.helpers.bender_kink_margin of the oracle run `_gradients` makes for this case."""
    from oracle import render_oracle as ro
    comp = build(cfg, alpha_bias=bias).train(True)
    o, d, nrm, w2o, sty, dfm, ins = composer_inputs(cfg, scene, pixels=grid_pixels(scene["image_size"][0], scene["image_size"][1], n))
    if absent is not None:
        ins = ins.clone()
        flat = ins.reshape(-1, ins.size(-1))
        if absent[1] is None:
            flat[:, absent[0]] = False
        else:
            flat[absent[1] % flat.size(0), absent[0]] = False
    sd = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}

    def run_oracle():
        torch.manual_seed(noise_seed)
        ro.composer_forward(cfg, sd, o, d, nrm, w2o, sty, dfm, ins, perturb, training=True, record_noise={}, stable_merge=True)
    return bender_kink_margin(run_oracle)


def backward_sweep(cases, rng, only=None):
    from tests.test_gpu import GRAD_KEYS, KINK_MARGIN, ForwardFieldMismatch, drain_settlements, _gradients as _gradients_fp32
    # PR_FUZZ_PRECISION=f16x3: the same sweep with the split-precision training kernels (fp16-pair forward phase, backward chains and
    # weight gradients) against the same oracle, tolerances and classifications
    precision = os.environ.get("PR_FUZZ_PRECISION", "fp32")

    def _gradients(*a, **kw):
        return _gradients_fp32(*a, precision=precision, **kw)
    failures = 0
    for i in range(cases):
        world = rng.choice(["tennis", "minecraft"])
        base = configs.tennis_config() if world == "tennis" else configs.minecraft_config()
        layers, bl = rng.randint(2, 6), rng.randint(2, 5)
        shape = dict(width=rng.choice([32, 48, 64, 96, 128]), layers=layers, skip=rng.randint(1, layers - 1),
                     features=rng.choice([16, 32, 48, 64]), octaves=rng.randint(1, 6), bender_width=rng.choice([16, 32, 48, 64]),
                     bender_layers=bl, bender_skip=rng.randint(1, bl - 1), bender_octaves=rng.randint(1, 4))
        hierarchical = world == "tennis" and rng.random() < 0.3
        positions = None
        if hierarchical:
            positions = {o["name"]: (rng.randint(4, 14), rng.randint(2, 20)) for o in base["model"]["object_models"]}
        cfg = configs.reduced_config(configs.enable_fine(base) if hierarchical else base, positions=positions, **shape)
        scene_fn = synthetic.tennis_scene if world == "tennis" else synthetic.minecraft_scene
        frames = rng.choice([(1, 1), (2, 1), (1, 2)])
        scene = scene_fn(batch=frames[0], observations=frames[1], seed=rng.randint(0, 10 ** 6))
        n = rng.choice([8, 12, 16])
        perturb, rays = rng.random() < 0.5, rng.random() < 0.5
        keys = GRAD_KEYS + (("integrated_divergence",) if rng.random() < 0.5 else ())
        absent = (rng.randrange(4), rng.choice([None, 0, 1])) if rng.random() < 0.3 else None
        label = f"case {i}: {world} {shape} frames={frames} rays={n * n} perturb={perturb} ray grads={rays} keys={len(keys)} positions={positions} absent={absent}"
        bias = rng.choice([2.0, 3.0])
        if only is not None and i != only:
            continue
        try:
            poison()
            drain_settlements()
            grads = _gradients(cfg, scene, n, bias, perturb, keys=keys, rays=rays, min_divergence=0.0, absent=absent)
            settlements = drain_settlements()
            for entry in settlements:         # (a forward field the harness settled instead of failing on: never silent)
                print("    settled:", entry)
            bad = {}
            for k, (a, b) in grads.items():
                scale = float(a.abs().max())
                if k == "ray_origins":
                    scale = max(scale, float(grads["ray_directions"][0].abs().max()))
                err = float((a - b).abs().max())
                if err > (5e-3 if hierarchical else 5e-4) * scale + 1e-9:
                    bad[k] = (f"{err:.2e}", f"{scale:.2e}")
            if bad:
                worst = max(float(v[0]) / float(v[1]) for v in bad.values())
                own = oracle_sensitivity(cfg, scene, n, bias, perturb, keys, rays)
                def clean_with(seed):     # the same case with another realisation of the perturbation noise
                    again = _gradients(cfg, scene, n, bias, perturb, keys=keys, rays=rays, min_divergence=0.0, absent=absent, noise_seed=seed)
                    for k2, (a2, b2) in again.items():
                        s2 = float(a2.abs().max())
                        if k2 == "ray_origins":
                            s2 = max(s2, float(again["ray_directions"][0].abs().max()))
                        if float((a2 - b2).abs().max()) > (5e-3 if hierarchical else 5e-4) * s2 + 1e-9:
                            return False
                    return True
                def arbitrated():         # the oracle's autograd in float64 as the exact result
                    exact = _gradients(cfg, scene, n, bias, perturb, keys=keys, rays=rays, min_divergence=0.0, absent=absent, exact=True)
                    for k2, (a2, b2, e2) in exact.items():
                        s2 = float(e2.abs().max())
                        if float((b2.double() - e2).abs().max()) > 4.0 * float((a2.double() - e2).abs().max()) + 1e-5 * s2:
                            return False
                    return True
                if worst <= 20 * own:
                    print(f"ill-conditioned (HIP vs oracle {worst:.1e} relative; the oracle moves {own:.1e} under a 1e-6 parameter perturbation)", label[:120])
                elif perturb and clean_with(1123) and clean_with(2123):
                    # relu(sigma + noise) has a kink at 0: a sample whose noisy density sits there within fp32 rounding passes its
                    # gradient on one side and not on the other (the forward value is continuous) - one realisation in ~100 cases has one
                    print(f"noise kink (HIP vs oracle {worst:.1e} relative with this noise realisation only: two other realisations agree)", label[:120])
                elif arbitrated():
                    print(f"ill-conditioned (HIP vs oracle {worst:.1e} relative; in float64 arbitration the HIP gradients are no farther from the exact ones than 4 x the fp32 oracle's)", label[:120])
                else:
                    failures += 1
                    print(f"MISMATCH (worst {worst:.1e}, oracle self-sensitivity {own:.1e})", label, dict(list(bad.items())[:4]))
                    # where the excess sits: a flipped ReLU decision of ONE hidden unit shows as one row of its layer's weight
                    # gradient (and one entry of its bias gradient) carrying the error
                    for k in list(bad)[:8]:
                        a, b = grads[k]
                        e = (a - b.cpu() if b.is_cuda else a - b).double()
                        if e.dim() == 2:
                            rows = (e ** 2).sum(1)
                            print(f"    {k}: row {int(rows.argmax())} holds {float(rows.max() / rows.sum()):.3f} of the squared error "
                                  f"({e.shape[0]} rows)")
                        elif e.dim() == 1:
                            print(f"    {k}: entry {int(e.abs().argmax())} holds {float((e ** 2).max() / (e ** 2).sum()):.3f} of the squared error")
            elif settlements:
                kinds = sorted({e["kind"] for e in settlements})
                print(f"ok (forward {' + '.join(kinds)}) " + label[:150])
            else:
                print("ok", label[:170])
        except ValueError as e:       # train-mode BatchNorm on exactly one sample: the reference raises too
            print("skipped", label[:120], str(e)[:60])
        except ForwardFieldMismatch as e:
            # only the Hutchinson divergence estimate, with a sample within fp32 rounding of a kink of the benders' Jacobian (its
            # displacement at the clamp bound, a hidden unit at 0): the estimate is discontinuous there
            margin = 1.0
            if all(k.endswith("integrated_divergence") for k in e.fields):
                margin = divergence_kink_margin(cfg, scene, n, bias, perturb, absent)
            if margin < KINK_MARGIN[precision]:
                print(f"divergence kink (a sample {margin:.1e} of its scale from a kink of the ray bender's Jacobian; every other field agrees)", label[:120])
            else:
                failures += 1
                print("ERROR", label, e.fields, f"kink margin {margin:.1e}")
        except Exception:
            failures += 1
            print("ERROR", label)
            traceback.print_exc()
    print(f"{cases} backward cases, {failures} failures")
    return failures


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = random.Random(seed)
    only = int(sys.argv[4]) if len(sys.argv) > 4 else None
    if len(sys.argv) > 3 and sys.argv[3] == "backward":
        return backward_sweep(cases, rng, only)
    return forward_sweep(cases, rng, only)


def forward_sweep(cases, rng, only=None):
    failures = 0
    for i in range(cases):
        world, cfg, inputs, flags, hierarchical, shape, positions, frames, n = random_case(rng)
        label = f"case {i}: {world} {shape} positions={positions} frames={frames} rays={n * n} {flags} hierarchical={hierarchical}"
        bias = rng.choice([0.0, 1.0, 2.0, 3.0])
        precision = "f16x3" if rng.random() < 0.3 else "fp32"
        rechunk = rng.random() < 0.5
        if only is not None and i != only:
            continue
        try:
            poison()
            comp = build(cfg, seed=i, alpha_bias=bias, precision=precision)
            label += f" {precision}"
            want, got = run_both(cfg, comp, inputs, perturb=flags["perturb"], canonical=flags["canonical"])
            # the same call split along the rays by a small workspace budget must give the same bits (rays are independent)
            if not flags["perturb"] and rechunk:
                budget = type(comp).max_workspace_bytes
                try:
                    comp.max_workspace_bytes = 24 << 20
                    with torch.no_grad():
                        again = comp(*[v.cuda() for v in inputs], False, canonical_pose=flags["canonical"])
                finally:
                    comp.max_workspace_bytes = budget
                for ty in got:
                    if not isinstance(got[ty], dict):
                        continue
                    for name in got[ty]:
                        if not isinstance(got[ty][name], dict):
                            continue
                        for key, v in got[ty][name].items():
                            if torch.is_tensor(v) and not torch.equal(torch.nan_to_num(v), torch.nan_to_num(again[ty][name][key])):
                                raise AssertionError(f"chunked render differs in {ty}.{name}.{key}")
            tol = dict(rtol=1e-4, atol=1e-5)
            rep = compare_results(want, got, **tol)
            bad = {k: f"{v[0]:.2e}" for k, v in rep.items() if not v[1]}
            arbitrated = False
            if bad and hierarchical:
                # resampling amplifies fp32 round-off of the coarse pass: which side is off?  float64 decides, field by field
                state = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
                exact = run_exact(cfg, state, inputs, flags["perturb"], run_both.noise if flags["perturb"] else None,
                                  canonical=flags["canonical"])
                verdict = arbitrate(exact, want, got, factor=4.0, floor=1e-6)
                bad = {k: f"HIP {verdict[k][0]:.2e} vs fp32 oracle {verdict[k][1]:.2e} from float64" for k in bad if not verdict[k][2]}
                arbitrated = not bad
            for key in [k for k in bad if k.endswith("depth")]:
                # depth = sum w_i t_i with t up to ~60: on a nearly transparent ray alpha = 1 - exp(-sigma delta) carries the
                # absolute error of 1 ulp(1) = 6e-8 per sample whatever exp is used, i.e. up to ~4e-6 x samples in the depth
                ty, name, _ = key.split(".")
                a, b = want[ty][name]["depth"].detach().cpu().float(), got[ty][name]["depth"].detach().cpu().float()
                if torch.allclose(a, b, rtol=tol["rtol"], atol=5e-5, equal_nan=True):
                    del bad[key]
            for key in [k for k in bad if k.endswith("disparity")]:
                # disparity = 1 / max(eps, depth / opacity) is NaN exactly where the opacity is 0.  1 - exp(-sigma delta) rounds to 0
                # or to 2^-24 around sigma delta = 2^-25: a ray whose only contribution sits on that boundary has opacity 0 on one
                # side and 6e-8 on the other (equal at the suite's tolerance) and differs in NaN-ness only
                ty, name, _ = key.split(".")
                a, b = want[ty][name]["disparity"].detach().cpu().float(), got[ty][name]["disparity"].detach().cpu().float()
                differ = torch.isnan(a) != torch.isnan(b)
                tiny = (want[ty][name]["opacity"].detach().cpu().abs() < 1e-6) & (got[ty][name]["opacity"].detach().cpu().abs() < 1e-6)
                rest = ~(torch.isnan(a) | torch.isnan(b))
                if bool((differ & ~tiny).sum() == 0) and torch.allclose(a[rest], b[rest], **tol):
                    del bad[key]
            if bad and hierarchical:
                # Still beyond 4 x: the comparison above is one of MAXIMA, and with thousands of rays the maximum of either fp32 side is
                # a single ray whose uniform draw sits within rounding of an edge of the coarse CDF - the resampled position lands in
                # the neighbouring bin (a discontinuity; ~1e-5 of the draws of a 6 400-ray case lie within 1e-6 of an edge).  Both
                # sides have such rays, which ones and how much they matter is chance (seed 25 large case 36: ONE ray off on each
                # side, HIP's in a denser region).  Ray by ray against float64: HIP may have as many rays beyond the tolerance as the
                # fp32 oracle has (+ 1), and its typical error (99.9 % quantile) must stay within 2 x the oracle's.
                isolated = {}
                for key in list(bad):
                    ty, name, field = key.split(".")
                    e = exact[ty][name][field].detach().cpu().double()
                    a, b = want[ty][name][field].detach().cpu().double(), got[ty][name][field].detach().cpu().double()
                    if field == "weights":
                        e, a, b = torch.sort(e, -1)[0], torch.sort(a, -1)[0], torch.sort(b, -1)[0]
                    rays = int(torch.tensor(e.shape[:4]).prod())
                    e, a, b = (torch.nan_to_num(t).reshape(rays, -1) for t in (e, a, b))
                    lim = tol["atol"] + tol["rtol"] * e.abs()
                    off_a, off_b = int(((a - e).abs() > lim).any(dim=1).sum()), int(((b - e).abs() > lim).any(dim=1).sum())
                    qa, qb = (float(torch.quantile((t - e).abs().reshape(-1)[:16_000_000], 0.999)) for t in (a, b))
                    fine = off_b <= off_a + 1 and qb <= 2.0 * qa + 1e-6 * float(e.abs().max())
                    isolated[key] = (f"rays beyond the tolerance from float64: HIP {off_b} / fp32 oracle {off_a} of {rays}; 99.9 % quantile "
                                     f"HIP {qb:.2e} / oracle {qa:.2e}", fine)
                if all(v[1] for v in isolated.values()):
                    print("ok (arbitrated, isolated rays) " + label[:150], {k: v[0] for k, v in isolated.items()})
                    continue
            if bad and not hierarchical:
                # a single-pass case beyond the tolerance (1 of 1 340 forward cases of the round-5 sweeps: eight octaves in front of
                # shallow random layers - the fp32 ORACLE is 4.7e-5 from float64 there): the same float64 arbitration, reported under
                # its own label and capped by tests/test_gpu.py::test_randomized_sweep_slice (never a plain "ok")
                state = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
                exact = run_exact(cfg, state, inputs, flags["perturb"], run_both.noise if flags["perturb"] else None,
                                  canonical=flags["canonical"])
                verdict = arbitrate(exact, want, got, factor=4.0, floor=1e-6)
                report = {k: f"HIP {verdict[k][0]:.2e} vs fp32 oracle {verdict[k][1]:.2e} from float64" for k in bad}
                bad = {k: report[k] for k in bad if not verdict[k][2]}
                if not bad:
                    print("ok (arbitrated, single pass) " + label[:150], report)
                    continue
            if bad:
                failures += 1
                print("MISMATCH", label, bad)
                if only is not None:
                    for key in bad:
                        ty, name, field = key.split(".")
                        a, b = want[ty][name][field].detach().cpu().float(), got[ty][name][field].detach().cpu().float()
                        d = (a - b).abs().reshape(-1)
                        idx = int(d.argmax())
                        print("  ", key, "shape", tuple(a.shape), "worst at flat", idx, "oracle", float(a.reshape(-1)[idx]), "hip", float(b.reshape(-1)[idx]),
                              "nan oracle/hip", int(torch.isnan(a).sum()), int(torch.isnan(b).sum()), "entries off", int((d > 1e-3).sum()),
                              "entries beyond the tolerance", int((d > tol["atol"] + tol["rtol"] * a.abs().reshape(-1)).sum()))
                        if True:
                            # the float64 diagnosis entry by entry: is one side off on MORE entries / in its typical error, or do both
                            # sides have a few entries where a resampled position changed its bin (the maxima of two heavy tails)?
                            e = exact[ty][name][field].detach().cpu().double().reshape(-1)
                            ea, eb = (a.double().reshape(-1) - e).abs(), (b.double().reshape(-1) - e).abs()
                            lim = tol["atol"] + tol["rtol"] * e.abs()
                            q = lambda t, f: float(torch.quantile(torch.nan_to_num(t), f))
                            print(f"     vs float64: entries beyond the tolerance oracle {int((ea > lim).sum())} / hip {int((eb > lim).sum())} of {e.numel()}; "
                                  f"rms oracle {float(torch.nan_to_num(ea).square().mean().sqrt()):.2e} / hip {float(torch.nan_to_num(eb).square().mean().sqrt()):.2e}; "
                                  f"99.9 % quantile oracle {q(ea, 0.999):.2e} / hip {q(eb, 0.999):.2e}; max oracle {float(torch.nan_to_num(ea).max()):.2e} / hip {float(torch.nan_to_num(eb).max()):.2e}")
                    # single-case mode: where float64 puts the two fp32 sides (diagnosis only - the sweep's verdict stays MISMATCH)
                    state = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
                    exact = run_exact(cfg, state, inputs, flags["perturb"], run_both.noise if flags["perturb"] else None,
                                      canonical=flags["canonical"])
                    verdict = arbitrate(exact, want, got, factor=4.0, floor=1e-6)
                    for key in bad:
                        print("   float64:", key, f"HIP {verdict[key][0]:.2e}, fp32 oracle {verdict[key][1]:.2e} from the float64 result; within 4 x: {verdict[key][2]}")
            else:
                print("ok (arbitrated)" if arbitrated else "ok", label[:150])
        except Exception:
            failures += 1
            print("ERROR", label)
            traceback.print_exc()
    print(f"{cases} cases, {failures} failures")
    return failures


if __name__ == "__main__":
    main()
