"""The fine guide on the GPU (python -m pytest tests -m gpu): the keep predicate of the resampler and the fine compaction against
its torch restatement, the identities at threshold -inf / +inf, guided renders against the oracle, retention and recorded frames.

Every test sets ``composer.fine_guide`` and asserts on the mask or on fewer evaluated samples.  The scenes are two tennis frames
with one player absent from the second; the rays cross the whole image (most miss a player's box) with a share aimed at each
player; densities of both signs inside every object (``mixed_sigma``), so that threshold 0 neither keeps nor drops everything."""
import pytest
import torch

from oracle import render_oracle as ro
from playableenvironments_amd import configs, synthetic
from playableenvironments_amd import environment_model as em
from playableenvironments_amd.guidance import FineGuide, keep_mask
from tests.helpers import compare_results, composer_inputs, grid_pixels
from tests.test_gpu import ATOL, RTOL, SMALL_NETS, assert_no_farther_than_the_oracle, build, mixed_sigma, run_exact
from tests.test_occupancy_gpu import mask_lookup, object_positions, random_masks, render, same_entries

pytestmark = pytest.mark.gpu

INF = float("inf")
RAYS = (1, 65, 257)                              # rays straddle a 64-lane wave and a 256-ray block
POSITIONS = ((5, 7), (33, 32), (64, 128))        # one partial keep word; a one-bit tail in a third word; six full words
ABSENT = (1, 3)                                  # (frame, object): player_2 is absent from the second frame


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def aimed_pixels(cfg, scene, rays):
    """``rays`` pixels of the image: a third through the box of each player in the first frame (found with the oracle's slab
    test on a 64 x 64 grid), the rest spread over the whole image."""
    h, w = scene["image_size"]
    rows, cols = grid_pixels(h, w, 64)
    o, d, n, w2o, _, _, ins = composer_inputs(cfg, scene, pixels=(rows, cols))
    lay = ro.ObjectLayout(cfg)
    chosen = []
    for k in (2, 3):
        bbox = ro._bbox_tensor(cfg["model"]["object_models"][lay.model_of_object[k]])
        oo, dd, _ = ro.transform_rays(o, d, n, w2o[..., k])
        near, far = ro.raywise_z_bounds(oo, dd, bbox, ins[..., k])
        hits = torch.nonzero((far > near).reshape(-1, rows.numel())[0]).reshape(-1).tolist()
        assert len(hits) >= 8, (k, len(hits))
        step = max(1, len(hits) // max(1, rays // 3))
        chosen += [i for i in hits[::step] if i not in chosen][:max(1, rays // 3)]
    chosen = chosen[:rays]
    spread = [int(i) for i in torch.linspace(0, rows.numel() - 1, 2 * rays + 8).long().tolist()]
    for i in spread:
        if len(chosen) == rays:
            break
        if i not in chosen:
            chosen.append(i)
    assert len(chosen) == rays and len(set(chosen)) == rays
    index = torch.tensor(sorted(chosen))
    return rows[index], cols[index]


_PREPARED = {}


def scene_inputs(rays, positions):
    """(cfg, the seven composer inputs on the CPU): the small tennis networks at ``positions = (Pc, Pf)``, two frames."""
    cfg = configs.reduced_config(configs.tennis_config(hierarchical=positions), **SMALL_NETS)
    key = (rays, positions)
    if key not in _PREPARED:            # (the ray set-up runs once per shape and is left unchanged)
        scene = synthetic.tennis_scene(batch=2, seed=21)
        inputs = [v.contiguous().clone() for v in composer_inputs(cfg, scene, pixels=aimed_pixels(cfg, scene, rays))]
        inputs[6][ABSENT[0], ..., ABSENT[1]] = False
        _PREPARED[key] = inputs
    inputs = [v.clone() for v in _PREPARED[key]]
    assert inputs[1].shape[-2] == rays and inputs[1].reshape(-1, rays, 3).size(0) == 2
    return cfg, inputs


# The density head's scale of the comparison with the oracle.  ``mixed_sigma`` zeroes the head's bias - which alone gives densities of
# both signs, whatever the scale - and multiplies its weights.  At the occupancy suite's 40 the fp32 ORACLE itself is 6 to 75 times
# the suite's tolerance away from its own float64 evaluation on these scenes (the weights of single samples: the inverse-CDF depths
# of near-empty pdf bins are ill-conditioned in fp32, and two neighbouring samples trade weight), so a comparison of maxima would
# measure nothing about the renderer; at 1 it is within 1.3 times the tolerance.  tests/test_fine_guide_cpu.py holds both facts -
# the oracle's own error and that the guide still drops and keeps in-box samples - without the renderer.
ORACLE_SCALE = 1.0
ORACLE_CASES = ((65, (33, 32)), (257, (5, 7)), (65, (64, 128)))


def mixed_composer(cfg, precision="fp32", scale=40.0):
    """Densities of both signs inside every object, as the lossless-grid test of the occupancy suite sets them up."""
    comp = mixed_sigma(build(cfg, alpha_bias=0.0, precision=precision), scale=scale)
    return comp, {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}


def prepare(rays, positions, precision="fp32", scale=40.0):
    """(cfg, composer on the GPU, inputs, state dict)."""
    cfg, inputs = scene_inputs(rays, positions)
    comp, state = mixed_composer(cfg, precision, scale)
    return cfg, comp.cuda(), inputs, state


def guided_objects(cfg):
    return list(range(ro.ObjectLayout(cfg).objects_count))           # (tennis: no skybox, every object has a fine model)


def coarse_density_as_read(cfg, inputs, ex_coarse, k):
    """The raw coarse density of object k as the resampler reads it: the export, or empty_space_alpha where the object is absent."""
    lay = ro.ObjectLayout(cfg)
    m = cfg["model"]["object_models"][lay.model_of_object[k]]
    sigma = ex_coarse["sigma"][k].cpu()
    present = inputs[6][..., k].reshape(-1)                          # (N)
    return torch.where(present.reshape(-1, 1, 1), sigma, torch.full_like(sigma, m["empty_space_alpha"]))


def guide_masks(cfg, inputs, plain, threshold, guard, objects=None):
    """{k: (in box (N, R, Pm), keep_mask (N, R, Pm))} from the exports of a render without the guide."""
    out = {}
    for k in guided_objects(cfg) if objects is None else objects:
        tc = plain["coarse"]["_samples"][0]["t"][k].cpu()
        t = plain["fine"]["_samples"][0]["t"][k].cpu()
        x, bbox, _ = object_positions(cfg, inputs, k, t.reshape(inputs[1].shape[:-1] + (t.size(-1),)))
        inb = ro._in_box(x, bbox).reshape(t.shape)
        out[k] = (inb, keep_mask(tc, coarse_density_as_read(cfg, inputs, plain["coarse"]["_samples"][0], k), t, threshold, guard))
    return out


def median_in_box_density(plain, objects):
    ex = plain["coarse"]["_samples"][0]
    values = torch.cat([ex["sigma"][k].cpu()[ex["slot"][k].cpu() >= 0] for k in objects])
    assert values.numel() > 0
    return float(values.median())


def check_exports(cfg, inputs, plain, got, expected, what):
    """The fine level of ``got`` evaluates exactly ``expected[k]`` (object -> bool mask); everything else is the plain render's."""
    lay = ro.ObjectLayout(cfg)
    a, b = plain["coarse"]["_samples"][0], got["coarse"]["_samples"][0]
    for k in range(lay.objects_count):               # the coarse pass is untouched
        for field in ("t", "sigma", "slot", "delta"):
            assert torch.equal(a[field][k], b[field][k]), (what, "coarse", field, k)
    assert torch.equal(a["evaluated"], b["evaluated"]) and torch.equal(a["head_evaluated"], b["head_evaluated"]), what
    for entry in plain["coarse"]:
        if not entry.startswith("_"):
            for key, v in plain["coarse"][entry].items():
                if torch.is_tensor(v):
                    assert torch.equal(torch.nan_to_num(v), torch.nan_to_num(got["coarse"][entry][key])), (what, entry, key)
    a, b = plain["fine"]["_samples"][0], got["fine"]["_samples"][0]
    for k in range(lay.objects_count):
        empty = cfg["model"]["object_models"][lay.model_of_object[k]]["empty_space_alpha"]
        assert torch.equal(a["t"][k], b["t"][k]), (what, "fine depths", k)                  # a dropped sample keeps its depth
        keep = expected[k]
        slots = b["slot"][k].cpu()
        evaluated = int(b["evaluated"][k])
        print(f"{what}: object {k} evaluates {evaluated} of {int(a['evaluated'][k])} fine samples")
        assert torch.equal(slots >= 0, keep), (what, k, int(((slots >= 0) != keep).sum()))
        assert evaluated == int(keep.sum()), (what, k)
        assert int(b["head_evaluated"][k]) <= evaluated
        flat = slots.reshape(-1)
        assert torch.equal(flat[flat >= 0], torch.arange(evaluated, dtype=torch.int32)), (what, k)
        assert bool((b["sigma"][k].cpu()[~keep] == empty).all()), (what, k)
        assert bool((b["delta"][k].cpu()[~keep] == 0).all()), (what, k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the predicate
@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("rays", RAYS)
def test_the_predicate_is_bit_exact(rays, positions):
    """slot >= 0  <=>  in the box & keep_mask(exports of the unguided render), sample for sample, at both cull sites (the resampler's
    count and the fine fill): the kept slots enumerate 0 .. evaluated - 1 in flat order, which they only do when the counts that
    produced the offsets agree with the fill."""
    cfg, comp, inputs, _ = prepare(rays, positions)
    objects = guided_objects(cfg)
    plain = render(comp, inputs, export=True)
    median = median_in_box_density(plain, objects)
    dropped = kept = 0
    for threshold in (0.0, median):
        for guard in (0, 1, 3):
            comp.fine_guide = FineGuide(threshold=threshold, guard=guard)
            got = render(comp, inputs, export=True)
            masks = guide_masks(cfg, inputs, plain, threshold, guard)
            check_exports(cfg, inputs, plain, got, {k: inb & keep for k, (inb, keep) in masks.items()}, f"threshold {threshold:.3g} guard {guard}")
            dropped += sum(int((inb & ~keep).sum()) for inb, keep in masks.values())
            kept += sum(int((inb & keep).sum()) for inb, keep in masks.values())
    # the absent player evaluates nothing in its absent frame (every coarse density it reads is empty_space_alpha <= 0)
    inb, keep = guide_masks(cfg, inputs, plain, 0.0, 1, [ABSENT[1]])[ABSENT[1]]
    assert not bool(keep[ABSENT[0]].any())
    print(f"rays {rays} positions {positions}: the guide dropped {dropped} and kept {kept} in-box samples over all settings")
    assert dropped > 0
    assert kept > 0 or rays == 1


def test_the_predicate_with_a_fine_occupancy_grid_and_a_subset_of_the_objects():
    cfg, comp, inputs, _ = prepare(257, (33, 32))
    occupancy_masks = random_masks(cfg, 2)
    comp.occupancy = comp.occupancy_from_mask({key: m.cuda() for key, m in occupancy_masks.items()})
    plain = render(comp, inputs, export=True)
    for objects in (None, [1, 3]):
        comp.fine_guide = FineGuide(threshold=0.0, guard=1, objects=objects)
        got = render(comp, inputs, export=True)
        masks = guide_masks(cfg, inputs, plain, 0.0, 1)
        expected = {}
        for k, (inb, keep) in masks.items():
            t = plain["fine"]["_samples"][0]["t"][k].cpu()
            x, bbox, _ = object_positions(cfg, inputs, k, t.reshape(inputs[1].shape[:-1] + (t.size(-1),)))
            bit = mask_lookup(occupancy_masks[(k, "fine")], x, bbox).reshape(t.shape)
            expected[k] = inb & bit & (keep if objects is None or k in objects else torch.ones_like(keep))
        check_exports(cfg, inputs, plain, got, expected, f"fine grid, objects {objects}")
        assert sum(int((inb & ~keep).sum()) for inb, keep in masks.values()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. identities
@pytest.mark.parametrize("rays,positions", [(65, (5, 7)), (257, (33, 32)), (65, (64, 128))])
def test_identities(rays, positions):
    cfg, comp, inputs, _ = prepare(rays, positions)
    K = len(guided_objects(cfg))
    plain = render(comp, inputs, export=True)
    # threshold -inf keeps everything: every entry and export is the unguided render's
    comp.fine_guide = FineGuide(threshold=-INF, guard=0)
    everything = render(comp, inputs, export=True)
    same_entries(plain, everything, "threshold -inf")
    for ty in ("coarse", "fine"):
        a, b = plain[ty]["_samples"][0], everything[ty]["_samples"][0]
        assert torch.equal(a["evaluated"], b["evaluated"]) and torch.equal(a["head_evaluated"], b["head_evaluated"])
        for k in range(K):
            for field in ("t", "sigma", "slot", "delta"):
                assert torch.equal(a[field][k], b[field][k]), (ty, field, k)
    assert int(plain["fine"]["_samples"][0]["evaluated"].sum()) > 0
    # threshold +inf drops everything: the fine level is the one of a render whose fine occupancy masks are all zero
    comp.fine_guide = FineGuide(threshold=INF, guard=3)
    nothing = render(comp, inputs, export=True)
    assert nothing["fine"]["_samples"][0]["evaluated"].tolist() == [0] * K
    comp.fine_guide = None
    comp.occupancy = comp.occupancy_from_mask({(k, "fine"): torch.zeros((2, 2, 2, 2), dtype=torch.bool, device="cuda") for k in range(K)})
    zeros = render(comp, inputs, export=True)
    comp.occupancy = None
    assert zeros["fine"]["_samples"][0]["evaluated"].tolist() == [0] * K
    same_entries(zeros, nothing, "threshold +inf")
    for k in range(K):
        for field in ("t", "sigma", "slot", "delta"):
            assert torch.equal(zeros["fine"]["_samples"][0][field][k], nothing["fine"]["_samples"][0][field][k]), (field, k)
    # an object outside the mask is the unguided render's in its own entry
    comp.fine_guide = FineGuide(threshold=INF, guard=0, objects=[0, 2])
    some = render(comp, inputs, export=True)
    counts = some["fine"]["_samples"][0]["evaluated"].tolist()
    want = plain["fine"]["_samples"][0]["evaluated"].tolist()
    assert counts == [0, want[1], 0, want[3]], (counts, want)
    for k in (1, 3):
        for key, v in plain["fine"][f"object_{k}"].items():
            if torch.is_tensor(v):
                assert torch.equal(torch.nan_to_num(v), torch.nan_to_num(some["fine"][f"object_{k}"][key])), (k, key)
        for field in ("t", "sigma", "slot", "delta"):
            assert torch.equal(plain["fine"]["_samples"][0][field][k], some["fine"]["_samples"][0][field][k]), (field, k)


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the oracle
def oracle_with_keep_masks(cfg, state, inputs, keep, double=False):
    """ro.composer_forward with object_model_forward wrapped: the original runs, then (0, empty_space_alpha, 0) goes where the
    keep mask of that call's object is 0 at the fine level.  Calls arrive with objects ascending, coarse then fine; rows are
    independent in evaluation mode, so masking afterwards equals culling before."""
    lay = ro.ObjectLayout(cfg)
    order = [(k, level) for k in range(lay.objects_count) for level in ("coarse", "fine")]
    calls = []
    original = ro.object_model_forward

    def wrapped(sd, prefix, model_cfg, positions, *args, **kwargs):
        feats, raw, disp = original(sd, prefix, model_cfg, positions, *args, **kwargs)
        k, level = order[len(calls)]
        calls.append(prefix)
        assert prefix.startswith(f"object_models_{level}.")
        if level == "fine" and k in keep:
            mask = keep[k].reshape(raw.shape)
            feats, raw, disp = feats.clone(), raw.clone(), disp.clone()
            feats[~mask] = 0
            raw[~mask] = model_cfg["empty_space_alpha"]
            disp[~mask] = 0
        return feats, raw, disp

    ro.object_model_forward = wrapped
    try:
        with torch.no_grad():
            if double:
                out = run_exact(cfg, state, inputs, False, {})
            else:
                out = ro.composer_forward(cfg, state, *inputs, False, stable_merge=True)
    finally:
        ro.object_model_forward = original
    assert len(calls) == len(order)
    return out


@pytest.mark.parametrize("rays,positions,precision", [(65, (33, 32), "fp32"), (65, (33, 32), "f16x3"), (65, (33, 32), "f16"),
                                                      (257, (5, 7), "fp32"), (65, (64, 128), "fp32")])
def test_guided_render_matches_the_masked_oracle(rays, positions, precision):
    cfg, comp, inputs, state = prepare(rays, positions, precision, scale=ORACLE_SCALE)
    plain = render(comp, inputs, export=True)
    masks = guide_masks(cfg, inputs, plain, 0.0, 1)
    # not an empty cull: the guide drops in-box samples and keeps in-box samples at the guided (fine) level
    dropped = {k: int((inb & ~keep).sum()) for k, (inb, keep) in masks.items()}
    kept = {k: int((inb & keep).sum()) for k, (inb, keep) in masks.items()}
    print(f"{precision} rays {rays} positions {positions}: dropped {dropped}, kept {kept} in-box fine samples")
    assert sum(dropped.values()) >= 1 and sum(kept.values()) >= 1
    want = oracle_with_keep_masks(cfg, state, inputs, {k: keep for k, (_, keep) in masks.items()})
    comp.fine_guide = FineGuide()
    got = render(comp, inputs, export=True)
    assert int(got["fine"]["_samples"][0]["evaluated"].sum()) == sum(kept.values()) < int(plain["fine"]["_samples"][0]["evaluated"].sum())
    del got["coarse"]["_samples"], got["fine"]["_samples"]
    assert set(got) == set(want)
    if precision == "f16":
        # the throughput tier's own rule (test_half_precision_tier_is_close_to_the_oracle): rtol 2e-2 / atol 2e-2 of the peak, >= 40 dB
        for level in ("coarse", "fine"):
            for field in ("integrated_features", "opacity", "depth"):
                w, g = want[level]["global"][field].double(), got[level]["global"][field].cpu().double()
                peak = float(w.abs().max())
                print(f"f16 {level} {field}: max |diff| {float((g - w).abs().max()):.3e}, peak {peak:.3e}")
                assert torch.allclose(g, w, rtol=2e-2, atol=2e-2 * peak), (level, field, float((g - w).abs().max()), peak)
        w, g = want["fine"]["global"]["integrated_features"].double(), got["fine"]["global"]["integrated_features"].cpu().double()
        psnr = 10.0 * torch.log10(w.abs().max() ** 2 / ((g - w) ** 2).mean())
        print(f"f16 PSNR {float(psnr):.1f} dB")
        assert float(psnr) >= 40.0, float(psnr)
        return
    rep = compare_results(want, got, rtol=RTOL, atol=ATOL)
    bad = {k: f"{v[0]:.3e}" for k, v in rep.items() if not v[1]}
    if bad:
        # (no wider tolerance: fields that leave rtol 1e-4 / atol 1e-5 are arbitrated against the float64 oracle, as test_gpu.py does)
        print(f"{precision} rays {rays} positions {positions}: arbitrating {bad} against float64")
        exact = oracle_with_keep_masks(cfg, state, inputs, {k: keep for k, (_, keep) in masks.items()}, double=True)
        assert_no_farther_than_the_oracle(exact, want, got, tuple(bad))


# ---------------------------------------------------------------------------------------------------------------------
# 4. retention
def test_guided_and_retained():
    from tests.test_retention_gpu import check, expectations
    cfg, comp, inputs, _ = prepare(257, (33, 32))
    K, static, none, reuse = expectations(comp)
    assert 1 <= static < K
    comp.fine_guide = FineGuide()
    unguided_fine = None
    comp.retained = comp.retain_objects()
    want, _ = check(comp, inputs, none, "populate")                  # (against the guided call without retention)
    comp.fine_guide, kept_guide = None, comp.fine_guide
    comp.retained, kept_retained = None, comp.retained
    unguided_fine = render(comp, inputs, export=True)["fine"]["_samples"][0]["evaluated"]
    comp.fine_guide, comp.retained = kept_guide, kept_retained
    assert int(want["fine"]["_samples"][0]["evaluated"].sum()) < int(unguided_fine.sum())          # the guide is at work
    check(comp, inputs, reuse, "reuse")                               # flags set, bit-identical, fine evaluated == 0 for the reused
    # another guard, another threshold, another mask: nothing is reused on the next frame, everything static on the one after
    comp.fine_guide.guard = 2
    check(comp, inputs, none, "guard changed")
    check(comp, inputs, reuse, "guard changed, recovered")
    comp.fine_guide.threshold = 0.25
    check(comp, inputs, none, "threshold changed")
    check(comp, inputs, reuse, "threshold changed, recovered")
    comp.fine_guide.objects = [0, 2]
    check(comp, inputs, none, "mask changed")
    check(comp, inputs, reuse, "mask changed, recovered")
    comp.fine_guide = None
    check(comp, inputs, none, "guide cleared")
    check(comp, inputs, reuse, "guide cleared, recovered")


# ---------------------------------------------------------------------------------------------------------------------
# 5. recorded frames
def test_recorded_frames_with_a_guide():
    from playableenvironments_amd.frame_graph import FrameGraph, SCENE_KEYS
    cfg = configs.reduced_config(configs.tennis_config(hierarchical=(33, 32)), **SMALL_NETS)
    model = em.EnvironmentModel(cfg)
    synthetic.randomize_module_state(model.object_composer, seed=0, step=20000, alpha_bias=0.0, bender_scale=1e4)
    mixed_sigma(model.object_composer)
    model = model.eval().cuda()
    comp = model.object_composer
    size = (24, 40)
    scenes = [{k: v.cuda() for k, v in synthetic.tennis_scene(seed=s, image_size=size).items() if torch.is_tensor(v)} for s in (5, 6)]

    def eager(scene):
        replay, model.frame_replay = model.frame_replay, None
        try:
            with torch.no_grad():
                out = model(*[scene[k] for k in SCENE_KEYS[:3]], size, *[scene[k] for k in SCENE_KEYS[3:]], 0, False, mode="scene_encodings")
            torch.cuda.synchronize()
            return {ty: {e: {k: v.clone() for k, v in out[ty][e].items() if torch.is_tensor(v)} for e in out[ty] if isinstance(out[ty][e], dict)}
                    for ty in ("coarse", "fine")}
        finally:
            model.frame_replay = replay

    def same(a, b, what):
        for ty in ("coarse", "fine"):
            entries = [e for e in b[ty] if "weights" in b[ty][e]]
            assert "global" in entries and len(entries) > 1
            for entry in entries:
                for key in ("integrated_features", "opacity", "depth", "weights"):
                    assert torch.equal(a[ty][entry][key], b[ty][entry][key]), (what, ty, entry, key)

    def differs(a, b):
        return not torch.equal(a["fine"]["global"]["weights"], b["fine"]["global"]["weights"])

    unguided = [eager(s) for s in scenes]
    comp.fine_guide = FineGuide()
    guided = [eager(s) for s in scenes]
    assert differs(unguided[0], guided[0]) and differs(unguided[1], guided[1])            # the guide changes these frames
    graph = FrameGraph(model, scenes[0], size)
    print("census of the guided recording", graph.census)
    assert graph.census["memsets"] == 0 and graph.census["kernels"] > 0
    assert graph.census["kernels"] == graph.census["nodes"], graph.census                 # kernel nodes only
    for i in (0, 1, 0):
        got = graph.render(scenes[i])
        torch.cuda.synchronize()
        same(got, guided[i], f"replay of scene {i}")
    # changing, clearing or swapping the guide never replays the stale recording
    comp.fine_guide.guard = 3
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[0])
    comp.fine_guide.guard = 1
    graph.render(scenes[0])
    comp.fine_guide.threshold = 0.5
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[0])
    comp.fine_guide = None
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[0])
    comp.fine_guide = FineGuide()
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[0])
    torch.cuda.synchronize()
    # the automatic recordings (frame_replay = "clone") key on the guide as well
    model.frame_replay = "clone"

    def replayed(scene):
        with torch.no_grad():
            out = model(*[scene[k] for k in SCENE_KEYS[:3]], size, *[scene[k] for k in SCENE_KEYS[3:]], 0, False, mode="scene_encodings")
        torch.cuda.synchronize()
        return out

    for _ in range(3):                       # eager, recorded, replayed
        out = replayed(scenes[0])
    assert any(entry[1] not in (None, False) for entry in model._replays.values())
    same(out, guided[0], "replay, default guide")
    comp.fine_guide.guard = 0
    want = eager(scenes[0])
    assert differs(want, guided[0])
    for i in range(3):
        same(replayed(scenes[0]), want, f"replay {i}, guard 0")
    comp.fine_guide = None
    for i in range(3):
        same(replayed(scenes[0]), unguided[0], f"replay {i}, no guide")
