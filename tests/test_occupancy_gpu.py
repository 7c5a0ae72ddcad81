"""Occupancy grids (empty-space skipping of evaluation renders) on the GPU (python -m pytest tests -m gpu): the build kernel, the three
cull sites against the torch restatement of the lookup, culled renders against the oracle, lossless grids, grids that follow the
scene and recorded frames."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import render_oracle as ro
from playableenvironments_amd import _lib, configs, occupancy, synthetic
from playableenvironments_amd import environment_model as em
from playableenvironments_amd.object_composer import ENTRY_KEYS
from tests.helpers import compare_results, composer_inputs, grid_pixels
from tests.test_gpu import ATOL, CASES, RTOL, SMALL_NETS, assert_no_farther_than_the_oracle, build, mixed_sigma, run_exact

pytestmark = pytest.mark.gpu

RENDER_CASES = ("tennis", "minecraft", "tennis_hierarchical")
CELLS = (16, 16, 16)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def restate_build(sigma, s, threshold, d):
    """The build kernel in torch: max over the s^3 blocks, > threshold, dilation by a (2d + 1)^3 max pool clipped at the box."""
    x = sigma.unsqueeze(1)
    if s > 1:
        x = F.max_pool3d(x, s)
    occ = (x > threshold).float()
    if d > 0:
        occ = F.max_pool3d(occ, 2 * d + 1, stride=1, padding=d)
    return occ[:, 0] > 0.5


def run_build(sigma, cells, s, threshold, d):
    G = sigma.size(0)
    words = occupancy.words_of(cells)
    bits = torch.full((G, words), 0x5A5A5A5A, dtype=torch.int32, device="cuda")         # (every word must be written)
    sigma = sigma.contiguous().cuda()
    _lib.check(_lib.load().pr_occupancy_build(sigma.data_ptr(), G, (C.c_int32 * 3)(*cells), s, threshold, d, bits.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "pr_occupancy_build")
    torch.cuda.synchronize()
    return bits.cpu()


def prepare(name, precision="fp32", sigma="default", n=None):
    make_cfg, make_scene, rays, bias = CASES[name]
    cfg, scene = make_cfg(), make_scene()
    comp = build(cfg, alpha_bias=bias, precision=precision) if sigma == "default" else mixed_sigma(build(cfg, alpha_bias=0.0, precision=precision))
    inputs = composer_inputs(cfg, scene, pixels=grid_pixels(scene["image_size"][0], scene["image_size"][1], n or rays))
    state = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
    return cfg, comp.cuda(), inputs, state


def frames_of(inputs):
    lead = inputs[1].shape[:-2]
    return int(torch.tensor(lead).prod()) if len(lead) else 1


def grid_objects(cfg):
    """[(object, [levels])] of the objects that can carry a grid (not the skybox)."""
    lay = ro.ObjectLayout(cfg)
    out = []
    for k in range(lay.objects_count):
        m = cfg["model"]["object_models"][lay.model_of_object[k]]
        if m["nerf_model"]["architecture"].endswith("skybox_adain_style_nerf_model_v3"):
            continue
        out.append((k, ["coarse", "fine"] if m.get("use_fine", True) is not False else ["coarse"]))
    return out


def random_masks(cfg, frames, cells=CELLS, p=0.5):
    """A seeded 50 % mask per object instance and level, all different."""
    masks = {}
    for k, levels in grid_objects(cfg):
        for j, level in enumerate(levels):
            g = torch.Generator().manual_seed(7000 + 10 * k + j)
            masks[(k, level)] = torch.rand((frames,) + tuple(cells), generator=g) < p
    return masks


def render(comp, inputs, export=False):
    with torch.no_grad():
        out = comp(*[v.cuda() for v in inputs], False, _export=export)
    torch.cuda.synchronize()
    return out


def same_entries(a, b, what):
    for ty in [t for t in ("coarse", "fine") if t in a]:
        assert set(a[ty]) == set(b[ty])
        for entry in a[ty]:
            if entry.startswith("_"):
                continue
            for key in ENTRY_KEYS:
                x, y = a[ty][entry][key], b[ty][entry][key]
                assert torch.equal(torch.isnan(x), torch.isnan(y)), (what, ty, entry, key)
                assert torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)), (what, ty, entry, key, float((x - y).abs().max()))


def object_positions(cfg, inputs, k, t=None):
    """Object-frame sample positions of object k as the kernels form them: the oracle's coarse placement, or o + d t for exported
    depths ``t``.  Returns (x (..., R, P, 3), bbox, model config)."""
    o, d, n, w2o, sty, dfm, ins = inputs
    lay = ro.ObjectLayout(cfg)
    m = cfg["model"]["object_models"][lay.model_of_object[k]]
    bbox = ro._bbox_tensor(m)
    oo, dd, _ = ro.transform_rays(o, d, n, w2o[..., k])
    if t is None:
        near, far = ro.raywise_z_bounds(oo, dd, bbox, ins[..., k])
        near = near.clamp(m["z_near_min"], m["z_far_max"])
        far = far.clamp(m["z_near_min"], m["z_far_max"])
        x, t, _ = ro.stratified_positions(oo, dd, near, far, m["positions_count_coarse"], False)
    else:
        x = oo.unsqueeze(-2).unsqueeze(-2) + dd.unsqueeze(-2) * t.unsqueeze(-1)
    return x, bbox, m


def mask_lookup(mask, x, bbox):
    """mask[frame][cell_index(x)] for x (..., R, P, 3) whose leading dimensions are the frames."""
    N = mask.size(0)
    cell = occupancy.cell_index(x.reshape(N, -1, 3), bbox, mask.shape[1:])
    return torch.gather(mask.reshape(N, -1), 1, cell).reshape(x.shape[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the build kernel
@pytest.mark.parametrize("cells", [(16, 16, 16), (5, 3, 7), (4, 4, 2), (1, 1, 1), (3, 33, 2)])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_occupancy_build_equals_the_torch_restatement(cells, s, d):
    torch.manual_seed(cells[0] * 100 + s * 10 + d)
    shape = (3,) + tuple(c * s for c in cells)
    lattices = {"random": (torch.randn(shape), 1.2), "sparse": (torch.randn(shape), 2.5), "all_cold": (torch.full(shape, -1.0), 0.0),
                "all_hot": (torch.full(shape, 1.0), 0.0), "on_threshold": (torch.zeros(shape), 0.0)}       # (> is strict)
    corner = torch.full(shape, -1.0)
    corner[0, 0, 0, 0] = 5.0
    corner[1, -1, -1, -1] = 5.0
    corner[2, 0, -1, 0] = 5.0
    lattices["corner"] = (corner, 0.0)
    words = occupancy.words_of(cells)
    total = cells[0] * cells[1] * cells[2]
    for name, (sigma, threshold) in lattices.items():
        want_mask = restate_build(sigma, s, threshold, d)
        got = run_build(sigma, cells, s, threshold, d)
        assert torch.equal(got, occupancy.pack_bits(want_mask)), (name, cells, s, d)
        if total % 32:            # tail bits of the last word are 0
            assert int(got[0, words - 1]) & 0xFFFFFFFF < (1 << (total % 32)), name
    assert bool(restate_build(lattices["all_hot"][0], s, 0.0, d).all()) and not bool(restate_build(lattices["all_cold"][0], s, 0.0, d).any())
    assert int(restate_build(corner, s, 0.0, d)[0].sum()) == min(d + 1, cells[0]) * min(d + 1, cells[1]) * min(d + 1, cells[2])


# ---------------------------------------------------------------------------------------------------------------------
# 2. off == all ones
@pytest.mark.parametrize("name", RENDER_CASES)
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_no_grid_and_an_all_ones_grid_are_identical(name, precision):
    cfg, comp, inputs, _ = prepare(name, precision)
    N = frames_of(inputs)
    assert comp.occupancy is None
    plain = render(comp, inputs, export=True)
    comp.occupancy = comp.occupancy_from_mask({key: torch.ones((N, 8, 6, 5), dtype=torch.bool, device="cuda")
                                               for key in random_masks(cfg, N)})
    assert len(comp.occupancy.grids) >= 2
    ones = render(comp, inputs, export=True)
    same_entries(plain, ones, "all ones")
    for ty in [t for t in ("coarse", "fine") if t in plain]:
        a, b = plain[ty]["_samples"][0], ones[ty]["_samples"][0]
        assert torch.equal(a["evaluated"], b["evaluated"]) and torch.equal(a["head_evaluated"], b["head_evaluated"])
        for k in range(len(a["slot"])):
            assert torch.equal(a["slot"][k], b["slot"][k]) and torch.equal(a["sigma"][k], b["sigma"][k])
    # ... and a grid of zeros evaluates nothing of the objects that carry one
    comp.occupancy = comp.occupancy_from_mask({key: torch.zeros((N, 8, 6, 5), dtype=torch.bool, device="cuda")
                                               for key in random_masks(cfg, N)})
    none = render(comp, inputs, export=True)
    for ty in [t for t in ("coarse", "fine") if t in none]:
        for k, _levels in grid_objects(cfg):
            assert int(none[ty]["_samples"][0]["evaluated"][k]) == 0
            assert bool((none[ty]["_samples"][0]["slot"][k] == -1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. geometry
@pytest.mark.parametrize("name", RENDER_CASES)
def test_culled_geometry_is_bit_exact(name):
    """slot >= 0  <=>  in the box and the mask bit of cell_index(x) set, at all three cull sites (the coarse count and fill, the
    resampler's count and the fine fill): kept slots enumerate 0 .. evaluated - 1 in flat order, which they only do when the
    counts that produced the offsets agree with the fill."""
    cfg, comp, inputs, _ = prepare(name)
    N = frames_of(inputs)
    masks = random_masks(cfg, N)
    plain = render(comp, inputs, export=True)
    comp.occupancy = comp.occupancy_from_mask({key: m.cuda() for key, m in masks.items()})
    got = render(comp, inputs, export=True)
    checked = 0
    for ty in [t for t in ("coarse", "fine") if t in got]:
        ex, ex_plain = got[ty]["_samples"][0], plain[ty]["_samples"][0]
        for k in range(len(ex["slot"])):
            t = ex["t"][k].cpu()
            x, bbox, m = object_positions(cfg, inputs, k, None if ty == "coarse" else t.reshape(inputs[1].shape[:-1] + (t.size(-1),)))
            inb = ro._in_box(x, bbox)
            keep = inb & mask_lookup(masks[(k, ty)], x, bbox) if (k, ty) in masks else inb
            slots = ex["slot"][k].cpu()
            assert torch.equal((slots >= 0).reshape(keep.shape), keep), (ty, k)
            assert int(ex["evaluated"][k]) == int(keep.sum()), (ty, k)
            flat = slots.reshape(-1)
            assert torch.equal(flat[flat >= 0], torch.arange(int(keep.sum()), dtype=torch.int32)), (ty, k)
            if ty == "coarse":            # depths are untouched by the grid; culled samples carry the empty-space density
                assert torch.equal(ex["t"][k], ex_plain["t"][k])
            assert bool((ex["sigma"][k].cpu().reshape(keep.shape)[~keep] == m["empty_space_alpha"]).all())
            assert bool((ex["delta"][k].cpu().reshape(keep.shape + (3,))[~keep] == 0).all())
            if (k, ty) in masks:
                unculled = int(inb.sum())
                print(f"{name} {ty} object {k}: evaluated {int(keep.sum())} of {unculled} in-box samples")
                if unculled >= 64:
                    assert int(keep.sum()) < unculled, (ty, k)
                    checked += 1
                else:         # (a 50 % mask may keep every one of a handful of samples: said, not asserted)
                    print(f"{name} {ty} object {k}: only {unculled} in-box samples, 'strictly fewer' not asserted")
            else:
                assert int(ex["evaluated"][k]) == int(inb.sum())
    assert checked >= 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. against the oracle
def oracle_with_masks(cfg, state, inputs, masks, double=False):
    """ro.composer_forward with object_model_forward wrapped: the original runs, then (0, empty_space_alpha, 0) goes where the
    mask bit of that call's object, level and frame is 0.  Calls arrive with objects ascending, coarse then fine; rows are
    independent in evaluation mode, so masking afterwards equals culling before."""
    lay = ro.ObjectLayout(cfg)
    order = []
    for k in range(lay.objects_count):
        m = cfg["model"]["object_models"][lay.model_of_object[k]]
        order.append((k, "coarse"))
        if m.get("use_fine", True) is not False:
            order.append((k, "fine"))
    calls = []
    original = ro.object_model_forward

    def wrapped(sd, prefix, model_cfg, positions, *args, **kwargs):
        feats, raw, disp = original(sd, prefix, model_cfg, positions, *args, **kwargs)
        k, level = order[len(calls)]
        calls.append(prefix)
        assert prefix.startswith(f"object_models_{level}.")
        mask = masks.get((k, level))
        if mask is not None:
            keep = mask_lookup(mask, positions.float(), ro._bbox_tensor(model_cfg).float())
            feats, raw, disp = feats.clone(), raw.clone(), disp.clone()
            feats[~keep] = 0
            raw[~keep] = model_cfg["empty_space_alpha"]
            disp[~keep] = 0
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


@pytest.mark.parametrize("name", RENDER_CASES)
@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16"])
def test_culled_render_matches_the_masked_oracle(name, precision):
    cfg, comp, inputs, state = prepare(name, precision)
    N = frames_of(inputs)
    masks = random_masks(cfg, N)
    want = oracle_with_masks(cfg, state, inputs, masks)
    comp.occupancy = comp.occupancy_from_mask({key: m.cuda() for key, m in masks.items()})
    got = render(comp, inputs)
    assert set(got) == set(want)
    if precision == "f16":
        # the throughput tier's own rule (test_half_precision_tier_is_close_to_the_oracle): rtol 2e-2 / atol 2e-2 of the peak, >= 40 dB
        last = "fine" if "fine" in got else "coarse"
        for level in [t for t in ("coarse", "fine") if t in got]:
            for field in ("integrated_features", "opacity", "depth"):
                w, g = want[level]["global"][field].double(), got[level]["global"][field].cpu().double()
                peak = float(w.abs().max())
                assert torch.allclose(g, w, rtol=2e-2, atol=2e-2 * peak), (level, field, float((g - w).abs().max()), peak)
        w, g = want[last]["global"]["integrated_features"].double(), got[last]["global"]["integrated_features"].cpu().double()
        psnr = 10.0 * torch.log10(w.abs().max() ** 2 / ((g - w) ** 2).mean())
        assert float(psnr) >= 40.0, float(psnr)
        return
    rep = compare_results(want, got, rtol=RTOL, atol=ATOL)
    bad = {k: f"{v[0]:.3e}" for k, v in rep.items() if not v[1]}
    if bad:
        # (no wider tolerance: fields that leave rtol 1e-4 / atol 1e-5 are arbitrated against the float64 oracle, as test_gpu.py does)
        print(f"{name} {precision}: arbitrating {bad} against float64")
        exact = oracle_with_masks(cfg, state, inputs, masks, double=True)
        assert_no_farther_than_the_oracle(exact, want, got, tuple(bad))


# ---------------------------------------------------------------------------------------------------------------------
# 5. a lossless grid
@pytest.mark.parametrize("name", RENDER_CASES)
def test_a_grid_that_keeps_every_positive_density_changes_nothing(name):
    """Cells that hold at least one sample with density > 0 stay; every culled sample then has alpha exactly 0 with and without
    the grid, so every integrated field - coarse, and fine behind the resampler that reads the coarse weights - must be
    bit-identical at fp32 while fewer samples are evaluated."""
    cfg, comp, inputs, _ = prepare(name, sigma="mixed")
    N = frames_of(inputs)
    plain = render(comp, inputs, export=True)
    masks = {}
    for ty in [t for t in ("coarse", "fine") if t in plain]:
        ex = plain[ty]["_samples"][0]
        for k, levels in grid_objects(cfg):
            if ty not in levels:
                continue
            t = ex["t"][k].cpu()
            x, bbox, _ = object_positions(cfg, inputs, k, t.reshape(inputs[1].shape[:-1] + (t.size(-1),)))
            live = (ex["sigma"][k].cpu() > 0).reshape(N, -1) & (ex["slot"][k].cpu() >= 0).reshape(N, -1)
            cell = occupancy.cell_index(x.reshape(N, -1, 3), bbox, CELLS)
            mask = torch.zeros((N, CELLS[0] * CELLS[1] * CELLS[2]), dtype=torch.bool)
            for f in range(N):
                mask[f, cell[f][live[f]]] = True
            masks[(k, ty)] = mask.reshape((N,) + CELLS)
    comp.occupancy = comp.occupancy_from_mask({key: m.cuda() for key, m in masks.items()})
    got = render(comp, inputs, export=True)
    same_entries(plain, got, "lossless grid")
    dropped = 0
    for ty in [t for t in ("coarse", "fine") if t in plain]:
        a, b = plain[ty]["_samples"][0]["evaluated"].cpu(), got[ty]["_samples"][0]["evaluated"].cpu()
        print(f"{name} {ty}: evaluated {a.tolist()} -> {b.tolist()}")
        assert bool((b <= a).all())
        assert int(b.sum()) < int(a.sum()), ty
        dropped += int(a.sum() - b.sum())
    assert dropped > 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. build_occupancy / update / follow
def test_build_occupancy_update_and_follow():
    """Densities of both signs (mixed_sigma) and no dilation, so that the grids are neither full nor empty and move with the
    deformation code: a stale ``update`` / ``follow`` cannot pass."""
    cfg, comp, inputs, _ = prepare("tennis_hierarchical", sigma="mixed")
    other = composer_inputs(cfg, synthetic.tennis_scene(seed=77), pixels=grid_pixels(256, 256, 16))
    K = comp.object_id_helper.objects_count
    style, deformation = inputs[4].cuda(), inputs[5].cuda()
    N = frames_of(inputs)
    res, ss, thr, dil = (8, 8, 8), 2, 0.0, 0

    def restated(k, level, sty, dfm):
        """The bits of one grid from density_grid + the torch restatement: independent of build_occupancy / update."""
        sigma, _ = comp.density_grid(k, [r * ss for r in res], sty[..., k].reshape(N, -1), dfm[..., k].reshape(N, -1), fine=level == "fine")
        return occupancy.pack_bits(restate_build(sigma, ss, thr, dil))

    with torch.no_grad():
        occ = comp.build_occupancy(style, deformation, resolution=res, supersample=ss, threshold=thr, dilate=dil)
        assert occ.frames == N and set(occ.grids) == {(k, level) for k in range(K) for level in ("coarse", "fine")}
        for (k, level), g in occ.grids.items():
            assert torch.equal(g["bits"], restated(k, level, style, deformation)), (k, level)
        kept = occ.kept_fraction()
        print("kept fractions", kept)
        assert any(0.0 < v < 1.0 for v in kept.values()), kept
        # in-place update: same storage, new bits for new codes - checked against the independent restatement
        before = {key: (g["bits"].data_ptr(), g["bits"].clone()) for key, g in occ.grids.items()}
        other_style, other_deformation = other[4].cuda(), other[5].cuda()
        occ.update(other_style, other_deformation)
        fresh = comp.build_occupancy(other_style, other_deformation, resolution=res, supersample=ss, threshold=thr, dilate=dil)
        changed = 0
        for (k, level), g in occ.grids.items():
            assert g["bits"].data_ptr() == before[(k, level)][0]
            assert torch.equal(g["bits"], restated(k, level, other_style, other_deformation)), (k, level)
            assert torch.equal(g["bits"], fresh.grids[(k, level)]["bits"])
            changed += int(not torch.equal(g["bits"], before[(k, level)][1]))
        print("grids changed by the update", changed)
        assert changed >= 1
        with pytest.raises(ValueError, match="frame"):
            occ.update(torch.cat([style, style]), torch.cat([deformation, deformation]))
        # follow: two scenes in a row equal a freshly built grid each
        follower = comp.build_occupancy(style, deformation, resolution=res, supersample=ss, threshold=thr, dilate=dil)
        follower.follow = True
        for scene_inputs in (other, inputs):
            comp.occupancy = follower
            stale = {key: g["bits"].clone() for key, g in follower.grids.items()}
            got = render(comp, scene_inputs, export=True)
            assert any(not torch.equal(stale[key], g["bits"]) for key, g in follower.grids.items())     # (the render rebuilt the bits)
            comp.occupancy = comp.build_occupancy(scene_inputs[4].cuda(), scene_inputs[5].cuda(), resolution=res, supersample=ss,
                                                  threshold=thr, dilate=dil)
            assert comp.occupancy.follow is False
            want = render(comp, scene_inputs, export=True)
            same_entries(want, got, "follow")
            for ty in ("coarse", "fine"):
                assert torch.equal(want[ty]["_samples"][0]["evaluated"], got[ty]["_samples"][0]["evaluated"])
    # a perturbed call never sees the grid
    comp.occupancy = comp.occupancy_from_mask({2: torch.zeros((N, 2, 2, 2), dtype=torch.bool, device="cuda")})
    with torch.no_grad():
        torch.manual_seed(1)
        noisy = comp(*[v.cuda() for v in inputs], True, _export=True)
        comp.occupancy = None
        plain = render(comp, inputs, export=True)
    assert int(plain["coarse"]["_samples"][0]["evaluated"][2]) > 0 and int(noisy["coarse"]["_samples"][0]["evaluated"][2]) > 0
    # a call with another frame count names both numbers
    comp.occupancy = comp.occupancy_from_mask({2: torch.ones((N + 1, 2, 2, 2), dtype=torch.bool, device="cuda")})
    with pytest.raises(ValueError, match=rf"{N + 1} frame\(s\).*renders {N}"):
        render(comp, inputs)


# ---------------------------------------------------------------------------------------------------------------------
# 7. recorded frames
def test_recorded_frames_with_a_grid():
    from playableenvironments_amd.frame_graph import FrameGraph, SCENE_KEYS
    cfg = configs.reduced_config(configs.minecraft_config(), **SMALL_NETS)
    model = em.EnvironmentModel(cfg)
    synthetic.randomize_module_state(model.object_composer, seed=0, step=20000, alpha_bias=0.0, bender_scale=1e4)
    mixed_sigma(model.object_composer)
    model = model.eval().cuda()
    comp = model.object_composer
    size = (64, 96)
    scenes = [{k: v.cuda() for k, v in synthetic.minecraft_scene(seed=s, image_size=size).items() if torch.is_tensor(v)} for s in (5, 6, 7)]
    codes = lambda scene: (scene["object_style"], scene["object_deformation"])

    def eager(scene):
        replay, model.frame_replay = model.frame_replay, None
        try:
            with torch.no_grad():
                out = model(*[scene[k] for k in SCENE_KEYS[:3]], size, *[scene[k] for k in SCENE_KEYS[3:]], 0, False, mode="scene_encodings")
            torch.cuda.synchronize()
            return {ty: {e: {k: v.clone() for k, v in out[ty][e].items() if torch.is_tensor(v)} for e in out[ty] if isinstance(out[ty][e], dict)}
                    for ty in ("coarse",)}
        finally:
            model.frame_replay = replay

    def same(a, b, what):
        entries = [e for e in a["coarse"] if isinstance(a["coarse"][e], dict) and "weights" in a["coarse"][e]]
        assert "global" in entries and len(entries) > 1
        for entry in entries:
            for key in ("integrated_features", "opacity", "depth", "weights"):
                assert torch.equal(a["coarse"][entry][key], b["coarse"][entry][key]), (what, entry, key)

    build_args = dict(resolution=8, supersample=2, threshold=0.0, dilate=0)
    with torch.no_grad():
        occ = comp.build_occupancy(*codes(scenes[0]), **build_args)
    unculled = eager(scenes[1])
    comp.occupancy = occ
    kept = occ.kept_fraction()
    print("kept fractions", kept)
    assert any(0.0 < v < 1.0 for v in kept.values()), kept          # (a full grid could not tell new bits from old ones)
    # follow = False: replays read whatever update last wrote
    graph = FrameGraph(model, scenes[0], size)
    assert graph.census["memsets"] == 0 and graph.census["kernels"] > 0
    same(graph.render(scenes[0]), eager(scenes[0]), "captured scene")
    captured_bits = {key: g["bits"].clone() for key, g in occ.grids.items()}
    occ.update(*codes(scenes[1]))
    assert any(not torch.equal(captured_bits[key], g["bits"]) for key, g in occ.grids.items())
    got = graph.render(scenes[1])
    torch.cuda.synchronize()
    want = eager(scenes[1])
    same(got, want, "after update")
    if not torch.equal(want["coarse"]["global"]["weights"], unculled["coarse"]["global"]["weights"]):
        print("the grid changes the frame (cells with matter thinner than the lattice were culled)")
    # follow = True: the build launches are part of the recording
    occ.follow = True
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[1])
    graph = FrameGraph(model, scenes[0], size)
    assert graph.census["memsets"] == 0
    for scene in (scenes[2], scenes[1]):
        stale = {key: g["bits"].clone() for key, g in occ.grids.items()}
        got = graph.render(scene)
        torch.cuda.synchronize()
        assert any(not torch.equal(stale[key], g["bits"]) for key, g in occ.grids.items())       # (the replay rebuilt the bits)
        with torch.no_grad():
            fresh = comp.build_occupancy(*codes(scene), **build_args)
        comp.occupancy = fresh
        want = eager(scene)
        comp.occupancy = occ
        same(got, want, "follow")
        same(got, eager(scene), "follow, eager")
    # clearing or swapping the grid never replays the stale recording
    comp.occupancy = None
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[0])
    comp.occupancy = fresh
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scenes[0])
    # the automatic recordings (frame_replay = "clone") key on the grid as well
    N = occ.frames
    targets = [key for key in occ.grids]
    first = comp.occupancy_from_mask({key: torch.ones((N, 4, 4, 4), dtype=torch.bool, device="cuda") for key in targets})
    g = torch.Generator().manual_seed(3)
    second = comp.occupancy_from_mask({key: (torch.rand((N, 4, 4, 4), generator=g) < 0.5).cuda() for key in targets})
    model.frame_replay = "clone"

    def replayed(scene):
        with torch.no_grad():
            out = model(*[scene[k] for k in SCENE_KEYS[:3]], size, *[scene[k] for k in SCENE_KEYS[3:]], 0, False, mode="scene_encodings")
        torch.cuda.synchronize()
        return out

    comp.occupancy = first
    for _ in range(3):                       # eager, recorded, replayed
        out = replayed(scenes[0])
    assert any(entry[1] not in (None, False) for entry in model._replays.values())
    same(out, eager(scenes[0]), "replay, first grid")
    comp.occupancy = second
    want = eager(scenes[0])
    assert not torch.equal(want["coarse"]["global"]["weights"], out["coarse"]["global"]["weights"])
    for i in range(3):
        same(replayed(scenes[0]), want, f"replay {i}, second grid")
    comp.occupancy = None
    want = eager(scenes[0])
    for i in range(3):
        same(replayed(scenes[0]), want, f"replay {i}, no grid")
