"""Retained per-sample state across evaluation frames on the GPU (python -m pytest tests -m gpu): a retained render is bit for bit
the plain render, a reused object does no MLP work, and every input an object's state depends on makes exactly that state stale.

"Plain" = the same composer with ``retained = None``.  Bitwise equality alone cannot tell reuse from recomputation, so every
reuse assertion comes with ``last_reused[k] == 1`` and ``evaluated_samples[k] == 0``, every staleness assertion with
``last_reused[k] == 0``."""
import pytest
import torch

from playableenvironments_amd import configs, synthetic
from playableenvironments_amd import environment_model as em
from tests.helpers import composer_inputs, grid_pixels
from tests.test_gpu import CASES, SMALL_NETS, build, mixed_sigma
from tests.test_occupancy_gpu import frames_of, prepare as prepare_full, random_masks, same_entries

pytestmark = pytest.mark.gpu

RENDER_CASES = ("tennis", "minecraft", "tennis_hierarchical")
SIDE = 23       # 23 x 23 = 529 rays: three 256-ray blocks with a tail, 1587 direction words (no multiple of 4 x 64)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


# ---------------------------------------------------------------------------------------------------------------------
# helpers
def prepare(name, precision="fp32", defer=True, side=SIDE):
    make_cfg, make_scene, _, bias = CASES[name]
    cfg, scene = configs.reduced_config(make_cfg(), **SMALL_NETS), make_scene()
    comp = build(cfg, alpha_bias=bias, precision=precision)
    comp.defer_feature_projection = defer
    inputs = composer_inputs(cfg, scene, pixels=grid_pixels(scene["image_size"][0], scene["image_size"][1], side))
    return cfg, comp.cuda(), [v.contiguous().clone() for v in inputs]


def render(comp, inputs):
    with torch.no_grad():
        out = comp(*[v.cuda() for v in inputs], False, _export=True)
    torch.cuda.synchronize()
    return out


def plain(comp, inputs):
    kept, comp.retained = comp.retained, None
    try:
        return render(comp, inputs)
    finally:
        comp.retained = kept


def levels(out):
    return [t for t in ("coarse", "fine") if t in out]


def check(comp, inputs, expect, what):
    """One retained render against the plain one: every entry field, the per-sample exports, the reuse flags and the MLP work."""
    if comp._workspace is not None:
        comp._workspace.fill_(0xFF)                    # NaN bytes: reuse cannot lean on what the workspace held
    got = render(comp, inputs)
    flags = comp.retained.last_reused.tolist()
    want = plain(comp, inputs)
    same_entries(want, got, what)
    assert flags == list(expect), (what, flags, list(expect))
    for ty in levels(want):
        a, b = want[ty]["_samples"][0], got[ty]["_samples"][0]
        for k in range(len(expect)):
            for field in ("t", "sigma", "slot"):
                assert torch.equal(a[field][k], b[field][k]), (what, ty, field, k)
            if expect[k]:
                assert int(b["evaluated"][k]) == 0 and int(b["head_evaluated"][k]) == 0, (what, ty, k)
            else:
                assert int(b["evaluated"][k]) == int(a["evaluated"][k]), (what, ty, k)
                assert int(b["head_evaluated"][k]) == int(a["head_evaluated"][k]), (what, ty, k)
    return want, got


def expectations(comp):
    helper = comp.object_id_helper
    K, static = helper.objects_count, helper.static_objects_count
    none = [0] * K
    reuse = [1 if k < static else 0 for k in range(K)]
    return K, static, none, reuse


def ulp(t, index):
    """One ulp up, in place: ``index`` is a flat position of a contiguous tensor, or an index tuple."""
    if isinstance(index, int):
        assert t.is_contiguous()
        t, index = t.view(-1), (index,)
    t[index] = torch.nextafter(t[index], torch.full_like(t[index], float("inf")))


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. / 6. / 8. populate, reuse, recovery, exports
@pytest.mark.parametrize("name", RENDER_CASES)
@pytest.mark.parametrize("mode", ["fp32", "fp32_per_sample_projection", "f16x3"])
def test_populate_then_reuse(name, mode):
    cfg, comp, inputs = prepare(name, "f16x3" if mode == "f16x3" else "fp32", defer=mode == "fp32")
    K, static, none, reuse = expectations(comp)
    assert 1 <= static < K
    comp.retained = comp.retain_objects()
    assert comp.retained.objects == tuple(range(static))
    want, _ = check(comp, inputs, none, "populate")
    for ty in levels(want):
        for k in range(static, K):
            assert int(want[ty]["_samples"][0]["evaluated"][k]) > 0, (ty, k)     # (the dynamic objects do MLP work every frame)
    assert comp.retained.bytes > 0
    check(comp, inputs, reuse, "reuse")
    check(comp, inputs, reuse, "reuse again")
    comp.retained.invalidate()
    check(comp, inputs, none, "after invalidate")
    check(comp, inputs, reuse, "recovered")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the players move, the static objects are reused
@pytest.mark.parametrize("name", RENDER_CASES)
def test_dynamic_objects_change_and_static_objects_are_reused(name):
    cfg, comp, inputs = prepare(name)
    K, static, none, reuse = expectations(comp)
    comp.retained = comp.retain_objects()
    check(comp, inputs, none, "populate")
    moved = [v.clone() for v in inputs]
    for k in range(static, K):
        moved[3][..., 0, 3, k] += 0.05          # pose
        moved[4][..., k] *= 1.25                # style
        moved[5][..., k] += 0.1                 # deformation
    want, _ = check(comp, moved, reuse, "moved players")
    before = plain(comp, inputs)
    assert not torch.equal(want["coarse"]["global"]["weights"], before["coarse"]["global"]["weights"])
    check(comp, moved, reuse, "moved players again")


# ---------------------------------------------------------------------------------------------------------------------
# 4. staleness, one input at a time
def _object_mutations(comp, k):
    helper = comp.object_id_helper
    model = comp.object_models_coarse[helper.model_idx_by_object_idx(k)]
    mean = [b for n, b in model.named_buffers() if n.endswith("running_mean")][0]

    def bn(_):
        with torch.no_grad():
            mean.view(-1)[0] += 1e-3
    return {"w2o": lambda x: ulp(x[3], (Ellipsis, 0, 3, k)), "style": lambda x: ulp(x[4], (Ellipsis, 0, k)),
            "deformation": lambda x: ulp(x[5], (Ellipsis, 0, k)), "presence": lambda x: x[6][..., k].logical_not_(), "bn_running_mean": bn}


@pytest.mark.parametrize("name,side", [("tennis", SIDE), ("minecraft", SIDE), ("tennis_hierarchical", SIDE), ("tennis", 1)])
def test_every_input_makes_exactly_its_dependants_stale(name, side):
    cfg, comp, inputs = prepare(name, side=side)
    helper = comp.object_id_helper
    K, static, none, reuse = expectations(comp)
    comp.retained = comp.retain_objects()
    check(comp, inputs, none, "populate")
    check(comp, inputs, reuse, "reuse")
    rays = inputs[1].reshape(-1, 3).size(0)
    assert rays == side * side * frames_of(inputs)
    # the camera: one ulp in ONE component of the last ray, of the first ray, of an origin - everything is stale
    for what, change in (("last ray", lambda x: ulp(x[1], 3 * rays - 2)), ("first ray", lambda x: ulp(x[1], 0)),
                         ("origin", lambda x: ulp(x[0], 1))):
        cur = [v.clone() for v in inputs]
        change(cur)
        assert not all(torch.equal(a, b) for a, b in zip(cur, inputs))
        check(comp, cur, none, what)
        check(comp, cur, reuse, what + ", recovered")
        inputs = cur
    # an object's own inputs: only that object (and, for a model's statistics, the objects that share the model) is stale
    for k in range(static):
        for what, change in _object_mutations(comp, k).items():
            cur = [v.clone() for v in inputs]
            change(cur)
            model = helper.model_idx_by_object_idx(k)
            shared = [j for j in range(static) if helper.model_idx_by_object_idx(j) == model] if what == "bn_running_mean" else [k]
            expect = [0 if j in shared else reuse[j] for j in range(K)]
            check(comp, cur, expect, f"object {k}: {what}")
            check(comp, cur, reuse, f"object {k}: {what}, recovered")
            inputs = cur
    # weight values: the device cannot see them, the host epoch moves with the packed copies
    key = comp.retained.host_key
    with torch.no_grad():
        p = [q for n, q in comp.object_models_coarse[helper.model_idx_by_object_idx(0)].named_parameters() if n.endswith("weight")][0]
        p.data.mul_(1.0 + 2.0 ** -10)
    comp.weights_changed()
    check(comp, inputs, none, "weights_changed")
    assert comp.retained.host_key > key
    check(comp, inputs, reuse, "weights_changed, recovered")


def test_weights_that_change_while_detached_are_not_missed():
    """Detach, change the weights, let a plain render re-pack them, re-attach: the next retained call re-packs nothing, and must
    still find every object stale."""
    cfg, comp, inputs = prepare("minecraft")
    helper = comp.object_id_helper
    K, static, none, reuse = expectations(comp)
    r = comp.retain_objects()
    comp.retained = r
    check(comp, inputs, none, "populate")
    check(comp, inputs, reuse, "reuse")
    comp.retained = None
    with torch.no_grad():
        p = [q for n, q in comp.object_models_coarse[helper.model_idx_by_object_idx(0)].named_parameters() if n.endswith("weight")][0]
        p.data.mul_(1.0 + 2.0 ** -8)
    comp.weights_changed()
    changed = render(comp, inputs)                       # plain: packs the new weights
    comp.retained = r
    want, got = check(comp, inputs, none, "re-attached after a weight change")
    assert torch.equal(want["coarse"]["global"]["weights"], changed["coarse"]["global"]["weights"])
    check(comp, inputs, reuse, "re-attached, recovered")
    # the same through another Retained that was attached in between
    comp.retained = comp.retain_objects()
    with torch.no_grad():
        p.mul_(1.0 + 2.0 ** -8)
    check(comp, inputs, none, "the other one populates")
    comp.retained = r
    check(comp, inputs, none, "swapped back after a weight change")
    check(comp, inputs, reuse, "swapped back, recovered")


def test_a_call_split_along_the_rays_renders_without_retention():
    cfg, comp, inputs = prepare("tennis")
    comp.retained = comp.retain_objects()
    comp.max_workspace_bytes = 1 << 20                   # far below what 529 rays need: the call is cut into ray chunks
    with pytest.warns(UserWarning, match="split along the rays"):
        got = render(comp, inputs)
    assert len(got["coarse"]["_samples"]) > 1            # (one export per chunk)
    assert comp.retained.last_reused is None and comp.retained.bytes == 0
    same_entries(plain(comp, inputs), got, "split call")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # (said once)
        same_entries(plain(comp, inputs), render(comp, inputs), "split call again")
    comp.max_workspace_bytes = type(comp).max_workspace_bytes
    K, static, none, reuse = expectations(comp)
    check(comp, inputs, none, "whole call: populate")
    check(comp, inputs, reuse, "whole call: reuse")


# ---------------------------------------------------------------------------------------------------------------------
# 5. occupancy bits are part of an object's key
def test_occupancy_bits_belong_to_the_key():
    cfg, comp, inputs, _ = prepare_full("tennis_hierarchical", sigma="mixed")
    other = composer_inputs(cfg, synthetic.tennis_scene(seed=77), pixels=grid_pixels(256, 256, 16))
    K = comp.object_id_helper.objects_count
    N = frames_of(inputs)
    everything = [1] * K
    comp.retained = comp.retain_objects(range(K))
    comp.occupancy = comp.occupancy_from_mask({key: m.cuda() for key, m in random_masks(cfg, N, cells=(8, 8, 8)).items()})
    check(comp, inputs, [0] * K, "populate with a grid")
    want, _ = check(comp, inputs, everything, "reuse with a grid")
    comp.occupancy.grids[(1, "fine")]["bits"][0, 3] ^= 1 << 7
    check(comp, inputs, [0 if k == 1 else 1 for k in range(K)], "one bit of object 1's fine grid")
    check(comp, inputs, everything, "one bit, recovered")
    # a grid built from the density fields, rewritten in place for other codes
    with torch.no_grad():
        occ = comp.build_occupancy(inputs[4].cuda(), inputs[5].cuda(), resolution=(8, 8, 8), supersample=2, threshold=0.0, dilate=0)
    comp.occupancy = occ
    check(comp, inputs, [0] * K, "another grid: nothing is reused")
    check(comp, inputs, everything, "another grid, reuse")
    before = {key: g["bits"].clone() for key, g in occ.grids.items()}
    with torch.no_grad():
        occ.update(other[4].cuda(), other[5].cuda())
    moved = {k for (k, _level), g in occ.grids.items() if not torch.equal(g["bits"], before[(k, _level)])}
    print("objects whose bits the update changed", sorted(moved))
    assert moved
    check(comp, inputs, [0 if k in moved else 1 for k in range(K)], "Occupancy.update")
    check(comp, inputs, everything, "Occupancy.update, recovered")


# ---------------------------------------------------------------------------------------------------------------------
# 7. recorded frames hold both outcomes
def test_recorded_frame_reuses_and_refreshes():
    from playableenvironments_amd.frame_graph import FrameGraph, SCENE_KEYS
    cfg = configs.reduced_config(configs.minecraft_config(), **SMALL_NETS)
    model = em.EnvironmentModel(cfg)
    synthetic.randomize_module_state(model.object_composer, seed=0, step=20000, alpha_bias=0.0, bender_scale=1e4)
    mixed_sigma(model.object_composer)
    model = model.eval().cuda()
    comp = model.object_composer
    K, static, none, reuse = expectations(comp)
    size = (48, 64)
    scene = {k: v.cuda() for k, v in synthetic.minecraft_scene(seed=5, image_size=size).items() if torch.is_tensor(v)}
    players = {k: v.clone() for k, v in scene.items()}
    players["object_translation_parameters"][..., static:] += 0.05
    players["object_style"][..., static:] *= 1.25
    camera = {k: v.clone() for k, v in scene.items()}
    camera["camera_translations"] += 0.01

    def eager_plain(s):
        kept, comp.retained = comp.retained, None
        try:
            with torch.no_grad():
                out = model(*[s[k] for k in SCENE_KEYS[:3]], size, *[s[k] for k in SCENE_KEYS[3:]], 0, False, mode="scene_encodings")
            torch.cuda.synchronize()
            return {e: {k: v.clone() for k, v in out["coarse"][e].items() if torch.is_tensor(v)} for e in out["coarse"]
                    if isinstance(out["coarse"][e], dict)}
        finally:
            comp.retained = kept

    def same(got, want, what):
        entries = [e for e in want if "weights" in want[e]]
        assert "global" in entries and len(entries) > 1
        for entry in entries:
            for key in ("integrated_features", "opacity", "depth", "weights"):
                assert torch.equal(got["coarse"][entry][key], want[entry][key]), (what, entry, key)

    comp.retained = comp.retain_objects()
    graph = FrameGraph(model, scene, size)
    flags = comp.retained.last_reused               # the recording's own flag tensor, rewritten by every replay
    assert graph.census["memsets"] == 0 and graph.census["kernels"] > 0
    for what, s, expect in (("unchanged", scene, reuse), ("moved players", players, reuse), ("moved camera", camera, none),
                            ("camera stays", camera, reuse), ("back", scene, none), ("back, again", scene, reuse)):
        got = graph.render(s)
        torch.cuda.synchronize()
        assert flags.tolist() == expect, (what, flags.tolist())
        same(got, eager_plain(s), what)
    # setting, swapping or clearing the retained set never replays the stale recording
    first = comp.retained
    comp.retained = None
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scene)
    comp.retained = comp.retain_objects()
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scene)
    comp.retained = first
    graph.render(scene)
    first.clear()
    with pytest.raises(RuntimeError, match="build a new FrameGraph"):
        graph.render(scene)
    torch.cuda.synchronize()
