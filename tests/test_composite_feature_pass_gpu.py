"""The feature pass of k_composite<4> in deferred calls (one object per wave, 16-byte row loads) and k_project_features behind it,
on an MI355X: every output tensor against a fixture RECORDED FROM THE PARENT COMMIT's library (tests/golden/composite_feature_pass/
*.npz, bit for bit - the pass and the projection were reordered for latency, never for arithmetic), and - so that the fixture is not
the only witness - ``integrated_features`` against the float64 replay of tests/helpers (replay_features / expected_features) with the
project's tolerance.

All cases are coarse-only fp32 evaluation calls with the deferred projection on and 256 or more entries per ray (k_composite<4>).
The part of an object with P positions is round_up(ceil(P / 4), 64) entries:
  P = 64   one part                      P = 65   a second part with one entry
  P = 192  three parts, no fourth        P = 320  parts of 128, 128, 64
Object counts 1, 3, 4, 5: waves without an object, one object per wave, a wave with two.  R = 65 rays (two projection tiles, the
second with one ray) or R = 1.  Two further calls keep the shared pass (not deferred): f16x3, and a perturbed training-mode call.

A change that deliberately moves the MLP's bits regenerates the fixture by the recipe each file records:
    python -m tests.test_composite_feature_pass_gpu <commit the library was built from>"""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import render_oracle as ro
from playableenvironments_amd import ObjectComposer, configs, synthetic
from tests import helpers as H
from tests.helpers import REPLAY_ATOL, REPLAY_RTOL

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_feature_pass")
SHIPPED_WIDTH = dict(width=256, layers=4, skip=2, features=192, octaves=4)      # rows of 128 + 1 -> 132 floats: 33 lanes of 16 bytes
ROWS_IN_FLIGHT = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


def _tennis(objects, positions, seed, **nets):
    """Tennis with ``objects`` object instances: 3 drops player_2 (model and instance), 5 gives the player_2 model a second
    instance two metres beside the first.  ``positions``: coarse positions per MODEL name."""
    cfg = configs.reduced_config(configs.tennis_config(), positions={k: (v, v) for k, v in positions.items()}, **nets)
    scene = synthetic.tennis_scene(seed=seed)
    m = cfg["model"]
    per_object = ("object_rotation_parameters", "object_translation_parameters", "object_style", "object_deformation", "object_in_scene")
    if objects == 3:
        for key in ("object_models", "object_parameters_encoder", "object_encoders", "sampling_weights"):
            m[key] = m[key][:3]
        for key in per_object:
            scene[key] = scene[key][..., :3].contiguous()
    elif objects == 5:
        m["object_parameters_encoder"][3]["objects_count"] = 2
        m["sampling_weights"] = [0.4, 0.15, 0.15, 0.15, 0.15]
        for key in per_object:
            scene[key] = torch.cat([scene[key], scene[key][..., 3:]], dim=-1)
        scene["object_translation_parameters"][..., 0, 4] += 2.0
        scene["object_style"][..., 4] = scene["object_style"][..., 4].flip(-1)
    else:
        assert objects == 4
    return cfg, scene


def _single(positions, seed):
    return configs.reduced_config(configs.tennis_single_player_config(positions=positions)), synthetic.single_player_scene(seed=seed)


def _pixels(scene, rays):
    """``rays`` pixels spread over a 16 x 16 grid of the image (1: a pixel of the lower half, where the court is)."""
    rows, cols = H.grid_pixels(scene["image_size"][0], scene["image_size"][1], 16)
    pick = torch.linspace(0, rows.numel() - 1, rays).long() if rays > 1 else torch.tensor([rows.numel() * 5 // 8 + 7])
    return rows[pick], cols[pick]


# name: (config and scene, rays, density regime of helpers.DENSITY_REGIMES, decoder layout or None)
CASES = {
    "one_object_320": (lambda: _single(320, seed=3), 65, "surfaces", None),
    "three_objects_192_65_64": (lambda: _tennis(3, dict(background=192, background_backplate=65, player_1=64), seed=5), 65, "surfaces", None),
    "four_objects_shipped_width": (lambda: _tennis(4, dict(background=64, background_backplate=64, player_1=64, player_2=64), seed=7,
                                                   **SHIPPED_WIDTH), 65, "sparse", None),
    "five_objects_one_ray": (lambda: _tennis(5, dict(background=192, background_backplate=65, player_1=64, player_2=64), seed=9), 1,
                             "surfaces", None),
    "five_objects_320": (lambda: _tennis(5, dict(background=320, background_backplate=65, player_1=192, player_2=64), seed=11), 65,
                         "solid", None),
    "four_objects_decoder": (lambda: _tennis(4, dict(background=192, background_backplate=64, player_1=65, player_2=64), seed=13), 65,
                             "surfaces", dict(rays=[60, 5], width=[12, 5], channels=[10, 6])),
}
# the shared (not deferred) pass: name: (case whose scene it renders, precision, training mode and perturbed)
UNTOUCHED = {
    "f16x3": ("three_objects_192_65_64", "f16x3", False),
    "train_perturb": ("three_objects_192_65_64", "fp32", True),
}


@functools.lru_cache(maxsize=None)
def case_side(name):
    """(cfg, composer on the CPU with shaped densities, composer inputs, state dict) of one case - shared, read only."""
    make, rays, regime, _ = CASES[name]
    cfg, scene = make()
    torch.manual_seed(0)
    comp = ObjectComposer(cfg)
    synthetic.randomize_module_state(comp, seed=0, step=20000, alpha_bias=2.0, bender_scale=1e4)
    comp.eval()
    inputs = H.composer_inputs(cfg, scene, pixels=_pixels(scene, rays))
    scale, quantile = H.DENSITY_REGIMES[regime]
    H.shape_sigma(comp, scale, quantile, cfg, inputs)
    sd = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
    return cfg, comp, inputs, sd


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_to_cpu(v) for v in x]
    return x


@functools.lru_cache(maxsize=None)
def render(name):
    """The HIP call of a case (deferred projection on, exports), on the CPU."""
    cfg, comp, inputs, _ = case_side(name)
    comp = copy.deepcopy(comp).cuda()
    comp.defer_feature_projection = True
    with torch.no_grad():
        out = comp(*[v.cuda() for v in inputs], False, _export=True, _decoder_layout=CASES[name][3])
    torch.cuda.synchronize()
    return _to_cpu(out)


@functools.lru_cache(maxsize=None)
def render_untouched(name):
    base, precision, training = UNTOUCHED[name]
    cfg, comp, inputs, sd = case_side(base)
    comp = copy.deepcopy(comp)
    comp.precision = precision
    rec = {}
    if training:
        with torch.no_grad():
            torch.manual_seed(123)
            ro.composer_forward(cfg, sd, *inputs, True, record_noise=rec, stable_merge=True)
        comp.train()
    comp = comp.cuda()
    with torch.no_grad():
        out = comp(*[v.cuda() for v in inputs], training, _noise=rec if training else None)
    torch.cuda.synchronize()
    return _to_cpu(out)


def _fields(result, prefix=""):
    for k, v in result.items():
        if k in ("pytorch_hook", "extra_outputs") or k.startswith("_"):
            continue
        if isinstance(v, dict):
            yield from _fields(v, prefix + k + ".")
        elif torch.is_tensor(v):
            yield prefix + k, v
        elif isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                yield f"{prefix}{k}.{i}", t


def _assert_equals_fixture(name, result):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        want = {k: torch.from_numpy(z[k]) for k in z.files if k != "recipe"}
    got = dict(_fields(result))
    assert set(got) == set(want) and any(k.endswith("integrated_features") for k in got), sorted(set(got) ^ set(want))
    same = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    moved = {k: float(torch.nan_to_num(got[k].double() - want[k].double()).abs().max()) for k in got
             if got[k].shape != want[k].shape or not same(got[k], want[k])}
    assert not moved, (name, moved)


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_equals_the_parent_build(name):
    """integrated_features of every object and of the global entry (and the decoder maps), weights, depth, opacity, disparity and the
    magnitudes: torch.equal with what the parent commit's library rendered."""
    _assert_equals_fixture(name, render(name))


@pytest.mark.parametrize("name", list(UNTOUCHED))
def test_the_shared_pass_is_untouched(name):
    _assert_equals_fixture("untouched_" + name, render_untouched(name))


@pytest.mark.parametrize("name", list(CASES))
def test_features_match_the_float64_replay(name):
    """sum_i w_i f_i with the oracle's float64 ``object_model_forward`` at the kernels' own sample positions and the call's own
    per-object and global weights (tests/test_density_regimes_gpu.py::test_features): RTOL, and ATOL times the field's peak."""
    cfg, _, inputs, sd = case_side(name)
    got = render(name)
    flat = H.flat_composer_inputs(inputs)
    K, R = flat["K"], flat["R"]
    fold = lambda v, tail=1: v.reshape([-1, R] + list(v.shape[v.dim() - tail:]))
    assert len(got["coarse"]["_samples"]) == 1
    ex = got["coarse"]["_samples"][0]
    with H.oracle_in_float64():
        sd64 = H.to_double(sd)
        feats = []
        for k in range(K):
            f, inside = H.replay_features(cfg, sd64, flat, k, "coarse", ex["t"][k], ex["slot"][k])
            assert torch.equal(inside, ex["slot"][k] >= 0), (k, "in-box decisions")
            feats.append(f)
        lists = [(ex["t"][k], ex["sigma"][k], ex["delta"][k]) for k in range(K)]
        replay = H.replay_composition(cfg, lists, flat["d"], None)
        weights = [fold(got["coarse"][f"object_{k}"]["weights"]) for k in range(K)]
        per_object, total = H.expected_features(feats, weights, fold(got["coarse"]["global"]["weights"]), replay["order"])
    rep = {}
    for entry, want in [(f"object_{k}", per_object[k]) for k in range(K)] + [("global", total)]:
        peak = float(want.abs().max())
        rep[entry] = H.field_mismatch(want, fold(got["coarse"][entry]["integrated_features"]), REPLAY_RTOL, REPLAY_ATOL * max(peak, 1e-30))
    print(name, {k: f"{v[0]:.3g}" for k, v in rep.items()})
    bad = {k: v[0] for k, v in rep.items() if not v[1]}
    assert not bad, (name, bad)
    layout = CASES[name][3]
    if layout is not None:      # the decoder maps are the channels-first fold of the same call's global features, bit for bit
        g = fold(got["coarse"]["global"]["integrated_features"])
        r0 = c0 = 0
        for m, rays, width, channels in zip(got["coarse"]["global"]["decoder_features"], layout["rays"], layout["width"], layout["channels"]):
            want = g[:, r0:r0 + rays, c0:c0 + channels].reshape(-1, rays // width, width, channels).movedim(-1, -3)
            assert torch.equal(m.reshape(want.shape), want), (r0, c0)
            r0, c0 = r0 + rays, c0 + channels


def _part_rows(name):
    """Contributing rows (inside the box, a non-zero own or global weight) per (object, ray, part) of a case."""
    got = render(name)
    ex = got["coarse"]["_samples"][0]
    K = len(ex["slot"])
    order = None
    out = []
    begin = 0
    gw = got["coarse"]["global"]["weights"]
    gw = gw.reshape(-1, gw.shape[-1])
    for k in range(K):
        slot = ex["slot"][k].reshape(-1, ex["slot"][k].shape[-1])
        P = slot.shape[-1]
        wo = got["coarse"][f"object_{k}"]["weights"].reshape(-1, P)
        if order is None:
            # global weights per concatenation index: undo the merge with the depths (stable in object order)
            t = torch.cat([e.reshape(-1, e.shape[-1]) for e in ex["t"]], dim=-1)
            order = torch.sort(t, dim=-1, stable=True).indices
            by_entry = torch.zeros_like(gw).scatter_(-1, order, gw)
        wg = by_entry[:, begin:begin + P]
        take = (slot >= 0) & ((wo != 0) | (wg != 0))
        part = ((P + 3) // 4 + 63) // 64 * 64
        out.append([take[:, b:b + part].sum(-1) for b in range(0, P, part)])
        begin += P
    return out


def test_cases_reach_what_they_are_for():
    """Over the cases: an object without a contributing row on a ray where another object has one, an empty part behind a non-empty
    one, parts whose row count runs the batched loop, its tail, or the tail alone; and the part counts the docstring names."""
    rows = {name: _part_rows(name) for name in CASES}
    assert [len(p) for p in rows["three_objects_192_65_64"]] == [3, 2, 1]
    assert [len(p) for p in rows["one_object_320"]] == [3] and [len(p) for p in rows["five_objects_320"]] == [3, 2, 3, 1, 1]
    absent = empty_part = batched = tail = tail_only = 0
    for name, objects in rows.items():
        per_object = torch.stack([torch.stack(parts).sum(0) for parts in objects])          # (K, rays)
        absent += int(((per_object == 0) & (per_object.sum(0, keepdim=True) > 0)).sum())
        for parts in objects:
            counts = torch.stack(parts)
            empty_part += int(((counts[1:] == 0) & (counts[:-1] > 0)).sum())
            batched += int((counts >= ROWS_IN_FLIGHT).sum())
            tail += int(((counts >= ROWS_IN_FLIGHT) & (counts % ROWS_IN_FLIGHT != 0)).sum())
            tail_only += int(((counts > 0) & (counts < ROWS_IN_FLIGHT)).sum())
    print(dict(absent=absent, empty_part=empty_part, batched=batched, tail=tail, tail_only=tail_only))
    assert min(absent, empty_part, batched, tail, tail_only) >= 1


def record(commit):
    """Writes the fixture from the library that is built now (module docstring)."""
    from playableenvironments_amd import _lib
    _lib.load()
    os.makedirs(GOLDEN, exist_ok=True)
    recipe = (f"rendered on an MI355X by the library built from commit {commit} (make -C playableenvironments_amd/csrc): "
              f"python -m tests.test_composite_feature_pass_gpu {commit}")
    results = {name: render(name) for name in CASES}
    results.update({"untouched_" + name: render_untouched(name) for name in UNTOUCHED})
    for name, result in results.items():
        arrays = {k: v.numpy() for k, v in _fields(result)}
        assert "recipe" not in arrays, name
        np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), recipe=np.array(recipe), **arrays)
        print(name, len(arrays), "fields", os.path.getsize(os.path.join(GOLDEN, name + ".npz")), "bytes")


if __name__ == "__main__":
    record(sys.argv[1])
