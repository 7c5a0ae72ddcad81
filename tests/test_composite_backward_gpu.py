"""Compositing backward on surface-like densities on an MI355X ("Compositing backward in the density
regimes"): the per-sample gradients k_composite_bwd wrote - d loss / d sigma, d t, d |delta|, d feature row per object, d |d| per
level, exported right behind its launch (pr_sample_grads_t) - against float64 autograd of the oracle's functions of that stage
(helpers.replay_gradients), fed the kernel's OWN inputs of the stage: the depths, densities, slots and displacements the forward
pass exported and the feature rows the backward kernel read.  Position by position at 1e-4 |want| + 1e-5 max |want| plus the
derived cancellation term (helpers.gradient_mismatch), which the fp32 oracle and a sequential fp32 restatement of the kernel's
arithmetic are shown to need on the CPU alone (tests/test_composite_backward_cpu.py); the kernel never chose a constant.

Final parameter gradients are NOT compared in these regimes (the fp32 oracle's own are more than its tensors' peaks away from
float64: DESIGN.md): they are asserted finite.

Cases x regimes x {eval, perturb} x {fp32, f16x3}, the cases' own rays (256 / 64 / 144): one differentiable HIP call plus
backward() per combination, shared by its tests; five single combinations reach the paths the main probe does not.

Measured on an MI355X, worst ratio to the tolerance per tensor: d sigma 0.59 (tennis_64_128 / sparse / perturb, where the fp32
oracle needs 0.54), d t 0.047, feature rows 0.051, d |delta| 0.051, d |d| 0.061."""
import functools

import pytest
import torch

from tests import helpers as H
from tests.helpers import DENSITY_CASES, DENSITY_REGIMES, GRADIENT_FIELDS
from tests.test_density_regimes_gpu import oracle_side

pytestmark = pytest.mark.gpu
REGIMES = list(DENSITY_REGIMES)
LEVELS = ("coarse", "fine")
MAX_RAYS = {"tennis_16_32": 256, "tennis_64_128": 128, "minecraft_hierarchical": 256}
combos = lambda f: pytest.mark.parametrize("name", DENSITY_CASES)(pytest.mark.parametrize("regime", REGIMES)(
    pytest.mark.parametrize("perturb", [False, True], ids=["eval", "perturb"])(pytest.mark.parametrize("precision", ["fp32", "f16x3"])(f))))

#: variant: (fields the loss reads, entries it reads - None: all -, apply_activation, objects taken out of the scene)
VARIANTS = {
    "main": (GRADIENT_FIELDS, None, False, ()),
    # no integrated_features and no weights probe: entry_backward's has_gf == false path and the NULL gW
    "scalars_only": (("opacity", "depth", "integrated_displacements_magnitude"), None, False, ()),
    # the loss reads one object's entry: the uniform early return is taken for every other entry, the global one included
    "one_entry": (GRADIENT_FIELDS, ("object_2",), False, ()),
    # the sigmoid path's scalar feature loop (samples without a row carry sigmoid(0))
    "sigmoid": (GRADIENT_FIELDS, None, True, ()),
    # the loss reads the global entry only: whatever a masked static sample receives comes from the merged list
    "global_only": (GRADIENT_FIELDS, ("global",), False, ()),
    # an object that is not in the scene
    "absent": (GRADIENT_FIELDS, None, False, (3,)),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


def _cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_cpu(v) for v in x]
    return x


@functools.lru_cache(maxsize=None)
def hip_side(name, regime, perturb, precision, variant="main"):
    """One differentiable HIP call (eval mode: frozen BatchNorm statistics; recorded noise replayed; ``_export=True``) and its
    backward(): the forward exports, the exported per-sample gradients, the probes, and whether every gradient of the call is
    finite - all on the CPU."""
    fields, entries, sigmoid, absent = VARIANTS[variant]
    side = oracle_side(name, regime, perturb)
    cfg, comp, inputs, _ = H.density_case(name, regime, precision)
    flat = side["flat"]
    assert flat["d"].size(0) * flat["R"] <= MAX_RAYS[name]
    if sigmoid:
        comp.apply_activation = cfg["model"]["apply_activation"] = True
    comp = comp.cuda()
    comp._export_sample_grads = True
    gin = [v.cuda() for v in inputs]
    if absent:
        gin[6] = gin[6].clone()
        gin[6][..., list(absent)] = False
    for i in (3, 4, 5):
        gin[i] = gin[i].clone().requires_grad_(True)
    with torch.enable_grad():
        out = comp(*gin, perturb, _noise=side["noise"], _export=True)
        exports = {level: out[level]["_samples"][0] for level in LEVELS}
        assert all(len(out[level]["_samples"]) == 1 for level in LEVELS)
        probes = {level: H.stage_probes(cfg, flat, [t.size(-1) for t in exports[level]["t"]], seed=11 + i, fields=fields, entries=entries)
                  for i, level in enumerate(LEVELS)}
        loss = 0.0
        for level in LEVELS:
            for entry, per_field in probes[level].items():
                for field, probe in per_field.items():
                    value = out[level][entry][field]
                    loss = loss + (value * probe.cuda().reshape(value.shape)).sum()
        loss.backward()
    torch.cuda.synchronize()
    params = {k: v.grad for k, v in comp.named_parameters() if v.grad is not None}
    assert params
    finite = {k: bool(torch.isfinite(g).all()) for k, g in params.items()}
    finite.update({f"input {i}": bool(torch.isfinite(gin[i].grad).all()) for i in (3, 4, 5)})
    in_scene = flat["in_scene"].clone()
    in_scene[:, list(absent)] = False
    return dict(cfg=cfg, exports=_cpu({level: {k: exports[level][k] for k in ("t", "sigma", "slot", "delta")} for level in LEVELS}),
                grads=_cpu(comp.last_sample_grads), probes=probes, finite=finite, in_scene=in_scene)


def _report(what, rep):
    print(what, {k: f"{v[0]:.3g}" for k, v in rep.items()})
    bad = {k: v[0] for k, v in rep.items() if not v[1]}
    assert not bad, (what, bad)


def _check(name, regime, perturb, precision, variant="main"):
    """The comparison of one combination: per level and object the five exported tensors against the float64 replay."""
    side, got = oracle_side(name, regime, perturb), hip_side(name, regime, perturb, precision, variant)
    K = side["flat"]["K"]
    worst = {}
    for level in LEVELS:
        ex, grads = got["exports"][level], got["grads"][level]
        lists = [(ex["t"][k], ex["sigma"][k], ex["delta"][k]) for k in range(K)]
        bender = [grads["displacement_magnitude"][k] is not None for k in range(K)]
        for k in range(K):
            assert torch.equal(grads["feature_rows"][k] != 0, (grads["feature_rows"][k] != 0) & (ex["slot"][k] >= 0).unsqueeze(-1))
            assert not grads["features"][k][ex["slot"][k] < 0].any(), (level, k, "feature gradients of samples without a row")
        args = (got["cfg"], level, lists, ex["slot"], grads["feature_rows"], side["flat"]["d"], side["noise"], got["probes"][level])
        with H.oracle_in_float64():
            want = H.replay_gradients(*args)
        rep = H.compare_gradients(want, grads, bender, H.gradient_magnitudes(*args))
        _report(f"{variant} {level}", rep)
        for key, value in rep.items():
            tensor = key.split("/")[0]
            worst[tensor] = max(worst.get(tensor, 0.0), value[0])
        # ---- exact zeros
        for k in range(K):
            if not perturb:
                assert not grads["sigma"][k][ex["sigma"][k] <= 0].any(), (level, k, "d sigma where sigma <= 0")
            if not bool(got["in_scene"][:, k].all()):
                gone = ~got["in_scene"][:, k]
                for tensor in H.GRADIENT_TENSORS:
                    if grads[tensor][k] is not None:
                        assert not grads[tensor][k][gone].any(), (level, k, tensor, "an object that is not in the scene")
        if variant == "global_only":
            masked = want["masked"]
            assert sum(int(m.sum()) for m in masked) >= 1
            for k, m in enumerate(masked):
                for tensor in H.GRADIENT_TENSORS:
                    if grads[tensor][k] is not None:
                        assert not grads[tensor][k][m].any(), (level, k, tensor, "a masked static sample")
    print(f"{name} {regime} {'perturb' if perturb else 'eval'} {precision} {variant}: worst ratio per tensor",
          {k: f"{v:.3f}" for k, v in worst.items()})
    assert not [k for k, ok in got["finite"].items() if not ok], "a gradient of the call is not finite"


@combos
def test_sample_gradients(name, regime, perturb, precision):
    """sigma, t, |delta|, feature rows and |d|, position by position; every exported value finite (a non-finite value fails its
    tensor); unperturbed: d sigma exactly zero where the exported sigma is <= 0; every parameter, style, deformation and w2o gradient
    of the call finite."""
    _check(name, regime, perturb, precision)


@pytest.mark.parametrize("variant", ["scalars_only", "one_entry", "sigmoid", "absent"])
def test_other_paths(variant):
    """tennis_16_32 / surfaces / eval / fp32 through the paths the main probe does not reach (VARIANTS); the gradients of an object
    that is not in the scene are exactly zero."""
    _check("tennis_16_32", "surfaces", False, "fp32", variant)


def test_masked_static_samples_receive_nothing_from_the_merged_list():
    """minecraft_hierarchical / surfaces / eval / fp32 with a loss that reads the global entry only: the exported gradients of the
    static samples the overlap fix masked are exactly zero.  (With the main probe a masked sample carries the gradient of its own
    object's entry, which is integrated before the overlap fix: that sum is compared position by position in the main test.)"""
    _check("minecraft_hierarchical", "surfaces", False, "fp32", "global_only")
