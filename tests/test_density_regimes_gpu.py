"""Surface-like densities on an MI355X ("Density regimes and stage replays"): everything behind the MLP - the
alphas and the transmittance scan, k_resample's cdf / inverse CDF / merge, k_composite's per-object and cross-object weights with the
overlap fix, the compaction of contributing samples and k_project_features - stage by stage against the oracle's function for that
stage in float64, fed the kernels' OWN exported inputs of the stage (``_export=True``: t, sigma, slot, delta per object and level).
That factors out the MLP's round-off and the legitimate sensitivity of an earlier stage, so every stage keeps the project's tolerance
(RTOL 1e-4 / ATOL 1e-5) where a whole-pipeline comparison cannot: the bound of a resampled depth and its either-branch rules are
derived in tests/helpers.replay_resampling and measured on the CPU alone (tests/test_density_regimes_cpu.py).

Cases x regimes x {eval, perturb} x {fp32, f16x3}: one HIP call per switch setting, shared by the tests of the combination."""
import functools

import pytest
import torch

from oracle import render_oracle as ro
from tests import helpers as H
from tests.helpers import DENSITY_CASES, DENSITY_REGIMES, INTEGRATED_FIELDS, REPLAY_ATOL, REPLAY_RTOL

pytestmark = pytest.mark.gpu
REGIMES = list(DENSITY_REGIMES)
LEVELS = ("coarse", "fine")
combos = lambda f: pytest.mark.parametrize("name", DENSITY_CASES)(pytest.mark.parametrize("regime", REGIMES)(
    pytest.mark.parametrize("perturb", [False, True], ids=["eval", "perturb"])(pytest.mark.parametrize("precision", ["fp32", "f16x3"])(f))))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_library):
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a GPU: the renderer has no CPU fallback")


@functools.lru_cache(maxsize=None)
def oracle_side(name, regime, perturb):
    """The fp32 and the float64 oracle of the whole pipeline and the recorded draws (CPU; shared by both precisions, read only)."""
    cfg, _, inputs, sd = H.density_case(name, regime)
    rec = {}
    with torch.no_grad():
        torch.manual_seed(123)
        want = ro.composer_forward(cfg, sd, *inputs, perturb, record_noise=rec, stable_merge=True)
        with H.oracle_in_float64():
            exact = ro.composer_forward(cfg, H.to_double(sd), *H.to_double(list(inputs)), perturb, noise=H.to_double(rec),
                                        update_stats=False, stable_merge=True)
            sd64 = H.to_double(sd)
    return dict(cfg=cfg, inputs=inputs, sd64=sd64, noise=rec if perturb else None, want=want, exact=exact,
                flat=H.flat_composer_inputs(inputs))


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_to_cpu(v) for v in x]
    return x


@functools.lru_cache(maxsize=None)
def hip_side(name, regime, perturb, precision):
    """{(defer_feature_projection, gate_feature_head): the HIP call's results and exports, on the CPU}: both settings of the deferred
    projection, and for unperturbed calls both settings of the sigma gate (a perturbed call ignores it)."""
    side = oracle_side(name, regime, perturb)
    _, comp, inputs, _ = H.density_case(name, regime, precision)
    comp = comp.cuda()
    gin = [v.cuda() for v in inputs]
    out = {}
    with torch.no_grad():
        for defer in (True, False):
            for gate in (True, False) if not perturb else (True,):
                comp.defer_feature_projection, comp.gate_feature_head = defer, gate
                out[defer, gate] = _to_cpu(comp(*gin, perturb, _noise=side["noise"], _export=True))
    torch.cuda.synchronize()
    return out


def _exports(result, level):
    assert len(result[level]["_samples"]) == 1            # (one launch: the call was not split along the rays)
    return result[level]["_samples"][0]


def _noise(side, key):
    return None if side["noise"] is None else side["noise"][key]


def _fold(side, v, tail=1):
    return v.reshape([-1, side["flat"]["R"]] + list(v.shape[v.dim() - tail:]))


def _entry(side, result, level, entry):
    e = result[level][entry]
    return {f: _fold(side, e[f], 1 if f == "weights" else 0) for f in ("weights",) + INTEGRATED_FIELDS}


def _lists(result, level, K):
    ex = _exports(result, level)
    return [(ex["t"][k], ex["sigma"][k], ex["delta"][k]) for k in range(K)]


def _report(what, rep):
    print(what, {k: f"{v[0]:.3g}" for k, v in rep.items()})
    bad = {k: v[0] for k, v in rep.items() if not v[1]}
    assert not bad, (what, bad)


@combos
def test_resampling(name, regime, perturb, precision):
    """The exported fine depths against replay_resampling of the exported coarse depths and densities: position by position within the
    derived bound (helpers.compare_resampling), sorted, every coarse depth in the list bit for bit.  perturb=True is k_resample's
    bitonic fallback, perturb=False its rank merge."""
    side, got = oracle_side(name, regime, perturb), hip_side(name, regime, perturb, precision)[True, True]
    coarse, fine = _exports(got, "coarse"), _exports(got, "fine")
    for k in range(side["flat"]["K"]):
        _, d = H.object_frame_rays(side["flat"], k)
        with H.oracle_in_float64():
            _, info = H.replay_resampling(side["cfg"], k, coarse["t"][k], coarse["sigma"][k], d, side["flat"]["in_scene"][:, k], side["noise"])
        rep = H.compare_resampling(coarse["t"][k], info, fine["t"][k])
        print(f"object {k}: worst {rep['worst']:.3f} of its interval, {rep['alternatives']} alternative candidates, "
              f"{int(info['either'].sum())} either depths of {info['either'].numel()}")
        assert rep["ok"], (k, rep)


@combos
def test_object_integration(name, regime, perturb, precision):
    """Every object's weights (sample for sample), opacity, depth, disparity and displacement magnitude at both levels against
    replay_integration of the exported list, RTOL / ATOL, NaNs in the same places, and the transmittance floor
    (helpers.compare_integration).  No field needed arbitration."""
    side, got = oracle_side(name, regime, perturb), hip_side(name, regime, perturb, precision)[True, True]
    K = side["flat"]["K"]
    for level in LEVELS:
        for k, (t, sigma, delta) in enumerate(_lists(got, level, K)):
            with H.oracle_in_float64():
                replay = H.replay_integration(t, sigma, delta, side["flat"]["d"], _noise(side, f"int_{level}_{k}"))
            _report(f"{level} object {k}", H.compare_integration(replay, _entry(side, got, level, f"object_{k}")))


@combos
def test_composition(name, regime, perturb, precision):
    """The global weights in merged order (position by position) and the scalar fields at both levels against replay_composition
    (overlap fix + stable merge + integrate) of the exported lists; sum(weights) = opacity; 0 <= weights <= 1."""
    side, got = oracle_side(name, regime, perturb), hip_side(name, regime, perturb, precision)[True, True]
    K = side["flat"]["K"]
    for level in LEVELS:
        with H.oracle_in_float64():
            replay = H.replay_composition(side["cfg"], _lists(got, level, K), side["flat"]["d"], _noise(side, f"int_{level}_global"))
        entry = _entry(side, got, level, "global")
        rep = H.compare_integration(replay, entry)
        rep["sum(weights) = opacity"] = H.field_mismatch(entry["weights"].double().sum(-1), entry["opacity"])
        _report(f"{level} global", rep)
        if name == "minecraft_hierarchical":
            assert sum(int(m.sum()) for m in replay["masked"]) >= 1, "the overlap fix masks nothing on the exported lists"


@combos
def test_features(name, regime, perturb, precision):
    """integrated_features of every object and of the global list, for both settings of the deferred projection (and of the sigma gate,
    unperturbed), against sum_i w_i f_i with the oracle's float64 ``object_model_forward`` at the kernels' own sample positions and
    the call's own per-object and global weights.  RTOL, and ATOL times the field's peak."""
    side, runs = oracle_side(name, regime, perturb), hip_side(name, regime, perturb, precision)
    K, main = side["flat"]["K"], runs[True, True]
    for level in LEVELS:
        ex = _exports(main, level)
        feats = []
        with H.oracle_in_float64():
            for k in range(K):
                f, inside = H.replay_features(side["cfg"], side["sd64"], side["flat"], k, level, ex["t"][k], torch.zeros_like(ex["slot"][k]))
                assert torch.equal(inside, ex["slot"][k] >= 0), (level, k, "in-box decisions")
                feats.append(f)
            for switches, got in runs.items():
                own = _exports(got, level)
                assert all(torch.equal(own["t"][k], ex["t"][k]) and torch.equal(own["slot"][k] >= 0, ex["slot"][k] >= 0) for k in range(K))
                masked = [f * (own["slot"][k] >= 0).unsqueeze(-1) for k, f in enumerate(feats)]
                replay = H.replay_composition(side["cfg"], _lists(got, level, K), side["flat"]["d"], _noise(side, f"int_{level}_global"))
                weights = [_fold(side, got[level][f"object_{k}"]["weights"]) for k in range(K)]
                per_object, total = H.expected_features(masked, weights, _fold(side, got[level]["global"]["weights"]), replay["order"])
                rep = {}
                for entry, want in [(f"object_{k}", per_object[k]) for k in range(K)] + [("global", total)]:
                    peak = float(want.abs().max())
                    rep[entry] = H.field_mismatch(want, _fold(side, got[level][entry]["integrated_features"]), REPLAY_RTOL, REPLAY_ATOL * peak)
                _report(f"{level} defer={switches[0]} gate={switches[1]}", rep)


WHOLE_FIELDS = INTEGRATED_FIELDS + ("integrated_features",)


def _coarse_fields(result):
    return {"coarse": {e: {f: v for f, v in fields.items() if f in WHOLE_FIELDS} for e, fields in result["coarse"].items()
                       if not e.startswith("_")}}


@functools.lru_cache(maxsize=None)
def fp32_realisations(name, regime, perturb, ulps):
    """The fp32 oracle, and three more fp32 evaluations of the reference whose weights and biases are ``ulps`` fp32 ulp away (random
    signs): what an fp32 evaluation of these networks is known to - the project's yardstick for ill-conditioned comparisons
    ("perturbing the ORACLE's weights by one ulp moves its own ...")."""
    side = oracle_side(name, regime, perturb)
    cfg, _, inputs, sd = H.density_case(name, regime)
    out = [_coarse_fields(side["want"])]
    for seed in range(3):
        g = torch.Generator().manual_seed(seed)
        moved = {k: v * (1 + (torch.randint(0, 2, v.shape, generator=g) * 2 - 1).to(v.dtype) * (ulps * H.FP32_EPS))
                 if v.is_floating_point() and k.endswith((".weight", ".bias")) else v for k, v in sd.items()}
        with torch.no_grad():
            out.append(_coarse_fields(ro.composer_forward(cfg, moved, *inputs, perturb, noise=side["noise"], update_stats=False,
                                                          stable_merge=True)))
    return out


@combos
def test_whole_pipeline_sanity(name, regime, perturb, precision):
    """End to end against ``composer_forward``, coarse-level integrated fields only (nothing upstream of them is ill-conditioned except
    the MLP's own density at this scale), by the rule of tests/test_gpu.py::assert_no_farther_than_the_oracle with float64 arbitration:
    |HIP - fp64| <= 4 x |fp32 oracle - fp64| + 1e-6 max |fp64|.  This only guards against gross errors - a wrong input of the chain,
    which the stage replays, fed the chain's own inputs, cannot see.

    The fp32 side of that rule is the farthest of four fp32 evaluations of the reference, the oracle and three with weights one ulp
    away (two for f16x3, whose fp16 operand pairs hold 22 bits): the sigma head times 3e4 turns the round-off of ONE evaluation into
    a max-norm error that is luck - the fp32 oracle's own |error| of minecraft / solid / perturb ``object_0.depth`` is 6.9e-5 on one
    CPU and 4.5e-6 on another (torch's summation order follows the vector width), the three neighbours give 1e-5 .. 9e-5; the kernels
    measured 5.4e-5 (fp32) and 3.3e-5 (f16x3) there."""
    side, got = oracle_side(name, regime, perturb), _coarse_fields(hip_side(name, regime, perturb, precision)[True, True])
    exact = _coarse_fields(side["exact"])
    reps = [H.arbitrate(exact, want, got, factor=4.0) for want in fp32_realisations(name, regime, perturb, 1 if precision == "fp32" else 2)]
    assert reps[0] and all(k.endswith(WHOLE_FIELDS) for k in reps[0])
    print({k: f"HIP {reps[0][k][0]:.3g} fp32 {max(r[k][1] for r in reps):.3g}" for k in reps[0]})
    bad = {k: f"HIP {reps[0][k][0]:.3e} vs fp32 {max(r[k][1] for r in reps):.3e}" for k in reps[0] if not any(r[k][2] for r in reps)}
    assert not bad, bad


@pytest.mark.parametrize("name", DENSITY_CASES)
def test_exports_reach_what_the_regimes_are_for(name):
    """The reach conditions of tests/test_density_regimes_cpu.py on what the KERNELS exported (fp32, eval and perturbed calls, the
    three regimes together)."""
    rays = saturated = empty = depths = either = threshold = fallback = ties = 0
    for regime in REGIMES:
        for perturb in (False, True):
            side, got = oracle_side(name, regime, perturb), hip_side(name, regime, perturb, "fp32")[True, True]
            K, coarse = side["flat"]["K"], _exports(got, "coarse")
            any_saturated = any_empty = None
            for k in range(K):
                _, d = H.object_frame_rays(side["flat"], k)
                args = (side["cfg"], k, coarse["t"][k], coarse["sigma"][k], d, side["flat"]["in_scene"][:, k], side["noise"])
                _, info32 = H.replay_resampling(*args)
                with H.oracle_in_float64():
                    _, info64 = H.replay_resampling(*args)
                sat = (info32["alphas"][..., :-1] == 1.0).any(-1)
                zero = (_fold(side, got["coarse"][f"object_{k}"]["weights"]) == 0).all(-1) & side["flat"]["in_scene"][:, k].unsqueeze(-1)
                any_saturated = sat if any_saturated is None else any_saturated | sat
                any_empty = zero if any_empty is None else any_empty | zero
                depths += info64["either"].numel()
                either += int(info64["either"].sum())
                threshold += int(info64["threshold"].sum())
                fallback += int(info64["fallback"].sum())
            rays += any_saturated.numel()
            saturated += int(any_saturated.sum())
            empty += int(any_empty.sum())
            for level in LEVELS:
                lists = _lists(got, level, K)
                comp = H.replay_composition(side["cfg"], lists, side["flat"]["d"], _noise(side, f"int_{level}_global"))
                owner = torch.cat([torch.full((lists[k][0].size(-1),), k) for k in range(K)])[comp["order"]]
                ties += int(((comp["t"][..., 1:] == comp["t"][..., :-1]) & (owner[..., 1:] != owner[..., :-1])).any(-1).sum())
    print(f"{name}: saturated rays {saturated / rays:.3f}, empty rays {empty / rays:.3f}, threshold {threshold}, fallback {fallback}, "
          f"either {either / depths:.4f} of {depths} depths, rays with a cross-object tie {ties}")
    assert saturated >= 0.10 * rays and empty >= 0.10 * rays
    assert threshold >= 1 and fallback >= 1
    assert either <= 0.05 * depths
    assert ties >= 1
