"""Surface-like densities, CPU part ("Density regimes and stage replays"): the stage replays of
tests/helpers.py - what tests/test_density_regimes_gpu.py holds the HIP kernels against - are checked on the oracle alone.

  * fed the oracle's own intermediates, every replay reproduces ``ro.composer_forward`` (bit for bit in fp32, RTOL / ATOL in float64);
  * the derived bound of a resampled depth holds, with c = helpers.RESAMPLING_C, for two fp32 computations against float64;
  * the regimes reach what they are for (saturated alphas, the uniform-pdf path, the 1e-5 threshold, ties, the overlap fix);
  * the comparisons notice a swapped pair of weights, a depth in the wrong bin and a transmittance without its 1e-10 floor.

Case table (tests/helpers.py): tennis 16 + 32 positions on 16 x 16 pixels, tennis 64 + 128 on 8 x 8, the reduced minecraft
configuration with the overlap fix on 12 x 12; regimes: sigma head x 3e4 (x 3e5 with 64 coarse positions) with the 0.5 (surfaces),
0.05 (solid) and 0.95 (sparse) quantile of every network's in-box densities moved to zero."""
import functools

import pytest
import torch

from oracle import render_oracle as ro
from tests import helpers as H
from tests.helpers import DENSITY_CASES, DENSITY_REGIMES, INTEGRATED_FIELDS, REPLAY_ATOL, REPLAY_RTOL, RESAMPLING_C

REGIMES = list(DENSITY_REGIMES)
LEVELS = ("coarse", "fine")


@functools.lru_cache(maxsize=None)
def oracle_run(name, regime, perturb):
    """The fp32 and the float64 oracle of one case on the same weights, inputs and draws, with the arguments of every resampling and
    integration call (computed once, shared, read only)."""
    cfg, _, inputs, sd = H.density_case(name, regime)
    rec = {}
    with torch.no_grad():
        torch.manual_seed(123)
        want, resampled, integrated = H.capture_oracle_stages(
            lambda: ro.composer_forward(cfg, sd, *inputs, perturb, record_noise=rec, stable_merge=True))
        with H.oracle_in_float64():
            exact, resampled64, integrated64 = H.capture_oracle_stages(
                lambda: ro.composer_forward(cfg, H.to_double(sd), *H.to_double(list(inputs)), perturb, noise=H.to_double(rec),
                                            update_stats=False, stable_merge=True))
    flat = H.flat_composer_inputs(inputs)
    return dict(cfg=cfg, sd=sd, inputs=inputs, flat=flat, noise=rec if perturb else None, K=flat["K"],
                fp32=dict(result=want, resampled=resampled, integrated=integrated),
                fp64=dict(result=exact, resampled=resampled64, integrated=integrated64))


def _fold(run, v, tail=1):
    """(lead..., R, ...) -> (N, R, ...), the layout of the replays."""
    return v.reshape([-1, run["flat"]["R"]] + list(v.shape[v.dim() - tail:]))


def _object_list(run, side, level, k):
    """(t, raw, displacements) object ``k`` was integrated with at ``level`` (integration calls: per level the objects, then global)."""
    call = run[side]["integrated"][LEVELS.index(level) * (run["K"] + 1) + k]
    return _fold(run, call["t"]), _fold(run, call["raw"]), _fold(run, call["displacements"], 2)


def _noise(run, key):
    return None if run["noise"] is None else run["noise"][key]


def _resampling(run, side, k, dtype64):
    """replay_resampling of object ``k`` fed the coarse list of ``side``'s oracle run, in fp32 or float64."""
    t, raw, _ = _object_list(run, side, "coarse", k)
    d = _fold(run, run[side]["resampled"][k]["directions"])
    if side == "fp32":
        assert torch.equal(d, H.object_frame_rays(run["flat"], k)[1])          # (what the GPU tests feed the replay)
    args = (run["cfg"], k, t, raw, d, run["flat"]["in_scene"][:, k], run["noise"])
    if dtype64:
        with H.oracle_in_float64():      # (fed the float64 run, it also takes that run's float64 abscissae)
            fixed_u = torch.linspace(0.0, 1.0, H._object_config(run["cfg"], k)["positions_count_fine"]) if side == "fp64" else None
            return t, H.replay_resampling(*args, fixed_u=fixed_u)
    return t, H.replay_resampling(*args)


def _assert_fields(want, got, exact, what):
    rtol, atol = (0.0, 0.0) if exact else (REPLAY_RTOL, REPLAY_ATOL)
    rep = H.compare_results(want, got, rtol=rtol, atol=atol, position_wise=True)
    bad = {k: f"{v[0]:.3e}" for k, v in rep.items() if not v[1]}
    assert rep and not bad, (what, bad)


@pytest.mark.parametrize("side", ["fp32", "fp64"])
@pytest.mark.parametrize("perturb", [False, True], ids=["eval", "perturb"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", DENSITY_CASES)
def test_replays_reproduce_the_oracle(name, regime, perturb, side):
    """Every replay, fed the intermediates of the oracle run of its own dtype, returns that run's fields: bit for bit in fp32 (the
    replays ARE the oracle's functions), within RTOL / ATOL in float64; weights sample for sample."""
    run = oracle_run(name, regime, perturb)
    exact = side == "fp32"
    result, K = run[side]["result"], run["K"]
    ctx = H.oracle_in_float64 if side == "fp64" else torch.no_grad
    with ctx():
        for k in range(K):
            _, (merged, _) = _resampling(run, side, k, side == "fp64")
            _assert_fields({"t": _fold(run, run[side]["resampled"][k]["merged"])}, {"t": merged}, exact, ("resampling", k))
        for level in LEVELS:
            lists, feats = [], []
            for k in range(K):
                t, raw, disp = _object_list(run, side, level, k)
                lists.append((t, raw, disp))
                got = H.replay_integration(t, raw, disp, run["flat"]["d"], _noise(run, f"int_{level}_{k}"))
                want = {f: _fold(run, result[level][f"object_{k}"][f], 1 if f == "weights" else 0) for f in ("weights",) + INTEGRATED_FIELDS}
                _assert_fields(want, {f: got[f] for f in want}, exact, ("integration", level, k))
                if exact:
                    feats.append(H.replay_features(run["cfg"], run["sd"], run["flat"], k, level, t, torch.zeros(t.shape, dtype=torch.int32))[0])
            got = H.replay_composition(run["cfg"], lists, run["flat"]["d"], _noise(run, f"int_{level}_global"))
            want = {f: _fold(run, result[level]["global"][f], 1 if f == "weights" else 0) for f in ("weights",) + INTEGRATED_FIELDS}
            _assert_fields(want, {f: got[f] for f in want}, exact, ("composition", level))
            assert got["order"].shape == got["weights"].shape
            if exact:       # (the float64 run places its samples with float64 depths: its in-box decisions are its own)
                weights = [_fold(run, result[level][f"object_{k}"]["weights"]) for k in range(K)]
                per_object, total = H.expected_features(feats, weights, got["weights"], got["order"])
                want = {f"object_{k}": _fold(run, result[level][f"object_{k}"]["integrated_features"]) for k in range(K)}
                want["global"] = _fold(run, result[level]["global"]["integrated_features"])
                _assert_fields(want, dict({f"object_{k}": per_object[k] for k in range(K)}, **{"global": total}), True, ("features", level))


@pytest.mark.parametrize("perturb", [False, True], ids=["fixed_u", "random_u"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", DENSITY_CASES)
def test_resampling_bound_holds_for_two_fp32_computations(name, regime, perturb):
    """The bound of helpers.replay_resampling with c = RESAMPLING_C against the float64 replay, for (a) the fp32 torch oracle and (b)
    the sequential fp32 restatement of k_resample's arithmetic, sample for sample; and the position-wise comparison the kernel is
    held to accepts the fp32 oracle's merged list.  Prints the worst ratio (in units of c = 1): the figure in the helper's docstring."""
    run = oracle_run(name, regime, perturb)
    worst = 0.0
    for k in range(run["K"]):
        t, (merged32, info32) = _resampling(run, "fp32", k, False)
        _, (_, info64) = _resampling(run, "fp32", k, True)
        flat2 = lambda v: v.reshape(-1, v.shape[-1])
        sequential = H.sequential_resampling_fp32(flat2(t), flat2(info32["alphas"]), flat2(info32["u"])).reshape(info32["new_t"].shape)
        for label, values in (("torch fp32", info32["new_t"]), ("sequential fp32", sequential)):
            ratio = float(H.resampling_ratio(info64, values).max())
            worst = max(worst, ratio)
            assert ratio <= RESAMPLING_C, (label, k, ratio)
        rep = H.compare_resampling(t, info64, merged32)
        assert rep["ok"], (k, rep)
    print(f"{name} {regime} {'random' if perturb else 'fixed'} u: worst ratio {worst:.3f} of c = 1 (c = {RESAMPLING_C})")


@pytest.mark.parametrize("name", DENSITY_CASES)
def test_regimes_reach_what_they_are_for(name):
    """Conditions on the ORACLE, over the three regimes of a case together (eval and perturbed runs): saturated alphas, the uniform
    pdf, the 1e-5 threshold and the fallback, a cap on the either-branch depths, cross-object ties, and the overlap fix."""
    rays = saturated = empty = depths = either = threshold = fallback = ties = masked = 0
    for regime in REGIMES:
        for perturb in (False, True):
            run = oracle_run(name, regime, perturb)
            K = run["K"]
            any_saturated = any_empty = None
            for k in range(K):
                _, (_, info32) = _resampling(run, "fp32", k, False)
                _, (_, info64) = _resampling(run, "fp32", k, True)
                assert info32["alphas"].dtype == torch.float32
                # a coarse alpha of exactly 1.0f - not counting the last sample, whose 1e10 step saturates any positive density
                sat = (info32["alphas"][..., :-1] == 1.0).any(-1)
                zero = (info32["weights"] == 0).all(-1) & run["flat"]["in_scene"][:, k].unsqueeze(-1)
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
                lists = [_object_list(run, "fp32", level, k) for k in range(K)]
                comp = H.replay_composition(run["cfg"], lists, run["flat"]["d"], _noise(run, f"int_{level}_global"))
                owner = torch.cat([torch.full((lists[k][0].size(-1),), k) for k in range(K)])[comp["order"]]
                tie = (comp["t"][..., 1:] == comp["t"][..., :-1]) & (owner[..., 1:] != owner[..., :-1])
                ties += int(tie.any(-1).sum())
                masked += sum(int(m.sum()) for m in comp["masked"][:ro.ObjectLayout(run["cfg"]).static_objects])
    print(f"{name}: saturated rays {saturated / rays:.3f}, empty rays {empty / rays:.3f}, threshold {threshold}, fallback {fallback}, "
          f"either {either / depths:.4f} of {depths} depths, rays with a cross-object tie {ties}, masked static samples {masked}")
    assert saturated >= 0.10 * rays
    assert empty >= 0.10 * rays
    assert threshold >= 1 and fallback >= 1
    assert either <= 0.05 * depths
    assert ties >= 1
    if name == "minecraft_hierarchical":
        assert masked >= 1


def _saturated_list(run):
    """(level, k, ray index) of an object list with an alpha of exactly 1.0f in front of a sample with alpha > 1e-6, and its replays."""
    for level in LEVELS:
        for k in range(run["K"]):
            t, raw, disp = _object_list(run, "fp32", level, k)
            got = H.replay_integration(t, raw, disp, run["flat"]["d"], None)
            hit = ((got["alphas"] == 1.0).cumsum(-1) > 0)[..., :-1] & (got["alphas"][..., 1:] > 1e-6)
            if hit.any():
                with H.oracle_in_float64():
                    exact = H.replay_integration(t, raw, disp, run["flat"]["d"], None)
                return got, exact
    raise AssertionError("no saturated list")


@pytest.mark.parametrize("name", DENSITY_CASES)
def test_the_comparisons_are_sensitive(name):
    """Each tampering must fail the comparison the kernels are held to (and the untampered fp32 oracle must pass it): two adjacent
    global weights swapped, one resampled depth moved by one bin, the transmittance without its 1e-10."""
    run = oracle_run(name, "surfaces", False)
    K = run["K"]
    # ---- 1. two adjacent global weights of a ray with two non-zero weights change places
    lists = [_object_list(run, "fp32", "fine", k) for k in range(K)]
    got = H.replay_composition(run["cfg"], lists, run["flat"]["d"], None)
    with H.oracle_in_float64():
        exact = H.replay_composition(run["cfg"], lists, run["flat"]["d"], None)
    assert all(v[1] for v in H.compare_integration(exact, got).values())
    w = got["weights"]
    pair = ((w[..., 1:] > 1e-3) & (w[..., :-1] > 1e-3) & ((w[..., 1:] - w[..., :-1]).abs() > 1e-3)).nonzero()
    assert len(pair), "no ray with two different non-zero neighbours"
    n, r, j = pair[0].tolist()
    swapped = dict(got, weights=w.clone())
    swapped["weights"][n, r, j], swapped["weights"][n, r, j + 1] = w[n, r, j + 1], w[n, r, j]
    assert not H.compare_integration(exact, swapped)["weights"][1]
    assert H.compare_results({"weights": exact["weights"]}, {"weights": swapped["weights"]}, REPLAY_RTOL, REPLAY_ATOL)["weights"][1], \
        "the sorted comparison does not see it: what position_wise is for"
    assert not H.compare_results({"weights": exact["weights"]}, {"weights": swapped["weights"]}, REPLAY_RTOL, REPLAY_ATOL,
                                 position_wise=True)["weights"][1]
    # ---- 2. one resampled depth lands one bin further.  The depth is the one whose bin width AND distance to its nearest neighbour
    #         in the merged list are largest against its bound: on a thin, distant box a bin is barely wider than RTOL |t|, and among
    #         densely placed depths the sorted lists differ by one spacing per position, whatever moved - both are properties of
    #         the tolerance, not of the comparison
    best = None
    for k in range(K):
        t, (merged32, info32) = _resampling(run, "fp32", k, False)
        _, (_, info64) = _resampling(run, "fp32", k, True)
        assert H.compare_resampling(t, info64, merged32)["ok"]
        inner = (~info64["fallback"]) & (~info64["either"]) & (info64["den"] > 1e-3)
        others = torch.cat([t.double(), info64["new_t"]], -1).unsqueeze(-2) - info64["new_t"].unsqueeze(-1)
        others[..., t.size(-1):].diagonal(dim1=-2, dim2=-1).fill_(float("inf"))
        alone = others.abs().amin(-1)
        margin = torch.where(inner, torch.minimum(info64["width"].abs(), alone) / info64["candidate_bounds"][..., 0],
                             torch.zeros_like(info64["width"]))
        if best is None or float(margin.max()) > best[0]:
            best = (float(margin.max()), k, margin)
    margin, k, where = best
    assert margin > 2.0, margin
    t, (merged32, info32) = _resampling(run, "fp32", k, False)
    _, (_, info64) = _resampling(run, "fp32", k, True)
    n, r, f = (where == where.max()).nonzero()[0].tolist()
    moved = info32["new_t"].clone()
    moved[n, r, f] += info64["width"][n, r, f].float()
    shifted = torch.sort(torch.cat([t, moved], -1), -1)[0]
    rep = H.compare_resampling(t, info64, shifted)
    assert not rep["ok"] and rep["outside"] >= 1 and rep["sorted"] and rep["coarse_present"], rep
    dropped = merged32.clone()                     # and a coarse depth that is not there bit for bit
    at = (dropped[n, r] == t[n, r, 1]).nonzero()[0]
    dropped[n, r, at] = torch.nextafter(t[n, r, 1], t[n, r, 2])
    rep = H.compare_resampling(t, info64, dropped)
    assert not rep["coarse_present"] and not rep["ok"]
    # ---- 3. the transmittance without its floor: exact zeros behind the first saturated sample
    got, exact = _saturated_list(run)
    assert all(v[1] for v in H.compare_integration(exact, got).values())
    alphas = got["alphas"]
    shifted = torch.cat([torch.ones_like(alphas[..., :1]), 1.0 - alphas[..., :-1]], -1)            # (no + 1e-10)
    bare = dict(got, weights=alphas * torch.cumprod(shifted, -1))
    rep = H.compare_integration(exact, bare)
    assert rep["weights"][1], "the floor is far below ATOL: the tolerance alone cannot see it"
    assert not rep["weights/floor"][1] and rep["weights/floor"][0] >= 1
