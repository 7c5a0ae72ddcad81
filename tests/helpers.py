"""Shared helpers of the test-suite (tests may use the oracle; the product never does)."""
import contextlib

import torch

from oracle import render_oracle as ro


def grid_pixels(h, w, n):
    r = torch.linspace(0, h - 1, n).long()
    c = torch.linspace(0, w - 1, n).long()
    rr, cc = torch.meshgrid(r, c, indexing="ij")
    return rr.reshape(-1), cc.reshape(-1)


def composer_inputs(config, scene, strides=None, pixels=None):
    """Scene encoding -> the seven tensors ObjectComposer.forward takes (CPU, via the oracle's ray set-up)."""
    rows = cols = None
    if strides:
        rows, cols = ro.strided_grid_pixels(scene["image_size"][0], scene["image_size"][1], strides)
    if pixels is not None:
        rows, cols = pixels
    o, d, n = ro.world_rays_from_cameras(config, scene["camera_rotations"], scene["camera_translations"],
                                         scene["focals"], scene["image_size"], rows, cols)
    w2o, _ = ro.object_matrices(scene["object_rotation_parameters"], scene["object_translation_parameters"])
    return (o, d, n, w2o, scene["object_style"].unsqueeze(-3), scene["object_deformation"].unsqueeze(-3),
            scene["object_in_scene"].unsqueeze(-2))


def poison_device_memory():
    """Leaves NaN bit patterns in the blocks torch's caching allocator hands out next (the renderer's workspaces are
    ``torch.empty``): a kernel that reads scratch it never wrote - padded columns, rows beyond the compacted count - then
    produces NaNs instead of passing by luck on fresh (zero) pages."""
    blocks = [torch.full((64 << 20,), float("nan"), device="cuda") for _ in range(4)]
    small = [torch.full((n,), float("nan"), device="cuda") for n in (1 << 10, 1 << 14, 1 << 18, 1 << 20, 1 << 22) for _ in range(4)]
    del blocks, small


@contextlib.contextmanager
def oracle_in_float64():
    """The oracle's op graph in float64 (every tensor it creates takes torch's default dtype): the arbiter where a tolerance
    is wider than fp32 round-off.  Pass weights / inputs through ``to_double``."""
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


def to_double(x):
    if torch.is_tensor(x):
        return x.detach().cpu().double() if x.is_floating_point() else x.detach().cpu()
    if isinstance(x, dict):
        return {k: to_double(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to_double(v) for v in x)
    return x


def arbitrate(exact, oracle32, hip, factor=4.0, floor=1e-6, path="", out=None, position_wise=False):
    """Per field of a composer result: (max |HIP - fp64|, max |fp32 oracle - fp64|, ok) with
    ok = |HIP - fp64| <= factor x |fp32 oracle - fp64| + floor x max |fp64| - the HIP path may be as far from the exact
    result as the fp32 restatement of the reference is (times a small factor), not farther.  ``weights`` are sorted before the
    comparison unless ``position_wise`` (all three sides then need the same tie rule, e.g. ``stable_merge=True``)."""
    out = out if out is not None else {}
    for k in exact:
        if k in ("pytorch_hook", "extra_outputs") or k.startswith("_"):
            continue
        if isinstance(exact[k], dict):
            arbitrate(exact[k], oracle32[k], hip[k], factor, floor, path + k + ".", out, position_wise)
            continue
        e, a, b = (t.detach().cpu().double() for t in (exact[k], oracle32[k], hip[k]))
        if k == "weights" and not position_wise:
            e, a, b = torch.sort(e, -1)[0], torch.sort(a, -1)[0], torch.sort(b, -1)[0]
        clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)
        err_hip = float(clean(b - e).abs().max()) if e.numel() else 0.0
        err_ref = float(clean(a - e).abs().max()) if e.numel() else 0.0
        scale = float(clean(e).abs().max()) if e.numel() else 0.0
        out[path + k] = (err_hip, err_ref, err_hip <= factor * err_ref + floor * scale)
    return out


def bender_kink_margin(run_oracle):
    """Smallest relative distance of a sample to a KINK of the ray benders' Jacobian while ``run_oracle()`` (a callable that runs
    the oracle) executes: a raw displacement at its clamp bound (``minimum(maximum(delta, lo - x), hi - x)``,
    model/nerf_models/positional_ray_bender_model.py:81-163 - the Jacobian switches between the network's and -1) or a hidden
    unit's pre-activation at 0.  The Hutchinson divergence estimate is a function of that Jacobian: it is DISCONTINUOUS there, and a
    sample within fp32 rounding of a kink legitimately lands on either side (randomized backward sweep, seed 7 case 0: one sample
    6e-9 of the box size from its clamp bound moved object_2's integrated_divergence by 3 % while every other field agreed to 4e-9)."""
    import torch.nn.functional as F
    from oracle import render_oracle as ro
    original = ro.bender_forward
    margins = []

    def traced(sd, prefix, cfg, bbox, x, deformation):
        with torch.no_grad():
            if x.numel():
                pe_cfg = cfg["position_encoder"]
                size = bbox[:, 1] - bbox[:, 0]
                w = ro.annealing_weights(sd[prefix + "positional_encoder.current_step"], pe_cfg["octaves"], pe_cfg["num_steps"])
                enc = ro.positional_encoding(x / size, pe_cfg["octaves"], pe_cfg["append_original"], w)
                h = torch.cat([enc, deformation], dim=-1)
                for i in range(cfg["layers_count"]):
                    if i == cfg["skip_layer_idx"]:
                        h = torch.cat([h, enc, deformation], dim=-1)
                    pre = F.linear(h, sd[prefix + f"backbone_layers.{i}.weight"], sd[prefix + f"backbone_layers.{i}.bias"])
                    margins.append(float((pre.abs() / pre.abs().max().clamp_min(1e-30)).min()))
                    h = F.relu(pre)
                delta = F.linear(h, sd[prefix + "output_head.weight"]) * size
                lo, hi = bbox[:, 0].unsqueeze(0) - x, bbox[:, 1].unsqueeze(0) - x
                margins.append(float(torch.minimum((delta - lo).abs(), (delta - hi).abs()).min() / size.max()))
        return original(sd, prefix, cfg, bbox, x, deformation)

    ro.bender_forward = traced
    try:
        run_oracle()
    finally:
        ro.bender_forward = original
    return min(margins) if margins else 1.0


def compare_results(want, got, rtol, atol, path="", out=None, position_wise=False):
    """NaN-aware comparison of two composer result dicts; ``weights`` are compared after sorting
    (tie order inside equal-t groups is unspecified in the reference) unless ``position_wise``: then sample for sample, which
    needs both sides to define their ties alike (``stable_merge=True``).  Returns {field: (maxdiff, ok)}."""
    out = out if out is not None else {}
    for k in want:
        if k in ("pytorch_hook", "extra_outputs") or k.startswith("_"):
            continue
        if isinstance(want[k], dict):
            compare_results(want[k], got[k], rtol, atol, path + k + ".", out, position_wise)
            continue
        a, b = want[k].detach().cpu().float(), got[k].detach().cpu().float()
        assert a.shape == b.shape, f"{path + k}: shape {tuple(b.shape)} != {tuple(a.shape)}"
        if k == "weights" and not position_wise:
            a, _ = torch.sort(a, dim=-1)
            b, _ = torch.sort(b, dim=-1)
        nan_ok = torch.equal(torch.isnan(a), torch.isnan(b))
        diff = torch.nan_to_num(a - b, nan=0.0, posinf=0.0, neginf=0.0).abs().max().item()
        ok = nan_ok and torch.allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)
        out[path + k] = (diff, ok)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Stand-in encoders for the observation-driven modes (EnvironmentModel.forward_from_observations needs one object encoder
# and one object-parameters encoder per object model; the reference's are CNNs with roi_pool crops, out of scope).  Small
# deterministic, differentiable torch modules with the call contracts of the reference's modules, so that the reference
# itself (build container) and this package (GPU box) can run the same scene.
class StandInObjectEncoder(torch.nn.Module):
    """Contract of ObjectEncoderV4.forward (model/object_encoder_v4.py:80-178): (observations (..., O, C, 3, H, W),
    bounding_box (..., O, C, 4), camera_rotations, camera_translations, global_frame_indexes, video_frame_indexes,
    video_indexes) -> (style (..., O, S), deformation (..., O, D), attention, crops)."""

    def __init__(self, style_features: int, deformation_features: int, seed: int):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.to_style = torch.nn.Parameter(torch.randn(7, style_features, generator=g))
        self.to_deformation = torch.nn.Parameter(torch.randn(7, deformation_features, generator=g))

    def forward(self, observations, bounding_box, camera_rotations, camera_translations, global_frame_indexes,
                video_frame_indexes, video_indexes):
        colour = observations[..., 0, :, :, :].mean(dim=(-1, -2))                      # first camera, (..., O, 3)
        code = torch.cat([colour, bounding_box[..., 0, :]], dim=-1)                    # (..., O, 7)
        style = torch.tanh(code @ self.to_style)
        deformation = torch.tanh(code @ self.to_deformation)
        attention = torch.zeros(list(code.shape[:-1]) + [1, 1, 2, 2], device=code.device)
        crops = observations[..., 0:1, :, :4, :4]
        return style, deformation, attention, crops


class StandInStaticParameters(torch.nn.Module):
    """Static object models sit at the world origin (model/static_object_parameters_encoder.py): (observations) ->
    rotations, translations (..., O, 3, objects)."""

    def __init__(self, objects_count: int):
        super().__init__()
        self.objects_count = objects_count

    def forward(self, observations):
        shape = list(observations.shape[:-4]) + [3, self.objects_count]
        zeros = torch.zeros(shape, device=observations.device)
        return zeros, zeros.clone()


class StandInDynamicParameters(torch.nn.Module):
    """Contract of ClassicObjectParametersEncoder.forward (model/classic_object_parameters_encoder.py:129-237):
    (observations, transformation_matrix_w2c, camera_rotations, focals, bounding_boxes (..., O, C, 4, n),
    bounding_boxes_validity (..., O, C, n)) -> rotations, translations (..., O, 3, n).  The pose is an affine function of
    the first camera's box centre: ``translation = origin + u * (cx - .5) + v * (cy - .5)``, rotation about ``up``."""

    def __init__(self, origin, u, v, up_axis: int, gain: float = 1.0):
        super().__init__()
        self.register_buffer("origin", torch.as_tensor(origin, dtype=torch.float32))
        self.register_buffer("u", torch.as_tensor(u, dtype=torch.float32))
        self.register_buffer("v", torch.as_tensor(v, dtype=torch.float32))
        self.up_axis = up_axis
        self.gain = torch.nn.Parameter(torch.tensor(float(gain)))

    def forward(self, observations, transformation_matrix_w2c, camera_rotations, focals, bounding_boxes,
                bounding_boxes_validity):
        box = bounding_boxes[..., 0, :, :]                                             # first camera, (..., O, 4, n)
        cx = (box[..., 0, :] + box[..., 2, :]) / 2 - 0.5                               # (..., O, n)
        cy = (box[..., 1, :] + box[..., 3, :]) / 2 - 0.5
        translation = (self.origin.unsqueeze(-1) + self.u.unsqueeze(-1) * cx.unsqueeze(-2) * self.gain
                       + self.v.unsqueeze(-1) * cy.unsqueeze(-2) * self.gain)          # (..., O, 3, n)
        rotation = torch.zeros_like(translation)
        rotation[..., self.up_axis, :] = cx * 0.5
        return rotation, translation


def stand_in_encoders(config, world: str, seed: int = 5):
    """(object_encoders, object_parameters_encoders) for a tennis or minecraft configuration: one module per object model."""
    static = config["model"]["static_object_models"]
    enc, par = [], []
    for m, mcfg in enumerate(config["model"]["object_models"]):
        enc.append(StandInObjectEncoder(mcfg["style_features"], mcfg["deformation_features"], seed + m))
        count = int(config["model"]["object_parameters_encoder"][m]["objects_count"])
        if m < static:
            par.append(StandInStaticParameters(count))
        elif world == "tennis":   # z up, court in the xy plane
            par.append(StandInDynamicParameters(origin=(0.0, 1.0, 0.01), u=(8.0, 0.0, 0.0), v=(0.0, -30.0, 0.0), up_axis=2))
        else:                     # minecraft: y up
            par.append(StandInDynamicParameters(origin=(0.0, 0.0, 0.0), u=(0.0, 0.0, 8.0), v=(8.0, 0.0, 0.0), up_axis=1))
    return enc, par


from playableenvironments_amd.synthetic import observation_batch  # noqa: E402,F401  (shared with bench.py)


# ---------------------------------------------------------------------------------------------------------------------
# forward_pose_consistency / forward_keypoint_consistency against the reference's recorded outputs (tests/golden/consistency,
# oracle/make_golden.py consistency): shared by the CPU suite (oracle composer behind the product's host logic) and the GPU suite
CONSISTENCY_KEYS = ("camera_rotations", "camera_translations", "focals", "bounding_boxes", "bounding_boxes_validity",
                    "global_frame_indexes", "video_frame_indexes", "video_indexes")


def run_consistency_fixture(z, model, device, monkeypatch):
    """Replays the fixture's random draws through ``model`` and returns {label: (reference tensor, product tensor)}."""
    from playableenvironments_amd import ray_sampling
    t = lambda name: torch.from_numpy(z[name]).to(device)
    queues = {"object": [], "keypoints": []}
    for kind in queues:
        i = 0
        while f"draw/{kind}/{i}/0" in z.files:
            queues[kind].append(tuple(t(f"draw/{kind}/{i}/{j}") for j in range(3)))
            i += 1
    assert len(queues["object"]) == 2 and len(queues["keypoints"]) == 2
    monkeypatch.setattr(ray_sampling, "sample_rays_at_object", lambda *a, **k: queues["object"].pop(0))
    monkeypatch.setattr(ray_sampling, "sample_rays_at_keypoints", lambda *a, **k: queues["keypoints"].pop(0))
    common = [t("in/" + k) for k in CONSISTENCY_KEYS] + [t("se/" + k) for k in ("object_style", "object_deformation",
                                                                                "object_rotation_parameters",
                                                                                "object_translation_parameters")]
    with torch.no_grad():
        pose = model(t("in/optical_flow"), *common, 30, False, mode="pose_consistency")
        kp = model(t("in/observations"), *common, t("in/keypoints"), t("in/bounding_boxes_validity"), 20, False,
                   mode="keypoint_consistency")
    assert not queues["object"] and not queues["keypoints"]
    pairs = {}
    for name, (previous, following) in pose["coarse"].items():
        for tag, (positions, opacity) in (("previous", previous), ("following", following)):
            pairs[f"pose/{name}/{tag}/positions"] = positions
            pairs[f"pose/{name}/{tag}/opacity"] = opacity
    for name, (positions, confidence, opacity, sampled) in kp["coarse"].items():
        for tag, value in (("positions", positions), ("confidence", confidence), ("opacity", opacity), ("sampled", sampled)):
            pairs[f"keypoint/{name}/{tag}"] = value
    recorded = [k for k in z.files if k.startswith(("pose/", "keypoint/"))]
    assert sorted(recorded) == sorted(pairs), (sorted(recorded), sorted(pairs))
    return {k: (torch.from_numpy(z[k]), v.detach().cpu()) for k, v in pairs.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Surface-like densities and the stage-wise replay of everything behind the MLP ("Density regimes and stage
# replays"): every stage of the HIP chain - alphas / transmittance, inverse CDF + merge, per-object and cross-object weights, the
# feature sums - is compared with the oracle's function for THAT stage, fed the kernel's own exported inputs of the stage.
REPLAY_RTOL, REPLAY_ATOL = 1e-4, 1e-5          # the project's fp32 tolerance (tests/test_gpu.py)
FP32_EPS = 2.0 ** -23
#: the one free constant of the resampled depths' error bound (replay_resampling): measured on the CPU only, never on the kernel
RESAMPLING_C = 1.0
#: regime: (sigma-head scale - times the case's own factor, see the case table -, quantile of each network's in-box densities that
#: is moved to zero).  Chosen on the CPU so that the
#: oracle alone meets the reach conditions of tests/test_density_regimes_cpu.py on every case:
#:   surfaces  empty and opaque regions alternate inside each box,
#:   solid     nearly every in-box sample is opaque, the first hit saturates,
#:   sparse    most rays are empty, a few carry a thin opaque shell.
DENSITY_REGIMES = {"surfaces": (3e4, 0.5), "solid": (3e4, 0.05), "sparse": (3e4, 0.95)}


def in_box_densities(cfg, sd, inputs):
    """{state-dict prefix of a NeRF network: its raw in-box densities} over one unperturbed oracle run."""
    original = ro.adain_nerf_forward
    seen = {}

    def traced(sd_, prefix, ncfg, bbox, empty_alpha, x, *rest):
        feats, sigma = original(sd_, prefix, ncfg, bbox, empty_alpha, x, *rest)
        seen.setdefault(prefix, []).append(sigma[ro._in_box(x, bbox)])
        return feats, sigma

    ro.adain_nerf_forward = traced
    try:
        with torch.no_grad():
            ro.composer_forward(cfg, sd, *inputs, False, update_stats=False, stable_merge=True)
    finally:
        ro.adain_nerf_forward = original
    return {k: torch.cat(v) for k, v in seen.items()}


def shape_sigma(comp, scale, quantile, cfg=None, inputs=None, biases=None):
    """Densities of a trained model's kind: every ``alpha_head.weight`` times ``scale``, every ``alpha_head.bias`` set so that the
    ``quantile`` of that network's in-box densities is zero (tests/test_query_gpu.py does this with the median of one network).
    The quantiles are measured with the oracle on the CPU module (``cfg``, ``inputs``: the composer inputs of the case; the coarse
    networks first - the fine networks are sampled where the coarse ones send them) unless ``biases`` ({parameter name: value},
    what an earlier call returned) is given.  Returns the biases, so that every side carries identical weights."""
    params = dict(comp.named_parameters())
    with torch.no_grad():
        for name, p in params.items():
            if name.endswith("alpha_head.weight"):
                p.mul_(scale)
            elif name.endswith("alpha_head.bias"):
                p.zero_()
        if biases is None:
            biases = {}
            for level in ("coarse", "fine"):
                sd = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
                for prefix, sigma in in_box_densities(cfg, sd, inputs).items():
                    name = prefix + "alpha_head.bias"
                    if prefix.startswith(f"object_models_{level}.") and name in params and sigma.numel():
                        biases[name] = -float(torch.quantile(sigma.double(), quantile))
                        params[name].fill_(biases[name])
        else:
            for name, value in biases.items():
                params[name].fill_(value)
    return biases


def flat_composer_inputs(inputs):
    """The seven composer inputs with the leading dimensions folded into one (N), as the renderer's exports are laid out:
    o (N, 3), d (N, R, 3), n (N, 3), w2o (N, 4, 4, K), style (N, S, K), deformation (N, D, K), in_scene (N, K)."""
    o, d, n, w2o, style, deformation, in_scene = inputs
    lead, R, K = list(d.shape[:-2]), d.size(-2), w2o.size(-1)
    fold = lambda v, tail: torch.broadcast_to(v, lead + tail).reshape([-1] + tail)
    return dict(lead=lead, R=R, K=K, o=fold(o, [3]), d=d.reshape(-1, R, 3), n=fold(n, [3]), w2o=fold(w2o, [4, 4, K]),
                style=fold(style, [style.size(-2), K]), deformation=fold(deformation, [deformation.size(-2), K]),
                in_scene=fold(in_scene, [K]))


def object_frame_rays(flat, k):
    """(o, d) of object ``k`` in its own frame, fp32 op for op as the oracle (and, bit for bit, the kernels) form them."""
    o, d, _ = ro.transform_rays(flat["o"], flat["d"], flat["n"], flat["w2o"][..., k])
    return o, d


def _object_config(cfg, k):
    return cfg["model"]["object_models"][ro.ObjectLayout(cfg).model_of_object[k]]


def resampling_bound(width, den, gain, t, c=RESAMPLING_C):
    """|bin_hi - bin_lo| c 2^-23 g / den + RTOL |t| + ATOL (see replay_resampling)."""
    return width.abs() * (c * FP32_EPS) * gain / den + REPLAY_RTOL * t.abs() + REPLAY_ATOL


def replay_resampling(cfg, k, t_coarse, sigma_coarse, d_object, in_scene, noise, c=RESAMPLING_C, fixed_u=None):
    """Object ``k``'s coarse alphas, weights, the inverse CDF and the merge (oracle: alphas_from_raw, weights_from_alphas,
    sample_pdf, hierarchical_positions - the same operations in the same order, so in fp32 it IS the oracle) from the depths and
    raw densities of its coarse list, in torch's default dtype (float64 under ``oracle_in_float64``).  t_coarse, sigma_coarse
    (N, R, Pc); d_object (N, R, 3) object-frame directions; in_scene (N,); ``noise``: the recorded draws of a perturbed call
    (``alpha_k``, ``pdf_k``) or None; ``fixed_u``: the (Pf,) abscissae of an unperturbed call, by default the fp32
    ``linspace(0, 1, Pf)`` every fp32 side uses (the float64 oracle draws its own in float64).

    Returns (merged, info): ``merged`` (N, R, Pc + Pf) is the sorted fine depth list with every resampled depth on the branch the
    arithmetic of this dtype takes; ``info`` holds per resampled depth ``new_t``, its ``den`` (1 where the fallback applies), the
    bin ``width``, the flags ``fallback`` and ``threshold``, its ``second`` candidate (the other branch of ``den < 1e-5 -> 1``)
    with ``second_den``, and ``candidates`` / ``candidate_bounds`` / ``candidate_valid`` (..., Pf, 6): every value a correct fp32
    computation may produce with its bound (below); ``either`` marks the depths with more than one.  Also the coarse ``alphas``,
    ``weights`` and ``total`` (S, the sum that normalises the pdf).

    ERROR BOUND of a resampled depth (derived, not tuned):
        |bin_hi - bin_lo| c 2^-23 / (den min(1, S)) + RTOL |t| + ATOL,        S = sum(weights[1:-1] + 1e-5).
    alpha = 1 - exp(.) <= 1 and every factor 1 - alpha + 1e-10 carries an absolute error of an fp32 ulp of 1, so every coarse
    weight does (a few of them), however small it is; pdf = (w + 1e-5) / S and its running sum therefore carry a few 2^-23 / S -
    and S is far below 1 on a ray whose FIRST sample is nearly opaque (weights[0] is not part of the pdf: the samples behind it
    share a transmittance of 1e-3, known to 2^-23, i.e. to 1e-4 of itself).  ``frac = (u - cdf_lo) / den`` carries that over den,
    the depth that times the bin width; the last two terms are the project's tolerance on the depth itself.  ``c`` is the only
    free constant: the smallest power of two for which two fp32 computations - this function in fp32, and
    sequential_resampling_fp32 - stay inside the bound against this function in float64 on every case of
    tests/test_density_regimes_cpu.py.  MEASURED there (the test prints it): worst ratio 0.79 of c = 1 for the sequential restatement and 0.69 for the torch oracle
    (both on minecraft_hierarchical, the 16-position background behind a nearly opaque first sample), 0.00 wherever RTOL |t|
    alone covers the difference (the tennis boxes, 20 - 50 units from the camera) - so c = 1.  The kernel is held to the same bound
    and is never used to choose c.

    EITHER-BRANCH RULES (both are discontinuities of the reference's algorithm, not of an implementation):
      threshold  ``den`` within c 2^-23 / min(1, S) of 1e-5: the depth computed with den and the one computed with 1 are both
                 accepted, each with its bound;
      bin edge   ``u`` within c 2^-23 / min(1, S) of a cdf entry: searchsorted may place it in the neighbouring bin.  The
                 inverse CDF is continuous across an edge EXCEPT next to a fallback bin, whose depths all sit at its lower end:
                 the fixed u = 1 against cdf[-1] = 1 +- ulp behind an empty last bin is the case every opaque ray has.
    compare_resampling picks, per ray, the candidate nearest to an element of the list under test; nothing is left out of the
    comparison, and the share of ``either`` depths is capped by the reach conditions."""
    dt = torch.get_default_dtype()
    mcfg = _object_config(cfg, k)
    noise = noise or {}
    alpha_noise, u_noise = noise.get(f"alpha_{k}"), noise.get(f"pdf_{k}")
    perturb = alpha_noise is not None
    t = t_coarse.to(dt)
    raw = sigma_coarse.to(dt).clone()
    raw[torch.logical_not(in_scene)] = mcfg["empty_space_alpha"]
    dist = ro.position_distances(t, d_object.to(dt))
    alphas, _ = ro.alphas_from_raw(raw, dist, perturb, alpha_noise.to(dt).reshape(raw.shape) if perturb else None)
    weights = ro.weights_from_alphas(alphas)
    count = mcfg["positions_count_fine"]
    # ---- ro.sample_pdf, with its intermediates kept ----
    bins = (t[..., 1:] + t[..., :-1]) / 2
    w = weights[..., 1:-1] + 1e-5
    total = torch.sum(w, dim=-1, keepdim=True)
    pdf = w / total
    cdf = torch.cumsum(pdf, dim=-1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], dim=-1)
    if not perturb:
        u = (torch.linspace(0.0, 1.0, count, dtype=torch.float32) if fixed_u is None else fixed_u).to(dt)
        u = u.expand(list(cdf.shape[:-1]) + [count]).contiguous()
    else:
        u = u_noise.to(dt).reshape(list(cdf.shape[:-1]) + [count]).contiguous()
    idx = torch.searchsorted(cdf, u, right=True)
    last = cdf.size(-1) - 1
    # exact zeros stay exact: a ray whose alphas in front of the last pdf bin are all 0.0 has the uniform pdf 1e-5 / S to ulps of 1
    gain = torch.where((alphas[..., :-1] != 0).any(-1, keepdim=True), 1.0 / total.clamp(max=1.0), torch.ones_like(total))
    window = c * FP32_EPS * gain

    def in_bin(idx):
        below = torch.clamp(idx - 1, min=0)
        above = torch.clamp(idx, max=last)
        cdf_lo, cdf_hi = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
        bin_lo, bin_hi = torch.gather(bins, -1, below), torch.gather(bins, -1, above)
        denom = cdf_hi - cdf_lo
        fallback = denom < 1e-5
        den = torch.where(fallback, torch.ones_like(denom), denom)
        first = bin_lo + (u - cdf_lo) / den * (bin_hi - bin_lo)
        second_den = torch.where(fallback & (denom > 0), denom, torch.ones_like(denom))
        second = bin_lo + (u - cdf_lo) / second_den * (bin_hi - bin_lo)
        return dict(first=first, den=den, second=second, second_den=second_den, width=bin_hi - bin_lo, fallback=fallback,
                    threshold=(denom - 1e-5).abs() <= window, cdf_lo=cdf_lo, cdf_hi=cdf_hi, below=below, above=above)

    here = in_bin(idx)
    new_t = here["first"]
    # the neighbouring bins of a depth whose u sits on a bin edge (cdf[0] = 0 <= u exactly: no bin below the first)
    down, up = in_bin(torch.clamp(idx - 1, min=1)), in_bin(torch.clamp(idx + 1, max=last + 1))
    down_ok = (idx >= 2) & ((u - here["cdf_lo"]).abs() <= window)
    up_ok = (idx <= last) & ((here["cdf_hi"] - u).abs() <= window)
    cands, bounds, valid = [], [], []
    for b, ok in ((here, torch.ones_like(down_ok)), (down, down_ok), (up, up_ok)):
        for value, den, on in ((b["first"], b["den"], ok), (b["second"], b["second_den"], ok & b["threshold"])):
            cands.append(value)
            bounds.append(resampling_bound(b["width"], den, gain, value, c))
            valid.append(on)
    valid = torch.stack(valid, -1)
    # a depth is an EITHER depth when an accepted candidate is another answer than the first, beyond the tolerance on a depth
    cands = torch.stack(cands, -1)
    either = (valid & ((cands - new_t.unsqueeze(-1)).abs() > REPLAY_RTOL * new_t.abs().unsqueeze(-1) + REPLAY_ATOL)).any(-1)
    merged, _ = torch.sort(torch.cat([t, new_t], dim=-1), dim=-1)
    info = dict(new_t=new_t, den=here["den"], width=here["width"], fallback=here["fallback"], threshold=here["threshold"],
                second=here["second"], second_den=here["second_den"], candidates=cands,
                candidate_bounds=torch.stack(bounds, -1), candidate_valid=valid, either=either, edge=down_ok | up_ok,
                alphas=alphas, weights=weights, total=total, gain=gain, u=u, cdf=cdf)
    return merged, info


def sequential_resampling_fp32(t_coarse, alphas, u):
    """numpy fp32 restatement of k_resample's lane-0 arithmetic and its inverse CDF: transmittance, sum and running sum strictly
    left to right (torch.sum is not), one rounding per operation.  t_coarse, alphas (M, Pc) fp32, u (M, Pf) fp32 -> (M, Pf)."""
    import numpy as np
    f = np.float32
    t, a, u = (np.ascontiguousarray(v.detach().cpu().numpy(), dtype=f) for v in (t_coarse, alphas, u))
    M, Pc = t.shape
    w = np.empty_like(a)
    trans = np.ones(M, f)
    for i in range(Pc):
        w[:, i] = a[:, i] * trans
        trans = trans * ((f(1.0) - a[:, i]) + f(1e-10))
    nb = Pc - 2
    total = np.zeros(M, f)
    for j in range(nb):
        total = total + (w[:, j + 1] + f(1e-5))
    cdf = np.zeros((M, nb + 1), f)
    run = np.zeros(M, f)
    for j in range(nb):
        run = run + (w[:, j + 1] + f(1e-5)) / total
        cdf[:, j + 1] = run
    mids = (t[:, 1:] + t[:, :-1]) / f(2.0)
    idx = (cdf[:, None, :] <= u[:, :, None]).sum(-1)            # searchsorted(right=True): first index with cdf > u
    below = np.clip(idx - 1, 0, None)
    above = np.clip(idx, None, nb)
    take = lambda v, i: np.take_along_axis(v, i, axis=1)
    den = take(cdf, above) - take(cdf, below)
    den = np.where(den < f(1e-5), f(1.0), den).astype(f)
    frac = (u - take(cdf, below)) / den
    out = take(mids, below) + frac * (take(mids, above) - take(mids, below))
    assert out.dtype == f
    return torch.from_numpy(out)


def resampling_ratio(info, new_t, c=RESAMPLING_C):
    """Per resampled depth of ``new_t`` (sample for sample, unsorted): what its distance to the float64 ``info`` beyond
    RTOL |t| + ATOL costs in units of |bin_hi - bin_lo| 2^-23 / (den min(1, S)) - the number that must stay <= c.  A depth with
    several candidates (replay_resampling) takes the best.  inf where the bin term is zero and the tolerance is exceeded."""
    got = new_t.double().unsqueeze(-1)
    cand, bound = info["candidates"].double(), info["candidate_bounds"].double()
    tol = REPLAY_RTOL * cand.abs() + REPLAY_ATOL
    excess = ((got - cand).abs() - tol).clamp_min(0.0)
    unit = (bound - tol) / c
    ratio = torch.where(excess > 0, excess / unit, torch.zeros_like(excess))          # (x / 0 = inf for x > 0)
    ratio = torch.where(info["candidate_valid"], ratio, torch.full_like(ratio, float("inf")))
    return ratio.amin(-1)


def compare_resampling(t_coarse, info, t_fine):
    """The merged, sorted list ``t_fine`` (N, R, Pc + Pf) of the side under test against the float64 ``info`` of
    replay_resampling, position by position.  Per ray every depth with several candidates takes the one nearest to an element of
    ``t_fine``; with every expected entry e_i known to its bound b_i (coarse depths: 0), the j-th smallest entry of a correct
    list lies between the j-th smallest e_i - b_i and the j-th smallest e_i + b_i (order statistics are monotone in every
    argument) - that interval is the position-wise check, it needs no assumption about which entries swap places.  Also: the list
    is sorted, and every coarse depth is in it bit for bit.
    Returns dict(ok, worst - the largest |t_fine - expected| in units of its interval's half-width -, sorted, coarse_present,
    outside - the number of entries outside their interval -, alternatives - the depths that took another candidate than the first)."""
    tc, got = t_coarse.double(), t_fine.double()
    cand, bound, valid = info["candidates"].double(), info["candidate_bounds"].double(), info["candidate_valid"]
    nearest = torch.stack([(cand[..., i].unsqueeze(-1) - got.unsqueeze(-2)).abs().amin(-1) for i in range(cand.size(-1))], -1)
    # (nearest in units of the candidate's own bound: two candidates of one value can differ in how well it is known)
    nearest = torch.where(valid, nearest / bound, torch.full_like(nearest, float("inf")))
    pick = nearest.argmin(-1, keepdim=True)                   # (ties: the first, i.e. the branch float64 takes)
    chosen, b_chosen = torch.gather(cand, -1, pick).squeeze(-1), torch.gather(bound, -1, pick).squeeze(-1)
    e = torch.cat([tc, chosen], dim=-1)
    b = torch.cat([torch.zeros_like(tc), b_chosen], dim=-1)
    lo, hi, mid = torch.sort(e - b, dim=-1)[0], torch.sort(e + b, dim=-1)[0], torch.sort(e, dim=-1)[0]
    inside = (got >= lo) & (got <= hi)
    half = torch.where(got >= mid, hi - mid, mid - lo)
    off = (got - mid).abs()
    worst = torch.where(off > 0, off / half, torch.zeros_like(off))
    is_sorted = bool((got[..., 1:] >= got[..., :-1]).all())
    # multiset inclusion of the coarse depths, bit for bit (a repeated depth must be there as often)
    have = (t_fine.unsqueeze(-1) == t_coarse.unsqueeze(-2)).sum(-2)
    need = (t_coarse.unsqueeze(-1) == t_coarse.unsqueeze(-2)).sum(-2)
    coarse_present = bool((have >= need).all())
    return dict(ok=bool(inside.all()) and is_sorted and coarse_present, worst=float(worst.max()), sorted=is_sorted,
                coarse_present=coarse_present, outside=int((~inside).sum()), alternatives=int((pick.squeeze(-1) != 0).sum()))


INTEGRATED_FIELDS = ("opacity", "depth", "disparity", "integrated_displacements_magnitude")


def replay_integration(t, sigma, delta, d_world, noise):
    """ro.integrate on one object's sample list (t, sigma (N, R, P); delta (N, R, P, 3) or None; d_world (N, R, 3); ``noise``: the
    recorded (N, R, P) draw of a perturbed call or None) in torch's default dtype: ``weights`` in sample order, the four scalar
    fields, and the ``alphas`` behind them."""
    dt = torch.get_default_dtype()
    t, sigma, d_world = t.to(dt), sigma.to(dt), d_world.to(dt)
    disp = delta.to(dt) if delta is not None else torch.zeros(list(t.shape) + [3])
    perturb = noise is not None
    noise = noise.to(dt).reshape(t.shape) if perturb else None
    out, _ = ro.integrate(torch.zeros(list(t.shape) + [0]), sigma, d_world, t, disp, torch.zeros_like(t), perturb, noise)
    alphas, _ = ro.alphas_from_raw(sigma, ro.position_distances(t, d_world), perturb, noise)
    return dict({k: out[k] for k in ("weights",) + INTEGRATED_FIELDS}, alphas=alphas)


def replay_composition(cfg, lists, d_world, noise):
    """ro.fix_overlaps + ro.compose(stable_merge=True) + ro.integrate on the objects' lists (``lists``: per object (t, sigma, delta or
    None), before the overlap fix; ``noise``: the recorded draw of the GLOBAL list or None): the global ``weights`` in merged
    order, the merged ``order`` itself (concatenation index per rank), the merged ``t``, the scalar fields, the ``alphas``, and
    ``masked`` (per object: the samples the overlap fix moved to t = 0)."""
    dt = torch.get_default_dtype()
    layout = ro.ObjectLayout(cfg)
    d_world = d_world.to(dt)
    all_t = [t.to(dt) for t, _, _ in lists]
    all_raw = [s.to(dt) for _, s, _ in lists]
    all_disp = [d.to(dt) if d is not None else torch.zeros(list(t.shape) + [3]) for t, _, d in lists]
    all_pos = [torch.zeros(list(t.shape) + [3]) for t in all_t]
    all_div = [torch.zeros_like(t) for t in all_t]
    index, begin = [], 0
    for t in all_t:                        # the "features" carried through the merge are the concatenation indices
        index.append((torch.arange(t.size(-1), dtype=dt) + begin).expand(t.shape).unsqueeze(-1))
        begin += t.size(-1)
    origins = torch.zeros(list(d_world.shape))
    masked = [torch.zeros(t.shape, dtype=torch.bool) for t in all_t]
    if cfg["model"]["fix_object_overlaps"]:
        fixed = ro.fix_overlaps(layout, all_raw, all_t, all_pos, all_disp, all_div, origins)
        masked = [(fr != r) | (ft != t) for fr, r, ft, t in zip(fixed[0], all_raw, fixed[1], all_t)]
    f, raw, t, disp, div = ro.compose(cfg, layout, origins, index, all_raw, all_t, all_pos, all_disp, all_div, stable_merge=True)
    perturb = noise is not None
    noise = noise.to(dt).reshape(t.shape) if perturb else None
    out, _ = ro.integrate(torch.zeros(list(t.shape) + [0]), raw, d_world, t, disp, div, perturb, noise)
    alphas, _ = ro.alphas_from_raw(raw, ro.position_distances(t, d_world), perturb, noise)
    return dict({k: out[k] for k in ("weights",) + INTEGRATED_FIELDS}, order=f[..., 0].round().long(), t=t, alphas=alphas,
                masked=masked)


def replay_features(cfg, sd, flat, k, level, t, slot):
    """The oracle's ``object_model_forward`` of object ``k``'s ``level`` network (``sd``: its state dict in torch's default
    dtype) at the sample positions the depths ``t`` (N, R, P) give - the object-frame o + d t, formed in fp32 op for op as the
    kernels form them, THEN widened - masked with ``slot >= 0``.  Returns (features (N, R, P, F), inside (N, R, P): the oracle's
    own in-box decision at those positions)."""
    dt = torch.get_default_dtype()
    layout = ro.ObjectLayout(cfg)
    m = layout.model_of_object[k]
    mcfg = cfg["model"]["object_models"][m]
    o, d = object_frame_rays(flat, k)
    x = o.unsqueeze(-2).unsqueeze(-2) + d.unsqueeze(-2) * t.float().unsqueeze(-1)
    inside = ro._in_box(x, ro._bbox_tensor(mcfg).float())
    sty = flat["style"][..., k].unsqueeze(-2).to(dt)
    dfm = flat["deformation"][..., k].unsqueeze(-2).to(dt)
    o_exp = o.unsqueeze(-2).expand(list(d.shape)).to(dt)
    with torch.no_grad():
        feats, _, _ = ro.object_model_forward(sd, f"object_models_{level}.{m}.", mcfg, x.to(dt), o_exp, d.to(dt), sty, dfm, False, False,
                                              update_stats=False)
    feats = feats * (slot >= 0).unsqueeze(-1).to(dt)
    if cfg["model"]["apply_activation"]:
        feats = torch.sigmoid(feats)
    return feats, inside


def expected_features(features, object_weights, global_weights, order):
    """sum_i w_i f_i with given weights: per object (``features`` / ``object_weights``: lists over the objects, sample order) and
    for the global list (``global_weights`` in merged order, ``order`` from replay_composition), summed as the oracle sums them."""
    dt = features[0].dtype
    per_object = [torch.sum(w.to(dt).unsqueeze(-1) * f, dim=-2) for w, f in zip(object_weights, features)]
    f = torch.cat(features, dim=-2)
    f = torch.gather(f, -2, order.unsqueeze(-1).expand_as(f))
    return per_object, torch.sum(global_weights.to(dt).unsqueeze(-1) * f, dim=-2)


def field_mismatch(want, got, rtol=REPLAY_RTOL, atol=REPLAY_ATOL):
    """(worst |got - want| / (atol + rtol |want|), ok) of two tensors compared position by position, NaNs in the same places."""
    a, b = want.detach().cpu().double(), got.detach().cpu().double().reshape(want.shape)
    same_nans = torch.equal(torch.isnan(a), torch.isnan(b))
    ratio = torch.nan_to_num((a - b).abs() / (atol + rtol * a.abs()), nan=0.0, posinf=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return worst, same_nans and worst <= 1.0


def compare_integration(replay, got, fields=("weights",) + INTEGRATED_FIELDS):
    """An integration or composition replay (float64) against the fields of the side under test: {field: (worst ratio to the
    tolerance, ok)}.  Beyond RTOL / ATOL the ``weights`` must keep the transmittance floor: behind a saturated sample the reference's
    ``1 - alpha + 1e-10`` leaves weights of 1e-10 alpha - far below ATOL, but never zero - so a sample with alpha > 1e-6 whose exact
    weight is above 1e-30 (fp32 holds it as a normal number) must have a POSITIVE weight, and 0 <= weights <= 1 everywhere."""
    rep = {k: field_mismatch(replay[k], got[k]) for k in fields}
    w = got["weights"].detach().cpu().double().reshape(replay["weights"].shape)
    must = (replay["alphas"].double() > 1e-6) & (replay["weights"].double() > 1e-30)
    rep["weights/floor"] = (float((must & ~(w > 0)).sum()), bool((w[must] > 0).all()))
    rep["weights/range"] = (float(w.max()) if w.numel() else 0.0, bool(((w >= 0) & (w <= 1)).all()))
    return rep


def _minecraft_hierarchical_config():
    """The ``minecraft_hierarchical`` reduced configuration of tests/test_gpu.py::CASES: overlap fix on, the skybox with 3 + 2
    positions (it ships with one, which the reference's resampler cannot handle)."""
    from playableenvironments_amd import configs
    return configs.reduced_config(configs.enable_fine(configs.minecraft_config()), width=256, layers=8, skip=4, features=192, octaves=10,
                                  bender_width=128, bender_layers=6, bender_skip=3, bender_octaves=6,
                                  positions={"background": (16, 16), "skybox": (3, 2), "player_1": (32, 32)})


def _density_case_table():
    from playableenvironments_amd import configs, synthetic
    return {
        # one-wave compositing and the resampler's rank merge
        "tennis_16_32": (lambda: configs.tennis_config(hierarchical=(16, 32)), lambda: synthetic.tennis_scene(seed=5), 16, 2.0, 1.0),
        # 768 merged entries per ray: the four-wave transmittance scan with its cross-wave carries.  Four times as many coarse
        # positions are four times shorter steps: an alpha only saturates (sigma dt > 17) with the densities ten times higher
        # (measured on the oracle: 0 % / 5 % / 0 % of the rays at 3e4, 69 % / 95 % / 22 % at 3e5)
        "tennis_64_128": (lambda: configs.tennis_config(hierarchical=(64, 128)), lambda: synthetic.tennis_scene(seed=1234), 8, 2.0, 10.0),
        # overlap fix, skybox, the masked t = 0 ties
        "minecraft_hierarchical": (_minecraft_hierarchical_config, lambda: synthetic.minecraft_scene(seed=6), 12, 3.0, 1.0),
    }


DENSITY_CASES = ("tennis_16_32", "tennis_64_128", "minecraft_hierarchical")
_density_biases = {}


def density_case(name, regime, precision="fp32"):
    """(cfg, composer on the CPU with the regime's densities, composer inputs, state dict) of one case x regime; the biases are
    measured once per case x regime and reused, so every composer of it carries identical weights."""
    from playableenvironments_amd import ObjectComposer, synthetic
    make_cfg, make_scene, n, alpha_bias, gain = _density_case_table()[name]
    cfg, scene = make_cfg(), make_scene()
    torch.manual_seed(0)
    comp = ObjectComposer(cfg)
    comp.precision = precision
    synthetic.randomize_module_state(comp, seed=0, step=20000, alpha_bias=alpha_bias, bender_scale=1e4)
    comp.eval()
    inputs = composer_inputs(cfg, scene, pixels=grid_pixels(scene["image_size"][0], scene["image_size"][1], n))
    scale, quantile = DENSITY_REGIMES[regime]
    _density_biases[name, regime] = shape_sigma(comp, scale * gain, quantile, cfg, inputs, biases=_density_biases.get((name, regime)))
    sd = {k: v.detach().cpu().clone() for k, v in comp.state_dict().items()}
    return cfg, comp, inputs, sd


def capture_oracle_stages(run_oracle):
    """Runs ``run_oracle()`` (a callable that runs ro.composer_forward) with ro.hierarchical_positions and ro.integrate wrapped:
    returns (its result, resampling calls, integration calls) - per call the arguments and what it returned, in call order
    (resampling: one per object; integration: per level the objects, then the global list)."""
    h0, i0 = ro.hierarchical_positions, ro.integrate
    resampled, integrated = [], []

    def hierarchical(origins, directions, count, ref_t, weights, perturb, rand=None):
        x, merged, used = h0(origins, directions, count, ref_t, weights, perturb, rand)
        resampled.append(dict(directions=directions, t=ref_t, weights=weights, merged=merged, used=used))
        return x, merged, used

    def integrate(features, raw, directions, t, displacements, divergences, perturb, noise=None):
        out, used = i0(features, raw, directions, t, displacements, divergences, perturb, noise)
        integrated.append(dict(features=features, raw=raw, directions=directions, t=t, displacements=displacements, out=out, used=used))
        return out, used

    ro.hierarchical_positions, ro.integrate = hierarchical, integrate
    try:
        result = run_oracle()
    finally:
        ro.hierarchical_positions, ro.integrate = h0, i0
    return result, resampled, integrated


# ---------------------------------------------------------------------------------------------------------------------
# Compositing backward on surface-like densities ("Compositing backward in the density regimes"): the
# per-sample gradients k_composite_bwd wrote (pr_sample_grads_t) against float64 autograd of the oracle's functions for that stage
GRADIENT_FIELDS = ("integrated_features", "opacity", "depth", "integrated_displacements_magnitude", "weights")
GRADIENT_TENSORS = ("sigma", "t", "displacement_magnitude", "features")


def stage_probes(cfg, flat, positions, seed, fields=GRADIENT_FIELDS, entries=None):
    """{entry: {field: probe}}: the random linear functional of one level (the suite's ``_probe_loss`` pattern) in the folded layout
    (N, R, ...); ``positions``: per object the length of its list; ``entries``: the entries the loss reads (default: all)."""
    g = torch.Generator().manual_seed(seed)
    N, R, K = flat["d"].size(0), flat["R"], flat["K"]
    F = _object_config(cfg, 0)["nerf_model"]["output_features"]
    out = {}
    for k in range(K + 1):
        name = f"object_{k}" if k < K else "global"
        P = positions[k] if k < K else sum(positions)
        shapes = {"integrated_features": (N, R, F), "weights": (N, R, P)}
        probes = {f: torch.randn(shapes.get(f, (N, R)), generator=g, dtype=torch.float32) for f in GRADIENT_FIELDS}       # (drawn whether read or not)
        if entries is None or name in entries:
            out[name] = {f: probes[f] for f in fields}
    return out


def replay_gradients(cfg, level, lists, slots, features, d_world, noise, probes):
    """Autograd (torch's default dtype: float64 under ``oracle_in_float64``) through replay_integration, replay_composition and
    expected_features - the oracle's functions of the compositing stage - of the loss
        sum over the entries and fields of ``probes`` of (probe * field).sum().
    Leaves: per object the depths ``t``, raw densities ``sigma`` (N, R, P), the displacement magnitudes |delta| and the raw feature
    rows ``features`` (N, R, P, F; masked with ``slots >= 0``, then the sigmoid of ``apply_activation``), and the ray direction norm
    |d| (N, R).  ``lists``: per object (t, sigma, delta or None); ``noise``: the recorded draws of a perturbed call or None
    (``int_<level>_<k>``, ``int_<level>_global``).

    |delta| as a variable: the lists carry (|delta| + 1, 0, 0) - torch.norm's subgradient at 0 is 0, the derivative with respect to
    the magnitude is w / n everywhere (a sample outside its box has delta = 0 and, with density noise, a weight); the weights are
    detached in that field, so the shift adds nothing to any gradient.

    Returns dict(objects=[{sigma, t, displacement_magnitude, features}], norm, masked): ``t`` and ``sigma`` summed over the object's
    own entry and the global entry, as the kernel accumulates them."""
    dt = torch.get_default_dtype()
    K = len(lists)
    leaf = lambda v: v.detach().to(dt).clone().requires_grad_(True)
    d_world = d_world.detach().to(dt)
    length = torch.linalg.norm(d_world, dim=-1)
    norm = leaf(length)
    directions = d_world / length.unsqueeze(-1) * norm.unsqueeze(-1)
    ts, sigmas, mags, feats, disps = [], [], [], [], []
    for k, (t, sigma, delta) in enumerate(lists):
        ts.append(leaf(t))
        sigmas.append(leaf(sigma))
        mags.append(leaf(torch.linalg.norm(delta.detach().to(dt), dim=-1) if delta is not None else torch.zeros(t.shape)))
        feats.append(leaf(features[k]))
        zero = torch.zeros_like(mags[k])
        disps.append(torch.stack([mags[k] + 1.0, zero, zero], dim=-1))
    key = lambda name: None if noise is None else noise[f"int_{level}_{name}"]
    own = [replay_integration(ts[k], sigmas[k], disps[k], directions, key(k)) for k in range(K)]
    comp = replay_composition(cfg, [(ts[k], sigmas[k], disps[k]) for k in range(K)], directions, key("global"))
    shown = [f * (slots[k] >= 0).unsqueeze(-1).to(dt) for k, f in enumerate(feats)]
    if cfg["model"]["apply_activation"]:
        shown = [torch.sigmoid(f) for f in shown]
    per_object, total = expected_features(shown, [o["weights"] for o in own], comp["weights"], comp["order"])
    loss = torch.zeros(())
    for name, fields in probes.items():
        entry = comp if name == "global" else own[int(name.split("_")[1])]
        for f, probe in fields.items():
            if f == "integrated_features":
                value = total if name == "global" else per_object[int(name.split("_")[1])]
            else:
                value = entry[f]
            loss = loss + (value * probe.to(dt).reshape(value.shape)).sum()
    leaves = ts + sigmas + mags + feats + [norm]
    if loss.requires_grad:
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    else:
        grads = [None] * len(leaves)
    grads = [torch.zeros_like(v) if g is None else g for g, v in zip(grads, leaves)]
    objects = [dict(t=grads[k], sigma=grads[K + k], displacement_magnitude=grads[2 * K + k], features=grads[3 * K + k]) for k in range(K)]
    return dict(objects=objects, norm=grads[4 * K], masked=comp["masked"], order=comp["order"])


GRADIENT_RTOL, GRADIENT_ATOL = 1e-4, 1e-5      # |got - want| <= RTOL |want| + ATOL max |want| (+ the cancellation term), per tensor
#: the one free constant of the cancellation term (gradient_mismatch): measured on the CPU only, never on the kernel
GRADIENT_C = 2.0


def gradient_mismatch(want, got, magnitude=None, c=GRADIENT_C):
    """(worst |got - want| / tolerance, ok) position by position; every value of ``got`` finite.  A tensor whose reference is zero
    everywhere must be zero everywhere.

    TOLERANCE (derived, not tuned):  1e-4 |want| + 1e-5 max |want| + c 2^-23 ``magnitude``.
    d alpha_j = dw_j T_j - (sum_{i>j} dw_i w_i) / (1 - alpha_j + 1e-10) is a difference: behind a dense sample both terms are small
    multiples of T_j and cancel to a fraction of themselves, and d t_j = gD w_j + dd_{j-1} - dd_j is a difference of neighbours.
    Each term is the end of a running product or sum over the n samples of the list, known in fp32 to n 2^-24 of itself at best,
    whatever the order of the scan - so a gradient is known to 2^-23 n (sum of the absolute values of its terms), which
    gradient_magnitudes forms in float64 from the inputs of the stage alone (``magnitude``; None: the first two terms only).  The
    first two terms - the issue's tolerance - do not cover it: measured on the CPU (tests/test_composite_backward_cpu.py prints both
    ratios), fp32 torch autograd of the oracle's function and the sequential restatement need 1.54 of them on tennis_64_128 /
    surfaces / perturb (coarse d sigma of object 2, a sample behind sigma dt = 12), each other's error to 3 digits.  ``c`` is the
    smallest power of two for which both stay inside the tolerance on every case x regime x {eval, perturb}: with c = 1 both
    need 1.05 on tennis_64_128 / sparse / perturb (fine d sigma of object 3; 19.5 of the first two terms alone), so c = 2.  The kernel is held to
    the same tolerance and is never used to choose c."""
    a, b = want.detach().cpu().double(), got.detach().cpu().double().reshape(want.shape)
    if not a.numel():
        return 0.0, True
    if not bool(torch.isfinite(b).all()):
        return float("inf"), False
    tol = GRADIENT_RTOL * a.abs() + GRADIENT_ATOL * a.abs().max()
    if magnitude is not None:
        tol = tol + c * FP32_EPS * magnitude.detach().cpu().double().reshape(want.shape)
    diff = (a - b).abs()
    ratio = torch.where(diff > 0, diff / tol, torch.zeros_like(diff))          # (x / 0 = inf for x > 0)
    worst = float(ratio.max())
    return worst, worst <= 1.0


def compare_gradients(want, got, bender, magnitudes=None, c=GRADIENT_C):
    """replay_gradients' result against the tensors of the side under test ({"sigma", "t", "displacement_magnitude", "features": per
    object, "norm"}): {"<tensor>/<object>": (worst ratio, ok)}; ``bender``: per object whether |delta| exists; ``magnitudes``:
    gradient_magnitudes of the same inputs (sigma, t and norm carry a cancellation term) or None."""
    rep = {}
    for k, obj in enumerate(want["objects"]):
        for name in GRADIENT_TENSORS:
            if name == "displacement_magnitude" and not bender[k]:
                continue
            m = magnitudes["objects"][k][name] if magnitudes is not None and name in ("sigma", "t") else None
            rep[f"{name}/{k}"] = gradient_mismatch(obj[name], got[name][k], m, c)
    rep["norm"] = gradient_mismatch(want["norm"], got["norm"], None if magnitudes is None else magnitudes["norm"], c)
    return rep


def gradient_magnitudes(cfg, level, lists, slots, features, d_world, noise, probes):
    """Per gradient of replay_gradients (sigma, t, norm): n times the sum of the absolute values of the terms it is a difference of,
    in float64 (sequential_composite_bwd_fp32 with ``magnitude=True``) - the cancellation term of gradient_mismatch."""
    return sequential_composite_bwd_fp32(cfg, level, lists, slots, features, d_world, noise, probes, magnitude=True)


def sequential_composite_bwd_fp32(cfg, level, lists, slots, features, d_world, noise, probes, mutation=None, magnitude=False):
    """numpy fp32 restatement of k_composite_bwd's ``entry_backward`` arithmetic over the entries of a level, one rounding per
    operation, every scan strictly sequential (the precedent: sequential_resampling_fp32): alpha_j = 1 - exp(-relu(raw) dt |d|),
    T_j = prod_{i<j} (1 - alpha_i + 1e-10), w_j = alpha_j T_j, dw_j = gF . f_j (skipped where T_j = 0 or the sample has no row)
    + gO + gD t_j + gW_j, d alpha_j = dw_j T_j - (sum_{i>j} dw_i w_i) / (1 - alpha_j + 1e-10), and from it d sigma, d t (both
    neighbours' spacings and gD w_j), d |delta| = gM w_j / n and d |d|.  The per-object entries run on the lists as exported, the
    global entry on the merged list behind the overlap fix, whose masked samples are constants.  Same arguments and result layout
    as replay_gradients (without d features: the kernel forms them from the weights the forward tests cover).

    ``mutation``: one of four wrong kernels the comparison must notice - "no_floor" (the quotient without its 1e-10),
    "no_carry" (the suffix sum restarts at every 64-entry block, counted from the front as the kernel's blocks are),
    "concatenation_order" (the global entry's gradients assigned by position in the merged list instead of through the order),
    ``magnitude=True`` (gradient_magnitudes): the same pass in float64 with every difference replaced by the sum of the absolute
    values of its terms, each entry's share times the length n of its list - what the cancelling terms of a gradient amount to.

    "masked_gradient" (the backward pass of the global entry forgets the overlap fix: the masked static samples keep their density
    and depth there and so receive gradient.  Dropping only the kernel's ``!mk`` guards changes nothing that can be seen: a masked
    sample's sigma = -10 and t = 0 leave alpha = 0 and d alpha / d t = 0 exactly, so whatever it would accumulate is zero)."""
    import numpy as np
    f = np.float64 if magnitude else np.float32
    K = len(lists)
    arr = lambda v: np.ascontiguousarray(v.detach().cpu().numpy(), dtype=f)
    mag = (lambda v: np.abs(v)) if magnitude else (lambda v: v)
    sign = f(-1.0) if magnitude else f(1.0)                # a - b becomes |a| + |b|
    d = arr(d_world).reshape(-1, 3)
    M = d.shape[0]
    norm = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f)).astype(f)
    counts = [int(t.size(-1)) for t, _, _ in lists]
    PT = sum(counts)
    tt = np.concatenate([arr(t).reshape(M, -1) for t, _, _ in lists], 1)
    sg = np.concatenate([arr(s).reshape(M, -1) for _, s, _ in lists], 1)
    sl = np.concatenate([s.detach().cpu().numpy().reshape(M, -1) for s in slots], 1)
    ff = np.concatenate([arr(v).reshape(M, c, -1) for v, c in zip(features, counts)], 1)
    if cfg["model"]["apply_activation"]:
        ff = np.where(sl[..., None] >= 0, ff, f(0.0))
        ff = (f(1.0) / (f(1.0) + np.exp(-ff))).astype(f)
        has_row = np.ones_like(sl, dtype=bool)
    else:
        has_row = sl >= 0
    gs, gt, gd = np.zeros((M, PT), f), np.zeros((M, PT), f), np.zeros((M, PT), f)
    mk = np.zeros((M, PT), bool)
    g_norm = np.zeros(M, f)
    rows = np.arange(M)[:, None]

    def entry(name, idx, n):
        with np.errstate(all="ignore"):            # (the "no_floor" mutation divides by zero: its NaNs are what the comparison sees)
            _entry(name, idx, n)

    def _entry(name, idx, n):
        nonlocal g_norm
        pr = probes.get(name, {})
        get = lambda field: arr(pr[field]).reshape(M, -1) if field in pr else None
        gO, gD, gM, gW, gF = (get(x) for x in ("opacity", "depth", "integrated_displacements_magnitude", "weights", "integrated_features"))
        gO, gD, gM = (np.zeros(M, f) if v is None else mag(v[:, 0]) for v in (gO, gD, gM))
        scale = f(n) if magnitude else f(1.0)
        t_e, raw = tt[rows, idx], sg[rows, idx].copy()
        nz = None if noise is None else noise.get(f"int_{level}_{name.replace('object_', '')}")
        if nz is not None:
            raw = (raw + arr(nz).reshape(M, n)).astype(f)
        dtv = np.concatenate([t_e[:, 1:] - t_e[:, :-1], np.full((M, 1), 1e10, f)], 1).astype(f)
        dist = (dtv * norm[:, None]).astype(f)
        s = np.maximum(raw, f(0.0))
        E = np.exp((-s * dist).astype(f)).astype(f)
        a = (f(1.0) - E).astype(f)
        T, w = np.empty((M, n), f), np.empty((M, n), f)
        run = np.ones(M, f)
        for j in range(n):
            T[:, j] = run
            w[:, j] = a[:, j] * run
            run = (run * ((f(1.0) - a[:, j]) + f(1e-10))).astype(f)
        if gF is None and gW is None and not gO.any() and not gD.any() and not gM.any():
            return
        dw = np.zeros((M, n), f)
        if gF is not None:
            dot = np.einsum("mf,mjf->mj", mag(gF), mag(ff[rows, idx])).astype(f)
            dw = np.where(has_row[rows, idx] & (T != 0), dot, f(0.0)).astype(f)
        dw = (dw + gO[:, None] + gD[:, None] * mag(t_e) + (mag(gW) if gW is not None else f(0.0))).astype(f)
        da = np.empty((M, n), f)
        suffix = np.zeros(M, f)
        with np.errstate(all="ignore"):
            for j in range(n - 1, -1, -1):
                if mutation == "no_carry" and j % 64 == 63:
                    suffix = np.zeros(M, f)
                den = (f(1.0) - a[:, j]) if mutation == "no_floor" else ((f(1.0) - a[:, j]) + f(1e-10))
                da[:, j] = dw[:, j] * T[:, j] - sign * suffix / den
                suffix = (suffix + dw[:, j] * w[:, j]).astype(f)
        inner = np.arange(n)[None, :] < n - 1
        dd = np.where(inner, da * s * E * norm[:, None], f(0.0)).astype(f)
        g_norm = (g_norm + scale * np.where(inner, da * s * E * dtv, f(0.0)).astype(f).sum(1, dtype=f)).astype(f)
        to = np.broadcast_to(np.arange(n)[None, :], (M, n)) if (mutation == "concatenation_order" and name == "global") else idx
        live = ~mk[rows, idx]
        before = np.concatenate([np.zeros((M, 1), f), dd[:, :-1]], 1)
        np.add.at(gs, (rows, to), scale * np.where(live & (raw > 0), da * dist * E, f(0.0)).astype(f))
        np.add.at(gt, (rows, to), scale * np.where(live, gD[:, None] * w + (before - sign * dd), f(0.0)).astype(f))
        np.add.at(gd, (rows, to), np.where(live, gM[:, None] * w / f(n), f(0.0)).astype(f))

    off = 0
    for k in range(K):
        entry(f"object_{k}", np.broadcast_to(off + np.arange(counts[k])[None, :], (M, counts[k])), counts[k])
        off += counts[k]
    layout = ro.ObjectLayout(cfg)
    if cfg["model"]["fix_object_overlaps"] and mutation != "masked_gradient":
        offs = np.concatenate([[0], np.cumsum(counts)])
        for sidx in range(layout.static_objects):
            ps = counts[sidx]
            ts_ = tt[:, offs[sidx]:offs[sidx] + ps].copy()
            hit = np.zeros((M, ps), bool)
            for dyn in range(layout.static_objects, K):
                b0, b1 = tt[:, offs[dyn]], tt[:, offs[dyn] + ps - 1]
                lo = (ts_ < b0[:, None]).sum(1)              # searchsorted(left) on a sorted list
                hi = (ts_ < b1[:, None]).sum(1)
                i = np.arange(ps)[None, :]
                hit |= (i >= lo[:, None]) & (i < hi[:, None])
            tt[:, offs[sidx]:offs[sidx] + ps][hit] = 0.0
            sg[:, offs[sidx]:offs[sidx] + ps][hit] = -10.0
            mk[:, offs[sidx]:offs[sidx] + ps][hit] = True
    order = np.argsort(tt, axis=1, kind="stable")
    entry("global", order, PT)
    out, off = [], 0
    for k in range(K):
        cut = lambda v: torch.from_numpy(v[:, off:off + counts[k]].copy()).reshape(lists[k][0].shape)
        out.append(dict(sigma=cut(gs), t=cut(gt), displacement_magnitude=cut(gd)))
        off += counts[k]
    return dict(objects=out, norm=torch.from_numpy(g_norm).reshape(lists[0][0].shape[:-1]))


def projection_tensor_formulation(pts, o2w, w2c, focals, height, width, boxes):
    """The package's tensor formulation of the projections - ``EnvironmentModel._project`` with the normalisation, reduction and clamps
    of ``compute_object_bounding_boxes`` / ``compute_object_axes_projection`` (``_lazy=True``, past the kernel route) - on the tensors it is
    given, on their device: ``pts`` (K, P, 3) - for the axes the same (4, 3) for every object -, ``o2w`` (F, K, 4, 4), ``w2c`` (F, C, 4, 4),
    ``focals`` (F, C).  Returns (points, boxes or None).  The methods run on a stand-in that holds just the hooks they read."""
    import types
    from playableenvironments_amd.environment_model import EnvironmentModel
    stub = types.SimpleNamespace(_no_graph=lambda *tensors: False, _edge_points=lambda device: pts, _project=EnvironmentModel._project,
                                 _pixel_cache={}, _axes_point_cache={str(o2w.device): pts[0]},
                                 object_id_helper=types.SimpleNamespace(objects_count=pts.shape[0]))
    stub._image_scale = lambda w, h, like: EnvironmentModel._image_scale(stub, w, h, like)
    o2w = o2w.permute(0, 2, 3, 1)
    if boxes:
        got_boxes, got_points = EnvironmentModel.compute_object_bounding_boxes(stub, o2w, w2c, focals, height, width, _lazy=True)
        return got_points, got_boxes
    return EnvironmentModel.compute_object_axes_projection(stub, o2w, w2c, focals, height, width, _lazy=True), None
