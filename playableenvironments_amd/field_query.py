"""Point queries of the object fields (``pr_query_field``, include/playrender.h): density, style-modulated feature and ray-bender
displacement of ONE object model at explicit object-frame positions - what the reference's ``RayBendingStyleNerfModel.forward``
computes (model/nerf_models/ray_bending_style_nerf_model.py:137-219), in evaluation mode, on the renderer's own fused MLP kernel.

Two callers share this module: ``ObjectComposer.query_object`` / ``density_grid`` (the composer's precision, cached model structs and
packed weights) and ``modules.RayBendingStyleNerfModel.forward`` (no composer: struct and fp32 packing made per call).

Out of scope: gradients of a query, train-mode BatchNorm statistics, ``forward`` of the inner ``nerf_model`` / ``ray_bender`` modules
on their own, world-frame positions (the caller applies ``w2o``).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, Optional, Sequence

import torch

from . import _lib

NO_CPU = "the HIP renderer needs device tensors (there is no CPU fallback)"


def linear_struct(layer) -> _lib.Linear:
    s = _lib.Linear()
    if layer is not None:
        s.weight = layer.weight.data_ptr()
        s.bias = layer.bias.data_ptr() if layer.bias is not None else None
        s.out_features, s.in_features = layer.weight.shape
    return s


def build_model_struct(model, positions: int, octave_weights: Optional[Sequence[float]] = None) -> _lib.ObjectModel:
    """``pr_object_model_t`` of a ``RayBendingStyleNerfModel``: raw parameter / buffer pointers, shapes, the bender's octave weights.
    ``octave_weights``: host copy of ``positional_encoder.annealing_weights()``; ``None`` reads them back here (a device
    synchronisation - the composer keeps a cached copy instead)."""
    cfg = model.model_config
    nerf, bender = model.nerf_model, model.ray_bender
    s = _lib.ObjectModel()
    s.kind = nerf.kind
    s.has_bender = 1 if bender.has_weights else 0
    s.positions = positions
    s.style_features = cfg["style_features"]
    s.deformation_features = cfg["deformation_features"]
    s.output_features = nerf.output_features
    s.layers_width = nerf.layers_width
    s.backbone_count = nerf.backbone_layers_count
    s.skip_layer_idx = nerf.skip_layer_idx
    s.octaves = nerf.octaves
    box = [float(v) for row in cfg["bounding_box"] for v in row]
    for i in range(6):
        s.bbox[i] = box[i]
    s.empty_space_alpha = float(cfg["empty_space_alpha"])
    s.z_near_min = float(cfg["z_near_min"])
    s.z_far_max = float(cfg["z_far_max"])
    head = nerf.features_head
    s.bn_eps = float(head[1].ada_in.normalization.eps)
    for i, layer in enumerate(nerf.backbone_layers):
        s.backbone[i] = linear_struct(layer)
    s.alpha_head = linear_struct(nerf.alpha_head if nerf.kind == 0 else None)
    s.head0 = linear_struct(head[0])
    s.affine1 = linear_struct(head[1].affine_transform)
    s.bn1_mean = head[1].ada_in.normalization.running_mean.data_ptr()
    s.bn1_var = head[1].ada_in.normalization.running_var.data_ptr()
    s.bn1_batches = head[1].ada_in.normalization.num_batches_tracked.data_ptr()
    s.head3 = linear_struct(head[3])
    s.affine4 = linear_struct(head[4].affine_transform)
    s.bn4_mean = head[4].ada_in.normalization.running_mean.data_ptr()
    s.bn4_var = head[4].ada_in.normalization.running_var.data_ptr()
    s.bn4_batches = head[4].ada_in.normalization.num_batches_tracked.data_ptr()
    s.head6 = linear_struct(head[6])
    if bender.has_weights:
        s.bender_width = bender.layers_width
        s.bender_count = bender.layers_count
        s.bender_skip = bender.skip_layer_idx
        s.bender_octaves = bender.positional_encoder.octaves_count
        if octave_weights is None:
            octave_weights = bender.positional_encoder.annealing_weights().detach().cpu().tolist()
        for i, v in enumerate(octave_weights):
            s.bender_octave_weights[i] = v
        for i, layer in enumerate(bender.backbone_layers):
            s.bender[i] = linear_struct(layer)
        s.bender_out = linear_struct(bender.output_head)
    return s


def fold_query_shapes(positions_shape: Sequence[int], style_shape: Sequence[int], deformation_shape: Sequence[int]) -> Dict:
    """How the tensors of ``RayBendingStyleNerfModel.forward`` become the (G groups, M points) of a query.  Pure shape arithmetic.

    ``positions (..., P, 3)``; ``style (..., S)`` / ``deformation (..., D)`` with the leading dimensions of the positions WITHOUT the
    ``P`` axis, each of size 1 (broadcast: the reference's ``expand_latent_code``) or of full size.  The trailing leading
    dimensions on which BOTH codes have size 1 are folded into M together with P - the composer's ``(N, R, P, 3)`` positions with
    ``(N, 1, S)`` codes are G = N groups of M = R x P points, not N x R groups (one AdaIN table row per group).  Where a code has size
    1 in front of a dimension that is not folded (any other broadcast pattern) it is expanded: ``code_shape`` is the shape both codes
    are broadcast to before they are flattened to ``(G, .)``.

    Returns ``{"lead": [...], "split": j, "groups": G, "points": M, "code_shape": lead[:j]}`` with ``lead`` = positions_shape[:-1]."""
    positions_shape, style_shape, deformation_shape = list(positions_shape), list(style_shape), list(deformation_shape)
    if len(positions_shape) < 2 or positions_shape[-1] != 3:
        raise ValueError(f"ray_positions must be (..., positions_count, 3), got {positions_shape}")
    lead = positions_shape[:-1]                    # (..., P)
    outer = lead[:-1]
    codes = []
    for name, shape in (("style", style_shape), ("deformation", deformation_shape)):
        if len(shape) < 1 or len(shape) - 1 > len(outer):
            raise ValueError(f"{name} {shape} has more leading dimensions than ray_positions {positions_shape}")
        dims = [1] * (len(outer) - (len(shape) - 1)) + shape[:-1]
        for c, full in zip(dims, outer):
            if c != 1 and c != full:
                raise ValueError(f"{name} {shape}: leading dimension {c} is neither 1 nor {full} (ray_positions {positions_shape})")
        codes.append(dims)
    merged = [max(a, b) for a, b in zip(*codes)]
    split = len(outer)
    while split > 0 and merged[split - 1] == 1:
        split -= 1
    return {"lead": lead, "split": split, "groups": int(math.prod(lead[:split])), "points": int(math.prod(lead[split:])),
            "code_shape": lead[:split]}


def default_budget(dev, need: int) -> int:
    """Scratch bytes a composer-less query may use: 80 % of what the device can still provide (asked only for large queries)."""
    if need <= (256 << 20) or torch.cuda.is_current_stream_capturing():
        return max(need, 256 << 20)
    free, _ = torch.cuda.mem_get_info(dev)
    cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    return max(1 << 20, int(0.8 * (free + cached)))


def require_queryable(module, tensors, parameters) -> None:
    """The checks both entry points share: evaluation mode, device tensors, no silently detached result."""
    if module.training:
        raise RuntimeError("point queries run in evaluation mode (the running BatchNorm statistics): call .eval() first - train-mode "
                           "batch statistics over an arbitrary point set are not supported")
    if not tensors[0].is_cuda:
        raise RuntimeError(NO_CPU)
    if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors) or any(p.requires_grad for p in parameters)):
        raise RuntimeError("point queries are not differentiable: call them under torch.no_grad() (an input or a parameter requires "
                           "grad and the result would be silently detached)")


def run_query(struct: _lib.ObjectModel, packed: torch.Tensor, precision: int, positions: torch.Tensor, style: torch.Tensor,
              deformation: torch.Tensor, ray_origins: Optional[torch.Tensor], ray_directions: Optional[torch.Tensor], *,
              canonical_pose: bool, features: bool, return_slot: bool, budget_of: Callable[[int], int],
              workspace_of: Callable[[int], torch.Tensor]) -> Dict[str, torch.Tensor]:
    """One query on prepared tensors: ``positions (G,M,3)``, ``style (G,S)``, ``deformation (G,D)``, skybox: ``ray_origins (G,3)``,
    ``ray_directions (G,M,3)`` - fp32, contiguous, on the current device.  Enqueues on the current stream; outputs are
    ``torch.empty`` tensors every element of which the kernels write.  A query whose workspace exceeds ``budget_of(bytes)`` (or with
    G x M >= 2^31) is split along M, group by group; the pieces write into views of the same output tensors, ``evaluated`` is their
    sum and ``slot`` then counts rows per piece."""
    lib = _lib.load()
    dev = positions.device
    G, M = positions.shape[0], positions.shape[1]
    F = struct.output_features
    stream = torch.cuda.current_stream(dev).cuda_stream
    out: Dict[str, torch.Tensor] = {}
    if features:
        out["features"] = torch.empty((G, M, F), dtype=torch.float32, device=dev)
    out["sigma"] = torch.empty((G, M), dtype=torch.float32, device=dev)
    out["displacements"] = torch.empty((G, M, 3), dtype=torch.float32, device=dev)
    if return_slot:
        out["slot"] = torch.empty((G, M), dtype=torch.int32, device=dev)
    if G * M == 0:
        out["evaluated"] = torch.zeros(2, dtype=torch.int32, device=dev)
        return out

    def make(g0: int, g1: int, m0: int, m1: int, counters: torch.Tensor) -> _lib.Query:
        whole = m0 == 0 and m1 == M
        cut = (lambda t: t[g0:g1]) if whole else (lambda t: t[g0, m0:m1])      # (a piece of ONE group is contiguous)
        q = _lib.Query()
        q.groups, q.points = g1 - g0, m1 - m0
        q.flags = _lib.PR_FLAG_CANONICAL_POSE if canonical_pose else 0
        q.precision = precision
        q.positions = cut(positions).data_ptr()
        if ray_origins is not None:
            q.ray_origins = ray_origins[g0:g1].data_ptr()
        if ray_directions is not None:
            q.ray_directions = cut(ray_directions).data_ptr()
        q.style = style[g0:g1].data_ptr()
        q.deformation = deformation[g0:g1].data_ptr()
        q.features = cut(out["features"]).data_ptr() if features else None
        q.sigma = cut(out["sigma"]).data_ptr()
        q.displacement = cut(out["displacements"]).data_ptr()
        q.slot = cut(out["slot"]).data_ptr() if return_slot else None
        q.counters = counters.data_ptr()
        return q

    def size_of(q: _lib.Query) -> int:
        size = C.c_size_t()
        _lib.check(lib.pr_query_workspace_size(C.byref(q), C.byref(struct), C.byref(size)), "pr_query_workspace_size")
        return size.value

    def launch(q: _lib.Query) -> None:
        need = size_of(q)
        ws = workspace_of(need)
        _lib.check(lib.pr_query_field(C.byref(q), C.byref(struct), packed.data_ptr(), ws.data_ptr(), need, stream), "pr_query_field")

    if G * M < 2 ** 31:
        counters = torch.empty(2, dtype=torch.int32, device=dev)
        q = make(0, G, 0, M, counters)
        need = size_of(q)
        if need <= budget_of(need):
            launch(q)
            out["evaluated"] = counters
            return out
    # split along M, group by group (the pieces of one group are contiguous views of the (G, M, .) tensors)
    dummy = torch.empty(2, dtype=torch.int32, device=dev)
    chunk = min(M, 2 ** 31 - 1)
    need = size_of(make(0, 1, 0, chunk, dummy))
    budget = budget_of(need)
    if need > budget:
        chunk = max(1, int(chunk * budget / need))
        while chunk > 1 and size_of(make(0, 1, 0, chunk, dummy)) > budget:
            chunk = max(1, int(chunk * 0.8))
    pieces = [(g, m0, min(M, m0 + chunk)) for g in range(G) for m0 in range(0, M, chunk)]
    counters = torch.empty((len(pieces), 2), dtype=torch.int32, device=dev)
    for i, (g, m0, m1) in enumerate(pieces):
        launch(make(g, g + 1, m0, m1, counters[i]))
    out["evaluated"] = counters.sum(0, dtype=torch.int32)
    return out


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32)


def module_forward(model, ray_positions, ray_origins, ray_directions, style, deformation, canonical_pose: bool = False):
    """``RayBendingStyleNerfModel.forward`` of the reference on the HIP path (see ``fold_query_shapes`` for the shapes).  No composer:
    the model struct is built and the weights are packed (``pr_pack_model``, fp32) on every call - correct by construction, at the
    price of a ~2.9 MB pass and, for models with a ray bender, one small read-back of the annealing weights."""
    require_queryable(model, (ray_positions, ray_origins, ray_directions, style, deformation), list(model.parameters()))
    with torch.cuda.device(ray_positions.device):
        fold = fold_query_shapes(ray_positions.shape, style.shape, deformation.shape)
        lead, split, G, M = fold["lead"], fold["split"], fold["groups"], fold["points"]
        S, D = style.shape[-1], deformation.shape[-1]
        if S != model.style_features or D != model.deformation_features:
            raise ValueError(f"style / deformation carry {S} / {D} features, the model expects {model.style_features} / "
                             f"{model.deformation_features}")
        dev = ray_positions.device
        pos = _f32(ray_positions).reshape(G, M, 3).contiguous()
        outer = lead[:-1]

        def code(t, width):
            t = _f32(t)
            t = t.reshape([1] * (len(outer) - (t.dim() - 1)) + list(t.shape))
            t = t[(Ellipsis,) + (0,) * (len(outer) - split) + (slice(None),)]          # the folded dimensions (size 1 on both codes)
            return t.expand(fold["code_shape"] + [width]).reshape(G, width).contiguous()

        sty, dfm = code(style, S), code(deformation, D)
        org = dirs = None
        if model.nerf_model.kind == 1:
            o = _f32(ray_origins)
            o = o.reshape([1] * (len(outer) - (o.dim() - 1)) + list(o.shape))
            varies = any(n != 1 for n in o.shape[split:-1])
            ob = o.expand(outer + [3]).reshape(G, -1, 3)
            if varies and not bool((ob == ob[:, :1]).all()):
                raise ValueError("skybox queries take ONE ray origin per group (per camera): ray_origins vary inside a group of points "
                                 "that share a style / deformation code")
            org = ob[:, 0].contiguous()
            d = _f32(ray_directions)
            dirs = d.expand(outer + [3]).unsqueeze(-2).expand(lead + [3]).reshape(G, M, 3).contiguous()
        struct = build_model_struct(model, 1)
        lib = _lib.load()
        stream = torch.cuda.current_stream(dev).cuda_stream
        size = C.c_size_t()
        _lib.check(lib.pr_packed_size(C.byref(struct), C.byref(size)), "pr_packed_size")
        packed = torch.empty(size.value, dtype=torch.uint8, device=dev)
        _lib.check(lib.pr_pack_model(C.byref(struct), _lib.PR_PRECISION_FP32, packed.data_ptr(), size.value, stream), "pr_pack_model")
        res = run_query(struct, packed, _lib.PR_PRECISION_FP32, pos, sty, dfm, org, dirs, canonical_pose=bool(canonical_pose),
                        features=True, return_slot=False, budget_of=lambda need: default_budget(dev, need),
                        workspace_of=lambda need: torch.empty(need, dtype=torch.uint8, device=dev))
        F = struct.output_features
        return (res["features"].reshape(lead + [F]), res["sigma"].reshape(lead), res["displacements"].reshape(lead + [3]), {})
