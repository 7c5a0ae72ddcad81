"""Torch restatements of the two extra outputs of a geometry-only render (``pr_render_geometry``, include/playrender.h):
the per-object visibility under occlusion and the front object of a ray.  Plain tensor code on any device - what the tests and the
reports compare the compositing kernel's results with."""
from __future__ import annotations

from typing import Sequence

import torch


def visibility_from_weights(global_weights: torch.Tensor, order: torch.Tensor, positions: Sequence[int]) -> torch.Tensor:
    """(..., R, K) per-object alpha mattes from the weights of the merged list.

    global_weights (..., R, sum P_k): the global entry's weights, in merged (sorted) order; order (..., R, sum P_k) integer: the
    concatenation index of every merged rank (objects concatenated in object order, object k owning ``positions[k]`` consecutive
    indices); positions: P_k per object.  visibility[..., k] is the sum of the weights of the ranks that belong to object k
    (scatter-add by the object of each rank): a sample the overlap fix masked stays with its object, with the weight 0 it has."""
    positions = [int(p) for p in positions]
    total = sum(positions)
    if global_weights.shape != order.shape or global_weights.size(-1) != total:
        raise ValueError(f"weights {tuple(global_weights.shape)} / order {tuple(order.shape)} do not describe {total} merged entries")
    ends = torch.cumsum(torch.tensor(positions, dtype=torch.long, device=order.device), 0)
    owner = torch.bucketize(order.long(), ends, right=True)           # entry e belongs to the first object whose end is > e
    out = torch.zeros(list(global_weights.shape[:-1]) + [len(positions)], dtype=global_weights.dtype, device=global_weights.device)
    return out.scatter_add_(-1, owner, global_weights)


def front_object(visibility: torch.Tensor) -> torch.Tensor:
    """(..., R) int32: the lowest object index whose visibility (..., R, K) is the ray's maximum, -1 where no visibility is greater than
    zero.  A NaN visibility counts as not greater than anything: it is never the front object."""
    clean = torch.where(torch.isnan(visibility), torch.full_like(visibility, float("-inf")), visibility)
    best = clean.amax(-1, keepdim=True)
    K = visibility.size(-1)
    index = torch.arange(K, device=visibility.device).expand(visibility.shape)
    lowest = torch.where(clean == best, index, torch.full_like(index, K)).amin(-1)      # (ties: the lowest index)
    return torch.where(best.squeeze(-1) > 0, lowest, torch.full_like(lowest, -1)).to(torch.int32)
