"""Fine guide: the fine pass evaluates a merged sample only where the coarse pass found density (``pr_render_forward_guided``).

Hierarchical sampling already holds a per-ray, per-frame estimate of where an object has matter: the coarse densities.  With
``composer.fine_guide = FineGuide()`` a merged (coarse + resampled) sample of the fine pass is sent through the fine model only
when a coarse sample next to it has a density above ``threshold``; every other sample is treated exactly like a sample outside the
object's box.  No grid, no build, no extra query; it follows every pose and deformation code and works for static and dynamic
objects alike.  It is an approximation for evaluation renders and only as good as the coarse model's agreement with the fine one.

>>> composer.fine_guide = FineGuide()                  # threshold 0.0, guard 1, every object with a fine model but the skybox
>>> frame = composer(*inputs, False)                   # the fine pass evaluates fewer samples
>>> composer.fine_guide = None                         # today's render, bit for bit
"""
from __future__ import annotations

import itertools
import math
from typing import Optional, Sequence, Tuple

import torch

_SERIAL = itertools.count(1)


def keep_mask(t_coarse: torch.Tensor, sigma_coarse: torch.Tensor, t_merged: torch.Tensor, threshold: float, guard: int) -> torch.Tensor:
    """The guide's predicate in torch, bit for bit what the resampling kernel decides.  ``t_coarse`` / ``sigma_coarse`` (..., Pc):
    the coarse depths and the raw coarse densities as the resampler reads them (``empty_space_alpha`` for an object that is absent
    from the frame); ``t_merged`` (..., Pm): the depths of the fine pass.  Coarse sample i is live iff ``sigma_coarse[i] >
    threshold``; a merged sample at depth t has ``j = max(0, #{i : t_coarse[i] <= t} - 1)`` and is kept iff some i in
    ``[j - guard, j + 1 + guard]``, clipped to the ray, is live.  Returns a bool tensor (..., Pm).  The box test and the occupancy
    bit are not part of it."""
    guard = int(guard)
    if guard < 0:
        raise ValueError(f"guard must be >= 0, got {guard}")
    Pc = t_coarse.size(-1)
    live = sigma_coarse > threshold
    # near[j]: any live sample in [j - guard, j + 1 + guard] - differences of the running count of live samples
    count = torch.cat([torch.zeros_like(live[..., :1], dtype=torch.int64), live.to(torch.int64).cumsum(-1)], dim=-1)      # (..., Pc + 1)
    j_all = torch.arange(Pc, device=t_coarse.device)
    first = (j_all - guard).clamp(min=0)
    last = (j_all + 1 + guard).clamp(max=Pc - 1)
    near = (count[..., last + 1] - count[..., first]) > 0                                                                # (..., Pc)
    # comparisons only (the count, not a search: the definition also where the depths do not ascend)
    below = (t_coarse.unsqueeze(-2) <= t_merged.unsqueeze(-1)).sum(-1)                                                  # (..., Pm)
    j = (below - 1).clamp(min=0)
    return torch.gather(near, -1, j)


class FineGuide:
    """Parameters of the fine guide of a composer.  ``threshold``: a coarse sample is live iff its raw density is above it (0.0: a
    density <= 0 has alpha exactly 0); ``guard``: how many coarse samples the live window extends to either side; ``objects``: the
    guided object instances, ``None`` = every object that has a fine model and is not a skybox.  The attributes may be changed in
    place: recorded frames key on their values."""

    def __init__(self, threshold: float = 0.0, guard: int = 1, objects: Optional[Sequence[int]] = None):
        self.serial = next(_SERIAL)          # identity in the signatures of recorded frames
        self.threshold = threshold
        self.guard = guard
        self.objects = objects
        self.check()

    def check(self) -> None:
        if isinstance(self.guard, bool) or int(self.guard) != self.guard or int(self.guard) < 0:
            raise ValueError(f"FineGuide.guard must be an integer >= 0, got {self.guard!r}")
        if math.isnan(float(self.threshold)):
            raise ValueError("FineGuide.threshold is NaN")
        if self.objects is not None:
            ids = [int(k) for k in self.objects]
            if not ids or min(ids) < 0:
                raise ValueError(f"FineGuide.objects must name at least one object instance (or be None), got {self.objects!r}")

    def object_ids(self, eligible: Sequence[int], count: int) -> Tuple[int, ...]:
        """The guided objects of a call with ``count`` objects of which ``eligible`` can be guided."""
        if self.objects is None:
            return tuple(eligible)
        ids = sorted({int(k) for k in self.objects})
        for k in ids:
            if not 0 <= k < count:
                raise ValueError(f"FineGuide.objects: object {k} out of range 0..{count - 1}")
            if k not in eligible:
                raise ValueError(f"FineGuide.objects: object {k} has no fine model to guide or is a skybox")
        return tuple(ids)

    def signature(self):
        return (self.serial, float(self.threshold), int(self.guard), None if self.objects is None else tuple(int(k) for k in self.objects))
