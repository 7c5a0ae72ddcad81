"""Occupancy grids: empty-space skipping for evaluation renders (``pr_render_forward_culled`` / ``pr_occupancy_build``,
include/playrender.h).

A grid divides the bounding box of an object's model into ``nx x ny x nz`` cells and holds one bit per cell and frame.  A sample
whose cell bit is 0 is treated exactly like a sample outside the box: it never reaches the MLP and composites as
``(feature 0, sigma = empty_space_alpha, displacement 0)`` - with the negative ``empty_space_alpha`` of every shipped configuration
its alpha is exactly 0.  ``cell_index`` restates the kernels' lookup in torch (CPU tensors work); ``Occupancy`` owns the bit
tensors a composer renders with (``ObjectComposer.occupancy``, built by ``ObjectComposer.build_occupancy`` or
``ObjectComposer.occupancy_from_mask``).  Evaluation only: perturbed, training and differentiable calls and
``forward_expected_positions`` never see the grid.
"""
from __future__ import annotations

import ctypes as C
import itertools
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib, surface

LEVELS = ("coarse", "fine")
_SERIAL = itertools.count(1)


def _cells_of(cells) -> Tuple[int, int, int]:
    n = (int(cells),) * 3 if isinstance(cells, int) else tuple(int(v) for v in cells)
    if len(n) != 3 or min(n) < 1:
        raise ValueError(f"cells must be a positive integer or three of them, got {cells!r}")
    return n


def cell_scale(bounding_box, cells) -> torch.Tensor:
    """``s_a = float32(n_a) / (hi_a - lo_a)``: what the library computes on the host from ``pr_object_model_t.bbox`` (fp32)."""
    box = torch.as_tensor(bounding_box, dtype=torch.float32).reshape(3, 2).cpu()
    if bool((box[:, 1] <= box[:, 0]).any()):
        raise ValueError(f"the bounding box {box.tolist()} has an empty axis (hi <= lo): it cannot carry an occupancy grid")
    return torch.tensor(_cells_of(cells), dtype=torch.float32) / (box[:, 1] - box[:, 0])


def cell_index(positions: torch.Tensor, bounding_box, cells) -> torch.Tensor:
    """Flat cell of object-frame ``positions (..., 3)`` in a grid of ``cells`` = n or (nx, ny, nz) over ``bounding_box``
    ((3, 2): [lo, hi] per axis) - the lookup of the renderer's kept-sample predicate, in fp32 with separate round-to-nearest
    operations: ``u_a = (x_a - lo_a) * s_a``, ``c_a = min(n_a - 1, trunc(u_a))``, ``cell = (c_x * ny + c_y) * nz + c_z``; bit
    ``cell & 31`` of word ``cell >> 5``.  Positions on ``lo`` map to cell 0 of the axis, positions on ``hi`` to cell ``n - 1``.
    Only positions inside the box mean anything; those outside are clamped to the nearest cell so that the result can always
    index a mask.  int64, on the device of ``positions``."""
    n = _cells_of(cells)
    dev = positions.device
    box = torch.as_tensor(bounding_box, dtype=torch.float32).reshape(3, 2).cpu()
    lo = box[:, 0].to(dev)
    scale = cell_scale(box, n).to(dev)
    u = (positions.to(torch.float32) - lo) * scale
    top = torch.tensor([v - 1 for v in n], dtype=torch.int64, device=dev)
    c = torch.minimum(torch.nan_to_num(u, nan=0.0, posinf=3.0e9, neginf=-3.0e9).to(torch.int64), top).clamp_(min=0)
    return (c[..., 0] * n[1] + c[..., 1]) * n[2] + c[..., 2]


def words_of(cells) -> int:
    n = _cells_of(cells)
    return (n[0] * n[1] * n[2] + 31) // 32


def pack_bits(mask: torch.Tensor) -> torch.Tensor:
    """``mask (N, nx, ny, nz)`` bool -> ``(N, words)`` int32 words holding the cells little-endian (cell c = bit ``c & 31`` of word
    ``c >> 5``, tail bits 0): the layout ``pr_occupancy_build`` writes.  The int32 tensor carries the uint32 bit patterns."""
    if mask.dim() != 4:
        raise ValueError(f"an occupancy mask is (N, nx, ny, nz), got {list(mask.shape)}")
    N = mask.size(0)
    flat = mask.reshape(N, -1).to(torch.int64)
    words = (flat.size(1) + 31) // 32
    padded = torch.zeros((N, words * 32), dtype=torch.int64, device=mask.device)
    padded[:, :flat.size(1)] = flat
    weights = torch.ones(32, dtype=torch.int64, device=mask.device) << torch.arange(32, dtype=torch.int64, device=mask.device)
    value = (padded.reshape(N, words, 32) * weights).sum(-1)
    value = torch.where(value >= 2 ** 31, value - 2 ** 32, value)
    return value.to(torch.int32).contiguous()


def unpack_bits(bits: torch.Tensor, cells) -> torch.Tensor:
    """Inverse of ``pack_bits``: ``(N, words)`` int32 -> bool ``(N, nx, ny, nz)``."""
    n = _cells_of(cells)
    shifts = torch.arange(32, dtype=torch.int64, device=bits.device)
    flat = ((bits.to(torch.int64).unsqueeze(-1) >> shifts) & 1).reshape(bits.size(0), -1)[:, :n[0] * n[1] * n[2]]
    return flat.to(torch.bool).reshape(bits.size(0), *n)


class Occupancy:
    """The occupancy bits of a composer's objects: ``grids[(object_idx, level)] = {"bits": int32 (N, words), "cells": (nx, ny,
    nz)}`` for ``level`` in ("coarse", "fine").  The bit tensors keep their storage for the life of the object (``update`` writes
    in place), so that recorded frames - which bake the pointers in - see new bits.

    ``follow``: ``True`` makes every evaluation render of the composer call ``update`` with the call's own style / deformation codes
    first - correct by construction for animated objects, at the price of one build per call.  Grids made from masks cannot be
    updated."""

    def __init__(self, composer, frames: int, grids: Dict, build: Optional[dict] = None):
        self._composer = composer
        self.frames = int(frames)
        self.grids = grids
        self.build = build            # resolution / supersample / threshold / dilate / canonical_pose / keep_largest / min_points, or None (from masks)
        self.follow = False
        self.serial = next(_SERIAL)   # identity of the grid in the signatures of recorded frames
        self._centres: Dict = {}

    def signature(self):
        return (self.serial, bool(self.follow))

    # ------------------------------------------------------------------ what a renderer call is handed
    def call_struct(self, frames: int, object_ids: Sequence[int], use_fine: bool, device=None) -> _lib.Occupancy:
        """``pr_occupancy_t`` of a call with ``frames`` frames over the object instances ``object_ids``."""
        if int(frames) != self.frames:
            raise ValueError(f"the occupancy grid holds {self.frames} frame(s), the call renders {int(frames)}: build the grid for the "
                             "frames of the call")
        s = _lib.Occupancy()
        for j, k in enumerate(object_ids):
            for level in LEVELS[:2 if use_fine else 1]:
                g = self.grids.get((k, level))
                if g is None:
                    continue
                bits = g["bits"]
                if device is not None and bits.device != torch.device(device):
                    raise ValueError(f"the occupancy bits of object {k} live on {bits.device}, the call runs on {device}")
                entry = getattr(s, level)[j]
                entry.bits = bits.data_ptr()
                for a in range(3):
                    entry.cells[a] = g["cells"][a]
                entry.words = bits.size(1)
        return s

    def mask(self, object_idx: int, level: str = "coarse") -> torch.Tensor:
        """The bits of one grid as a bool tensor ``(N, nx, ny, nz)`` (a copy)."""
        g = self.grids[(object_idx, level)]
        return unpack_bits(g["bits"], g["cells"])

    # ------------------------------------------------------------------ (re)building from the density field
    def update(self, style: torch.Tensor, deformation: torch.Tensor, canonical_pose: Optional[bool] = None) -> "Occupancy":
        """Rewrites the bits in place for new codes - ``style (..., S, K)`` / ``deformation (..., D, K)`` in ``forward``'s layout.
        Stream-ordered, no host synchronisation."""
        S, D = style.size(-2), deformation.size(-2)
        K = style.size(-1)
        sty = style.detach().to(torch.float32).reshape(-1, S, K).permute(0, 2, 1)
        dfm = torch.broadcast_to(deformation.detach().to(torch.float32), list(style.shape[:-2]) + [D, K]).reshape(-1, D, K).permute(0, 2, 1)
        return self.update_prepared(sty, dfm, canonical_pose)

    def update_prepared(self, style_nks: torch.Tensor, deformation_nkd: torch.Tensor, canonical_pose: Optional[bool] = None) -> "Occupancy":
        """``update`` for codes in the renderer's layouts: ``style (N, K, S)`` / ``deformation (N, K, D)``."""
        if self.build is None:
            raise RuntimeError("this occupancy grid was made from masks (occupancy_from_mask): it has no density field to follow")
        if style_nks.size(0) != self.frames:
            raise ValueError(f"the occupancy grid holds {self.frames} frame(s), the codes describe {style_nks.size(0)}")
        composer = self._composer
        lib = _lib.load()
        b = self.build
        canonical = b["canonical_pose"] if canonical_pose is None else bool(canonical_pose)
        with torch.no_grad():
            for (k, level), g in self.grids.items():
                dev = g["bits"].device
                n = [c * b["supersample"] for c in g["cells"]]
                centres = self._centres.get((k, level))
                if centres is None:
                    centres = self._centres[(k, level)] = composer._grid_centres(k, n, level == "fine", dev).reshape(1, -1, 3)
                with torch.cuda.device(dev):
                    sigma = composer.query_object(k, centres.expand(self.frames, -1, 3), style_nks[:, k], deformation_nkd[:, k],
                                                  fine=level == "fine", canonical_pose=canonical, features=False)["sigma"]
                    if b.get("keep_largest", 0) or b.get("min_points", 0):          # floaters leave the lattice before the bits are made
                        sigma, _ = surface.clean_lattice(sigma.reshape([self.frames] + n), float(b["threshold"]),
                                                         keep_largest=b.get("keep_largest", 0), min_points=b.get("min_points", 0))
                    cells = (C.c_int32 * 3)(*g["cells"])
                    _lib.check(lib.pr_occupancy_build(sigma.data_ptr(), self.frames, cells, b["supersample"], float(b["threshold"]),
                                                      int(b["dilate"]), g["bits"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                               "pr_occupancy_build")
        return self

    def kept_fraction(self) -> Dict:
        """Share of set bits per grid (reads the bits back: a host synchronisation; for reports)."""
        return {key: float(unpack_bits(g["bits"], g["cells"]).float().mean()) for key, g in self.grids.items()}
