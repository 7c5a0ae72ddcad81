"""Retention of chosen objects' per-sample state across evaluation frames (``pr_render_forward_retained``).

The play loop renders one frame after another from a camera that usually stands still; the static objects hold most of the in-box
samples and do not change.  With ``composer.retained = composer.retain_objects()`` the sample depths, densities, compact rows and
displacement magnitudes of those objects stay in a device cache between calls, next to a copy of everything they are a function
of.  The device compares that copy with each call's inputs bitwise and reuses an object's arrays only when nothing moved; only
compositing runs again.  Results are bit for bit those of a render without retention.

>>> composer.retained = composer.retain_objects()        # the static objects; any object may be named
>>> frame = composer(*inputs, False)                     # populates the cache
>>> frame = composer(*inputs_with_moved_players, False)  # static objects: no placement, no resampling, no MLP
>>> composer.retained.last_reused                        # (K,) int32 on the device: 1 = reused by the last call
"""
from __future__ import annotations

import ctypes as C
import itertools
import warnings
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib

_SERIAL = itertools.count(1)


class Retained:
    """The caches of one set of retained objects.  One cache per call signature (frames, rays, levels, precision, deferral, gate,
    pose flag, occupancy identity, device), allocated at the first call with that signature, reset once and kept until ``clear()``;
    a recorded frame holds their pointers.  MEMORY: every signature keeps its cache alive - a precision switch or a new
    ``Occupancy`` object adds another one (the headline frame's is 16.9 GiB at fp32, 24.4 GiB at f16x3): call
    ``clear()`` when a signature is not coming back.  ``host_key`` is the epoch of what the device cannot see, the weight values: it
    advances whenever a call finds that the packed weights of the retained objects' models were made from other parameter versions
    than at the previous call that used this object - also when the change happened while it was detached from the composer."""

    #: cells a grid on a retained object may have: the cache keeps a copy of its bits (64^3; RETAIN_OCC_WORDS x 32 in pr_common.h)
    MAX_OCCUPANCY_CELLS = 8192 * 32

    def __init__(self, composer, objects: Sequence[int]):
        helper = composer.object_id_helper
        ids = sorted({int(k) for k in objects})
        if not ids:
            raise ValueError("retain_objects needs at least one object")
        for k in ids:
            if not 0 <= k < helper.objects_count:
                raise ValueError(f"retain_objects: object {k} out of range 0..{helper.objects_count - 1}")
        self.objects: Tuple[int, ...] = tuple(ids)
        self.serial = next(_SERIAL)          # identity in the signatures of recorded frames
        self.host_key = 0
        self.last_reused: Optional[torch.Tensor] = None
        self._caches: Dict[tuple, torch.Tensor] = {}
        self._flags: Dict[tuple, torch.Tensor] = {}     # one (K,) flag tensor per cache: stable for a recording, no allocation per frame
        self._weights_key = None
        self._warned_split = False

    @property
    def mask(self) -> int:
        return sum(1 << k for k in self.objects)

    @property
    def bytes(self) -> int:
        """Total size of the caches held."""
        return sum(t.numel() for t in self._caches.values())

    def signature(self):
        return (self.serial,)

    def clear(self) -> None:
        """Drops the caches; the next call allocates anew.  Recorded frames keep the memory they wrote to alive and are re-recorded
        (the serial moves)."""
        self._caches.clear()
        self._flags.clear()
        self.serial = next(_SERIAL)
        self.last_reused = None

    def invalidate(self) -> None:
        """Marks every cache invalid (one small kernel each, stream-ordered): the next call renders every object."""
        lib = _lib.load()
        for cache in self._caches.values():
            with torch.cuda.device(cache.device):
                _lib.check(lib.pr_retained_reset(cache.data_ptr(), cache.numel(), torch.cuda.current_stream(cache.device).cuda_stream),
                           "pr_retained_reset")

    def weights_seen(self, key) -> None:
        """Called by the composer on every call that uses this object, with what the packed weights of the retained objects' models
        were made from (``ObjectComposer._retained_weights_key``): another key than last time = other weight values."""
        if key != self._weights_key:
            self._weights_key = key
            self.host_key += 1

    def check_occupancy(self, occupancy) -> None:
        """A grid on a retained object must fit the cache's copy of its bits."""
        for (k, level), g in occupancy.grids.items():
            cells = int(g["cells"][0]) * int(g["cells"][1]) * int(g["cells"][2])
            if k in self.objects and cells > self.MAX_OCCUPANCY_CELLS:
                raise ValueError(f"object {k} is retained: its {level} occupancy grid has {cells} cells, more than the "
                                 f"{self.MAX_OCCUPANCY_CELLS} (64^3) the retained cache keeps a copy of")

    def warn_split(self) -> None:
        if not self._warned_split:
            self._warned_split = True
            warnings.warn("ObjectComposer.retained: this call is split along the rays to fit the workspace budget and renders without "
                          "retention", UserWarning, stacklevel=4)

    def call_struct(self, lib, call, objs, K: int, key: tuple, device, stream: int) -> "_lib.Retained":
        """``pr_retained_t`` of a call: its cache (made and reset at the first call with this signature) and a fresh flag tensor."""
        if self.objects[-1] >= K:
            raise ValueError(f"the retained objects {self.objects} do not fit a call with {K} objects")
        size = C.c_size_t()
        _lib.check(lib.pr_retained_size(C.byref(call), objs, self.mask, C.byref(size)), "pr_retained_size")
        key = (str(device),) + tuple(key)
        cache = self._caches.get(key)
        if cache is None or cache.numel() != size.value:
            cache = None
            self._caches.pop(key, None)
            cache = torch.empty(size.value, dtype=torch.uint8, device=device)
            _lib.check(lib.pr_retained_reset(cache.data_ptr(), cache.numel(), stream), "pr_retained_reset")
            self._caches[key] = cache
            self._flags[key] = torch.empty((K,), dtype=torch.int32, device=device)       # (every element is written by every call)
        self.last_reused = self._flags[key]
        r = _lib.Retained()
        r.object_mask = self.mask
        r.host_key = self.host_key
        r.cache = cache.data_ptr()
        r.cache_bytes = cache.numel()
        r.reused = self.last_reused.data_ptr()
        return r
