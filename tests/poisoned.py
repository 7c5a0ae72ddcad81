"""Poisoned device allocations for the tests that call the C ABI directly (tests/test_adam_gpu.py, tests/test_scene_gpu.py): every array
lives in an allocation of its own that is filled with a NaN bit pattern, with guard words on both sides, so that a write outside the
array - or into an input - is seen after the call instead of landing in a neighbour."""
import numpy as np
import torch

F = np.float32
POISON = 0x7FC0DEAD                # a NaN as fp32
GUARD = 8                          # 4-byte words in front of and behind every array that must stay poisoned (plus up to 4 of padding)
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


class Placed:
    """``values`` (fp32; or, with ``dtype``, int32 / uint8) inside a poisoned allocation, ``shift`` words past a 16-byte boundary."""

    def __init__(self, values, shift=0, dtype=F):
        self.dtype = np.dtype(dtype)
        values = np.ascontiguousarray(values, dtype=self.dtype).reshape(-1)
        size = self.dtype.itemsize
        self.n, self.first = values.size, (GUARD + shift) * 4 // size
        words = (self.n * size + 3) // 4
        self.buffer = torch.full((words + 2 * GUARD + 4,), POISON, dtype=torch.int32, device="cuda")
        assert self.buffer.data_ptr() % 16 == 0
        self.view = self.buffer.view(_TORCH[self.dtype])[self.first:self.first + self.n]
        if self.n:
            self.view.copy_(torch.from_numpy(values))
        self.sent = values.copy()
        self.pointer = self.buffer.data_ptr() + size * self.first
        # the claim of the case, checked where the pointer is made
        assert self.pointer % 16 == 4 * shift and (self.n == 0 or self.view.data_ptr() == self.pointer)

    @classmethod
    def poisoned(cls, n, dtype=F, shift=0):
        """An output of ``n`` elements that holds the poison pattern itself: what the call does not write stays recognisable."""
        size = np.dtype(dtype).itemsize
        pattern = np.tile(np.frombuffer(np.int32(POISON).tobytes(), np.uint8), (n * size + 3) // 4)[:n * size]
        return cls(pattern.view(dtype), shift, dtype)

    def read(self, what):
        """The values after a call; the guards must be what they were."""
        raw = self.buffer.cpu().numpy().view(np.uint8)
        size = self.dtype.itemsize
        begin, end = self.first * size, (self.first + self.n) * size
        poison = np.frombuffer(np.int32(POISON).tobytes(), np.uint8)
        outside = np.concatenate([raw[:begin] != poison[np.arange(begin) % 4], raw[end:] != poison[np.arange(end, raw.size) % 4]])
        assert outside.size >= 2 * GUARD * 4 and not outside.any(), \
            f"{what}: guard bytes written at {np.flatnonzero(outside)[:8]} (of {begin} in front, {outside.size - begin} behind)"
        return raw[begin:end].copy().view(self.dtype)

    def unchanged(self, what):
        assert np.array_equal(self.read(what).view(np.uint8), self.sent.view(np.uint8)), f"{what} was written"
