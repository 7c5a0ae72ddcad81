"""A numpy restatement of the band contract (``pr_band_plan`` / ``pr_band_fill``, include/playrender.h), written from the header's
words and not from the kernels: skeleton indices, cells, mixed and active cells, the band list in its fixed order, the fill and the
``exact`` bytes.  Not a test: the CPU tests check its properties, the GPU tests compare the library against it with ``torch.equal``."""
import numpy as np

DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]       # the mesher's seven edge directions


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def skeleton_indices(n, stride):
    """0, r, 2r, ... below n, plus n - 1 if it is not among them."""
    idx = list(range(0, n, stride))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return np.array(idx, dtype=np.int64)


def skeleton_mask(shape, stride):
    """bool (nx, ny, nz): all three indices are skeleton indices."""
    on = []
    for n in shape:
        m = np.zeros(n, dtype=bool)
        m[skeleton_indices(n, stride)] = True
        on.append(m)
    return on[0][:, None, None] & on[1][None, :, None] & on[2][None, None, :]


def cell_ranges(n, stride):
    """Per point index the lowest and the highest cell that contains it: cell c is the closed interval [idx[c], idx[c + 1]]."""
    idx = skeleton_indices(n, stride)
    lo, hi = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i in range(n):
        holds = [c for c in range(len(idx) - 1) if idx[c] <= i <= idx[c + 1]]
        lo[i], hi[i] = holds[0], holds[-1]
    return lo, hi, idx


def plan(sigma, level, stride, guard):
    """``sigma (G, nx, ny, nz)``: only its skeleton entries are read.  Returns a dict: ``mixed`` / ``active (G, cx, cy, cz)`` uint8,
    ``band (G, nx, ny, nz)`` bool, ``point_offsets (G + 1)`` int32, ``point_index (rows)`` int32 (by group, ascending),
    ``counts (G, 4)`` int32, ``source (nx, ny, nz)`` int64: the flat index of the lower corner of the lowest-indexed cell of a point."""
    sigma = np.asarray(sigma, dtype=np.float32)
    G, shape = sigma.shape[0], sigma.shape[1:]
    assert sigma.ndim == 4 and min(shape) >= 2 and 2 <= stride <= 64 and 0 <= guard <= 8
    ranges = [cell_ranges(n, stride) for n in shape]
    idx = [r[2] for r in ranges]
    cells = tuple(len(i) - 1 for i in idx)
    with np.errstate(invalid="ignore"):
        inside = sigma[np.ix_(np.arange(G), idx[0], idx[1], idx[2])] > np.float32(level)        # at the skeleton points; NaN: False
    some = np.zeros((G,) + cells, dtype=bool)
    every = np.ones((G,) + cells, dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                corner = inside[:, dx:dx + cells[0], dy:dy + cells[1], dz:dz + cells[2]]
                some |= corner
                every &= corner
    mixed = some & ~every
    g = guard
    padded = np.zeros((G, cells[0] + 2 * g, cells[1] + 2 * g, cells[2] + 2 * g), dtype=bool)
    padded[:, g:g + cells[0], g:g + cells[1], g:g + cells[2]] = mixed
    active = np.zeros_like(mixed)
    for dx in range(2 * g + 1):
        for dy in range(2 * g + 1):
            for dz in range(2 * g + 1):
                active |= padded[:, dx:dx + cells[0], dy:dy + cells[1], dz:dz + cells[2]]
    touched = np.zeros((G,) + shape, dtype=bool)
    for cx in (ranges[0][0], ranges[0][1]):
        for cy in (ranges[1][0], ranges[1][1]):
            for cz in (ranges[2][0], ranges[2][1]):
                touched |= active[np.ix_(np.arange(G), cx, cy, cz)]
    band = touched & ~skeleton_mask(shape, stride)[None]
    index = [np.nonzero(band[gr].reshape(-1))[0] for gr in range(G)]
    source = ((idx[0][ranges[0][0]][:, None, None] * shape[1] + idx[1][ranges[1][0]][None, :, None]) * shape[2]
              + idx[2][ranges[2][0]][None, None, :])
    counts = np.stack([np.full(G, int(np.prod(cells))), mixed.reshape(G, -1).sum(1), active.reshape(G, -1).sum(1),
                       band.reshape(G, -1).sum(1)], axis=1).astype(np.int32)
    return {"mixed": mixed.astype(np.uint8), "active": active.astype(np.uint8), "band": band, "cells": cells,
            "point_offsets": np.concatenate([[0], np.cumsum([len(i) for i in index])]).astype(np.int32),
            "point_index": np.concatenate(index).astype(np.int32), "counts": counts, "source": source}


def positions(p, axes):
    """``(rows, 3)`` fp32: the coordinates of the listed points, read from the axes."""
    shape = p["band"].shape[1:]
    i, j, k = np.unravel_index(p["point_index"].astype(np.int64), shape)
    return np.stack([np.asarray(axes[0], dtype=np.float32)[i], np.asarray(axes[1], dtype=np.float32)[j],
                     np.asarray(axes[2], dtype=np.float32)[k]], axis=1).reshape(-1, 3)


def fill(sigma, p, values, stride):
    """The lattice after ``pr_band_fill`` as int32 bit patterns, and ``exact`` uint8: ``values`` at the band points, a bitwise copy of
    the source skeleton entry at every other non-skeleton point, skeleton entries as they were."""
    out = bits(sigma).copy()
    G, shape = out.shape[0], out.shape[1:]
    skeleton = skeleton_mask(shape, stride)
    values = bits(values).reshape(-1)
    exact = np.zeros(out.shape, dtype=np.uint8)
    for g in range(G):
        flat = out[g].reshape(-1)
        copied = flat[p["source"].reshape(-1)]
        rest = ~(skeleton.reshape(-1) | p["band"][g].reshape(-1))
        flat[rest] = copied[rest]
        rows = slice(p["point_offsets"][g], p["point_offsets"][g + 1])
        flat[p["point_index"][rows]] = values[rows]
        exact[g] = (skeleton | p["band"][g]).astype(np.uint8)
    return out, exact


def refine(dense, level, stride, guard):
    """The band lattice of a field that is known everywhere: the plan from ``dense``'s skeleton entries, ``dense``'s own values at the
    band points, the fill elsewhere.  Returns ``(lattice fp32, exact uint8, plan)``."""
    dense = np.asarray(dense, dtype=np.float32)
    p = plan(dense, level, stride, guard)
    G = dense.shape[0]
    values = np.concatenate([bits(dense[g]).reshape(-1)[p["point_index"][p["point_offsets"][g]:p["point_offsets"][g + 1]]] for g in range(G)])
    out, exact = fill(dense, p, values.view(np.float32), stride)
    return out.view(np.float32), exact, p


def crossing_ends(field, level):
    """bool (nx, ny, nz): the point is an end of a crossing edge of the mesher (one of the seven directions, exactly one end inside)."""
    with np.errstate(invalid="ignore"):
        inside = np.asarray(field, dtype=np.float32) > np.float32(level)
    n = inside.shape
    ends = np.zeros(n, dtype=bool)
    for d in DIRECTIONS:
        a = inside[:n[0] - d[0], :n[1] - d[1], :n[2] - d[2]]
        b = inside[d[0]:, d[1]:, d[2]:]
        cross = a != b
        ends[:n[0] - d[0], :n[1] - d[1], :n[2] - d[2]] |= cross
        ends[d[0]:, d[1]:, d[2]:] |= cross
    return ends


def gradient_stencil(points):
    """bool: ``points`` and their neighbours at plus and minus one along every axis - what the normals of vertices there read."""
    out = points.copy()
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        out[tuple(lo)] |= points[tuple(hi)]
        out[tuple(hi)] |= points[tuple(lo)]
    return out
